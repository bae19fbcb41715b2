"""Time of the CTC prefix scorer at the shape of a joint CTC / attention decode:
K = 10 slots per utterance, V = 5000, T = 250 frames, B = 64 and 256.

Kernel rows (HIP events around each call, warm-up, then interleaved rounds;
median, min and max of the rounds):
    score/kernel     asr_ctc_prefix_score, the fused joint row from att [N, V]
    score/torch      yardstick: the same deltas stated in torch on the device, a logsumexp over t of
                     phi[:, :, None] + x in fp32, chunked over V (the c == last column and eos are left out:
                     it does less than the kernel)
    score/read_x     yardstick: one read of the emission matrix (a torch sum over [T*B, V]), whose bytes
                     over its time is the HBM rate the kernel's emission traffic is compared with
    advance          asr_ctc_prefix_advance with random parents and tokens
Search rows (host clock around calls that end in a device synchronise), the
6-layer decoder of tools/attn_decode_bench.py, the eos bias lowered so that no
hypothesis ends, 32 steps:
    search/attention beam_search without ctc
    search/joint     beam_search with ctc and ctc_weight 0.3 on the same memory
Every buffer is built inside bench_shape() from the shape it is given.  Without
--child the tool runs one child process per B under its own time limit and
stops at the first that fails.
    python tools/ctc_prefix_bench.py [--B 64 256] [--rounds 11] [--warmup 2] [--search-B 64]
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
import types
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tests"))


def view(t, rows, cols):
    return types.SimpleNamespace(ptr=t.data_ptr(), rows=rows, cols=cols, nbytes=4 * rows * cols, keep=t)


def bench_shape(B, K, T, V, L, E, heads, F, layers, rounds, warmup, search):
    from conftest import asr
    import torch
    dev = torch.device("cuda")
    torch.manual_seed(0)
    rng = np.random.default_rng(B)
    st = torch.cuda.Stream()
    N = B * K
    shape = {"B": B, "K": K, "N": N, "T": T, "V": V}
    x = torch.log_softmax(torch.rand(T * B, V, device=dev) * 6 - 3, dim=-1)
    att = torch.log_softmax(torch.rand(N, V, device=dev) * 6 - 3, dim=-1)
    lens = rng.integers(T // 2, T + 1, B)
    lens[0] = T
    sc = asr.CTCPrefixScorer(view(x, T * B, V), T, B, lens.tolist(), K, 0, V - 1)
    live = types.SimpleNamespace(cur=0, scores=[asr._upload(np.zeros(N))], fin=[asr._upload(np.zeros(N, np.int32))])
    sc.begin(st.cuda_stream)
    for _ in range(3):                               # three real tokens per slot: no state is trivial
        live.parent = asr._upload(((np.arange(N) // K) * K + rng.integers(0, K, N)).astype(np.int32))
        live.token = asr._upload(rng.integers(1, V - 1, N).astype(np.int32))
        sc.advance(live, st.cuda_stream)
    out = torch.empty(N, V, device=dev)
    # the torch statement reads the same state: phi = (rn + rb) - psi as fp32 [N][T]
    c = sc.cur
    rn, rb = (torch.from_numpy(asr._download(d, (T, N), np.float64, st.cuda_stream)).to(dev) for d in (sc.rn[c], sc.rb[c]))
    psi = torch.from_numpy(asr._download(sc.psi[c], N, np.float64, st.cuda_stream)).to(dev)
    phi = torch.nan_to_num((torch.logaddexp(rn, rb) - psi[None, :]).float(), nan=-1e30, neginf=-1e30)   # [T][N]
    phi = phi.t().reshape(B, K, T).contiguous()
    xt = x.view(T, B, V)
    mask = (torch.arange(T, device=dev)[None, :] >= torch.from_numpy(lens).to(dev)[:, None])             # [B][T]
    vchunk = max(1, min(V, (1 << 28) // (N * T)))    # at most 2^28 fp32 terms alive at once

    def torch_scores():
        with torch.cuda.stream(st):
            for v0 in range(0, V, vchunk):
                xs = xt[1:, :, v0:v0 + vchunk].permute(1, 0, 2)                                    # [B][T-1][v]
                xs = xs.masked_fill(mask[:, 1:, None], -1e30)
                out.view(B, K, V)[:, :, v0:v0 + vchunk] = torch.logsumexp(phi[:, :, :T - 1, None] + xs[:, None], dim=2)

    def read_x():
        with torch.cuda.stream(st):
            x.sum()

    variants = {
        "score/kernel": lambda: sc.score(live, view(att, N, V), view(out, N, V), 0.3, 0.0, stream=st.cuda_stream),
        "score/torch": torch_scores,
        "score/read_x": read_x,
        "advance": lambda: sc.advance(live, st.cuda_stream),
    }
    for _ in range(warmup):
        for call in variants.values():
            call()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, call in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            call()
            e1.record(st)
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in ms.items()}
    frames = int(lens.sum())
    for k in variants:
        row = {"variant": k, **shape, "rounds": rounds, "ms": round(med[k], 4), "ms_min": round(min(ms[k]), 4),
               "ms_max": round(max(ms[k]), 4)}
        if k == "score/kernel":
            row.update(ratio_to_torch=round(med[k] / med["score/torch"], 4),
                       ratio_to_read_x=round(med[k] / med["score/read_x"], 3),
                       emission_GB=round(4e-9 * frames * V, 3), terms_G=round(1e-9 * frames * V * K, 3),
                       exp_per_ns=round(1e-6 * frames * V * K * 9 / 8 / med[k], 1))
        if k == "score/read_x":
            row["GB_per_s"] = round(4e-6 * T * B * V / med[k], 1)
        print(json.dumps(row), flush=True)
    if not search:
        return

    emb = torch.nn.Embedding(V, E)
    layer = torch.nn.TransformerDecoderLayer(E, heads, F, dropout=0.0, norm_first=True)
    tdec = torch.nn.TransformerDecoder(layer, layers, norm=torch.nn.LayerNorm(E))
    lin = torch.nn.Linear(E, V)
    with torch.no_grad():
        lin.bias[V - 1] = -30.0                      # no hypothesis ends: every search runs its L steps
    dec = asr.TransformerDecoder.from_torch(emb, tdec, lin)
    memory = torch.rand(T * B, E, device=dev) * 2 - 1
    args = (view(memory, T * B, E), T, B, lens.tolist())
    kw = dict(beam=K, max_len=L, sos=V - 1, eos=V - 1)
    calls = {"search/attention": lambda: dec.beam_search(*args, **kw),
             "search/joint": lambda: dec.beam_search(*args, **kw, ctc=view(x, T * B, V), ctc_weight=0.3, blank=0)}
    wall = {k: [] for k in calls}
    for _ in range(warmup):
        for call in calls.values():
            call()
    for _ in range(rounds):
        for k, call in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    wmed = {k: statistics.median(v) for k, v in wall.items()}
    for k in wall:
        row = {"variant": k, **shape, "E": E, "layers": layers, "steps": L, "rounds": rounds, "ms": round(wmed[k], 3),
               "ms_min": round(min(wall[k]), 3), "ms_max": round(max(wall[k]), 3)}
        if k == "search/joint":
            row["ratio_to_attention"] = round(wmed[k] / wmed["search/attention"], 3)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--search-B", type=int, nargs="*", default=[64], help="the B that also run the two searches")
    for k, v in (("K", 10), ("T", 250), ("V", 5000), ("L", 32), ("E", 256), ("heads", 4), ("F", 2048), ("layers", 6),
                 ("rounds", 11), ("warmup", 2)):
        ap.add_argument(f"--{k}", type=int, default=v)
    ap.add_argument("--limit", type=int, default=300, help="seconds each child process may take")
    ap.add_argument("--child", action="store_true", help="run the one shape given by --B in this process")
    ap.add_argument("--search", action="store_true")
    a = ap.parse_args()
    if a.rounds < 10:
        sys.exit("--rounds: at least 10 timed runs")
    if a.child:
        bench_shape(a.B[0], a.K, a.T, a.V, a.L, a.E, a.heads, a.F, a.layers, a.rounds, a.warmup, a.search)
        return
    for B in a.B:
        cmd = [sys.executable, __file__, "--child", "--B", str(B)] + (["--search"] if B in a.search_B else [])
        for k in ("K", "T", "V", "L", "E", "heads", "F", "layers", "rounds", "warmup"):
            cmd += [f"--{k}", str(getattr(a, k))]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"B = {B}: no result within {a.limit} s; nothing more is started")
        if rc != 0:
            sys.exit(f"B = {B}: the child ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
