"""Time of the attention decoder's autoregressive step and of a whole beam
search at the shape of an `attention` decode: E = 256, 4 heads, T = 250 encoder
frames, K = 10 slots per utterance, B = 64 and 256 utterances (N = K B slots),
a self-attention cache of 32 keys, 32 steps.

Kernel rows (HIP events around each call, warm-up, then interleaved rounds;
median, min and max of the rounds):
    self/decode          asr_decode_attention_fwd over the cache [32 N, 3E] through a random ancestry table
    self/gather+attn     yardstick: the cache physically gathered through the same table (one torch index
                         gather into [32 N, 2E], timed) and asr_attention_fwd with Tq = 1, q_pos0 = 31
    cross/decode         asr_decode_attention_fwd with ldc = 0 over the memories' K / V [T B, 2E]
    cross/xattn_u1       yardstick: asr_cross_attention_fwd at U = 1 (a 64-query tile holds the utterance's K
                         queries: one wave of four works)
Search rows (host clock around calls that end in a device synchronise), a
6-layer decoder, V = 5000, the eos bias lowered so that no hypothesis ends:
    search/beam          asr.TransformerDecoder.beam_search, 32 steps on the K/V cache
    search/recompute     yardstick: the same search with log_probs() on the whole prefix at every step (what
                         the library could do before), the prune on the device by asr_attn_beam_step, the
                         tokens reordered on the host
    search/torch         yardstick: torch.nn.TransformerDecoder in fp32 eager on the whole prefix at every
                         step, memory.repeat_interleave(K), torch.topk over K V candidates
with the kernel launches per step of search/beam and the share of a step's wall
time its host code needs to issue them (step() returns before the device ends;
prune() waits for the live count).

Every buffer is built inside bench_shape() from the shape it is given; there are
no module-level sizes and nothing rebinds a shape between warm-up and timing.
Without --child the tool runs one child process per B under its own time limit
and stops at the first that fails.
    python tools/attn_decode_bench.py [--B 64 256] [--rounds 11] [--warmup 2] [--layers 6]
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tests"))


class View:
    """A torch tensor's memory as the rows x cols matrix (or int32 buffer) the mirror's calls take."""

    def __init__(self, t, rows, cols, offset=0):
        self.ptr, self.rows, self.cols, self._keep = t.data_ptr() + 4 * offset, rows, cols, t
        self.nbytes = 4 * rows * cols


def timed(variants, st, rounds, warmup, torch):
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
    return ms


def bench_shape(B, K, T, L, E, heads, F, V, layers, rounds, warmup, search):
    from conftest import asr
    import torch
    dev = torch.device("cuda")
    torch.manual_seed(0)
    rng = np.random.default_rng(B)
    st = torch.cuda.Stream()
    N, D = K * B, E // heads
    shape = {"B": B, "K": K, "N": N, "T": T, "cache": L, "E": E, "heads": heads}

    def uni(*s):
        return torch.rand(s, device=dev) * 2 - 1

    # ---- the two attentions of one step
    cache = uni(L * N, 3 * E)
    anc_h = ((np.arange(N) // K) * K + rng.integers(0, K, (L, N))).astype(np.int32)
    anc_h[L - 1] = np.arange(N)
    anc = torch.from_numpy(anc_h).to(dev)
    rows = (torch.arange(L, device=dev)[:, None] * N + anc.long()).reshape(-1)
    gathered = torch.empty(L * N, 2 * E, device=dev)
    out = torch.empty(N, E, device=dev)
    kv = uni(T * B, 2 * E)
    q = uni(N, E)
    cols = torch.from_numpy(np.repeat(np.arange(B), K).astype(np.int32)).to(dev)
    off = asr.device_lengths(np.arange(B + 1) * K)
    xd, ad = asr.xattn_desc(heads, D), asr.attn_desc(heads, D)
    ov, qv = View(out, N, E), View(q, N, E)
    q_last = View(cache, N, 3 * E, (L - 1) * N * 3 * E)
    ck, cv = View(cache, L * N, 3 * E, E), View(cache, L * N, 3 * E, 2 * E)
    gk, gv = View(gathered, L * N, 2 * E), View(gathered, L * N, 2 * E, E)
    mk, mv = View(kv, T * B, 2 * E), View(kv, T * B, 2 * E, E)
    anc_v, cols_v = View(anc, L, N), View(cols, 1, N)

    def gather_attn():
        with torch.cuda.stream(st):
            torch.index_select(cache[:, E:], 0, rows, out=gathered)
        asr.attention_fwd(q_last, gk, gv, ov, 1, L, N, ad, q_pos0=L - 1, ldq=3 * E, ldk=2 * E, ldv=2 * E,
                          stream=st.cuda_stream)

    variants = {
        "self/decode": lambda: asr.decode_attention_fwd(q_last, ck, cv, ov, N, L, N, xd, anc_v, ldc=N, ldq=3 * E,
                                                        ldk=3 * E, ldv=3 * E, stream=st.cuda_stream),
        "self/gather+attn": gather_attn,
        "cross/decode": lambda: asr.decode_attention_fwd(qv, mk, mv, ov, N, T, B, xd, cols_v, ldc=0, ldk=2 * E,
                                                         ldv=2 * E, stream=st.cuda_stream),
        "cross/xattn_u1": lambda: asr.cross_attention_fwd(qv, mk, mv, ov, 1, N, T, B, xd, off, K, ldk=2 * E,
                                                          ldv=2 * E, stream=st.cuda_stream),
    }
    ms = timed(variants, st, rounds, warmup, torch)
    med = {k: statistics.median(v) for k, v in ms.items()}
    yard = {"self/decode": "self/gather+attn", "cross/decode": "cross/xattn_u1"}
    for k in variants:
        row = {"variant": k, **shape, "rounds": rounds, "ms": round(med[k], 4), "ms_min": round(min(ms[k]), 4),
               "ms_max": round(max(ms[k]), 4)}
        if k in yard:
            row["ratio_to_yardstick"] = round(med[k] / med[yard[k]], 3)
        print(json.dumps(row), flush=True)
    del cache, gathered, kv
    if not search:
        return

    # ---- the whole search
    emb = torch.nn.Embedding(V, E)
    layer = torch.nn.TransformerDecoderLayer(E, heads, F, dropout=0.0, norm_first=True)
    tdec = torch.nn.TransformerDecoder(layer, layers, norm=torch.nn.LayerNorm(E))
    lin = torch.nn.Linear(E, V)
    with torch.no_grad():
        lin.bias[V - 1] = -30.0                    # no hypothesis ends: every search runs its L steps
    dec = asr.TransformerDecoder.from_torch(emb, tdec, lin)
    emb, tdec, lin = emb.to(dev).eval(), tdec.to(dev).eval(), lin.to(dev).eval()
    memory = uni(T * B, E)
    mem_v = View(memory, T * B, E)
    klen = rng.integers(T // 2, T + 1, B)
    enc_len = klen.tolist()
    utt = np.repeat(np.arange(B), K).tolist()
    sos = eos = V - 1
    pe = torch.from_numpy(asr.sinusoidal_positional_encoding(L, E)).float().to(dev)
    mpad = torch.from_numpy(np.arange(T)[None, :] >= np.repeat(klen, K)[:, None]).to(dev)

    def ours():
        return dec.beam_search(mem_v, T, B, enc_len, beam=K, max_len=L, sos=sos, eos=eos)

    def recompute():
        tin = np.full((1, N), sos, np.int32)
        scores = np.full(N, -np.inf)
        scores[::K] = 0.0
        so, fo = asr._upload(scores), asr._upload(np.zeros(N, np.int32))
        so2, fo2, par, tok, live = (asr.DeviceBytes(8 * N), asr.DeviceBytes(4 * N), asr.DeviceBytes(4 * N),
                                    asr.DeviceBytes(4 * N), asr.DeviceBytes(16))
        tabs = [asr._upload(np.zeros((L, N), np.int32)) for _ in range(4)]
        for s in range(L):
            logp, U, _ = dec.log_probs(tin, [s + 1] * N, utt, mem_v, T, B, enc_len)
            asr.attn_beam_step(asr.attn_beam_desc(B, K, V, L, s, eos), asr.RowView(logp, s * N, N), so, fo, tabs[0],
                               tabs[1], so2, fo2, par, tok, tabs[2], tabs[3], live)
            p, t = asr._download(par, N, np.int32), asr._download(tok, N, np.int32)
            tin = np.concatenate([tin[:, p], t[None, :]])
            so, so2, fo, fo2 = so2, so, fo2, fo
            tabs = [tabs[2], tabs[3], tabs[0], tabs[1]]
        return tin

    def theirs():
        with torch.no_grad():
            mem = memory.view(T, B, E).repeat_interleave(K, dim=1)
            tin = torch.full((1, N), sos, dtype=torch.long, device=dev)
            scores = torch.full((B, K), -float("inf"), device=dev)
            scores[:, 0] = 0.0
            base = (torch.arange(B, device=dev) * K)[:, None]
            for s in range(L):
                x = emb(tin) * (E ** 0.5) + pe[:s + 1, None, :]
                causal = torch.triu(torch.ones(s + 1, s + 1, dtype=torch.bool, device=dev), diagonal=1)
                y = tdec(x, mem, tgt_mask=causal, memory_key_padding_mask=mpad)[-1]
                lp = torch.log_softmax(lin(y), dim=-1).view(B, K, V)
                scores, idx = torch.topk((scores[:, :, None] + lp).view(B, K * V), K, dim=1)
                parent = (base + idx // V).reshape(-1)
                tin = torch.cat([tin[:, parent], (idx % V).reshape(1, -1)])
            return tin.cpu().numpy()

    calls = {"search/beam": ours, "search/recompute": recompute, "search/torch": theirs}
    first = ours()
    same = [[y for y, _ in u] for u in first] == [[col.tolist() for col in recompute()[1:, b * K:(b + 1) * K].T]
                                                  for b in range(B)]
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
    # the host's share of a step: the time step() needs to issue its launches over the step's wall time
    issue, total = 0.0, 0.0
    state = dec.begin(mem_v, T, B, enc_len, beam=K, max_len=L, sos=sos)
    for _ in range(L):
        t0 = time.perf_counter()
        logp = dec.step(state)
        t1 = time.perf_counter()
        dec.prune(state, logp, eos)
        issue, total = issue + (t1 - t0), total + (time.perf_counter() - t0)
    norm_first = 1
    per_layer = 3 + 3 * norm_first + 8              # LayerNorms, residual adds (pre-norm), 6 GEMMs, 2 attentions
    wmed = {k: statistics.median(v) for k, v in wall.items()}
    for k in wall:
        row = {"variant": k, **shape, "F": F, "V": V, "layers": layers, "steps": L, "rounds": rounds,
               "ms": round(wmed[k], 3), "ms_min": round(min(wall[k]), 3), "ms_max": round(max(wall[k]), 3)}
        if k == "search/beam":
            row.update(ratio_to_recompute=round(wmed[k] / wmed["search/recompute"], 3),
                       ratio_to_torch=round(wmed[k] / wmed["search/torch"], 3), ms_per_step=round(wmed[k] / L, 3),
                       launches_per_step=1 + layers * per_layer + 2 + 1, host_issue_share=round(issue / total, 3),
                       tokens_equal_recompute=bool(same))
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--T", type=int, default=250)
    ap.add_argument("--L", type=int, default=32, help="cache length and search steps")
    ap.add_argument("--E", type=int, default=256)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--F", type=int, default=2048)
    ap.add_argument("--V", type=int, default=5000)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-search", action="store_true")
    ap.add_argument("--limit", type=int, default=420, help="seconds each child process may take")
    ap.add_argument("--child", action="store_true", help="run the one shape given by --B in this process")
    a = ap.parse_args()
    if a.rounds < 10:
        sys.exit("--rounds: at least 10 timed runs")
    if a.child:
        bench_shape(a.B[0], a.K, a.T, a.L, a.E, a.heads, a.F, a.V, a.layers, a.rounds, a.warmup, not a.no_search)
        return
    for B in a.B:
        cmd = [sys.executable, __file__, "--child", "--B", str(B)]
        for k in ("K", "T", "L", "E", "heads", "F", "V", "layers", "rounds", "warmup"):
            cmd += [f"--{k}", str(getattr(a, k))]
        if a.no_search:
            cmd.append("--no-search")
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"B = {B}: no result within {a.limit} s; nothing more is started")
        if rc != 0:
            sys.exit(f"B = {B}: the child ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
