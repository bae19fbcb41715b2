"""Time of asr_cross_attention_fwd and of a 6-layer TransformerDecoder.score()
at the shape of an attention-rescoring pass: E = 256, 4 heads, T = 250 encoder
frames, U = 32 tokens, n = 10 hypotheses per utterance, B = 64 and 256
utterances (N = n B hypotheses).

Kernel rows (HIP events around each call, warm-up, then interleaved rounds;
median, min and max of the rounds), no lengths so that all three do the same
work:
    xattn/grouped        asr_cross_attention_fwd on K / V [T*B, 2E], the map from utterance to hypotheses
    xattn/repeated       yardstick (a): asr_attention_fwd with the N hypotheses as the batch, on K / V
                         repeated n times [T*N, 2E] (what repeat_interleave makes; building it is not timed)
    xattn/torch_sdpa     yardstick (b): torch scaled_dot_product_attention, fp32, on the repeated memory
    xattn/grouped_ragged asr_cross_attention_fwd with ragged token and frame counts (no yardstick: a
                         self-attention call has one length per column for queries and keys alike)
Neither yardstick is the code under test.  Each row carries its query-tile fill
(live queries over 64 x the workgroups that do not exit at once) and the bytes
of K and V it reads from memory at least once.

Decoder rows (host clock around calls that end in a device synchronise):
    decoder/score        asr.TransformerDecoder.score(): host embedding and upload, per layer one K/V
                         projection of the B memories, causal self-attention, grouped cross-attention,
                         feed-forward; log-softmax; asr_token_score; N doubles back
    decoder/torch        the same torch.nn.TransformerDecoder in fp32 eager on
                         memory.repeat_interleave(n), log_softmax and a gather
with the bytes of the repeated K / V buffers the grouped path never builds.

Every buffer is built inside bench_shape() from the shape it is given; there are
no module-level sizes.  Without --child the tool runs one child process per B
under its own time limit and stops at the first that fails.
    python tools/cross_attention_bench.py [--B 64 256] [--rounds 11] [--warmup 2] [--layers 6]
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
    """A torch tensor's memory as the rows x cols matrix the mirror's calls take."""

    def __init__(self, t, rows, cols, offset=0):
        self.ptr, self.rows, self.cols, self._keep = t.data_ptr() + 4 * offset, rows, cols, t


def bench_shape(B, n, T, U, E, heads, F, V, layers, rounds, warmup, decoder):
    from conftest import asr
    import torch
    dev = torch.device("cuda")
    torch.manual_seed(0)
    rng = np.random.default_rng(B)
    st = torch.cuda.Stream()
    N, D = n * B, E // heads
    shape = {"B": B, "n": n, "N": N, "T": T, "U": U, "E": E, "heads": heads}

    def uni(*s):
        return torch.rand(s, device=dev) * 2 - 1

    q, out = uni(U * N, E), torch.empty(U * N, E, device=dev)
    kv = uni(T * B, 2 * E)
    kv_rep = kv.view(T, B, 2 * E).repeat_interleave(n, dim=1).contiguous().view(T * N, 2 * E)
    off = asr.device_lengths(np.arange(B + 1) * n)
    qlen = rng.integers(U // 2, U + 1, N)
    klen = rng.integers(T // 2, T + 1, B)
    d_qlen, d_klen = asr.device_lengths(qlen), asr.device_lengths(klen)
    xd, ad = asr.xattn_desc(heads, D), asr.attn_desc(heads, D)
    qv, ov = View(q, U * N, E), View(out, U * N, E)
    kg, vg = View(kv, T * B, 2 * E), View(kv, T * B, 2 * E, E)
    kr, vr = View(kv_rep, T * N, 2 * E), View(kv_rep, T * N, 2 * E, E)
    qt = q.view(U, N, heads, D).permute(1, 2, 0, 3).contiguous()
    kt = kv_rep.view(T, N, 2, heads, D)[:, :, 0].permute(1, 2, 0, 3).contiguous()
    vt = kv_rep.view(T, N, 2, heads, D)[:, :, 1].permute(1, 2, 0, 3).contiguous()

    def sdpa():
        with torch.cuda.stream(st), torch.no_grad():
            torch.nn.functional.scaled_dot_product_attention(qt, kt, vt)

    tiles = -(-U * n // 64) * B
    kv_bytes = 4 * T * 2 * E
    variants = {
        "xattn/grouped": (lambda: asr.cross_attention_fwd(qv, kg, vg, ov, U, N, T, B, xd, off, n, ldk=2 * E, ldv=2 * E,
                                                          stream=st.cuda_stream),
                          {"tile_fill": round(U * N / (64 * tiles), 3), "kv_bytes": kv_bytes * B}),
        "xattn/repeated": (lambda: asr.attention_fwd(qv, kr, vr, ov, U, T, N, ad, ldk=2 * E, ldv=2 * E,
                                                     stream=st.cuda_stream),
                           {"tile_fill": round(U / 64, 3), "kv_bytes": kv_bytes * N}),
        "xattn/torch_sdpa": (sdpa, {"kv_bytes": kv_bytes * N}),
        "xattn/grouped_ragged": (lambda: asr.cross_attention_fwd(qv, kg, vg, ov, U, N, T, B, xd, off, n, d_qlen, d_klen,
                                                                 ldk=2 * E, ldv=2 * E, stream=st.cuda_stream),
                                 {"tile_fill": round(float(qlen.sum()) / (64 * tiles), 3),
                                  "kv_bytes": int(4 * 2 * E * klen.sum())}),
    }
    for _ in range(warmup):
        for call, _r in variants.values():
            call()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (call, _r) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            call()
            e1.record(st)
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, (_c, rec) in variants.items():
        row = {"variant": k, **shape, **rec, "rounds": rounds, "ms": round(med[k], 4), "ms_min": round(min(ms[k]), 4),
               "ms_max": round(max(ms[k]), 4)}
        if k == "xattn/grouped":
            row["ratio_to_repeated"] = round(med[k] / med["xattn/repeated"], 3)
            row["ratio_to_torch_sdpa"] = round(med[k] / med["xattn/torch_sdpa"], 3)
        print(json.dumps(row), flush=True)
    del kv_rep, kt, vt, qt
    if not decoder:
        return

    # ---- the whole decoder
    emb = torch.nn.Embedding(V, E)
    layer = torch.nn.TransformerDecoderLayer(E, heads, F, dropout=0.0, norm_first=True)
    tdec = torch.nn.TransformerDecoder(layer, layers, norm=torch.nn.LayerNorm(E))
    lin = torch.nn.Linear(E, V)
    dec = asr.TransformerDecoder.from_torch(emb, tdec, lin)
    emb, tdec, lin = emb.to(dev).eval(), tdec.to(dev).eval(), lin.to(dev).eval()
    hyps = [rng.integers(0, V - 1, int(m)).tolist() for m in rng.integers(U // 2, U, N)]
    utt = np.repeat(np.arange(B), n).tolist()
    memory = uni(T * B, E)
    enc_len = klen.tolist()
    mem_v = View(memory, T * B, E)
    tin, tgt, ln = dec.teacher_forcing(hyps, V - 1, V - 1)
    Uq = tin.shape[0]
    pe = torch.from_numpy(asr.sinusoidal_positional_encoding(Uq, E)).float().to(dev)
    tin_t, tgt_t = torch.from_numpy(tin).long().to(dev), torch.from_numpy(tgt).long().to(dev)
    causal = torch.triu(torch.ones(Uq, Uq, dtype=torch.bool, device=dev), diagonal=1)
    tpad = torch.from_numpy(np.arange(Uq)[None, :] >= ln[:, None]).to(dev)
    mpad = torch.from_numpy(np.arange(T)[None, :] >= np.repeat(klen, n)[:, None]).to(dev)

    def ours():
        return dec.score(hyps, utt, mem_v, T, B, enc_len)

    def theirs():
        with torch.no_grad():
            x = emb(tin_t) * (E ** 0.5) + pe[:, None, :]
            mem = memory.view(T, B, E).repeat_interleave(n, dim=1)
            y = tdec(x, mem, tgt_mask=causal, tgt_key_padding_mask=tpad, memory_key_padding_mask=mpad)
            lp = torch.log_softmax(lin(y), dim=-1).gather(2, tgt_t[:, :, None])[:, :, 0]
            return (lp.double() * (~tpad.T)).sum(0).cpu().numpy()

    a, b = ours(), theirs()
    worst = float(np.max(np.abs(a - b) / (1 + np.abs(b))))
    wall = {"decoder/score": [], "decoder/torch": []}
    for _ in range(warmup):
        ours(), theirs()
    for _ in range(rounds):
        for k, call in (("decoder/score", ours), ("decoder/torch", theirs)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    wmed = {k: statistics.median(v) for k, v in wall.items()}
    rep_bytes = layers * 4 * T * N * 2 * E
    for k in wall:
        row = {"variant": k, **shape, "F": F, "V": V, "layers": layers, "U_max": int(Uq), "rounds": rounds,
               "ms": round(wmed[k], 3), "ms_min": round(min(wall[k]), 3), "ms_max": round(max(wall[k]), 3)}
        if k == "decoder/score":
            row.update(ratio_to_torch=round(wmed[k] / wmed["decoder/torch"], 3),
                       max_score_diff_to_torch_rel=worst, repeated_kv_bytes_avoided=rep_bytes,
                       kv_bytes_built=layers * 4 * T * B * 2 * E,
                       kv_projection_rows={"grouped": T * B, "repeated": T * N})
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--T", type=int, default=250)
    ap.add_argument("--U", type=int, default=32)
    ap.add_argument("--E", type=int, default=256)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--F", type=int, default=2048)
    ap.add_argument("--V", type=int, default=5000)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-decoder", action="store_true")
    ap.add_argument("--limit", type=int, default=240, help="seconds each child process may take")
    ap.add_argument("--child", action="store_true", help="run the one shape given by --B in this process")
    a = ap.parse_args()
    if a.rounds < 10:
        sys.exit("--rounds: at least 10 timed runs")
    if a.child:
        bench_shape(a.B[0], a.n, a.T, a.U, a.E, a.heads, a.F, a.V, a.layers, a.rounds, a.warmup, not a.no_decoder)
        return
    for B in a.B:
        cmd = [sys.executable, __file__, "--child", "--B", str(B)]
        for k in ("n", "T", "U", "E", "heads", "F", "V", "layers", "rounds", "warmup"):
            cmd += [f"--{k}", str(getattr(a, k))]
        if a.no_decoder:
            cmd.append("--no-decoder")
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"B = {B}: no result within {a.limit} s; nothing more is started")
        if rc != 0:
            sys.exit(f"B = {B}: the child ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
