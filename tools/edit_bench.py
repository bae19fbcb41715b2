"""Time of asr_nbest_mbr and asr_edit_distance (csrc/edit.hip) against their
one-thread host twins on the same arrays.

Two calls: the MBR call on the final beam shape of a C4 batch — 2048 groups of
50 hypotheses, lengths 40 to 60 over V = 29 labels, three quarters of a group's
hypotheses being one- or two-edit variants of each other, the rest random — and
a WER call of 2048 pairs of 100 labels (the hypothesis a corrupted reference).
Device: HIP events on an otherwise idle stream around each call, warm-up calls,
then the median of --rounds calls.  Host: wall clock around the host twin, the
median of --host-rounds calls.  One JSON line per call; "speedup" is host ms
over device ms; the integers must equal the host's, the risks agree to 1e-12.
    python tools/edit_bench.py [--groups 2048] [--hyps 50] [--rounds 11] [--warmup 2] [--host-rounds 1]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tests"))
from conftest import asr  # noqa: E402
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--groups", type=int, default=2048)
ap.add_argument("--hyps", type=int, default=50)
ap.add_argument("--pairs", type=int, default=2048)
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--host-rounds", type=int, default=1)
a = ap.parse_args()
if a.rounds < 10:
    sys.exit("--rounds: at least 10 timed runs")
V = 29


def edit(rng, seq, n_edits):
    seq = list(seq)
    for _ in range(n_edits):
        op, at = rng.integers(0, 3), rng.integers(0, len(seq))
        if op == 0:
            seq[at] = int(rng.integers(1, V))
        elif op == 1:
            seq.insert(at, int(rng.integers(1, V)))
        else:
            del seq[at]
    return seq


def make_beam(rng, G, n):
    """[G * n][60] tokens, lengths in 40 .. 60, group starts."""
    tok = np.zeros((G * n, 60), np.int32)
    lens = np.zeros(G * n, np.int32)
    for g in range(G):
        hyps = [rng.integers(1, V, rng.integers(42, 59)).tolist()]
        while len(hyps) < n:
            if len(hyps) % 4 == 3:
                hyps.append(rng.integers(1, V, rng.integers(40, 61)).tolist())
            else:   # one or two edits away from the first, so at most four from each other
                hyps.append(edit(rng, hyps[0], int(rng.integers(1, 3))))
        for k, h in enumerate(hyps):
            tok[g * n + k, :len(h)] = h
            lens[g * n + k] = len(h)
    return tok, lens, (np.arange(G + 1) * n).astype(np.int32)


def timed(run, st):
    for _ in range(a.warmup):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        run()
        e1.record(st)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def host_timed(run):
    out = []
    for _ in range(a.host_rounds):
        h0 = time.perf_counter()
        run()
        out.append((time.perf_counter() - h0) * 1e3)
    return statistics.median(out)


dev = torch.device("cuda")
st = torch.cuda.Stream()
rng = np.random.default_rng(0)

# ---- the MBR call
G, n = a.groups, a.hyps
tok, lens, gs = make_beam(rng, G, n)
N, max_len = G * n, 60
w = rng.uniform(-12.0, 0.0, N)
d_tok, d_len, d_gs, d_w = (torch.from_numpy(x).to(dev) for x in (tok, lens, gs, w))
d_dist = torch.empty((N, n), dtype=torch.int32, device=dev)
d_risk = torch.empty(N, dtype=torch.float64, device=dev)
d_best = torch.empty(G, dtype=torch.int32, device=dev)


def run_mbr():
    asr.check(asr.lib().asr_nbest_mbr(d_tok.data_ptr(), 60, d_len.data_ptr(), N, max_len, d_gs.data_ptr(), G, n,
                                      d_w.data_ptr(), d_dist.data_ptr(), n, d_risk.data_ptr(), d_best.data_ptr(),
                                      st.cuda_stream), "asr_nbest_mbr")


ms = timed(run_mbr, st)
h_dist, h_risk, h_best = np.zeros((N, n), np.int32), np.zeros(N, np.float64), np.zeros(G, np.int32)
hmed = host_timed(lambda: asr.check(asr.lib().asr_nbest_mbr_host(
    tok.ctypes.data, 60, lens.ctypes.data, N, max_len, gs.ctypes.data, G, n, w.ctypes.data, h_dist.ctypes.data, n,
    h_risk.ctypes.data, h_best.ctypes.data), "asr_nbest_mbr_host"))
same = bool((d_dist.cpu().numpy() == h_dist).all())
risk_ok = bool((np.abs(d_risk.cpu().numpy() - h_risk) <= 1e-12 * np.maximum(1.0, h_risk)).all())
best_same = int((d_best.cpu().numpy() == h_best).sum())
med = statistics.median(ms)
pairs = G * n * (n - 1) // 2
cells = int(sum(int(lens[g * n + k]) * int(lens[g * n + j]) for g in range(min(G, 64)) for k in range(n)
                for j in range(k)) * (G / min(G, 64)))
print(json.dumps({"call": "asr_nbest_mbr", "groups": G, "hyps": n, "pairs": pairs, "cells_estimate": cells,
                  "device_ms": round(med, 4), "device_ms_min": round(min(ms), 4), "device_ms_max": round(max(ms), 4),
                  "host_ms": round(hmed, 1), "speedup": round(hmed / med, 1),
                  "device_pairs_per_s": round(pairs / med * 1e3), "distances_equal_to_host": same,
                  "risks_within_1e-12": risk_ok, "best_equal": best_same, "mean_distance": round(float(h_dist.mean()), 2)}),
      flush=True)
if not (same and risk_ok):
    sys.exit("device and host differ")

# ---- the WER call
P, L = a.pairs, 100
ref = rng.integers(1, V, (P, L)).astype(np.int32)
hyp = np.zeros((P, L + 20), np.int32)
hl = np.zeros(P, np.int32)
for p in range(P):
    h = edit(rng, ref[p].tolist(), int(rng.integers(0, 16)))
    hyp[p, :len(h)] = h
    hl[p] = len(h)
mh = int(hl.max())
d_ref, d_hyp, d_hl = (torch.from_numpy(x).to(dev) for x in (ref, hyp, hl))
d_d = torch.empty(P, dtype=torch.int32, device=dev)
d_o = torch.empty((P, 4), dtype=torch.int32, device=dev)


def run_wer():
    asr.check(asr.lib().asr_edit_distance(d_ref.data_ptr(), L, None, P, L, d_hyp.data_ptr(), L + 20, d_hl.data_ptr(), P,
                                          mh, None, None, P, d_d.data_ptr(), d_o.data_ptr(), st.cuda_stream),
              "asr_edit_distance")


ms = timed(run_wer, st)
h_d, h_o = np.zeros(P, np.int32), np.zeros((P, 4), np.int32)
hmed = host_timed(lambda: asr.check(asr.lib().asr_edit_distance_host(
    ref.ctypes.data, L, None, P, L, hyp.ctypes.data, L + 20, hl.ctypes.data, P, mh, None, None, P, h_d.ctypes.data,
    h_o.ctypes.data), "asr_edit_distance_host"))
same = bool((d_d.cpu().numpy() == h_d).all() and (d_o.cpu().numpy() == h_o).all())
med = statistics.median(ms)
errors, ref_tokens = int(h_o[:, 1:].sum()), int(h_o[:, :3].sum())
print(json.dumps({"call": "asr_edit_distance", "pairs": P, "ref_len": L, "max_hyp_len": mh,
                  "device_ms": round(med, 4), "device_ms_min": round(min(ms), 4), "device_ms_max": round(max(ms), 4),
                  "host_ms": round(hmed, 2), "speedup": round(hmed / med, 1),
                  "device_pairs_per_s": round(P / med * 1e3), "equal_to_host": same,
                  "wer": round(errors / ref_tokens, 4)}), flush=True)
if not same:
    sys.exit("device and host differ")
