"""Times of the Conformer additions at a medium Conformer after 4x subsampling:
E = 256, F = 1024, 4 heads, k = 31, T = 200, B = 64 and 256.
  (a) asr_linear_fwd [T*B, E] -> [T*B, F] with EPI_BIAS_SILU against EPI_BIAS_RELU
      and EPI_BIAS, same buffers, under split-bf16 and under ASR_DENSE_F32;
  (b) asr_glu_dwconv_fwd (GLU -> depthwise k = 31 -> bias -> SiLU, one launch)
      against torch's F.glu + F.conv1d(groups = C) + F.silu in fp32 on the same
      GPU, on u in torch's own [B][2C][T] layout; with the bytes the fused op
      must move (3 E floats per frame) over its time;
  (c) one ConformerLayer.forward against the same block (the torch module of
      tests/conformer_reference.py) in torch fp32 eager, and the layer's
      per-launch breakdown: every library call of one forward between HIP events.
Neither torch figure is the code under test.  HIP events around `inner`
back-to-back calls, warm-up runs, then interleaved rounds (every variant once
per round); median and min of the rounds, per call.  One JSON line per variant.
    python tools/conformer_bench.py [--rounds 11] [--warmup 2] [--batches 64,256]
"""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tests"))
from conftest import asr  # noqa: E402
import conformer_reference as cf  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--batches", default="64,256")
a = ap.parse_args()
if a.rounds < 10:
    sys.exit("--rounds: at least 10 timed runs")
E, F, HEADS, K, T = 256, 1024, 4, 31, 200
dev = torch.device("cuda")
torch.manual_seed(0)
L = asr.lib()
st = torch.cuda.Stream()
S = st.cuda_stream
TRACED = ["asr_layernorm_fwd", "asr_linear_fwd", "asr_matadd", "asr_attention_fwd", "asr_glu_dwconv_fwd",
          "asr_mask_rows"]


def uni(shape, s):
    return (torch.rand(shape, device=dev) * 2 - 1) * s


class Buf:
    """A torch tensor seen as a device matrix of the library."""

    def __init__(self, t):
        self.t, self.ptr, self.rows, self.cols = t, t.data_ptr(), t.shape[0], t.shape[1]


variants = {}   # name -> (call, inner, record)
keep = []
layers = {}
for B in (int(v) for v in a.batches.split(",")):
    M = T * B
    # (a) the first feed-forward linear with each epilogue
    x, W, b, y = Buf(uni((M, E), 1.0)), Buf(uni((E, F), E ** -0.5)), Buf(uni((F, 1), 0.1)), Buf(torch.empty((M, F), device=dev))
    for arith, aname in ((asr.DENSE_SPLIT_BF16, "split_bf16"), (asr.DENSE_F32, "f32")):
        for epi in ("EPI_BIAS", "EPI_BIAS_RELU", "EPI_BIAS_SILU"):
            def lin(arith=arith, epi=getattr(asr, epi), x=x, W=W, b=b, y=y):
                asr.set_dense_arith(arith)
                asr.linear_fwd(x, W, b, y, epi, S)
            variants[f"a/B{B}/{aname}/{epi}"] = (lin, 20, {"part": "a", "B": B, "M": M, "K": E, "N": F, "arith": aname,
                                                           "kernel": f"asr_linear_fwd {epi}"})
    # (b) the fused GLU-conv against torch's three passes
    u, w, cb, out = Buf(uni((M, 2 * E), 1.0)), Buf(uni((K, E), K ** -0.5)), Buf(uni((E, 1), 0.1)), Buf(torch.empty((M, E), device=dev))
    desc = asr.glu_dwconv_desc(E, K, act="silu")
    gbytes = 3.0 * E * 4 * M / 1e9

    def glu(u=u, w=w, cb=cb, out=out, desc=desc, B=B):
        asr.glu_dwconv_fwd(u, w, cb, out, T, B, desc, stream=S)
    variants[f"b/B{B}/glu_dwconv"] = (glu, 20, {"part": "b", "B": B, "C": E, "k": K, "kernel": "asr_glu_dwconv_fwd",
                                                "min_gbytes": round(gbytes, 4)})
    ut, wt, bt = uni((B, 2 * E, T), 1.0), uni((E, 1, K), K ** -0.5), uni((E,), 0.1)

    def tglu(ut=ut, wt=wt, bt=bt):
        with torch.cuda.stream(st), torch.no_grad():
            f = torch.nn.functional
            f.silu(f.conv1d(f.glu(ut, dim=1), wt, bt, padding=K // 2, groups=E), inplace=True)
    variants[f"b/B{B}/torch_glu_conv1d_silu"] = (tglu, 20, {"part": "b", "B": B, "C": E, "k": K,
                                                            "kernel": "torch F.glu + F.conv1d(groups=C) + F.silu (fp32)"})
    # (c) the whole block
    block = cf.make_block((T, B, E, HEADS, F, K))
    layer = asr.ConformerLayer.from_torch(**block.explicit_parts())
    xl = Buf(uni((M, E), 1.0))
    tblock = block.to(dev)
    xt = xl.t.reshape(T, B, E)
    layers[B] = (layer, xl)

    def fwd(layer=layer, xl=xl, B=B):
        asr.set_dense_arith(asr.DENSE_SPLIT_BF16)
        layer.forward(xl, T, B, stream=S)

    def tfwd(tblock=tblock, xt=xt):
        with torch.cuda.stream(st), torch.no_grad():
            tblock(xt)
    variants[f"c/B{B}/ConformerLayer"] = (fwd, 5, {"part": "c", "B": B, "kernel": "ConformerLayer.forward (split-bf16 GEMMs)"})
    variants[f"c/B{B}/torch_block"] = (tfwd, 5, {"part": "c", "B": B, "kernel": "torch fp32 eager block"})
    keep.append((x, W, b, y, u, w, cb, out, ut, wt, bt, xl, tblock))


def breakdown(layer, xl, B, rounds):
    """Every library call of one forward between two events: [(name, median ms)]."""
    real = {n: getattr(L, n) for n in TRACED}
    log = []

    def wrap(name):
        def f(*args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            rc = real[name](*args)
            e1.record(st)
            log.append((name, e0, e1))
            return rc
        return f
    per = []
    try:
        for n in TRACED:
            setattr(L, n, wrap(n))
        for _ in range(rounds):
            log.clear()
            layer.forward(xl, T, B, stream=S)
            st.synchronize()
            per.append([(n, e0.elapsed_time(e1)) for n, e0, e1 in log])
    finally:
        for n in TRACED:
            setattr(L, n, real[n])
    assert all([n for n, _ in p] == [n for n, _ in per[0]] for p in per)
    return [(per[0][i][0], statistics.median(p[i][1] for p in per)) for i in range(len(per[0]))]


before = asr.get_dense_arith()
try:
    for _ in range(a.warmup):
        for call, _i, _r in variants.values():
            call()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, (call, inner, _r) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _j in range(inner):
                call()
            e1.record(st)
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / inner)
    asr.set_dense_arith(asr.DENSE_SPLIT_BF16)
    steps = {B: breakdown(layer, xl, B, a.rounds) for B, (layer, xl) in layers.items()}
finally:
    asr.set_dense_arith(before)

for k, (_c, inner, rec) in variants.items():
    med = statistics.median(ms[k])
    row = {"variant": k, **rec, "rounds": a.rounds, "calls_per_round": inner, "ms": round(med, 4),
           "ms_min": round(min(ms[k]), 4)}
    if "min_gbytes" in rec:
        row["gbytes_per_s"] = round(rec["min_gbytes"] / (med * 1e-3), 1)
    yard = {"a": f"a/B{rec['B']}/{rec.get('arith')}/EPI_BIAS_RELU", "b": f"b/B{rec['B']}/glu_dwconv",
            "c": f"c/B{rec['B']}/ConformerLayer"}[rec["part"]]
    if yard != k:
        row["ratio_to_" + yard.split("/")[-1]] = round(med / statistics.median(ms[yard]), 3)
    print(json.dumps(row), flush=True)
for B, rows in steps.items():
    print(json.dumps({"variant": f"c/B{B}/launches", "part": "c", "B": B, "rounds": a.rounds,
                      "sum_ms": round(sum(m for _n, m in rows), 4),
                      "launches": [[n.replace("asr_", ""), round(m, 4)] for n, m in rows]}), flush=True)
