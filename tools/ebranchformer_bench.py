"""Times of the E-Branchformer additions at a medium encoder after 4x
subsampling: E = 256, cgMLP units 2048 (C = 1024), 4 heads, k = 31, T = 200,
B = 64 and 256.
  (a) asr_linear_fwd [T*B, E] -> [T*B, units] with EPI_BIAS_GELU against
      EPI_BIAS_RELU and EPI_BIAS_SILU, same buffers, in both arithmetics;
  (b) asr_csgu_fwd (statistics pre-pass + normalise -> depthwise -> bias ->
      product) against torch's F.layer_norm + F.conv1d(groups = C) + mul in fp32
      on the same GPU, u in torch's own [B][T][2C] layout; with the bytes the
      fused op must move (3 C floats per frame) over its time;
  (c) asr_merge_dwconv_fwd against torch's cat + F.conv1d(groups = 2E) + add;
  (d) one EBranchformerLayer.forward against the stand-in block of
      tests/ebranchformer_reference.py in torch fp32 eager, and the layer's
      per-launch breakdown: every library call of one forward between HIP events.
No torch figure is the code under test.  HIP events around `inner` back-to-back
calls, warm-up runs, then interleaved rounds (every variant once per round);
median and min of the rounds, per call.  One JSON line per variant.
    python tools/ebranchformer_bench.py [--rounds 11] [--warmup 2] [--batches 64,256]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tests"))
from conftest import asr  # noqa: E402
import ebranchformer_reference as eb  # noqa: E402
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--batches", default="64,256")
a = ap.parse_args()
if a.rounds < 10:
    sys.exit("--rounds: at least 10 timed runs")
E, UNITS, HEADS, K, T = 256, 2048, 4, 31, 200
C = UNITS // 2
dev = torch.device("cuda")
torch.manual_seed(0)
L = asr.lib()
st = torch.cuda.Stream()
S = st.cuda_stream
TRACED = ["asr_layernorm_fwd", "asr_linear_fwd", "asr_matadd", "asr_attention_fwd", "asr_csgu_fwd",
          "asr_merge_dwconv_fwd", "asr_mask_rows"]
f = torch.nn.functional


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
    x, W, b, y = Buf(uni((M, E), 1.0)), Buf(uni((E, UNITS), E ** -0.5)), Buf(uni((UNITS, 1), 0.1)), Buf(
        torch.empty((M, UNITS), device=dev))
    for arith, aname in ((asr.DENSE_SPLIT_BF16, "split_bf16"), (asr.DENSE_F32, "f32")):
        for epi in ("EPI_BIAS_RELU", "EPI_BIAS_SILU", "EPI_BIAS_GELU"):
            def lin(arith=arith, epi=getattr(asr, epi), x=x, W=W, b=b, y=y):
                asr.set_dense_arith(arith)
                asr.linear_fwd(x, W, b, y, epi, S)
            variants[f"a/B{B}/{aname}/{epi}"] = (lin, 20, {"part": "a", "B": B, "M": M, "K": E, "N": UNITS,
                                                           "arith": aname, "kernel": f"asr_linear_fwd {epi}"})
    # (b) the gating unit against torch's three passes
    u, w, cb, out = Buf(uni((M, 2 * C), 1.0)), Buf(uni((K, C), K ** -0.5)), Buf(uni((C, 1), 0.1)), Buf(
        torch.empty((M, C), device=dev))
    gm, bt, stats = Buf(uni((C, 1), 0.5) + 1), Buf(uni((C, 1), 0.1)), Buf(torch.empty((M, 3), device=dev))
    desc = asr.csgu_desc(C, K)

    def csgu(u=u, w=w, cb=cb, out=out, gm=gm, bt=bt, stats=stats, desc=desc, B=B):
        asr.csgu_fwd(u, w, cb, out, T, B, desc, gm, bt, stats, stream=S)
    variants[f"b/B{B}/csgu"] = (csgu, 20, {"part": "b", "B": B, "C": C, "k": K, "kernel": "asr_csgu_fwd",
                                           "min_gbytes": round(3.0 * C * 4 * M / 1e9, 4)})
    ut, wt = uni((B, T, 2 * C), 1.0), uni((C, 1, K), K ** -0.5)

    def tcsgu(ut=ut, wt=wt, gm=gm, bt=bt, cb=cb):
        with torch.cuda.stream(st), torch.no_grad():
            r, g = ut.chunk(2, dim=-1)
            g = f.layer_norm(g, (C,), gm.t[:, 0], bt.t[:, 0])
            r * f.conv1d(g.transpose(1, 2), wt, cb.t[:, 0], padding=K // 2, groups=C).transpose(1, 2)
    variants[f"b/B{B}/torch_layernorm_conv1d_mul"] = (tcsgu, 20, {
        "part": "b", "B": B, "C": C, "k": K, "kernel": "torch F.layer_norm + F.conv1d(groups=C) + mul (fp32)"})
    # (c) the merge against torch's cat + conv + add
    x1, x2, wm, bm = Buf(uni((M, E), 1.0)), Buf(uni((M, E), 1.0)), Buf(uni((K, 2 * E), K ** -0.5)), Buf(
        uni((2 * E, 1), 0.1))
    om, mdesc = Buf(torch.empty((M, 2 * E), device=dev)), asr.merge_dwconv_desc(E, K)

    def merge(x1=x1, x2=x2, wm=wm, bm=bm, om=om, mdesc=mdesc, B=B):
        asr.merge_dwconv_fwd(x1, x2, wm, bm, om, T, B, mdesc, stream=S)
    variants[f"c/B{B}/merge_dwconv"] = (merge, 20, {"part": "c", "B": B, "C": E, "k": K,
                                                    "kernel": "asr_merge_dwconv_fwd",
                                                    "min_gbytes": round(4.0 * E * 4 * M / 1e9, 4)})
    t1, t2, wmt = uni((B, T, E), 1.0), uni((B, T, E), 1.0), uni((2 * E, 1, K), K ** -0.5)

    def tmerge(t1=t1, t2=t2, wmt=wmt, bm=bm):
        with torch.cuda.stream(st), torch.no_grad():
            cat = torch.cat([t1, t2], dim=-1)
            cat + f.conv1d(cat.transpose(1, 2), wmt, bm.t[:, 0], padding=K // 2, groups=2 * E).transpose(1, 2)
    variants[f"c/B{B}/torch_cat_conv1d_add"] = (tmerge, 20, {"part": "c", "B": B, "C": E, "k": K,
                                                             "kernel": "torch cat + F.conv1d(groups=2E) + add (fp32)"})
    # (d) the whole block
    block = eb.make_block((T, B, E, HEADS, UNITS, K, K))
    layer = asr.EBranchformerLayer.from_espnet(block)
    xl = Buf(uni((M, E), 1.0))
    tblock = block.to(dev)
    xt = xl.t.reshape(T, B, E).transpose(0, 1)
    layers[B] = (layer, xl)

    def fwd(layer=layer, xl=xl, B=B):
        asr.set_dense_arith(asr.DENSE_SPLIT_BF16)
        layer.forward(xl, T, B, stream=S)

    def tfwd(tblock=tblock, xt=xt):
        with torch.cuda.stream(st), torch.no_grad():
            tblock(xt)
    variants[f"d/B{B}/EBranchformerLayer"] = (fwd, 5, {"part": "d", "B": B,
                                                       "kernel": "EBranchformerLayer.forward (split-bf16 GEMMs)"})
    variants[f"d/B{B}/torch_block"] = (tfwd, 5, {"part": "d", "B": B, "kernel": "torch fp32 eager block"})
    keep.append((x, W, b, y, u, w, cb, out, gm, bt, stats, ut, wt, x1, x2, wm, bm, om, t1, t2, wmt, xl, tblock))


def breakdown(layer, xl, B, rounds):
    """Every library call of one forward between two events: [(name, median ms)]."""
    real = {n: getattr(L, n) for n in TRACED}
    log = []

    def wrap(name):
        def g(*args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            rc = real[name](*args)
            e1.record(st)
            log.append((name, e0, e1))
            return rc
        return g
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
    yard = {"a": f"a/B{rec['B']}/{rec.get('arith')}/EPI_BIAS_RELU", "b": f"b/B{rec['B']}/csgu",
            "c": f"c/B{rec['B']}/merge_dwconv", "d": f"d/B{rec['B']}/EBranchformerLayer"}[rec["part"]]
    if yard != k:
        row["ratio_to_" + yard.split("/")[-1]] = round(med / statistics.median(ms[yard]), 3)
    print(json.dumps(row), flush=True)
for B, rows in steps.items():
    print(json.dumps({"variant": f"d/B{B}/launches", "part": "d", "B": B, "rounds": a.rounds,
                      "sum_ms": round(sum(m for _n, m in rows), 4),
                      "launches": [[n.replace("asr_", ""), round(m, 4)] for n, m in rows]}), flush=True)
