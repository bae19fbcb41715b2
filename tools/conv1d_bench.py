"""Time of asr_conv1d_fwd (bias + ReLU fused) at three shapes:
    ds2   T 1000, B 64,  80 -> 256, k 11, stride 2, padding 5/5
    mid   T  500, B 64, 256 -> 256, k 11, stride 1, padding 5/5
    dw    T  500, B 64, depthwise C = 256, k 33, padding 16/16
against two yardsticks timed in the same process (neither is the code under
test):
  - asr_linear_fwd (bias + ReLU) on a pre-built im2col matrix [T_out*B][k*c_in]:
    the same contraction with contiguous A, under ASR_DENSE_F32 and, for
    information, under split-bf16 (dense shapes only; building and re-reading
    the im2col matrix, which a caller without the layer also pays, is NOT in
    that time);
  - torch.nn.functional.conv1d (+ bias, relu) in fp32 on the device, on x in
    torch's own [B][C][T] layout.
HIP events around each call, warm-up runs, then interleaved rounds (every
variant once per round); median and min of the rounds.  One JSON line per
variant and shape, with the fp32 MFMA floor of the dense shapes:
2 M K N / (256 FLOP/clk/CU x CUs filled x clock).
    python tools/conv1d_bench.py [--rounds 11] [--warmup 2] [--shapes ds2,mid,dw]
"""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tests"))
from conftest import asr  # noqa: E402
import torch  # noqa: E402

SHAPES = {   # T, B, c_in, c_out, k, s, d, pl, pr, groups
    "ds2": (1000, 64, 80, 256, 11, 2, 1, 5, 5, 1),
    "mid": (500, 64, 256, 256, 11, 1, 1, 5, 5, 1),
    "dw": (500, 64, 256, 256, 33, 1, 1, 16, 16, 256),
}
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--shapes", default="ds2,mid,dw")
a = ap.parse_args()
if a.rounds < 10:
    sys.exit("--rounds: at least 10 timed runs")
dev = torch.device("cuda")
torch.manual_seed(0)
L = asr.lib()
st = torch.cuda.Stream()
props = torch.cuda.get_device_properties(0)
CUS, GHZ = props.multi_processor_count, 2.4   # the MI355X's peak engine clock


def uni(shape, s):
    return (torch.rand(shape, device=dev) * 2 - 1) * s


variants = {}   # name -> (call, record)
keep = []
for name in a.shapes.split(","):
    T, B, ci, co, k, s, d, pl, pr, g = SHAPES[name]
    desc = asr.conv1d_desc(ci, co, k, s, d, pl, pr, g, "relu")
    T_out = asr.conv1d_out_frames(desc, T)
    M, K = T_out * B, k * (ci // g)
    x = uni((T * B, ci), 1.0)
    W = uni((K, co), K ** -0.5)
    b = uni((co,), 0.1)
    out = torch.empty((M, co), device=dev)
    keep.append((desc, x, W, b, out))
    rec = {"shape": name, "T": T, "B": B, "c_in": ci, "c_out": co, "k": k, "stride": s, "groups": g, "M": M, "K": K}
    if g == 1:
        # workgroups of 128 x 64 outputs; the floor counts the CUs the launch can fill
        wgs = -(-M // 128) * -(-co // 64)
        rec["mfma_floor_ms"] = round(2.0 * M * K * co / (256.0 * min(wgs, CUS) * GHZ * 1e9) * 1e3, 4)

    def conv(desc=desc, x=x, W=W, b=b, out=out, T=T, B=B, ci=ci, co=co):
        asr.check(L.asr_conv1d_fwd(ctypes.byref(desc), x.data_ptr(), ci, None, W.data_ptr(), b.data_ptr(),
                                   out.data_ptr(), co, None, T, B, st.cuda_stream), "asr_conv1d_fwd")

    variants[f"{name}/conv1d"] = (conv, {**rec, "kernel": "asr_conv1d_fwd"})

    if g == 1:
        col = uni((M, K), 1.0)           # the im2col matrix, pre-built (its content does not matter to the time)
        y = torch.empty((M, co), device=dev)
        keep.append((col, y))

        def gemm(arith, col=col, W=W, b=b, y=y, M=M, K=K, co=co):
            asr.set_dense_arith(arith)
            asr.check(L.asr_linear_fwd(col.data_ptr(), W.data_ptr(), b.data_ptr(), y.data_ptr(), M, K, co,
                                       asr.EPI_BIAS_RELU, st.cuda_stream), "asr_linear_fwd")

        variants[f"{name}/im2col_gemm_f32"] = (lambda gemm=gemm: gemm(asr.DENSE_F32),
                                               {**rec, "kernel": "asr_linear_fwd(im2col) ASR_DENSE_F32"})
        variants[f"{name}/im2col_gemm_bf16x3"] = (lambda gemm=gemm: gemm(asr.DENSE_SPLIT_BF16),
                                                  {**rec, "kernel": "asr_linear_fwd(im2col) split-bf16"})

    xt = uni((B, ci, T), 1.0)
    wt = uni((co, ci // g, k), K ** -0.5)
    keep.append((xt, wt))

    assert pl == pr

    def tconv(xt=xt, wt=wt, b=b, s=s, d=d, pl=pl, g=g):
        with torch.cuda.stream(st), torch.no_grad():
            torch.relu_(torch.nn.functional.conv1d(xt, wt, b, stride=s, padding=pl, dilation=d, groups=g))

    variants[f"{name}/torch_conv1d"] = (tconv, {**rec, "kernel": "torch.nn.functional.conv1d + relu (fp32)"})

before = asr.get_dense_arith()
try:
    for _ in range(a.warmup):
        for call, _r in variants.values():
            call()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, (call, _r) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            call()
            e1.record(st)
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
finally:
    asr.set_dense_arith(before)

for k, (_c, rec) in variants.items():
    med = statistics.median(ms[k])
    row = {**rec, "rounds": a.rounds, "ms": round(med, 4), "ms_min": round(min(ms[k]), 4)}
    yard = f"{rec['shape']}/im2col_gemm_f32"
    if yard in ms:
        row["ratio_to_im2col_gemm_f32"] = round(med / statistics.median(ms[yard]), 3)
    print(json.dumps(row), flush=True)
