"""Time of asr_conv2d_fwd and the Conv2dSubsampling front end at one shape
given by arguments (default: F 80 mel bins, C 256 channels, B 64, T 1000):
    sub4/layer1   Conv2d 1 -> C, 3x3, stride 2x2, unpadded, ReLU   (a log-mel matrix in)
    sub4/layer2   Conv2d C -> C, 3x3, stride 2x2, unpadded, ReLU   (the implicit GEMM, K = 9 C)
    sub4/whole    asr.Conv2dSubsampling.forward: both layers, the Linear C F'' -> C, the row mask
    dw/chain      NeMo dw_striding after its first layer: depthwise 3x3 stride 2 padding 1, then the
                  1x1 pointwise C -> C with ReLU (two asr_conv2d_fwd calls in one timed window)
against yardsticks timed in the same process (none is the code under test):
  - torch.nn.functional.conv2d + relu in fp32, in torch's own [B][C][T][F] layout, for both layers;
  - for layer 2, asr_linear_fwd (bias + ReLU) under ASR_DENSE_F32 on a pre-built im2col matrix
    [T''*B*F''][9 C]: the same contraction with contiguous A; building and re-reading that matrix,
    which a caller without the layer also pays, is NOT in that time.
Every buffer is allocated inside main() from the (T, B, F, C) the calls are given, and no shape is
rebound between warm-up and timing.  HIP events around each call, warm-up runs, then interleaved
rounds (every variant once per round); median and min of the rounds.  One JSON line per variant, with
the fp32 MFMA floor of the dense layers, 2 M K N / (256 FLOP/clk/CU x 256 CUs x 2.4 GHz), and the
bytes each call must move over its time.
    python tools/conv2d_bench.py [--T 1000] [--B 64] [--F 80] [--C 256] [--rounds 11] [--warmup 2]
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


class View:
    """A torch tensor's memory as the rows x cols matrix the mirror's calls take."""

    def __init__(self, t, rows, cols):
        self.ptr, self.rows, self.cols, self._keep = t.data_ptr(), rows, cols, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--F", type=int, default=80)
    ap.add_argument("--C", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-yardsticks", action="store_true", help="skip torch and the im2col GEMM")
    a = ap.parse_args()
    if a.rounds < 10:
        sys.exit("--rounds: at least 10 timed runs")
    T, B, F, C = a.T, a.B, a.F, a.C
    dev = torch.device("cuda")
    torch.manual_seed(0)
    L = asr.lib()
    st = torch.cuda.Stream()
    FLOOR = 256.0 * 256 * 2.4e9          # fp32 MFMA FLOP/s of the whole chip at the peak engine clock

    def uni(shape, s):
        return (torch.rand(shape, device=dev) * 2 - 1) * s

    d1 = asr.conv2d_desc(1, C, F, 3, 3, 2, 2, act="relu")
    T1, F1 = asr.conv2d_out_frames(d1, T), asr.conv2d_out_feats(d1)
    d2 = asr.conv2d_desc(C, C, F1, 3, 3, 2, 2, act="relu")
    T2, F2 = asr.conv2d_out_frames(d2, T1), asr.conv2d_out_feats(d2)
    ddw = asr.conv2d_desc(C, C, F1, 3, 3, 2, 2, 1, 1, 1, 1, groups=C)
    Tw, Fw = asr.conv2d_out_frames(ddw, T1), asr.conv2d_out_feats(ddw)
    dpw = asr.conv2d_desc(C, C, Fw, 1, 1, act="relu")
    assert min(T1, T2, Tw, F1, F2, Fw) > 0, "the shape is too small for two stride-2 layers"
    M1, M2, K2 = T1 * B * F1, T2 * B * F2, 9 * C
    shape = {"T": T, "B": B, "F": F, "C": C}

    x = uni((T * B, F), 1.0)
    W1, b1 = uni((9, C), 1.0 / 3), uni((C,), 0.1)
    h1 = torch.empty((T1 * B, F1 * C), device=dev)            # layer 1's output, every later call's input
    W2, b2 = uni((K2, C), K2 ** -0.5), uni((C,), 0.1)
    h2 = torch.empty((T2 * B, F2 * C), device=dev)
    Wd, bd = uni((9, C), 1.0 / 3), uni((C,), 0.1)
    hd = torch.empty((Tw * B, Fw * C), device=dev)
    Wp, bp = uni((C, C), C ** -0.5), uni((C,), 0.1)
    hp = torch.empty((Tw * B, Fw * C), device=dev)

    def conv(desc, xin, ldx, W, b, out, ldo, t):
        asr.check(L.asr_conv2d_fwd(ctypes.byref(desc), xin.data_ptr(), ldx, None, W.data_ptr(), b.data_ptr(),
                                   out.data_ptr(), ldo, None, t, B, st.cuda_stream), "asr_conv2d_fwd")

    variants = {}
    variants["sub4/layer1"] = (
        lambda: conv(d1, x, F, W1, b1, h1, F1 * C, T),
        {"kernel": "asr_conv2d_fwd 1->C 3x3 s2 relu", "M": M1, "K": 9, "N": C,
         "mfma_floor_ms": round(2.0 * M1 * 12 * C / FLOOR * 1e3, 4),       # K = 3 taps x one group of 4
         "bytes": 4 * (T * B * F + M1 * C)})
    variants["sub4/layer2"] = (
        lambda: conv(d2, h1, F1 * C, W2, b2, h2, F2 * C, T1),
        {"kernel": "asr_conv2d_fwd C->C 3x3 s2 relu", "M": M2, "K": K2, "N": C,
         "mfma_floor_ms": round(2.0 * M2 * K2 * C / FLOOR * 1e3, 4), "bytes": 4 * (M1 * C + M2 * C + K2 * C)})

    seq = torch.nn.Sequential(torch.nn.Conv2d(1, C, 3, 2), torch.nn.ReLU(), torch.nn.Conv2d(C, C, 3, 2),
                              torch.nn.ReLU())
    sub = asr.Conv2dSubsampling.from_torch(seq, torch.nn.Linear(C * F2, C), F, scale=float(C) ** 0.5)
    xv, lens = View(x, T * B, F), asr.device_lengths([T] * B)
    variants["sub4/whole"] = (
        lambda: sub.forward(xv, T, B, lengths=lens, stream=st.cuda_stream),
        {"kernel": "asr.Conv2dSubsampling.forward (2 x asr_conv2d_fwd, asr_linear_fwd, asr_mask_rows)"})

    def dw_chain():
        conv(ddw, h1, F1 * C, Wd, bd, hd, Fw * C, T1)
        conv(dpw, hd, Fw * C, Wp, bp, hp, Fw * C, Tw)

    variants["dw/chain"] = (dw_chain, {"kernel": "asr_conv2d_fwd depthwise 3x3 s2 p1, then 1x1 C->C relu",
                                       "M": Tw * B * Fw, "bytes": 4 * (M1 * C + 3 * Tw * B * Fw * C)})

    if not a.no_yardsticks:
        xt1, wt1 = uni((B, 1, T, F), 1.0), uni((C, 1, 3, 3), 1.0 / 3)
        xt2, wt2 = uni((B, C, T1, F1), 1.0), uni((C, C, 3, 3), K2 ** -0.5)

        def tconv(xt, wt, b):
            with torch.cuda.stream(st), torch.no_grad():
                torch.relu_(torch.nn.functional.conv2d(xt, wt, b, stride=2))

        variants["sub4/layer1_torch"] = (lambda: tconv(xt1, wt1, b1), {"kernel": "torch conv2d + relu (fp32)"})
        variants["sub4/layer2_torch"] = (lambda: tconv(xt2, wt2, b2), {"kernel": "torch conv2d + relu (fp32)"})
        col = uni((M2, K2), 1.0)          # the im2col matrix, pre-built (its content does not matter to the time)
        y = torch.empty((M2, C), device=dev)

        def gemm():
            asr.set_dense_arith(asr.DENSE_F32)
            asr.check(L.asr_linear_fwd(col.data_ptr(), W2.data_ptr(), b2.data_ptr(), y.data_ptr(), M2, K2, C,
                                       asr.EPI_BIAS_RELU, st.cuda_stream), "asr_linear_fwd")
            asr.set_dense_arith(before)

        variants["sub4/layer2_im2col_gemm_f32"] = (gemm, {"kernel": "asr_linear_fwd(im2col) ASR_DENSE_F32",
                                                          "M": M2, "K": K2, "N": C})

    before = asr.get_dense_arith()
    try:
        conv(d1, x, F, W1, b1, h1, F1 * C, T)                 # h1 holds real activations for what reads it
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
        row = {"variant": k, **shape, **rec, "rounds": a.rounds, "ms": round(med, 4), "ms_min": round(min(ms[k]), 4),
               "ms_max": round(max(ms[k]), 4)}
        if "bytes" in rec:
            row["gb_per_s"] = round(rec["bytes"] / med / 1e6, 1)
        if k == "sub4/layer2" and "sub4/layer2_im2col_gemm_f32" in ms:
            row["ratio_to_im2col_gemm_f32"] = round(med / statistics.median(ms["sub4/layer2_im2col_gemm_f32"]), 3)
        for lay in ("layer1", "layer2"):
            if k == f"sub4/{lay}" and f"sub4/{lay}_torch" in ms:
                row["ratio_to_torch"] = round(med / statistics.median(ms[f"sub4/{lay}_torch"]), 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
