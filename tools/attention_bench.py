"""Time of asr_attention_fwd at four shapes (T, B, E, heads), lengths ragged
between T/2 and T:
    s144   250, 64, 144, 4     full mask
    s256   250, 64, 256, 4     full mask
    s512   500, 64, 512, 8     full mask
    chunk  500, 64, 256, 4     chunk 16, left 4, right 0
against torch.nn.functional.scaled_dot_product_attention in fp32 on the same
device and inputs (a boolean mask [B][1][T][T] of the window and the lengths;
building the mask is NOT in torch's time), timed in the same process.
HIP events around --iters back-to-back calls, warm-up runs, then interleaved
rounds (every variant once per round); median and min of the rounds' per-call
times.  One JSON line per
variant and shape.  FLOP: 4 D per visible (query, key) pair and head, pairs
counted from the lengths and the window (a full mask over full lengths would be
4 Tq Tk E B); utilisation = FLOP / time over the fp32-MFMA peak
256 FLOP/clk/CU x CUs x clock.  The largest difference between the two outputs
on valid rows is printed with each shape (a check, not a benchmark).
    python tools/attention_bench.py [--rounds 11] [--warmup 2] [--iters 20] [--shapes s144,s256,s512,chunk]
"""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tests"))
from conftest import asr  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = {   # T, B, E, heads, chunk, left, right
    "s144": (250, 64, 144, 4, 1, -1, -1),
    "s256": (250, 64, 256, 4, 1, -1, -1),
    "s512": (500, 64, 512, 8, 1, -1, -1),
    "chunk": (500, 64, 256, 4, 16, 4, 0),
}
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--iters", type=int, default=20, help="calls per timed window")
ap.add_argument("--shapes", default="s144,s256,s512,chunk")
a = ap.parse_args()
if a.rounds < 10:
    sys.exit("--rounds: at least 10 timed runs")
dev = torch.device("cuda")
torch.manual_seed(0)
L = asr.lib()
st = torch.cuda.Stream()
props = torch.cuda.get_device_properties(0)
CUS, GHZ = props.multi_processor_count, 2.4   # the MI355X's peak engine clock
PEAK = 256.0 * CUS * GHZ * 1e9                # fp32 MFMA FLOP/s

variants, keep, checks = {}, [], {}
for name in a.shapes.split(","):
    T, B, E, H, chunk, left, right = SHAPES[name]
    D = E // H
    lens = np.random.default_rng(T + E).integers(T // 2, T + 1, B)
    lens[0] = T
    pos = np.arange(T)
    win = np.ones((T, T), bool)
    if left >= 0:
        win &= pos[None, :] // chunk >= pos[:, None] // chunk - left
    if right >= 0:
        win &= pos[None, :] // chunk <= pos[:, None] // chunk + right
    valid = pos[None, :] < lens[:, None]                                       # [B][T]
    allowed = win[None] & valid[:, None, :] & valid[:, :, None]                # [B][Tq][Tk]
    pairs = int(allowed.sum())
    flop = 4.0 * D * H * pairs
    qkv = (torch.rand((T * B, 3 * E), device=dev) * 2 - 1)
    out = torch.zeros((T * B, E), device=dev)
    dl = torch.from_numpy(lens.astype(np.int32)).to(dev)
    desc = asr.attn_desc(H, D, 0.0, chunk, left, right)
    # torch: [B][H][T][D] views of the same values, contiguous; padded queries keep themselves visible (no NaN rows)
    tq, tk, tv = (qkv[:, i * E:(i + 1) * E].reshape(T, B, H, D).permute(1, 2, 0, 3).contiguous() for i in range(3))
    tmask = torch.from_numpy(allowed | (~valid[:, :, None] & np.eye(T, dtype=bool)[None]))[:, None].to(dev)
    keep.append((qkv, out, dl, desc, tq, tk, tv, tmask))
    rec = {"shape": name, "T": T, "B": B, "E": E, "heads": H, "chunk": chunk, "left": left, "right": right,
           "visible_pairs": pairs, "gflop": round(flop / 1e9, 3)}

    def ours(qkv=qkv, out=out, dl=dl, desc=desc, T=T, B=B, E=E):
        p = qkv.data_ptr()
        asr.check(L.asr_attention_fwd(ctypes.byref(desc), p, 3 * E, p + 4 * E, 3 * E, p + 8 * E, 3 * E, dl.data_ptr(),
                                      out.data_ptr(), E, T, 0, T, 0, B, st.cuda_stream), "asr_attention_fwd")

    res = {}

    def sdpa(tq=tq, tk=tk, tv=tv, tmask=tmask, res=res):
        with torch.cuda.stream(st), torch.no_grad():
            res["o"] = torch.nn.functional.scaled_dot_product_attention(tq, tk, tv, attn_mask=tmask)

    variants[f"{name}/asr_attention_fwd"] = (ours, {**rec, "kernel": "asr_attention_fwd"}, flop)
    variants[f"{name}/torch_sdpa_fp32"] = (sdpa, {**rec, "kernel": "torch scaled_dot_product_attention (fp32)"}, flop)
    checks[name] = (out, res, torch.from_numpy(valid).to(dev), (T, B, H, D))

torch.cuda.synchronize()   # the inputs were made on the default stream
for _ in range(a.warmup):
    for call, _r, _f in variants.values():
        call()
torch.cuda.synchronize()
for name, (out, res, valid, (T, B, H, D)) in checks.items():
    mine = out.reshape(T, B, H, D).permute(1, 2, 0, 3)
    diff = ((mine - res["o"]).abs() * valid[:, None, :, None]).max().item()
    print(json.dumps({"shape": name, "max_abs_diff_to_torch_on_valid_rows": diff}), flush=True)
ms = {k: [] for k in variants}
for _ in range(a.rounds):
    for k, (call, _r, _f) in variants.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(a.iters):
            call()
        e1.record(st)
        e1.synchronize()
        ms[k].append(e0.elapsed_time(e1) / a.iters)

for k, (_c, rec, flop) in variants.items():
    med = statistics.median(ms[k])
    row = {**rec, "rounds": a.rounds, "ms": round(med, 4), "ms_min": round(min(ms[k]), 4),
           "tflops": round(flop / med / 1e9, 2), "fp32_mfma_utilisation": round(flop / (med * 1e-3) / PEAK, 4)}
    if k.endswith("asr_attention_fwd"):
        row["ratio_to_torch"] = round(med / statistics.median(ms[k.split("/")[0] + "/torch_sdpa_fp32"]), 3)
    print(json.dumps(row), flush=True)
