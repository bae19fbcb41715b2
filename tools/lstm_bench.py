"""Per-frame time of the LSTM recurrence (asr_lstm_recur_fwd) at B = 1024,
T = 200, H = 128 (resident kernel), 256 and 512 (step kernel), against the
yardstick timed in the same process: the tanh recurrence asr_rnn_recur_fwd at
H = 256 on the fp32 MFMA kernel (ASR_RNN_RECUR_MFMA, ASR_DENSE_F32), which
issues the same MFMAs per wave and step as the resident LSTM at H = 128.
HIP events around each call, warm-up runs, then interleaved rounds (every
variant once per round); the median of the rounds.  One JSON line per shape.
    python tools/lstm_bench.py [--B 1024] [--T 200] [--H 128,256,512] [--rounds 11] [--warmup 2]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tests"))
from conftest import asr  # noqa: E402
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=1024)
ap.add_argument("--T", type=int, default=200)
ap.add_argument("--H", default="128,256,512")
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
a = ap.parse_args()
B, T = a.B, a.T
if a.rounds < 10:
    sys.exit("--rounds: at least 10 timed runs")
dev = torch.device("cuda")
torch.manual_seed(0)
L = asr.lib()
st = torch.cuda.Stream()


def uni(shape, s):
    return (torch.rand(shape, device=dev) * 2 - 1) * s


variants = {}   # name -> (call, record)

# the yardstick: tanh recurrence, H = 256, fp32 MFMA kernel (in place over P: timing only)
YH = 256
yw = [uni((YH, YH), YH ** -0.5), uni((YH,), 0.1), uni((YH,), 0.1)]
yhid = uni((T * B, YH), 1.0)


def yard():
    asr.check(L.asr_rnn_recur_fwd(None, yw[0].data_ptr(), yw[1].data_ptr(), yw[2].data_ptr(), yhid.data_ptr(),
                                  T, B, YH, st.cuda_stream), "asr_rnn_recur_fwd")


variants["rnn_tanh_mfma_f32_H256"] = (yard, {"kernel": "asr_rnn_recur_fwd", "H": YH})

keep = []
for H in (int(v) for v in a.H.split(",")):
    w = [uni((H, 4 * H), H ** -0.5), uni((4 * H,), 0.1), uni((4 * H,), 0.1)]
    P, hid = uni((T * B, 4 * H), 1.0), torch.empty((T * B, H), device=dev)
    work = torch.empty(asr.lstm_workspace_bytes(T, B, H) // 4, device=dev)
    wptr = work.data_ptr()
    keep.append((w, P, hid, work))

    def call(w=w, P=P, hid=hid, wptr=wptr, H=H):
        asr.check(L.asr_lstm_recur_fwd(P.data_ptr(), None, None, w[0].data_ptr(), w[1].data_ptr(), w[2].data_ptr(),
                                       hid.data_ptr(), H, None, None, None, wptr, T, B, H, 0, st.cuda_stream),
                  "asr_lstm_recur_fwd")

    variants[f"lstm_H{H}"] = (call, {"kernel": "asr_lstm_recur_fwd", "H": H,
                                     "form": "resident" if H <= 128 else "step"})

prev_kind, prev_arith = asr.rnn_get_recurrence(), asr.get_dense_arith()
asr.rnn_set_recurrence(asr.RNN_RECUR_MFMA)
asr.set_dense_arith(asr.DENSE_F32)
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
    asr.rnn_set_recurrence(prev_kind)
    asr.set_dense_arith(prev_arith)

yard_us = 1e3 * statistics.median(ms["rnn_tanh_mfma_f32_H256"]) / T
for k, (_c, rec) in variants.items():
    us = 1e3 * statistics.median(ms[k]) / T
    print(json.dumps({**rec, "B": B, "T": T, "rounds": a.rounds, "us_per_frame": round(us, 3),
                      "us_per_frame_min": round(1e3 * min(ms[k]) / T, 3),
                      "ratio_to_yardstick": round(us / yard_us, 3)}), flush=True)
