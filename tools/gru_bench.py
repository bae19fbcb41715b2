"""Per-frame time of the GRU recurrence (asr_gru_recur_fwd) at B = 1024,
T = 200, H = 128 (resident kernel), 256, 512 and 1024 (step kernel), against
the yardstick timed in the same process: the LSTM recurrence
asr_lstm_recur_fwd at the same H, whose kernel of the same form issues 4/3 of
the GRU's MFMAs, reads 4/3 of its P bytes and has five transcendentals per
element against three.  HIP events around each call, warm-up runs, then
interleaved rounds (every variant once per round); the median of the rounds.
One JSON line per kernel and shape.
    python tools/gru_bench.py [--B 1024] [--T 200] [--H 128,256,512,1024] [--rounds 11] [--warmup 2]
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
ap.add_argument("--H", default="128,256,512,1024")
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
keep = []
for H in (int(v) for v in a.H.split(",")):
    form = "resident" if H <= 128 else "step"
    hid = torch.empty((T * B, H), device=dev)

    # the yardstick: the LSTM recurrence at this H
    lw = [uni((H, 4 * H), H ** -0.5), uni((4 * H,), 0.1), uni((4 * H,), 0.1)]
    lP = uni((T * B, 4 * H), 1.0)
    lwork = torch.empty(asr.lstm_workspace_bytes(T, B, H) // 4, device=dev)
    # the GRU recurrence
    gw = [uni((H, 3 * H), H ** -0.5), uni((3 * H,), 0.1), uni((3 * H,), 0.1)]
    gP = uni((T * B, 3 * H), 1.0)
    keep.append((hid, lw, lP, lwork, gw, gP))

    def lstm(w=lw, P=lP, hid=hid, wptr=lwork.data_ptr(), H=H):
        asr.check(L.asr_lstm_recur_fwd(P.data_ptr(), None, None, w[0].data_ptr(), w[1].data_ptr(), w[2].data_ptr(),
                                       hid.data_ptr(), H, None, None, None, wptr, T, B, H, 0, st.cuda_stream),
                  "asr_lstm_recur_fwd")

    def gru(w=gw, P=gP, hid=hid, H=H):
        asr.check(L.asr_gru_recur_fwd(P.data_ptr(), None, w[0].data_ptr(), w[1].data_ptr(), w[2].data_ptr(),
                                      hid.data_ptr(), H, None, None, T, B, H, 0, st.cuda_stream),
                  "asr_gru_recur_fwd")

    variants[f"lstm_H{H}"] = (lstm, {"kernel": "asr_lstm_recur_fwd", "H": H, "form": form})
    variants[f"gru_H{H}"] = (gru, {"kernel": "asr_gru_recur_fwd", "H": H, "form": form})

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

for k, (_c, rec) in variants.items():
    us = 1e3 * statistics.median(ms[k]) / T
    yard_us = 1e3 * statistics.median(ms[f"lstm_H{rec['H']}"]) / T
    print(json.dumps({**rec, "B": B, "T": T, "rounds": a.rounds, "us_per_frame": round(us, 3),
                      "us_per_frame_min": round(1e3 * min(ms[k]) / T, 3),
                      "ratio_to_lstm_same_H": round(us / yard_us, 3)}), flush=True)
