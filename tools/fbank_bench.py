"""Time of the audio front end (asr_fbank_fwd) at B = 1024 utterances of 10 s at
16 kHz (S = 160000; win 400, hop 160, n_fft 512, 40 mels, 26 MFCCs), without
(C = 0) and with a +-9 frame context window (C = 9), against the yardstick
timed in the same process: the torch-on-GPU composition of the same maths
(pre-emphasis, unfold framing, window, torch.fft.rfft, power, mel matmul, log,
DCT matmul, context unfold, permute to time-major) on the library's own fp32
tables.  HIP events around each call, warm-up runs, then interleaved rounds
(every variant once per round); the median of the rounds.  One JSON line per
variant; the largest difference between the two results is printed with it.
    python tools/fbank_bench.py [--B 1024] [--S 160000] [--C 0,9] [--rounds 11] [--warmup 2]
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
ap.add_argument("--S", type=int, default=160000)
ap.add_argument("--C", default="0,9")
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
a = ap.parse_args()
B, S = a.B, a.S
if a.rounds < 10:
    sys.exit("--rounds: at least 10 timed runs")
dev = torch.device("cuda")
torch.manual_seed(0)
L = asr.lib()
st = torch.cuda.Stream()
CFG = dict(sample_rate=16000.0, win_length=400, hop_length=160, n_fft=512, window="hann", preemph=0.97, n_mels=40,
           f_min=0.0, f_max=8000.0, log_floor=1e-10, n_mfcc=26)
WIN, HOP, NFFT, PRE, FLOOR = CFG["win_length"], CFG["hop_length"], CFG["n_fft"], CFG["preemph"], CFG["log_floor"]

wave = torch.rand((B, S), device=dev) - 0.5
variants, keep, results = {}, [], {}
for C in (int(v) for v in a.C.split(",")):
    fe = asr.FeatureFrontend(n_context=C, **CFG)
    T, F = fe.num_frames(S), fe.feature_dim
    win, mel, dct = (torch.from_numpy(t).to(dev) for t in fe.host_tables())
    out = torch.empty((T * B, F), device=dev)
    frames = torch.empty(B, dtype=torch.int32, device=dev)
    work = torch.empty(max(4, fe.workspace_bytes(T, B) // 4), device=dev)
    keep.append((fe, out, frames, work))

    def fused(fe=fe, out=out, frames=frames, work=work, T=T, F=F):
        asr.check(L.asr_fbank_fwd(fe.h, wave.data_ptr(), S, None, B, S, out.data_ptr(), F, frames.data_ptr(),
                                  work.data_ptr(), T, st.cuda_stream), "asr_fbank_fwd")
        return out

    def composed(win=win, melT=mel.T.contiguous(), dctT=dct.T.contiguous(), C=C, T=T, F=F):
        with torch.cuda.stream(st):
            y = wave.clone()
            y[:, 1:] -= PRE * wave[:, :-1]
            X = torch.fft.rfft(y.unfold(1, WIN, HOP) * win, n=NFFT)
            e = torch.log(torch.clamp((X.real ** 2 + X.imag ** 2) @ melT, min=FLOOR)) @ dctT   # [B, T, D]
            if C:
                e = torch.nn.functional.pad(e, (0, 0, C, C)).unfold(1, 2 * C + 1, 1)           # [B, T, D, 2C+1]
                return e.permute(1, 0, 3, 2).reshape(T * B, F).contiguous()
            return e.permute(1, 0, 2).reshape(T * B, F).contiguous()

    rec = {"B": B, "S": S, "T": T, "F": F, "n_context": C}
    variants[f"fbank_C{C}"] = (fused, {**rec, "kernel": "asr_fbank_fwd"})
    variants[f"torch_C{C}"] = (composed, {**rec, "kernel": "torch composition"})

res = {}
for _ in range(a.warmup):
    for k, (call, _r) in variants.items():
        res[k] = call()
torch.cuda.synchronize()
for C in (int(v) for v in a.C.split(",")):
    d = (res[f"fbank_C{C}"] - res[f"torch_C{C}"]).abs().max().item()
    results[C] = d
res.clear()
ms = {k: [] for k in variants}
for _ in range(a.rounds):
    for k, (call, _r) in variants.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        r = call()
        e1.record(st)
        e1.synchronize()
        del r
        ms[k].append(e0.elapsed_time(e1))

for k, (_c, rec) in variants.items():
    med = statistics.median(ms[k])
    yard = statistics.median(ms["torch_C%d" % rec["n_context"]])
    print(json.dumps({**rec, "rounds": a.rounds, "ms": round(med, 3), "ms_min": round(min(ms[k]), 3),
                      "frames_per_s": round(rec["T"] * B / med * 1e3), "ratio_to_torch": round(med / yard, 3),
                      "max_abs_diff_fused_vs_torch": results[rec["n_context"]]}), flush=True)
