"""Time of the torch.stft-style front end (asr_stft_fwd) at Whisper's shape
(n_fft = win 400, hop 160, 80 mels, 30 s: 3000 frames per utterance; B = 8 and
64) against the torch-on-GPU composition of the same maths in fp32 (torch.stft,
power, mel matmul, log10, range clamp, affine, permute to time-major), and at
n_fft 512, win 400, hop 160, 40 mels against asr_fbank_fwd at its nearest
configuration (Kaldi framing, the same sizes).  HIP events around each call,
warm-up runs, then interleaved rounds (every variant once per round); median
and min - max of the rounds.  One JSON line per variant, with the fraction of
the fp32 MFMA peak the DFT's 2 * frames * n_fft * 2 NBp flops reach.
    python tools/stft_bench.py [--B 8,64] [--rounds 11] [--warmup 2] [--peak_tflops 157.3]
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
ap.add_argument("--B", default="8,64")
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--peak_tflops", type=float, default=157.3)
a = ap.parse_args()
if a.rounds < 10:
    sys.exit("--rounds: at least 10 timed runs")
dev = torch.device("cuda")
torch.manual_seed(0)
L = asr.lib()
st = torch.cuda.Stream()
S = 480000
variants, keep = {}, []


def add_stft(name, fe, wave, B, pad_to):
    T = fe.num_frames(pad_to or S)
    out = torch.empty((T * B, fe.cfg.n_mels), device=dev)
    frames = torch.empty(B, dtype=torch.int32, device=dev)
    work = torch.empty(max(4, fe.workspace_bytes(T, B) // 4), device=dev)
    keep.append((fe, out, frames, work))

    def call():
        asr.check(L.asr_stft_fwd(fe.h, wave.data_ptr(), S, None, B, S, pad_to, out.data_ptr(), fe.cfg.n_mels,
                                 frames.data_ptr(), work.data_ptr(), T, st.cuda_stream), "asr_stft_fwd")
        return out
    nbp = (fe.cfg.n_fft // 2 + 1 + 15) // 16 * 16
    variants[name] = (call, {"B": B, "T": T, "kernel": "asr_stft_fwd", "n_fft": fe.cfg.n_fft,
                             "dft_gflop": 2e-9 * T * B * fe.cfg.n_fft * 2 * nbp})


for B in (int(v) for v in a.B.split(",")):
    wave = torch.rand((B, S), device=dev) - 0.5
    fe = asr.StftFrontend.whisper(80)
    add_stft(f"stft_whisper_B{B}", fe, wave, B, 0)
    win, melT = torch.from_numpy(fe.window).to(dev), torch.from_numpy(fe.mel).to(dev).T.contiguous()

    def composed(wave=wave, win=win, melT=melT, B=B):
        with torch.cuda.stream(st):
            X = torch.stft(wave, 400, 160, window=win, return_complex=True)[..., :-1]          # [B, 201, 3000]
            x = torch.log10(torch.clamp((X.real ** 2 + X.imag ** 2).transpose(1, 2) @ melT, min=1e-10))
            x = torch.maximum(x, x.amax(dim=(1, 2), keepdim=True) - 8.0)
            return ((x + 4.0) / 4.0).permute(1, 0, 2).reshape(-1, 80).contiguous()
    variants[f"torch_whisper_B{B}"] = (composed, {"B": B, "T": 3000, "kernel": "torch composition"})

    cfg = asr.stft_config(512, 400, 160, False, 2, 40, "ln", "clamp", 1e-10)
    add_stft(f"stft_512_B{B}", asr.StftFrontend(cfg, asr.stft_window("hann", 400, False),
                                                asr.mel_filter_bank(257, 40, 0.0, 8000.0, 16000.0)), wave, B, 0)
    fb = asr.FeatureFrontend(n_fft=512, win_length=400, hop_length=160, preemph=0.0, n_mels=40, n_mfcc=0)
    Tf = fb.num_frames(S)
    fout, ffr = torch.empty((Tf * B, 40), device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    keep.append((fb, fout, ffr))

    def fbank(fb=fb, fout=fout, ffr=ffr, wave=wave, B=B, Tf=Tf):
        asr.check(L.asr_fbank_fwd(fb.h, wave.data_ptr(), S, None, B, S, fout.data_ptr(), 40, ffr.data_ptr(), None, Tf,
                                  st.cuda_stream), "asr_fbank_fwd")
        return fout
    variants[f"fbank_512_B{B}"] = (fbank, {"B": B, "T": Tf, "kernel": "asr_fbank_fwd", "n_fft": 512})

res = {}
for _ in range(a.warmup):
    for k, (call, _r) in variants.items():
        res[k] = call()
torch.cuda.synchronize()
diff = {B: (res[f"stft_whisper_B{B}"] - res[f"torch_whisper_B{B}"]).abs().max().item()
        for B in (int(v) for v in a.B.split(","))}
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
    row = {"variant": k, **rec, "rounds": a.rounds, "ms": round(med, 3), "ms_min": round(min(ms[k]), 3),
           "ms_max": round(max(ms[k]), 3), "frames_per_s": round(rec["T"] * rec["B"] / med * 1e3)}
    if "dft_gflop" in rec:
        row["fraction_of_fp32_mfma_peak"] = round(rec["dft_gflop"] / med / a.peak_tflops, 4)
    if k.startswith("stft_whisper"):
        row["max_abs_diff_vs_torch"] = diff[rec["B"]]
    print(json.dumps(row), flush=True)
