"""Kernel time of asr_ctc_align (CTC forced alignment / exact scoring) at
N = B = 2048 targets of L = 100 labels over T = 1000 frames, V = 29: score only,
Viterbi score only, path only, and every output; an n-best call (B = 256
utterances, 8 hypotheses each through d_utt); and, for scale, the beam-search
kernel time of decoding the same emissions (asr_ctc_last_kernel_ms).  HIP
events on an otherwise idle stream around each call, warm-up calls, then
interleaved rounds (every variant once per round); the median of the rounds.
One JSON line per variant.  ASR_LIB selects an A/B build of the library
(csrc/ctc_align.hip: ASR_ALIGN_TB_CHUNK, ASR_ALIGN_NO_TRACEBACK).
    python tools/ctc_align_bench.py [--B 2048] [--T 1000] [--V 29] [--L 100] [--rounds 11] [--warmup 2] [--beam 50]
"""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tests"))
from conftest import asr  # noqa: E402
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=2048)
ap.add_argument("--T", type=int, default=1000)
ap.add_argument("--V", type=int, default=29)
ap.add_argument("--L", type=int, default=100)
ap.add_argument("--nbest", type=int, default=8)
ap.add_argument("--beam", type=int, default=50, help="beam of the decode timed for scale (0: skip it)")
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
a = ap.parse_args()
if a.rounds < 10:
    sys.exit("--rounds: at least 10 timed runs")
B, T, V, L = a.B, a.T, a.V, a.L
dev = torch.device("cuda")
torch.manual_seed(0)
st = torch.cuda.Stream()

emis = torch.log_softmax(torch.randn((T, B, V), device=dev) * 3.0, dim=2).contiguous()
targets = torch.randint(1, V, (B, L), dtype=torch.int32, device=dev)
tlen = torch.full((B,), L, dtype=torch.int32, device=dev)
utt = (torch.arange(B, dtype=torch.int32, device=dev) // a.nbest).contiguous()   # n-best: B / nbest utterances
score = torch.empty(B, dtype=torch.float64, device=dev)
vscore = torch.empty(B, dtype=torch.float64, device=dev)
path = torch.empty((B, T), dtype=torch.int32, device=dev)
spans = torch.empty((B, L, 2), dtype=torch.int32, device=dev)
work = torch.empty(asr.ctc_align_workspace_bytes(T, B, L), dtype=torch.uint8, device=dev)


def call(nb, d_utt, d_score, d_vscore, d_path, d_spans):
    def run():
        asr.ctc_align_device(emis.data_ptr(), T, nb, V, B * V, V, 0, True, 0, targets.data_ptr(), L, tlen.data_ptr(),
                             d_utt, B, L, d_score, d_vscore, d_path, T, d_spans,
                             work.data_ptr() if (d_path or d_spans) else 0, st.cuda_stream)
    return run


variants = {
    "score": call(B, 0, score.data_ptr(), 0, 0, 0),
    "vscore": call(B, 0, 0, vscore.data_ptr(), 0, 0),
    "path": call(B, 0, 0, 0, path.data_ptr(), 0),
    "all": call(B, 0, score.data_ptr(), vscore.data_ptr(), path.data_ptr(), spans.data_ptr()),
    "nbest_score": call(B // a.nbest, utt.data_ptr(), score.data_ptr(), 0, 0, 0),
    "nbest_all": call(B // a.nbest, utt.data_ptr(), score.data_ptr(), vscore.data_ptr(), path.data_ptr(),
                      spans.data_ptr()),
}
for _ in range(a.warmup):
    for run in variants.values():
        run()
torch.cuda.synchronize()
ms = {k: [] for k in variants}
for _ in range(a.rounds):
    for k, run in variants.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        run()
        e1.record(st)
        e1.synchronize()
        ms[k].append(e0.elapsed_time(e1))
rec = {"lib": os.environ.get("ASR_LIB", "libasr_amd.so"), "N": B, "T": T, "V": V, "L": L, "rounds": a.rounds}
for k in variants:
    med = statistics.median(ms[k])
    print(json.dumps({**rec, "variant": k, "B": B // a.nbest if k.startswith("nbest") else B, "ms": round(med, 3),
                      "ms_min": round(min(ms[k]), 3), "ms_max": round(max(ms[k]), 3),
                      "target_frames_per_s": round(B * T / med * 1e3)}), flush=True)
if a.beam:
    dec = asr.CTCDecoder(V, a.beam, 0)
    t = []
    for _ in range(3):
        dec.decode_device(emis.data_ptr(), T, B, True, st.cuda_stream)
        dec.best_arrays()
        t.append(dec.last_kernel_ms())
    print(json.dumps({**rec, "variant": f"decode_beam{a.beam}", "B": B, "ms": round(statistics.median(t[1:]), 3)}),
          flush=True)
    dec.close()
