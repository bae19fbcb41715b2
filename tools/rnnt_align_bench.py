"""Time of transducer lattice scoring (asr_rnnt_align: the f GEMM, the predictor,
the fused joint kernel and the lattice kernel) at an n-best rescoring shape: the
c640 model of tests/rnnt_beam_cases.UPPER_CASES (E = 64, D = Hp = J = 640,
V = 1025, one layer, ReLU), T = 200, K = 4 hypotheses of 20 to 40 labels per
utterance, B = 64 (N = 256) and B = 256 (N = 1024), the one-per-frame lattice.
The yardstick is the same computation in torch on the device, in the same
process on the same weights: the teacher-forced nn.LSTM, the broadcast joint
[N][T][U+1][V], log_softmax, two gathers and a batched alpha recursion over the
frames in float64.  The tool first checks its own scores against the yardstick's,
then warms every variant and times them in interleaved rounds with HIP events
(every variant once per round); the median, the minimum and the spread of the
rounds.  One JSON line per variant and batch size.
    python tools/rnnt_align_bench.py [--B 64,256] [--T 200] [--K 4] [--rounds 11] [--warmup 2]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tests"))
from conftest import asr  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402
import rnnt_beam_cases as bc  # noqa: E402
import rnnt_cases as rc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--B", default="64,256")
ap.add_argument("--T", type=int, default=200)
ap.add_argument("--K", type=int, default=4)
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--clock-ghz", type=float, default=2.4, help="for the fraction of the fp32-MFMA rate")
ap.add_argument("--cus", type=int, default=256)
a = ap.parse_args()
if a.rounds < 10:
    sys.exit("--rounds: at least 10 timed runs")
T, K = a.T, a.K
model = bc.UPPER_CASES[0].model
assert model.name == "c640-k4"
_T0, _B0, E, D, Hp, J, V, L = model.shape
BLANK = model.blank
TOPO = asr.RNNT_LATTICE_ONE_PER_FRAME
dev = torch.device("cuda")
gen = torch.Generator().manual_seed(0)
st = torch.cuda.Stream()

w, _enc = rc.make_model(model)
dec = rc.make_decoder(asr, model, w)
dec.upload()
tw = {n: torch.from_numpy(v[0] if isinstance(v, list) else v).to(dev) for n, v in w.items()}
lstm = torch.nn.LSTM(D, Hp, 1).to(dev)
with torch.no_grad():
    lstm.weight_ih_l0.copy_(tw["w_ih"].T)
    lstm.weight_hh_l0.copy_(tw["w_hh"].T)
    lstm.bias_ih_l0.copy_(tw["b_ih"])
    lstm.bias_hh_l0.copy_(tw["b_hh"])
NEG = float("-inf")


@torch.no_grad()
def torch_score(enc, tg, tl, utt):
    """enc [T, B, E], tg int64 [N, Umax], tl int64 [N], utt int64 [N] on the device: the one-per-frame score [N]."""
    N, Umax = tg.shape
    U1 = Umax + 1
    tokens = torch.cat([torch.full((N, 1), BLANK, dtype=torch.int64, device=dev), tg], 1)       # [N, U1]
    htop, _ = lstm(tw["emb"][tokens].transpose(0, 1).contiguous())                            # [U1, N, Hp]
    g = (htop @ tw["w_pred"] + tw["b_pred"]).transpose(0, 1)                                    # [N, U1, J]
    f = (enc @ tw["w_enc"] + tw["b_enc"]).transpose(0, 1)[utt]                                  # [N, T, J]
    lp = torch.log_softmax(torch.relu(f[:, :, None, :] + g[:, None, :, :]) @ tw["w_out"] + tw["b_out"], dim=-1)
    lpb = lp[..., BLANK].double()                                                               # [N, T, U1]
    idx = torch.cat([tg, torch.zeros((N, 1), dtype=torch.int64, device=dev)], 1)              # label of state u
    lpy = lp.gather(3, idx[:, None, :, None].expand(N, T, U1, 1))[..., 0].double()
    lpy = torch.where(torch.arange(U1, device=dev)[None, None, :] < tl[:, None, None], lpy, NEG)
    del lp
    alpha = torch.full((N, U1), NEG, dtype=torch.float64, device=dev)
    alpha[:, 0] = 0.0
    pad = torch.full((N, 1), NEG, dtype=torch.float64, device=dev)
    for t in range(T):
        stay = alpha + lpb[:, t]
        move = torch.cat([pad, (alpha + lpy[:, t])[:, :-1]], 1)
        alpha = torch.logaddexp(stay, move)
    return alpha.gather(1, tl[:, None])[:, 0]


variants, keep = {}, []
for B in (int(v) for v in a.B.split(",")):
    N = B * K
    enc = (torch.rand((T, B, E), generator=gen) * 2 - 1).to(dev)
    tl = torch.randint(20, 41, (N,), generator=gen)
    mtl = int(tl.max())
    tg = torch.randint(1, V, (N, mtl), generator=gen)                       # blank = 0 never drawn
    utt = torch.arange(N) // K
    d = {"tg": tg.to(torch.int32).to(dev), "tl": tl.to(torch.int32).to(dev), "utt": utt.to(torch.int32).to(dev),
         "score": torch.zeros(N, dtype=torch.float64, device=dev)}
    work_bytes = dec.align_workspace_bytes(T, B, N, mtl)
    d["work"] = torch.empty(work_bytes // 4 + 4, device=dev)
    t64 = (tg.to(dev), tl.to(dev), utt.to(dev))
    flop = 2.0 * float((tl + 1).sum()) * T * J * V
    keep.append((B, N, enc, d, t64, flop, work_bytes))

    def fused(enc=enc, d=d, B=B, N=N, mtl=mtl):
        dec.align_device(enc.data_ptr(), T, B, d["tg"].data_ptr(), mtl, d["tl"].data_ptr(), N, mtl, TOPO,
                         d["score"].data_ptr(), 0, 0, d["work"].data_ptr(), 0, d["utt"].data_ptr(), stream=st.cuda_stream)

    def loop(enc=enc, t64=t64):
        with torch.cuda.stream(st):
            return torch_score(enc, *t64)

    variants[f"fused_B{B}"] = (fused, {"path": "asr_rnnt_align", "B": B, "N": N})
    variants[f"torch_B{B}"] = (loop, {"path": "torch", "B": B, "N": N})

# the scores agree before anything is timed (this is also the first warm-up)
peak = {}
for B, N, enc, d, t64, flop, work_bytes in keep:
    variants[f"fused_B{B}"][0]()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ref = variants[f"torch_B{B}"][0]()
    torch.cuda.synchronize()
    peak[B] = torch.cuda.max_memory_allocated() - base
    got, ref = d["score"].cpu().numpy(), ref.cpu().numpy()
    rel = np.abs(got - ref) / ((1.0 + np.abs(ref)) * (T + t64[1].cpu().numpy()))
    print(json.dumps({"check": f"B{B}", "max_rel_err_per_term": float(f"{rel.max():.3e}"), "bound": 2e-5}), flush=True)
    if not np.all(rel <= 2e-5):
        sys.exit(f"B = {B}: the fused scores differ from the torch yardstick's")
    torch.cuda.synchronize()

for _ in range(a.warmup):
    for call, _r in variants.values():
        call()
torch.cuda.synchronize()
ms = {n: [] for n in variants}
for _ in range(a.rounds):
    for n, (call, _r) in variants.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        call()
        e1.record(st)
        e1.synchronize()
        ms[n].append(e0.elapsed_time(e1))

for B, N, enc, d, t64, flop, work_bytes in keep:
    for kind in ("fused", "torch"):
        n = f"{kind}_B{B}"
        med = statistics.median(ms[n])
        row = {**variants[n][1], "T": T, "K": K, "rounds": a.rounds, "ms": round(med, 3), "ms_min": round(min(ms[n]), 3),
               "ms_max": round(max(ms[n]), 3), "spread_pct": round(100.0 * (max(ms[n]) - min(ms[n])) / med, 1)}
        row["ratio_to_torch"] = round(med / statistics.median(ms[f"torch_B{B}"]), 4)
        if kind == "fused":
            row["workspace_bytes"] = int(work_bytes)
            row["joint_gflop"] = round(flop / 1e9, 1)
            # the whole call's time against the joint's FLOP: a lower bound of the joint kernel's own fraction
            row["fraction_of_fp32_mfma_rate_whole_call"] = round(flop / (med * 1e-3) / (64.0 * 4 * a.cus * a.clock_ghz * 1e9), 4)
        else:
            row["peak_bytes"] = int(peak[B])
        print(json.dumps(row), flush=True)
dec.close()
