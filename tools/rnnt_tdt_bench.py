"""Time of a token-and-duration transducer greedy decode (asr_rnnt_greedy_tdt: the
f GEMM and the one decode launch) at D = Hp = J = 640, V = 1025, E = 512, L = 1,
T = 200, durations [0, 1, 2, 3, 4], B = 64 and 1024, against two things timed in
the same process on the same weights: the same TDT walk as a batched torch loop
on the device (the usual per-step form: every utterance at its own frame, one
matmul over the V + D outputs, two argmaxes, a masked LSTMCell, one `any()` per
step), and asr_rnnt_greedy on the token head alone, another walk (it cannot
jump), for the time per joint evaluation of the two kernels.  HIP events around
each call, warm-up runs, then interleaved rounds (every variant once per
round); the median of the rounds.  One JSON line per variant and batch size.
The tokens of the kernel and of the torch loop must agree on every utterance,
else the exit status is 1.
    python tools/rnnt_tdt_bench.py [--B 64,1024] [--T 200] [--rounds 11] [--warmup 2] [--max-symbols 10]
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

ap = argparse.ArgumentParser()
ap.add_argument("--B", default="64,1024")
ap.add_argument("--T", type=int, default=200)
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--max-symbols", type=int, default=10)
ap.add_argument("--blank-bias", type=float, default=7.8)
a = ap.parse_args()
if a.rounds < 10:
    sys.exit("--rounds: at least 10 timed runs")
T, MS = a.T, a.max_symbols
E = 512
D = Hp = J = 640
V, BLANK = 1025, 1024
DUR = [0, 1, 2, 3, 4]
ND = len(DUR)
dev = torch.device("cuda")
gen = torch.Generator().manual_seed(0)
st = torch.cuda.Stream()


def uni(shape, s):
    return ((torch.rand(shape, generator=gen) * 2 - 1) * s).numpy()


k = Hp ** -0.5
w = {"emb": uni((V, D), 1.0), "w_ih": [uni((D, 4 * Hp), k)], "w_hh": [uni((Hp, 4 * Hp), k)],
     "b_ih": [uni((4 * Hp,), k)], "b_hh": [uni((4 * Hp,), k)],
     "w_enc": uni((E, J), (3.0 / E) ** 0.5), "b_enc": uni((J,), 0.1),
     "w_pred": uni((Hp, J), (3.0 / Hp) ** 0.5 * 4.0), "b_pred": uni((J,), 0.1),
     "w_out": uni((J, V), (3.0 / J) ** 0.5 * 4.0), "b_out": uni((V,), 0.1)}
w["b_out"][BLANK] = a.blank_bias
desc = asr.rnnt_desc(V, BLANK, E, D, Hp, 1, J, "relu", MS)
plain = asr.TransducerDecoder(desc, w)
w["w_dur"], w["b_dur"] = uni((J, ND), (3.0 / J) ** 0.5 * 4.0), uni((ND,), 0.1)
tdt = asr.TransducerDecoder.tdt(desc, w, DUR)
plain.upload()
tdt.upload()
tw = {n: torch.from_numpy(v[0] if isinstance(v, list) else v).to(dev) for n, v in w.items()}
cell_b = tw["b_ih"] + tw["b_hh"]
w_cat, b_cat = torch.cat([tw["w_out"], tw["w_dur"]], 1), torch.cat([tw["b_out"], tw["b_dur"]])
table = torch.tensor(DUR, device=dev)


def torch_cell(x, h, c):
    """torch.nn.LSTMCell's arithmetic on the library's [in][out] weights."""
    z = x @ tw["w_ih"] + h @ tw["w_hh"] + cell_b
    i, f, g, o = z.chunk(4, 1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c), c


def torch_tdt(enc):
    """enc [T, B, E] on the device.  Returns (tokens [n, B], emitted [n, B] bool, evaluations [B])."""
    B = enc.shape[1]
    F = (enc.reshape(T * B, E) @ tw["w_enc"] + tw["b_enc"]).reshape(T, B, J)
    h, c = torch_cell(tw["emb"][BLANK].expand(B, D), torch.zeros(B, Hp, device=dev), torch.zeros(B, Hp, device=dev))
    g = h @ tw["w_pred"] + tw["b_pred"]
    rows = torch.arange(B, device=dev)
    t = torch.zeros(B, dtype=torch.int64, device=dev)
    n, evals = torch.zeros_like(t), torch.zeros_like(t)
    toks, emits, lps = [], [], []
    while True:
        live = t < T
        if not bool(live.any()):       # the per-step host sync of the usual form
            break
        logit = torch.relu(F[t.clamp(max=T - 1), rows] + g) @ w_cat + b_cat
        top, kk = logit[:, :V].max(1)
        dtop, dd = logit[:, V:].max(1)
        lps.append((top - torch.logsumexp(logit[:, :V], 1)) + (dtop - torch.logsumexp(logit[:, V:], 1)))
        dur = table[dd]
        blank = kk == BLANK
        emit = live & ~blank
        h2, c2 = torch_cell(tw["emb"][kk], h, c)
        m = emit.unsqueeze(1)
        h, c = torch.where(m, h2, h), torch.where(m, c2, c)
        g = h @ tw["w_pred"] + tw["b_pred"]
        n = torch.where(emit, n + 1, torch.zeros_like(n))
        adv = torch.where(blank, dur.clamp(min=1), torch.where(dur > 0, dur, (n == MS).long()))
        n = torch.where(adv > 0, torch.zeros_like(n), n)
        t = torch.where(live, t + adv, t)
        evals += live
        toks.append(kk), emits.append(emit)
    return toks, emits, evals


variants, keep = {}, []
for B in (int(v) for v in a.B.split(",")):
    enc = (torch.rand((T, B, E), generator=gen) * 2 - 1).to(dev)
    mo = T * MS
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)      # noqa: E731
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)    # noqa: E731
    outs = {kind: {"tok": i32(B, mo), "ts": i32(B, mo), "dur": i32(B, mo), "lp": f64(B, mo), "cnt": i32(B),
                   "tot": f64(B), "work": torch.empty(tdt.workspace_bytes(T, B) // 4, device=dev)}
            for kind in ("tdt", "plain")}
    keep.append((enc, outs))

    def fused(dec, o, enc=enc, B=B, mo=mo):
        dec.decode_device(enc.data_ptr(), T, B, mo, o["tok"].data_ptr(), o["ts"].data_ptr(), o["lp"].data_ptr(),
                          o["cnt"].data_ptr(), o["tot"].data_ptr(), o["work"].data_ptr(), stream=st.cuda_stream,
                          **({"d_durations": o["dur"].data_ptr()} if dec is tdt else {}))

    def loop(enc=enc):
        with torch.cuda.stream(st):
            return torch_tdt(enc)

    variants[f"tdt_B{B}"] = (lambda f=fused, o=outs["tdt"]: f(tdt, o), {"decode": "asr_rnnt_greedy_tdt", "B": B})
    variants[f"torch_B{B}"] = (loop, {"decode": "torch loop, the TDT walk", "B": B})
    variants[f"plain_B{B}"] = (lambda f=fused, o=outs["plain"]: f(plain, o),
                               {"decode": "asr_rnnt_greedy, the token head alone", "B": B})

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

status = 0
for (enc, outs), B in zip(keep, (int(v) for v in a.B.split(","))):
    toks, emits, evals_tdt = variants[f"torch_B{B}"][0]()
    torch.cuda.synchronize()
    o = {kind: {n: v.cpu().numpy() for n, v in outs[kind].items() if n != "work"} for kind in outs}
    cnt, tok = o["tdt"]["cnt"], o["tdt"]["tok"]
    tk, em = torch.stack(toks).cpu().numpy(), torch.stack(emits).cpu().numpy()
    agree = sum(tk[em[:, b], b].tolist() == tok[b, :cnt[b]].tolist() for b in range(B))
    status |= agree != B
    # joint evaluations of each utterance: the TDT walk's from the loop that agrees with it; the plain walk's from
    # its outputs (every frame ends by a blank or at the cap)
    pc, pts = o["plain"]["cnt"], o["plain"]["ts"]
    capped = np.array([int((np.bincount(pts[b, :pc[b]], minlength=T) == MS).sum()) for b in range(B)])
    evals = {"tdt": evals_tdt.cpu().numpy(), "torch": evals_tdt.cpu().numpy(), "plain": T + pc - capped}
    per_eval = {kind: 1e3 * statistics.median(ms[f"{kind}_B{B}"]) / int(evals[kind].max()) for kind in evals}
    for kind in ("tdt", "torch", "plain"):
        n = f"{kind}_B{B}"
        med = statistics.median(ms[n])
        print(json.dumps({**variants[n][1], "T": T, "max_symbols": MS, "rounds": a.rounds, "ms": round(med, 3),
                          "ms_min": round(min(ms[n]), 3), "ms_max": round(max(ms[n]), 3),
                          "emissions_per_frame": round(float((pc if kind == "plain" else cnt).mean()) / T, 3),
                          "joint_evals_longest_walk": int(evals[kind].max()),
                          "joint_evals_mean": round(float(evals[kind].mean()), 1),
                          "us_per_joint_eval": round(per_eval[kind], 2),
                          "per_eval_ratio_to_plain_kernel": round(per_eval[kind] / per_eval["plain"], 3),
                          "ratio_to_torch_loop": round(med / statistics.median(ms[f"torch_B{B}"]), 3),
                          "utterances_agreeing_with_torch": f"{agree}/{B}"}), flush=True)
plain.close()
tdt.close()
sys.exit(status)
