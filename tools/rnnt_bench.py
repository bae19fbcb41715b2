"""Time of a transducer greedy decode (asr_rnnt_greedy: the f GEMM and the one
decode launch) at D = Hp = J = 640, V = 1025, E = 512, L = 1, T = 200, B = 64
and 1024, against the yardstick timed in the same process on the same weights:
a batched greedy loop written in torch on the device, the usual per-step form
(LSTMCell, matmuls, argmax, one `any()` per step to leave a frame early).
Decoding is latency-critical, so the figure is the time of one whole decode.
HIP events around each call, warm-up runs, then interleaved rounds (every
variant once per round); the median of the rounds.  One JSON line per variant
and batch size, with the time per joint evaluation on the longest walk.
    python tools/rnnt_bench.py [--B 64,1024] [--T 200] [--rounds 11] [--warmup 2] [--max-symbols 10]
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
dev = torch.device("cuda")
gen = torch.Generator().manual_seed(0)
L = asr.lib()
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
dec = asr.TransducerDecoder(asr.rnnt_desc(V, BLANK, E, D, Hp, 1, J, "relu", MS), w)
dec.upload()
tw = {n: torch.from_numpy(v[0] if isinstance(v, list) else v).to(dev) for n, v in w.items()}
cell_b = tw["b_ih"] + tw["b_hh"]


def torch_cell(x, h, c):
    """torch.nn.LSTMCell's arithmetic on the library's [in][out] weights."""
    z = x @ tw["w_ih"] + h @ tw["w_hh"] + cell_b
    i, f, g, o = z.chunk(4, 1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c), c


def torch_greedy(enc):
    """enc [T, B, E] on the device.  Returns (tokens [n, B], emitted [n, B] bool, frames [n])."""
    B = enc.shape[1]
    F = (enc.reshape(T * B, E) @ tw["w_enc"] + tw["b_enc"]).reshape(T, B, J)
    h, c = torch_cell(tw["emb"][BLANK].expand(B, D), torch.zeros(B, Hp, device=dev), torch.zeros(B, Hp, device=dev))
    g = h @ tw["w_pred"] + tw["b_pred"]
    toks, emits, frames, lps = [], [], [], []
    for t in range(T):
        live = torch.ones(B, dtype=torch.bool, device=dev)
        for _n in range(MS):
            logit = torch.relu(F[t] + g) @ tw["w_out"] + tw["b_out"]
            top, kk = logit.max(1)
            lps.append(top - torch.logsumexp(logit, 1))
            emit = live & (kk != BLANK)
            if not bool(emit.any()):       # the per-step host sync of the usual form
                break
            h2, c2 = torch_cell(tw["emb"][kk], h, c)
            m = emit.unsqueeze(1)
            h, c = torch.where(m, h2, h), torch.where(m, c2, c)
            g = h @ tw["w_pred"] + tw["b_pred"]
            toks.append(kk), emits.append(emit), frames.append(t)
            live = emit
    return toks, emits, frames


variants, keep = {}, []
for B in (int(v) for v in a.B.split(",")):
    enc = (torch.rand((T, B, E), generator=gen) * 2 - 1).to(dev)
    mo = T * MS
    out = {"tok": torch.zeros((B, mo), dtype=torch.int32, device=dev), "ts": torch.zeros((B, mo), dtype=torch.int32, device=dev),
           "lp": torch.zeros((B, mo), dtype=torch.float64, device=dev), "cnt": torch.zeros(B, dtype=torch.int32, device=dev),
           "tot": torch.zeros(B, dtype=torch.float64, device=dev),
           "work": torch.empty(dec.workspace_bytes(T, B) // 4, device=dev)}
    keep.append((enc, out))

    def fused(enc=enc, out=out, B=B, mo=mo):
        dec.decode_device(enc.data_ptr(), T, B, mo, out["tok"].data_ptr(), out["ts"].data_ptr(), out["lp"].data_ptr(),
                          out["cnt"].data_ptr(), out["tot"].data_ptr(), out["work"].data_ptr(), stream=st.cuda_stream)

    def loop(enc=enc):
        with torch.cuda.stream(st):
            return torch_greedy(enc)

    variants[f"fused_B{B}"] = (fused, {"decode": "asr_rnnt_greedy", "B": B})
    variants[f"torch_B{B}"] = (loop, {"decode": "torch loop", "B": B})

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

for (enc, out), B in zip(keep, (int(v) for v in a.B.split(","))):
    # what the walk did, and whether the two decoders agree (fp32 near-ties may part them)
    cnt = out["cnt"].cpu().numpy()
    ts = out["ts"].cpu().numpy()
    tok = out["tok"].cpu().numpy()
    capped = np.array([int((np.bincount(ts[b, :cnt[b]], minlength=T) == MS).sum()) for b in range(B)])
    evals = T + cnt - capped            # joint evaluations of each utterance
    toks, emits, _frames = variants[f"torch_B{B}"][0]()
    torch.cuda.synchronize()
    agree = 0
    if toks:
        tk, em = torch.stack(toks).cpu().numpy(), torch.stack(emits).cpu().numpy()
        agree = sum(tk[em[:, b], b].tolist() == tok[b, :cnt[b]].tolist() for b in range(B))
    else:
        agree = int((cnt == 0).sum())
    for kind in ("fused", "torch"):
        n = f"{kind}_B{B}"
        med = statistics.median(ms[n])
        print(json.dumps({**variants[n][1], "T": T, "max_symbols": MS, "rounds": a.rounds, "ms": round(med, 3),
                          "ms_min": round(min(ms[n]), 3), "emissions_per_frame": round(float(cnt.mean()) / T, 3),
                          "joint_evals_longest_walk": int(evals.max()),
                          "us_per_joint_eval": round(1e3 * med / int(evals.max()), 2),
                          "ratio_to_torch_loop": round(med / statistics.median(ms[f"torch_B{B}"]), 3),
                          "utterances_agreeing_with_torch": f"{agree}/{B}"}), flush=True)
dec.close()
