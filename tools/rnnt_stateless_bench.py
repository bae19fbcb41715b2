"""Time of a stateless-predictor transducer decode (asr_rnnt_greedy_stateless and
asr_rnnt_beam at K = 4 on a stateless handle: C = 2, D = Hp = J = 512, V = 500,
tanh, E = 512, T = 200, B = 64 and 256) against two baselines timed in the same
process: the same search on the same weights as a batched torch loop on the
device (the usual per-step form: masked embedding, the conv as an einsum, ReLU,
the joiner's matmuls, argmax or top-K; rnnt_beam_bench.py's loop with the
stateless predictor), and an LSTM handle (L = 1) of the same Hp / J / V: the
kernels the stateless ones were cut from, another model.  The figure is the
time of one whole decode (the f GEMM and the one launch).  HIP events around
each call, warm-up runs, then interleaved rounds (every variant once per
round); the median and the range of the rounds.  One JSON line per variant and
batch size.
    python tools/rnnt_stateless_bench.py [--B 64,256] [--T 200] [--rounds 11] [--warmup 2]
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
ap.add_argument("--B", default="64,256")
ap.add_argument("--T", type=int, default=200)
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--blank-bias", type=float, default=4.0)
a = ap.parse_args()
if a.rounds < 10:
    sys.exit("--rounds: at least 10 timed runs")
T, K, MS = a.T, 4, 1
E = D = Hp = J = 512
V, BLANK, C = 500, 0, 2
dev = torch.device("cuda")
gen = torch.Generator().manual_seed(0)
st = torch.cuda.Stream()


def uni(shape, s):
    return ((torch.rand(shape, generator=gen) * 2 - 1) * s).numpy()


k = Hp ** -0.5
joint = {"w_enc": uni((E, J), (3.0 / E) ** 0.5), "b_enc": uni((J,), 0.1),
         "w_pred": uni((Hp, J), (3.0 / Hp) ** 0.5 * 4.0), "b_pred": uni((J,), 0.1),
         "w_out": uni((J, V), (3.0 / J) ** 0.5 * 4.0), "b_out": uni((V,), 0.1)}
joint["b_out"][BLANK] = a.blank_bias
emb = uni((V, D), 1.0)
w_ctx = uni((C, D, Hp), (3.0 / (D * C)) ** 0.5 * 2.0)
decs = {"stateless": asr.TransducerDecoder.stateless(
            asr.rnnt_stateless_desc(V, BLANK, E, D, Hp, J, "tanh", MS, C, -1),
            {"emb": emb, "w_ctx": w_ctx, "b_ctx": None, **joint}),
        "lstm": asr.TransducerDecoder(
            asr.rnnt_desc(V, BLANK, E, D, Hp, 1, J, "tanh", MS),
            {"emb": emb, "w_ih": [uni((D, 4 * Hp), k)], "w_hh": [uni((Hp, 4 * Hp), k)], "b_ih": [uni((4 * Hp,), k)],
             "b_hh": [uni((4 * Hp,), k)], **joint})}
for d in decs.values():
    d.upload()

tw = {n: torch.from_numpy(v).to(dev) for n, v in {"emb": emb, "w_ctx": w_ctx, **joint}.items()}
NEG = float("-inf")


def torch_pred(ctx):
    """ctx [N, C] int64, -1 for none -> g [N, J]."""
    e = tw["emb"][ctx.clamp(min=0)] * (ctx >= 0).unsqueeze(2)
    return torch.relu(torch.einsum("ncd,cdh->nh", e, tw["w_ctx"])) @ tw["w_pred"] + tw["b_pred"]


def start_ctx(N):
    ctx = torch.full((N, C), -1, dtype=torch.int64, device=dev)
    ctx[:, C - 1] = BLANK
    return ctx


def torch_greedy(enc):
    """One symbol per frame.  Returns tokens [T, B] (the blank where nothing was emitted)."""
    B = enc.shape[1]
    F = (enc.reshape(T * B, E) @ tw["w_enc"] + tw["b_enc"]).reshape(T, B, J)
    ctx = start_ctx(B)
    g = torch_pred(ctx)
    toks = []
    for t in range(T):
        kk = (torch.tanh(F[t] + g) @ tw["w_out"] + tw["b_out"]).argmax(1)
        emit = (kk != BLANK).unsqueeze(1)
        ctx = torch.where(emit, torch.cat([ctx[:, 1:], kk.unsqueeze(1)], 1), ctx)
        g = torch_pred(ctx)
        toks.append(kk)
    return torch.stack(toks)


def torch_beam(enc):
    """rnnt_beam_bench.py's loop: top-K over K V candidates, merge by length and hash, the context by parent."""
    B = enc.shape[1]
    F = (enc.reshape(T * B, E) @ tw["w_enc"] + tw["b_enc"]).reshape(T, B, J)
    ctx = start_ctx(B * K)
    g = torch_pred(ctx)
    score = torch.full((B, K), NEG, dtype=torch.float64, device=dev)
    score[:, 0] = 0.0
    ys = torch.full((B, K, T + 1), -1, dtype=torch.int64, device=dev)
    ln = torch.zeros((B, K), dtype=torch.int64, device=dev)
    hsh = torch.zeros((B, K), dtype=torch.int64, device=dev)
    rows = torch.arange(B, device=dev).unsqueeze(1)
    upper = torch.triu(torch.ones(K, K, dtype=torch.bool, device=dev))
    strict = torch.triu(torch.ones(K, K, dtype=torch.bool, device=dev), 1)
    for t in range(T):
        logit = torch.tanh(F[t].repeat_interleave(K, 0) + g) @ tw["w_out"] + tw["b_out"]
        lp = (logit - torch.logsumexp(logit, 1, keepdim=True)).reshape(B, K, V)
        top, idx = (score.unsqueeze(2) + lp.double()).reshape(B, K * V).topk(K, dim=1)
        par, tok = idx // V, idx % V
        emit = tok != BLANK
        ys, ln, hsh = ys[rows, par], ln[rows, par], hsh[rows, par]
        ys.scatter_(2, torch.where(emit, ln, T).unsqueeze(2), tok.unsqueeze(2))
        ln = ln + emit
        hsh = torch.where(emit, hsh * 1000003 + tok + 1, hsh)
        live = top > NEG
        eq = (hsh.unsqueeze(2) == hsh.unsqueeze(1)) & (ln.unsqueeze(2) == ln.unsqueeze(1)) & \
            live.unsqueeze(2) & live.unsqueeze(1)
        merged = torch.logsumexp(torch.where(eq & upper, top.unsqueeze(1).expand(B, K, K), NEG), dim=2)
        merged = torch.where((eq & strict).any(1) | ~live, NEG, merged)
        score, order = merged.sort(dim=1, descending=True, stable=True)
        ys, ln, hsh = ys[rows, order], ln[rows, order], hsh[rows, order]
        par, tok, emit = par[rows, order], tok[rows, order], emit[rows, order]
        c0 = ctx[(rows * K + par).reshape(-1)]
        ctx = torch.where(emit.reshape(-1, 1), torch.cat([c0[:, 1:], tok.reshape(-1, 1)], 1), c0)
        g = torch_pred(ctx)
    return ys, ln, score


variants, keep = {}, []
for B in (int(v) for v in a.B.split(",")):
    enc = (torch.rand((T, B, E), generator=gen) * 2 - 1).to(dev)
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)      # noqa: E731
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)    # noqa: E731
    for kind, dec in decs.items():
        o = {"tok": i32(B, K, T), "ts": i32(B, K, T), "lp": f64(B, T), "cnt": i32(B), "tot": f64(B), "len": i32(B, K),
             "sc": f64(B, K), "nh": i32(B),
             "work": torch.empty(max(dec.workspace_bytes(T, B), dec.beam_workspace_bytes(T, B, K)) // 4 + 4, device=dev)}
        keep.append((enc, o))

        def greedy(dec=dec, enc=enc, o=o, B=B):
            dec.decode_device(enc.data_ptr(), T, B, T, o["tok"].data_ptr(), o["ts"].data_ptr(), o["lp"].data_ptr(),
                              o["cnt"].data_ptr(), o["tot"].data_ptr(), o["work"].data_ptr(), stream=st.cuda_stream)

        def beam(dec=dec, enc=enc, o=o, B=B):
            dec.beam_search_device(enc.data_ptr(), T, B, K, K, T, o["tok"].data_ptr(), o["ts"].data_ptr(),
                                   o["len"].data_ptr(), o["sc"].data_ptr(), o["nh"].data_ptr(), o["work"].data_ptr(),
                                   stream=st.cuda_stream)

        variants[f"{kind}_greedy_B{B}"] = (greedy, {"predictor": kind, "search": "greedy", "B": B}, o)
        variants[f"{kind}_beam{K}_B{B}"] = (beam, {"predictor": kind, "search": f"beam {K}", "B": B}, o)

    def loop(fn, enc=enc):
        with torch.cuda.stream(st):
            return fn(enc)

    variants[f"torch_greedy_B{B}"] = (lambda loop=loop: loop(torch_greedy),
                                      {"predictor": "stateless, torch loop", "search": "greedy", "B": B}, None)
    variants[f"torch_beam{K}_B{B}"] = (lambda loop=loop: loop(torch_beam),
                                       {"predictor": "stateless, torch loop", "search": f"beam {K}", "B": B}, None)

for _ in range(a.warmup):
    for call, _r, _o in variants.values():
        call()
torch.cuda.synchronize()
ms = {n: [] for n in variants}
for _ in range(a.rounds):
    for n, (call, _r, _o) in variants.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        call()
        e1.record(st)
        e1.synchronize()
        ms[n].append(e0.elapsed_time(e1))

for n, (call, rec, o) in variants.items():
    res = call()
    torch.cuda.synchronize()
    kind, rest = n.split("_", 1)
    extra = {}
    if kind == "torch":      # does the loop find what the kernel finds (fp32 near-ties may part them)?
        variants["stateless_" + rest][0]()      # the kernel's outputs of this search, afresh (the buffers are shared)
        torch.cuda.synchronize()
        ko = variants["stateless_" + rest][2]
        B = rec["B"]
        if rec["search"] == "greedy":
            tk, cnt, tok = res.cpu().numpy(), ko["cnt"].cpu().numpy(), ko["tok"].reshape(-1)[:B * T].reshape(B, T).cpu().numpy()
            agree = sum(tk[tk[:, b] != BLANK, b].tolist() == tok[b, :cnt[b]].tolist() for b in range(B))
        else:
            ys, ln, _sc = (x.cpu().numpy() for x in res)
            tok, kl = ko["tok"].cpu().numpy(), ko["len"].cpu().numpy()
            agree = sum(ys[b, 0, :ln[b, 0]].tolist() == tok[b, 0, :kl[b, 0]].tolist() for b in range(B))
        extra = {"best_agreeing_with_kernel": f"{agree}/{B}"}
    else:
        per_frame = float(o["cnt"].float().mean()) if rec["search"] == "greedy" else float(o["len"][:, 0].float().mean())
        extra = {"emissions_per_frame": round(per_frame / T, 3)}
    med = statistics.median(ms[n])
    print(json.dumps({**rec, "T": T, "rounds": a.rounds, "ms": round(med, 3), "ms_min": round(min(ms[n]), 3),
                      "ms_max": round(max(ms[n]), 3), **extra,
                      "ratio_to_torch_loop": round(med / statistics.median(ms["torch_" + rest]), 3),
                      "ratio_to_lstm_handle": round(med / statistics.median(ms["lstm_" + rest]), 3)}), flush=True)
for d in decs.values():
    d.close()
