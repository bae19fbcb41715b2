"""Time of the LM-fused transducer beam search (asr_rnnt_beam_lm) at §25's shape
(D = Hp = J = 640, V = 1025, E = 512, L = 1, T = 200, K = 4, B = 64 and 256) with
a random bigram ARPA model over the 1024 labels, against asr_rnnt_beam on the
same input and against the yardstick timed in the same process: §25's batched
torch loop with the LM added as a dense [V + 1][V] table (row: the hypothesis's
last label, the last row <s>) filled from the same model by asr_lm_score_host
and gathered per row.  A trigram model is timed through the kernel alone.
HIP events around each call, warm-up runs, then interleaved rounds (every
variant once per round); the median of the rounds.  One JSON line per variant
and batch size.
    python tools/rnnt_lm_bench.py [--B 64,256] [--T 200] [--beam 4] [--rounds 11] [--warmup 2]
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
from lm_reference import random_arpa  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--B", default="64,256")
ap.add_argument("--T", type=int, default=200)
ap.add_argument("--beam", type=int, default=4)
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--blank-bias", type=float, default=7.8)
ap.add_argument("--alpha", type=float, default=0.5)
ap.add_argument("--beta", type=float, default=0.5)
ap.add_argument("--ngrams", type=int, default=20000)
a = ap.parse_args()
if a.rounds < 10:
    sys.exit("--rounds: at least 10 timed runs")
T, K = a.T, a.beam
E = 512
D = Hp = J = 640
V, BLANK = 1025, 1024
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
dec = asr.TransducerDecoder(asr.rnnt_desc(V, BLANK, E, D, Hp, 1, J, "relu", 1), w)
dec.upload()
tw = {n: torch.from_numpy(v[0] if isinstance(v, list) else v).to(dev) for n, v in w.items()}
cell_b = tw["b_ih"] + tw["b_hh"]
NEG = float("-inf")

# the models: label v < 1024 is token "w<v>"
lms, fuses, tok = {}, {}, None
for name, order in (("bigram", 2), ("trigram", 3)):
    lm = asr.NGramLM.from_string(random_arpa(np.random.default_rng(order), V - 1, order, [a.ngrams] * (order - 1)))
    lm.upload()
    tok = np.array([lm.token_id("w%d" % v) for v in range(V - 1)] + [-1], np.int32)
    lms[name] = (lm, tok)
    fuses[name] = dec._lm_handle(lm, a.alpha, a.beta, tok, True, False)
# the dense table of the bigram: value of label v after label u (row V - 1: after <s>), by the host scorer
lm, tok = lms["bigram"]
pairs = np.stack([np.repeat(tok[:V - 1], V - 1), np.tile(tok[:V - 1], V - 1)], 1).astype(np.int32)
_lp, _cnt, vals, _ord = lm.score(pairs.tolist(), bos=False, eos=False, detail=True, host=True)
table = np.zeros((V, V), np.float64)
table[:V - 1, :V - 1] = np.array([v[1] for v in vals]).reshape(V - 1, V - 1)
_lp, _cnt, vals, _ord = lm.score([[int(t)] for t in tok[:V - 1]], bos=True, eos=False, detail=True, host=True)
table[V - 1, :V - 1] = np.array([v[0] for v in vals])
aln10 = float(np.float32(a.alpha)) * 2.302585092994046
addw = torch.from_numpy(table).to(dev) * aln10 + float(np.float32(a.beta))     # (aln10 * v) + beta, two roundings
addw[:, BLANK] = 0.0


def torch_cell(x, h, c):
    """torch.nn.LSTMCell's arithmetic on the library's [in][out] weights."""
    z = x @ tw["w_ih"] + h @ tw["w_hh"] + cell_b
    i, f, g, o = z.chunk(4, 1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c), c


def torch_beam(enc):
    """§25's loop with the bigram: every row carries W and its last label.  Returns (ys [B, K, T] padded with -1,
    lengths [B, K], totals [B, K] float64, -inf for a slot without a hypothesis), best first."""
    B = enc.shape[1]
    F = (enc.reshape(T * B, E) @ tw["w_enc"] + tw["b_enc"]).reshape(T, B, J)
    h, c = torch_cell(tw["emb"][BLANK].expand(B * K, D), torch.zeros(B * K, Hp, device=dev),
                      torch.zeros(B * K, Hp, device=dev))
    g = h @ tw["w_pred"] + tw["b_pred"]
    score = torch.full((B, K), NEG, dtype=torch.float64, device=dev)
    score[:, 0] = 0.0
    W = torch.zeros((B, K), dtype=torch.float64, device=dev)
    last = torch.full((B, K), V - 1, dtype=torch.int64, device=dev)
    ys = torch.full((B, K, T + 1), -1, dtype=torch.int64, device=dev)
    ln = torch.zeros((B, K), dtype=torch.int64, device=dev)
    hsh = torch.zeros((B, K), dtype=torch.int64, device=dev)
    rows = torch.arange(B, device=dev).unsqueeze(1)
    upper = torch.triu(torch.ones(K, K, dtype=torch.bool, device=dev))
    strict = torch.triu(torch.ones(K, K, dtype=torch.bool, device=dev), 1)
    for t in range(T):
        logit = torch.relu(F[t].repeat_interleave(K, 0) + g) @ tw["w_out"] + tw["b_out"]
        lp = (logit - torch.logsumexp(logit, 1, keepdim=True)).reshape(B, K, V)
        ac = score.unsqueeze(2) + lp.double()
        wt = W.unsqueeze(2) + addw[last]                      # [B, K, V]: W at the blank
        top, idx = (ac + wt).reshape(B, K * V).topk(K, dim=1)
        acs, Wn = ac.reshape(B, K * V).gather(1, idx), wt.reshape(B, K * V).gather(1, idx)
        par, tk = idx // V, idx % V
        emit = tk != BLANK
        ys, ln, hsh, last = ys[rows, par], ln[rows, par], hsh[rows, par], last[rows, par]
        ys.scatter_(2, torch.where(emit, ln, T).unsqueeze(2), tk.unsqueeze(2))
        ln = ln + emit
        hsh = torch.where(emit, hsh * 1000003 + tk + 1, hsh)
        last = torch.where(emit, tk, last)
        live = top > NEG
        eq = (hsh.unsqueeze(2) == hsh.unsqueeze(1)) & (ln.unsqueeze(2) == ln.unsqueeze(1)) & \
            live.unsqueeze(2) & live.unsqueeze(1)
        merged = torch.logsumexp(torch.where(eq & upper, acs.unsqueeze(1).expand(B, K, K), NEG), dim=2)
        dead = (eq & strict).any(1)
        merged = torch.where(dead | ~live, NEG, merged)
        _f, order = (merged + Wn).sort(dim=1, descending=True, stable=True)
        score, W = merged[rows, order], Wn[rows, order]
        ys, ln, hsh, last = ys[rows, order], ln[rows, order], hsh[rows, order], last[rows, order]
        par, tk, emit = par[rows, order], tk[rows, order], emit[rows, order]
        src = (rows * K + par).reshape(-1)
        h0, c0 = h[src], c[src]
        h2, c2 = torch_cell(tw["emb"][tk.reshape(-1)], h0, c0)
        m = emit.reshape(-1, 1)
        h, c = torch.where(m, h2, h0), torch.where(m, c2, c0)
        g = h @ tw["w_pred"] + tw["b_pred"]
    return ys, ln, score + W


variants, keep = {}, []
for B in (int(v) for v in a.B.split(",")):
    enc = (torch.rand((T, B, E), generator=gen) * 2 - 1).to(dev)
    need = max(dec.beam_lm_workspace_bytes(z, T, B, K) for z in fuses.values())
    out = {"tok": torch.zeros((B, K, T), dtype=torch.int32, device=dev),
           "ts": torch.zeros((B, K, T), dtype=torch.int32, device=dev),
           "len": torch.zeros((B, K), dtype=torch.int32, device=dev),
           "score": torch.zeros((B, K), dtype=torch.float64, device=dev),
           "nhyp": torch.zeros(B, dtype=torch.int32, device=dev),
           "work": torch.empty(need // 4 + 4, device=dev)}
    keep.append((enc, out))

    def plain(enc=enc, out=out, B=B):
        dec.beam_search_device(enc.data_ptr(), T, B, K, K, T, out["tok"].data_ptr(), out["ts"].data_ptr(),
                               out["len"].data_ptr(), out["score"].data_ptr(), out["nhyp"].data_ptr(),
                               out["work"].data_ptr(), stream=st.cuda_stream)

    def fused(name, enc=enc, out=out, B=B):
        dec.beam_search_lm_device(fuses[name], enc.data_ptr(), T, B, K, K, T, out["tok"].data_ptr(), out["ts"].data_ptr(),
                                  out["len"].data_ptr(), out["score"].data_ptr(), out["nhyp"].data_ptr(),
                                  out["work"].data_ptr(), stream=st.cuda_stream)

    def loop(enc=enc):
        with torch.cuda.stream(st):
            return torch_beam(enc)

    variants[f"plain_B{B}"] = (plain, {"search": "asr_rnnt_beam", "B": B})
    variants[f"bigram_B{B}"] = (lambda f=fused: f("bigram"), {"search": "asr_rnnt_beam_lm, bigram", "B": B})
    variants[f"trigram_B{B}"] = (lambda f=fused: f("trigram"), {"search": "asr_rnnt_beam_lm, trigram", "B": B})
    variants[f"torch_B{B}"] = (loop, {"search": "torch loop with the dense bigram table", "B": B})

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
    variants[f"bigram_B{B}"][0]()
    ys, ln, score = variants[f"torch_B{B}"][0]()
    torch.cuda.synchronize()
    tk, hl, nh, sc = out["tok"].cpu().numpy(), out["len"].cpu().numpy(), out["nhyp"].cpu().numpy(), out["score"].cpu().numpy()
    ys, ln, score = ys.cpu().numpy(), ln.cpu().numpy(), score.cpu().numpy()
    agree, worst = 0, 0.0
    for b in range(B):
        mine = [tk[b, j, :hl[b, j]].tolist() for j in range(nh[b])]
        theirs = [ys[b, j, :ln[b, j]].tolist() for j in range(K) if np.isfinite(score[b, j])]
        if mine == theirs:
            agree += 1
            worst = max([worst] + [abs(sc[b, j] - score[b, j]) / (1 + abs(score[b, j])) for j in range(nh[b])])
    for kind in ("plain", "bigram", "trigram", "torch"):
        n = f"{kind}_B{B}"
        med = statistics.median(ms[n])
        print(json.dumps({**variants[n][1], "T": T, "K": K, "rounds": a.rounds, "ms": round(med, 3),
                          "ms_min": round(min(ms[n]), 3), "us_per_frame": round(1e3 * med / T, 2),
                          "ratio_to_torch_loop": round(med / statistics.median(ms[f"torch_B{B}"]), 3),
                          "ratio_to_asr_rnnt_beam": round(med / statistics.median(ms[f"plain_B{B}"]), 3),
                          "tokens_in_bigram_best": round(float(hl[:, 0].mean()), 1),
                          "utterances_with_bigram_nbest_agreeing_with_torch": f"{agree}/{B}",
                          "max_rel_total_diff_where_agreeing": float(f"{worst:.3e}")}), flush=True)
dec.close()
