"""float64 references for attention-decoder beam search (no device code), shared
by test_attention_decode_cpu.py and test_attention_decode_gpu.py:

- decode_attention_ref: asr_decode_attention_fwd in numpy, one query per
  hypothesis over keys named by a column table (the ancestry) or one column;
- beam_step_ref: the prune rule of asr_attn_beam_step in plain numpy;
- CachedDecoderRef: a float64 decoder that steps on a K/V cache through an
  ancestry table (the formulation the device code uses), from the weights of
  attention_decoder_reference.make_decoder's torch modules;
- beam_search_ref: a full beam search that recomputes the whole prefix of every
  hypothesis at every step with attention_decoder_reference.decoder_ref (no
  cache), with the smallest margin it met;
- the shapes, draws and seeds of the GPU cases."""
import numpy as np
import torch

import attention_decoder_reference as adr

ATOL = adr.ATOL


# ---------------------------------------------------------------- the kernel
# (heads, head_dim): one case per head_dim the issue names; Tk: one key, the block edge, a third block of 2.
DATTN_DIMS = [(2, 4), (2, 16), (2, 20), (2, 36), (2, 64), (1, 128)]
DATTN_TK = [1, 63, 64, 65, 130]
DATTN_N, DATTN_S = 7, 3


def dattn_lengths(Tk):
    """Ragged lengths of the N = 7 hypotheses with 0 and Tk."""
    return np.array([Tk, 0, max(Tk - 3, 1), 1, Tk, (Tk + 1) // 2, min(Tk, 64)], np.int32)


def draw_decode(heads, head_dim, Tk, N=DATTN_N, S=DATTN_S, seed=0):
    """q [N][E], k, v [Tk][S][E] float32 U(+-1), a random table [Tk][N] and one column per hypothesis [N]."""
    E = heads * head_dim
    rng = np.random.default_rng(100000 * head_dim + 1000 * heads + 10 * Tk + N + seed)
    return (rng.uniform(-1, 1, (N, E)).astype(np.float32), rng.uniform(-1, 1, (Tk, S, E)).astype(np.float32),
            rng.uniform(-1, 1, (Tk, S, E)).astype(np.float32), rng.integers(0, S, (Tk, N)).astype(np.int32),
            rng.integers(0, S, N).astype(np.int32))


def nan_unnamed(x, table, lengths):
    """x [Tk][S][E] with NaN in every (j, column) that no live (j, n) of table [Tk][N] names."""
    Tk, S, _ = x.shape
    named = np.zeros((Tk, S), bool)
    for n, ln in enumerate(lengths):
        j = np.arange(min(max(int(ln), 0), Tk))
        named[j, table[j, n]] = True
    x = x.copy()
    x[~named] = np.nan
    return x


def decode_attention_ref(q, k, v, heads, cols, lengths=None, scale=0.0):
    """out [N][E] float64: hypothesis n attends to keys j < lengths[n], key j
    being k[j, cols[j, n]] (cols [Tk][N]) or k[j, cols[n]] (cols [N]); a row
    with no key is zeros."""
    q = np.asarray(q, np.float64)
    N, E = q.shape
    Tk = k.shape[0]
    D = E // heads
    sc = scale if scale else 1.0 / np.sqrt(D)
    cols = np.asarray(cols)
    if cols.ndim == 1:
        cols = np.broadcast_to(cols[None, :], (Tk, N))
    out = np.zeros((N, E))
    for n in range(N):
        nk = Tk if lengths is None else min(max(int(lengths[n]), 0), Tk)
        if nk == 0:
            continue
        j = np.arange(nk)
        kk, vv = np.asarray(k[j, cols[j, n]], np.float64), np.asarray(v[j, cols[j, n]], np.float64)
        for h in range(heads):
            sl = slice(h * D, (h + 1) * D)
            s = kk[:, sl] @ q[n, sl] * sc
            pr = np.exp(s - s.max())
            out[n, sl] = (pr / pr.sum()) @ vv[:, sl]
    return out


# ------------------------------------------------------------ the beam step
def beam_step_ref(logp, scores, finished, tokens_in, anc_in, B, K, V, max_len, step, eos):
    """(scores, finished, parent, token, tokens_out, anc_out, live) of one
    prune: per utterance every candidate (a live unfinished slot: V tokens,
    score + float64(logp); a finished slot: itself with eos; an empty slot:
    none; -inf sums dropped) sorted by score descending, parent ascending,
    token ascending; the first K kept.  The out tables start as copies."""
    N = B * K
    so, fo = np.full(N, -np.inf), np.zeros(N, np.int32)
    par, tok = np.arange(N, dtype=np.int32), np.full(N, eos, np.int32)
    tout, aout = np.array(tokens_in, np.int32), np.array(anc_in, np.int32)
    live = 0
    for b in range(B):
        cand = []
        for k in range(K):
            n = b * K + k
            if not scores[n] > -np.inf:
                continue
            if finished[n]:
                cand.append((-scores[n], k, eos, scores[n]))
                continue
            for v in range(V):
                x = np.float64(scores[n]) + np.float64(logp[n, v])
                if x > -np.inf:
                    cand.append((-x, k, v, x))
        cand.sort(key=lambda c: c[:3])
        for k, (_, pk, v, x) in enumerate(cand[:K]):
            n = b * K + k
            so[n], par[n], tok[n] = x, b * K + pk, v
            fo[n] = int(bool(finished[b * K + pk]) or v == eos)
            live += not fo[n]
    tout[:step] = np.asarray(tokens_in)[:step][:, par]
    tout[step] = tok
    aout[:step + 1] = np.asarray(anc_in)[:step + 1][:, par]
    if step + 1 < max_len:
        aout[step + 1] = np.arange(N)
    return so, fo, par, tok, tout, aout, live


# The prune cases of both test files: (name, V, K); B = 3 always.
BEAM_SHAPES = [(5, 1), (5, 4), (70, 4), (70, 16), (1000, 1), (1000, 16), (5, 16)]
BEAM_B, BEAM_MAX_LEN = 3, 6


def beam_case(kind, V, K, seed=0):
    """(logp [N][V] float32, scores, finished, tokens_in, anc_in, step) of one named case."""
    B, L, N = BEAM_B, BEAM_MAX_LEN, BEAM_B * K
    rng = np.random.default_rng(1000 * V + 10 * K + seed + sum(map(ord, kind)))
    logits = rng.uniform(-3, 3, (N, V))
    logp = (logits - np.log(np.exp(logits).sum(1, keepdims=True))).astype(np.float32)
    scores, fin = -rng.uniform(0, 5, N), np.zeros(N, np.int32)
    step = 3
    if kind == "step0":                          # one live slot per utterance
        scores[:] = -np.inf
        scores[::K] = 0.0
        step = 0
    elif kind == "all_finished":                 # utterance 1 has ended in every slot
        fin[K:2 * K] = 1
    elif kind == "mixed":                        # finished and live slots side by side, one empty
        fin[rng.random(N) < 0.4] = 1
        scores[N - 1] = -np.inf
    elif kind == "neg_inf":                      # empty slots and -inf log-probs
        scores[rng.random(N) < 0.5] = -np.inf
        logp[rng.random((N, V)) < 0.3] = -np.inf
        logp[0] = -np.inf                        # a live slot none of whose candidates survives
    elif kind == "ties_tokens":                  # equal logp across tokens: the token rule
        logp[:] = np.float32(-1.5)
        scores[:] = -np.arange(N) % 2            # and equal sums across parents
    elif kind == "ties_parents":                 # equal sums across parents: the parent rule
        logp[:] = np.round(logp * 2) / 2         # a grid of halves: sums are exact
        scores[:] = -np.round(rng.uniform(0, 3, N) * 2) / 2
    elif kind == "few":                          # fewer than K candidates in utterance 0 and none in utterance 2
        scores[1:K] = -np.inf
        fin[0] = 1
        scores[2 * K:] = -np.inf
    else:
        assert kind == "random", kind
    tokens_in = rng.integers(0, V, (L, N)).astype(np.int32)
    anc_in = ((np.arange(N) // K) * K + rng.integers(0, K, (L, N))).astype(np.int32)
    return logp, scores, fin, tokens_in, anc_in, step


BEAM_KINDS = ["random", "step0", "all_finished", "mixed", "neg_inf", "ties_tokens", "ties_parents", "few"]


# ------------------------------------------- the decoder, stepping on a cache
def _ln(x, m):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + m.eps) * m.weight.detach().double().numpy() + m.bias.detach().double().numpy()


class CachedDecoderRef:
    """The float64 decoder of make_decoder's modules, one step at a time on a
    K/V cache read through an ancestry table: slot n = b*K + k of N = B*K."""

    def __init__(self, emb, dec, out, memory, enc_lengths, K, max_len):
        w = lambda p: p.detach().double().numpy()   # noqa: E731
        self.emb, self.dec, self.out = w(emb.weight), dec, (w(out.weight), w(out.bias))
        T, B, E = memory.shape
        self.E, self.N, self.K, self.s = E, B * K, K, 0
        self.heads = dec.layers[0].self_attn.num_heads
        self.pe = adr.positional_encoding(max_len, E).numpy()
        self.cols = np.repeat(np.arange(B), K)
        self.klen = np.repeat(np.asarray(enc_lengths), K)
        self.anc = np.tile(np.arange(self.N), (max_len, 1))
        self.kc = [np.zeros((max_len, self.N, E)) for _ in dec.layers]
        self.vc = [np.zeros((max_len, self.N, E)) for _ in dec.layers]
        mem = np.asarray(memory, np.float64)
        self.mk, self.mv = [], []
        for l in dec.layers:
            wi, bi = w(l.multihead_attn.in_proj_weight), w(l.multihead_attn.in_proj_bias)
            self.mk.append(mem @ wi[E:2 * E].T + bi[E:2 * E])
            self.mv.append(mem @ wi[2 * E:].T + bi[2 * E:])

    def reorder(self, parents):
        """Slot n continues slot parents[n]: rows 0 .. s - 1 of the table are permuted, the cache is not."""
        self.anc[:self.s] = self.anc[:self.s, parents]

    def step(self, tokens):
        """log-probs [N][V] float64 for the input tokens [N] of step s."""
        w = lambda p: p.detach().double().numpy()   # noqa: E731
        s, E = self.s, self.E
        x = self.emb[np.asarray(tokens)] * np.sqrt(E) + self.pe[s]
        for li, l in enumerate(self.dec.layers):
            def own(z):
                wi, bi = w(l.self_attn.in_proj_weight), w(l.self_attn.in_proj_bias)
                qkv = z @ wi.T + bi
                self.kc[li][s], self.vc[li][s] = qkv[:, E:2 * E], qkv[:, 2 * E:]
                ctx = decode_attention_ref(qkv[:, :E], self.kc[li][:s + 1], self.vc[li][:s + 1], self.heads,
                                           self.anc[:s + 1])
                return ctx @ w(l.self_attn.out_proj.weight).T + w(l.self_attn.out_proj.bias)

            def cross(z):
                wi, bi = w(l.multihead_attn.in_proj_weight), w(l.multihead_attn.in_proj_bias)
                ctx = decode_attention_ref(z @ wi[:E].T + bi[:E], self.mk[li], self.mv[li], self.heads, self.cols,
                                           self.klen)
                return ctx @ w(l.multihead_attn.out_proj.weight).T + w(l.multihead_attn.out_proj.bias)

            ff = lambda z: (np.maximum(z @ w(l.linear1.weight).T + w(l.linear1.bias), 0) @ w(l.linear2.weight).T   # noqa: E731
                            + w(l.linear2.bias))
            if l.norm_first:
                h = x + own(_ln(x, l.norm1))
                h2 = h + cross(_ln(h, l.norm2))
                x = h2 + ff(_ln(h2, l.norm3))
            else:
                h = _ln(x + own(x), l.norm1)
                h2 = _ln(h + cross(h), l.norm2)
                x = _ln(h2 + ff(h2), l.norm3)
        if self.dec.norm is not None:
            x = _ln(x, self.dec.norm)
        z = x @ self.out[0].T + self.out[1]
        self.s = s + 1
        z = z - z.max(1, keepdims=True)
        return z - np.log(np.exp(z).sum(1, keepdims=True))


def prefix_logp_ref(modules, prefixes, utt, memory, enc_lengths, sos):
    """float64 log-probs [N][V] after the last token of each prefix (sos + prefix), recomputed from scratch with
    decoder_ref; utt non-decreasing."""
    eos = 0                                        # the padding token: its rows are never read
    tin, tgt, ln = adr.teacher_forcing(prefixes, sos, eos)
    logp, _ = adr.decoder_ref(*modules, tin, tgt, ln, utt, memory, enc_lengths)
    return np.stack([logp[len(p), n] for n, p in enumerate(prefixes)])


# --------------------------------------------------- the recompute beam search
def beam_search_ref(modules, memory, enc_lengths, K, max_len, sos, eos):
    """(results, worst): per utterance [(tokens, score)] score descending, by a
    float64 search that recomputes every live prefix at every step, and the
    smallest (gap / bound) it met: at every step and utterance the gap between
    the K-th kept candidate and the best one dropped, and at the end the gaps
    between neighbouring results, each over score_bound of the terms summed so
    far.  Every utterance needs at least one frame."""
    T, B, E = memory.shape
    beams = [[([], 0.0, False)] for _ in range(B)]
    worst = np.inf
    for s in range(max_len):
        live = [(b, i) for b in range(B) for i, h in enumerate(beams[b]) if not h[2]]
        if not live:
            break
        lp = prefix_logp_ref(modules, [beams[b][i][0] for b, i in live], [b for b, _ in live], memory, enc_lengths,
                             sos)
        rows = {bi: lp[j] for j, bi in enumerate(live)}
        for b in range(B):
            cand = []
            for i, (y, sc, fin) in enumerate(beams[b]):
                if fin:
                    cand.append((-sc, i, eos, y, sc, True))
                else:
                    cand += [(-(sc + rows[(b, i)][v]), i, v, y + [v], sc + rows[(b, i)][v], v == eos)
                             for v in range(len(rows[(b, i)]))]
            cand.sort(key=lambda c: c[:3])
            if len(cand) > K:
                gap = cand[K - 1][4] - cand[K][4]
                worst = min(worst, gap / np.max(adr.score_bound(s + 1, np.array([cand[K - 1][4], cand[K][4]]))))
            beams[b] = [(c[3], c[4], c[5]) for c in cand[:K]]
    out = []
    for b in range(B):
        rows = sorted(beams[b], key=lambda h: -h[1])
        for a, c in zip(rows[:-1], rows[1:]):
            worst = min(worst, (a[1] - c[1]) / np.max(adr.score_bound(max(len(a[0]), len(c[0])),
                                                                       np.array([a[1], c[1]]))))
        out.append([([t for t in y if t != eos] if fin else list(y), sc) for y, sc, fin in rows])
    return out, worst


# The search cases: decoder E = 32, 2 heads, F = 64, 2 layers, V = 11 (sos = eos = 10), B = 3, T = 70.
SEARCH = dict(E=32, heads=2, F=64, layers=2, V=11, B=3, T=70, enc_lengths=(70, 33, 5))
# (K, eos bias, max_len, seed): the seed is the first of 0 .. 199 at which the float64 search keeps
# smallest gap / bound >= 2 (test_attention_decode_cpu.py asserts it again, on the references alone).
SEARCH_CASES = [(1, 0.0, 12, 0), (4, 0.0, 24, 1), (16, 0.0, 10, 8), (4, 0.5, 16, 1), (4, -6.0, 24, 53)]


def search_model(seed, eos_bias, norm_first=True):
    """(memory [T][B][E] float32, (embedding, decoder, output)) of a search case."""
    c = SEARCH
    emb, dec, out = adr.make_decoder(norm_first, seed=300 + seed, E=c["E"], heads=c["heads"], F=c["F"],
                                     layers=c["layers"], V=c["V"])
    with torch.no_grad():
        out.bias[c["V"] - 1] += eos_bias
    return adr.draw_memory(c["T"], c["B"], c["E"], seed=500 + seed), (emb, dec, out)
