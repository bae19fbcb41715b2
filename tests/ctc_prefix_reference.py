"""float64 reference of the CTC prefix scorer (asr_ctc_prefix_begin / _score /
_advance; no device code), stated from the formulas in include/asr_amd.h with
np.logaddexp and loops over t, and the joint CTC / attention beam search on top
of attention_decode_reference.beam_search_ref.

A state is (rn [T_b][H], rb [T_b][H], psi [H], last [H]) for H hypotheses of ONE
utterance whose emissions are x [T_b][V] (log-softmax, float64)."""
import numpy as np

import attention_decode_reference as adref

NEG = -np.inf
np_quiet = np.errstate(invalid="ignore")         # logaddexp(-inf, -inf) and the NaN state of an empty slot


def begin(x, blank, H=1):
    Tb = x.shape[0]
    rb = np.repeat(np.cumsum(x[:, blank])[:, None], H, axis=1)
    return np.full((Tb, H), NEG), rb, np.zeros(H), np.full(H, -1)


@np_quiet
def score(x, state, blank, eos):
    """The deltas psi(g.c) - psi(g) [H][V]; a hypothesis with psi -inf gets a row of -inf."""
    rn, rb, psi, last = state
    Tb, V = x.shape
    both = np.logaddexp(rn, rb)
    same = np.arange(V)[None, :] == last[:, None]
    acc = np.where(last[:, None] < 0, x[0][None, :], NEG)
    for t in range(1, Tb):
        phi = np.where(same, rb[t - 1][:, None], both[t - 1][:, None])
        acc = np.logaddexp(acc, phi + x[t][None, :])
    acc[:, eos] = both[Tb - 1]
    acc[:, blank] = NEG
    d = acc - psi[:, None]
    d[psi == NEG] = NEG
    return d


@np_quiet
def advance(x, state, parent, token, blank, eos):
    """The state of the hypotheses (parent[h], token[h]); token eos passes the parent's state on."""
    rn, rb, psi, last = (a[..., np.asarray(parent)] for a in state)
    c = np.asarray(token)
    Tb, H = rn.shape
    cols = np.where(c == eos, blank, c)           # any valid column: the result is not used
    both, same, first = np.logaddexp(rn, rb), cols == last, last < 0
    nrn, nrb = np.full((Tb, H), NEG), np.full((Tb, H), NEG)
    nrn[0] = np.where(first, x[0, cols], NEG)
    npsi = nrn[0].copy()
    for t in range(1, Tb):
        phi = np.where(same, rb[t - 1], both[t - 1])
        nrn[t] = np.logaddexp(nrn[t - 1], phi) + x[t, cols]
        nrb[t] = np.logaddexp(nrn[t - 1], nrb[t - 1]) + x[t, blank]
        npsi = np.logaddexp(npsi, phi + x[t, cols])
    keep = c == eos
    return (np.where(keep, rn, nrn), np.where(keep, rb, nrb), np.where(keep, psi, npsi), np.where(keep, last, c))


def prefix_state(x, prefix, blank, eos):
    """The state of one hypothesis after the tokens of prefix."""
    st = begin(x, blank)
    for c in prefix:
        st = advance(x, st, [0], [c], blank, eos)
    return st


def log_softmax_emissions(T, B, V, seed, spread=3.0):
    """float32 [T][B][V] log-softmax of U(-spread, spread) logits."""
    z = np.random.default_rng(seed).uniform(-spread, spread, (T, B, V))
    return (z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(np.float32)


def joint_beam_search_ref(modules, memory, emis, enc_lengths, K, max_len, sos, eos, weight, blank, bonus=0.0):
    """adref.beam_search_ref with every candidate row (1 - weight) * attention
    log-prob + weight * CTC delta + bonus: the function is run as it is, on rows
    from a wrapped prefix_logp_ref.  Hypotheses that come out -inf (fewer than K
    candidates CTC can emit) are dropped, as the prune drops them."""
    att_rows = adref.prefix_logp_ref
    x = np.asarray(emis, np.float64)

    def joint_rows(mods, prefixes, utt, mem, enc, sos_):
        rows = att_rows(mods, prefixes, utt, mem, enc, sos_)
        for i, (g, b) in enumerate(zip(prefixes, utt)):
            xb = x[:enc[b], b]
            d = score(xb, prefix_state(xb, g, blank, eos), blank, eos)[0]
            with np.errstate(invalid="ignore"):
                rows[i] = np.where(d > NEG, (1.0 - weight) * rows[i] + weight * d + bonus, NEG)
        return rows

    adref.prefix_logp_ref = joint_rows
    try:
        with np.errstate(invalid="ignore"):
            out, worst = adref.beam_search_ref(modules, memory, enc_lengths, K, max_len, sos, eos)
    finally:
        adref.prefix_logp_ref = att_rows
    return [[h for h in u if h[1] > NEG] for u in out], worst


# The search cases on adref.SEARCH's model: (K, ctc_weight, length_bonus, max_len, seed), the seed the first of
# 0 .. 199 at which the float64 joint search keeps smallest gap / bound >= 2 (asserted again by the GPU test).  The
# model is adref.search_model(seed, 0.0), the emissions log_softmax_emissions(T, B, V, 700 + seed), blank 0.
SEARCH_CASES = [(1, 0.3, 0.0, 12, 0), (4, 0.3, 0.0, 12, 2), (1, 0.7, 0.0, 12, 0), (4, 0.7, 0.0, 12, 1),
                (4, 0.3, 0.4, 12, 2)]
