"""Shared fixtures of the LM-fused decoder's tests (test_ctc_lm_cpu.py,
test_ctc_lm_gpu.py): random models and emissions by fixed seeds, the label /
token mapping, the worked example and the comparison rules."""
import math

import numpy as np

from conftest import asr
from ctc_lm_reference import FusedSearch
from lm_reference import ArpaModel, random_arpa

TOL = 1e-9      # the project's score tolerance, relative to max(1, |x|)
MIN_GAP = 1e-6  # 1000 x TOL: below this gap a rank difference cannot be rounding


def close(x, y):
    if x == y:
        return True
    return abs(x - y) <= TOL * max(1.0, abs(y))


def assert_same_beams(got, ref, what=""):
    """Labels, ranks and n_tokens identical; total, ctc_logp, lm_log10 within TOL."""
    assert len(got) == len(ref), (what, len(got), len(ref))
    for b, (g, r) in enumerate(zip(got, ref)):
        assert [h[0] for h in g] == [list(h[0]) for h in r], (what, b)
        for k, (hg, hr) in enumerate(zip(g, r)):
            assert hg[4] == hr[4], (what, b, k, hg, hr)
            for i in (1, 2, 3):
                assert close(hg[i], hr[i]), (what, b, k, i, hg[i], hr[i])


def largest_difference(got, ref):
    """Largest |score - reference score| over total, ctc_logp and lm_log10 of
    beams that assert_same_beams would compare (a figure to report, no check)."""
    return max((abs(hg[i] - hr[i]) for g, r in zip(got, ref) for hg, hr in zip(g, r) for i in (1, 2, 3)
                if hg[i] != hr[i]), default=0.0)


def zero_out(logp, seed, fraction, blank):
    """logp [T][B][V] with `fraction` of the non-blank entries at -inf, chosen by
    a second generator: the first one's draws (model, emissions) stay as they are."""
    hit = np.random.default_rng([seed, 1]).random(logp.shape) < fraction
    hit[:, :, blank] = False
    return np.where(hit, -np.inf, logp)


class Case:
    """One randomised configuration: a random ARPA model over the tokens w0..,
    labels of which the last n_oov are no token of the model, emissions drawn
    from `seed`; `zero` is the fraction of the non-blank emissions set to
    probability 0 (-inf when is_log), drawn from a generator of its own."""

    def __init__(self, seed, T, B, V, beam, order=3, bos=True, eos=False, unk=False, n_oov=0, alpha=0.7, beta=0.3,
                 top_n=0, quant=0.0, blank=0, is_log=True, batch_major=False, lengths=None, codes=None,
                 max_states=0, sigma=2.0, zero=0.0):
        self.seed, self.T, self.B, self.V, self.beam, self.order = seed, T, B, V, beam, order
        self.bos, self.eos, self.alpha, self.beta, self.top_n = bos, eos, alpha, beta, top_n
        self.blank, self.is_log, self.batch_major, self.lengths = blank, is_log, batch_major, lengths
        self.codes, self.max_states = codes, max_states
        rng = np.random.default_rng(seed)
        vocab = V - 1 - n_oov
        ngrams = [min(3 * vocab, vocab ** k) for k in range(2, order + 1)]
        self.text = random_arpa(rng, vocab, order, ngrams, bos=True, eos=True, unk=unk)
        names = ["w%d" % i for i in range(vocab)] + ["oov%d" % i for i in range(n_oov)]
        self.labels = names[:blank] + [""] + names[blank:]
        logits = rng.normal(0.0, sigma, (T, B, V))
        logp = logits - np.log(np.exp(logits).sum(-1, keepdims=True))
        if quant:
            logp = np.round(logp / quant) * quant   # few distinct values: the label-id tie rule decides
        if zero:
            logp = zero_out(logp, seed, zero, blank)
        self.emis = (logp if is_log else np.exp(logp)).astype(np.float32)   # [T][B][V]

    def lm(self):
        return asr.NGramLM.from_string(self.text)

    def decoder(self, lm):
        return asr.CTCLMDecoder(self.V, self.beam, lm, lm.label_tokens(self.labels), self.alpha, self.beta,
                                blank_id=self.blank, bos=self.bos, eos=self.eos, top_n=self.top_n,
                                max_states=self.max_states, codes=self.codes)

    def feed(self):
        """The emissions as the decoders take them and the batch_major flag."""
        return (np.ascontiguousarray(self.emis.transpose(1, 0, 2)) if self.batch_major else self.emis)

    def reference(self):
        """([hyps per utterance], smallest gap) of the Python reference."""
        model = ArpaModel(self.text)
        tok = [model.ids.get(s, -1) if s != "" else -1 for s in self.labels]
        search = FusedSearch(model, self.V, self.beam, self.blank, tok, self.alpha, self.beta, bos=self.bos,
                             eos=self.eos, top_n=self.top_n, codes=self.codes)
        out, gap = [], math.inf
        for b in range(self.B):
            n = self.T if self.lengths is None else int(self.lengths[b])
            h, g = search.decode(self.emis[:n, b], self.is_log)
            out.append(h)
            gap = min(gap, g)
        return out, gap

    def host(self, dec):
        """(beams, smallest gap) of the host twin."""
        dec.decode_host(self.feed(), is_log=self.is_log, lengths=self.lengths, batch_major=self.batch_major)
        return dec.beams(256), float(dec.host_gaps().min())

    def device(self, dec):
        dec.decode(self.feed(), is_log=self.is_log, lengths=self.lengths, batch_major=self.batch_major)
        return dec.beams(256)


# Every seed below was chosen on the CPU so that the reference's smallest gap is
# >= MIN_GAP: a rank difference cannot then be rounding.
HOST_CASES = {
    "order1": dict(seed=101, T=10, B=2, V=6, beam=3, order=1),
    "order2": dict(seed=102, T=10, B=2, V=6, beam=3, order=2),
    "order3": dict(seed=103, T=10, B=2, V=6, beam=4, order=3),
    "order5": dict(seed=104, T=14, B=2, V=7, beam=4, order=5),
    "bos_off": dict(seed=105, T=8, B=2, V=6, beam=3, order=3, bos=False),
    "eos_on": dict(seed=106, T=8, B=2, V=6, beam=3, order=3, eos=True),
    "bos_off_eos_on": dict(seed=107, T=8, B=2, V=6, beam=3, order=2, bos=False, eos=True),
    "beta_pos": dict(seed=108, T=8, B=2, V=6, beam=3, order=3, beta=1.5),
    "beta_neg": dict(seed=109, T=8, B=2, V=6, beam=3, order=3, beta=-1.5),
    "oov_unk": dict(seed=110, T=8, B=2, V=7, beam=3, order=3, n_oov=2, unk=True),
    "oov_no_unk": dict(seed=111, T=8, B=2, V=7, beam=3, order=3, n_oov=2, unk=False),
    "top1": dict(seed=112, T=8, B=2, V=7, beam=3, order=3, top_n=1, quant=1.0),
    "top3": dict(seed=113, T=8, B=2, V=7, beam=3, order=3, top_n=3, quant=1.0),
    "top_all": dict(seed=114, T=8, B=2, V=7, beam=3, order=3, top_n=6, quant=1.0),
    "lengths": dict(seed=115, T=9, B=4, V=6, beam=3, order=3, lengths=[1, 9, 4, 2]),
    "batch_major": dict(seed=116, T=7, B=3, V=6, beam=3, order=3, batch_major=True, lengths=[7, 1, 5]),
    "probabilities": dict(seed=117, T=8, B=2, V=6, beam=3, order=3, is_log=False),
    "blank_last_codes": dict(seed=118, T=8, B=2, V=6, beam=3, order=3, blank=5, codes=[9, 3, 7, 1, 8, 4]),
    "beam_wider_than_states": dict(seed=119, T=3, B=1, V=4, beam=200, order=3),
}


# ---- every option at the widths where the kernel's paths change -----------------
def distinct_codes(n, seed):
    """n distinct symbol codes in a fixed random order, not 0 .. n-1."""
    return [int(x) for x in 3 * np.random.default_rng([seed, 2]).permutation(n) + 1]


def ragged_lengths(B, T, seed):
    """B lengths drawn in [1, T], the first T and the last 1."""
    n = np.random.default_rng([seed, 3]).integers(1, T + 1, B)
    n[0], n[-1] = T, 1
    return [int(x) for x in n]


# The smallest shapes that still span more than one wave of (state, label) pairs
# or sit on a limit, each with the options that decide how the kernel indexes by
# utterance, frame and lane.  Seeds chosen on the CPU with the reference alone,
# as above.
WIDE_OPTION_CASES = {
    # strides, lengths, codes, blank last, probabilities across the wave width
    "v65_strides_codes_blank_last": dict(seed=900, T=16, B=3, V=65, beam=8, blank=64, codes=distinct_codes(65, 900),
                                         lengths=[16, 1, 7], batch_major=True, is_log=False),
    # </s> on, <s> off, beta < 0, OOV labels without <unk>, wide beam
    "beam50_eos_no_bos_oov": dict(seed=904, T=40, B=3, V=29, beam=50, order=5, sigma=6.0, eos=True, bos=False,
                                  beta=-1.5, n_oov=3),
    "beam50_oov_unk_eos": dict(seed=904, T=40, B=3, V=29, beam=50, order=5, sigma=6.0, n_oov=3, unk=True, eos=True),
    # prefixes longer than the 7-token context: the window shifts
    "order8_long_prefixes": dict(seed=901, T=48, B=2, V=29, beam=20, order=8, sigma=8.0),
    # the label cutoff with strides, lengths, probabilities and quantised ties
    "v1000_top40_strides_quant": dict(seed=900, T=24, B=3, V=1000, beam=20, top_n=40, batch_major=True,
                                      lengths=[24, 5, 13], is_log=False, quant=0.5),
    "v256_255_candidates": dict(seed=900, T=6, B=2, V=256, beam=4),
    "v4096_top255": dict(seed=900, T=6, B=2, V=4096, beam=4, top_n=255, sigma=3.0),
    # zero probabilities: log(0) and the -inf keys of the select
    "zero_probabilities": dict(seed=900, T=24, B=4, V=29, beam=8, is_log=False, zero=0.3),
    "minus_inf_log_probabilities": dict(seed=900, T=24, B=4, V=29, beam=8, is_log=True, zero=0.3),
    # ragged lengths over more utterances than CUs, the blank in the middle
    "b300_ragged_blank_mid": dict(seed=900, T=8, B=300, V=6, beam=3, blank=3, lengths=ragged_lengths(300, 8, 900)),
    # the beam across the wave width with codes, the blank in the middle, </s>
    "beam64_codes_blank_mid_eos": dict(seed=900, T=16, B=2, V=12, beam=64, blank=5, codes=distinct_codes(12, 900),
                                       eos=True),
}

_WIDE = {}


def wide_reference(name):
    """(case, reference beams, gap) of a WIDE_OPTION_CASES entry, computed once per
    session and never modified, with what the entry needs of its reference
    checked: a gap >= MIN_GAP; order 8: a best hypothesis of more than 8 tokens;
    zeroed emissions: at least `beam` hypotheses of finite total per utterance."""
    if name not in _WIDE:
        c = Case(**WIDE_OPTION_CASES[name])
        ref, gap = c.reference()
        _WIDE[name] = (c, ref, gap)
    c, ref, gap = _WIDE[name]
    assert gap >= MIN_GAP, gap
    if c.order > 5:   # only then does the window shift (the 7-token context is full)
        assert all(u[0][4] > 8 for u in ref), [u[0][4] for u in ref]
    if WIDE_OPTION_CASES[name].get("zero"):
        assert not np.isfinite(c.emis).all() if c.is_log else (c.emis == 0).any()
        for u in ref:
            assert sum(math.isfinite(h[1]) for h in u) >= c.beam, len(u)
    return c, ref, gap


def batch_independence(dec, emis, row, n):
    """emis [T][6][V]: utterance `row` with n frames decoded alone, then as the
    first and as the last of the six, time-major and batch-major, the other
    rows with lengths of their own: bit-identical every time."""
    T = emis.shape[0]
    u = emis[:, row:row + 1]
    dec.decode(u, is_log=True, lengths=[n])
    alone = dec.beams(64)[0]
    assert len(alone) >= 2
    for at, others in ((0, [T, 1, 5, 3, T - 1]), (5, [2, T, 1, T - 2, 4])):
        batch = emis.copy()
        batch[:, at] = u[:, 0]
        lengths = others[:at] + [n] + others[at:]
        dec.decode(batch, is_log=True, lengths=lengths)
        assert dec.beams(64)[at] == alone   # bit-identical: labels, ranks and every fp64 score
        dec.decode(np.ascontiguousarray(batch.transpose(1, 0, 2)), is_log=True, lengths=lengths, batch_major=True)
        assert dec.beams(64)[at] == alone


# ---- the worked example: fusion keeps what the plain search pruned ------------
# Labels: 0 blank, 1 "a", 2 "b"; beam 1 (two states kept, ties aside); alpha 1,
# beta 0; <s> on, </s> off.  ln10 * log10 P is ln P, so W is a sum of ln P.
#   P(a | <s>) = 0.1 (-1)    P(b | <s>) = 0.8 (-0.09691)    P(a | b) = 0.9 (-0.045757)
# Frame 0 emits ($ .35, a .40, b .25), frame 1 ($ .20, a .70, b .10).
# Plain, frame 0: a .40 > $ .35 > b .25: "b" is pruned, and with it every
#   hypothesis that starts with b.  Frame 1: "a" = .40*.70 + .35*.70 = .525,
#   "a$" .08, "$" .07, "ab" .04, "b" .035: "a" and "a$" stay, the beam is ["a"].
#   No re-ranking of that beam can produce "ba".
# Fused, frame 0: "$" ln .35 = -1.050; "b" ln .25 + ln .8 = -1.609;
#   "a" ln .40 + ln .1 = -3.219: "a" is pruned.  Frame 1:
#   "ba" ln(.25*.70) + ln .8 + ln .9 = -1.743 - 0.223 - 0.105 = -2.071
#   "$"  ln .07 = -2.659
#   "b"  ln(.35*.10 + .25*.10) + ln .8 = -2.813 - 0.223 = -3.036
#   "b$" ln .05 + ln .8 = -3.219        "a" ln .245 + ln .1 = -3.709
#   "ba" and "$" stay; the best is "ba" with total -2.0715, ctc ln .175 = -1.7430,
#   lm_log10 -0.142667, two tokens.
WORKED_ARPA = """
\\data\\
ngram 1=4
ngram 2=3

\\1-grams:
-99\t<s>\t0
-1.5\t</s>
-0.5\ta\t0
-0.5\tb\t0

\\2-grams:
-1\t<s> a
-0.09691\t<s> b
-0.045757\tb a

\\end\\
"""
WORKED_LABELS = ["", "a", "b"]
WORKED_EMIS = np.array([[[0.35, 0.40, 0.25]], [[0.20, 0.70, 0.10]]], np.float32)   # [T=2][B=1][V=3]
WORKED_BEST = [2, 1]
WORKED_CTC = math.log(0.25 * 0.70)
WORKED_LM10 = -0.09691 + -0.045757
WORKED_TOTAL = WORKED_CTC + asr.LN10 * WORKED_LM10


def tie_case(V, beam, T, max_states=0):
    """Uniform emissions and equal unigram probabilities: whole classes of
    states tie at every prune."""
    names = ["w%d" % i for i in range(V - 1)]
    text = "\n\\data\\\nngram 1=%d\n\n\\1-grams:\n" % (V + 1)
    text += "-99\t<s>\n-1\t</s>\n" + "".join("-1\t%s\n" % n for n in names) + "\n\\end\\\n"
    emis = np.full((T, 1, V), 1.0 / V, np.float32)
    return text, [""] + names, emis
