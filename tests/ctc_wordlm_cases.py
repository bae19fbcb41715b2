"""Shared fixtures of the word-mode tests of the LM-fused decoder
(test_ctc_wordlm_cpu.py, test_ctc_wordlm_gpu.py): random lexicons, word-level
models and emissions by fixed seeds, and the worked example of DESIGN §23.  The
comparison rules are ctc_lm_cases' (assert_same_beams, close, MIN_GAP)."""
import math
import re

import numpy as np

from conftest import asr
from ctc_lm_cases import MIN_GAP, zero_out
from ctc_wordlm_reference import WordFusedSearch
from lm_reference import ArpaModel, random_arpa


def letter(i, V):
    """The string of letter i (label i + 1): a.. for the small alphabets."""
    return chr(ord("a") + i) if V <= 28 else chr(0x100 + i)


class WordCase:
    """One randomised configuration.  Labels: 0 the blank (""), 1 .. V-2 letters,
    V-1 the space.  The lexicon is n_words distinct random spellings of 1 ..
    max_word letters (or `words`, strings), the model a random ARPA model whose
    tokens are those spellings, the emissions drawn from `seed`; `peak` =
    (labels per frame, logit bonus) pushes one label per frame; `oov` is the
    model's oov_log10; n_letters limits the random spellings to the first
    letters and `boost` raises those letters' and the space's logits; `zero` is
    the fraction of the non-blank emissions set to probability 0 (-inf when
    is_log), drawn from a generator of its own."""

    def __init__(self, seed, T, B, V, beam, n_words=6, max_word=3, order=3, bos=True, eos=False, unk=False,
                 alpha=0.7, beta=0.3, top_n=0, quant=0.0, is_log=True, batch_major=False, lengths=None, closed=False,
                 max_states=0, sigma=2.0, words=None, peak=None, oov=-100.0, n_letters=0,
                 boost=0.0, zero=0.0):
        self.seed, self.T, self.B, self.V, self.beam, self.order = seed, T, B, V, beam, order
        self.bos, self.eos, self.alpha, self.beta, self.top_n = bos, eos, alpha, beta, top_n
        self.is_log, self.batch_major, self.lengths = is_log, batch_major, lengths
        self.closed, self.max_states, self.blank, self.space, self.oov = closed, max_states, 0, V - 1, oov
        rng = np.random.default_rng(seed)
        nl = V - 2
        used = n_letters or nl   # the letters the random spellings draw from
        self.labels = [""] + [letter(i, V) for i in range(nl)] + [" "]
        if words is None:
            got = set()
            while len(got) < n_words:
                got.add(tuple(int(x) for x in rng.integers(0, used, int(rng.integers(1, max_word + 1)))))
            spell = sorted(got, key=lambda w: rng.random())
            words = ["".join(letter(i, V) for i in w) for w in spell]
        self.words = list(words)
        vocab = len(self.words)
        ngrams = [min(3 * vocab, vocab ** k) for k in range(2, order + 1)]
        text = random_arpa(rng, vocab, order, ngrams, bos=True, eos=True, unk=unk)
        self.text = re.sub(r"\bw(\d+)\b", lambda m: self.words[int(m.group(1))], text)
        logits = rng.normal(0.0, sigma, (T, B, V))
        if boost:   # a large alphabet: the lexicon's letters and the space stand out
            logits[:, :, 1:used + 1] += boost
            logits[:, :, V - 1] += boost
        if peak is not None:
            which, bonus = peak
            for t in range(T):
                logits[t, :, which[t]] += bonus
        logp = logits - np.log(np.exp(logits).sum(-1, keepdims=True))
        if quant:
            logp = np.round(logp / quant) * quant   # few distinct values: the label-id tie rule decides
        if zero:
            logp = zero_out(logp, seed, zero, 0)
        self.emis = (logp if is_log else np.exp(logp)).astype(np.float32)   # [T][B][V]

    def lm(self):
        return asr.NGramLM.from_string(self.text, self.oov)

    def lexicon(self, lm):
        return asr.Lexicon.from_lm(lm, self.labels)

    def decoder(self, lm, lex):
        return asr.CTCLMDecoder.word(self.V, self.beam, lm, lex, self.alpha, self.beta, blank_id=self.blank,
                                     bos=self.bos, eos=self.eos, top_n=self.top_n, closed=self.closed,
                                     max_states=self.max_states)

    def feed(self):
        return np.ascontiguousarray(self.emis.transpose(1, 0, 2)) if self.batch_major else self.emis

    def spellings(self, ids):
        """{spelling in label ids: token id} of the words, ids a token -> id map."""
        index = {s: i for i, s in enumerate(self.labels)}
        return {tuple(index[ch] for ch in w): ids[w] for w in self.words}

    def search(self):
        model = ArpaModel(self.text)
        return WordFusedSearch(model, self.V, self.beam, self.blank, self.space, self.spellings(model.ids), self.alpha,
                               self.beta, bos=self.bos, eos=self.eos, top_n=self.top_n, closed=self.closed,
                               oov_log10=self.oov)

    def reference(self):
        """([hyps per utterance], smallest gap) of the Python reference."""
        search = self.search()
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
    "order1": dict(seed=1, T=10, B=2, V=5, beam=3, order=1),
    "order2": dict(seed=2, T=10, B=2, V=5, beam=3, order=2),
    "order3": dict(seed=3, T=10, B=2, V=5, beam=4, order=3),
    "order5": dict(seed=4, T=14, B=2, V=6, beam=4, order=5, n_words=8),
    "order3_closed": dict(seed=5, T=10, B=2, V=5, beam=4, order=3, closed=True),
    "order5_closed": dict(seed=6, T=14, B=2, V=6, beam=4, order=5, n_words=8, closed=True),
    "bos_off": dict(seed=7, T=8, B=2, V=5, beam=3, bos=False),
    "eos_on": dict(seed=8, T=8, B=2, V=5, beam=3, eos=True),
    "bos_off_eos_on_closed": dict(seed=9, T=8, B=2, V=5, beam=3, order=2, bos=False, eos=True, closed=True),
    "beta_pos": dict(seed=10, T=8, B=2, V=5, beam=3, beta=1.5),
    "beta_neg": dict(seed=11, T=8, B=2, V=5, beam=3, beta=-1.5),
    "beta_neg_closed": dict(seed=12, T=8, B=2, V=5, beam=3, beta=-1.5, closed=True),
    "unk": dict(seed=13, T=8, B=2, V=5, beam=3, unk=True),
    "unk_closed": dict(seed=14, T=8, B=2, V=5, beam=3, unk=True, closed=True),
    "top1": dict(seed=15, T=8, B=2, V=6, beam=3, top_n=1, quant=1.0),
    "top3": dict(seed=16, T=8, B=2, V=6, beam=3, top_n=3, quant=1.0),
    "top3_closed": dict(seed=17, T=8, B=2, V=6, beam=3, top_n=3, quant=1.0, closed=True),
    "top_all": dict(seed=18, T=8, B=2, V=6, beam=3, top_n=5, quant=1.0),
    "lengths": dict(seed=19, T=9, B=4, V=5, beam=3, lengths=[1, 9, 4, 2]),
    "lengths_closed": dict(seed=20, T=9, B=4, V=5, beam=3, lengths=[1, 9, 4, 2], closed=True),
    "batch_major": dict(seed=21, T=7, B=3, V=5, beam=3, batch_major=True, lengths=[7, 1, 5]),
    "probabilities": dict(seed=22, T=8, B=2, V=5, beam=3, is_log=False),
    "probabilities_closed": dict(seed=23, T=8, B=2, V=5, beam=3, is_log=False, closed=True),
    # letter / space alternation pushed by the emissions: 9 words and more, so the 7-token window shifts
    "nine_words": dict(seed=24, T=18, B=2, V=5, beam=4, order=5, n_words=3, max_word=1,
                       peak=([1, 4, 2, 4, 3, 4, 1, 4, 1, 4, 2, 4, 3, 4, 2, 4, 1, 4], 12.0)),
    "nine_words_closed": dict(seed=25, T=20, B=2, V=5, beam=4, order=5, n_words=3, max_word=1, closed=True, eos=True,
                              peak=([1, 4, 2, 4, 3, 4, 1, 4, 1, 4, 2, 4, 3, 4, 2, 4, 1, 4, 3, 0], 12.0)),
}


# ---- every option at the widths where the kernel's paths change -----------------
# Both lexicon modes between them; seeds chosen on the CPU with the reference
# alone, as above.
WIDE_OPTION_CASES = {
    # closed, </s> on, <s> off, lengths, wide beam
    "beam50_closed_eos_no_bos_lengths": dict(seed=900, T=48, B=3, V=29, beam=50, order=5, sigma=8.0, n_words=200,
                                             max_word=3, n_letters=12, closed=True, eos=True, bos=False,
                                             lengths=[48, 3, 20]),
    # open, <unk>, beta < 0, strides, probabilities
    "beam50_open_unk_strides": dict(seed=900, T=40, B=3, V=29, beam=50, order=5, sigma=8.0, n_words=200, max_word=3,
                                    n_letters=12, oov=-4.0, unk=True, batch_major=True, is_log=False, beta=-1.5),
    # open, the label cutoff, strides and lengths at V = 1000
    "v1000_top40_open_strides": dict(seed=900, T=24, B=3, V=1000, beam=20, top_n=40, n_words=200, max_word=3,
                                     n_letters=28, boost=6.0, oov=-4.0, batch_major=True, lengths=[24, 5, 13]),
    # many short words: more than 8 are scored, the window shifts.  The word bonus is what makes them many:
    # at the default beta the best hypotheses of 200 seeds had 1 to 4 words, the LM cost of a word being what it is
    "order8_short_words": dict(seed=900, T=40, B=2, V=8, beam=20, order=8, n_words=20, max_word=2, n_letters=4,
                               sigma=4.0, boost=2.0, oov=-4.0, beta=6.0),
    # zero probabilities: log(0) and the -inf keys of the select
    "zero_probabilities_closed": dict(seed=910, T=40, B=8, V=29, beam=8, n_words=60, max_word=4, n_letters=8,
                                      closed=True, is_log=False, zero=0.3),
}

_WIDE = {}


def wide_reference(name):
    """(case, reference beams, gap) of a WIDE_OPTION_CASES entry, computed once per
    session and never modified, with what the entry needs of its reference
    checked: a gap >= MIN_GAP; order 8: more than 8 words scored in the best
    hypothesis; zeroed emissions: at least `beam` hypotheses of finite total per
    utterance."""
    if name not in _WIDE:
        c = WordCase(**WIDE_OPTION_CASES[name])
        ref, gap = c.reference()
        _WIDE[name] = (c, ref, gap)
    c, ref, gap = _WIDE[name]
    assert gap >= MIN_GAP, gap
    if c.order > 5:   # only then does the window shift (the 7-token context is full)
        assert all(u[0][4] > 8 for u in ref), [u[0][4] for u in ref]
    if WIDE_OPTION_CASES[name].get("zero"):
        assert (c.emis == 0).any()
        for u in ref:
            assert sum(math.isfinite(h[1]) for h in u) >= c.beam, len(u)
    return c, ref, gap


# ---- the worked example: the word LM keeps what the plain search pruned -------
# Labels: 0 blank, 1 "a", 2 "b", 3 "c", 4 " "; the lexicon is the three one-letter
# words; beam 2 (three states kept, ties aside); alpha 1, beta 0; <s> on, </s> off.
#   P(a | <s>) = P(b | <s>) = 0.05 (-1.30103)     P(c | <s>) = 0.9 (-0.045757)
# Frame 0 emits ($ .05, a .40, b .30, c .20, sp .05), frame 1 ($ .355, a .015,
# b .015, c .015, sp .60).
# Frame 0, both searches (no word has ended, W = 0): "a" .40, "b" .30, "c" .20 stay.
# Plain, frame 1: "a " .24 > "b " .18 > "a$" .142 > "c " .12 > "b$" .1065 > "c$"
#   .071: "c " and "c$" are pruned, no hypothesis that starts with c is left, and
#   the final beam is ["a ", "b ", "a"].  No re-ranking of it can produce "c ".
# Fused, frame 1: the space ends a word, so "a " .24 * .05 = .012, "b " .18 * .05
#   = .009, "c " .12 * .9 = .108; the states inside a word keep W = 0: "a$" .142,
#   "b$" .1065, "c$" .071.  "a$", "c " and "b$" stay.  At the final the pending
#   words of "a" and "b" are scored: "a" .142 * .05 = .0071, "b" .005325.
#   The best is "c " with total ln .108 = -2.2256, ctc ln .12 = -2.1203, lm_log10
#   -0.045757, one word; then "a" (ln .0071) and "b" (ln .005325).
WORKED_ARPA = """
\\data\\
ngram 1=5
ngram 2=3

\\1-grams:
-99\t<s>\t0
-1.5\t</s>
-0.7\ta\t0
-0.7\tb\t0
-0.7\tc\t0

\\2-grams:
-1.30103\t<s> a
-1.30103\t<s> b
-0.045757\t<s> c

\\end\\
"""
WORKED_LABELS = ["", "a", "b", "c", " "]
WORKED_EMIS = np.array([[[0.05, 0.40, 0.30, 0.20, 0.05]], [[0.355, 0.015, 0.015, 0.015, 0.60]]], np.float32)
WORKED_BEAM = 2
WORKED_BEST = [3, 4]
WORKED_CTC = math.log(0.20 * 0.60)
WORKED_LM10 = -0.045757
WORKED_TOTAL = WORKED_CTC + asr.LN10 * WORKED_LM10
WORKED_RANKED = [[3, 4], [1], [2]]
WORKED_PLAIN = [[1, 4], [2, 4], [1]]
