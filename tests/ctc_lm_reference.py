"""Pure-Python reference of the LM-fused CTC beam search of include/asr_amd.h
(asr_ctc_lm_*): the rules written literally over dicts and sets.

States are tuples of symbol codes ("q" / "q$"), Python's tuple order is the
reference's std::string order.  Emissions are fp64 (the fp32 inputs widened, or
their math.log), lse is math.exp / math.log1p, and every LM value is
lm_reference.ArpaModel.score(row, flags)[2][-1] of a prefix's token row: the row
itself while it is no longer than the longest context (so that <s> is in
reach), else its last ASR_LM_MAX_ORDER tokens with ASR_LM_BOS off, which the
contract states is all a prefix needs.

decode() also returns the smallest relative gap it met: |x - y| / max(1, |x|,
|y|) between the cutoff and every other (differing, finite) fused score at every
prune, and between adjacent differing final totals.  Two implementations whose
scores agree to 1e-9 cannot differ in ranks on a case whose gap is >= 1e-6.
"""
import math

import numpy as np

from lm_reference import BOS, EOS

LN10 = 2.302585092994046
MAX_CTX = 7   # ASR_LM_MAX_ORDER - 1


def lse(a, b):
    if a == -math.inf:
        return b
    if b == -math.inf:
        return a
    m = a if a > b else b
    return m + math.log1p(math.exp(-abs(a - b)))


class _Gap:
    def __init__(self):
        self.value = math.inf

    def note(self, x, y):
        if x == y or not (math.isfinite(x) and math.isfinite(y)):
            return
        self.value = min(self.value, abs(x - y) / max(1.0, abs(x), abs(y)))


class FusedSearch:
    """One configuration; decode(emis[T][V]) -> (hyps, gap), hyps ranked
    [(labels, total, ctc_logp, lm_log10, n_tokens)]."""

    def __init__(self, model, V, beam, blank, tok_of_label, alpha, beta, bos=True, eos=False, top_n=0,
                 codes=None, oov_log10=-100.0):
        self.model, self.V, self.beam, self.blank = model, V, beam, blank
        self.tok = [int(x) for x in tok_of_label]
        self.aln10 = float(np.float32(alpha)) * LN10
        self.beta = float(np.float32(beta))
        self.bos, self.eos, self.oov = bos, eos, oov_log10
        self.top_n = 0 if (top_n == 0 or top_n >= V - 1) else top_n
        self.code = list(range(V)) if codes is None else [int(c) for c in codes]
        self.label_of = {c: v for v, c in enumerate(self.code)}
        self._lm_memo = {}

    # value of the last token of `row` (</s> when eos), the row given by labels
    def lm_value(self, labels, eos=False):
        row = [self.tok[c] for c in labels]
        flags = BOS if self.bos else 0
        keep = MAX_CTX if eos else MAX_CTX + 1
        if len(row) > keep:   # <s> is out of reach of the longest context
            row, flags = row[-keep:], 0
        key = (tuple(row), flags, eos)
        if key not in self._lm_memo:
            self._lm_memo[key] = self.model.score(row, flags | (EOS if eos else 0), self.oov)[2][-1]
        return self._lm_memo[key]

    def terms(self, labels, memo):
        """(W, L, n) of a prefix, from its one parent."""
        if labels not in memo:
            if not labels:
                memo[labels] = (0.0, 0.0, 0)
            else:
                W, L, n = self.terms(labels[:-1], memo)
                v = self.lm_value(labels)
                memo[labels] = (W + ((self.aln10 * v) + self.beta), L + v, n + 1)
        return memo[labels]

    def candidates(self, raw):
        """Labels that take part at a frame: the blank and C_t."""
        nonblank = [v for v in range(self.V) if v != self.blank]
        if self.top_n:
            nonblank = sorted(nonblank, key=lambda v: (-float(raw[v]), v))[:self.top_n]
        return set(nonblank) | {self.blank}

    def decode(self, emis, is_log=True):
        emis = np.asarray(emis, dtype=np.float32)
        T = emis.shape[0]
        code, blank, bcode = self.code, self.blank, self.code[self.blank]
        gap = _Gap()
        memo = {}

        def prefix_of(s):
            return s[:-1] if s and s[-1] == bcode else s

        def W_of(s):
            return self.terms(tuple(self.label_of[c] for c in prefix_of(s)), memo)[0]

        def prune(score):
            if len(score) <= self.beam:
                return score
            fused = {s: x + W_of(s) for s, x in score.items()}
            cutoff = sorted(fused.values(), reverse=True)[self.beam]
            for x in fused.values():
                gap.note(x, cutoff)
            return {s: x for s, x in score.items() if fused[s] >= cutoff}

        def log_emis(t):
            return [float(x) if is_log else (math.log(float(x)) if x > 0 else -math.inf) for x in emis[t]]

        le = log_emis(0)
        C = self.candidates(emis[0])
        score = {(code[i],): le[i] for i in range(self.V) if i in C}
        score = prune(score)
        for t in range(1, T):
            le = log_emis(t)
            C = self.candidates(emis[t])
            new = {}
            for s in sorted(score):
                sc = score[s]
                for i in range(self.V):
                    if i not in C:
                        continue
                    if i == blank:
                        ns = s if s[-1] == bcode else s + (bcode,)
                    elif s[-1] == bcode:
                        ns = s[:-1] + (code[i],)
                    elif s[-1] == code[i]:
                        ns = s
                    else:
                        ns = s + (code[i],)
                    x = sc + le[i]
                    new[ns] = lse(new[ns], x) if ns in new else x
            score = prune(new)
        fin = {}
        for s in sorted(score):
            p = prefix_of(s)
            fin[p] = lse(fin[p], score[s]) if p in fin else score[s]
        hyps = []
        for p in sorted(fin):
            labels = tuple(self.label_of[c] for c in p)
            W, L, n = self.terms(labels, memo)
            total = fin[p] + W
            if self.eos:
                v = self.lm_value(labels, eos=True)
                total = total + (self.aln10 * v)
                L = L + v
            hyps.append((list(labels), total, fin[p], L, n))
        hyps.sort(key=lambda h: -h[1])   # stable: equal totals keep the code-string order
        for a, b in zip(hyps, hyps[1:]):
            gap.note(a[1], b[1])
        return hyps, gap.value


def decode_batch(search, emis, is_log=True, lengths=None):
    """emis [T][B][V]; -> ([hyps per utterance], smallest gap)."""
    emis = np.asarray(emis)
    out, gap = [], math.inf
    for b in range(emis.shape[1]):
        n = emis.shape[0] if lengths is None else int(lengths[b])
        h, g = search.decode(emis[:n, b], is_log)
        out.append(h)
        gap = min(gap, g)
    return out, gap
