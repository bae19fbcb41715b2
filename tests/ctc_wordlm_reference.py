"""Pure-Python reference of the word mode of the LM-fused CTC beam search
(asr_ctc_lm_create_word, include/asr_amd.h): the rules written
literally over dicts and sets.

The search is ctc_lm_reference.FusedSearch's (states as tuples of symbol codes,
the sorted fold order, math.exp / math.log1p lse, the prune at the (beam+1)-th
largest fused score with ties kept).  What differs is what a prefix carries:
its partial word (the labels after the last space), the row of word tokens
scored so far, W, L and n, all functions of the label string alone.  The
lexicon is a dict from a spelling (tuple of label ids) to an LM token id; "z is
OFF" is "the partial word is no prefix of a spelling".  Every LM value is
lm_reference.ArpaModel.score(row, flags)[2][-1] of a word-token row: the row
itself while it is no longer than the longest context, else its last
ASR_LM_MAX_ORDER tokens with ASR_LM_BOS off.

decode() also returns the smallest relative gap it met, as FusedSearch does; the
final totals it compares include the pending word's term.
"""
import math

import numpy as np

from ctc_lm_reference import MAX_CTX, FusedSearch, _Gap, lse
from lm_reference import BOS, EOS


class WordFusedSearch(FusedSearch):
    """One configuration; decode(emis[T][V]) -> (hyps, gap), hyps ranked
    [(labels, total, ctc_logp, lm_log10, n_words)]."""

    def __init__(self, model, V, beam, blank, space, lexicon, alpha, beta, bos=True, eos=False, top_n=0, closed=False,
                 codes=None, oov_log10=-100.0):
        super().__init__(model, V, beam, blank, [-1] * V, alpha, beta, bos=bos, eos=eos, top_n=top_n, codes=codes,
                         oov_log10=oov_log10)
        self.space, self.closed = space, closed
        self.lexicon = {tuple(int(c) for c in w): int(t) for w, t in lexicon.items()}
        self.prefixes = {w[:i] for w in self.lexicon for i in range(len(w) + 1)} | {()}

    def partial(self, labels):
        """The labels after the last space."""
        labels = tuple(labels)
        for i in range(len(labels) - 1, -1, -1):
            if labels[i] == self.space:
                return labels[i + 1:]
        return labels

    def value(self, row, eos=False):
        """LM value of the last token of the word-token row (</s> when eos)."""
        row = list(row)
        flags = BOS if self.bos else 0
        keep = MAX_CTX if eos else MAX_CTX + 1
        if len(row) > keep:   # <s> is out of reach of the longest context
            row, flags = row[-keep:], 0
        key = (tuple(row), flags, eos)
        if key not in self._lm_memo:
            self._lm_memo[key] = self.model.score(row, flags | (EOS if eos else 0), self.oov)[2][-1]
        return self._lm_memo[key]

    def end_word(self, state, word):
        """(W, L, n, row) after the non-empty partial word `word` ended."""
        W, L, n, row = state
        w = self.lexicon.get(tuple(word), -1)   # not terminal: an OOV
        row = row + (w,)
        v = self.value(row)
        return (W + ((self.aln10 * v) + self.beta), L + v, n + 1, row)

    def word_terms(self, labels, memo):
        """(W, L, n, row of word tokens) of a prefix, from its one parent."""
        if labels not in memo:
            if not labels:
                memo[labels] = (0.0, 0.0, 0, ())
            else:
                parent = self.word_terms(labels[:-1], memo)
                word = self.partial(labels[:-1])
                if labels[-1] != self.space or not word:   # a letter, or a space after an empty word
                    memo[labels] = parent
                else:
                    memo[labels] = self.end_word(parent, word)
        return memo[labels]

    def exists(self, q, c):
        """Is there a transition q -> q + c (labels)?"""
        if not self.closed:
            return True
        word = self.partial(q)
        if c == self.space:
            return word in self.lexicon
        return word + (c,) in self.prefixes

    def decode(self, emis, is_log=True):
        emis = np.asarray(emis, dtype=np.float32)
        T = emis.shape[0]
        code, blank, bcode = self.code, self.blank, self.code[self.blank]
        gap = _Gap()
        memo = {}

        def prefix_of(s):
            return s[:-1] if s and s[-1] == bcode else s

        def labels_of(s):
            return tuple(self.label_of[c] for c in prefix_of(s))

        def prune(score):
            if len(score) <= self.beam:
                return score
            fused = {s: x + self.word_terms(labels_of(s), memo)[0] for s, x in score.items()}
            cutoff = sorted(fused.values(), reverse=True)[self.beam]
            for x in fused.values():
                gap.note(x, cutoff)
            return {s: x for s, x in score.items() if fused[s] >= cutoff}

        def log_emis(t):
            return [float(x) if is_log else (math.log(float(x)) if x > 0 else -math.inf) for x in emis[t]]

        le = log_emis(0)
        C = self.candidates(emis[0])
        score = {(code[i],): le[i] for i in range(self.V) if i in C and (i == blank or self.exists((), i))}
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
                    elif s[-1] == code[i]:
                        ns = s                                   # the repeat always exists
                    else:
                        if not self.exists(labels_of(s), i):
                            continue                             # closed mode: no such transition
                        ns = (s[:-1] if s[-1] == bcode else s) + (code[i],)
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
            state = self.word_terms(labels, memo)
            word = self.partial(labels)
            if word:   # the pending word, scored as a space would score it
                state = self.end_word(state, word)
            W, L, n, row = state
            total = fin[p] + W
            if self.eos:
                v = self.value(row, eos=True)
                total = total + (self.aln10 * v)
                L = L + v
            hyps.append((list(labels), total, fin[p], L, n))
        hyps.sort(key=lambda h: -h[1])   # stable: equal totals keep the code-string order
        for a, b in zip(hyps, hyps[1:]):
            gap.note(a[1], b[1])
        return hyps, gap.value
