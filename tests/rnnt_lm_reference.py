"""The transducer beam search with the n-gram LM fused into every prune, restated
in plain torch float64 on top of rnnt_beam_reference.BeamReference and
lm_reference.ArpaModel, independent of the library: the reference of
tests/test_rnnt_lm_cpu.py and tests/test_rnnt_lm_gpu.py.

The search is BeamReference.search's; a hypothesis carries beside its acoustic
score s the LM weight W and the log10 sum L of its tokens,
    W(ys + [y]) = W(ys) + ((aln10 * v) + beta),   L(ys + [y]) = L(ys) + v,
v the model's value of tok(y) after tok(ys) (lm_reference, ASR_LM_BOS as
configured, ASR_LM_EOS off), in Python floats in exactly this order.  Candidates
are kept and ordered by fused = acoustic + weight; a merge adds the acoustic
scores (logaddexp) and takes the timesteps of the higher fused score; the final
A is ranked by total = s + W (+ aln10 * v_eos with ASR_LM_EOS).
"""
import math

import numpy as np
import torch

from lm_reference import BOS, EOS
from rnnt_beam_reference import BeamReference, _Hyp, _key
from rnnt_reference import F64, _t

LN10 = 2.302585092994046


class _LmHyp(_Hyp):
    __slots__ = ("W", "L")


class LmBeamReference(BeamReference):
    def lm_setup(self, model, tok_of_label, alpha, beta, flags, oov_log10=-100.0):
        """model: lm_reference.ArpaModel; alpha and beta go through fp32 as in the C ABI."""
        self.lm, self.tok = model, [int(x) for x in tok_of_label]
        self.aln10 = float(np.float32(alpha)) * LN10
        self.beta = float(np.float32(beta))
        self.flags, self.oov_log10 = int(flags), oov_log10
        self._values = {}
        return self

    def _value(self, ys, eos=False):
        """(value, matched order, context tokens in reach, is OOV) of the token after ys[:-1] (of </s> after ys)."""
        key = (ys, eos)
        if key not in self._values:
            row = [self.tok[y] for y in ys]
            _tot, _cnt, values, orders = self.lm.score(row, (self.flags & BOS) | (EOS if eos else 0), self.oov_log10)
            n = len(row) if eos else len(row) - 1          # tokens before the scored one
            reach = 0
            for j in range(n - 1, -1, -1):
                if reach == self.lm.order - 1 or ((row[j] < 0 or row[j] >= self.lm.vocab) and self.lm.unk < 0):
                    break
                reach += 1
            else:
                if reach < self.lm.order - 1 and (self.flags & BOS):
                    reach += 1
            oov = (not eos) and (row[-1] < 0 or row[-1] >= self.lm.vocab)
            self._values[key] = (values[-1], orders[-1], reach, oov)
        return self._values[key]

    def search_lm(self, enc, lengths=None, beam=4, nbest=None, max_out=None):
        """As BeamReference.search; a hypothesis is (tokens, timesteps, total, am,
        lm_log10, n_tokens), the margins are over fused scores and totals, and
        the dict also has backoffs ({orders backed off: lookups} over the tokens
        hypotheses took), oov (OOV tokens scored), and per hypothesis weights (W)
        and eos_terms (aln10 * v_eos, 0.0 without ASR_LM_EOS): total is
        (am + W) + eos_term where the flag is set, am + W where not.
        For the option cases also: frame_sizes and kept_labels as in
        BeamReference.search; over the tokens hypotheses took: max_order (the
        highest order a lookup was answered at), max_ctx (the longest context in
        reach of a lookup) and full_ctx_backoffs (lookups with order - 1 tokens
        in reach that backed off); over the final lists: eos_full_ctx (</s>
        terms looked up with order - 1 tokens in reach), max_len (the longest
        final hypothesis) and pre_eos_rank (per utterance and final hypothesis,
        its rank before the </s> term, so [0, 1, ..] where the term reorders
        nothing)."""
        enc = _t(enc)
        T, B = enc.shape[0], enc.shape[1]
        K = int(beam)
        nbest = K if nbest is None else int(nbest)
        max_out = T if max_out is None else int(max_out)
        V = self.w["b_out"].shape[0]
        out = {"hyps": [], "lens": [], "margin": [], "frames": [], "merges": 0, "deep_merges": 0, "short_frames": 0,
               "backoffs": {}, "oov": 0, "weights": [], "eos_terms": [], "frame_sizes": [], "kept_labels": set(),
               "max_order": 0, "max_ctx": 0, "full_ctx_backoffs": 0, "eos_full_ctx": 0, "max_len": 0,
               "pre_eos_rank": []}
        max_abs = 0.0

        def hyp(ys, ts, score, h, c, node, pnode, W, L):
            x = _LmHyp(ys, ts, score, h, c, node, pnode)
            x.W, x.L = W, L
            return x

        for b in range(B):
            h = [torch.zeros(self.Hp, dtype=F64) for _ in range(self.L)]
            c = [torch.zeros(self.Hp, dtype=F64) for _ in range(self.L)]
            self._step(self.blank, h, c)
            A = [hyp((), (), 0.0, h, c, 0, None, 0.0, 0.0)]
            nodes = 0
            ln = T if lengths is None else max(0, min(int(lengths[b]), T))
            margins, sizes = [], []
            for t in range(ln):
                f = enc[t, b] @ self.w["w_enc"] + self.w["b_enc"]
                cands = []
                for i, x in enumerate(A):
                    logit = self._joint(f, x.h[self.L - 1])
                    max_abs = max(max_abs, float(logit.abs().max()))
                    lp = (logit - torch.logsumexp(logit, 0)).tolist()
                    for v in range(V):
                        ac = x.score + lp[v]
                        if v == self.blank:
                            w = x.W
                        else:
                            val = self._value(x.ys + (v,))[0]
                            w = x.W + ((self.aln10 * val) + self.beta)
                        cands.append((ac + w, ac, w, i, v))
                cands.sort(key=lambda e: _key(e[0], e[3] * V + e[4]))
                nk = min(K, len(cands))
                if len(cands) > nk:
                    margins.append(cands[nk - 1][0] - cands[nk][0])
                ent = []
                for pos, (fu, ac, w, i, v) in enumerate(cands[:nk]):
                    x = A[i]
                    if v == self.blank:
                        ent.append(dict(fused=fu, score=ac, W=w, L=x.L, ys=x.ys, ts=x.ts, src=x, tok=None, pos=pos,
                                        node=x.node, pnode=x.pnode))
                    else:
                        val, q, reach, oov = self._value(x.ys + (v,))
                        out["oov"] += int(oov)
                        out["kept_labels"].add(v)
                        out["max_order"], out["max_ctx"] = max(out["max_order"], q), max(out["max_ctx"], reach)
                        if q >= 1 and reach + 1 - q > 0:
                            out["backoffs"][reach + 1 - q] = out["backoffs"].get(reach + 1 - q, 0) + 1
                            out["full_ctx_backoffs"] += int(reach == self.lm.order - 1)
                        ent.append(dict(fused=fu, score=ac, W=w, L=x.L + val, ys=x.ys + (v,), ts=x.ts + (t,), src=x,
                                        tok=v, pos=pos, node=None, pnode=x.node))
                merged = []
                for e in ent:
                    for m in merged:
                        if m["ys"] == e["ys"]:
                            assert m["W"] == e["W"] and m["L"] == e["L"]    # functions of the sequence alone
                            out["merges"] += 1
                            if m["pnode"] != e["pnode"]:
                                out["deep_merges"] += 1
                            margins.append(abs(m["fused"] - e["fused"]))
                            if e["fused"] > m["fused"]:
                                m["ts"], m["node"], m["pnode"] = e["ts"], e["node"], e["pnode"]
                            if m["tok"] is not None:
                                m["src"], m["tok"] = e["src"], e["tok"]
                            hi, lo = max(m["score"], e["score"]), min(m["score"], e["score"])
                            m["score"] = hi + math.log1p(math.exp(lo - hi))
                            m["fused"] = m["score"] + m["W"]
                            break
                    else:
                        merged.append(e)
                merged.sort(key=lambda e: _key(e["fused"], e["pos"]))
                if len(merged) < K:
                    out["short_frames"] += 1
                sizes.append((nk, len(merged)))
                new = []
                for e in merged:
                    src = e["src"]
                    if e["node"] is None:
                        nodes += 1
                        e["node"] = nodes
                    if e["tok"] is None:
                        new.append(hyp(e["ys"], e["ts"], e["score"], src.h, src.c, e["node"], e["pnode"], e["W"], e["L"]))
                    else:
                        h2, c2 = [x.clone() for x in src.h], [x.clone() for x in src.c]
                        self._step(e["tok"], h2, c2)
                        new.append(hyp(e["ys"], e["ts"], e["score"], h2, c2, e["node"], e["pnode"], e["W"], e["L"]))
                A = new
            final = []
            for rank, x in enumerate(A):
                total, L, term = x.score + x.W, x.L, 0.0
                if self.flags & EOS:
                    ve, _q, reach, _oov = self._value(x.ys, eos=True)
                    out["eos_full_ctx"] += int(reach == self.lm.order - 1)
                    term = self.aln10 * ve
                    total = total + term
                    L = L + ve
                final.append((total, rank, x, L, term))
            final.sort(key=lambda e: _key(e[0], e[1]))
            for x, y in zip(final, final[1:]):
                margins.append(x[0] - y[0])
            out["hyps"].append([(list(x.ys[:max_out]), list(x.ts[:max_out]), total, x.score, L, len(x.ys))
                                for total, _r, x, L, _e in final[:nbest]])
            out["lens"].append([len(x.ys) for _t2, _r, x, _L, _e in final[:nbest]])
            out["weights"].append([e[2].W for e in final[:nbest]])
            out["eos_terms"].append([e[4] for e in final[:nbest]])
            out["margin"].append(min(margins, default=math.inf))
            out["frames"].append(ln)
            out["frame_sizes"].append(sizes)
            out["pre_eos_rank"].append([e[1] for e in final])
            out["max_len"] = max([out["max_len"]] + [len(e[2].ys) for e in final])
        out["max_abs_logit"] = max_abs
        return out
