"""Token-and-duration transducer greedy decoding restated in plain torch
float64, independent of the library: the reference of tests/test_rnnt_tdt_cpu.py
and tests/test_rnnt_tdt_gpu.py.  The model is rnnt_reference.py's plus
dlogit = z.W_dur + b_dur and a table durations[D].

One evaluation: k = argmax logit, d = argmax dlogit (the lowest index among
equal maxima, a NaN never wins), logp = (logit[k] - logsumexp(logit)) +
(dlogit[d] - logsumexp(dlogit)).  Walk: t = skip_in, n = 0; while t < len:
evaluate, dur = durations[d]; k == blank: logp to the total only,
t += max(dur, 1), n = 0; else record (k, t, dur, logp), step the predictor,
n += 1, then dur > 0: t += dur, n = 0; else n == max_symbols: t += 1, n = 0.
skip_out = t - len (skip_in - len for a chunk skipped whole).
"""
import math

import torch

from rnnt_reference import F64, Reference, _t


def _head(x):
    clean = torch.where(torch.isnan(x), torch.full_like(x, -math.inf), x)
    k = int(torch.nonzero(clean == clean.max())[0])     # the lowest index among equal maxima
    two = torch.topk(clean, 2).values if len(x) > 1 else (clean[0], _t(-math.inf))
    return k, float(x[k] - torch.logsumexp(x, 0)), float(two[0] - two[1])


class TdtReference(Reference):
    """weights: Reference's plus w_dur [J, D], b_dur [D]."""

    def __init__(self, weights, durations, blank, act="relu", max_symbols=10):
        super().__init__(weights, blank, act, max_symbols)
        self.durations = [int(d) for d in durations]

    def decode(self, enc, lengths=None, state=None, max_out=None):
        """enc [T, B, E]; state None or (hc [2, L, B, Hp], skip [B]).  Returns a
        dict: per utterance tokens, timesteps, durations, logps (cut at
        max_out), total, count (not cut), evals (joint evaluations), skip,
        gap and dgap (smallest top-2 gap of each head), kinds (the kinds of
        step the walk took); state (hc, skip); max_abs_logit over both heads."""
        enc = _t(enc)
        T, B = enc.shape[0], enc.shape[1]
        if max_out is None:
            max_out = T * self.max_symbols
        names = ("tokens", "timesteps", "durations", "logps", "total", "count", "evals", "skip", "gap", "dgap", "kinds")
        out = {k: [] for k in names}
        new_state = torch.zeros((2, self.L, B, self.Hp), dtype=F64)
        max_abs = 0.0
        for b in range(B):
            h = [torch.zeros(self.Hp, dtype=F64) for _ in range(self.L)]
            c = [torch.zeros(self.Hp, dtype=F64) for _ in range(self.L)]
            t = 0
            if state is not None:
                st = _t(state[0])
                for l in range(self.L):
                    h[l], c[l] = st[0, l, b].clone(), st[1, l, b].clone()
                t = max(int(state[1][b]), 0)
            else:
                self._step(self.blank, h, c)
            ln = T if lengths is None else max(0, min(int(lengths[b]), T))
            toks, tss, durs, lps, kinds = [], [], [], [], set()
            total, gap, dgap, count, evals, n = 0.0, math.inf, math.inf, 0, 0, 0
            while t < ln:
                f = enc[t, b] @ self.w["w_enc"] + self.w["b_enc"]
                v = f + (h[self.L - 1] @ self.w["w_pred"] + self.w["b_pred"])
                z = torch.tanh(v) if self.act == "tanh" else torch.clamp(v, min=0.0)
                logit, dlogit = z @ self.w["w_out"] + self.w["b_out"], z @ self.w["w_dur"] + self.w["b_dur"]
                (k, lpk, gk), (d, lpd, gd) = _head(logit), _head(dlogit)
                dur, lp = self.durations[d], lpk + lpd
                gap, dgap = min(gap, gk), min(dgap, gd)
                max_abs = max(max_abs, float(logit.abs().max()), float(dlogit.abs().max()))
                total += lp
                evals += 1
                if k == self.blank:
                    kinds.add("blank>1" if dur > 1 else "blank0" if dur == 0 else "blank1")
                    t, n = t + max(dur, 1), 0
                    continue
                if count < max_out:
                    toks.append(k), tss.append(t), durs.append(dur), lps.append(lp)
                count += 1
                n += 1
                self._step(k, h, c)
                kinds.add("token>0" if dur > 0 else "token0")
                if dur > 0:
                    t, n = t + dur, 0
                elif n == self.max_symbols:
                    kinds.add("cap")
                    t, n = t + 1, 0
            if t > ln:
                kinds.add("skip")
            for l in range(self.L):
                new_state[0, l, b], new_state[1, l, b] = h[l], c[l]
            for k, v in zip(names, (toks, tss, durs, lps, total, count, evals, t - ln, gap, dgap, kinds)):
                out[k].append(v)
        out["state"] = (new_state.numpy(), out["skip"])
        out["max_abs_logit"] = max_abs
        return out
