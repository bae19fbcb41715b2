"""RNN-T greedy decoding restated in plain torch float64, independent of the
library: the reference of tests/test_rnnt_cpu.py and tests/test_rnnt_gpu.py.

Model (weights [in][out], as the library stores them): Emb [V, D]; L LSTM
layers, gates i, f, g, o, z = (x.W_ih + h.W_hh) + (b_ih + b_hh); joint
f_t = enc_t.W_enc + b_enc, g = h_top.W_pred + b_pred, z = act(f_t + g),
logit = z.W_out + b_out.  k = argmax logit, the lowest index among equal
maxima, a NaN never wins; logp = logit[k] - logsumexp(logit).

Walk of one utterance (length clamped to [0, T]): without a state h = c = 0
and the predictor takes one step on Emb[blank]; t = 0, n = 0; while t < len:
evaluate; k != blank: record (k, t, logp), step the predictor on Emb[k],
n += 1, and at n == max_symbols: t += 1, n = 0; k == blank: logp goes to the
total only, t += 1, n = 0.
"""
import math

import torch

F64 = torch.float64


def _t(a):
    return torch.as_tensor(a, dtype=F64)


class Reference:
    """weights: emb, w_ih[l], w_hh[l], b_ih[l], b_hh[l], w_enc, b_enc, w_pred,
    b_pred, w_out, b_out (arrays or tensors); act 'relu' or 'tanh'."""

    def __init__(self, weights, blank, act="relu", max_symbols=10):
        self.w = {k: ([_t(x) for x in v] if isinstance(v, (list, tuple)) else _t(v)) for k, v in weights.items()}
        self.blank, self.act, self.max_symbols = int(blank), act, int(max_symbols)
        self.L = len(self.w["w_ih"])
        self.Hp = self.w["w_hh"][0].shape[0]

    def _step(self, tok, h, c):
        x = self.w["emb"][tok]
        Hp = self.Hp
        for l in range(self.L):
            z = (x @ self.w["w_ih"][l] + h[l] @ self.w["w_hh"][l]) + (self.w["b_ih"][l] + self.w["b_hh"][l])
            i, f = torch.sigmoid(z[:Hp]), torch.sigmoid(z[Hp:2 * Hp])
            g, o = torch.tanh(z[2 * Hp:3 * Hp]), torch.sigmoid(z[3 * Hp:])
            c[l] = f * c[l] + i * g
            h[l] = o * torch.tanh(c[l])
            x = h[l]

    def _joint(self, f, h_top):
        v = f + (h_top @ self.w["w_pred"] + self.w["b_pred"])
        z = torch.tanh(v) if self.act == "tanh" else torch.clamp(v, min=0.0)
        return z @ self.w["w_out"] + self.w["b_out"]

    def decode(self, enc, lengths=None, state=None, max_out=None):
        """enc [T, B, E].  Returns a dict: per utterance tokens, timesteps,
        logps (lists, cut at max_out), total, count (not cut), frames (the
        emissions of each frame it walked); state [2, L, B, Hp] float64; gap
        [B] (smallest best-minus-second-best logit of the walk, inf when
        nothing was evaluated) and max_abs_logit."""
        enc = _t(enc)
        T, B = enc.shape[0], enc.shape[1]
        if max_out is None:
            max_out = T * self.max_symbols
        out = {k: [] for k in ("tokens", "timesteps", "logps", "total", "count", "frames", "gap")}
        new_state = torch.zeros((2, self.L, B, self.Hp), dtype=F64)
        max_abs = 0.0
        for b in range(B):
            h = [torch.zeros(self.Hp, dtype=F64) for _ in range(self.L)]
            c = [torch.zeros(self.Hp, dtype=F64) for _ in range(self.L)]
            if state is not None:
                st = _t(state)
                for l in range(self.L):
                    h[l], c[l] = st[0, l, b].clone(), st[1, l, b].clone()
            else:
                self._step(self.blank, h, c)
            ln = T if lengths is None else max(0, min(int(lengths[b]), T))
            toks, tss, lps, frames = [], [], [], []
            total, gap, count = 0.0, math.inf, 0
            for t in range(ln):
                f = enc[t, b] @ self.w["w_enc"] + self.w["b_enc"]
                n = 0
                while True:
                    logit = self._joint(f, h[self.L - 1])
                    clean = torch.where(torch.isnan(logit), torch.full_like(logit, -math.inf), logit)
                    top = clean.max()
                    k = int(torch.nonzero(clean == top)[0])     # the lowest index among equal maxima
                    lp = float(logit[k] - torch.logsumexp(logit, 0))
                    two = torch.topk(clean, 2).values
                    gap = min(gap, float(two[0] - two[1]))
                    max_abs = max(max_abs, float(logit.abs().max()))
                    total += lp
                    if k == self.blank:
                        break
                    if count < max_out:
                        toks.append(k), tss.append(t), lps.append(lp)
                    count += 1
                    n += 1
                    self._step(k, h, c)
                    if n == self.max_symbols:
                        break
                frames.append(n)
            for l in range(self.L):
                new_state[0, l, b], new_state[1, l, b] = h[l], c[l]
            for k, v in zip(("tokens", "timesteps", "logps", "total", "count", "frames", "gap"),
                            (toks, tss, lps, total, count, frames, gap)):
                out[k].append(v)
        out["state"] = new_state.numpy()
        out["max_abs_logit"] = max_abs
        return out
