"""The stateless-predictor transducer in plain torch float64, independent of the
library: the references of tests/test_rnnt_stateless_cpu.py and _gpu.py.

    p = relu(sum_c Emb[y_c] @ W_ctx[c] + b_ctx)     (C = 1 without W_ctx: Emb[y_0])
    g = p @ W_pred + b_pred, then rnnt_reference's joint.

(y_0 .. y_{C-1}) are the last C tokens of (start_fill, ..., blank) + ys, -1 adding
nothing.  The searches are not restated: the four references run as they are
with the predictor step replaced.  They keep (h[l], c[l]) of Hp floats and start
from zeros with a step on the blank; here L = 1, h[0] is p, c[0] holds the
context and behind it a flag that the start was made.
"""
import torch

from rnnt_align_reference import AlignReference
from rnnt_beam_reference import BeamReference
from rnnt_lm_reference import LmBeamReference
from rnnt_reference import F64, Reference, _t


class _Stateless:
    def __init__(self, weights, blank, act="tanh", max_symbols=1, context=2, start_fill=-1):
        self.w = {k: _t(v) for k, v in weights.items() if v is not None}
        self.blank, self.act, self.max_symbols = int(blank), act, int(max_symbols)
        self.C, self.start_fill = int(context), int(start_fill)
        self.L, self.Hp = 1, self.w["w_pred"].shape[0]

    def _pred(self, ctx):
        p = torch.zeros(self.Hp, dtype=F64)
        for i, y in enumerate(ctx):
            if y >= 0:
                e = self.w["emb"][y]
                p = p + (e @ self.w["w_ctx"][i] if "w_ctx" in self.w else e)
        if "b_ctx" in self.w:
            p = p + self.w["b_ctx"]
        return torch.clamp(p, min=0.0)

    def _step(self, tok, h, c):
        C = self.C
        if c[0][C] == 0:      # the start: tok is the blank
            ctx = [self.start_fill] * (C - 1) + [self.blank]
        else:
            ctx = [int(x) for x in c[0][1:C]] + [int(tok)]
        c[0] = torch.zeros(self.Hp, dtype=F64)
        c[0][:C] = torch.tensor(ctx, dtype=F64)
        c[0][C] = 1.0
        h[0] = self._pred(ctx)

    def state_of(self, ctx):
        """A context [B, C] as the [2, 1, B, Hp] state Reference.decode takes."""
        ctx = torch.as_tensor(ctx)
        st = torch.zeros((2, 1, ctx.shape[0], self.Hp), dtype=F64)
        for b in range(ctx.shape[0]):
            st[0, 0, b] = self._pred([int(x) for x in ctx[b]])
            st[1, 0, b, :self.C] = ctx[b].to(F64)
            st[1, 0, b, self.C] = 1.0
        return st

    def context_of(self, state):
        """The context [B, C] of a state Reference.decode returned."""
        return state[1, 0, :, :self.C].round().astype("int32")


class StatelessReference(_Stateless, Reference):
    pass


class StatelessBeamReference(_Stateless, BeamReference):
    pass


class StatelessLmBeamReference(_Stateless, LmBeamReference):
    pass


class StatelessAlignReference(_Stateless, AlignReference):
    pass
