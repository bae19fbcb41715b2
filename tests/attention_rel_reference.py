"""References for relative-position (Transformer-XL) self-attention, no device
code: a float64 numpy restatement of the formula in the library's layout
(positions, lengths and the chunk / left / right window as asr_attention_fwd
has them), built on attention_reference.mask_matrix, and a torch stand-in
written from the published formulas of the toolkits'
RelPositionMultiHeadedAttention (matrix_ac, matrix_bd, the pad-and-view
rel_shift done literally, the sinusoidal RelPositionalEncoding with
flip(positive) + negative[1:]).  test_attention_rel_cpu.py checks the one
against the other.  No kernel reads these yet: they are the
yardstick a device implementation is to be checked against."""
import math

import numpy as np
import torch

import attention_reference as ar


def needed_rows(Tq, Tk, chunk=1, left=-1, right=-1, q_pos0=0, k_pos0=0):
    """(delta_max, delta_min): the largest and smallest distance query frame -
    key frame a call can ask for, from its frames and the window, lengths ignored."""
    dmax = q_pos0 + Tq - 1 - k_pos0
    dmin = q_pos0 - (k_pos0 + Tk - 1)
    if left >= 0:
        dmax = min(dmax, (left + 1) * chunk - 1)
    if right >= 0:
        dmin = max(dmin, -((right + 1) * chunk - 1))
    return dmax, dmin


def draw_rel(shape, mask=(1, -1, -1), seed=0):
    """(table [n_pos][E] U(+-1) of exactly the rows a plain call over T frames
    needs, pos_zero, u [E], v [E] U(+-0.5)); float32."""
    T, B, H, D = shape
    dmax, dmin = needed_rows(T, T, *mask)
    rng = np.random.default_rng(7000 * D + 300 * H + T + 13 * mask[0] + seed)
    pos = rng.uniform(-1, 1, (dmax - dmin + 1, H * D)).astype(np.float32)
    u, v = (rng.uniform(-0.5, 0.5, H * D).astype(np.float32) for _ in range(2))
    return pos, dmax, u, v


def attention_rel_ref(q, k, v, heads, pos, pos_zero, bias_u=None, bias_v=None, chunk=1, left=-1, right=-1,
                      lengths=None, scale=0.0, q_pos0=0, k_pos0=0):
    """(out [Tq][B][E] float64, seen [Tq][B] bool): softmax_r(scale ((q_p + u) .
    k_r + (q_p + v) . pos[pos_zero - (p - r)])) v_r per head over the keys each
    query sees; zeros for queries past the length and for queries that see no
    key.  Only the table rows of visible pairs are read."""
    q, k, v, pos = (np.asarray(a, np.float64) for a in (q, k, v, pos))
    Tq, B, E = q.shape
    Tk = k.shape[0]
    D = E // heads
    bu = np.zeros(E) if bias_u is None else np.asarray(bias_u, np.float64).reshape(E)
    bv = np.zeros(E) if bias_v is None else np.asarray(bias_v, np.float64).reshape(E)
    sc = scale if scale else 1.0 / np.sqrt(D)
    out = np.zeros((Tq, B, E))
    seen = np.zeros((Tq, B), bool)
    row = pos_zero - ((q_pos0 + np.arange(Tq))[:, None] - (k_pos0 + np.arange(Tk))[None, :])   # [Tq][Tk]
    for b in range(B):
        n = 2 ** 40 if lengths is None else max(int(lengths[b]), 0)
        m = ar.mask_matrix(Tq, Tk, n, chunk, left, right, q_pos0, k_pos0)
        seen[:, b] = m.any(1)
        ii, jj = np.nonzero(m)
        if ii.size == 0:
            continue
        assert row[ii, jj].min() >= 0 and row[ii, jj].max() < pos.shape[0], "the table does not cover a visible pair"
        rows, cols = m.any(1), m.any(0)                        # keys nobody sees may hold NaN
        for h in range(heads):
            sl = slice(h * D, (h + 1) * D)
            qq, kk, vv = q[rows, b, sl], k[:, b, sl], v[:, b, sl]
            bd = np.zeros((Tq, Tk))
            bd[ii, jj] = np.einsum("nd,nd->n", q[ii, b, sl] + bv[sl], pos[row[ii, jj], sl])
            s = np.full((qq.shape[0], Tk), -np.inf)
            s[:, cols] = ((qq + bu[sl]) @ kk[cols].T + bd[rows][:, cols]) * sc
            s[~m[rows]] = -np.inf
            s -= s.max(1, keepdims=True)
            pr = np.exp(s)
            pr /= pr.sum(1, keepdims=True)
            out[rows, b, sl] = pr[:, cols] @ vv[cols]
    return out, seen


def rel_pos_emb(T, E, dtype=torch.float64):
    """The toolkits' RelPositionalEncoding for T frames, [1][2T - 1][E]: positive
    positions sin / cos(+pos w), flipped; negative ones sin / cos(-pos w) from 1."""
    position = torch.arange(0, T, dtype=dtype).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, E, 2, dtype=dtype) * -(math.log(10000.0) / E))
    pe_positive, pe_negative = torch.zeros(T, E, dtype=dtype), torch.zeros(T, E, dtype=dtype)
    pe_positive[:, 0::2] = torch.sin(position * div_term)
    pe_positive[:, 1::2] = torch.cos(position * div_term)
    pe_negative[:, 0::2] = torch.sin(-1 * position * div_term)
    pe_negative[:, 1::2] = torch.cos(-1 * position * div_term)
    pe_positive = torch.flip(pe_positive, [0]).unsqueeze(0)
    pe_negative = pe_negative[1:].unsqueeze(0)
    return torch.cat([pe_positive, pe_negative], dim=1)


class RelPositionAttention(torch.nn.Module):
    """Batch-first [B][T][E] relative-position self-attention in the toolkits'
    attribute layout: linear_q / k / v / out with bias, linear_pos without,
    pos_bias_u / pos_bias_v [heads][d_k]."""

    def __init__(self, E, heads):
        super().__init__()
        assert E % heads == 0
        self.h, self.d_k = heads, E // heads
        self.linear_q, self.linear_k, self.linear_v, self.linear_out = (torch.nn.Linear(E, E) for _ in range(4))
        self.linear_pos = torch.nn.Linear(E, E, bias=False)
        self.pos_bias_u = torch.nn.Parameter(torch.zeros(heads, self.d_k))
        self.pos_bias_v = torch.nn.Parameter(torch.zeros(heads, self.d_k))

    @staticmethod
    def rel_shift(x):
        """[B][h][T][2T - 1] -> [B][h][T][T]: pad a zero column, view with the
        last two sizes swapped, drop the first row, view back, keep T columns."""
        zero_pad = torch.zeros((*x.size()[:3], 1), dtype=x.dtype)
        x_padded = torch.cat([zero_pad, x], dim=-1)
        x_padded = x_padded.view(*x.size()[:2], x.size(3) + 1, x.size(2))
        return x_padded[:, :, 1:].view_as(x)[:, :, :, : x.size(-1) // 2 + 1]

    def core(self, q, k, v, p, allowed=None):
        """q, k, v [B][T][h][d_k], p [1][2T - 1][h][d_k] (projected already),
        allowed [T][T] bool or None -> [B][T][E]."""
        q_with_bias_u = (q + self.pos_bias_u).transpose(1, 2)
        q_with_bias_v = (q + self.pos_bias_v).transpose(1, 2)
        k, v, p = k.transpose(1, 2), v.transpose(1, 2), p.transpose(1, 2)
        matrix_ac = torch.matmul(q_with_bias_u, k.transpose(-2, -1))
        matrix_bd = self.rel_shift(torch.matmul(q_with_bias_v, p.transpose(-2, -1)))
        scores = (matrix_ac + matrix_bd) / math.sqrt(self.d_k)
        if allowed is not None:
            scores = scores.masked_fill(~allowed, -float("inf"))
        attn = torch.softmax(scores, dim=-1)
        x = torch.matmul(attn, v)
        return x.transpose(1, 2).contiguous().view(q.size(0), -1, self.h * self.d_k)

    def forward(self, x, pos_emb, allowed=None):
        B, T = x.shape[:2]
        split = lambda t: t.view(t.size(0), -1, self.h, self.d_k)   # noqa: E731
        return self.linear_out(self.core(split(self.linear_q(x)), split(self.linear_k(x)), split(self.linear_v(x)),
                                         split(self.linear_pos(pos_emb)), allowed))
