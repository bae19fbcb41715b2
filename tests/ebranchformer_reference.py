"""References for the E-Branchformer tests (no device code): float64 numpy
restatements of the exact GELU, asr_csgu_fwd and asr_merge_dwconv_fwd in the
library's layout, and a small torch E-Branchformer block with the attribute
names of ESPnet's EBranchformerEncoderLayer / ConvolutionalGatingMLP /
PositionwiseFeedForward (the stand-in for EBranchformerLayer.from_espnet).
test_ebranchformer_cpu.py checks the restatements against torch in float64,
test_ebranchformer_gpu.py checks the device against both."""
import copy
import math

import numpy as np
import torch

import attention_reference as ar
import attention_rel_reference as arr
import conformer_reference as cr

WINDOWS = cr.WINDOWS
# EBranchformerLayer: (T, B, E, heads, units, k_cgmlp, k_merge)
LAYER_SHAPES = [(70, 5, 144, 4, 288, 15, 31), (40, 3, 64, 4, 128, 31, 31)]
LENGTHS = (None, 0, 1, 63, 64)          # None stands for T; each clamps to T


def lengths_for(T, B):
    return tuple(min(T if n is None else n, T) for n in (LENGTHS * B)[:B])


def gelu_ref(v):
    """0.5 v (1 + erf(v / sqrt 2)) in float64, as 0.5 v erfc(-v / sqrt 2)."""
    v = np.asarray(v, np.float64)
    return 0.5 * v * torch.special.erfc(torch.as_tensor(-v / math.sqrt(2.0))).numpy()


def _dwconv(x, w, b, pl):
    """x [n][C] float64 -> sum_j x(t - pl + j) w[j] + b over its own frames."""
    n, k = x.shape[0], w.shape[0]
    pad = np.zeros((n + k - 1, x.shape[1]))
    pad[pl:pl + n] = x
    acc = sum(pad[j:j + n] * np.asarray(w[j], np.float64) for j in range(k))
    return acc if b is None else acc + np.asarray(b, np.float64)


def csgu_ref(u, w, b, pl, gamma=None, beta=None, eps=1e-5, lengths=None):
    """[T][B][C] float64: x_r * (dwconv(LayerNorm(x_g)) + b) on each utterance's
    own frames; zeros past its length, frames past it never read."""
    T, B = u.shape[:2]
    C = w.shape[1]
    out = np.zeros((T, B, C))
    for bi in range(B):
        n = T if lengths is None else min(max(int(lengths[bi]), 0), T)
        uu = u[:n, bi].astype(np.float64)
        g = uu[:, C:2 * C]
        g = (g - g.mean(1, keepdims=True)) / np.sqrt(g.var(1, keepdims=True) + eps)
        g = g * (1 if gamma is None else np.asarray(gamma, np.float64)) + (0 if beta is None else
                                                                          np.asarray(beta, np.float64))
        if n:
            out[:n, bi] = uu[:, :C] * _dwconv(g, w, b, pl)
    return out


def merge_ref(x1, x2, w, b, pl, lengths=None):
    """[T][B][2C] float64: s + dwconv(s) + b, s = cat(x1, x2)."""
    T, B, C = x1.shape[0], x1.shape[1], w.shape[1] // 2
    out = np.zeros((T, B, 2 * C))
    for bi in range(B):
        n = T if lengths is None else min(max(int(lengths[bi]), 0), T)
        if n:
            s = np.concatenate([x1[:n, bi, :C], x2[:n, bi, :C]], axis=1).astype(np.float64)
            out[:n, bi] = s + _dwconv(s, w, b, pl)
    return out


def draw_conv(T, B, cols, k, C, seed=0):
    """x [T][B][cols] U(+-1), w [k][C] U(+-1/sqrt(k)), b [C] U(+-0.1); float32."""
    rng = np.random.default_rng(100000 * k + 1000 * C + 10 * T + B + seed)
    return (rng.uniform(-1, 1, (T, B, cols)).astype(np.float32),
            (rng.uniform(-1, 1, (k, C)) / np.sqrt(k)).astype(np.float32),
            rng.uniform(-0.1, 0.1, C).astype(np.float32))


# ------------------------------------------------------------- torch stand-in
class Swish(torch.nn.Module):
    def forward(self, x):
        return x * torch.sigmoid(x)


class PositionwiseFeedForward(torch.nn.Module):
    def __init__(self, E, F):
        super().__init__()
        self.w_1, self.w_2, self.activation = torch.nn.Linear(E, F), torch.nn.Linear(F, E), Swish()

    def forward(self, x):
        return self.w_2(self.activation(self.w_1(x)))


class Csgu(torch.nn.Module):
    def __init__(self, C, k, use_linear=False, act=None):
        super().__init__()
        self.norm = torch.nn.LayerNorm(C)
        self.conv = torch.nn.Conv1d(C, C, k, 1, (k - 1) // 2, groups=C)
        self.linear = torch.nn.Linear(C, C) if use_linear else None
        self.act = torch.nn.Identity() if act is None else act

    def forward(self, x):                                   # [B][T][2C]
        x_r, x_g = x.chunk(2, dim=-1)
        x_g = self.conv(self.norm(x_g).transpose(1, 2)).transpose(1, 2)
        if self.linear is not None:
            x_g = self.linear(x_g)
        return x_r * self.act(x_g)


class CgMLP(torch.nn.Module):
    def __init__(self, E, units, k, **kw):
        super().__init__()
        self.channel_proj1 = torch.nn.Sequential(torch.nn.Linear(E, units), torch.nn.GELU())
        self.csgu = Csgu(units // 2, k, **kw)
        self.channel_proj2 = torch.nn.Linear(units // 2, E)

    def forward(self, x):
        return self.channel_proj2(self.csgu(self.channel_proj1(x)))


class EBranchformerBlock(torch.nn.Module):
    """ESPnet's EBranchformerEncoderLayer, batch-first [B][T][E], dropout 0."""

    def __init__(self, E, heads, units, k, k_merge, rel=False, macaron=True):
        super().__init__()
        self.rel = rel
        self.attn = arr.RelPositionAttention(E, heads) if rel else torch.nn.MultiheadAttention(E, heads,
                                                                                             batch_first=True)
        self.cgmlp = CgMLP(E, units, k)
        self.feed_forward = PositionwiseFeedForward(E, units)
        self.feed_forward_macaron = PositionwiseFeedForward(E, units) if macaron else None
        self.ff_scale = 0.5 if macaron else 1.0
        self.norm_ff, self.norm_mha, self.norm_mlp, self.norm_final = (torch.nn.LayerNorm(E) for _ in range(4))
        self.norm_ff_macaron = torch.nn.LayerNorm(E) if macaron else None
        self.depthwise_conv_fusion = torch.nn.Conv1d(2 * E, 2 * E, k_merge, 1, (k_merge - 1) // 2, groups=2 * E)
        self.merge_proj = torch.nn.Linear(2 * E, E)

    def forward(self, x, allowed=None):                     # allowed [T][T] bool or None
        if self.feed_forward_macaron is not None:
            x = x + self.ff_scale * self.feed_forward_macaron(self.norm_ff_macaron(x))
        n = self.norm_mha(x)
        if self.rel:
            x1 = self.attn(n, arr.rel_pos_emb(x.shape[1], x.shape[2], x.dtype), allowed)
        else:
            x1, _ = self.attn(n, n, n, attn_mask=None if allowed is None else ~allowed, need_weights=False)
        x2 = self.cgmlp(self.norm_mlp(x))
        cat = torch.cat([x1, x2], dim=-1)
        x = x + self.merge_proj(cat + self.depthwise_conv_fusion(cat.transpose(1, 2)).transpose(1, 2))
        x = x + self.ff_scale * self.feed_forward(self.norm_ff(x))
        return self.norm_final(x)


def draw_module(mod, seed):
    """conformer_reference.draw_module's distributions, for modules that may
    have a Linear without a bias (linear_pos) and pos_bias_u / v (U(+-0.5))."""
    g = torch.Generator().manual_seed(seed)
    uni = lambda t, lo, hi: t.copy_(torch.rand(t.shape, generator=g, dtype=torch.float64) * (hi - lo) + lo)  # noqa: E731
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, (torch.nn.Linear, torch.nn.Conv1d)):
                uni(m.weight, -m.weight[0].numel() ** -0.5, m.weight[0].numel() ** -0.5)
                if m.bias is not None:
                    uni(m.bias, -0.1, 0.1)
            elif isinstance(m, torch.nn.MultiheadAttention):
                uni(m.in_proj_weight, -m.embed_dim ** -0.5, m.embed_dim ** -0.5)
                uni(m.in_proj_bias, -0.1, 0.1)
            elif isinstance(m, torch.nn.LayerNorm):
                uni(m.weight, 0.5, 1.5)
                uni(m.bias, -0.1, 0.1)
            elif isinstance(m, arr.RelPositionAttention):
                uni(m.pos_bias_u, -0.5, 0.5)
                uni(m.pos_bias_v, -0.5, 0.5)
    return mod


def make_block(shape, rel=False, macaron=True, seed=0):
    T, B, E, heads, units, k, km = shape
    return draw_module(EBranchformerBlock(E, heads, units, k, km, rel, macaron), 1000 * E + 10 * k + seed)


def on_own_frames(mod, x, lengths, window=None, dtype=torch.float64):
    """mod (batch-first, float64 by default) on each utterance's own frames of
    time-major x: [T][B][E] float64, zeros past its length."""
    m = copy.deepcopy(mod).to(dtype)
    T, B, E = x.shape
    out = np.zeros((T, B, E))
    with torch.no_grad():
        for b, n in enumerate(lengths):
            if n:
                xu = torch.from_numpy(x[:n, b][None]).to(dtype)
                args = () if window is None else (torch.from_numpy(ar.mask_matrix(n, n, n, *window)),)
                out[:n, b] = m(xu, *args)[0].double().numpy()
    return out
