"""The Zipformer additions restated in float64 (the specification the kernels
are tested against), and a float32 torch stand-in layer that carries icefall's
attribute names and follows its forward (zipformer.py, Zipformer2, written from
memory: no icefall is installed, a real checkpoint was never loaded).

BiasNorm of a row equal to its bias: the mean square is 0, the factor +inf, so
the float64 formula gives +-inf where x != 0 and NaN where x == 0; biasnorm_ref
returns exactly that.
"""
import numpy as np
import torch

import attention_reference as ar

WINDOWS = {"full": (1, -1, -1), "chunked": (16, 2, 0)}


def rel_shift(raw):
    """raw [..., T, 2T - 1] -> [..., T, T]: out[i, j] = raw[i, T - 1 - i + j] (icefall's as_strided)."""
    T = raw.shape[-2]
    return np.take_along_axis(raw, (T - 1 - np.arange(T)[:, None] + np.arange(T)[None, :])
                              .reshape((1,) * (raw.ndim - 2) + (T, T)), -1)


def swoosh(v, kind):
    c, k = (4.0, 0.035) if kind == "l" else (1.0, 0.313261687)
    v = np.asarray(v, np.float64)
    return np.logaddexp(0.0, v - c) - 0.08 * v - k


def biasnorm_ref(x, bias, log_scale, x0=None, bypass=None, lengths=None):
    """x [T][B][N] -> float64; rows past lengths zeros."""
    x = np.asarray(x, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = x * (np.exp(np.float64(log_scale)) / np.sqrt(np.mean((x - bias) ** 2, -1, keepdims=True)))
        if x0 is not None:
            out = x0 + (out - x0) * np.asarray(bypass, np.float64)
    return zero_past(out, lengths)


def zero_past(x, lengths):
    x = np.array(x, np.float64)
    for b, n in enumerate(lengths if lengths is not None else ()):
        x[n:, b] = 0.0
    return x


def zattn_ref(q, k, v, H, G=None, pz=None, pos=None, pos_zero=0, score_head=0, mask=(1, -1, -1), lengths=None,
              scale=0.0, sg=None, y=None, q_pos0=0, k_pos0=0):
    """asr_attention_zip_fwd in float64: q [Tq][B][H dq], k [Tk][B][H dq], pz
    [Tq][B][H dp] or None, v / sg [Tk][B][G dv], y [Tq][B][G dv], pos [n_pos][H dp]."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    (Tq, B, _), Tk, G = q.shape, k.shape[0], H if G is None else G
    dq, dv = q.shape[2] // H, v.shape[2] // G
    if sg is not None:
        v = v * np.tanh(np.asarray(sg, np.float64))
    s = np.einsum("ibhd,jbhd->bhij", q.reshape(Tq, B, H, dq), k.reshape(Tk, B, H, dq))
    if pz is not None:
        dp = pz.shape[2] // H
        delta = (q_pos0 + np.arange(Tq))[:, None] - (k_pos0 + np.arange(Tk))[None, :]
        row = pos_zero - delta
        ok = (row >= 0) & (row < pos.shape[0])
        pg = np.where(ok[:, :, None], np.nan_to_num(np.asarray(pos, np.float64)[row.clip(0, pos.shape[0] - 1)]), 0.0)
        s = s + np.einsum("ibhd,ijhd->bhij", np.asarray(pz, np.float64).reshape(Tq, B, H, dp), pg.reshape(Tq, Tk, H, dp))
    s = s * (scale or 1.0 / np.sqrt(dq))
    out, seen = np.zeros((Tq, B, G * dv)), np.zeros((Tq, B, 1), bool)
    for b in range(B):
        n = Tk + k_pos0 + Tq + q_pos0 if lengths is None else lengths[b]
        allowed = ar.mask_matrix(Tq, Tk, n, *mask, q_pos0=q_pos0, k_pos0=k_pos0)
        live = seen[:, b, 0] = allowed.any(1)
        for g in range(G):
            sc = np.where(allowed[live], s[b, g if G == H else score_head][live], -np.inf)
            p = np.exp(sc - sc.max(1, keepdims=True))
            out[live, b, g * dv:(g + 1) * dv] = p / p.sum(1, keepdims=True) @ v[:, b, g * dv:(g + 1) * dv]
    return out if y is None else np.where(seen, out * np.nan_to_num(np.asarray(y, np.float64)), 0.0)


def glu_dwconv_ref(u, w, b, lengths, act):
    """u [T][B][2C] -> act(depthwise 'same' conv of value * sigmoid(gate) + b), zeros past lengths."""
    T, B, C2 = u.shape
    C, k = C2 // 2, w.shape[0]
    out = np.zeros((T, B, C))
    for bi in range(B):
        n = T if lengths is None else lengths[bi]
        g = np.zeros((n + k - 1, C))
        g[(k - 1) // 2:(k - 1) // 2 + n] = u[:n, bi, :C] / (1 + np.exp(-np.asarray(u[:n, bi, C:], np.float64)))
        out[:n, bi] = act(sum(g[j:j + n] * np.asarray(w[j], np.float64) for j in range(k)) + b)
    return out


def layer_ref(p, x, H, dq, dp, pos, pos_zero, mask=(1, -1, -1), lengths=None):
    """The layer in float64 from asr.ZipformerLayer.pack_torch's arrays; x [T][B][E]; zeros past lengths."""
    p = {key: np.asarray(a, np.float64) for key, a in p.items()}
    lin = lambda key, a, s="in": a @ p[f"{key}.w_{s}"] + p[f"{key}.b_{s}"]   # noqa: E731
    x = np.asarray(x, np.float64)
    qkp = lin("attn", x)
    q, k, pz = qkp[..., :H * dq], qkp[..., H * dq:2 * H * dq], qkp[..., 2 * H * dq:]
    kw = dict(pz=pz, pos=np.asarray(pos, np.float64) @ p["attn.w_pos"], pos_zero=pos_zero, mask=mask, lengths=lengths,
              scale=1.0)
    ff = lambda i, h: h + lin(f"ff{i}", swoosh(lin(f"ff{i}", h), "l"), "out")   # noqa: E731
    sa = lambda i, h: h + lin(f"sa{i}", zattn_ref(q, k, lin(f"sa{i}", h), H, **kw), "out")   # noqa: E731
    conv = lambda i, h: h + lin(f"conv{i}", glu_dwconv_ref(lin(f"conv{i}", h), p[f"conv{i}.wd"], p[f"conv{i}.bd"],   # noqa: E731
                                                           lengths, lambda t: swoosh(t, "r")), "out")
    h = ff(1, x)
    s, xv, y = np.split(lin("nla", h), 3, -1)
    h = h + lin("nla", zattn_ref(q, k, xv, H, 1, sg=s, y=y, **kw), "out")
    h = ff(2, conv(1, sa(1, h)))
    h = x + (h - x) * p["bypass_mid.scale"]
    h = ff(3, conv(2, sa(2, h)))
    return biasnorm_ref(zero_past(h, lengths), p["norm.bias"], p["norm.log_scale"], zero_past(x, lengths),
                        p["bypass.scale"], lengths)


# ------------------------------------------------------------- the stand-in
class _Swoosh(torch.nn.Module):
    def __init__(self, c, k):
        super().__init__()
        self.c, self.k = c, k

    def forward(self, x):
        return torch.logaddexp(torch.zeros_like(x), x - self.c) - 0.08 * x - self.k


class _ActLinear(torch.nn.Linear):
    """icefall's ActivationDropoutAndLinear: a Linear (weight, bias) behind an activation."""

    def __init__(self, i, o, act):
        super().__init__(i, o)
        self.act = _Swoosh(4.0, 0.035) if act == "SwooshL" else _Swoosh(1.0, 0.313261687)

    def forward(self, x):
        return super().forward(self.act(x))


def _mod(**kw):
    m = torch.nn.Module()
    for key, val in kw.items():
        if isinstance(val, torch.Tensor):
            val = torch.nn.Parameter(val)
        setattr(m, key, val)
    return m


class StandInLayer(torch.nn.Module):
    """Zipformer2EncoderLayer's attributes and eval-mode forward (batch-major matmuls, the rel-shift)."""

    def __init__(self, E, H, dq, dp, dv, ffs, kernel, pos_dim, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        L, hid = torch.nn.Linear, 3 * E // 4
        self.self_attn_weights = _mod(in_proj=L(E, H * (2 * dq + dp)), linear_pos=L(pos_dim, H * dp, bias=False),
                                      num_heads=H, query_head_dim=dq, pos_head_dim=dp)
        for i, F in enumerate(ffs, 1):
            setattr(self, f"feed_forward{i}", _mod(in_proj=L(E, F), out_proj=_ActLinear(F, E, "SwooshL")))
        self.nonlin_attention = _mod(in_proj=L(E, 3 * hid), out_proj=L(hid, E))
        for i in (1, 2):
            setattr(self, f"self_attn{i}", _mod(in_proj=L(E, H * dv), out_proj=L(H * dv, E)))
            setattr(self, f"conv_module{i}", _mod(in_proj=L(E, 2 * E), out_proj=_ActLinear(E, E, "SwooshR"),
                                                  depthwise_conv=torch.nn.Conv1d(E, E, kernel, groups=E,
                                                                                 padding=kernel // 2)))
        self.bypass_mid = _mod(bypass_scale=torch.rand(E) * 0.5 + 0.4)
        self.bypass = _mod(bypass_scale=torch.rand(E) * 0.5 + 0.4)
        self.norm = _mod(bias=torch.rand(E) * 0.4 - 0.2, log_scale=torch.tensor(0.3))
        for prm in self.parameters():               # livelier than the default init: biases and scores of order 1
            if prm.ndim == 1 and prm.shape[0] != E:
                prm.data.uniform_(-0.5, 0.5)
        self.eval()

    def weights(self, x, pos_emb, allowed):
        """[H][B][T][T] probabilities; x [T][B][E], pos_emb [2T - 1][pos_dim], allowed [B][T][T] bool."""
        m = self.self_attn_weights
        (T, B, _), H, dq = x.shape, m.num_heads, m.query_head_dim
        qkp = m.in_proj(x)
        q, k, p = qkp[..., :H * dq], qkp[..., H * dq:2 * H * dq], qkp[..., 2 * H * dq:]
        q, k, p = (a.reshape(T, B, H, -1).permute(2, 1, 0, 3) for a in (q, k, p))
        scores = q @ k.transpose(2, 3)
        pe = m.linear_pos(pos_emb).reshape(1, 2 * T - 1, H, -1).permute(2, 0, 3, 1)   # [H][1][dp][2T - 1]
        raw = p @ pe                                                               # [H][B][T][2T - 1]
        scores = scores + raw.as_strided((H, B, T, T), (raw.stride(0), raw.stride(1), raw.stride(2) - raw.stride(3),
                                                        raw.stride(3)), storage_offset=raw.stride(3) * (T - 1))
        return torch.softmax(scores.masked_fill(~allowed.unsqueeze(0), -1e30), -1)

    def forward(self, src, pos_emb, allowed, keep):
        """keep [T][B][1] bool: frames inside the utterance (the convolution's padding mask)."""
        T, B, E = src.shape
        w = self.weights(src, pos_emb, allowed)
        apply = lambda w, v: (w @ v.reshape(T, B, w.shape[0], -1).permute(2, 1, 0, 3)).permute(2, 1, 0, 3).reshape(T, B, -1)   # noqa: E731
        ff = lambda m, h: h + m.out_proj(m.in_proj(h))   # noqa: E731
        sa = lambda m, h: h + m.out_proj(apply(w, m.in_proj(h)))   # noqa: E731

        def conv(m, h):
            a, g = m.in_proj(h).chunk(2, dim=2)
            c = (a * torch.sigmoid(g) * keep).permute(1, 2, 0)
            return h + m.out_proj(m.depthwise_conv(c).permute(2, 0, 1))

        h = ff(self.feed_forward1, src)
        s, x, y = self.nonlin_attention.in_proj(h).chunk(3, dim=2)
        h = h + self.nonlin_attention.out_proj(apply(w[0:1], x * torch.tanh(s)) * y)
        h = ff(self.feed_forward2, conv(self.conv_module1, sa(self.self_attn1, h)))
        h = src + (h - src) * self.bypass_mid.bypass_scale
        h = ff(self.feed_forward3, conv(self.conv_module2, sa(self.self_attn2, h)))
        h = h * ((h - self.norm.bias).pow(2).mean(-1, keepdim=True) ** -0.5 * self.norm.log_scale.exp())
        return src + (h - src) * self.bypass.bypass_scale


LAYER = dict(E=48, H=2, dq=8, dp=4, dv=4, ffs=(64, 96, 128), kernel=7, pos_dim=16)
