"""References for the Conformer tests (no device code): a float64 numpy
restatement of asr_glu_dwconv_fwd in the library's layout, a small torch
Conformer block written from the description of asr.ConformerLayer (its
attribute names are those of torchaudio's ConformerLayer, so it doubles as the
stand-in for ConformerLayer.from_torchaudio), draw helpers and the shape lists.
Shared by test_conformer_cpu.py (which checks the restatement against
torch.nn.functional.glu / conv1d / silu in float64) and test_conformer_gpu.py
(which checks the device against both)."""
import copy

import numpy as np
import torch

import attention_reference as ar

MAX_KERNEL = 80   # ASR_GLU_DWCONV_MAX_KERNEL

# (T, B, C, k, pad_left, pad_right).  The kernel tiles 64 channels x 64 output
# frames of one utterance and stages 64 + k - 1 gated frames and k taps in LDS
# for every k it takes (there is no second path).
GLU_SHAPES = [
    (8, 4, 1, 1, 0, 0),              # everything minimal
    (9, 3, 19, 3, 1, 1),             # one partial channel block
    (40, 3, 64, 15, 7, 7),           # one exact channel block
    (70, 5, 144, 31, 15, 15),        # three channel blocks, the last partial; two frame blocks (70 > 64)
    (12, 2, 72, 31, 15, 15),         # T < k
    (50, 4, 130, 15, 14, 0),         # causal
    (33, 6, 80, 4, 1, 2),            # even k, asymmetric
    (64, 2, 20, 5, 2, 2),            # exactly one frame block
    (129, 2, 8, 3, 2, 0),            # three frame blocks, the last of one frame; causal
    (90, 2, 70, MAX_KERNEL, 39, 40),  # the longest supported k: the largest LDS tile, two frame blocks
    (70, 2, 33, MAX_KERNEL, MAX_KERNEL - 1, 0),   # the longest k, causal
]
CAUSAL_SHAPES = [s for s in GLU_SHAPES if s[5] == 0 and s[3] > 1]
ACTS = [None, "relu", "silu"]

# ConformerLayer: (T, B, E, heads, F, k)
LAYER_SHAPES = [(70, 5, 144, 4, 288, 15), (40, 3, 64, 4, 128, 31)]
WINDOWS = {"full": (1, -1, -1), "chunked": (16, 2, 0)}


def ids(shape):
    return "x".join(map(str, shape))


def draw_glu(shape, seed=0):
    """u [T][B][2C] U(+-1), w [k][C] U(+-1/sqrt(k)), b [C] U(+-0.1); float32."""
    T, B, C, k, pl, pr = shape
    rng = np.random.default_rng(100000 * k + 1000 * C + 10 * T + B + seed)
    u = rng.uniform(-1, 1, (T, B, 2 * C)).astype(np.float32)
    w = (rng.uniform(-1, 1, (k, C)) / np.sqrt(k)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, C).astype(np.float32)
    return u, w, b


def glu_lengths(shape):
    """1, T and one > T (it clamps to T) always; 0 and others below T as B allows."""
    T, B = shape[0], shape[1]
    base = [T + 3, 1, T, 0, max(T // 2, 1), min(65, T), max(T - 1, 1)]
    return tuple(base[:B])


def sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def act_ref(v, act):
    if act == "relu":
        return np.maximum(v, 0)
    if act == "silu":
        return v * sigmoid(v)
    assert act is None
    return v


def glu_dwconv_ref(u, w, b, k, pl, act=None, lengths=None):
    """[T][B][C] float64: GLU over the two halves of u's columns, a depthwise
    convolution over each utterance's own frames with zero padding (pl, k-1-pl),
    the bias, the activation; rows t >= len_b are zeros, frames past len_b of u
    are never read."""
    T, B, C2 = u.shape
    C = w.shape[1]
    assert C2 >= 2 * C and w.shape[0] == k
    w = np.asarray(w, np.float64)
    out = np.zeros((T, B, C))
    for bi in range(B):
        n = T if lengths is None else min(max(int(lengths[bi]), 0), T)
        if n == 0:
            continue
        uu = u[:n, bi].astype(np.float64)
        g = np.zeros((n + k - 1, C))
        g[pl:pl + n] = uu[:, :C] * sigmoid(uu[:, C:2 * C])
        acc = np.zeros((n, C))
        for j in range(k):
            acc += g[j:j + n] * w[j]
        if b is not None:
            acc = acc + np.asarray(b, np.float64)
        out[:n, bi] = act_ref(acc, act)
    return out


def nan_past_lengths(x, lengths):
    x = x.copy()
    for b, n in enumerate(lengths):
        x[max(n, 0):, b] = np.nan
    return x


# ------------------------------------------------------------- torch block
class FeedForward(torch.nn.Module):
    """LayerNorm -> Linear -> SiLU -> Linear (dropouts of 0 in torchaudio's places)."""

    def __init__(self, E, F):
        super().__init__()
        self.sequential = torch.nn.Sequential(torch.nn.LayerNorm(E), torch.nn.Linear(E, F), torch.nn.SiLU(),
                                              torch.nn.Dropout(0.0), torch.nn.Linear(F, E), torch.nn.Dropout(0.0))

    def forward(self, x):
        return self.sequential(x)


class ConvModule(torch.nn.Module):
    """LayerNorm -> pointwise Conv1d to 2E -> GLU -> depthwise Conv1d -> BatchNorm1d
    -> SiLU -> pointwise Conv1d to E.  padding 'same': the depthwise convolution
    pads itself; (left, right) or 'causal': it has padding 0 and forward pads by
    hand between the GLU and the depthwise convolution."""

    def __init__(self, E, k, padding="same", norm="batch"):
        super().__init__()
        self.layer_norm = torch.nn.LayerNorm(E)
        self.manual = None if padding == "same" else (k - 1, 0) if padding == "causal" else tuple(padding)
        assert self.manual is not None or k % 2 == 1
        mid = {"batch": lambda: torch.nn.BatchNorm1d(E), "group": lambda: torch.nn.GroupNorm(1, E),
               "layer": lambda: torch.nn.LayerNorm(E)}[norm]()
        self.sequential = torch.nn.Sequential(
            torch.nn.Conv1d(E, 2 * E, 1), torch.nn.GLU(dim=1),
            torch.nn.Conv1d(E, E, k, padding=(k - 1) // 2 if self.manual is None else 0, groups=E),
            mid, torch.nn.SiLU(), torch.nn.Conv1d(E, E, 1), torch.nn.Dropout(0.0))

    def parts(self):
        s = self.sequential
        return self.layer_norm, s[0], s[2], s[3], s[5]

    def forward(self, x):                       # [B][T][E]
        x = self.layer_norm(x).transpose(1, 2)
        x = self.sequential[1](self.sequential[0](x))
        if self.manual is not None:
            x = torch.nn.functional.pad(x, self.manual)
        for m in list(self.sequential)[2:]:
            x = m(x)
        return x.transpose(1, 2)


class ConformerBlock(torch.nn.Module):
    """x + FFN1(x)/2 -> self-attention and convolution module, each with its
    residual (the convolution first if convolution_first) -> + FFN2/2 ->
    LayerNorm; time-major [T][B][E]."""

    def __init__(self, E, heads, F, k, convolution_first=False, conv_padding="same", conv_norm="batch"):
        super().__init__()
        self.ffn1 = FeedForward(E, F)
        self.self_attn_layer_norm = torch.nn.LayerNorm(E)
        self.self_attn = torch.nn.MultiheadAttention(E, heads, dropout=0.0)
        self.conv_module = ConvModule(E, k, conv_padding, conv_norm)
        self.ffn2 = FeedForward(E, F)
        self.final_layer_norm = torch.nn.LayerNorm(E)
        self.convolution_first = convolution_first

    def _conv(self, x):
        return x + self.conv_module(x.transpose(0, 1)).transpose(0, 1)

    def forward(self, x, key_padding_mask=None, attn_mask=None):
        x = self.ffn1(x) * 0.5 + x
        if self.convolution_first:
            x = self._conv(x)
        n = self.self_attn_layer_norm(x)
        a, _ = self.self_attn(n, n, n, key_padding_mask=key_padding_mask, attn_mask=attn_mask, need_weights=False)
        x = x + a
        if not self.convolution_first:
            x = self._conv(x)
        x = self.ffn2(x) * 0.5 + x
        return self.final_layer_norm(x)

    def explicit_parts(self):
        """The keywords of asr.ConformerLayer.from_torch."""
        f1, f2 = self.ffn1.sequential, self.ffn2.sequential
        return dict(ffn1=(f1[0], f1[1], f1[4]), attn=(self.self_attn_layer_norm, self.self_attn),
                    conv=self.conv_module.parts(), ffn2=(f2[0], f2[1], f2[4]), final_norm=self.final_layer_norm,
                    convolution_first=self.convolution_first)


def draw_module(mod, seed):
    """Parameters as the GPU tests draw them: weights U(+-1/sqrt(fan-in)), biases
    U(+-0.1), LayerNorm / BatchNorm gamma U(0.5, 1.5), BatchNorm running variance
    U(0.5, 1.5) and running mean U(+-0.3).  The BatchNorm goes to eval mode (the
    attention stays in training mode: no fused path, dropout is 0)."""
    g = torch.Generator().manual_seed(seed)
    uni = lambda t, lo, hi: t.copy_(torch.rand(t.shape, generator=g, dtype=torch.float64) * (hi - lo) + lo)  # noqa: E731
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, (torch.nn.Linear, torch.nn.Conv1d)):
                fan = m.weight[0].numel()
                uni(m.weight, -fan ** -0.5, fan ** -0.5)
                uni(m.bias, -0.1, 0.1)
            elif isinstance(m, torch.nn.MultiheadAttention):
                uni(m.in_proj_weight, -m.embed_dim ** -0.5, m.embed_dim ** -0.5)
                uni(m.in_proj_bias, -0.1, 0.1)
            elif isinstance(m, (torch.nn.LayerNorm, torch.nn.GroupNorm, torch.nn.BatchNorm1d)):
                uni(m.weight, 0.5, 1.5)
                uni(m.bias, -0.1, 0.1)
                if isinstance(m, torch.nn.BatchNorm1d):
                    uni(m.running_var, 0.5, 1.5)
                    uni(m.running_mean, -0.3, 0.3)
                    m.eval()
    return mod


def make_block(shape, convolution_first=False, conv_padding="same", seed=0):
    T, B, E, heads, F, k = shape
    return draw_module(ConformerBlock(E, heads, F, k, convolution_first, conv_padding),
                       1000 * E + 10 * k + int(convolution_first) + seed)


def draw_x(T, B, E, seed=0):
    return np.random.default_rng(77 * E + T + B + seed).uniform(-1, 1, (T, B, E)).astype(np.float32)


def per_utterance(fn, x, lengths, cols):
    """fn (a float64 torch function of [n][1][E] and n) on each utterance's own
    frames: [T][B][cols] float64, zeros past its length."""
    T, B = x.shape[:2]
    out = np.zeros((T, B, cols))
    with torch.no_grad():
        for b, n in enumerate(lengths):
            n = min(max(int(n), 0), T)
            if n:
                out[:n, b] = fn(torch.from_numpy(x[:n, b:b + 1].astype(np.float64)), n)[:, 0].numpy()
    return out


def block_ref(block, x, lengths, window=(1, -1, -1)):
    """The block in float64 on each utterance's own frames, the attention under
    the chunked window's mask (True = not allowed, as torch takes it)."""
    b64 = copy.deepcopy(block).double()

    def fn(xu, n):
        allowed = ar.mask_matrix(n, n, n, *window)
        return b64(xu, attn_mask=torch.from_numpy(~allowed))
    return per_utterance(fn, x, lengths, x.shape[2])


def conv_module_ref(mod, x, lengths):
    """ConvModule (without a residual) in float64 on each utterance's own frames."""
    m64 = copy.deepcopy(mod).double()
    return per_utterance(lambda xu, n: m64(xu.transpose(0, 1)).transpose(0, 1), x, lengths, x.shape[2])
