"""float64 restatement of asr_conv2d_fwd in the library's layout (no device
code): x [T][B][F][c_in] time-major (a row of the device matrix is the last
two axes flattened), W [kt][kf][c_in/groups][c_out], bias [c_out] or None,
lengths [B] or None, act None / 'relu' / 'clip'; each utterance on its own
frames.  Also torch stand-ins of the toolkits' subsampling modules, written
from their published definitions (ESPnet / WeNet Conv2dSubsampling4 / 6 / 8,
NeMo ConvSubsampling 'striding' and 'dw_striding'); the toolkits themselves
are not used.  Shared by test_conv2d_cpu.py (which checks the restatement
against torch.nn.functional.conv2d) and test_conv2d_gpu.py (which checks the
device against both)."""
import numpy as np
import torch

# (T, B, F, c_in, c_out, kt, kf, st, sf, pad_t_lo, pad_t_hi, pad_f_lo, pad_f_hi, groups).  The dense kernel
# tiles 128 flat output rows (t', b, f') x 64 output columns and stages 32 elements of a tap's run of
# kf * c_in floats at a time (16-byte loads when c_in % 4 == 0 and the rows are aligned); each shape is
# the smallest that reaches the boundary named beside it.
DENSE_SHAPES = [
    (9, 2, 9, 1, 8, 3, 3, 2, 2, 0, 0, 0, 0, 1),        # first layer: scalar path, run of 3 (all taps in one stage)
    (9, 3, 11, 5, 20, 3, 3, 2, 2, 0, 0, 0, 0, 1),      # c_in % 4 != 0, partial column tile
    (7, 2, 6, 12, 16, 3, 3, 1, 1, 1, 1, 1, 1, 1),      # run 36: a second, partial stage; frequency-edge zeros in a group of 4
    (6, 5, 9, 32, 80, 1, 1, 1, 1, 0, 0, 0, 0, 1),      # pointwise, run = one stage; M = 270: three row tiles; two column tiles
    (12, 3, 14, 4, 64, 5, 5, 3, 3, 0, 0, 0, 0, 1),     # Conv2dSubsampling6's second layer, vector path
    (8, 17, 5, 8, 130, 3, 2, 2, 1, 2, 0, 0, 1, 1),     # causal time pad, non-square kernel, asymmetric frequency pad, 3 column tiles
    (5, 2, 3, 16, 16, 3, 3, 2, 2, 1, 1, 1, 1, 1),      # F_out = 2
    (10, 4, 19, 64, 64, 3, 3, 2, 2, 0, 0, 0, 0, 1),    # six full stages per tap
    (7, 2, 7, 256, 256, 3, 3, 2, 2, 0, 0, 0, 0, 1),    # the workload's own K = 2304 at M = 18
]
# depthwise: lanes across 64 channels, 32 flat output positions per workgroup
DEPTHWISE_SHAPES = [
    (9, 2, 9, 19, 19, 3, 3, 2, 2, 1, 1, 1, 1, 19),     # a partial lane group of channels
    (8, 3, 12, 64, 64, 3, 3, 2, 2, 0, 0, 0, 0, 64),    # 64 channels
    (6, 2, 5, 130, 130, 5, 3, 1, 2, 4, 0, 1, 1, 130),  # non-square kernel, causal time pad
]
ALL_SHAPES = DENSE_SHAPES + DEPTHWISE_SHAPES


def ids(shape):
    return "x".join(map(str, shape))


def count(n, k, s, lo, hi):
    """Positions out for n positions in (dilation 1): out_frames on the time axis, out_feats on the other."""
    if n <= 0 or n + lo + hi < k:
        return 0
    return (n + lo + hi - k) // s + 1


def out_frames(shape, n):
    T, B, F, ci, co, kt, kf, st, sf, ptl, pth, pfl, pfh, g = shape
    return count(n, kt, st, ptl, pth)


def out_feats(shape):
    T, B, F, ci, co, kt, kf, st, sf, ptl, pth, pfl, pfh, g = shape
    return count(F, kf, sf, pfl, pfh)


def draw(shape, seed=0):
    """x U(+-1), W U(+-1/sqrt(K)) with K = kt kf c_in / groups, b U(+-0.1); float32."""
    T, B, F, ci, co, kt, kf, st, sf, ptl, pth, pfl, pfh, g = shape
    rng = np.random.default_rng(100000 * ci + 1000 * F + 100 * kt + 10 * B + T + seed)
    cg = ci // g
    sc = 1.0 / np.sqrt(kt * kf * cg)
    x = rng.uniform(-1, 1, (T, B, F, ci)).astype(np.float32)
    W = rng.uniform(-sc, sc, (kt, kf, cg, co)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, co).astype(np.float32)
    return x, W, b


def ragged_lengths(shape):
    """Lengths that include T, one utterance of zero frames and (B >= 3) others in [1, T]."""
    T, B = shape[0], shape[1]
    ln = np.random.default_rng(T * B + shape[5]).integers(1, T + 1, B)
    ln[0], ln[B - 1] = T, 0
    if B >= 4:
        ln[1] = 1
    return tuple(int(v) for v in ln)


def activation(v, act, clip):
    if act == "relu":
        return np.maximum(v, 0.0)
    if act == "clip":
        return np.minimum(np.maximum(v, 0.0), clip)
    assert act is None, act
    return v


def conv2d_ref(x, W, b, st, sf, pad_t, pad_f, groups=1, act=None, clip=20.0, lengths=None):
    """(out [T_out][B][F_out][c_out] float64, out_lengths [B]): rows past
    out_frames(len_b) are zeros; frames of x at or past len_b are never read."""
    x = np.asarray(x)
    T, B, F, ci = x.shape
    W = np.asarray(W, np.float64)
    kt, kf, cg, co = W.shape
    (ptl, pth), (pfl, pfh) = pad_t, pad_f
    assert cg == ci // groups and (groups == 1 or groups == ci == co)
    T_out, F_out = count(T, kt, st, ptl, pth), count(F, kf, sf, pfl, pfh)
    out = np.zeros((T_out, B, F_out, co), np.float64)
    oln = np.zeros(B, np.int64)
    for bi in range(B):
        n = T if lengths is None else min(max(int(lengths[bi]), 0), T)
        no = count(n, kt, st, ptl, pth)
        oln[bi] = no
        if no == 0 or F_out == 0:
            continue
        xp = np.zeros((ptl + n + pth, pfl + F + pfh, ci), np.float64)
        xp[ptl:ptl + n, pfl:pfl + F] = x[:n, bi].astype(np.float64)
        acc = np.zeros((no, F_out, co), np.float64)
        for jt in range(kt):
            for jf in range(kf):
                win = xp[jt:jt + (no - 1) * st + 1:st, jf:jf + (F_out - 1) * sf + 1:sf]      # [no][F_out][ci]
                acc += win * W[jt, jf, 0] if groups != 1 else win @ W[jt, jf]
        if b is not None:
            acc += np.asarray(b, np.float64)
        out[:no, bi] = activation(acc, act, clip)
    return out, oln


def nan_past_lengths(x, lengths):
    x = x.copy()
    for b, n in enumerate(lengths):
        x[max(n, 0):, b] = np.nan
    return x


# ------------------------------------------------------------- torch stand-ins
class EspnetSubsampling(torch.nn.Module):
    """ESPnet / WeNet Conv2dSubsampling4 / 6 / 8: unpadded Conv2d + ReLU layers
    on [B][1][T][idim], then Linear over the (c, f) axis flattened c-major, then
    the positional encoding's x * sqrt(odim) (the encoding itself is added
    elsewhere).  The Linear is .out[0] as in the toolkits."""
    SPECS = {4: ((3, 2), (3, 2)), 6: ((3, 2), (5, 3)), 8: ((3, 2), (3, 2), (3, 2))}

    def __init__(self, factor, idim, odim):
        super().__init__()
        self.specs = self.SPECS[factor]
        mods, c, f = [], 1, idim
        for k, s in self.specs:
            mods += [torch.nn.Conv2d(c, odim, k, s), torch.nn.ReLU()]
            c, f = odim, (f - k) // s + 1
        self.conv = torch.nn.Sequential(*mods)
        self.out = torch.nn.Sequential(torch.nn.Linear(odim * f, odim))
        self.xscale = float(odim) ** 0.5

    def forward(self, x):                      # [B][T][idim]
        x = self.conv(x.unsqueeze(1))
        b, c, t, f = x.size()
        return self.out(x.transpose(1, 2).contiguous().view(b, t, c * f)) * self.xscale

    def length(self, n):
        """What the toolkits' mask slicing mask[:, :, :-(k-1):s] per layer keeps of n frames."""
        for k, s in self.specs:
            n = len(range(n)[:-(k - 1):s])
        return n


class NemoSubsampling(torch.nn.Module):
    """NeMo ConvSubsampling, subsampling_factor 4, 'striding' (Conv2d k 3 s 2
    padding 1 + ReLU, twice) or 'dw_striding' (the first layer the same, then
    depthwise Conv2d k 3 s 2 padding 1 groups C -> pointwise Conv2d k 1 -> ReLU);
    .conv the Sequential, .out the Linear over the (c, f) axis flattened c-major."""

    def __init__(self, kind, feat_in, feat_out, channels):
        super().__init__()
        C = channels
        mods = [torch.nn.Conv2d(1, C, 3, 2, 1), torch.nn.ReLU()]
        if kind == "striding":
            mods += [torch.nn.Conv2d(C, C, 3, 2, 1), torch.nn.ReLU()]
        else:
            assert kind == "dw_striding"
            mods += [torch.nn.Conv2d(C, C, 3, 2, 1, groups=C), torch.nn.Conv2d(C, C, 1, 1, 0), torch.nn.ReLU()]
        self.conv = torch.nn.Sequential(*mods)
        f = feat_in
        for _ in range(2):
            f = (f + 2 - 3) // 2 + 1
        self.out = torch.nn.Linear(C * f, feat_out)

    def forward(self, x):                      # [B][T][feat_in]
        x = self.conv(x.unsqueeze(1))
        b, c, t, f = x.size()
        return self.out(x.transpose(1, 2).reshape(b, t, c * f))

    def length(self, n):
        """NeMo's calc_length: floor((n + 2 - 3) / 2 + 1), twice."""
        for _ in range(2):
            n = (n + 2 - 3) // 2 + 1
        return n


STAND_INS = ["espnet4", "espnet6", "espnet8", "nemo_striding", "nemo_dw_striding"]


def make_stand_in(name, feat_in, channels, E, seed=0):
    """(module in float64 with drawn parameters, its Sequential, its Linear, the scale after it)."""
    torch.manual_seed(1000 + seed + STAND_INS.index(name))
    if name.startswith("espnet"):
        assert channels == E, "the ESPnet modules use odim for both"
        m = EspnetSubsampling(int(name[6:]), feat_in, E)
        lin, scale = m.out[0], m.xscale
    else:
        m = NemoSubsampling(name[5:], feat_in, E, channels)
        lin, scale = m.out, 1.0
    m = m.double().eval()
    with torch.no_grad():
        for p in m.parameters():
            if p.ndim == 1:
                p.uniform_(-0.1, 0.1)
    return m, m.conv, lin, scale


def stand_in_ref(mod, x, lengths, T_out, E):
    """The float64 module on each utterance's own frames: [T_out][B][E], zeros past its count
    (an utterance too short for the first kernel has no frames)."""
    out = np.zeros((T_out, x.shape[1], E))
    counts = []
    with torch.no_grad():
        for bi, n in enumerate(lengths):
            no = mod.length(n) if n > 0 else 0
            no = max(no, 0)
            counts.append(no)
            if no == 0:
                continue
            y = mod(torch.from_numpy(x[:n, bi].astype(np.float64))[None])[0].numpy()
            assert y.shape == (no, E), (y.shape, no)
            out[:no, bi] = y
    return out, counts
