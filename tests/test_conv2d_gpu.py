"""GPU numerics of the Conv2d layer and the subsampling front end
(asr_conv2d_fwd / asr.Conv2d / asr.Conv2dSubsampling).

Reference: conv2d_reference.py (float64, itself checked against
torch.nn.functional.conv2d in test_conv2d_cpu.py).  Bound: the project's
Conv1d bound, |err| <= 2e-5 * (1 + |ref|) (measured worst there 1.7e-6 at
K = 2816; the largest K here is 2304).  Inputs as the Conv1d tests draw them:
x U(+-1), W U(+-1/sqrt(K)), b U(+-0.1).  Each case prints its max error.

The shapes (conv2d_reference.DENSE_SHAPES / DEPTHWISE_SHAPES) are the smallest
at which each mechanism can go wrong; the boundary each reaches is written
beside it there.  Bit-independence cases compare with np.array_equal, nothing
waived.
"""
import functools

import numpy as np
import pytest
import torch

import conformer_reference as cf
import conv1d_reference as cr
import conv2d_reference as c2
from conftest import asr

pytestmark = pytest.mark.gpu
ATOL = 2e-5
SENT = -12345.0
ACTS = [(None, 20.0), ("relu", 20.0), ("clip", 0.5)]   # a clip small enough that it bites

# bit-independence runs: the scalar path (c_in 1 and 5) and the 16-byte path (c_in 12, 4, 8), one column tile
# and several, rows that straddle frames and utterances, and the three depthwise shapes
BIT_SHAPES = [c2.DENSE_SHAPES[i] for i in (0, 1, 2, 4, 5)] + c2.DEPTHWISE_SHAPES


class View:
    """rows x cols floats at a device address that something else owns."""

    def __init__(self, ptr, rows, cols, keep):
        self.ptr, self.rows, self.cols, self._keep = ptr, rows, cols, keep


def dm(a):
    return asr.DeviceMatrix.from_numpy(np.asarray(a, np.float32))


def close(got, ref, what=""):
    ref = np.asarray(ref, np.float64)
    err = np.abs(np.asarray(got, np.float64) - ref)
    print(f"{what} max err {err.max():.3e} (max err / (1 + |ref|) {(err / (1 + np.abs(ref))).max():.3e})")
    assert np.all(np.isfinite(got))
    assert np.all(err <= ATOL * (1.0 + np.abs(ref))), f"{what} max err {err.max()}"


@functools.lru_cache(maxsize=None)
def inputs(shape):
    x, W, b = c2.draw(shape)
    for a in (x, W, b):
        a.setflags(write=False)
    return x, W, b


@functools.lru_cache(maxsize=None)
def reference(shape, bias, act, clip, lengths=None):
    x, W, b = inputs(shape)
    T, B, F, ci, co, kt, kf, st, sf, ptl, pth, pfl, pfh, g = shape
    out, oln = c2.conv2d_ref(x, W, b if bias else None, st, sf, (ptl, pth), (pfl, pfh), g, act, clip, lengths)
    out.setflags(write=False)
    return out, oln


def make_desc(shape, act=None, clip=20.0, ptl=None):
    T, B, F, ci, co, kt, kf, st, sf, ptl0, pth, pfl, pfh, g = shape
    return asr.conv2d_desc(ci, co, F, kt, kf, st, sf, ptl0 if ptl is None else ptl, pth, pfl, pfh, g, act, clip)


def run(shape, x, W, b, act=None, clip=20.0, lengths=None, ldx=None, ldo=None, misalign=False, desc=None,
        extra_rows=0):
    """asr_conv2d_fwd on x [T][B][F][c_in]; returns (out [T_out][B][F_out][c_out] float32, out_lengths or
    None, the columns of out past the content [T_out][B][...], the extra_rows rows allocated past out's).
    ldx / ldo: row strides (the extra columns of x hold NaN, of out a sentinel); misalign: x starts 4
    bytes past a 16-byte boundary."""
    T, B, F, ci = x.shape
    co = shape[4]
    desc = desc or make_desc(shape, act, clip)
    ldx = ldx or F * ci
    xh = np.full((T * B, ldx), np.nan, np.float32)
    xh[:, :F * ci] = x.reshape(T * B, F * ci)
    if misalign:
        flat = np.concatenate([np.zeros(1, np.float32), xh.reshape(-1), np.zeros(3, np.float32)])
        base = dm(flat.reshape(-1, 1))
        dx = View(base.ptr + 4, T * B, ldx, base)
        assert dx.ptr % 16 == 4
    else:
        dx = dm(xh)
        assert dx.ptr % 16 == 0
    T_out, F_out = asr.conv2d_out_frames(desc, T), asr.conv2d_out_feats(desc)
    assert T_out > 0 and F_out > 0
    ldo = ldo or F_out * co
    whole = dm(np.full(((T_out * B + extra_rows), ldo), SENT, np.float32))
    out = View(whole.ptr, T_out * B, ldo, whole)
    ln = None if lengths is None else asr.device_lengths(lengths)
    oln = None if lengths is None else asr.DeviceBytes(4 * B)
    asr.conv2d_fwd(dx, dm(W.reshape(-1, co)), None if b is None else dm(b.reshape(-1, 1)), out, T, B, desc,
                   lengths=ln, out_lengths=oln)
    asr.synchronize()
    got = whole.toCpu()
    body = got[:T_out * B].reshape(T_out, B, ldo)
    return (body[:, :, :F_out * co].reshape(T_out, B, F_out, co), None if oln is None else asr.device_int32(oln, B),
            body[:, :, F_out * co:], got[T_out * B:])


@pytest.mark.parametrize("act,clip", ACTS, ids=["none", "relu", "clip"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", c2.ALL_SHAPES, ids=c2.ids)
def test_conv2d_values(shape, bias, act, clip):
    x, W, b = inputs(shape)
    ref, _ = reference(shape, bias, act, clip)
    got, _, _, _ = run(shape, x, W, b if bias else None, act, clip)
    assert got.shape == ref.shape
    close(got, ref, f"conv2d {c2.ids(shape)}")


@pytest.mark.parametrize("shape", c2.ALL_SHAPES, ids=c2.ids)
def test_conv2d_lengths(shape):
    """Ragged lengths with one utterance of zero frames and NaN in the padding rows of
    x: finite, within the bound, exact zeros past out_frames(len), d_out_lengths equal
    to the formula, nothing written past out's rows."""
    B = shape[1]
    x, W, b = inputs(shape)
    ln = c2.ragged_lengths(shape)
    assert 0 in ln
    ref, roln = reference(shape, True, "relu", 20.0, ln)
    got, oln, _, past = run(shape, c2.nan_past_lengths(x, ln), W, b, "relu", lengths=ln, extra_rows=3)
    assert np.array_equal(oln, roln)
    assert [int(v) for v in oln] == [c2.out_frames(shape, n) for n in ln]
    for bi in range(B):
        assert not got[oln[bi]:, bi].any(), bi
    assert np.all(past == SENT)
    close(got, ref, f"conv2d lengths {c2.ids(shape)}")


def test_conv2d_lengths_clamped():
    """Lengths outside [0, T] clamp: negative is 0, above T is T."""
    shape = c2.DENSE_SHAPES[1]
    T = shape[0]
    x, W, b = inputs(shape)
    got, oln, _, _ = run(shape, x, W, b, lengths=(-3, T + 5, 4))
    ref, roln = reference(shape, True, None, 20.0, (0, T, 4))
    assert np.array_equal(oln, roln)
    close(got, ref, "clamped lengths")


# ------------------------------------------------------- bit-independence
@pytest.mark.parametrize("shape", [cr.ALL_SHAPES[1], cr.ALL_SHAPES[2], cr.ALL_SHAPES[11], cr.ALL_SHAPES[0],
                                   cr.ALL_SHAPES[7]], ids=lambda sh: "x".join(map(str, sh)))
def test_feat_1_is_conv1d_bit_for_bit(shape):
    """feat_in = 1, kernel_f = 1, no frequency padding == asr_conv1d_fwd (dilation 1),
    on Conv1d's own shapes: scalar path, 16-byte path, depthwise, and two whose taps all fit
    one stage (k 3 x c_in 4 on the 16-byte path, k 2 x c_in 1 on the scalar path): the
    one-stage route against Conv1d's tap-by-tap kernel."""
    T, B, ci, co, k, s, d, pl, pr, g = shape
    d = 1                                              # Conv2d has no dilation: both run with dilation 1
    x, W, b = cr.draw(shape)
    ln = cr.ragged_lengths(shape)
    d1 = asr.conv1d_desc(ci, co, k, s, d, pl, pr, g, "relu")
    T_out = asr.conv1d_out_frames(d1, T)
    o1, l1 = dm(np.full((T_out * B, co), SENT, np.float32)), asr.DeviceBytes(4 * B)
    dx, dW, db, dl = dm(c2.nan_past_lengths(x, ln).reshape(T * B, ci)), dm(W.reshape(-1, co)), dm(b.reshape(-1, 1)), \
        asr.device_lengths(ln)
    asr.conv1d_fwd(dx, dW, db, o1, T, B, d1, lengths=dl, out_lengths=l1)
    d2 = asr.conv2d_desc(ci, co, 1, k, 1, s, 1, pl, pr, 0, 0, g, "relu")
    assert asr.conv2d_out_frames(d2, T) == T_out and asr.conv2d_out_feats(d2) == 1
    o2, l2 = dm(np.full((T_out * B, co), SENT, np.float32)), asr.DeviceBytes(4 * B)
    asr.conv2d_fwd(dx, dW, db, o2, T, B, d2, lengths=dl, out_lengths=l2)
    asr.synchronize()
    assert np.array_equal(asr.device_int32(l1, B), asr.device_int32(l2, B))
    a1, a2 = o1.toCpu(), o2.toCpu()
    assert np.any(a1 > 0) and np.all(np.isfinite(a1))
    assert np.array_equal(a1, a2)


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=c2.ids)
def test_bits_do_not_depend_on_the_batch(shape):
    """One utterance alone (B = 1) == the same utterance at two positions of a ragged batch of 5."""
    T = shape[0]
    B = 5
    big = (T, B) + shape[2:]
    x5 = c2.draw(big, seed=3)[0]
    _, W, b = inputs(shape)
    n = max(T - 2, min(T, shape[5]))                 # a length of its own, the others ragged around it
    ln = [T, n, 0, n, max(T - 1, 1)]
    x5[:, 3] = x5[:, 1]
    got, oln, _, _ = run(big, c2.nan_past_lengths(x5, ln), W, b, "relu", lengths=tuple(ln))
    alone, aoln, _, _ = run(big, c2.nan_past_lengths(x5[:, 1:2], [n]), W, b, "relu", lengths=(n,))
    assert aoln[0] == oln[1] == oln[3] and aoln[0] > 0
    assert np.array_equal(got[:, 1], alone[:, 0])
    assert np.array_equal(got[:, 3], alone[:, 0])


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=c2.ids)
def test_bits_do_not_depend_on_strides(shape):
    """ldx = F c_in + 1 and ldo = F_out c_out + 3 against contiguous buffers; the
    untouched columns keep their sentinel (x's extra column holds NaN)."""
    F, ci = shape[2], shape[3]
    x, W, b = inputs(shape)
    ln = c2.ragged_lengths(shape)
    a, _, _, _ = run(shape, x, W, b, lengths=ln)
    s, _, tail, past = run(shape, x, W, b, lengths=ln, ldx=F * ci + 1, ldo=c2.out_feats(shape) * shape[4] + 3,
                           extra_rows=2)
    assert tail.shape[2] == 3 and np.all(tail == SENT) and np.all(past == SENT)
    assert np.array_equal(s, a)


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=c2.ids)
def test_bits_do_not_depend_on_alignment(shape):
    """A d_x 4 bytes past a 16-byte boundary against an aligned one."""
    x, W, b = inputs(shape)
    a, _, _, _ = run(shape, x, W, b)
    m, _, _, _ = run(shape, x, W, b, misalign=True)
    assert np.array_equal(a, m)


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=c2.ids)
def test_length_zero_is_a_data_zero(shape):
    """Frames zeroed by a length (NaN in the buffer) == the same frames truly
    zero with full lengths, on every row the utterance still produces."""
    T, B = shape[0], 4
    big = (T, B) + shape[2:]
    x = c2.draw(big, seed=5)[0]
    _, W, b = inputs(shape)
    ln = (T, max(T - 1, 1), max(T - 3, 1), 0)
    cut, oln, _, _ = run(big, c2.nan_past_lengths(x, ln), W, b, lengths=ln)
    xz = x.copy()
    for bi, n in enumerate(ln):
        xz[n:, bi] = 0.0
    full, _, _, _ = run(big, xz, W, b)
    assert oln.max() > 0 and oln[1] > 0
    for bi in range(B):
        assert np.array_equal(cut[:oln[bi], bi], full[:oln[bi], bi]), bi


# ---------------------------------------------------------------- streaming
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("groups", [1, 20], ids=["dense", "depthwise"])
def test_causal_streaming_chunks(groups, s):
    """A causal layer (pad_t_lo = kernel_t - 1, pad_t_hi = 0) over T = 24 in one call
    == chunks [0, 10) and [10, 24), each with its kernel_t - 1 history frames
    prepended and pad_t_lo = 0, bit for bit."""
    T, B, F, kt, kf = 24, 3, 7, 3, 3
    ci = 20
    co = 24 if groups == 1 else ci
    hist = kt - 1
    whole_shape = (T, B, F, ci, co, kt, kf, s, 2, hist, 0, 1, 1, groups)
    x, W, b = c2.draw(whole_shape)
    whole, _, _, _ = run(whole_shape, x, W, b, "relu")
    assert whole.shape[0] == (T - 1) // s + 1
    xh = np.concatenate([np.zeros((hist, B, F, ci), np.float32), x])    # frame t at row t + hist
    parts = []
    for lo, hi in ((0, 10), (10, 24)):
        assert lo % s == 0
        chunk = np.ascontiguousarray(xh[lo:hi + hist])
        got, _, _, _ = run(whole_shape, chunk, W, b, "relu", desc=make_desc(whole_shape, "relu", ptl=0))
        assert got.shape[0] == (hi - lo - 1) // s + 1
        parts.append(got)
    assert np.array_equal(np.concatenate(parts), whole)
    ref, _ = c2.conv2d_ref(x, W, b, s, 2, (hist, 0), (1, 1), groups, "relu")
    close(whole, ref, "causal")


# ------------------------------------------------------------------ modules
def ragged3(T):
    return (T, 0, max(T - 7, 1))


@pytest.mark.parametrize("name", c2.STAND_INS)
def test_subsampling_stand_ins(name):
    """The five stand-in modules at F 20, C 8, E 16 (the ESPnet ones use E for both), T 30, B 3 ragged with one
    empty utterance and NaN past the lengths, against the float64 module on each utterance alone."""
    F, E, T, B = 20, 16, 30, 3
    C = E if name.startswith("espnet") else 8
    mod, conv, lin, scale = c2.make_stand_in(name, F, C, E)
    sub = asr.Conv2dSubsampling.from_torch(conv, lin, F, scale)
    x = np.random.default_rng(21).uniform(-1, 1, (T, B, F)).astype(np.float32)
    ln = ragged3(T)
    out, T_out, oln = sub.forward(dm(c2.nan_past_lengths(x, ln).reshape(T * B, F)), T, B, lengths=ln)
    asr.synchronize()
    assert T_out == sub.frames(T) == mod.length(T) and (out.rows, out.cols) == (T_out * B, E)
    ref, counts = c2.stand_in_ref(mod, x, ln, T_out, E)
    assert [int(v) for v in asr.device_int32(oln, B)] == counts == [sub.frames(n) for n in ln]
    got = out.toCpu().reshape(T_out, B, E)
    for bi, n in enumerate(counts):
        assert not got[n:, bi].any(), bi
    close(got, ref, name)
    # without lengths every row is computed, and zero_padding=False leaves the Linear's bias past the counts
    full, _, none = sub.forward(dm(x.reshape(T * B, F)), T, B)
    assert none is None
    ref_full, _ = c2.stand_in_ref(mod, x, (T,) * B, T_out, E)
    close(full.toCpu().reshape(T_out, B, E), ref_full, name + " without lengths")
    with pytest.raises(ValueError):
        sub.forward(dm(x.reshape(T * B, F)), T + 1, B)
    with pytest.raises(ValueError):
        sub.forward(dm(x.reshape(T * B, F)[:, :F - 1]), T, B)


def test_conv2d_from_torch_batchnorm_clip():
    """Conv2d.from_torch with a folded BatchNorm2d and Hardtanh(0, 20), DeepSpeech2's first layer in small."""
    torch.manual_seed(31)
    T, B, F, ci, co = 19, 3, 13, 1, 6
    conv = torch.nn.Conv2d(ci, co, (5, 7), stride=(2, 2), padding=(2, 3))
    bn = torch.nn.BatchNorm2d(co)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(co) * 0.3)
        bn.running_var.copy_(torch.rand(co) * 2 + 0.2)
        bn.weight.copy_(torch.rand(co) + 0.5)
        bn.bias.copy_(torch.randn(co) * 0.2)
    bn.eval()
    layer = asr.Conv2d.from_torch(conv, bn, act="clip", clip=20.0, feat_in=F)
    x = np.random.default_rng(2).uniform(-1, 1, (T, B, F)).astype(np.float32)
    ln = (T, 0, 8)
    out, T_out, oln = layer.forward(dm(c2.nan_past_lengths(x, ln).reshape(T * B, F)), T, B, lengths=ln)
    asr.synchronize()
    Fo = layer.feat_out
    got = out.toCpu().reshape(T_out, B, Fo, co)
    ref = np.zeros((T_out, B, Fo, co))
    cd, bd = conv.double(), bn.double()
    with torch.no_grad():
        for bi, n in enumerate(ln):
            if n:
                y = torch.nn.functional.hardtanh(bd(cd(torch.from_numpy(x[:n, bi].astype(np.float64))[None, None])), 0., 20.)
                ref[:y.shape[2], bi] = y[0].permute(1, 2, 0).numpy()
    assert [int(v) for v in asr.device_int32(oln, B)] == [layer.out_frames(n) for n in ln]
    close(got, ref, "Conv2d+BN+clip")


def test_subsampling_then_conformer_layer():
    """Conv2dSubsampling -> ConformerLayer with the device out_lengths passed on unchanged, against the torch
    chain in float64 on each utterance's own frames."""
    F, E, heads, FF, k, T, B = 20, 16, 2, 32, 7, 41, 3
    mod, conv, lin, scale = c2.make_stand_in("espnet4", F, E, E, seed=7)
    sub = asr.Conv2dSubsampling.from_torch(conv, lin, F, scale)
    T1 = sub.frames(T)
    block = cf.make_block((T1, B, E, heads, FF, k))
    layer = asr.ConformerLayer.from_torch(**block.explicit_parts())
    x = np.random.default_rng(23).uniform(-1, 1, (T, B, F)).astype(np.float32)
    ln = (T, 9, 30)
    h, T_out, ln1 = sub.forward(dm(c2.nan_past_lengths(x, ln).reshape(T * B, F)), T, B, lengths=ln)
    y = layer.forward(h, T_out, B, lengths=ln1)
    asr.synchronize()
    assert T_out == T1
    oln = [sub.frames(n) for n in ln]
    assert [int(v) for v in asr.device_int32(ln1, B)] == oln and min(oln) >= 1
    got = y.toCpu().reshape(T1, B, E)
    b64 = block.double()
    with torch.no_grad():
        for bi, n in enumerate(ln):
            f = mod(torch.from_numpy(x[:n, bi].astype(np.float64))[None])[0][:, None, :]      # [n1][1][E]
            assert f.shape[0] == oln[bi]
            close(got[:oln[bi], bi], b64(f)[:, 0].numpy(), f"chain utterance {bi}")
            assert not got[oln[bi]:, bi].any()
