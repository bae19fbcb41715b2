"""GPU numerics of the Conv1d layer (asr_conv1d_fwd / asr.Conv1d).

Reference: conv1d_reference.py (float64, itself checked against
torch.nn.functional.conv1d in test_conv1d_cpu.py).  Bound: the project's bound
for fp32 kernels (test_gru_gpu.py close()): |err| <= 2e-5 * (1 + |ref|).
Inputs as the recurrent-layer tests draw them: x U(+-1), W
U(+-1/sqrt(k c_in / groups)), b U(+-0.1); torch float32 on the CPU stays at or
below 3.2e-7 * (1 + |ref|) at these shapes, so the reference is far inside the
bound.  Each case prints its max error.

The shapes (conv1d_reference.DENSE_SHAPES / DEPTHWISE_SHAPES) are the smallest
at which each mechanism can go wrong: the dense kernel tiles 128 output rows x
64 output columns and stages 32 channels at a time (16-byte loads of x when
c_in % 4 == 0 and the rows are aligned), the depthwise kernel 64 channels x 64
output frames of one utterance with the input frames and taps in LDS when
63 s + (k-1) d + 1 + k <= 224 (only (30, 4, 70, 9, 4, 3, ...) is past that).
Bit-independence cases compare with np.array_equal.
"""
import functools

import numpy as np
import pytest
import torch

import conv1d_reference as cr
from conftest import asr

pytestmark = pytest.mark.gpu
ATOL = 2e-5
SENT = -12345.0
ACTS = [(None, 20.0), ("relu", 20.0), ("clip", 0.5)]   # a clip small enough that it bites

ids = lambda sh: "x".join(map(str, sh))   # noqa: E731
# bit-independence runs: c_in % 4 == 0 (the 16-byte-load path) and not, one column tile and several,
# depthwise with the input frames in LDS and from memory
BIT_SHAPES = [cr.ALL_SHAPES[1], cr.ALL_SHAPES[2], cr.ALL_SHAPES[5], cr.ALL_SHAPES[8], cr.ALL_SHAPES[9],
              cr.ALL_SHAPES[10], cr.ALL_SHAPES[11], cr.ALL_SHAPES[12]]


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
    x, W, b = cr.draw(shape)
    for a in (x, W, b):
        a.setflags(write=False)
    return x, W, b


@functools.lru_cache(maxsize=None)
def reference(shape, bias, act, clip, lengths=None):
    x, W, b = inputs(shape)
    T, B, ci, co, k, s, d, pl, pr, g = shape
    out, oln = cr.conv1d_ref(x, W, b if bias else None, k, s, d, pl, pr, g, act, clip, lengths)
    out.setflags(write=False)
    return out, oln


def make_desc(shape, act=None, clip=20.0, pl=None):
    T, B, ci, co, k, s, d, pl0, pr, g = shape
    return asr.conv1d_desc(ci, co, k, s, d, pl0 if pl is None else pl, pr, g, act, clip)


def run(shape, x, W, b, act=None, clip=20.0, lengths=None, ldx=None, ldo=None, misalign=False, desc=None):
    """asr_conv1d_fwd on x [T][B][c_in]; returns (out [T_out][B][ldo] float32, out_lengths or None).
    ldx / ldo: row strides (the extra columns of x hold NaN, of out a sentinel);
    misalign: x starts 4 bytes past a 16-byte boundary."""
    T, B, ci, co = x.shape[0], x.shape[1], shape[2], shape[3]
    desc = desc or make_desc(shape, act, clip)
    ldx = ldx or ci
    xh = np.full((T * B, ldx), np.nan, np.float32)
    xh[:, :ci] = x.reshape(T * B, ci)
    if misalign:
        flat = np.concatenate([np.zeros(1, np.float32), xh.reshape(-1), np.zeros(3, np.float32)])
        base = dm(flat.reshape(-1, 1))
        dx = View(base.ptr + 4, T * B, ldx, base)
        assert dx.ptr % 16 == 4
    else:
        dx = dm(xh)
        assert dx.ptr % 16 == 0
    T_out = asr.conv1d_out_frames(desc, T)
    assert T_out > 0
    out = dm(np.full((T_out * B, ldo or co), SENT, np.float32))
    ln = None if lengths is None else asr.device_lengths(lengths)
    oln = None if lengths is None else asr.DeviceBytes(4 * B)
    asr.conv1d_fwd(dx, dm(W.reshape(-1, co)), None if b is None else dm(b.reshape(-1, 1)), out, T, B, desc,
                   lengths=ln, out_lengths=oln)
    asr.synchronize()
    got = out.toCpu().reshape(T_out, B, -1)
    return got, (None if oln is None else asr.device_int32(oln, B))


def nan_past_lengths(x, lengths):
    x = x.copy()
    for b, n in enumerate(lengths):
        x[max(n, 0):, b] = np.nan
    return x


@pytest.mark.parametrize("act,clip", ACTS, ids=["none", "relu", "clip"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", cr.ALL_SHAPES, ids=ids)
def test_conv1d_values(shape, bias, act, clip):
    x, W, b = inputs(shape)
    ref, _ = reference(shape, bias, act, clip)
    got, _ = run(shape, x, W, b if bias else None, act, clip)
    assert got.shape == ref.shape
    close(got, ref, f"conv1d {ids(shape)}")
    if act == "clip" and ref.size >= 500:
        assert (ref == clip).any() and (ref == 0).any()


@pytest.mark.parametrize("shape", cr.ALL_SHAPES, ids=ids)
def test_conv1d_lengths(shape):
    """Ragged lengths (0, 1, below the receptive field, T) with NaN in the padding
    region of x: finite, within the bound, exact zeros past out_frames(len),
    exact d_out_lengths."""
    T, B, ci, co, k, s, d, pl, pr, g = shape
    x, W, b = inputs(shape)
    ln = cr.ragged_lengths(shape)
    ref, roln = reference(shape, True, "relu", 20.0, ln)
    got, oln = run(shape, nan_past_lengths(x, ln), W, b, "relu", lengths=ln)
    assert np.array_equal(oln, roln)
    assert [int(v) for v in oln] == [cr.out_frames(n, k, s, d, pl, pr) for n in ln]
    for bi in range(B):
        assert not got[oln[bi]:, bi].any(), bi
    close(got, ref, f"conv1d lengths {ids(shape)}")


def test_conv1d_lengths_clamped():
    """Lengths outside [0, T] clamp: negative is 0, above T is T."""
    shape = cr.ALL_SHAPES[1]
    T, B = shape[0], shape[1]
    x, W, b = inputs(shape)
    got, oln = run(shape, x, W, b, lengths=(-3, T + 5, T, 0, T))
    ref, roln = reference(shape, True, None, 20.0, (0, T, T, 0, T))
    assert np.array_equal(oln, roln)
    close(got, ref, "clamped lengths")


@pytest.mark.parametrize("shape", [cr.ALL_SHAPES[3]], ids=ids)
def test_conv1d_pointwise_is_linear(shape):
    """kernel = 1: the same contraction as asr_linear_fwd under ASR_DENSE_F32."""
    T, B, ci, co = shape[:4]
    x, W, b = inputs(shape)
    ref, _ = reference(shape, True, "relu", 20.0)
    got, _ = run(shape, x, W, b, "relu")
    y = asr.DeviceMatrix(T * B, co)
    before = asr.get_dense_arith()
    asr.set_dense_arith(asr.DENSE_F32)
    try:
        asr.linear_fwd(dm(x.reshape(T * B, ci)), dm(W.reshape(ci, co)), dm(b.reshape(-1, 1)), y, asr.EPI_BIAS_RELU)
        asr.synchronize()
    finally:
        asr.set_dense_arith(before)
    close(y.toCpu(), ref.reshape(T * B, co), "asr_linear_fwd")
    close(got.reshape(T * B, co), ref.reshape(T * B, co), "conv1d k=1")


# ------------------------------------------------------- bit-independence
@pytest.mark.parametrize("shape", BIT_SHAPES, ids=ids)
def test_bits_do_not_depend_on_the_batch(shape):
    """One utterance alone (B = 1) == the same utterance at two positions of the batch."""
    T, B = shape[0], shape[1]
    x, W, b = inputs(shape)
    ln = list(cr.ragged_lengths(shape))
    u, p1, p2 = 1, 0, B - 1
    n = max(ln[u], min(T, 7))                # a length of its own, others ragged around it
    xb = x.copy()
    xb[:, p1], xb[:, p2] = x[:, u], x[:, u]
    ln[p1] = ln[p2] = n
    got, oln = run(shape, nan_past_lengths(xb, ln), W, b, "relu", lengths=tuple(ln))
    alone, aoln = run(shape, nan_past_lengths(x[:, u:u + 1], [n]), W, b, "relu", lengths=(n,))
    assert aoln[0] == oln[p1] == oln[p2] and aoln[0] > 0
    assert np.array_equal(got[:, p1], alone[:, 0])
    assert np.array_equal(got[:, p2], alone[:, 0])


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=ids)
def test_bits_do_not_depend_on_strides(shape):
    """ldx = c_in + 1 and ldo = c_out + 3 against contiguous buffers; the
    untouched columns keep their sentinel."""
    ci, co = shape[2], shape[3]
    x, W, b = inputs(shape)
    ln = cr.ragged_lengths(shape)
    a, _ = run(shape, x, W, b, lengths=ln)
    s, _ = run(shape, x, W, b, lengths=ln, ldx=ci + 1, ldo=co + 3)
    assert np.all(s[:, :, co:] == SENT)
    assert np.array_equal(s[:, :, :co], a)


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=ids)
def test_bits_do_not_depend_on_alignment(shape):
    """A d_x 4 bytes past a 16-byte boundary against an aligned one."""
    x, W, b = inputs(shape)
    a, _ = run(shape, x, W, b)
    m, _ = run(shape, x, W, b, misalign=True)
    assert np.array_equal(a, m)


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=ids)
def test_length_zero_is_a_data_zero(shape):
    """Frames zeroed by a length (NaN in the buffer) == the same frames truly
    zero with full lengths, on every row the utterance still produces."""
    x, W, b = inputs(shape)
    ln = cr.ragged_lengths(shape)
    cut, oln = run(shape, nan_past_lengths(x, ln), W, b, lengths=ln)
    xz = x.copy()
    for bi, n in enumerate(ln):
        xz[n:, bi] = 0.0
    full, _ = run(shape, xz, W, b)
    assert oln.max() > 0
    for bi in range(shape[1]):
        assert np.array_equal(cut[:oln[bi], bi], full[:oln[bi], bi]), bi


# ---------------------------------------------------------------- streaming
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("groups", [1, 20], ids=["dense", "depthwise"])
def test_causal_streaming_chunks(groups, s):
    """A causal layer over T = 24 in one call == chunks [0, 10) and [10, 24), each
    with its d (k-1) history frames prepended and pad_left = 0, bit for bit."""
    T, B, k, d = 24, 5, 3, 2
    ci = 20
    co = 24 if groups == 1 else ci
    hist = d * (k - 1)
    whole_shape = (T, B, ci, co, k, s, d, hist, 0, groups)
    x, W, b = cr.draw(whole_shape)
    whole, _ = run(whole_shape, x, W, b, "relu")
    assert whole.shape[0] == (T - 1) // s + 1
    xh = np.concatenate([np.zeros((hist, B, ci), np.float32), x])    # frame t at row t + hist
    parts = []
    for lo, hi in ((0, 10), (10, 24)):
        assert lo % s == 0
        chunk = np.ascontiguousarray(xh[lo:hi + hist])
        got, _ = run(whole_shape, chunk, W, b, "relu", desc=make_desc(whole_shape, "relu", pl=0))
        assert got.shape[0] == (hi - lo - 1) // s + 1
        parts.append(got)
    assert np.array_equal(np.concatenate(parts), whole)
    ref, _ = cr.conv1d_ref(x, W, b, k, s, d, hist, 0, groups, "relu")
    close(whole, ref, "causal")


# --------------------------------------------------------------- from_torch
def torch_per_utterance(mods, x, ln, T_out, co):
    """The float64 modules on each utterance's own frames: [T_out][B][co], zeros past its count."""
    out = np.zeros((T_out, x.shape[1], co))
    with torch.no_grad():
        for bi, n in enumerate(ln):
            if n == 0:
                continue
            y = torch.from_numpy(x[:n, bi].astype(np.float64).T.copy())[None]
            try:
                for m in mods:
                    y = m(y)
            except RuntimeError:      # torch refuses an input shorter than the kernel: no output frames
                continue
            y = y[0].numpy().T
            out[:y.shape[0], bi] = y
    return out


def test_from_torch_conv_bn_relu():
    torch.manual_seed(11)
    T, B, ci, co = 23, 6, 40, 48
    conv = torch.nn.Conv1d(ci, co, 11, stride=2, padding=5)
    bn = torch.nn.BatchNorm1d(co)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(co) * 0.3)
        bn.running_var.copy_(torch.rand(co) * 2 + 0.2)
        bn.weight.copy_(torch.rand(co) + 0.5)
        bn.bias.copy_(torch.randn(co) * 0.2)
    bn.eval()
    layer = asr.Conv1d.from_torch(conv, bn, act="relu")
    x = np.random.default_rng(2).uniform(-1, 1, (T, B, ci)).astype(np.float32)
    ln = (T, 0, 1, 9, 17, T)
    out, T_out, oln = layer.forward(dm(nan_past_lengths(x, ln).reshape(T * B, ci)), T, B, lengths=ln)
    asr.synchronize()
    got = out.toCpu().reshape(T_out, B, co)
    ref = torch_per_utterance([conv.double(), bn.double(), torch.nn.ReLU()], x, ln, T_out, co)
    assert [int(v) for v in asr.device_int32(oln, B)] == [layer.out_frames(n) for n in ln]
    close(got, ref, "Conv1d+BN+ReLU")


def test_from_torch_quartznet_pair():
    """Depthwise k = 33 'same' followed by pointwise + BatchNorm + ReLU, lengths passed on."""
    torch.manual_seed(12)
    T, B, C, co = 45, 4, 70, 36
    dw = torch.nn.Conv1d(C, C, 33, padding=16, groups=C, bias=False)
    pw = torch.nn.Conv1d(C, co, 1)
    bn = torch.nn.BatchNorm1d(co)
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(co) * 0.3)
        bn.running_var.copy_(torch.rand(co) * 2 + 0.2)
    bn.eval()
    l1, l2 = asr.Conv1d.from_torch(dw), asr.Conv1d.from_torch(pw, bn, act="relu")
    x = np.random.default_rng(3).uniform(-1, 1, (T, B, C)).astype(np.float32)
    ln = (T, 1, 20, 33)
    h, T1, ln1 = l1.forward(dm(nan_past_lengths(x, ln).reshape(T * B, C)), T, B, lengths=ln)
    out, T2, ln2 = l2.forward(h, T1, B, lengths=ln1)
    asr.synchronize()
    assert (T1, T2) == (T, T)
    assert [int(v) for v in asr.device_int32(ln2, B)] == list(ln)
    ref = torch_per_utterance([dw.double(), pw.double(), bn.double(), torch.nn.ReLU()], x, ln, T2, co)
    close(out.toCpu().reshape(T2, B, co), ref, "depthwise+pointwise")


def test_conv_then_gru_with_lengths_passed_on():
    """Conv1d(stride 2) -> GRU.from_torch with out_lengths passed on, against torch
    conv -> pack_padded_sequence -> torch.nn.GRU in float64."""
    torch.manual_seed(13)
    T, B, ci, co, H = 21, 6, 26, 32, 48
    conv = torch.nn.Conv1d(ci, co, 5, stride=2, padding=2)
    gru = torch.nn.GRU(co, H, 1)
    layer, net = asr.Conv1d.from_torch(conv, act="clip", clip=20.0), asr.GRU.from_torch(gru)
    x = np.random.default_rng(4).uniform(-1, 1, (T, B, ci)).astype(np.float32)
    ln = (T, 3, 12, 1, 20, 8)
    h, T1, ln1 = layer.forward(dm(nan_past_lengths(x, ln).reshape(T * B, ci)), T, B, lengths=ln)
    got = net.forward(h, T1, B, lengths=ln1).toCpu().reshape(T1, B, H)
    asr.synchronize()
    oln = [layer.out_frames(n) for n in ln]
    assert min(oln) >= 1
    cd, gd = conv.double(), gru.double()
    feats = torch_per_utterance([cd, torch.nn.Hardtanh(0.0, 20.0)], x, ln, T1, co)
    with torch.no_grad():
        pk = torch.nn.utils.rnn.pack_padded_sequence(torch.from_numpy(feats), torch.tensor(oln), enforce_sorted=False)
        ref, _ = gd(pk)
        ref, _ = torch.nn.utils.rnn.pad_packed_sequence(ref, total_length=T1)
    close(got, ref.numpy(), "conv -> GRU")
