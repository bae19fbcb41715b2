"""GPU numerics of the Conformer additions: the SiLU epilogue of asr_linear_fwd
(ASR_EPI_BIAS_SILU), asr_glu_dwconv_fwd, and asr.ConformerConv / ConformerLayer /
Conformer.

References: float64 numpy (conformer_reference.py, checked against torch in
test_conformer_cpu.py) and the torch block of conformer_reference.py in float64
on each utterance's own frames.  Bound: the project's bound for fp32 kernels,
|err| <= 2e-5 * (1 + |ref|), unless a test states another; torch float32 on the
CPU stays at or below 7e-7 * (1 + |ref|) for the whole block at these shapes, so
the reference is about 30x inside the bound.  Inputs: x U(+-1), weights
U(+-1/sqrt(fan-in)), biases U(+-0.1), LayerNorm gamma U(0.5, 1.5), BatchNorm
running variance U(0.5, 1.5).  Each case prints its max error.

asr_glu_dwconv_fwd tiles 64 channels x 64 output frames of one utterance and
stages every supported k in LDS (no second path); conformer_reference.GLU_SHAPES
says which shape covers what.  Bit-independence cases compare with
np.array_equal.
"""
import functools

import numpy as np
import pytest
import torch

import attention_reference as ar
import conformer_reference as cf
from conftest import asr

pytestmark = pytest.mark.gpu
ATOL = 2e-5
SENT = -12345.0


class View:
    """rows x cols floats at a device address that something else owns."""

    def __init__(self, ptr, rows, cols, keep):
        self.ptr, self.rows, self.cols, self._keep = ptr, rows, cols, keep


def dm(a):
    return asr.DeviceMatrix.from_numpy(np.asarray(a, np.float32))


def close(got, ref, what="", atol=ATOL):
    ref = np.asarray(ref, np.float64)
    err = np.abs(np.asarray(got, np.float64) - ref)
    print(f"{what} max err {err.max():.3e} (max err / (1 + |ref|) {(err / (1 + np.abs(ref))).max():.3e})")
    assert np.all(np.isfinite(got))
    assert np.all(err <= atol * (1.0 + np.abs(ref))), f"{what} max err {err.max()}"


def check_valid_rows(got, ref, ln, what):
    """Valid rows under the bound, padding rows exact zeros."""
    mask = np.arange(got.shape[0])[:, None] < np.asarray(ln)[None, :]
    assert not got[~mask].any()
    close(got[mask], ref[mask], what)
    assert mask.sum() >= got.shape[1]


@pytest.fixture
def arith():
    """Restore the process-wide setting after a test that changes it."""
    before = asr.get_dense_arith()
    yield
    asr.set_dense_arith(before)


# ============================================================ SiLU epilogue
# (M, K, N), one per kernel a bias GEMM can land on
SILU_SHAPES = [
    (17, 4, 70),          # tiled, unaligned
    (64, 32, 64),         # narrow
    (333, 96, 40),        # narrow
    (1000, 256, 256),     # split-bf16, K <= 256 (fp32 mode: tiled)
    (257, 300, 70),       # split-bf16, large K
    (130, 1024, 129),     # split-bf16, large K
    (140000, 16, 128),    # the wide kernel in fp32 mode
]
KINDS = {"split_bf16": "DENSE_SPLIT_BF16", "f32": "DENSE_F32"}


def silu64(v):
    v = np.asarray(v, np.float64)
    return v / (1.0 + np.exp(-v))


@functools.lru_cache(maxsize=None)
def gemm_inputs(shape):
    M, K, N = shape
    rng = np.random.default_rng(M + K + N)
    x = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    W = (rng.uniform(-1, 1, (K, N)) / np.sqrt(K)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, N).astype(np.float32)
    rows = np.unique(np.concatenate([np.arange(min(M, 256)), rng.integers(0, M, 256), [M - 1]]))
    xs, Wd = x[rows].astype(np.float64), W.astype(np.float64)
    pre = xs @ Wd + b
    scale = np.abs(xs) @ np.abs(Wd) + np.abs(b)
    for a in (x, W, b, rows, pre, scale):
        a.setflags(write=False)
    return x, W, b, rows, pre, scale


def gemm(x, W, b, epi, kind):
    asr.set_dense_arith(kind)
    y = asr.DeviceMatrix(x.shape[0], W.shape[1])
    asr.linear_fwd(dm(x), dm(W), dm(np.asarray(b).reshape(-1, 1)), y, epi)
    asr.synchronize()
    return y.toCpu()


@pytest.mark.parametrize("shape", SILU_SHAPES, ids=cf.ids)
def test_silu_epilogue_values(shape, arith):
    """(i) against float64 silu(x.W + b) at the bound in both arithmetics, and on
    the GEMM error measure of test_dense_x3_gpu.py (max |err| / sum |a b|) the
    split arithmetic no worse than 1.5 x the fp32 kernels' + 1e-8."""
    x, W, b, rows, pre, scale = gemm_inputs(shape)
    ref = silu64(pre)
    errs = {}
    for name, attr in KINDS.items():
        got = gemm(x, W, b, asr.EPI_BIAS_SILU, getattr(asr, attr))[rows]
        close(got, ref, f"silu {cf.ids(shape)} {name}")
        errs[name] = float((np.abs(got.astype(np.float64) - ref) / scale).max())
    print(f"silu {cf.ids(shape)} err / sum|a b|: {errs}")
    assert errs["split_bf16"] <= 1.5 * errs["f32"] + 1e-8, errs


@pytest.mark.parametrize("kind", list(KINDS), ids=list(KINDS))
@pytest.mark.parametrize("shape", SILU_SHAPES, ids=cf.ids)
def test_silu_epilogue_is_silu_of_the_bias_gemm(shape, kind, arith):
    """(ii) isolation: float64 SiLU of the device's own EPI_BIAS result at the same
    shape and setting, within 1e-6 * (1 + |ref|) (float32 SiLU of a float32
    input measures 1.05e-7 on that scale): the epilogue is SiLU and the GEMM
    under it did not change."""
    x, W, b, rows, _, _ = gemm_inputs(shape)
    k = getattr(asr, KINDS[kind])
    pre = gemm(x, W, b, asr.EPI_BIAS, k)
    got = gemm(x, W, b, asr.EPI_BIAS_SILU, k)
    close(got, silu64(pre), f"silu of bias gemm {cf.ids(shape)} {kind}", atol=1e-6)


@pytest.mark.parametrize("kind", list(KINDS), ids=list(KINDS))
@pytest.mark.parametrize("shape", SILU_SHAPES[:6], ids=cf.ids)
def test_silu_epilogue_extremes(shape, kind, arith):
    """(iii) pre-activations of +-100 and 0 in one matrix: finite, 100 stays 100,
    0 gives 0 and -100 underflows to -0.0 or 0."""
    M, K, N = shape
    rng = np.random.default_rng(9)
    x = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    W = np.zeros((K, N), np.float32)
    W[:, 3::7] = (rng.uniform(-1, 1, (K, len(range(3, N, 7)))) / np.sqrt(K)).astype(np.float32)   # some live columns
    b = np.resize(np.float32([-100, 0, 100, 0, -88, 30, -30]), N)
    b[3::7] = 0.05
    got = gemm(x, W, b, asr.EPI_BIAS_SILU, getattr(asr, KINDS[kind]))
    assert np.all(np.isfinite(got))
    col = np.arange(N) % 7
    assert np.all(got[:, col == 0] == 0.0)
    assert np.all(got[:, col == 1] == 0.0)
    assert np.all(got[:, col == 2] == 100.0)
    close(got, silu64(x.astype(np.float64) @ W.astype(np.float64) + b), f"extremes {cf.ids(shape)} {kind}")


@pytest.mark.parametrize("shape", [(1000, 256, 256), (600, 1024, 129)], ids=cf.ids)
def test_silu_rows_independent_of_m(shape, arith):
    """(iv) the rows of a sub-batch are the whole batch's bits (K <= 256 and the
    large-K kernel of the split arithmetic)."""
    asr.set_dense_arith(asr.DENSE_SPLIT_BF16)
    M, K, N = shape
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    W = (rng.uniform(-1, 1, (K, N)) / np.sqrt(K)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, N).astype(np.float32)
    full = gemm(x, W, b, asr.EPI_BIAS_SILU, asr.DENSE_SPLIT_BF16)
    for lo, hi in ((0, 16), (7, 300), (M - 100, M)):
        part = gemm(x[lo:hi], W, b, asr.EPI_BIAS_SILU, asr.DENSE_SPLIT_BF16)
        assert np.array_equal(part, full[lo:hi]), (lo, hi)


# ============================================================== glu_dwconv
@functools.lru_cache(maxsize=None)
def glu_inputs(shape):
    u, w, b = cf.draw_glu(shape)
    for a in (u, w, b):
        a.setflags(write=False)
    return u, w, b


@functools.lru_cache(maxsize=None)
def glu_reference(shape, bias, act, lengths=None):
    u, w, b = glu_inputs(shape)
    out = cf.glu_dwconv_ref(u, w, b if bias else None, shape[3], shape[4], act, lengths)
    out.setflags(write=False)
    return out


def run_glu(shape, u, w, b, act=None, lengths=None, ldu=None, ldo=None, misalign=False):
    """asr_glu_dwconv_fwd on u [T][B][2C]; returns out [T][B][ldo] float32.  ldu /
    ldo: row strides (the extra columns of u hold NaN, of out a sentinel);
    misalign: u starts 4 bytes past a 16-byte boundary."""
    T, B = u.shape[0], u.shape[1]
    C, k, pl, pr = shape[2:]
    desc = asr.glu_dwconv_desc(C, k, pl, pr, act)
    ldu = ldu or 2 * C
    uh = np.full((T * B, ldu), np.nan, np.float32)
    uh[:, :2 * C] = u.reshape(T * B, 2 * C)
    if misalign:
        flat = np.concatenate([np.zeros(1, np.float32), uh.reshape(-1), np.zeros(3, np.float32)])
        base = dm(flat.reshape(-1, 1))
        du = View(base.ptr + 4, T * B, ldu, base)
        assert du.ptr % 16 == 4
    else:
        du = dm(uh)
        assert du.ptr % 16 == 0
    out = dm(np.full((T * B, ldo or C), SENT, np.float32))
    ln = None if lengths is None else asr.device_lengths(lengths)
    asr.glu_dwconv_fwd(du, dm(w), None if b is None else dm(b.reshape(-1, 1)), out, T, B, desc, lengths=ln)
    asr.synchronize()
    return out.toCpu().reshape(T, B, -1)


@pytest.mark.parametrize("act", cf.ACTS, ids=["none", "relu", "silu"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", cf.GLU_SHAPES, ids=cf.ids)
def test_glu_dwconv_values(shape, bias, act):
    u, w, b = glu_inputs(shape)
    got = run_glu(shape, u, w, b if bias else None, act)
    close(got, glu_reference(shape, bias, act), f"glu_dwconv {cf.ids(shape)}")


@pytest.mark.parametrize("shape", cf.GLU_SHAPES, ids=cf.ids)
def test_glu_dwconv_lengths_strides_and_nan(shape):
    """Ragged lengths (1, T, one > T that clamps, 0 where B allows) with NaN in u
    past them and in the extra columns of ldu > 2C: finite, within the bound,
    exact zeros past the lengths, and the sentinel in the extra columns of
    ldo > C survives."""
    T, B, C = shape[:3]
    u, w, b = glu_inputs(shape)
    ln = cf.glu_lengths(shape)
    got = run_glu(shape, cf.nan_past_lengths(u, ln), w, b, "silu", lengths=ln, ldu=2 * C + 3, ldo=C + 2)
    assert np.all(got[:, :, C:] == SENT)
    for bi, n in enumerate(ln):
        assert not got[min(n, T):, bi, :C].any(), bi
    close(got[:, :, :C], glu_reference(shape, True, "silu", ln), f"glu_dwconv lengths {cf.ids(shape)}")


@pytest.mark.parametrize("shape", cf.GLU_SHAPES, ids=cf.ids)
def test_glu_dwconv_gates_of_100_stay_finite(shape):
    T, B, C, k, pl, pr = shape
    u, w, b = glu_inputs(shape)
    u = u.copy()
    u[:, :, C:] = np.resize(np.float32([100, -100, 0.5, -100, 100, -2]), (T, B, C))
    got = run_glu(shape, u, w, b, "silu")
    close(got, cf.glu_dwconv_ref(u, w, b, k, pl, "silu"), f"glu_dwconv gates +-100 {cf.ids(shape)}")


@pytest.mark.parametrize("shape", cf.GLU_SHAPES, ids=cf.ids)
def test_glu_bits_do_not_depend_on_the_batch(shape):
    """One utterance alone (B = 1) == the same utterance at two positions of the batch."""
    T, B = shape[0], shape[1]
    u, w, b = glu_inputs(shape)
    ln = list(cf.glu_lengths(shape))
    p1, p2 = 0, B - 1
    n = max(T - 2, 1)
    ub = u.copy()
    ub[:, p1], ub[:, p2] = u[:, 1], u[:, 1]
    ln[p1] = ln[p2] = n
    got = run_glu(shape, cf.nan_past_lengths(ub, ln), w, b, "silu", lengths=tuple(ln))
    alone = run_glu(shape, cf.nan_past_lengths(u[:, 1:2], [n]), w, b, "silu", lengths=(n,))
    assert np.array_equal(got[:, p1], alone[:, 0])
    assert np.array_equal(got[:, p2], alone[:, 0])
    assert got[:n, p1].any()


@pytest.mark.parametrize("shape", cf.GLU_SHAPES, ids=cf.ids)
def test_glu_bits_do_not_depend_on_strides_or_alignment(shape):
    """ldu = 2C + 1 and ldo = C + 3 against tight buffers, and a d_u 4 bytes past
    a 16-byte boundary against an aligned one."""
    C = shape[2]
    u, w, b = glu_inputs(shape)
    ln = cf.glu_lengths(shape)
    a = run_glu(shape, u, w, b, "silu", lengths=ln)
    s = run_glu(shape, u, w, b, "silu", lengths=ln, ldu=2 * C + 1, ldo=C + 3)
    assert np.all(s[:, :, C:] == SENT)
    assert np.array_equal(s[:, :, :C], a)
    m = run_glu(shape, u, w, b, "silu", lengths=ln, misalign=True)
    assert np.array_equal(m, a)


@pytest.mark.parametrize("chunk", [1, 7, 16])
@pytest.mark.parametrize("shape", cf.CAUSAL_SHAPES, ids=cf.ids)
def test_glu_causal_streaming_chunks(shape, chunk):
    """A causal module over T frames in one call == chunks of 1, 7 and 16 frames,
    each with its k - 1 history rows prepended (fewer at the start, where the
    zero padding stands in) and the history's output rows dropped, bit for bit."""
    T, B, C, k, pl, pr = shape
    assert (pl, pr) == (k - 1, 0)
    u, w, b = glu_inputs(shape)
    whole = run_glu(shape, u, w, b, "silu")
    parts = []
    for lo in range(0, T, chunk):
        hi, start = min(lo + chunk, T), max(lo - (k - 1), 0)
        got = run_glu(shape, np.ascontiguousarray(u[start:hi]), w, b, "silu")
        parts.append(got[lo - start:])
    assert np.array_equal(np.concatenate(parts), whole)
    close(whole, glu_reference(shape, True, "silu"), "causal")


@pytest.mark.parametrize("shape", cf.GLU_SHAPES, ids=cf.ids)
def test_glu_dwconv_is_conv1d_of_a_host_glu(shape):
    """Composition: asr_conv1d_fwd depthwise (ReLU fused) on a float32 GLU computed
    on the host; within the bound (the device's sigmoid is its own, so not bit
    for bit)."""
    T, B, C, k, pl, pr = shape
    u, w, b = glu_inputs(shape)
    ln = cf.glu_lengths(shape)
    got = run_glu(shape, u, w, b, "relu", lengths=ln)
    g = (u[:, :, :C] * (np.float32(1) / (np.float32(1) + np.exp(-u[:, :, C:])))).astype(np.float32)
    out = dm(np.zeros((T * B, C), np.float32))
    asr.conv1d_fwd(dm(g.reshape(T * B, C)), dm(w), dm(b.reshape(-1, 1)), out, T, B,
                   asr.conv1d_desc(C, C, k, 1, 1, pl, pr, C, "relu"), lengths=asr.device_lengths(ln))
    asr.synchronize()
    close(got, out.toCpu().reshape(T, B, C), f"glu_dwconv vs conv1d {cf.ids(shape)}")


# ================================================================== layers
@pytest.mark.parametrize("padding", ["same", "causal"])
def test_conformer_conv_from_torch(padding):
    T, B, E, k = 70, 5, 144, 15
    mod = cf.draw_module(cf.ConvModule(E, k, padding), 31)
    layer = asr.ConformerConv.from_torch(*mod.parts(), padding=None if padding == "same" else padding)
    assert (layer.desc.pad_left, layer.desc.pad_right) == ((7, 7) if padding == "same" else (14, 0))
    x = cf.draw_x(T, B, E)
    ln = ar.ragged_lengths(T, B)
    out = layer.forward(dm(cf.nan_past_lengths(x, ln).reshape(T * B, E)), T, B, lengths=ln)
    asr.synchronize()
    check_valid_rows(out.toCpu().reshape(T, B, E), cf.conv_module_ref(mod, x, ln), ln, f"ConformerConv {padding}")


@pytest.mark.parametrize("window", list(cf.WINDOWS), ids=list(cf.WINDOWS))
@pytest.mark.parametrize("first", [False, True], ids=["attention-first", "convolution-first"])
@pytest.mark.parametrize("shape", cf.LAYER_SHAPES, ids=cf.ids)
def test_conformer_layer_from_torch(shape, first, window):
    """The whole block against the torch block in float64 on each utterance's own
    frames (torch does not mask padding inside the convolution, the library does),
    ragged lengths with NaN past them; the convolution-first cases go through the
    torchaudio-layout adapter."""
    T, B, E, heads, F, k = shape
    win = cf.WINDOWS[window]
    block = cf.make_block(shape, convolution_first=first)
    if first:
        layer = asr.ConformerLayer.from_torchaudio(block, *win)
    else:
        layer = asr.ConformerLayer.from_torch(**block.explicit_parts(), chunk=win[0], left=win[1], right=win[2])
    assert layer.convolution_first is first
    x = cf.draw_x(T, B, E)
    ln = ar.ragged_lengths(T, B)
    out = layer.forward(dm(cf.nan_past_lengths(x, ln).reshape(T * B, E)), T, B, lengths=ln)
    asr.synchronize()
    assert (out.rows, out.cols) == (T * B, E)
    check_valid_rows(out.toCpu().reshape(T, B, E), cf.block_ref(block, x, ln, win), ln,
                     f"ConformerLayer {cf.ids(shape)} first={first} {window}")


def test_conformer_layer_second_call_with_another_shape():
    """The same layer object on (T, B) = (40, 3), then (23, 6), then (40, 3) again:
    the scratch buffers are reallocated, and the first result comes back bit for bit."""
    shape = cf.LAYER_SHAPES[1]
    E = shape[2]
    block = cf.make_block(shape)
    layer = asr.ConformerLayer.from_torch(**block.explicit_parts())
    outs = []
    for T, B in ((40, 3), (23, 6), (40, 3)):
        x = cf.draw_x(T, B, E)
        ln = ar.ragged_lengths(T, B)
        got = layer.forward(dm(cf.nan_past_lengths(x, ln).reshape(T * B, E)), T, B, lengths=ln).toCpu().reshape(T, B, E)
        asr.synchronize()
        check_valid_rows(got, cf.block_ref(block, x, ln), ln, f"ConformerLayer T={T} B={B}")
        outs.append(got)
    assert np.array_equal(outs[0], outs[2])
    # no lengths at all: every row is computed
    x = cf.draw_x(23, 6, E)
    got = layer.forward(dm(x.reshape(23 * 6, E)), 23, 6).toCpu().reshape(23, 6, E)
    close(got, cf.block_ref(block, x, (23,) * 6), "ConformerLayer without lengths")


def test_conv_then_conformer_then_logsoftmax():
    """Conv1d(stride 2) -> Conformer([layer, layer]) -> Linear + log-softmax, the
    convolution's device out_lengths passed straight on; against the torch chain in
    float64 on each utterance's own frames."""
    torch.manual_seed(41)
    T, B, ci, E, heads, F, k, V = 41, 6, 26, 32, 2, 64, 7, 29
    conv = torch.nn.Conv1d(ci, E, 5, stride=2, padding=2)
    blocks = [cf.make_block((T, B, E, heads, F, k), convolution_first=bool(i), seed=i) for i in range(2)]
    lin = torch.nn.Linear(E, V)
    c1 = asr.Conv1d.from_torch(conv, act="relu")
    enc = asr.Conformer([asr.ConformerLayer.from_torch(**blk.explicit_parts()) for blk in blocks])
    x = np.random.default_rng(8).uniform(-1, 1, (T, B, ci)).astype(np.float32)
    ln = (T, 3, 12, 1, 20, 8)
    h, T1, ln1 = c1.forward(dm(cf.nan_past_lengths(x, ln).reshape(T * B, ci)), T, B, lengths=ln)
    y = enc.forward(h, T1, B, lengths=ln1)
    l3 = asr.Linear(T1 * B, E, V, lin.weight.detach().numpy().T.copy(), lin.bias.detach().numpy(),
                    asr.EPI_BIAS_LOGSOFTMAX)
    got = l3.forward(y).toCpu().reshape(T1, B, V)
    asr.synchronize()
    oln = [c1.out_frames(n) for n in ln]
    assert [int(v) for v in asr.device_int32(ln1, B)] == oln and min(oln) >= 1
    yh = y.toCpu().reshape(T1, B, E)
    for b, n in enumerate(oln):
        assert not yh[n:, b].any()
    cd, ld = conv.double(), lin.double()
    b64 = [blk.double() for blk in blocks]
    with torch.no_grad():
        for b, n in enumerate(ln):
            f = torch.relu(cd(torch.from_numpy(x[:n, b].astype(np.float64).T.copy())[None]))[0].T[:, None, :]   # [n1][1][E]
            assert f.shape[0] == oln[b]
            for blk in b64:
                f = blk(f)
            ref = torch.log_softmax(ld(f[:, 0]), dim=1).numpy()
            close(got[:oln[b], b], ref, f"chain utterance {b}")
