"""GPU checks of the E-Branchformer additions: the GELU epilogue in every kernel
a bias GEMM can land on, asr_csgu_fwd and asr_merge_dwconv_fwd against the
float64 restatements of ebranchformer_reference.py (values, lengths with NaN
past them, bit independence of batch, strides, alignment and causal chunking),
and the layers against the stand-in module in float64 on each utterance's own
frames.  Bound: 2e-5 (1 + |ref|) unless a test says otherwise."""
import functools

import numpy as np
import pytest
import torch

import ebranchformer_reference as eb
from conftest import asr

pytestmark = pytest.mark.gpu
ATOL = 2e-5
KINDS = {"split_bf16": "DENSE_SPLIT_BF16", "f32": "DENSE_F32"}
# (M, K, N), one per kernel a bias GEMM can land on (test_conformer_gpu.py's list)
GELU_SHAPES = [(17, 4, 70), (64, 32, 64), (333, 96, 40), (1000, 256, 256), (257, 300, 70), (130, 1024, 129),
               (140000, 16, 128)]
ids = lambda s: "x".join(map(str, s))   # noqa: E731


def dm(a):
    return asr.DeviceMatrix.from_numpy(np.ascontiguousarray(a, np.float32))


def close(got, ref, what="", atol=ATOL):
    err = np.abs(np.asarray(got, np.float64) - ref) / (1 + np.abs(ref))
    print(f"{what} max err / (1 + |ref|) {err.max():.3e}")
    assert np.all(np.isfinite(got)) and np.all(err <= atol), f"{what} {err.max()}"


@pytest.fixture
def arith():
    before = asr.get_dense_arith()
    yield
    asr.set_dense_arith(before)


# ============================================================ GELU epilogue
@functools.lru_cache(maxsize=None)
def gemm_inputs(shape):
    """Biases U(+-6) so that the pre-activations cover [-6, 6]."""
    M, K, N = shape
    rng = np.random.default_rng(M + K + N)
    x = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    W = (rng.uniform(-1, 1, (K, N)) / np.sqrt(K)).astype(np.float32)
    b = rng.uniform(-6, 6, N).astype(np.float32)
    rows = np.unique(np.concatenate([np.arange(min(M, 256)), rng.integers(0, M, 256), [M - 1]]))
    pre = x[rows].astype(np.float64) @ W.astype(np.float64) + b
    return x, W, b, rows, pre


def gemm(x, W, b, epi, kind):
    asr.set_dense_arith(getattr(asr, KINDS[kind]))
    y = asr.DeviceMatrix(x.shape[0], W.shape[1])
    asr.linear_fwd(dm(x), dm(W), dm(np.asarray(b).reshape(-1, 1)), y, epi)
    asr.synchronize()
    return y.toCpu()


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("shape", GELU_SHAPES, ids=ids)
def test_gelu_epilogue(shape, kind, arith):
    """Against float64 gelu(x.W + b), and (the SiLU test's isolation, 1e-6)
    against float64 GELU of the device's own EPI_BIAS result."""
    x, W, b, rows, pre = gemm_inputs(shape)
    assert pre.min() < -5.5 and pre.max() > 5.5
    got = gemm(x, W, b, asr.EPI_BIAS_GELU, kind)
    close(got[rows], eb.gelu_ref(pre), f"gelu {ids(shape)} {kind}")
    close(got, eb.gelu_ref(gemm(x, W, b, asr.EPI_BIAS, kind)), f"gelu of bias gemm {ids(shape)} {kind}", atol=1e-6)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("shape", GELU_SHAPES[:6], ids=ids)
def test_gelu_epilogue_extremes(shape, kind, arith):
    """Pre-activations -100 / 0 / +100 by column: +-0, 0 and 100, never NaN."""
    M, K, N = shape
    x = np.random.default_rng(9).uniform(-1, 1, (M, K)).astype(np.float32)
    col = np.arange(N) % 3
    got = gemm(x, np.zeros((K, N), np.float32), np.float32([-100, 0, 100])[col], asr.EPI_BIAS_GELU, kind)
    assert np.all(got[:, col != 2] == 0.0) and np.all(got[:, col == 2] == 100.0)


@pytest.mark.parametrize("shape", [(1000, 256, 256), (600, 1024, 129)], ids=ids)
@pytest.mark.parametrize("kind", list(KINDS))
def test_gelu_rows_independent_of_m(shape, kind, arith):
    x, W, b = gemm_inputs(shape)[:3]
    full = gemm(x, W, b, asr.EPI_BIAS_GELU, kind)
    for lo, hi in ((0, 1), (16, 33), (shape[0] - 300, shape[0])):
        assert np.array_equal(gemm(x[lo:hi], W, b, asr.EPI_BIAS_GELU, kind), full[lo:hi])


# ==================================================== the two conv kernels
def run(kind, x, w, b, C, k, pl, ln=None, gamma=None, beta=None, spare=0, shift=0):
    """The kernel on time-major x [T][B][2C] (the CSGU's u; the merge's two
    sources side by side), each source in a buffer of its own with `spare` /
    `2 spare` extra columns of NaN and starting `shift` floats into a row."""
    T, B = x.shape[:2]

    def place(a, extra):
        m = np.full((T * B, a.shape[2] + extra + shift), np.nan, np.float32)
        m[:, shift:shift + a.shape[2]] = a.reshape(T * B, -1)
        d = dm(m)
        return asr.ColumnView(d, shift) if shift else d

    opt = lambda a: None if a is None else dm(np.asarray(a).reshape(-1, 1))   # noqa: E731
    lengths = None if ln is None else asr.device_lengths(ln)
    pr = k - 1 - pl
    if kind == "csgu":
        out = dm(np.full((T * B, C + spare), np.nan))
        asr.csgu_fwd(place(x, spare), dm(w), opt(b), out, T, B, asr.csgu_desc(C, k, pl, pr), opt(gamma), opt(beta),
                     lengths=lengths)
        n = C
    else:
        out = dm(np.full((T * B, 2 * C + spare), np.nan))
        asr.merge_dwconv_fwd(place(x[..., :C], spare), place(x[..., C:], 2 * spare), dm(w), opt(b), out, T, B,
                             asr.merge_dwconv_desc(C, k, pl, pr), lengths)
        n = 2 * C
    asr.synchronize()
    got = out.toCpu()
    assert np.all(np.isnan(got[:, n:]))                     # columns past the result are not touched
    return got[:, :n].reshape(T, B, n)


def ref(kind, x, w, b, C, pl, ln=None, gamma=None, beta=None):
    if kind == "csgu":
        return eb.csgu_ref(x, w, b, pl, gamma, beta, 1e-5, ln)
    return eb.merge_ref(x[..., :C], x[..., C:], w, b, pl, ln)


def nan_past(x, ln):
    x = x.copy()
    for b, n in enumerate(ln):
        x[n:, b] = np.nan
    return x


@functools.lru_cache(maxsize=None)
def case(kind, T, B, C, k):
    x, w, b = eb.draw_conv(T, B, 2 * C, k, C if kind == "csgu" else 2 * C)
    rng = np.random.default_rng(C + k)
    gamma, beta = rng.uniform(0.5, 1.5, C).astype(np.float32), rng.uniform(-.1, .1, C).astype(np.float32)
    return x, w, b, gamma, beta


# (T, B, C, k, causal): every C, T and k of the list, each padding at small and long k
CSGU_SHAPES = [(1, 2, 8, 1, False), (63, 3, 64, 3, False), (64, 2, 70, 31, False), (65, 5, 130, 31, True),
               (130, 5, 70, 80, False), (130, 2, 8, 80, True), (65, 2, 4096, 3, True), (130, 5, 64, 3, True)]
MERGE_SHAPES = [s for s in CSGU_SHAPES if s[2] <= 70] + [(65, 5, 70, 31, True)]


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("shape", [("csgu",) + s for s in CSGU_SHAPES] + [("merge",) + s for s in MERGE_SHAPES],
                         ids=ids)
def test_conv_values_and_lengths(shape, affine):
    """Lengths (T, 0, 1, 63, 64), NaN past them and in the spare columns; with
    and without bias / gamma / beta; unequal source strides for the merge."""
    kind, T, B, C, k, causal = shape
    x, w, b, gamma, beta = case(kind, T, B, C, k)
    if not affine:
        b = gamma = beta = None
    pl, ln = (k - 1 if causal else (k - 1) // 2), eb.lengths_for(T, B)
    kw = dict(gamma=gamma, beta=beta) if kind == "csgu" else {}
    got = run(kind, nan_past(x, ln), w, b, C, k, pl, ln, spare=3, **kw)
    want = ref(kind, x, w, b, C, pl, ln, **kw)
    mask = np.arange(T)[:, None] < np.asarray(ln)[None, :]
    assert not got[~mask].any()
    close(got[mask], want[mask], ids(shape))


def test_csgu_gate_row_at_1000():
    """Gates at 1000 +- 1: the mean is carried in two parts."""
    T, B, C, k = 65, 2, 130, 3
    x, w, b, gamma, beta = case("csgu", T, B, C, k)
    x = x.copy()
    x[..., C:] += 1000
    close(run("csgu", x, w, b, C, k, 1, gamma=gamma, beta=beta), ref("csgu", x, w, b, C, 1, gamma=gamma, beta=beta),
          "csgu 1000 +- 1")


@pytest.mark.parametrize("shape", [("csgu", 130, 5, 70, 31), ("csgu", 65, 3, 130, 80), ("merge", 130, 5, 70, 31),
                                   ("merge", 65, 3, 64, 80)], ids=ids)
def test_conv_bits_are_independent(shape):
    """An utterance alone against two positions of a batch, padded strides, a
    source 4 bytes past a 16-byte boundary, and causal chunks of 1, 7 and 16
    frames with k - 1 history rows prepended: all np.array_equal."""
    kind, T, B, C, k = shape
    x, w, b, gamma, beta = case(kind, T, B, C, k)
    kw = dict(gamma=gamma, beta=beta) if kind == "csgu" else {}
    ln = eb.lengths_for(T, B)
    for pl in ((k - 1) // 2, k - 1):
        full = run(kind, x, w, b, C, k, pl, ln, **kw)
        for bi in (0, B - 1):
            n = ln[bi]
            alone = run(kind, x[:n, bi:bi + 1], w, b, C, k, pl, **kw)
            assert np.array_equal(alone[:, 0], full[:n, bi])
        assert np.array_equal(run(kind, x, w, b, C, k, pl, ln, spare=5, **kw), full)
        assert np.array_equal(run(kind, x, w, b, C, k, pl, ln, spare=2, shift=1, **kw), full)
    whole = run(kind, x[:, :1], w, b, C, k, k - 1, **kw)          # causal, one utterance of T frames
    for step in (1, 7, 16):
        for t0 in (0, step, 64 - step, T - step):
            lo = max(t0 - (k - 1), 0)
            part = run(kind, x[lo:t0 + step, :1], w, b, C, k, k - 1, **kw)
            assert np.array_equal(part[t0 - lo:], whole[t0:t0 + step]), (step, t0)


# ==================================================================== layers
def test_cgmlp_from_torch():
    T, B, E, units, k = 70, 5, 144, 288, 15
    mod = eb.draw_module(eb.CgMLP(E, units, k), 7)
    x, ln = eb.cr.draw_x(T, B, E), eb.lengths_for(T, B)
    got = asr.ConvolutionalGatingMLP.from_torch(mod).forward(dm(nan_past(x, ln).reshape(T * B, E)), T, B, ln)
    asr.synchronize()
    close(got.toCpu().reshape(T, B, E), eb.on_own_frames(mod, x, ln), "cgmlp")


@pytest.mark.parametrize("macaron", [True, False], ids=["macaron", "plain-ffn"])
@pytest.mark.parametrize("window", list(eb.WINDOWS))
@pytest.mark.parametrize("rel", [False, True], ids=["mha", "relpos"])
@pytest.mark.parametrize("shape", eb.LAYER_SHAPES, ids=ids)
def test_layer_from_espnet(shape, rel, window, macaron):
    T, B, E = shape[:3]
    blk = eb.make_block(shape, rel, macaron)
    x, ln, win = eb.cr.draw_x(T, B, E), eb.lengths_for(T, B), eb.WINDOWS[window]
    layer = asr.EBranchformerLayer.from_espnet(blk, *win)
    stack = asr.EBranchformer([layer])
    for _ in range(2):                                      # the second call reuses the scratch buffers
        got = stack.forward(dm(nan_past(x, ln).reshape(T * B, E)), T, B, ln)
    asr.synchronize()
    want = eb.on_own_frames(blk, x, ln, win)
    f32 = eb.on_own_frames(blk, x, ln, win, torch.float32)
    print(f"torch float32 on the CPU: max err / (1 + |ref|) {(np.abs(f32 - want) / (1 + np.abs(want))).max():.3e}")
    close(got.toCpu().reshape(T, B, E), want, f"layer {ids(shape)} rel={rel} {window} macaron={macaron}")
