"""GPU checks of the wav2vec 2.0 / HuBERT additions against the float64
restatements of wav2vec2_reference.py: asr_grouped_conv1d_fwd, asr_wave_conv_fwd,
asr_layernorm_gelu_fwd and Wav2Vec2Encoder.from_transformers end to end, each
utterance against the model run on it alone.  NaN fills every row past a length
and every stride's slack.  Bound: 2e-5 (1 + |ref|) unless a test says otherwise."""
import functools
import itertools

import numpy as np
import pytest
import torch

import wav2vec2_reference as w2v
from conftest import asr

pytestmark = pytest.mark.gpu
ATOL = 2e-5
TT = 128          # asr_grouped_conv1d_fwd's output frames per workgroup
CHUNK = 256       # asr_wave_conv_fwd's statistics chunk (frames)


def dm(a):
    return asr.DeviceMatrix.from_numpy(np.ascontiguousarray(a, np.float32))


def col(a):
    return dm(np.asarray(a, np.float32).reshape(-1, 1))


def close(got, ref, what="", atol=ATOL):
    err = np.abs(np.asarray(got, np.float64) - ref) / (1 + np.abs(ref))
    print(f"{what} max err / (1 + |ref|) {err.max() if err.size else 0:.3e}")
    assert np.all(np.isfinite(got)) and np.all(err <= atol), f"{what} {err.max()}"


def padded(a, ld, fill=np.nan):
    """a [..., n] as rows of ld floats, the slack filled."""
    out = np.full(a.shape[:-1] + (ld,), fill, np.float32)
    out[..., :a.shape[-1]] = a
    return out.reshape(-1, ld)


# ============================================================ grouped conv
def gconv_lengths(T):
    return [T, 0, max(T // 2, 1), max(T - 1, 1)]


@functools.lru_cache(maxsize=None)
def gconv_case(cg, groups, k, pl, pr, T):
    cg_in, cg_out = cg
    c_in, c_out, B = cg_in * groups, cg_out * groups, 4
    rng = np.random.default_rng(c_in + 7 * k + T)
    x = rng.uniform(-1, 1, (T, B, c_in)).astype(np.float32)
    W = (rng.uniform(-1, 1, (k, cg_in, c_out)) / np.sqrt(k * cg_in)).astype(np.float32)
    b = rng.uniform(-2, 2, c_out).astype(np.float32)
    res = rng.uniform(-1, 1, (T + pl + pr - k + 1, B, c_out)).astype(np.float32)
    ln = gconv_lengths(T)
    pre = w2v.grouped_conv_ref(x, W, b, groups, pl, pr, ln)
    xn = x.copy()
    for bi, n in enumerate(ln):
        xn[n:, bi] = np.nan
    return x, xn, W, b, res, ln, pre


def run_gconv(xn, W, b, desc, T, B, ln, res=None, ldx=None, alias=False):
    c_in, c_out = desc.c_in, desc.c_out
    T_out = asr.grouped_conv1d_out_frames(desc, T)
    dx = dm(padded(xn, ldx or c_in + 3))
    out = dm(np.full((T_out * B, c_out + 1), 7.0))
    oln = asr.DeviceBytes(4 * B)
    dres = dx if alias else None if res is None else dm(padded(res, c_out + 2))
    asr.grouped_conv1d_fwd(dx, dm(W.reshape(-1, c_out)), col(b), out, T, B, desc, dres, asr.device_lengths(ln), oln)
    asr.synchronize()
    got = out.toCpu().reshape(T_out, B, c_out + 1)
    assert np.all(got[..., c_out] == 7.0), "columns past c_out were touched"
    counts = [asr.grouped_conv1d_out_frames(desc, n) for n in ln]
    assert asr.device_int32(oln, B).tolist() == counts
    return got[..., :c_out], counts


KPADS = [(1, 0, 0), (2, 1, 0), (16, 8, 7), (128, 64, 63), (5, 3, 0)]        # SamePad pads, then an asymmetric pair
GCONV_T = [1, 5, TT - 1, TT, TT + 1, 2 * TT + 3]


@pytest.mark.parametrize("T", GCONV_T)
@pytest.mark.parametrize("kpad", KPADS, ids=lambda v: "k%d_%d_%d" % v)
@pytest.mark.parametrize("groups", [2, 4])
@pytest.mark.parametrize("cg", [(3, 5), (16, 16), (48, 48)], ids=lambda v: "%dx%d" % v)
def test_grouped_conv(cg, groups, kpad, T):
    """GELU on and off x residual off, on and aliasing x (where c_in == c_out), ragged lengths 0 .. T."""
    k, pl, pr = kpad
    if T + pl + pr - k + 1 <= 0:
        assert asr.grouped_conv1d_out_frames(asr.grouped_conv1d_desc(cg[0] * groups, cg[1] * groups, k, groups, pl, pr),
                                             T) == 0
        return
    x, xn, W, b, res, ln, pre = gconv_case(cg, groups, k, pl, pr, T)
    for gelu, rmode in itertools.product((False, True), ("off", "on", "alias")):
        if rmode == "alias" and (cg[0] != cg[1] or pl + pr != k - 1):
            continue
        desc = asr.grouped_conv1d_desc(cg[0] * groups, cg[1] * groups, k, groups, pl, pr, "gelu" if gelu else None)
        got, counts = run_gconv(xn, W, b, desc, T, 4, ln, res if rmode == "on" else None, alias=rmode == "alias")
        ref = w2v.gelu_ref(pre) if gelu else pre.copy()
        radd = res if rmode == "on" else x if rmode == "alias" else 0 * res
        for bi, n in enumerate(counts):
            ref[:n, bi] += radd[:n, bi]
            ref[n:, bi] = 0
            assert not got[n:, bi].any()
        close(got, ref, f"gconv gelu={gelu} res={rmode}")


@pytest.mark.parametrize("cg,groups,kpad,T", [((3, 5), 2, (5, 3, 0), 2 * TT + 3), ((16, 16), 4, (128, 64, 63), TT + 1),
                                               ((48, 48), 2, (16, 8, 7), TT)], ids=str)
def test_grouped_conv_bits(cg, groups, kpad, T):
    """An utterance alone against the same utterance inside a batch, and ldx = c_in against c_in + 4: equal bits."""
    k, pl, pr = kpad
    x, xn, W, b, res, ln, _ = gconv_case(cg, groups, k, pl, pr, T)
    desc = asr.grouped_conv1d_desc(cg[0] * groups, cg[1] * groups, k, groups, pl, pr, "gelu")
    base, counts = run_gconv(xn, W, b, desc, T, 4, ln, res)
    wide, _ = run_gconv(xn, W, b, desc, T, 4, ln, res, ldx=desc.c_in + 4)
    tight, _ = run_gconv(xn, W, b, desc, T, 4, ln, res, ldx=desc.c_in)
    assert np.array_equal(base, wide) and np.array_equal(base, tight)
    for bi in (0, 2):
        n = ln[bi]
        alone, _ = run_gconv(xn[:n, bi:bi + 1], W, b, desc, n, 1, [n], res[:counts[bi], bi:bi + 1])
        assert np.array_equal(alone[:, 0], base[:counts[bi], bi])


# =============================================================== wave conv
def wave_inputs(k, s, C, frames, seed=0, centre=0.0):
    rng = np.random.default_rng(seed + k + C)
    ns = [0, k - 1] + [(f - 1) * s + k + (i % s) for i, f in enumerate(frames)]     # + i % s: samples past the last tap
    S = max(ns) + 3
    wave = (centre + rng.uniform(-1, 1, (len(ns), S))).astype(np.float32)
    W = rng.uniform(-.5, .5, (k, C)).astype(np.float32)
    b, gamma, beta = (rng.uniform(lo, hi, C).astype(np.float32) for lo, hi in ((-.3, .3), (.5, 1.5), (-.2, .2)))
    nan = wave.copy()
    for bi, n in enumerate(ns):
        nan[bi, n:] = np.nan
    return wave, nan, ns, W, b, gamma, beta


def run_wave(nan, ns, W, b, gamma, beta, s, mode, ldw=None, ldo=None, eps=1e-5):
    B, S = nan.shape
    k, C = W.shape
    desc = asr.wave_conv_desc(C, k, s, mode, eps)
    T1 = asr.wave_conv_out_frames(desc, S)
    ldo = ldo or C + 1
    out, oln = dm(np.full((T1 * B, ldo), 7.0)), asr.DeviceBytes(4 * B)
    dw = dm(padded(nan, ldw or S + 5))
    norm = mode != "none"
    asr.wave_conv_fwd(dw, dm(W), col(b), out, B, S, desc, col(gamma) if norm else None, col(beta) if norm else None,
                      None, asr.device_lengths(ns), oln)
    asr.synchronize()
    got = out.toCpu().reshape(T1, B, ldo)
    assert np.all(got[..., C:] == 7.0), "columns past C were touched"
    return got[..., :C], asr.device_int32(oln, B).tolist()


WAVE_FRAMES = [1, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 88]      # the last spans three chunks


@pytest.mark.parametrize("C", [5, 64, 96])
@pytest.mark.parametrize("ks", [(10, 5), (3, 2)], ids=lambda v: "k%d_s%d" % v)
@pytest.mark.parametrize("mode", ["none", "layer", "group"])
def test_wave_conv(mode, ks, C):
    k, s = ks
    wave, nan, ns, W, b, gamma, beta = wave_inputs(k, s, C, WAVE_FRAMES)
    got, counts = run_wave(nan, ns, W, b, gamma, beta, s, mode)
    v, want = w2v.wave_conv_pre(wave, ns, W, b, s)
    assert counts == want == [0, 0] + WAVE_FRAMES
    for bi, f in enumerate(counts):
        assert not got[f:, bi].any()
    close(got, w2v.wave_norm_ref(v, counts, mode, gamma, beta, 1e-5), f"wave conv {mode}")


@pytest.mark.parametrize("C", [5, 96])
def test_wave_conv_time_norm_far_from_zero(C):
    """Samples 1000 + U(+-1), one tap of weight 1, 1/2 or 2 per channel and no bias, so the fp32
    convolution is exact and the float64 reference normalises the same fp32 values.  The channel's
    standard deviation is 0.6 at a mean of 1000: E[x^2] - E[x]^2 in fp32 (quantum 0.06 at 1e6), or a
    mean kept in one float (3e-5 off), misses the bound."""
    k, s = 10, 5
    wave, nan, ns, _, _, gamma, beta = wave_inputs(k, s, C, [CHUNK + 1, 2 * CHUNK + 88], seed=1, centre=1000.0)
    W = np.zeros((k, C), np.float32)
    W[np.arange(C) % k, np.arange(C)] = np.array([1, .5, 2], np.float32)[np.arange(C) % 3]
    got, counts = run_wave(nan, ns, W, 0 * beta, gamma, beta, s, "group")
    v, _ = w2v.wave_conv_pre(wave, ns, W, 0 * beta, s)
    assert np.array_equal(v, v.astype(np.float32))
    close(got, w2v.wave_norm_ref(v, counts, "group", gamma, beta, 1e-5), "time norm at 1000 +- 1")


@pytest.mark.parametrize("mode", ["none", "layer", "group"])
def test_wave_conv_bits(mode):
    """An utterance alone (its own S) against the batch, and other strides: equal bits."""
    k, s, C = 10, 5, 96
    wave, nan, ns, W, b, gamma, beta = wave_inputs(k, s, C, [CHUNK + 1, 2 * CHUNK + 88, 65])
    base, counts = run_wave(nan, ns, W, b, gamma, beta, s, mode)
    other, _ = run_wave(nan, ns, W, b, gamma, beta, s, mode, ldw=nan.shape[1], ldo=C + 4)
    assert np.array_equal(base, other)
    for bi in (2, 3):
        alone, _ = run_wave(nan[bi:bi + 1, :ns[bi]], ns[bi:bi + 1], W, b, gamma, beta, s, mode)
        assert np.array_equal(alone[:, 0], base[:counts[bi], bi])


# ========================================================== LayerNorm-GELU
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("N", [5, 64, 512])
def test_layernorm_gelu(N, norm):
    """In place, with lengths, against float64 and (1e-6) against the float64 GELU of asr_layernorm_fwd's
    own result on the same rows."""
    T, B, ln = 7, 3, [7, 0, 4]
    rng = np.random.default_rng(N)
    x = rng.uniform(-3, 3, (T, B, N)).astype(np.float32)
    gamma, beta = rng.uniform(.5, 1.5, N).astype(np.float32), rng.uniform(-.5, .5, N).astype(np.float32)
    xn = x.copy()
    for bi, n in enumerate(ln):
        xn[n:, bi] = np.nan
    buf, y, dl = dm(padded(xn, N + 3)), asr.DeviceMatrix(T * B, N), asr.device_lengths(ln)
    asr.layernorm_fwd(buf, y, T, B, N, col(gamma), col(beta), 1e-5, lengths=dl)
    asr.layernorm_gelu_fwd(buf, buf, T, B, N, col(gamma), col(beta), 1e-5, norm, dl)
    asr.synchronize()
    raw = buf.toCpu().reshape(T, B, N + 3)
    got, pre = raw[..., :N], y.toCpu().reshape(T, B, N).astype(np.float64) if norm else x.astype(np.float64)
    ref = w2v.gelu_ref(w2v.ln_ref(x, gamma, beta, 1e-5) if norm else x)
    for bi, n in enumerate(ln):
        ref[n:, bi] = 0
        pre[n:, bi] = 0
        assert not got[n:, bi].any() and np.all(np.isnan(raw[:, bi, N:]))
    close(got, ref, f"layernorm_gelu N={N} norm={norm}")
    close(got, w2v.gelu_ref(pre), "against the GELU of asr_layernorm_fwd's rows", atol=1e-6)


# ============================================================== end to end
E2E_FP32_ERR = 3.27e-7          # torch float32 on the CPU against float64, max |err| / (1 + |ref|) over the 4 models
E2E_BOUND = 4 * E2E_FP32_ERR    # 1.31e-6
E2E_NS = (700, 400, 9)


@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("mode", ["group", "layer"])
def test_encoder_end_to_end(mode, stable):
    """The stand-in (conv_dim (32, 32, 32), strides (5, 2, 2), kernels (10, 3, 2), hidden 48, 4 heads, 2
    layers, positional conv k = 16 in 4 groups, V = 20) through Wav2Vec2Encoder.from_transformers, B = 3
    with 700, 400 and 9 samples, against the stand-in in float64 on each utterance alone.  Bound: 4 x the
    error of the same stand-in in torch float32 on the CPU against its float64 self on these inputs
    (3.27e-7 of 1 + |ref| at worst over the four models, so 1.31e-6), the 4 for another summation order through 2
    layers and 3 LayerNorms.  Measured on the device: 1.6e-7 to 2.8e-7."""
    m = w2v.StandIn(mode, stable, vocab=20)
    rng = np.random.default_rng(11)
    wave = rng.standard_normal((3, 705)).astype(np.float32)
    nan = wave.copy()
    for bi, n in enumerate(E2E_NS):
        nan[bi, n:] = np.nan
    enc = asr.Wav2Vec2Encoder.from_transformers(m)
    out, oln = enc.forward(nan, E2E_NS)
    asr.synchronize()
    T = out.rows // 3
    got, counts = out.toCpu().reshape(T, 3, 20), asr.device_int32(oln, 3).tolist()
    m64 = m.double()
    assert counts == [34, 19, 0] and T == enc.features.out_frames(705) and not got[:, 2].any()
    for bi, n in enumerate(E2E_NS[:2]):
        ref = m64(torch.from_numpy(wave[bi, :n].astype(np.float64))).numpy()
        assert ref.shape[0] == counts[bi] and not got[counts[bi]:, bi].any()
        close(got[:counts[bi], bi], ref, f"encoder {mode} stable={stable} utterance {bi}", atol=E2E_BOUND)
