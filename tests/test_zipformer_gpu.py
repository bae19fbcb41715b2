"""GPU numerics of the Zipformer additions: asr_attention_zip_fwd in both forms,
the Swoosh epilogues, asr_glu_dwconv_fwd with SwooshR, asr_biasnorm_fwd /
asr_bypass_fwd, asr.ZipformerLayer and asr.Zipformer.

Reference: zipformer_reference.py (float64).  Bound: the project's bound for
fp32 kernels, |err| <= 2e-5 * (1 + |ref|); the attention value cases also
compute the error of torch float32 on the CPU for the same formula and take
max(2e-5, 4 x that) if it exceeds 5e-6.  Inputs U(+-1) for operands and the
table.  Rows past the lengths and table rows outside the needed range hold NaN.
Bit-independence cases compare with np.array_equal.
"""
import functools

import numpy as np
import pytest
import torch

import attention_reference as ar
import zipformer_reference as zr
from conftest import asr
from test_attention_gpu import ATOL, SENT, close, dm, fetch, nan_past_lengths, put
from test_attention_gpu import run as run_plain
from test_ebranchformer_gpu import GELU_SHAPES, KINDS, arith, gemm, gemm_inputs  # noqa: F401

pytestmark = pytest.mark.gpu
ids = lambda s: "x".join(map(str, s))   # noqa: E731
MODES = {"full": (1, -1, -1), "causal": (1, -1, 0), "chunked": (16, 2, 0), "ragged": (1, -1, -1)}
KEYSIDE = ("k", "v", "sg")


@functools.lru_cache(maxsize=None)
def draw(T, B, H, dq, dp, dv, G):
    """q, k, pz, v, sg, y [T][B][.] and the table [2T - 1][H dp] (pos_zero = T - 1), U(+-1), read-only."""
    rng = np.random.default_rng(T + 10 * B + 100 * H + dq + dp + dv)
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)   # noqa: E731
    c = dict(q=u(T, B, H * dq), k=u(T, B, H * dq), pz=u(T, B, max(H * dp, 1)), v=u(T, B, G * dv), sg=u(T, B, G * dv),
             y=u(T, B, G * dv), pos=u(2 * T - 1, max(H * dp, 1)))
    for a in c.values():
        a.setflags(write=False)
    return c


def run(c, H, dq, dp, dv, G, mask=(1, -1, -1), lengths=None, gate=False, score_head=0, qs=None, ks=None, ld=0,
        misalign=False):
    """asr_attention_zip_fwd on the rows qs (queries) / ks (keys) of the case, frames from qs.start / ks.start.
    ld: extra NaN columns per row of every operand (the output's hold a sentinel)."""
    T, B = c["q"].shape[:2]
    qs, ks = qs or slice(0, T), ks or slice(0, T)
    Tq, Tk = qs.stop - qs.start, ks.stop - ks.start
    dev = {}
    for name in ("q", "k", "pz", "v", "sg", "y"):
        sl = ks if name in KEYSIDE else qs
        a = c[name][sl] if lengths is None else nan_past_lengths(c[name][sl], lengths, sl.start)
        dev[name] = put(a.reshape(-1, a.shape[2]), a.shape[2] + ld if ld else None, misalign=misalign)
    dmax, dmin = asr.rel_needed_rows(Tq, Tk, *mask, q_pos0=qs.start, k_pos0=ks.start)
    pos = c["pos"].copy()
    pos[:max(T - 1 - dmax, 0)] = np.nan
    pos[T - 1 - dmin + 1:] = np.nan
    dev["pos"] = put(pos, pos.shape[1] + ld if ld else None, misalign=misalign)
    ldo = G * dv + ld
    out = put(np.full((Tq * B, ldo), SENT, np.float32), misalign=misalign)
    d = asr.zattn_desc(H, dq, dp, dv, G, score_head, 0.0, *mask, gate=gate)
    asr.attention_zip_fwd(dev["q"], dev["k"], dev["v"], out, Tq, Tk, B, d, pz=dev["pz"] if dp else None,
                          pos=dev["pos"] if dp else None, pos_zero=T - 1, sg=dev["sg"] if gate else None,
                          y=dev["y"] if gate else None, lengths=None if lengths is None else asr.device_lengths(lengths),
                          q_pos0=qs.start, k_pos0=ks.start)
    asr.synchronize()
    got = fetch(out, Tq * B, ldo).reshape(Tq, B, ldo)
    assert np.all(got[:, :, G * dv:] == SENT)
    return got[:, :, :G * dv]


def reference(c, H, dp, G, f=np.float64, **kw):
    """zattn_ref of the case; f = np.float32: the same formula in torch float32 on the CPU."""
    if f is np.float64:
        return zr.zattn_ref(c["q"], c["k"], c["v"], H, G, c["pz"] if dp else None, c["pos"], c["q"].shape[0] - 1, **kw)
    T, B = c["q"].shape[:2]
    t = lambda a, n: torch.from_numpy(np.array(a)).view(a.shape[0], -1, n, a.shape[-1] // n)   # noqa: E731
    s = torch.einsum("ibhd,jbhd->bhij", t(c["q"], H), t(c["k"], H))
    if dp:
        row = torch.from_numpy(T - 1 - (np.arange(T)[:, None] - np.arange(T)[None, :]))
        s = s + torch.einsum("ibhd,ijhd->bhij", t(c["pz"], H), t(c["pos"], H)[row][:, :, 0])
    s = s / np.sqrt(c["q"].shape[2] // H)
    s = s[:, kw.get("score_head", 0):kw.get("score_head", 0) + 1] if G != H else s
    ok = torch.from_numpy(np.stack([ar.mask_matrix(T, T, n, *kw["mask"]) for n in kw["lengths"] or (T,) * B]))
    v = t(c["v"] * np.tanh(c["sg"]) if kw.get("sg") is not None else c["v"], G)
    out = torch.einsum("bhij,jbhd->ibhd", torch.softmax(s.masked_fill(~ok[:, None], -float("inf")), -1), v)
    out = out.reshape(T, B, -1).numpy() * (c["y"] if kw.get("y") is not None else 1)
    return np.nan_to_num(out)


def check_values(c, dims, mode, what, **kw):
    H, dq, dp, dv, G = dims
    T, B = c["q"].shape[:2]
    ln = ar.ragged_lengths(T, B) if mode == "ragged" else None
    gated = dict(sg=c["sg"], y=c["y"]) if kw.get("gate") else {}
    rkw = dict(mask=MODES[mode], lengths=ln, score_head=kw.get("score_head", 0), **gated)
    ref = reference(c, H, dp, G, **rkw)
    e32 = (np.abs(reference(c, H, dp, G, np.float32, **rkw) - ref) / (1 + np.abs(ref))).max()
    bound = max(ATOL, 4 * e32) if e32 > 5e-6 else ATOL
    print(f"torch float32 (CPU) err / (1 + |ref|) {e32:.3e}, bound {bound:.3e}")
    got = run(c, H, dq, dp, dv, G, MODES[mode], ln, **kw)
    for b, n in enumerate(ln or ()):
        assert not got[n:, b].any(), b
    close(got, ref, what, atol=bound)


HEAD_SHAPES = [(65, 2, 2, 32, 4, 12), (130, 3, 1, 20, 4, 12), (17, 1, 3, 4, 0, 4), (193, 1, 1, 32, 16, 16)]
WIDE_SHAPES = [(65, 2, 2, 132, 0), (40, 3, 4, 288, 0), (70, 1, 2, 64, 1)]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=ids)
def test_per_head_form(shape, mode):
    T, B, H, dq, dp, dv = shape
    check_values(draw(T, B, H, dq, dp, dv, H), (H, dq, dp, dv, H), mode, f"per-head {ids(shape)} {mode}")


@pytest.mark.parametrize("gate", [True, False], ids=["gate", "plain"])
@pytest.mark.parametrize("shape", WIDE_SHAPES, ids=ids)
def test_wide_form(shape, gate):
    """dq = 32, dp = 4, ragged lengths; sg = +-100 in live rows 0 and 1 (tanh saturates, no NaN)."""
    T, B, H, dv, sh = shape
    c = dict(draw(T, B, H, 32, 4, dv, 1))
    c["sg"] = c["sg"].copy()
    c["sg"][0], c["sg"][1, :, ::2] = 100.0, -100.0
    check_values(c, (H, 32, 4, dv, 1), "ragged" if B > 1 else "chunked", f"wide {ids(shape)} gate {gate}", gate=gate,
                 score_head=sh)


@pytest.mark.parametrize("mode", ["full", "chunked"])
def test_plain_form_equals_attention_fwd(mode):
    """dp = 0, gate = 0, G = H, dv = dq against asr_attention_fwd: within the bound.  Bitwise equality is printed,
    not demanded: the MFMA chain is the same but the two files are compiled apart."""
    T, B, H, D = 70, 3, 2, 36
    c = draw(T, B, H, D, 0, D, H)
    ln = ar.ragged_lengths(T, B)
    got = run(c, H, D, 0, D, H, MODES[mode], ln)
    plain = run_plain(c["q"], c["k"], c["v"], H, MODES[mode], lengths=ln)
    print("bitwise equal:", np.array_equal(got, plain))
    close(got, plain, f"zip against attention_fwd {mode}")


BITS = {"head": (130, 3, 2, 32, 4, 12, 2, False), "wide": (130, 3, 2, 32, 4, 132, 1, True)}


@pytest.mark.parametrize("form", list(BITS))
def test_bits_streaming_batch_and_strides(form):
    """A call cut into 16-frame chunks over a K/V cache of the last two chunks == the whole call; B = 1 == the row
    inside B = 3; strided, misaligned operands == packed ones.  Mask (16, 2, 0), ragged lengths."""
    T, B, H, dq, dp, dv, G, gate = BITS[form]
    c, ln, mask = draw(T, B, H, dq, dp, dv, G), (130, 0, 65), (16, 2, 0)
    args = (H, dq, dp, dv, G, mask)
    whole = run(c, *args, ln, gate)
    for lo in range(0, T, 16):
        qs, ks = slice(lo, min(lo + 16, T)), slice(max(lo - 32, 0), min(lo + 16, T))
        assert np.array_equal(run(c, *args, ln, gate, qs=qs, ks=ks), whole[qs]), lo
    one = {k: (a if k == "pos" else a[:, 2:3]) for k, a in c.items()}
    assert np.array_equal(run(one, *args, ln[2:], gate), whole[:, 2:3])
    assert np.array_equal(run(c, *args, ln, gate, ld=3, misalign=True), whole)


def test_bits_do_not_depend_on_the_value_width():
    T, B, H = 65, 2, 2
    c = draw(T, B, H, 32, 4, 260, 1)
    narrow = {k: (a[:, :, :132] if k in ("v", "sg", "y") else a) for k, a in c.items()}
    assert np.array_equal(run(narrow, H, 32, 4, 132, 1, gate=True), run(c, H, 32, 4, 260, 1, gate=True)[:, :, :132])


# ---------------------------------------------------------------- epilogues
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", ["l", "r"])
@pytest.mark.parametrize("shape", GELU_SHAPES, ids=ids)
def test_swoosh_epilogues(shape, name, kind, arith):  # noqa: F811
    """Against float64 of x.W + b (biases U(+-6)), and pre-activations -100 / 0 / +100 by column."""
    x, W, b, rows, pre = gemm_inputs(shape)
    epi = asr.EPI_BIAS_SWOOSHL if name == "l" else asr.EPI_BIAS_SWOOSHR
    close(gemm(x, W, b, epi, kind)[rows], zr.swoosh(pre, name), f"swoosh{name} {ids(shape)} {kind}")
    if shape[0] <= 1000:
        ext = np.float32([-100, 0, 100])[np.arange(shape[2]) % 3]
        close(gemm(x, np.zeros_like(W), ext, epi, kind), zr.swoosh(np.broadcast_to(ext, (shape[0], shape[2])), name),
              f"swoosh{name} extremes")


@pytest.mark.parametrize("shape", [(130, 5, 70, 31), (65, 3, 130, 80)], ids=ids)
def test_glu_dwconv_swooshr(shape):
    T, B, C, k = shape
    rng = np.random.default_rng(C)
    u, w = rng.uniform(-1, 1, (T, B, 2 * C)).astype(np.float32), rng.uniform(-.4, .4, (k, C)).astype(np.float32)
    b, ln = rng.uniform(-3, 3, C).astype(np.float32), ar.ragged_lengths(T, B)
    out = asr.DeviceMatrix(T * B, C)
    asr.glu_dwconv_fwd(dm(nan_past_lengths(u, ln).reshape(T * B, 2 * C)), dm(w), dm(b.reshape(C, 1)), out, T, B,
                       asr.glu_dwconv_desc(C, k, act="swooshr"), lengths=asr.device_lengths(ln))
    asr.synchronize()
    close(out.toCpu().reshape(T, B, C), zr.glu_dwconv_ref(u, w, b, ln, lambda t: zr.swoosh(t, "r")), ids(shape))


# --------------------------------------------------------------- row kernels
@pytest.mark.parametrize("mode", ["biasnorm", "biasnorm+bypass", "bypass"])
@pytest.mark.parametrize("N", [4, 70, 384, 1030])
def test_row_kernels(N, mode):
    """Ragged lengths, NaN past them; row (1, 0) equals its bias (with x[0] = 0 there): +-inf and NaN as the float64
    formula gives, compared with equal_nan."""
    T, B, ln = 6, 3, (6, 0, 3)
    rng = np.random.default_rng(N)
    x, x0 = (rng.uniform(-1, 1, (T, B, N)).astype(np.float32) for _ in range(2))
    bias, sc = rng.uniform(-.5, .5, N).astype(np.float32), rng.uniform(.2, 1, N).astype(np.float32)
    bias[0] = 0.0
    x[1, 0] = bias
    dx, dx0 = (dm(nan_past_lengths(a, ln).reshape(T * B, N)) for a in (x, x0))
    out, dl = asr.DeviceMatrix(T * B, N), asr.device_lengths(ln)
    if mode == "bypass":
        asr.bypass_fwd(dx, dx0, dm(sc.reshape(N, 1)), out, T, B, N, dl)
        ref = zr.zero_past(x0 + (x.astype(np.float64) - x0) * sc, ln)
    else:
        fused = dict(x0=dx0, bypass=dm(sc.reshape(N, 1))) if "+" in mode else {}
        asr.biasnorm_fwd(dx, dm(bias.reshape(N, 1)), 0.3, out, T, B, N, lengths=dl, **fused)
        ref = zr.biasnorm_ref(x, bias, 0.3, *((x0, sc) if "+" in mode else ()), lengths=ln)
    asr.synchronize()
    got = out.toCpu().reshape(T, B, N)
    odd = ~np.isfinite(ref)
    assert np.array_equal(got[odd].astype(np.float64), ref[odd], equal_nan=True) and odd.any() == (mode != "bypass")
    close(np.where(odd, 0, got), np.where(odd, 0, ref), f"{mode} N {N}")


# ------------------------------------------------------------------- layers
@pytest.mark.parametrize("window", list(zr.WINDOWS))
@pytest.mark.parametrize("layers", [1, 2])
def test_layer_and_stack(layers, window):
    """ZipformerLayer.from_torch / a two-layer Zipformer against the float64 layer reference; T = 70, B = 3, ragged.
    The bound is the attention cases': 2e-5, or 4 x the error of the float32 stand-in on the CPU if that exceeds 5e-6."""
    T, B, ln, E = 70, 3, (70, 1, 33), zr.LAYER["E"]
    mods = [zr.StandInLayer(**zr.LAYER, seed=s) for s in range(layers)]
    x = np.random.default_rng(5).uniform(-1, 1, (T, B, E)).astype(np.float32)
    pos = asr.compact_rel_positional_encoding(T, zr.LAYER["pos_dim"])
    allowed = torch.from_numpy(np.stack([ar.mask_matrix(T, T, T, *zr.WINDOWS[window]) & (np.arange(T) < n)[None, :]
                                         for n in ln]))
    keep = torch.from_numpy(np.arange(T)[:, None, None] < np.asarray(ln)[None, :, None])
    ref, t32 = x, torch.from_numpy(x)
    for m in mods:
        ref = zr.layer_ref(asr.ZipformerLayer.pack_torch(m), ref, 2, 8, 4, pos, T - 1, zr.WINDOWS[window], ln)
        with torch.no_grad():
            t32 = m(t32, torch.from_numpy(pos), allowed, keep) * keep
    e32 = (np.abs(t32.numpy() - ref) / (1 + np.abs(ref))).max()
    bound = max(ATOL, 4 * e32) if e32 > 5e-6 else ATOL
    print(f"torch float32 (CPU) err / (1 + |ref|) {e32:.3e}, bound {bound:.3e}")
    net = asr.Zipformer.from_torch(mods, zr.LAYER["pos_dim"], *zr.WINDOWS[window])
    got = net.forward(dm(nan_past_lengths(x, ln).reshape(T * B, E)), T, B, ln)
    asr.synchronize()
    got = got.toCpu().reshape(T, B, E)
    for b, n in enumerate(ln):
        assert not got[n:, b].any()
    close(got, ref, f"{layers} layer(s) {window}", atol=bound)
