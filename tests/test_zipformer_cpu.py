"""CPU checks of the Zipformer additions: the float64 reference's rel-shift
against a double loop, the reference layer (fed by ZipformerLayer.pack_torch)
against the float32 stand-in that carries icefall's attribute names and
follows its forward, the compact positional table, and every refusal of the
new entry points in the order include/asr_amd.h states, ahead of any HIP call
(fake pointers)."""
import ctypes

import numpy as np
import pytest
import torch

import attention_reference as ar
import zipformer_reference as zr
from conftest import asr

F, F2, ARG, UNS = 0x1000, 0x2000, asr.ASR_ERR_ARG, asr.ASR_ERR_UNSUPPORTED
INT_MAX = 2 ** 31 - 1


def test_rel_shift_against_a_double_loop():
    raw = np.random.default_rng(0).uniform(-1, 1, (2, 3, 7, 13))
    got = zr.rel_shift(raw)
    for i in range(7):
        for j in range(7):
            assert np.array_equal(got[..., i, j], raw[..., i, 7 - 1 - i + j])


@pytest.mark.parametrize("window", list(zr.WINDOWS))
def test_reference_layer_matches_the_stand_in(window):
    """Pins pack_torch's mapping: q | k | p of in_proj, s | x | y of the
    non-linear attention, the table order (pos_zero = T - 1).  float32 torch
    against float64: 2e-4 relative to 1 + |ref| (a whole layer, not a kernel)."""
    T, B, ln = 21, 3, (21, 9, 17)
    layer = zr.StandInLayer(**zr.LAYER, seed=3)
    x = np.random.default_rng(1).uniform(-1, 1, (T, B, zr.LAYER["E"])).astype(np.float32)
    pos = asr.compact_rel_positional_encoding(T, zr.LAYER["pos_dim"])
    allowed = torch.from_numpy(np.stack([ar.mask_matrix(T, T, T, *zr.WINDOWS[window]) & (np.arange(T) < n)[None, :]
                                         for n in ln]))
    keep = torch.from_numpy(np.arange(T)[:, None, None] < np.asarray(ln)[None, :, None])
    with torch.no_grad():
        want = layer(torch.from_numpy(x), torch.from_numpy(pos), allowed, keep).numpy()
    ref = zr.layer_ref(asr.ZipformerLayer.pack_torch(layer), x, 2, 8, 4, pos, T - 1, zr.WINDOWS[window], ln)
    for b, n in enumerate(ln):
        assert np.all(np.abs(want[:n, b] - ref[:n, b]) <= 2e-4 * (1 + np.abs(ref[:n, b]))), (window, b)
        assert not ref[n:, b].any()


def test_compact_rel_positional_encoding():
    pe = asr.compact_rel_positional_encoding(9, 16)
    assert pe.shape == (17, 16) and pe.dtype == np.float32
    assert np.all(pe[:, -1] == 1.0)
    assert np.array_equal(pe[::-1, 1:-1:2], -pe[:, 1:-1:2]) and np.array_equal(pe[::-1, 0::2], pe[:, 0::2])
    assert np.all(pe[8, 0::2] == 1.0) and np.all(pe[8, 1:-1:2] == 0.0)


def zdesc(**kw):
    base = dict(heads=2, query_dim=8, pos_dim=4, value_heads=2, value_dim=4, score_head=0, scale=0.0, chunk=1, left=-1,
                right=-1, gate=1)
    base.update(kw)
    return asr.ZattnDesc(*base.values())


def zcall(d=None, nulls=(), Tq=8, Tk=8, B=2, n_pos=15, pos_zero=7, q0=0, k0=0, **ld):
    """asr_attention_zip_fwd with fake pointers; nulls: names passed as NULL; ld: strides by name."""
    d = zdesc() if d is None else d
    ptr = lambda n: None if n in nulls else F   # noqa: E731
    L = lambda n, v: ld.get(n, v)   # noqa: E731
    eq, ep, ev = d.heads * d.query_dim, d.heads * d.pos_dim, d.value_heads * d.value_dim
    return asr.lib().asr_attention_zip_fwd(None if "d" in nulls else ctypes.byref(d), ptr("q"), L("ldq", eq), ptr("k"),
                                           L("ldk", eq), ptr("pz"), L("ldpz", ep), ptr("v"), L("ldv", ev), ptr("sg"),
                                           L("ldsg", ev), ptr("y"), L("ldy", ev), ptr("pos"), L("ldp", ep), n_pos,
                                           pos_zero, F, None if "out" in nulls else F2, L("ldo", ev), Tq, q0, Tk, k0, B,
                                           None)


# Each refusal carries a later violation too (an unsupported width), so the order is the header's.
BAD = dict(query_dim=6)
ZIP_ARG = [dict(nulls=("d",)), dict(nulls=("q",)), dict(nulls=("k",)), dict(nulls=("v",)), dict(nulls=("out",)),
           dict(d=dict(pos_dim=-4)), dict(d=dict(gate=2)), dict(nulls=("pz",)), dict(nulls=("pos",)),
           dict(nulls=("sg",)), dict(nulls=("y",)), dict(Tq=0), dict(Tk=0), dict(B=-1), dict(d=dict(heads=0)),
           dict(d=dict(query_dim=0)), dict(d=dict(value_dim=0)), dict(d=dict(chunk=0)), dict(n_pos=0),
           dict(d=dict(value_heads=3)), dict(d=dict(score_head=2)), dict(d=dict(score_head=-1)), dict(d=dict(left=-2)),
           dict(d=dict(right=-2)), dict(q0=-1), dict(k0=-1), dict(ldq=11), dict(ldk=11), dict(ldv=7), dict(ldo=7),
           dict(ldpz=7), dict(ldp=7), dict(ldsg=7), dict(ldy=7), dict(d=dict(scale=float("nan"))),
           dict(d=dict(scale=-1.0)), dict(pos_zero=6), dict(n_pos=14)]
ZIP_UNS = [dict(d=dict(query_dim=6)), dict(d=dict(query_dim=132)), dict(d=dict(heads=64, value_heads=64, query_dim=128)),
           dict(d=dict(pos_dim=6)), dict(d=dict(pos_dim=20)), dict(d=dict(value_dim=6)),
           dict(d=dict(value_heads=1, value_dim=4100)), dict(d=dict(heads=65536, value_heads=1, query_dim=4, pos_dim=0)),
           dict(B=65536), dict(q0=INT_MAX - 70, d=dict(pos_dim=0)), dict(k0=INT_MAX - 70, d=dict(pos_dim=0)),
           dict(Tq=40000, Tk=40000, B=60000, n_pos=80001, pos_zero=40000)]


@pytest.mark.parametrize("kw", ZIP_ARG, ids=str)
def test_zip_attention_arg_errors_in_order(kw):
    kw = dict(kw)
    d = dict(BAD, **kw.pop("d", {}))
    if "ldq" not in kw and "ldk" not in kw:      # keep the strides those of the valid widths
        kw.update(ldq=12, ldk=12)
    assert zcall(zdesc(**d), **kw) == ARG


@pytest.mark.parametrize("kw", ZIP_UNS, ids=str)
def test_zip_attention_unsupported(kw):
    kw = dict(kw)
    assert zcall(zdesc(**kw.pop("d", {})), **kw) == UNS


def test_zip_attention_optional_pointers():
    """pos_dim = 0 / gate = 0: NULL pz, pos, sg, y and lengths pass the checks (the next refusal is reached)."""
    d = zdesc(pos_dim=0, gate=0, query_dim=6)
    assert zcall(d, nulls=("pz", "pos", "sg", "y"), n_pos=0, ldq=12, ldk=12) == UNS


def rows(fn, x=F, x0=F, third=F, out=F2, T=4, B=2, N=8, ldx=8, ldx0=8, ldo=8, ls=0.0):
    L = asr.lib()
    if fn == "biasnorm":
        return L.asr_biasnorm_fwd(x, ldx, third, ls, x0, ldx0, F if x0 else None, F, out, ldo, T, B, N, None)
    return L.asr_bypass_fwd(x, ldx, x0, ldx0, third, F, out, ldo, T, B, N, None)


@pytest.mark.parametrize("fn", ["biasnorm", "bypass"])
def test_row_kernels_refusals_in_order(fn):
    big = dict(N=5000)                           # a later violation rides along
    for kw in (dict(x=None), dict(third=None), dict(out=None), dict(T=0), dict(B=0), dict(ldx=4999), dict(ldo=4999),
               dict(ldx0=4999)):
        assert rows(fn, **dict(dict(big, ldx=5000, ldx0=5000, ldo=5000), **kw)) == ARG, kw
    assert rows(fn, N=0) == ARG
    assert rows(fn, N=5000, ldx=5000, ldx0=5000, ldo=5000) == UNS
    assert rows(fn, T=70000, B=70000) == UNS
    L = asr.lib()
    if fn == "biasnorm":
        assert L.asr_biasnorm_fwd(F, 8, F, 0.0, F, 8, None, F, F2, 8, 4, 2, 8, None) == ARG    # x0 without bypass
        assert L.asr_biasnorm_fwd(F, 8, F, 0.0, None, 0, F, F, F2, 8, 4, 2, 8, None) == ARG
        assert rows(fn, ls=float("inf"), N=5000, ldx=5000, ldx0=5000, ldo=5000) == ARG
        assert L.asr_biasnorm_fwd(F, 5000, F, 0.0, None, 0, None, None, F2, 5000, 4, 2, 5000, None) == UNS
    else:
        assert rows(fn, x0=None) == ARG


def test_new_enums_and_exports():
    assert (asr.EPI_BIAS_SWOOSHL, asr.EPI_BIAS_SWOOSHR, asr.GLU_ACT_SWOOSHR) == (7, 8, 4)
    assert asr.lib().asr_linear_fwd(F, F, None, F2, 8, 8, 8, asr.EPI_BIAS_SWOOSHL, None) == ARG   # needs a bias
    assert asr.lib().asr_linear_fwd(F, F, F, F2, 0, 8, 8, asr.EPI_BIAS_SWOOSHR, None) == ARG
    assert asr.lib().asr_linear_fwd(F, F, F, F2, 8, 8, 8, 9, None) == ARG                       # the next value is free
    d = asr.glu_dwconv_desc(16, 90, act="swooshr")                                              # accepted: the next check
    assert asr.lib().asr_glu_dwconv_fwd(ctypes.byref(d), F, 32, F, F, F, F2, 16, 8, 4, None) == UNS
    for name in ("asr_attention_zip_fwd", "asr_biasnorm_fwd", "asr_bypass_fwd"):
        assert name in asr.EXPORTS and hasattr(asr.lib(), name)
