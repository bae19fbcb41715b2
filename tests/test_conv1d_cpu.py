"""CPU checks of the Conv1d layer (asr_conv1d_out_frames, asr_conv1d_fwd,
asr.Conv1d): exported, the output-length formula, every refusal ahead of any
HIP call (the fake device pointers are never dereferenced on the host), the
float64 reference of conv1d_reference.py against torch.nn.functional.conv1d,
and Conv1d.pack_torch (layout, BatchNorm fold, padding parsing, refusals).
No GPU here."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import conv1d_reference as cr
from conftest import asr

NAMES = ["asr_conv1d_out_frames", "asr_conv1d_fwd"]
FAKE = 0x10000   # a non-NULL, 16-byte aligned "device pointer"
INT_MAX = 2 ** 31 - 1


def desc(c_in=8, c_out=16, kernel=3, stride=1, dilation=1, pad_left=1, pad_right=1, groups=1, act=0, clip=20.0):
    return asr.Conv1dDesc(c_in, c_out, kernel, stride, dilation, pad_left, pad_right, groups, act, clip)


def fwd(d, T=8, B=4, ldx=None, ldo=None, null=None):
    """asr_conv1d_fwd with fake pointers; null: name of a pointer passed as NULL."""
    p = {"x": FAKE, "lengths": FAKE, "W": FAKE, "b": FAKE, "out": FAKE, "out_lengths": FAKE}
    if null is not None:
        p[null] = None
    dp = ctypes.byref(d) if d is not None else None
    return asr.lib().asr_conv1d_fwd(dp, p["x"], d.c_in if ldx is None else ldx, p["lengths"], p["W"], p["b"],
                                    p["out"], d.c_out if ldo is None else ldo, p["out_lengths"], T, B, None)


def test_symbols_in_mirror_and_library():
    for n in NAMES:
        assert n in asr.EXPORTS, n
        assert hasattr(asr.lib(), n), n
    out = subprocess.run(["nm", "-D", "--defined-only", str(asr.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (asr_[a-z0-9_]+)$", out, flags=re.M))
    assert set(NAMES) <= exported


def test_desc_mirrors_the_header_struct():
    assert ctypes.sizeof(asr.Conv1dDesc) == 10 * 4
    assert [f[0] for f in asr.Conv1dDesc._fields_] == ["c_in", "c_out", "kernel", "stride", "dilation", "pad_left",
                                                      "pad_right", "groups", "act", "clip"]


# ------------------------------------------------------------- out_frames
def test_out_frames_formula_and_torch():
    rng = np.random.default_rng(7)
    for _ in range(300):
        k, s, d = int(rng.integers(1, 12)), int(rng.integers(1, 5)), int(rng.integers(1, 4))
        pl, pr, n = int(rng.integers(0, 8)), int(rng.integers(0, 8)), int(rng.integers(1, 60))
        got = asr.conv1d_out_frames(desc(kernel=k, stride=s, dilation=d, pad_left=pl, pad_right=pr), n)
        assert got == cr.out_frames(n, k, s, d, pl, pr), (n, k, s, d, pl, pr)
        if n + pl + pr >= d * (k - 1) + 1:
            x = torch.nn.functional.pad(torch.zeros(1, 1, n), (pl, pr))
            ref = torch.nn.functional.conv1d(x, torch.zeros(1, 1, k), stride=s, dilation=d).shape[2]
            assert got == ref, (n, k, s, d, pl, pr)
        else:
            assert got == 0


def test_out_frames_zero_and_bad_descriptor():
    d = desc(kernel=5, dilation=2, pad_left=1, pad_right=0)      # receptive field 9
    assert asr.conv1d_out_frames(d, 0) == 0
    assert asr.conv1d_out_frames(d, -3) == 0
    assert asr.conv1d_out_frames(d, 7) == 0                      # 7 + 1 < 9
    assert asr.conv1d_out_frames(d, 8) == 1
    assert asr.conv1d_out_frames(dict(c_in=4, c_out=4, kernel=3, pad_left=2), 10) == 10   # keywords
    assert asr.lib().asr_conv1d_out_frames(None, 10) < 0
    for bad in (desc(kernel=0), desc(stride=0), desc(dilation=-1), desc(pad_left=-1), desc(c_in=0), desc(act=3),
                desc(kernel=129), desc(groups=2)):
        assert asr.conv1d_out_frames(bad, 10) < 0


# --------------------------------------------------------------- refusals
@pytest.mark.parametrize("null", ["x", "W", "out"])
def test_err_arg_null_pointer(null):
    assert fwd(desc(), null=null) == asr.ASR_ERR_ARG
    assert fwd(desc(c_in=8, c_out=8, groups=8), null=null) == asr.ASR_ERR_ARG


def test_err_arg_null_descriptor():
    assert asr.lib().asr_conv1d_fwd(None, FAKE, 8, FAKE, FAKE, FAKE, FAKE, 16, FAKE, 8, 4, None) == asr.ASR_ERR_ARG


@pytest.mark.parametrize("kw", [dict(c_in=0), dict(c_out=0), dict(c_in=-4), dict(kernel=0), dict(kernel=-1),
                                dict(stride=0), dict(dilation=0), dict(pad_left=-1), dict(pad_right=-1),
                                dict(act=3), dict(act=-1), dict(act=2, clip=0.0), dict(act=2, clip=-1.0),
                                dict(act=2, clip=float("inf")), dict(act=2, clip=float("nan"))],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_err_arg_descriptor(kw):
    d = desc(**kw)
    assert fwd(d, ldx=max(d.c_in, 1), ldo=max(d.c_out, 1)) == asr.ASR_ERR_ARG


def test_err_arg_sizes():
    d = desc()
    assert fwd(d, T=0) == asr.ASR_ERR_ARG
    assert fwd(d, T=-2) == asr.ASR_ERR_ARG
    assert fwd(d, B=0) == asr.ASR_ERR_ARG
    assert fwd(d, ldx=d.c_in - 1) == asr.ASR_ERR_ARG
    assert fwd(d, ldo=d.c_out - 1) == asr.ASR_ERR_ARG
    # T_out = 0: the receptive field does not fit T + padding
    assert fwd(desc(kernel=11, pad_left=0, pad_right=0), T=10) == asr.ASR_ERR_ARG


def test_optional_pointers_are_not_argument_errors():
    """NULL lengths, bias and out_lengths are allowed: the checks pass them and
    stop at a later refusal (an unsupported kernel size here), never ASR_ERR_ARG."""
    for null in ("lengths", "b", "out_lengths"):
        assert fwd(desc(kernel=129, pad_left=64, pad_right=64), T=200, null=null) == asr.ASR_ERR_UNSUPPORTED


def test_arg_errors_come_before_unsupported():
    assert fwd(desc(kernel=129, pad_left=64, pad_right=64), T=200, ldx=7) == asr.ASR_ERR_ARG
    assert fwd(desc(kernel=129, pad_left=0, pad_right=0), T=100) == asr.ASR_ERR_ARG     # T_out = 0
    assert fwd(desc(groups=2, act=7)) == asr.ASR_ERR_ARG


@pytest.mark.parametrize("kw,T,B", [
    (dict(groups=2), 8, 4),
    (dict(groups=0), 8, 4),
    (dict(c_in=8, c_out=16, groups=8), 8, 4),              # groups == c_in but != c_out
    (dict(c_in=16, c_out=16, groups=4), 8, 4),
    (dict(kernel=129, pad_left=64, pad_right=64), 200, 4),
    (dict(stride=17), 8, 4),
    (dict(dilation=17, pad_left=17, pad_right=17), 40, 4),
    (dict(c_in=4097), 8, 4),
    (dict(c_out=4097), 8, 4),
    (dict(), 1 << 20, 1 << 12),                            # T*B > INT_MAX
    (dict(pad_left=INT_MAX - 10, pad_right=0), 100, 1),    # T + pad_left + pad_right past an int
    (dict(pad_left=INT_MAX - 5000, pad_right=0), 1000, 1),  # ... past INT_MAX - 4096
], ids=["groups2", "groups0", "groups-cin-only", "grouped", "kernel129", "stride17", "dilation17", "c_in4097",
        "c_out4097", "TB", "pad-int", "pad-margin"])
def test_err_unsupported(kw, T, B):
    assert fwd(desc(**kw), T=T, B=B) == asr.ASR_ERR_UNSUPPORTED


def test_err_unsupported_out_rows_beyond_int():
    # T*B fits an int, T_out*B does not (padding makes more frames than it takes)
    T, B = 1 << 10, (1 << 21) - 1
    d = desc(kernel=1, pad_left=1000, pad_right=0)
    assert T * B <= INT_MAX < (T + 1000) * B
    assert fwd(d, T=T, B=B) == asr.ASR_ERR_UNSUPPORTED


def test_err_unsupported_depthwise_grid():
    # depthwise: B * ceil(T_out / 64) * ceil(C / 64) workgroups in one grid dimension
    C, T, B = 4096, 65, 1 << 24
    assert T * B <= INT_MAX < B * 2 * (C // 64)
    assert fwd(desc(c_in=C, c_out=C, groups=C, kernel=1, pad_left=0, pad_right=0), T=T, B=B) == asr.ASR_ERR_UNSUPPORTED


# ---------------------------------------------------- reference vs. torch
def torch_conv(x, W, b, k, s, d, pl, pr, g, n, bi):
    """torch.nn.functional.conv1d in float64 on utterance bi's own n frames."""
    xt = torch.from_numpy(np.ascontiguousarray(x[:n, bi].astype(np.float64).T))[None]      # [1][ci][n]
    wt = torch.from_numpy(np.ascontiguousarray(np.asarray(W, np.float64).transpose(2, 1, 0)))   # [co][ci/g][k]
    bt = None if b is None else torch.from_numpy(np.asarray(b, np.float64))
    y = torch.nn.functional.conv1d(torch.nn.functional.pad(xt, (pl, pr)), wt, bt, stride=s, dilation=d, groups=g)
    return y[0].numpy().T                                                                   # [n_out][co]


@pytest.mark.parametrize("shape", cr.ALL_SHAPES, ids=lambda sh: "x".join(map(str, sh)))
def test_reference_matches_torch(shape):
    T, B, ci, co, k, s, d, pl, pr, g = shape
    x, W, b = cr.draw(shape)
    ln = cr.ragged_lengths(shape)
    assert 0 in ln and 1 in ln and T in ln
    for act, clip, tact in ((None, 20.0, lambda v: v), ("relu", 20.0, lambda v: np.maximum(v, 0)),
                            ("clip", 0.5, lambda v: np.clip(v, 0, 0.5))):
        out, oln = cr.conv1d_ref(x, W, b, k, s, d, pl, pr, g, act, clip, ln)
        assert out.shape == (cr.out_frames(T, k, s, d, pl, pr), B, co)
        for bi in range(B):
            no = cr.out_frames(ln[bi], k, s, d, pl, pr)
            assert oln[bi] == no
            assert not out[no:, bi].any()
            if no:
                ref = tact(torch_conv(x, W, b, k, s, d, pl, pr, g, ln[bi], bi))
                assert ref.shape == (no, co)
                assert np.all(np.abs(out[:no, bi] - ref) <= 1e-13 * (1 + np.abs(ref)))
    # full lengths, no bias
    out, _ = cr.conv1d_ref(x, W, None, k, s, d, pl, pr, g)
    for bi in range(B):
        ref = torch_conv(x, W, None, k, s, d, pl, pr, g, T, bi)
        assert np.all(np.abs(out[:, bi] - ref) <= 1e-13 * (1 + np.abs(ref)))


# ------------------------------------------------------------- pack_torch
def module_out(mods, x):
    """The float64 torch modules on x [T][B][c_in] time-major -> [T_out][B][c_out]."""
    with torch.no_grad():
        y = torch.from_numpy(x.astype(np.float64)).permute(1, 2, 0)      # [B][C][T]
        for m in mods:
            y = m.double()(y)
        return y.permute(2, 0, 1).numpy()


@pytest.mark.parametrize("kw", [dict(in_channels=6, out_channels=10, kernel_size=5, stride=2, padding=3),
                                dict(in_channels=6, out_channels=10, kernel_size=4, dilation=2, padding="same"),
                                dict(in_channels=6, out_channels=10, kernel_size=3, bias=False),
                                dict(in_channels=12, out_channels=12, kernel_size=7, padding=3, groups=12)],
                         ids=["strided", "same", "no-bias", "depthwise"])
def test_pack_torch_layout(kw):
    torch.manual_seed(3)
    conv = torch.nn.Conv1d(**kw)
    W, b, k = asr.Conv1d.pack_torch(conv)
    ci, co, g = kw["in_channels"], kw["out_channels"], kw.get("groups", 1)
    assert W.dtype == np.float32 and b.dtype == np.float32
    assert W.shape == (kw["kernel_size"], ci // g, co) and b.shape == (co,)
    assert k["c_in"] == ci and k["c_out"] == co and k["groups"] == g
    x = np.random.default_rng(0).uniform(-1, 1, (19, 3, ci)).astype(np.float32)
    pl, pr = k["padding"]
    out, _ = cr.conv1d_ref(x, W, b, k["kernel"], k["stride"], k["dilation"], pl, pr, g)
    ref = module_out([conv], x)
    assert out.shape == ref.shape
    assert np.all(np.abs(out - ref) <= 1e-13 * (1 + np.abs(ref)))


@pytest.mark.parametrize("groups", [1, 8], ids=["dense", "depthwise"])
def test_pack_torch_batchnorm_fold(groups):
    torch.manual_seed(5)
    ci = co = 8
    conv = torch.nn.Conv1d(ci, co, 5, stride=2, padding=2, groups=groups)
    bn = torch.nn.BatchNorm1d(co)
    with torch.no_grad():   # non-trivial running statistics and affine parameters
        bn.running_mean.copy_(torch.randn(co) * 0.3)
        bn.running_var.copy_(torch.rand(co) * 2 + 0.2)
        bn.weight.copy_(torch.rand(co) + 0.5)
        bn.bias.copy_(torch.randn(co) * 0.2)
    bn.eval()
    W, b, k = asr.Conv1d.pack_torch(conv, bn)
    assert W.dtype == np.float32 and b.dtype == np.float32
    x = np.random.default_rng(1).uniform(-1, 1, (21, 4, ci)).astype(np.float32)
    out, _ = cr.conv1d_ref(x, W, b, k["kernel"], k["stride"], k["dilation"], *k["padding"], groups)
    ref = module_out([conv, bn], x)
    assert np.all(np.abs(out - ref) <= 1e-6 * (1 + np.abs(ref)))
    # the fold rounds once: the packed values are the float64 fold's nearest float32
    scale = (bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)).detach().numpy()
    w64 = conv.weight.detach().double().numpy() * scale[:, None, None]
    assert np.array_equal(W, w64.transpose(2, 1, 0).astype(np.float32))
    b64 = (conv.bias.detach().double().numpy() - bn.running_mean.double().numpy()) * scale + bn.bias.detach().double().numpy()
    assert np.array_equal(b, b64.astype(np.float32))


def test_padding_parsing():
    P = asr.Conv1d.parse_padding
    assert P(3, 5) == (3, 3)
    assert P((2, 7), 5) == (2, 7)
    assert P((4,), 5) == (4, 4)
    assert P("valid", 5) == (0, 0)
    assert P("same", 5) == (2, 2)
    assert P("same", 4, 1, 3) == (4, 5)            # total 9: left = 4, right = 5, as torch
    assert P("causal", 5, 2, 3) == (12, 0)
    with pytest.raises(ValueError):
        P("same", 5, 2)
    with pytest.raises(ValueError):
        P("reflect", 5)
    with pytest.raises(ValueError):
        P((1, 2, 3), 5)


def test_pack_torch_refusals():
    with pytest.raises(ValueError):
        asr.Conv1d.pack_torch(torch.nn.Conv1d(4, 4, 3, padding=1, padding_mode="reflect"))
    with pytest.raises(ValueError):
        asr.Conv1d.pack_torch(torch.nn.Conv1d(8, 8, 3, groups=2))
    with pytest.raises(ValueError):
        asr.Conv1d.pack_torch(torch.nn.Conv1d(4, 8, 3, groups=4))      # groups == c_in != c_out
    with pytest.raises(ValueError):
        asr.Conv1d.pack_torch(torch.nn.Conv1d(4, 4, 3), torch.nn.BatchNorm1d(4))   # still training
    with pytest.raises(ValueError):
        asr.Conv1d.pack_torch(torch.nn.Conv1d(4, 6, 3), torch.nn.BatchNorm1d(4).eval())
