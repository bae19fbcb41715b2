"""CPU checks of the Conv2d layer and the subsampling front end
(asr_conv2d_out_frames, asr_conv2d_out_feats, asr_conv2d_fwd, asr.Conv2d,
asr.Conv2dSubsampling): exported, the struct mirrors the header, the two
counts against the formula and torch's output shape, every refusal ahead of
any HIP call (the fake device pointers are never dereferenced on the host),
the float64 reference of conv2d_reference.py against
torch.nn.functional.conv2d, Conv2d.pack_torch (layout, BatchNorm fold,
refusals), the Linear's permutation and scale fold, and frames(n) against the
stand-ins' length rules.  No GPU here."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import conv2d_reference as c2
from conftest import asr

NAMES = ["asr_conv2d_out_frames", "asr_conv2d_out_feats", "asr_conv2d_fwd"]
FIELDS = ["c_in", "c_out", "feat_in", "kernel_t", "kernel_f", "stride_t", "stride_f", "pad_t_lo", "pad_t_hi",
          "pad_f_lo", "pad_f_hi", "groups", "act", "clip"]
FAKE = 0x10000   # a non-NULL, 16-byte aligned "device pointer"
INT_MAX = 2 ** 31 - 1
ARG, UNSUP = asr.ASR_ERR_ARG, asr.ASR_ERR_UNSUPPORTED


def desc(c_in=4, c_out=16, feat_in=20, kernel_t=3, kernel_f=3, stride_t=2, stride_f=2, pad_t_lo=0, pad_t_hi=0,
         pad_f_lo=0, pad_f_hi=0, groups=1, act=1, clip=20.0):
    return asr.Conv2dDesc(c_in, c_out, feat_in, kernel_t, kernel_f, stride_t, stride_f, pad_t_lo, pad_t_hi,
                          pad_f_lo, pad_f_hi, groups, act, clip)


def fwd(d, T=9, B=4, ldx=None, ldo=None, null=None):
    """asr_conv2d_fwd with fake pointers; ldx / ldo default to the rows' content; null: a pointer passed as NULL."""
    p = {"x": FAKE, "lengths": FAKE, "W": FAKE, "b": FAKE, "out": FAKE, "out_lengths": FAKE}
    if null is not None:
        p[null] = None
    fo = c2.count(d.feat_in, d.kernel_f, max(d.stride_f, 1), d.pad_f_lo, d.pad_f_hi)
    return asr.lib().asr_conv2d_fwd(ctypes.byref(d), p["x"], d.feat_in * d.c_in if ldx is None else ldx, p["lengths"],
                                    p["W"], p["b"], p["out"], fo * d.c_out if ldo is None else ldo, p["out_lengths"],
                                    T, B, None)


def test_symbols_in_mirror_and_library():
    for n in NAMES:
        assert n in asr.EXPORTS, n
        assert hasattr(asr.lib(), n), n
    out = subprocess.run(["nm", "-D", "--defined-only", str(asr.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (asr_[a-z0-9_]+)$", out, flags=re.M))
    assert set(NAMES) <= exported


def test_desc_mirrors_the_header_struct():
    assert ctypes.sizeof(asr.Conv2dDesc) == 14 * 4
    assert [f[0] for f in asr.Conv2dDesc._fields_] == FIELDS
    header = (Path(__file__).resolve().parents[1] / "include" / "asr_amd.h").read_text()
    body = re.search(r"typedef struct asr_conv2d_desc \{(.*?)\} asr_conv2d_desc;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip()
             for n in re.sub(r"^\s*(int|float)\s", "", decl.strip()).split(",")]
    assert names == FIELDS
    assert [f[1] for f in asr.Conv2dDesc._fields_] == [ctypes.c_int] * 13 + [ctypes.c_float]
    assert re.findall(r"\b(int|float)\b", body) == ["int"] * 8 + ["float"]      # the declarations, in order


# ------------------------------------------------------------------ counts
def test_counts_formula_and_torch():
    rng = np.random.default_rng(7)
    for _ in range(300):
        kt, kf = int(rng.integers(1, 8)), int(rng.integers(1, 8))
        st, sf = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        ptl, pth, pfl, pfh = (int(v) for v in rng.integers(0, 5, 4))
        n, F = int(rng.integers(1, 40)), int(rng.integers(1, 30))
        d = desc(feat_in=F, kernel_t=kt, kernel_f=kf, stride_t=st, stride_f=sf, pad_t_lo=ptl, pad_t_hi=pth,
                 pad_f_lo=pfl, pad_f_hi=pfh)
        fo, no = c2.count(F, kf, sf, pfl, pfh), c2.count(n, kt, st, ptl, pth)
        if fo == 0:                      # no output bin: the descriptor itself is refused
            assert asr.conv2d_out_feats(d) == -ARG and asr.conv2d_out_frames(d, n) == -ARG
            continue
        assert asr.conv2d_out_feats(d) == fo and asr.conv2d_out_frames(d, n) == no, (n, F, kt, kf, st, sf)
        if no:
            x = torch.nn.functional.pad(torch.zeros(1, 1, n, F), (pfl, pfh, ptl, pth))
            ref = torch.nn.functional.conv2d(x, torch.zeros(1, 1, kt, kf), stride=(st, sf)).shape
            assert (no, fo) == (ref[2], ref[3]), (n, F, kt, kf, st, sf)


def test_out_frames_is_the_toolkits_mask_slicing():
    d = desc()                            # kernel 3, stride 2, unpadded
    for n in range(1, 40):
        assert asr.conv2d_out_frames(d, n) == len(range(n)[:-2:2]), n


def test_counts_zero_keywords_and_bad_descriptor():
    d = desc(kernel_t=5, pad_t_lo=1)
    assert asr.conv2d_out_frames(d, 0) == 0 and asr.conv2d_out_frames(d, -3) == 0
    assert asr.conv2d_out_frames(d, 3) == 0 and asr.conv2d_out_frames(d, 4) == 1
    kw = dict(c_in=1, c_out=8, feat_in=80, kernel_t=3, kernel_f=3, stride_t=2, stride_f=2)
    assert asr.conv2d_out_frames(kw, 100) == 49 and asr.conv2d_out_feats(kw) == 39
    assert asr.lib().asr_conv2d_out_frames(None, 10) == -ARG and asr.lib().asr_conv2d_out_feats(None) == -ARG
    for bad in (desc(kernel_t=0), desc(kernel_f=0), desc(stride_t=0), desc(stride_f=-1), desc(pad_t_lo=-1),
                desc(pad_f_hi=-1), desc(c_in=0), desc(feat_in=0), desc(act=3), desc(feat_in=2)):
        assert asr.conv2d_out_frames(bad, 10) == -ARG and asr.conv2d_out_feats(bad) == -ARG
    for bad in (desc(kernel_t=17), desc(kernel_f=17), desc(groups=2), desc(stride_f=17), desc(feat_in=4097),
                desc(pad_f_lo=4097)):
        assert asr.conv2d_out_frames(bad, 40) == -UNSUP and asr.conv2d_out_feats(bad) == -UNSUP


# --------------------------------------------------------------- refusals
@pytest.mark.parametrize("null", ["x", "W", "out"])
def test_err_arg_null_pointer(null):
    assert fwd(desc(), null=null) == ARG
    assert fwd(desc(c_in=8, c_out=8, groups=8), null=null) == ARG


def test_err_arg_null_descriptor():
    assert asr.lib().asr_conv2d_fwd(None, FAKE, 80, FAKE, FAKE, FAKE, FAKE, 144, FAKE, 9, 4, None) == ARG


@pytest.mark.parametrize("kw", [dict(c_in=0), dict(c_out=0), dict(c_in=-4), dict(feat_in=0), dict(feat_in=-1),
                                dict(kernel_t=0), dict(kernel_f=0), dict(kernel_t=-1), dict(stride_t=0),
                                dict(stride_f=0), dict(pad_t_lo=-1), dict(pad_t_hi=-1), dict(pad_f_lo=-1),
                                dict(pad_f_hi=-1), dict(act=3), dict(act=-1), dict(act=2, clip=0.0),
                                dict(act=2, clip=-1.0), dict(act=2, clip=float("inf")), dict(act=2, clip=float("nan")),
                                dict(feat_in=2), dict(feat_in=4, kernel_f=5, pad_f_hi=0)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_err_arg_descriptor(kw):
    assert fwd(desc(**kw), ldx=1 << 20, ldo=1 << 20) == ARG


def test_err_arg_sizes():
    d = desc()                            # rows of 80 floats in, 9 * 16 = 144 out
    assert fwd(d, T=0) == ARG
    assert fwd(d, T=-2) == ARG
    assert fwd(d, B=0) == ARG
    assert fwd(d, ldx=79) == ARG
    assert fwd(d, ldo=143) == ARG
    assert fwd(d, T=2) == ARG             # T_out = 0: the kernel does not fit T + padding


def test_optional_pointers_are_not_argument_errors():
    """NULL lengths, bias and out_lengths are allowed: the checks pass them and
    stop at a later refusal (an unsupported kernel size here), never ASR_ERR_ARG."""
    for null in ("lengths", "b", "out_lengths"):
        assert fwd(desc(kernel_t=17), T=40, null=null) == UNSUP


def test_arg_errors_come_before_unsupported():
    assert fwd(desc(kernel_t=17), T=40, ldx=79) == ARG
    assert fwd(desc(kernel_t=17), T=10) == ARG                       # T_out = 0
    assert fwd(desc(kernel_f=17, feat_in=16), ldx=64, ldo=1 << 20) == ARG   # F_out = 0
    assert fwd(desc(groups=2, act=7)) == ARG
    assert fwd(desc(c_in=4097), ldx=80) == ARG


@pytest.mark.parametrize("kw,T,B", [
    (dict(groups=2), 9, 4),
    (dict(groups=0), 9, 4),
    (dict(groups=4), 9, 4),                                # groups == c_in but != c_out
    (dict(c_in=16, c_out=16, groups=4), 9, 4),
    (dict(kernel_t=17), 40, 4),
    (dict(kernel_f=17), 9, 4),
    (dict(stride_t=17), 9, 4),
    (dict(stride_f=17), 9, 4),
    (dict(c_in=4097), 9, 4),
    (dict(c_out=4097), 9, 4),
    (dict(feat_in=4097), 9, 4),
    (dict(pad_f_lo=4097), 9, 4),
    (dict(pad_f_hi=4097), 9, 4),
    (dict(), 1 << 20, 1 << 12),                            # T*B > INT_MAX
    (dict(kernel_t=1, stride_t=1, pad_t_lo=1000), 1 << 10, (1 << 21) - 1),   # T_out*B > INT_MAX
    (dict(stride_t=1), 1 << 15, 1 << 15),                  # T_out*B fits, T_out*B*F_out does not
    (dict(c_in=4096, c_out=4096, groups=4096, stride_t=1), 1 << 15, 1 << 15),   # the same, depthwise
    (dict(pad_t_lo=INT_MAX - 10), 100, 1),                 # T + pad_t_lo + pad_t_hi past an int
    (dict(pad_t_lo=INT_MAX - 5000), 1000, 1),              # ... past INT_MAX - 4096
], ids=["groups2", "groups0", "groups-cin-only", "grouped", "kernel_t17", "kernel_f17", "stride_t17", "stride_f17",
        "c_in4097", "c_out4097", "feat_in4097", "pad_f_lo4097", "pad_f_hi4097", "TB", "ToutB", "flat-rows",
        "flat-rows-depthwise", "pad-int", "pad-margin"])
def test_err_unsupported(kw, T, B):
    assert fwd(desc(**kw), T=T, B=B) == UNSUP


# ---------------------------------------------------- reference vs. torch
def torch_conv(x, W, b, shape, n, bi):
    """torch.nn.functional.conv2d in float64 on utterance bi's own n frames: [n_out][F_out][c_out]."""
    T, B, F, ci, co, kt, kf, st, sf, ptl, pth, pfl, pfh, g = shape
    xt = torch.from_numpy(np.ascontiguousarray(x[:n, bi].astype(np.float64).transpose(2, 0, 1)))[None]   # [1][ci][n][F]
    wt = torch.from_numpy(np.ascontiguousarray(np.asarray(W, np.float64).transpose(3, 2, 0, 1)))          # [co][ci/g][kt][kf]
    bt = None if b is None else torch.from_numpy(np.asarray(b, np.float64))
    y = torch.nn.functional.conv2d(torch.nn.functional.pad(xt, (pfl, pfh, ptl, pth)), wt, bt, stride=(st, sf), groups=g)
    return y[0].numpy().transpose(1, 2, 0)


@pytest.mark.parametrize("shape", c2.ALL_SHAPES, ids=c2.ids)
def test_reference_matches_torch(shape):
    T, B, F, ci, co, kt, kf, st, sf, ptl, pth, pfl, pfh, g = shape
    x, W, b = c2.draw(shape)
    ln = c2.ragged_lengths(shape)
    assert 0 in ln and T in ln
    for act, clip, tact in ((None, 20.0, lambda v: v), ("relu", 20.0, lambda v: np.maximum(v, 0)),
                            ("clip", 0.5, lambda v: np.clip(v, 0, 0.5))):
        out, oln = c2.conv2d_ref(x, W, b, st, sf, (ptl, pth), (pfl, pfh), g, act, clip, ln)
        assert out.shape == (c2.out_frames(shape, T), B, c2.out_feats(shape), co)
        for bi in range(B):
            no = c2.out_frames(shape, ln[bi])
            assert oln[bi] == no
            assert not out[no:, bi].any()
            if no:
                ref = tact(torch_conv(x, W, b, shape, ln[bi], bi))
                assert ref.shape == out[:no, bi].shape
                assert np.all(np.abs(out[:no, bi] - ref) <= 1e-13 * (1 + np.abs(ref)))
    out, _ = c2.conv2d_ref(x, W, None, st, sf, (ptl, pth), (pfl, pfh), g)      # full lengths, no bias
    for bi in range(B):
        ref = torch_conv(x, W, None, shape, T, bi)
        assert np.all(np.abs(out[:, bi] - ref) <= 1e-13 * (1 + np.abs(ref)))


# ------------------------------------------------------------- pack_torch
def module_out(mods, x):
    """The float64 torch modules on x [T][B][F][c_in] -> [T_out][B][F_out][c_out]."""
    with torch.no_grad():
        y = torch.from_numpy(x.astype(np.float64)).permute(1, 3, 0, 2)      # [B][C][T][F]
        for m in mods:
            y = m.double()(y)
        return y.permute(2, 0, 3, 1).numpy()


@pytest.mark.parametrize("kw", [dict(in_channels=3, out_channels=10, kernel_size=3, stride=2),
                                dict(in_channels=6, out_channels=10, kernel_size=(5, 3), stride=(3, 1), padding=(2, 1)),
                                dict(in_channels=6, out_channels=4, kernel_size=(1, 4), bias=False, padding="valid"),
                                dict(in_channels=12, out_channels=12, kernel_size=3, stride=2, padding=1, groups=12)],
                         ids=["strided", "non-square", "no-bias-valid", "depthwise"])
def test_pack_torch_layout(kw):
    torch.manual_seed(3)
    conv = torch.nn.Conv2d(**kw)
    W, b, k = asr.Conv2d.pack_torch(conv)
    ci, co, g = kw["in_channels"], kw["out_channels"], kw.get("groups", 1)
    kt, kf = conv.kernel_size
    assert W.dtype == np.float32 and b.dtype == np.float32
    assert W.shape == (kt, kf, ci // g, co) and b.shape == (co,)
    assert (k["c_in"], k["c_out"], k["groups"], k["kernel"], k["stride"]) == (ci, co, g, (kt, kf), tuple(conv.stride))
    x = np.random.default_rng(0).uniform(-1, 1, (13, 2, 9, ci)).astype(np.float32)
    out, _ = c2.conv2d_ref(x, W, b, *k["stride"], *k["padding"], g)
    ref = module_out([conv], x)
    assert out.shape == ref.shape
    assert np.all(np.abs(out - ref) <= 1e-13 * (1 + np.abs(ref)))


@pytest.mark.parametrize("groups", [1, 8], ids=["dense", "depthwise"])
def test_pack_torch_batchnorm_fold(groups):
    torch.manual_seed(5)
    ci = co = 8
    conv = torch.nn.Conv2d(ci, co, 3, stride=2, padding=1, groups=groups)
    bn = torch.nn.BatchNorm2d(co)
    with torch.no_grad():   # non-trivial running statistics and affine parameters
        bn.running_mean.copy_(torch.randn(co) * 0.3)
        bn.running_var.copy_(torch.rand(co) * 2 + 0.2)
        bn.weight.copy_(torch.rand(co) + 0.5)
        bn.bias.copy_(torch.randn(co) * 0.2)
    bn.eval()
    W, b, k = asr.Conv2d.pack_torch(conv, bn)
    assert W.dtype == np.float32 and b.dtype == np.float32
    x = np.random.default_rng(1).uniform(-1, 1, (11, 3, 7, ci)).astype(np.float32)
    out, _ = c2.conv2d_ref(x, W, b, *k["stride"], *k["padding"], groups)
    ref = module_out([conv, bn], x)
    assert np.all(np.abs(out - ref) <= 1e-6 * (1 + np.abs(ref)))
    # the fold rounds once: the packed values are the float64 fold's nearest float32
    scale = (bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)).detach().numpy()
    w64 = conv.weight.detach().double().numpy() * scale[:, None, None, None]
    assert np.array_equal(W, w64.transpose(2, 3, 1, 0).astype(np.float32))
    b64 = (conv.bias.detach().double().numpy() - bn.running_mean.double().numpy()) * scale + bn.bias.detach().double().numpy()
    assert np.array_equal(b, b64.astype(np.float32))


def test_padding_parsing():
    P = asr.Conv2d.parse_padding
    assert P(1) == ((1, 1), (1, 1))
    assert P((2, 0)) == ((2, 2), (0, 0))
    assert P(((2, 0), (0, 1))) == ((2, 0), (0, 1))
    assert P("valid") == ((0, 0), (0, 0))
    for bad in ("same", "reflect", (1, 2, 3)):
        with pytest.raises(ValueError):
            P(bad)


def test_pack_torch_refusals():
    C = torch.nn.Conv2d
    for bad in (C(4, 4, 3, padding=1, padding_mode="reflect"), C(4, 4, 3, dilation=2), C(4, 4, 3, dilation=(1, 2)),
                C(8, 8, 3, groups=2), C(4, 8, 3, groups=4), C(4, 4, 3, padding="same")):
        with pytest.raises(ValueError):
            asr.Conv2d.pack_torch(bad)
    with pytest.raises(ValueError):
        asr.Conv2d.pack_torch(C(4, 4, 3), torch.nn.BatchNorm2d(4))             # still training
    with pytest.raises(ValueError):
        asr.Conv2d.pack_torch(C(4, 6, 3), torch.nn.BatchNorm2d(4).eval())


# ------------------------------------------------- the subsampling module
def test_linear_permutation_and_scale_fold():
    torch.manual_seed(9)
    C, Fo, E, scale = 3, 4, 5, float(np.sqrt(5.0))
    lin = torch.nn.Linear(C * Fo, E).double()
    W, b = asr.Conv2dSubsampling.pack_linear(lin, C, Fo, scale)
    assert W.dtype == np.float32 and W.shape == (Fo * C, E) and b.shape == (E,)
    w64 = lin.weight.detach().numpy() * scale
    for f in range(Fo):
        for c in range(C):
            assert np.array_equal(W[f * C + c], w64[:, c * Fo + f].astype(np.float32))
    assert np.array_equal(b, (lin.bias.detach().numpy() * scale).astype(np.float32))
    # the same product as the toolkits' order: y[t] = out(x[c][f] flattened c-major) * scale
    x = np.random.default_rng(0).uniform(-1, 1, (Fo, C))                   # ours: [f][c]
    ours = x.reshape(-1) @ W.astype(np.float64) + b
    with torch.no_grad():
        ref = lin(torch.from_numpy(x.T.copy().reshape(-1))).numpy() * scale
    assert np.all(np.abs(ours - ref) <= 1e-6 * (1 + np.abs(ref)))
    with pytest.raises(ValueError):
        asr.Conv2dSubsampling.pack_linear(lin, C, Fo + 1)
    W1, b1 = asr.Conv2dSubsampling.pack_linear(torch.nn.Linear(C * Fo, E, bias=False), C, Fo)
    assert not b1.any() and W1.shape == (Fo * C, E)


def test_pack_torch_walk_refusals():
    N = torch.nn
    with pytest.raises(ValueError):
        asr.Conv2dSubsampling.pack_torch(N.Sequential(N.Conv2d(1, 4, 3, 2), N.Tanh()), N.Linear(36, 4), 20)
    with pytest.raises(ValueError):
        asr.Conv2dSubsampling.pack_torch(N.Sequential(N.ReLU(), N.Conv2d(1, 4, 3, 2)), N.Linear(36, 4), 20)
    with pytest.raises(ValueError):
        asr.Conv2dSubsampling.pack_torch(N.Sequential(), N.Linear(36, 4), 20)
    with pytest.raises(ValueError):   # out.in_features != c_out * F_out (4 * 9)
        asr.Conv2dSubsampling.pack_torch(N.Sequential(N.Conv2d(1, 4, 3, 2), N.ReLU()), N.Linear(40, 4), 20)
    with pytest.raises(ValueError):   # dilation
        asr.Conv2dSubsampling.pack_torch(N.Sequential(N.Conv2d(1, 4, 3, 2, dilation=2)), N.Linear(32, 4), 20)


@pytest.mark.parametrize("name", c2.STAND_INS)
def test_frames_equal_the_stand_ins_length_rule(name):
    """The layers' out_frames chained (what Conv2dSubsampling.frames does) against the
    toolkits' length rules and against the stand-in's own output length."""
    F, C, E = 20, 8, 8
    mod, conv, lin, scale = c2.make_stand_in(name, F, C, E)
    layers, w, b = asr.Conv2dSubsampling.pack_torch(conv, lin, F, scale)
    assert w.shape == (lin.in_features, E) and b.shape == (E,)
    assert [kw["act"] for kw in layers] == (["relu", None, "relu"] if name == "nemo_dw_striding"
                                            else ["relu"] * len(layers))
    descs = [asr.Conv2d.make_desc(**{k: v for k, v in kw.items() if k not in ("weight", "bias")}) for kw in layers]

    def frames(n):
        for d in descs:
            n = asr.conv2d_out_frames(d, n)
        return n
    for n in range(1, 40):
        assert frames(n) == max(mod.length(n), 0), n
        if frames(n):
            with torch.no_grad():
                assert mod(torch.zeros(1, n, F, dtype=torch.float64)).shape == (1, frames(n), E)


def test_causal_moves_the_time_padding_to_the_front():
    mod, conv, lin, scale = c2.make_stand_in("nemo_striding", 20, 8, 8)
    layers, _, _ = asr.Conv2dSubsampling.pack_torch(conv, lin, 20, causal=True)
    assert [kw["padding"] for kw in layers] == [((2, 0), (1, 1))] * 2
    layers, _, _ = asr.Conv2dSubsampling.pack_torch(conv, lin, 20)
    assert [kw["padding"] for kw in layers] == [((1, 1), (1, 1))] * 2
