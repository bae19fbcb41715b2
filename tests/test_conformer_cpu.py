"""CPU checks of the Conformer additions (ASR_EPI_BIAS_SILU, asr_glu_dwconv_fwd,
asr.ConformerConv / ConformerLayer): exported, the descriptor's layout, the
float64 restatement of conformer_reference.py against torch.nn.functional.glu /
conv1d / silu, every refusal ahead of any HIP call in the documented order (the
fake device pointers are never dereferenced on the host), and the packing
(BatchNorm fold, the exact 1/2 fold, refusals, the torchaudio-layout adapter).
No GPU here."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import conformer_reference as cf
from conftest import asr

FAKE, FAKE2 = 0x10000, 0x20000   # non-NULL "device pointers"
INT_MAX = 2 ** 31 - 1


def desc(channels=16, kernel=3, pad_left=1, pad_right=1, act=2):
    return asr.GluDwconvDesc(channels, kernel, pad_left, pad_right, act)


def fwd(d, T=8, B=4, ldu=None, ldo=None, null=None, out=FAKE2):
    """asr_glu_dwconv_fwd with fake pointers; null: name of a pointer passed as NULL."""
    p = {"u": FAKE, "lengths": FAKE, "w": FAKE, "b": FAKE, "out": out}
    if null is not None:
        p[null] = None
    return asr.lib().asr_glu_dwconv_fwd(ctypes.byref(d), p["u"], 2 * d.channels if ldu is None else ldu, p["lengths"],
                                        p["w"], p["b"], p["out"], d.channels if ldo is None else ldo, T, B, None)


def test_symbols_in_mirror_and_library():
    assert "asr_glu_dwconv_fwd" in asr.EXPORTS and hasattr(asr.lib(), "asr_glu_dwconv_fwd")
    out = subprocess.run(["nm", "-D", "--defined-only", str(asr.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    assert "asr_glu_dwconv_fwd" in set(re.findall(r" T (asr_[a-z0-9_]+)$", out, flags=re.M))
    assert asr.EPI_BIAS_SILU == 4
    assert (asr.GLU_ACT_NONE, asr.GLU_ACT_RELU, asr.GLU_ACT_SILU) == (0, 1, 2)
    for name in ("glu_dwconv_desc", "glu_dwconv_fwd", "ConformerConv", "ConformerLayer", "Conformer"):
        assert hasattr(asr, name), name


def test_desc_and_constants_mirror_the_header():
    assert ctypes.sizeof(asr.GluDwconvDesc) == 5 * 4
    assert [f[0] for f in asr.GluDwconvDesc._fields_] == ["channels", "kernel", "pad_left", "pad_right", "act"]
    header = (asr.PKG_DIR.parent / "include" / "asr_amd.h").read_text()
    m = re.search(r"typedef struct asr_glu_dwconv_desc \{(.*?)\} asr_glu_dwconv_desc;", header, flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [n.strip() for decl in re.findall(r"int ([^;]+);", body) for n in decl.split(",")]
    assert names == [f[0] for f in asr.GluDwconvDesc._fields_]
    assert int(re.search(r"#define ASR_GLU_DWCONV_MAX_KERNEL (\d+)", header).group(1)) == asr.GLU_DWCONV_MAX_KERNEL \
        == cf.MAX_KERNEL >= 63
    assert re.search(r"ASR_EPI_BIAS_SILU = 4\b", header)
    assert re.search(r"ASR_GLU_ACT_NONE = 0, ASR_GLU_ACT_RELU = 1, ASR_GLU_ACT_SILU = 2", header)
    d = asr.glu_dwconv_desc(10, 4)
    assert (d.pad_left, d.pad_right, d.act) == (1, 2, asr.GLU_ACT_SILU)            # "same", as torch splits it
    d = asr.glu_dwconv_desc(10, 5, pad_right=0, act=None)
    assert (d.pad_left, d.pad_right, d.act) == (4, 0, asr.GLU_ACT_NONE)


# ---------------------------------------------------- reference vs. torch
@pytest.mark.parametrize("shape", cf.GLU_SHAPES, ids=cf.ids)
def test_reference_matches_torch(shape):
    T, B, C, k, pl, pr = shape
    assert pl + pr == k - 1
    u, w, b = cf.draw_glu(shape)
    ln = cf.glu_lengths(shape)
    assert 1 in ln and max(ln) > T
    F = torch.nn.functional
    wt = torch.from_numpy(np.ascontiguousarray(w.astype(np.float64).T))[:, None, :]       # [C][1][k]
    bt = torch.from_numpy(b.astype(np.float64))
    for act, tact in ((None, lambda v: v), ("relu", torch.relu), ("silu", F.silu)):
        out = cf.glu_dwconv_ref(cf.nan_past_lengths(u, ln), w, b, k, pl, act, ln)
        assert out.shape == (T, B, C)
        for bi, n in enumerate(ln):
            n = min(n, T)
            assert not out[n:, bi].any()
            if n:
                x = torch.from_numpy(u[:n, bi].astype(np.float64).T.copy())[None]       # [1][2C][n]
                y = tact(F.conv1d(F.pad(F.glu(x, dim=1), (pl, pr)), wt, bt, groups=C))[0].numpy().T
                assert y.shape == (n, C)
                assert np.all(np.abs(out[:n, bi] - y) <= 1e-13 * (1 + np.abs(y)))
    # no bias, no lengths
    out = cf.glu_dwconv_ref(u, w, None, k, pl)
    x = torch.from_numpy(u.astype(np.float64)).permute(1, 2, 0)
    y = F.conv1d(F.pad(F.glu(x, dim=1), (pl, pr)), wt, None, groups=C).permute(2, 0, 1).numpy()
    assert np.all(np.abs(out - y) <= 1e-13 * (1 + np.abs(y)))


# --------------------------------------------------------------- refusals
@pytest.mark.parametrize("null", ["u", "w", "out"])
def test_err_arg_null_pointer(null):
    assert fwd(desc(), null=null) == asr.ASR_ERR_ARG


def test_err_arg_null_descriptor():
    assert asr.lib().asr_glu_dwconv_fwd(None, FAKE, 32, FAKE, FAKE, FAKE, FAKE2, 16, 8, 4, None) == asr.ASR_ERR_ARG


@pytest.mark.parametrize("kw", [dict(channels=0), dict(channels=-4), dict(kernel=0), dict(kernel=-1),
                                dict(pad_left=-1, pad_right=3), dict(pad_right=-1, pad_left=3), dict(act=3),
                                dict(act=-1)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_err_arg_descriptor(kw):
    assert fwd(desc(**kw), ldu=32, ldo=16) == asr.ASR_ERR_ARG


def test_err_arg_sizes_and_aliasing():
    d = desc()
    assert fwd(d, T=0) == asr.ASR_ERR_ARG
    assert fwd(d, T=-2) == asr.ASR_ERR_ARG
    assert fwd(d, B=0) == asr.ASR_ERR_ARG
    assert fwd(d, ldu=2 * d.channels - 1) == asr.ASR_ERR_ARG
    assert fwd(d, ldu=d.channels) == asr.ASR_ERR_ARG              # one half only
    assert fwd(d, ldo=d.channels - 1) == asr.ASR_ERR_ARG
    assert fwd(d, out=FAKE) == asr.ASR_ERR_ARG                    # d_out == d_u
    assert fwd(desc(channels=INT_MAX), ldu=INT_MAX, ldo=INT_MAX) == asr.ASR_ERR_ARG    # 2C does not wrap


def test_optional_pointers_are_not_argument_errors():
    """NULL lengths and bias are allowed: the checks pass them and stop at a
    later refusal (an unsupported kernel size here), never ASR_ERR_ARG."""
    k = cf.MAX_KERNEL + 1
    for null in ("lengths", "b"):
        assert fwd(desc(kernel=k, pad_left=k - 1, pad_right=0), T=200, null=null) == asr.ASR_ERR_UNSUPPORTED


def test_arg_errors_come_before_unsupported():
    k = cf.MAX_KERNEL + 1
    assert fwd(desc(kernel=k, pad_left=k - 1, pad_right=0), ldu=7) == asr.ASR_ERR_ARG
    assert fwd(desc(kernel=k, pad_left=k - 1, pad_right=0, act=7)) == asr.ASR_ERR_ARG
    assert fwd(desc(pad_left=5), out=FAKE) == asr.ASR_ERR_ARG
    assert fwd(desc(pad_left=5), T=1 << 20, B=1 << 12, ldo=3) == asr.ASR_ERR_ARG


@pytest.mark.parametrize("kw,T,B", [
    (dict(pad_left=2), 8, 4),                                              # pads sum to k
    (dict(pad_left=0, pad_right=0), 8, 4),                                 # "valid"
    (dict(pad_left=INT_MAX, pad_right=INT_MAX), 8, 4),                     # the sum does not wrap
    (dict(kernel=cf.MAX_KERNEL + 1, pad_left=cf.MAX_KERNEL, pad_right=0), 200, 4),
    (dict(kernel=128, pad_left=64, pad_right=63), 200, 4),
    (dict(), 1 << 20, 1 << 12),                                            # T*B > INT_MAX
    (dict(), INT_MAX - 100, 1),                                            # a tile's frame index past an int
    (dict(channels=1 << 20, kernel=1, pad_left=0, pad_right=0), 65, 1 << 20),   # 2^20 * 2 * 2^14 workgroups
], ids=["pads-long", "pads-short", "pads-wrap", "kernel-limit", "kernel128", "TB", "T-margin", "grid"])
def test_err_unsupported(kw, T, B):
    assert fwd(desc(**kw), T=T, B=B) == asr.ASR_ERR_UNSUPPORTED


@pytest.mark.parametrize("epi", ["EPI_BIAS_SILU", "EPI_BIAS"])
def test_linear_silu_needs_a_bias(epi):
    L = asr.lib()
    assert L.asr_linear_fwd(FAKE, FAKE, None, FAKE2, 8, 8, 8, getattr(asr, epi), None) == asr.ASR_ERR_ARG
    assert L.asr_linear_fwd(FAKE, FAKE, FAKE, FAKE2, 0, 8, 8, asr.EPI_BIAS_SILU, None) == asr.ASR_ERR_ARG
    assert L.asr_linear_fwd(FAKE, FAKE, FAKE, FAKE2, 8, 8, 8, 5, None) == asr.ASR_ERR_ARG   # the next value is free


# ------------------------------------------------------------- pack_torch
def conv_parts(E=12, k=7, padding="same", norm="batch", seed=3):
    return cf.draw_module(cf.ConvModule(E, k, padding, norm), seed)


@pytest.mark.parametrize("padding", ["same", "causal", (2, 4)], ids=["same", "causal", "manual"])
def test_conv_pack_batchnorm_fold(padding):
    E, k = 12, 7
    mod = conv_parts(E, k, padding)
    ln, pw1, dw, bn, pw2 = mod.parts()
    p = asr.ConformerConv.pack_torch(ln, pw1, dw, bn, pw2, padding=None if padding == "same" else padding)
    want = {"same": (3, 3), "causal": (6, 0)}.get(padding, padding)
    assert p["padding"] == want
    assert p["w1"].shape == (E, 2 * E) and p["w2"].shape == (E, E) and p["wd"].shape == (k, E)
    assert all(p[n].dtype == np.float32 for n in ("w1", "b1", "wd", "bd", "w2", "b2"))
    assert np.array_equal(p["w1"], pw1.weight.detach().numpy()[:, :, 0].T)
    assert np.array_equal(p["w2"], pw2.weight.detach().numpy()[:, :, 0].T)
    # the fold against bn(dw(g)) in float64, on the GLU's output
    g = np.random.default_rng(1).uniform(-1, 1, (3, E, 21))
    with torch.no_grad():
        ref = bn.double()(dw.double()(torch.nn.functional.pad(torch.from_numpy(g), want if padding != "same"
                                                              else (0, 0)))).numpy()
    gp = np.pad(g, ((0, 0), (0, 0), want))
    got = sum(gp[:, :, j:j + 21] * p["wd"][j].astype(np.float64)[None, :, None] for j in range(k))
    got = got + p["bd"].astype(np.float64)[None, :, None]
    assert np.all(np.abs(got - ref) <= 1e-6 * (1 + np.abs(ref)))
    # rounded once: the float64 fold's nearest float32
    scale = (bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)).detach().numpy()
    w64 = dw.weight.detach().double().numpy()[:, 0, :] * scale[:, None]
    assert np.array_equal(p["wd"], w64.T.astype(np.float32))


def test_half_fold_is_bit_exact():
    rng = np.random.default_rng(4)
    h = rng.uniform(-1, 1, (50, 96)).astype(np.float32)
    W = (rng.uniform(-1, 1, (96, 40)) / np.sqrt(96)).astype(np.float32)
    assert np.array_equal(np.float32(0.5) * (h @ W), h @ (np.float32(0.5) * W))
    ff = cf.draw_module(cf.FeedForward(40, 96), 5).sequential
    w1, b1, w2, b2 = asr.ConformerLayer.pack_ffn(ff[0], ff[1], ff[4])
    assert np.array_equal(w1, ff[1].weight.detach().numpy().T) and np.array_equal(b1, ff[1].bias.detach().numpy())
    assert np.array_equal(w2 * np.float32(2), ff[4].weight.detach().numpy().T)
    assert np.array_equal(b2 * np.float32(2), ff[4].bias.detach().numpy())
    assert all(a.dtype == np.float32 for a in (w1, b1, w2, b2))


def test_conv_pack_refusals():
    P = asr.ConformerConv.pack_torch
    E, k = 12, 7
    ln, pw1, dw, bn, pw2 = conv_parts(E, k).parts()
    P(ln, pw1, dw, bn, pw2)
    for norm in ("group", "layer"):
        with pytest.raises(ValueError, match="in place of the BatchNorm1d"):
            P(*conv_parts(E, k, norm=norm).parts())
    with pytest.raises(ValueError, match="eval"):
        P(ln, pw1, dw, torch.nn.BatchNorm1d(E), pw2)                                   # training mode
    with pytest.raises(ValueError, match="running statistics"):
        P(ln, pw1, dw, torch.nn.BatchNorm1d(E, track_running_stats=False).eval(), pw2)
    with pytest.raises(ValueError, match="groups"):
        P(ln, pw1, torch.nn.Conv1d(E, E, k, padding=3, groups=E // 2), bn, pw2)
    with pytest.raises(ValueError, match="stride"):
        P(ln, pw1, torch.nn.Conv1d(E, E, k, padding=3, groups=E, stride=2), bn, pw2)
    with pytest.raises(ValueError, match="dilation"):
        P(ln, pw1, torch.nn.Conv1d(E, E, k, padding=6, groups=E, dilation=2), bn, pw2)
    with pytest.raises(ValueError, match="first pointwise"):
        P(ln, torch.nn.Conv1d(E, 2 * E, 3, padding=1), dw, bn, pw2)
    with pytest.raises(ValueError, match="second pointwise"):
        P(ln, pw1, dw, bn, torch.nn.Conv1d(E, E, 3, padding=1))
    with pytest.raises(ValueError, match="kernel - 1"):
        P(ln, pw1, torch.nn.Conv1d(E, E, k, padding=2, groups=E), bn, pw2)             # "same" needs 3
    with pytest.raises(ValueError, match="kernel - 1"):
        P(ln, pw1, torch.nn.Conv1d(E, E, k, groups=E), bn, pw2)                        # padding 0, none given
    with pytest.raises(ValueError, match="padding argument"):
        P(ln, pw1, dw, bn, pw2, padding="causal")                                      # dw pads itself already


@pytest.mark.parametrize("first", [False, True], ids=["attention-first", "convolution-first"])
def test_from_torchaudio_layout_packs_like_explicit_parts(first):
    shape = (10, 2, 32, 4, 64, 7)
    block = cf.make_block(shape, convolution_first=first)
    parts = asr.ConformerLayer.torchaudio_parts(block)
    explicit = block.explicit_parts()
    assert parts["convolution_first"] is first and explicit["convolution_first"] is first
    a = asr.ConformerLayer.pack_torch(**{k: v for k, v in parts.items() if k != "convolution_first"})
    b = asr.ConformerLayer.pack_torch(**{k: v for k, v in explicit.items() if k != "convolution_first"})
    assert set(a) == set(b) and len(a) >= 30
    for key in a:
        if isinstance(a[key], np.ndarray):
            assert a[key].dtype == np.float32 and np.array_equal(a[key], b[key]), key
        else:
            assert a[key] == b[key], key
    # the parts are the block's own modules, each where the description puts it
    assert parts["ffn1"][1] is block.ffn1.sequential[1] and parts["ffn2"][2] is block.ffn2.sequential[4]
    assert parts["conv"][2] is block.conv_module.sequential[2] and parts["conv"][2].groups == 32
    assert isinstance(parts["conv"][3], torch.nn.BatchNorm1d) and parts["attn"][1] is block.self_attn
    assert a["ffn1.w2"].shape == (64, 32) and a["conv.wd"].shape == (7, 32) and a["attn.w_in"].shape == (32, 96)
    assert np.array_equal(a["ffn2.w2"] * np.float32(2), block.ffn2.sequential[4].weight.detach().numpy().T)
