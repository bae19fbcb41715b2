"""CPU checks of the E-Branchformer additions (ASR_EPI_BIAS_GELU, asr_csgu_fwd,
asr_merge_dwconv_fwd, asr.ConvolutionalGatingMLP / EBranchformerLayer): the
float64 restatements of ebranchformer_reference.py against torch, every refusal
ahead of any HIP call in the documented order (the fake device pointers are
never dereferenced on the host), and the packing.  No GPU here."""
import ctypes

import numpy as np
import pytest
import torch

import ebranchformer_reference as eb
from conftest import asr

FAKE, FAKE2, FAKE3 = 0x10000, 0x20000, 0x30000   # non-NULL "device pointers"
INT_MAX = 2 ** 31 - 1
F = torch.nn.functional
BIG_K = asr.CGMLP_MAX_KERNEL + 1


def csgu(null=None, T=8, B=4, ldu=None, ldo=None, out=FAKE2, **kw):
    d = asr.CsguDesc(**{**dict(channels=16, kernel=3, pad_left=1, pad_right=1, eps=1e-5), **kw})
    p = dict(u=FAKE, lengths=FAKE, gamma=FAKE, beta=FAKE, w=FAKE, b=FAKE, stats=FAKE3, out=out)
    p[null] = None
    return asr.lib().asr_csgu_fwd(None if null == "desc" else ctypes.byref(d), p["u"],
                                  2 * d.channels if ldu is None else ldu, p["lengths"], p["gamma"], p["beta"], p["w"],
                                  p["b"], p["stats"], p["out"], d.channels if ldo is None else ldo, T, B, None)


def merge(null=None, T=8, B=4, ldx1=None, ldx2=None, ldo=None, out=FAKE3, **kw):
    d = asr.MergeDwconvDesc(**{**dict(channels=16, kernel=3, pad_left=1, pad_right=1), **kw})
    p = dict(x1=FAKE, x2=FAKE2, lengths=FAKE, w=FAKE, b=FAKE, out=out)
    p[null] = None
    ld = lambda v, dflt: dflt if v is None else v   # noqa: E731
    return asr.lib().asr_merge_dwconv_fwd(None if null == "desc" else ctypes.byref(d), p["x1"], ld(ldx1, d.channels),
                                          p["x2"], ld(ldx2, d.channels), p["lengths"], p["w"], p["b"], p["out"],
                                          ld(ldo, 2 * d.channels), T, B, None)


# ---------------------------------------------------- references vs. torch
def close(a, ref):
    return np.all(np.abs(a - ref) <= 1e-13 * (1 + np.abs(ref)))


def test_gelu_reference_matches_torch():
    v = np.concatenate([np.linspace(-9, 9, 2001), [-100.0, 0.0, 100.0]])
    assert close(eb.gelu_ref(v), F.gelu(torch.from_numpy(v)).numpy())
    assert eb.gelu_ref(-100.0) == 0 and eb.gelu_ref(100.0) == 100


@pytest.mark.parametrize("T,B,C,k,pl", [(9, 3, 19, 3, 1), (70, 2, 8, 31, 15), (12, 2, 6, 5, 4)])
def test_conv_references_match_torch(T, B, C, k, pl):
    pr = k - 1 - pl
    u, w, b = eb.draw_conv(T, B, 2 * C, k, C)
    _, w2, b2 = eb.draw_conv(T, B, 1, k, 2 * C, seed=1)
    rng = np.random.default_rng(C)
    gamma, beta = rng.uniform(0.5, 1.5, C).astype(np.float32), rng.uniform(-.1, .1, C).astype(np.float32)
    ln = (T + 2, 1, T // 2)[:B]
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))   # noqa: E731
    dw = lambda x, w, b: F.conv1d(F.pad(x.T[None], (pl, pr)), t64(w).T[:, None, :].contiguous(), t64(b),   # noqa: E731
                                  groups=w.shape[1])[0].T.numpy()
    got_c = eb.csgu_ref(u, w, b, pl, gamma, beta, 1e-5, ln)
    got_m = eb.merge_ref(u[..., :C], u[..., C:], w2, b2, pl, ln)
    for bi, n in enumerate(ln):
        n = min(n, T)
        x = t64(u[:n, bi])
        ref_c = x[:, :C].numpy() * dw(F.layer_norm(x[:, C:], (C,), t64(gamma), t64(beta), 1e-5), w, b)
        ref_m = x.numpy() + dw(x, w2, b2)
        assert close(got_c[:n, bi], ref_c) and close(got_m[:n, bi], ref_m)
        assert not got_c[n:, bi].any() and not got_m[n:, bi].any()


# --------------------------------------------------------------- refusals
ARG, UNS = asr.ASR_ERR_ARG, asr.ASR_ERR_UNSUPPORTED
COMMON_ARG = [dict(T=0), dict(B=-1), dict(channels=0), dict(kernel=0), dict(pad_left=-1, pad_right=3),
              dict(pad_right=-1, pad_left=3), dict(ldo=15)]
COMMON_UNS = [dict(pad_left=2), dict(pad_left=INT_MAX, pad_right=INT_MAX),
              dict(kernel=BIG_K, pad_left=BIG_K - 1, pad_right=0, T=200), dict(channels=4097, ldo=2 * 4097),
              dict(T=1 << 20, B=1 << 12), dict(T=INT_MAX - 100, B=1)]
ids = lambda kw: ",".join(f"{k}={v}" for k, v in kw.items())   # noqa: E731


@pytest.mark.parametrize("kw", [dict(null=n) for n in ("desc", "u", "w", "stats", "out")] + COMMON_ARG + [
    dict(ldu=31), dict(eps=float("nan")), dict(eps=float("inf")), dict(eps=-1e-5), dict(out=FAKE),
    dict(channels=INT_MAX, ldu=INT_MAX, ldo=INT_MAX),                        # 2C does not wrap
    # each earlier check wins over a later one
    dict(null="stats", kernel=BIG_K), dict(ldu=7, pad_left=5), dict(eps=-1.0, out=FAKE, pad_left=5),
    dict(out=FAKE, kernel=BIG_K, pad_left=BIG_K - 1, pad_right=0)], ids=ids)
def test_csgu_err_arg(kw):
    assert csgu(**kw) == ARG


@pytest.mark.parametrize("kw", COMMON_UNS + [dict(channels=4097, ldu=2 * 4097, ldo=4097),
                                             dict(null="lengths", pad_left=2), dict(null="gamma", pad_left=2),
                                             dict(null="beta", pad_left=2), dict(null="b", pad_left=2),
                                             dict(channels=4096, kernel=1, pad_left=0, pad_right=0, ldu=8192,
                                                  ldo=4096, T=65, B=1 << 24)], ids=ids)   # 2^24 * 2 * 64 workgroups
def test_csgu_err_unsupported(kw):
    if kw.get("channels") == 4097 and "ldu" not in kw:
        kw = dict(kw, ldu=2 * 4097)
    assert csgu(**kw) == UNS


@pytest.mark.parametrize("kw", [dict(null=n) for n in ("desc", "x1", "x2", "w", "out")] + COMMON_ARG + [
    dict(ldx1=15), dict(ldx2=15), dict(ldo=31), dict(out=FAKE), dict(out=FAKE2),
    dict(out=FAKE2, pad_left=5), dict(ldx2=3, kernel=BIG_K)], ids=ids)
def test_merge_err_arg(kw):
    assert merge(**kw) == ARG


@pytest.mark.parametrize("kw", COMMON_UNS + [dict(null="lengths", pad_left=2), dict(null="b", pad_left=2)], ids=ids)
def test_merge_err_unsupported(kw):
    if kw.get("channels") == 4097:
        kw = dict(kw, ldx1=4097, ldx2=4097)
    assert merge(**kw) == UNS


def test_linear_gelu_needs_a_bias():
    L = asr.lib()
    assert asr.EPI_BIAS_GELU == 6
    assert L.asr_linear_fwd(FAKE, FAKE, None, FAKE2, 8, 8, 8, asr.EPI_BIAS_GELU, None) == ARG
    assert L.asr_linear_fwd(FAKE, FAKE, FAKE, FAKE2, 0, 8, 8, asr.EPI_BIAS_GELU, None) == ARG


# ------------------------------------------------------------- pack_torch
def test_cgmlp_pack_and_refusals():
    E, units, k = 12, 40, 7
    P = asr.ConvolutionalGatingMLP.pack_torch
    m = eb.draw_module(eb.CgMLP(E, units, k), 3)
    p = P(m)
    assert p["w1"].shape == (E, units) and p["wd"].shape == (k, units // 2) and p["w2"].shape == (units // 2, E)
    assert p["padding"] == (3, 3) and p["norm_eps"] == m.csgu.norm.eps
    assert np.array_equal(p["wd"], m.csgu.conv.weight.detach().numpy()[:, 0, :].T)
    assert np.array_equal(p["w1"], m.channel_proj1[0].weight.detach().numpy().T)
    with pytest.raises(ValueError, match="use_linear_after_conv"):
        P(eb.CgMLP(E, units, k, use_linear=True))
    with pytest.raises(ValueError, match="gate activation"):
        P(eb.CgMLP(E, units, k, act=torch.nn.ReLU()))
    for conv, what in ((torch.nn.Conv1d(20, 20, k, padding=3, groups=10), "depthwise"),
                       (torch.nn.Conv1d(20, 20, k, stride=2, padding=3, groups=20), "stride"),
                       (torch.nn.Conv1d(20, 20, k, padding=2, groups=20), "kernel - 1")):
        bad = eb.CgMLP(E, units, k)
        bad.csgu.conv = conv
        with pytest.raises(ValueError, match=what):
            P(bad)
    bad = eb.CgMLP(E, units, k)
    bad.channel_proj1[1] = torch.nn.GELU(approximate="tanh")
    with pytest.raises(ValueError, match="exact GELU"):
        P(bad)


@pytest.mark.parametrize("macaron", [True, False], ids=["macaron", "plain"])
def test_espnet_layout_packs_and_half_fold_is_bit_exact(macaron):
    blk = eb.make_block((10, 2, 32, 4, 64, 7, 5), rel=macaron, macaron=macaron)
    parts = asr.EBranchformerLayer.espnet_parts(blk)
    assert parts["ff_scale"] == (0.5 if macaron else 1.0) and (parts["ffn1"] is None) == (not macaron)
    p = asr.EBranchformerLayer.pack_torch(**parts)
    assert ("attn.w_pos" in p) == macaron and ("ffn1.w1" in p) == macaron
    w2 = blk.feed_forward.w_2.weight.detach().numpy().T
    assert p["ffn2.w2"].dtype == np.float32 and np.array_equal(p["ffn2.w2"] * np.float32(1 / parts["ff_scale"]), w2)
    h = np.random.default_rng(4).uniform(-1, 1, (50, 64)).astype(np.float32)
    assert np.array_equal(np.float32(0.5) * (h @ w2), h @ (np.float32(0.5) * w2))
    assert p["merge.wd"].shape == (5, 64) and p["merge.w"].shape == (64, 32) and p["merge.padding"] == (2, 2)
    assert p["cgmlp.wd"].shape == (7, 32) and p["mlp.norm_eps"] == blk.norm_mlp.eps
    blk.feed_forward.activation = torch.nn.ReLU()
    with pytest.raises(ValueError, match="Swish"):
        asr.EBranchformerLayer.espnet_parts(blk)
