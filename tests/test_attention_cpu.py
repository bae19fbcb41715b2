"""CPU checks of the attention and LayerNorm layers (asr_attention_fwd,
asr_layernorm_fwd, asr_mask_rows, asr.MultiheadAttention, asr.LayerNorm,
asr.TransformerEncoderLayer): exported, every refusal ahead of any HIP call and
in the documented order (the fake device pointers are never dereferenced on the
host), the float64 reference of attention_reference.py against
torch.nn.functional.scaled_dot_product_attention / layer_norm in float64, and
the from_torch packers (layouts, refusals).  No GPU here."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import attention_reference as ar
from conftest import asr

NAMES = ["asr_attention_fwd", "asr_layernorm_fwd", "asr_mask_rows"]
FAKE = 0x10000   # a non-NULL, 16-byte aligned "device pointer"
INT_MAX = 2 ** 31 - 1
ARG, UNSUP = asr.ASR_ERR_ARG, asr.ASR_ERR_UNSUPPORTED


def desc(heads=4, head_dim=16, scale=0.0, chunk=1, left=-1, right=-1):
    return asr.AttnDesc(heads, head_dim, scale, chunk, left, right)


def att(d, Tq=8, Tk=8, B=2, q0=0, k0=0, ld=None, null=None, lds=None):
    """asr_attention_fwd with fake pointers; null: the pointer passed as NULL;
    lds: (ldq, ldk, ldv, ldo) when they differ."""
    p = {"q": FAKE, "k": FAKE, "v": FAKE, "out": FAKE}
    if null in p:
        p[null] = None
    E = d.heads * d.head_dim
    l4 = lds or (E if ld is None else ld,) * 4
    dp = None if null == "desc" else ctypes.byref(d)
    return asr.lib().asr_attention_fwd(dp, p["q"], l4[0], p["k"], l4[1], p["v"], l4[2], FAKE, p["out"], l4[3],
                                       Tq, q0, Tk, k0, B, None)


def ln(T=8, B=2, N=16, ldx=None, ldr=None, ldo=None, eps=1e-5, x=FAKE, res=FAKE, out=FAKE):
    return asr.lib().asr_layernorm_fwd(x, N if ldx is None else ldx, res, N if ldr is None else ldr, FAKE, FAKE, eps,
                                       FAKE, out, N if ldo is None else ldo, T, B, N, None)


def test_symbols_in_mirror_and_library():
    for n in NAMES:
        assert n in asr.EXPORTS, n
        assert hasattr(asr.lib(), n), n
    out = subprocess.run(["nm", "-D", "--defined-only", str(asr.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (asr_[a-z0-9_]+)$", out, flags=re.M))
    assert set(NAMES) <= exported


def test_desc_mirrors_the_header_struct():
    assert ctypes.sizeof(asr.AttnDesc) == 6 * 4
    assert [f[0] for f in asr.AttnDesc._fields_] == ["heads", "head_dim", "scale", "chunk", "left", "right"]
    d = asr.attn_desc(4, 36, chunk=16, left=2, right=0)
    assert (d.heads, d.head_dim, d.scale, d.chunk, d.left, d.right) == (4, 36, 0.0, 16, 2, 0)
    assert asr.ATTN_KEY_BLOCK == 64


# --------------------------------------------------------------- refusals
@pytest.mark.parametrize("null", ["desc", "q", "k", "v", "out"])
def test_attention_err_arg_null(null):
    assert att(desc(), null=null) == ARG


@pytest.mark.parametrize("kw", [dict(Tq=0), dict(Tq=-1), dict(Tk=0), dict(Tk=-5), dict(B=0), dict(B=-2),
                                dict(q0=-1), dict(k0=-1), dict(ld=63), dict(lds=(64, 63, 64, 64)),
                                dict(lds=(64, 64, 0, 64)), dict(lds=(64, 64, 64, -64))],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_attention_err_arg_sizes(kw):
    assert att(desc(), **kw) == ARG


@pytest.mark.parametrize("kw", [dict(heads=0), dict(heads=-4), dict(head_dim=0), dict(head_dim=-16), dict(chunk=0),
                                dict(chunk=-1), dict(left=-2), dict(right=-2), dict(scale=-1.0),
                                dict(scale=float("inf")), dict(scale=float("nan"))],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_attention_err_arg_descriptor(kw):
    assert att(desc(**kw), ld=64) == ARG


@pytest.mark.parametrize("d,kw", [
    (dict(head_dim=18), {}), (dict(head_dim=2), {}), (dict(head_dim=132), {}),
    (dict(heads=33, head_dim=128), {}),                       # heads*head_dim = 4224
    (dict(heads=65536, head_dim=4), dict(ld=2 ** 40)),        # also > 4096
    (dict(), dict(B=65536)),
    (dict(), dict(B=1, q0=INT_MAX - 70)), (dict(), dict(B=1, k0=INT_MAX)),
    (dict(), dict(Tq=INT_MAX, B=1)),
    (dict(), dict(Tq=1 << 20, B=1 << 12)), (dict(), dict(Tk=1 << 20, B=1 << 12)),
], ids=lambda v: ",".join(f"{k}={x}" for k, x in v.items()) or "base")
def test_attention_err_unsupported(d, kw):
    assert att(desc(**d), **kw) == UNSUP


def test_attention_arg_comes_before_unsupported():
    assert att(desc(head_dim=18, chunk=0)) == ARG
    assert att(desc(head_dim=256, scale=float("nan"))) == ARG
    assert att(desc(head_dim=18), Tq=0) == ARG
    assert att(desc(heads=65536, head_dim=4), ld=8) == ARG            # the stride, before the grid limit
    assert att(desc(), Tq=INT_MAX, Tk=INT_MAX, B=70000, q0=-1) == ARG
    assert att(desc(head_dim=18), null="out") == ARG


def test_layernorm_refusals_in_order():
    assert ln(x=None) == ARG
    assert ln(out=None) == ARG
    for kw in (dict(T=0), dict(B=-1), dict(N=0), dict(N=-16), dict(ldx=15), dict(ldr=15), dict(ldo=15),
               dict(eps=-1e-5), dict(eps=float("inf")), dict(eps=float("nan"))):
        assert ln(**kw) == ARG, kw
    assert ln(N=5000, ldx=4999) == ARG                       # both: ARG
    assert ln(T=INT_MAX, B=INT_MAX, eps=float("nan")) == ARG
    assert ln(N=4097) == UNSUP
    assert ln(N=INT_MAX) == UNSUP
    assert ln(T=1 << 20, B=1 << 12) == UNSUP
    assert ln(T=1 << 20, B=1 << 12, res=None, ldr=0) == UNSUP   # ldr is not read without a residual


def test_mask_rows_refusals():
    f = asr.lib().asr_mask_rows
    assert f(None, 16, FAKE, 8, 2, 16, None) == ARG
    assert f(FAKE, 16, FAKE, 0, 2, 16, None) == ARG
    assert f(FAKE, 16, FAKE, 8, 0, 16, None) == ARG
    assert f(FAKE, 16, FAKE, 8, 2, 0, None) == ARG
    assert f(FAKE, 15, FAKE, 8, 2, 16, None) == ARG
    assert f(FAKE, 16, FAKE, INT_MAX, INT_MAX, 16, None) == UNSUP
    assert f(FAKE, 16, None, 8, 2, 16, None) == asr.ASR_OK    # no lengths: nothing to do, no launch


# ----------------------------------------------- the reference against torch
def close64(got, ref):
    assert np.all(np.abs(got - ref) <= 1e-12 * (1 + np.abs(ref))), np.abs(got - ref).max()


@pytest.mark.parametrize("mask", list(ar.MASKS), ids=list(ar.MASKS))
@pytest.mark.parametrize("shape", ar.ATTN_SHAPES[:4], ids=lambda s: "x".join(map(str, s)))
def test_attention_reference_equals_torch(shape, mask):
    T, B, H, D = shape
    chunk, left, right = ar.MASKS[mask]
    q, k, v = ar.draw_attention(shape)
    lengths = ar.ragged_lengths(T, B)
    ref, seen = ar.attention_ref(q, k, v, H, chunk, left, right, lengths)
    heads = lambda a, b: torch.from_numpy(a[:, b].astype(np.float64).reshape(T, H, D)).permute(1, 0, 2)   # noqa: E731
    for b in range(B):
        n = lengths[b]
        assert np.array_equal(seen[:, b], np.arange(T) < n)        # every query inside the length sees itself
        assert not ref[n:, b].any()
        if n == 0:
            continue
        m = torch.from_numpy(ar.mask_matrix(T, T, n, chunk, left, right)[:n, :n])
        got = torch.nn.functional.scaled_dot_product_attention(heads(q, b)[:, :n], heads(k, b)[:, :n],
                                                               heads(v, b)[:, :n], attn_mask=m)
        close64(got.permute(1, 0, 2).reshape(n, H * D).numpy(), ref[:n, b])


def test_attention_reference_offsets_are_a_slice():
    """q_pos0 / k_pos0: rows of a call on a slice of the frames equal the whole call's rows."""
    shape = (70, 3, 2, 36)
    q, k, v = ar.draw_attention(shape)
    lengths = (70, 40, 55)
    whole, _ = ar.attention_ref(q, k, v, 2, 16, 2, 0, lengths)
    part, seen = ar.attention_ref(q[48:64], k[16:64], v[16:64], 2, 16, 2, 0, lengths, q_pos0=48, k_pos0=16)
    assert seen[:, 0].all() and not seen[:, 1].any()
    close64(part, whole[48:64])


@pytest.mark.parametrize("N", ar.LN_SIZES)
def test_layernorm_reference_equals_torch(N):
    x, res, gamma, beta = ar.draw_layernorm(N)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))   # noqa: E731
    close64(ar.layernorm_ref(x, res, gamma, beta, 1e-5),
            torch.nn.functional.layer_norm(t(x) + t(res), (N,), t(gamma), t(beta), 1e-5).numpy())
    close64(ar.layernorm_ref(x, None, None, None, 1e-3), torch.nn.functional.layer_norm(t(x), (N,), eps=1e-3).numpy())
    cut = ar.layernorm_ref(x, res, gamma, beta, lengths=(ar.LN_T, 0, 3, -2, 100))
    assert not cut[:, 1].any() and not cut[3:, 2].any() and not cut[:, 3].any() and cut[-1, 4].any()


# ---------------------------------------------------------------- from_torch
def test_pack_multihead_attention():
    torch.manual_seed(1)
    E, H = 24, 2
    mha = torch.nn.MultiheadAttention(E, H)
    with torch.no_grad():
        mha.in_proj_bias.uniform_(-0.1, 0.1)
        mha.out_proj.bias.uniform_(-0.1, 0.1)
    w_in, b_in, w_out, b_out = asr.MultiheadAttention.pack_torch(mha)
    assert (w_in.shape, b_in.shape, w_out.shape, b_out.shape) == ((E, 3 * E), (3 * E,), (E, E), (E,))
    assert all(a.dtype == np.float32 for a in (w_in, b_in, w_out, b_out))
    x = torch.randn(5, E)
    qkv = torch.nn.functional.linear(x, mha.in_proj_weight, mha.in_proj_bias).detach().numpy()
    assert np.allclose(x.numpy() @ w_in + b_in, qkv, atol=1e-5)
    assert np.allclose(x.numpy() @ w_out + b_out, mha.out_proj(x).detach().numpy(), atol=1e-5)
    nb = asr.MultiheadAttention.pack_torch(torch.nn.MultiheadAttention(E, H, bias=False))
    assert not nb[1].any() and not nb[3].any()


def test_multihead_attention_refusals():
    pack = asr.MultiheadAttention.pack_torch
    with pytest.raises(ValueError, match="kdim"):
        pack(torch.nn.MultiheadAttention(24, 2, kdim=16, vdim=24))
    with pytest.raises(ValueError, match="bias_k"):
        pack(torch.nn.MultiheadAttention(24, 2, add_bias_kv=True))
    with pytest.raises(ValueError, match="add_zero_attn"):
        pack(torch.nn.MultiheadAttention(24, 2, add_zero_attn=True))
    # E / heads outside the kernel's range: refused before any device call
    for E, H in ((36, 6), (18, 1), (1024, 4)):
        with pytest.raises(ValueError, match="head_dim"):
            asr.MultiheadAttention.from_torch(torch.nn.MultiheadAttention(E, H))
    with pytest.raises(ValueError, match="embed_dim"):
        asr.MultiheadAttention(4224, 33)                       # head_dim 128, E > 4096
    with pytest.raises(ValueError, match="window"):
        asr.MultiheadAttention(16, 2, chunk=0)


def test_layernorm_from_torch_refuses_two_dimensions():
    with pytest.raises(ValueError, match="normalized_shape"):
        asr.LayerNorm.from_torch(torch.nn.LayerNorm((4, 8)))


def test_pack_transformer_encoder_layer():
    torch.manual_seed(2)
    layer = torch.nn.TransformerEncoderLayer(16, 2, 40)
    w1, b1, w2, b2 = asr.TransformerEncoderLayer.pack_torch(layer)
    assert (w1.shape, b1.shape, w2.shape, b2.shape) == ((16, 40), (40,), (40, 16), (16,))
    x = torch.randn(3, 16)
    assert np.allclose(x.numpy() @ w1 + b1, layer.linear1(x).detach().numpy(), atol=1e-5)
    h = torch.randn(3, 40)
    assert np.allclose(h.numpy() @ w2 + b2, layer.linear2(h).detach().numpy(), atol=1e-5)


def test_transformer_encoder_layer_refusals():
    mk = torch.nn.TransformerEncoderLayer
    with pytest.raises(ValueError, match="gelu"):
        asr.TransformerEncoderLayer.from_torch(mk(16, 2, 32, activation="gelu"))
    with pytest.raises(ValueError, match="ReLU only"):
        asr.TransformerEncoderLayer.from_torch(mk(16, 2, 32, activation=torch.nn.SiLU()))
    with pytest.raises(ValueError, match="head_dim"):
        asr.TransformerEncoderLayer.from_torch(mk(36, 6, 32))


@pytest.mark.parametrize("N", [144, 512])
def test_offset_rows_defeat_a_one_pass_variance(N):
    """The x + 1000 case of test_attention_gpu.py in float32 on the CPU: a
    one-pass variance E[v^2] - E[v]^2 misses the project's fp32 bound by orders
    of magnitude, the two-pass form (mean refined by the mean of the centred
    values, as the kernel does) stays inside it."""
    x, _, gamma, beta = ar.draw_layernorm(N)
    x = (x + 1000).astype(np.float32)
    ref = ar.layernorm_ref(x, None, gamma, beta)
    f = np.float32
    mean = x.sum(-1, keepdims=True, dtype=f) / f(N)
    one = (x * x).sum(-1, keepdims=True, dtype=f) / f(N) - mean * mean
    with np.errstate(invalid="ignore", divide="ignore"):
        y1 = (x - mean) / np.sqrt(one + f(1e-5)) * gamma + beta
    d = x - mean
    d = d - d.sum(-1, keepdims=True, dtype=f) / f(N)
    var = (d * d).sum(-1, keepdims=True, dtype=f) / f(N)
    y2 = d * (f(1) / np.sqrt(var + f(1e-5))) * gamma + beta
    bound = 2e-5 * (1 + np.abs(ref))
    assert not np.all(np.abs(np.nan_to_num(y1.astype(np.float64), nan=1e9) - ref) <= 100 * bound)
    assert np.all(np.abs(y2.astype(np.float64) - ref) <= bound)
