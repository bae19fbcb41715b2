"""GPU numerics of the attention and LayerNorm layers (asr_attention_fwd,
asr_layernorm_fwd, asr_mask_rows, asr.MultiheadAttention, asr.LayerNorm,
asr.TransformerEncoderLayer).

Reference: attention_reference.py (float64, itself checked against torch in
test_attention_cpu.py).  Bound: the project's bound for fp32 kernels
(test_gru_gpu.py close()): |err| <= 2e-5 * (1 + |ref|); the large-logit case
allows max(2e-5, 4 x the error of torch float32 on the CPU) * (1 + |ref|), the
factor covering a different summation order of the same fp32 arithmetic.
Inputs: Q, K, V and x U(+-1), gamma U(0.5, 1.5), beta U(+-0.1), res U(+-1).
Each case prints its max error.

The kernel's tiles are the ones the shapes of attention_reference.ATTN_SHAPES
were chosen for: 64 query rows per workgroup (16 per wave), 64-key blocks
aligned on absolute positions, 16-column MFMA tiles of a head (one kernel
instantiation per ceil(head_dim / 16): 4, 16, 20, 36, 64, 128 cover 1, 2, 3, 4
and 8), 4-wide contraction steps.  Bit-independence cases compare with
np.array_equal.
"""
import functools

import numpy as np
import pytest
import torch

import attention_reference as ar
from conftest import asr

pytestmark = pytest.mark.gpu
ATOL = 2e-5
SENT = -12345.0
ids = lambda sh: "x".join(map(str, sh))   # noqa: E731
MASK_IDS = list(ar.MASKS)


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


def put(a2d, ld=None, fill=np.nan, misalign=False):
    """a2d [rows][n] on the device with row stride ld (extra columns hold fill);
    misalign: the buffer starts 4 bytes past a 16-byte boundary."""
    rows, n = a2d.shape
    ld = ld or n
    h = np.full((rows, ld), fill, np.float32)
    h[:, :n] = a2d
    if not misalign:
        d = dm(h)
        assert d.ptr % 16 == 0
        return d
    base = dm(np.concatenate([np.zeros(1, np.float32), h.reshape(-1), np.zeros(3, np.float32)]).reshape(-1, 1))
    v = View(base.ptr + 4, rows, ld, base)
    assert v.ptr % 16 == 4
    return v


def fetch(view, rows, ld):
    """The rows x ld floats at view.ptr."""
    out = np.empty((rows, ld), np.float32)
    asr.check(asr.lib().asr_memcpy_d2h(out.ctypes.data, view.ptr, out.nbytes, None), "asr_memcpy_d2h")
    return out


def run(q, k, v, heads, mask=(1, -1, -1), lengths=None, q_pos0=0, k_pos0=0, ld=None, ldo=None, misalign=False,
        fused=False, scale=0.0):
    """asr_attention_fwd on q [Tq][B][E], k, v [Tk][B][E]; returns out [Tq][B][ldo].
    ld: row stride of q, k and v (extra columns NaN); ldo: of out (extra columns a
    sentinel); misalign: all four buffers 4 bytes past a 16-byte boundary; fused:
    q, k, v as the three column ranges of one [T*B, 3E] buffer."""
    Tq, B, E = q.shape
    Tk = k.shape[0]
    desc = asr.attn_desc(heads, E // heads, scale, *mask)
    if fused:
        assert Tq == Tk and ld is None
        buf = put(np.concatenate([q, k, v], axis=2).reshape(Tq * B, 3 * E), misalign=misalign)
        dq, dk, dv = (View(buf.ptr + 4 * E * i, Tq * B, 3 * E, buf) for i in range(3))
    else:
        dq, dk, dv = (put(a.reshape(-1, E), ld, misalign=misalign) for a in (q, k, v))
    ldo = ldo or E
    out = put(np.full((Tq * B, ldo), SENT, np.float32), misalign=misalign)
    ln = None if lengths is None else asr.device_lengths(lengths)
    asr.attention_fwd(dq, dk, dv, out, Tq, Tk, B, desc, lengths=ln, q_pos0=q_pos0, k_pos0=k_pos0, ldo=ldo)
    asr.synchronize()
    return fetch(out, Tq * B, ldo).reshape(Tq, B, ldo)


def nan_past_lengths(x, lengths, pos0=0):
    x = x.copy()
    for b, n in enumerate(lengths):
        x[max(n - pos0, 0):, b] = np.nan
    return x


@functools.lru_cache(maxsize=None)
def inputs(shape):
    qkv = ar.draw_attention(shape)
    for a in qkv:
        a.setflags(write=False)
    return qkv


@functools.lru_cache(maxsize=None)
def reference(shape, mask, lengths=None):
    q, k, v = inputs(shape)
    out, seen = ar.attention_ref(q, k, v, shape[2], *ar.MASKS[mask], lengths=lengths)
    out.setflags(write=False)
    return out, seen


# ------------------------------------------------------------------ values
@pytest.mark.parametrize("mask", MASK_IDS)
@pytest.mark.parametrize("shape", ar.ATTN_SHAPES, ids=ids)
def test_attention_values(shape, mask):
    q, k, v = inputs(shape)
    ref, seen = reference(shape, mask)
    assert seen.all()                         # the reference itself: every compared row sees a key
    got = run(q, k, v, shape[2], ar.MASKS[mask])
    close(got, ref, f"attention {ids(shape)} {mask}")


def test_attention_explicit_scale():
    shape = ar.ATTN_SHAPES[2]
    q, k, v = inputs(shape)
    ref, _ = ar.attention_ref(q, k, v, shape[2], scale=0.37)
    close(run(q, k, v, shape[2], scale=0.37), ref, "scale 0.37")


def test_attention_large_logits():
    """Q scaled by 40: raw scores q.k reach about +-500 (scaled: +-65) and the
    running-maximum rescale really runs.  Bound: max(2e-5, 4 x torch float32 on the CPU) * (1 + |ref|)."""
    shape = (130, 2, 2, 64)
    T, B, H, D = shape
    q, k, v = inputs(shape)
    q = (q * 40).astype(np.float32)
    ref, seen = ar.attention_ref(q, k, v, H)
    assert seen.all()
    scores = np.einsum("tbhd,sbhd->bhts", q.reshape(T, B, H, D).astype(np.float64), k.reshape(T, B, H, D)) / 8
    assert np.abs(scores).max() > 50
    heads = lambda a: torch.from_numpy(np.array(a).reshape(T, B, H, D)).permute(1, 2, 0, 3)   # noqa: E731
    t32 = torch.nn.functional.scaled_dot_product_attention(heads(q), heads(k), heads(v))
    t32 = t32.permute(2, 0, 1, 3).reshape(T, B, H * D).numpy().astype(np.float64)
    e32 = (np.abs(t32 - ref) / (1 + np.abs(ref))).max()
    bound = max(ATOL, 4 * e32)
    print(f"large logits: max |score| {np.abs(scores).max():.1f}, torch float32 (CPU) err / (1 + |ref|) {e32:.3e}, "
          f"bound {bound:.3e}")
    close(run(q, k, v, H), ref, "large logits", atol=bound)


# ----------------------------------------------------------------- lengths
@pytest.mark.parametrize("mask", ["full", "chunked"])
@pytest.mark.parametrize("shape", [ar.ATTN_SHAPES[2], ar.ATTN_SHAPES[3], ar.ATTN_SHAPES[5]], ids=ids)
def test_attention_lengths(shape, mask):
    """Ragged lengths with NaN in every Q/K/V row past its length: finite, within
    the bound, exact zeros past the length."""
    T, B, H, D = shape
    ln = ar.ragged_lengths(T, B)
    q, k, v = inputs(shape)
    ref, seen = reference(shape, mask, ln)
    for b, n in enumerate(ln):
        assert np.array_equal(seen[:, b], np.arange(T) < n)
    got = run(*(nan_past_lengths(a, ln) for a in (q, k, v)), H, ar.MASKS[mask], lengths=ln)
    for b, n in enumerate(ln):
        assert not got[n:, b].any(), b
    close(got, ref, f"attention lengths {ids(shape)} {mask}")


def test_attention_lengths_clamp_and_null():
    """A negative length is 0; a length past T only bounds nothing."""
    shape = ar.ATTN_SHAPES[2]
    T, B, H, D = shape
    q, k, v = inputs(shape)
    got = run(q, k, v, H, lengths=(-3, T + 100, 7))
    ref, _ = ar.attention_ref(q, k, v, H, lengths=(0, T, 7))
    assert not got[:, 0].any()
    close(got, ref, "clamped lengths")


def test_query_that_sees_no_key_is_zero():
    """Keys start after the query's window: the rows are exact zeros, not NaN."""
    shape = ar.ATTN_SHAPES[2]
    q, k, v = inputs(shape)
    got = run(q[:16], k[:16], v[:16], shape[2], (16, 0, 0), q_pos0=0, k_pos0=16)
    assert not got.any()


# ------------------------------------------------------- bit-independence
BIT_SHAPES = [ar.ATTN_SHAPES[2], ar.ATTN_SHAPES[5]]


@pytest.mark.parametrize("mask", ["full", "chunked"])
@pytest.mark.parametrize("shape", BIT_SHAPES, ids=ids)
def test_bits_do_not_depend_on_the_batch(shape, mask):
    """One utterance alone (B = 1) == the same utterance at two positions of a ragged batch."""
    T, B, H, D = shape
    q, k, v = inputs(shape)
    ln = list(ar.ragged_lengths(T, B))
    u, p1, p2, n = 2, 1, B - 1, T - 3
    batch = []
    for a in (q, k, v):
        a = a.copy()
        a[:, p1], a[:, p2] = a[:, u], a[:, u]
        batch.append(a)
    ln[p1] = ln[p2] = n
    got = run(*(nan_past_lengths(a, ln) for a in batch), H, ar.MASKS[mask], lengths=tuple(ln))
    alone = run(*(nan_past_lengths(a[:, u:u + 1], [n]) for a in (q, k, v)), H, ar.MASKS[mask], lengths=(n,))
    assert alone[:n].any()
    assert np.array_equal(got[:, p1], alone[:, 0])
    assert np.array_equal(got[:, p2], alone[:, 0])


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=ids)
def test_bits_do_not_depend_on_strides(shape):
    """ld = E + 1 for Q, K, V and E + 3 for out against contiguous buffers; the
    untouched output columns keep their sentinel."""
    T, B, H, D = shape
    E = H * D
    q, k, v = inputs(shape)
    ln = ar.ragged_lengths(T, B)
    a = run(q, k, v, H, ar.MASKS["window"], lengths=ln)
    s = run(q, k, v, H, ar.MASKS["window"], lengths=ln, ld=E + 1, ldo=E + 3)
    assert np.all(s[:, :, E:] == SENT)
    assert np.array_equal(s[:, :, :E], a)


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=ids)
def test_bits_do_not_depend_on_alignment(shape):
    """Pointers 4 bytes past a 16-byte boundary against aligned ones."""
    q, k, v = inputs(shape)
    a = run(q, k, v, shape[2], ar.MASKS["causal"])
    m = run(q, k, v, shape[2], ar.MASKS["causal"], misalign=True)
    assert np.array_equal(a, m)


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=ids)
def test_bits_do_not_depend_on_fused_qkv(shape):
    """Q, K, V as three buffers against three column ranges of one [T*B, 3E] buffer."""
    q, k, v = inputs(shape)
    ln = ar.ragged_lengths(shape[0], shape[1])
    a = run(q, k, v, shape[2], lengths=ln)
    f = run(q, k, v, shape[2], lengths=ln, fused=True)
    assert np.array_equal(a, f)


# ---------------------------------------------------------------- streaming
@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
def test_streaming_chunks_give_the_whole_calls_bits(ragged):
    """Mask (chunk 16, left 2, right 0): one call over T = 150 == calls chunk by
    chunk (Tq = 16 but for the last, q_pos0 = 16 c) on a K/V buffer that holds
    only frames [max(0, 16 (c - 2)), 16 (c + 1)), bit for bit."""
    shape = (150, 3, 2, 36)
    T, B, H, D = shape
    mask = ar.MASKS["chunked"]
    q, k, v = inputs(shape)
    ln = (T, 0, 65) if ragged else None
    if ragged:
        q, k, v = (nan_past_lengths(a, ln) for a in (q, k, v))
    whole = run(q, k, v, H, mask, lengths=ln)
    parts = []
    for c in range((T + 15) // 16):
        q0, q1 = 16 * c, min(16 * (c + 1), T)
        k0 = max(0, 16 * (c - 2))
        parts.append(run(q[q0:q1], k[k0:q1], v[k0:q1], H, mask, lengths=ln, q_pos0=q0, k_pos0=k0))
    assert np.array_equal(np.concatenate(parts), whole)
    ref, _ = ar.attention_ref(q, k, v, H, *mask, lengths=ln)
    close(whole, ref, "streaming whole")


# ---------------------------------------------------------------- LayerNorm
def run_ln(x, res=None, gamma=None, beta=None, eps=1e-5, lengths=None, inplace=None, ldo=None):
    """asr_layernorm_fwd on x [T][B][N]; inplace: None, 'x' or 'res' (out is that buffer)."""
    T, B, N = x.shape
    dx = dm(x.reshape(T * B, N))
    dr = None if res is None else dm(res.reshape(T * B, N))
    ldo = ldo or N
    out = {None: None, "x": dx, "res": dr}[inplace] or dm(np.full((T * B, ldo), SENT, np.float32))
    up = lambda a: None if a is None else dm(a.reshape(-1, 1))   # noqa: E731
    ln = None if lengths is None else asr.device_lengths(lengths)
    asr.layernorm_fwd(dx, out, T, B, N, up(gamma), up(beta), eps, dr, ln)
    asr.synchronize()
    return out.toCpu().reshape(T, B, -1)


@pytest.mark.parametrize("variant", ["all", "plain", "res", "affine"])
@pytest.mark.parametrize("N", ar.LN_SIZES)
def test_layernorm_values(N, variant):
    x, res, gamma, beta = ar.draw_layernorm(N)
    if variant in ("plain", "affine"):
        res = None
    if variant in ("plain", "res"):
        gamma = beta = None
    close(run_ln(x, res, gamma, beta), ar.layernorm_ref(x, res, gamma, beta), f"layernorm N={N} {variant}")


@pytest.mark.parametrize("N", [65, 512])
def test_layernorm_lengths_and_strides(N):
    """Rows past the lengths are exact zeros with NaN in the padding; lengths clamp
    to [0, T]; columns >= N of out keep their sentinel."""
    x, res, gamma, beta = ar.draw_layernorm(N)
    ln = (ar.LN_T, 0, 3, -2, ar.LN_T + 9)
    got = run_ln(nan_past_lengths(x, ln), nan_past_lengths(res, ln), gamma, beta, lengths=ln, ldo=N + 3)
    assert np.all(got[:, :, N:] == SENT)
    got = got[:, :, :N]
    for b, n in enumerate(ln):
        assert not got[max(n, 0):, b].any(), b
    close(got, ar.layernorm_ref(x, res, gamma, beta, lengths=ln), f"layernorm lengths N={N}")


@pytest.mark.parametrize("N", [63, 144, 4096])
def test_layernorm_in_place_and_row_alone(N):
    x, res, gamma, beta = ar.draw_layernorm(N)
    ln = (ar.LN_T, 2, 5, 0, 7)
    a = run_ln(x, res, gamma, beta, lengths=ln)
    assert np.array_equal(run_ln(x, res, gamma, beta, lengths=ln, inplace="x"), a)
    assert np.array_equal(run_ln(x, res, gamma, beta, lengths=ln, inplace="res"), a)
    t, b = 3, 2                                # one row alone: T = B = 1
    alone = run_ln(x[t:t + 1, b:b + 1], res[t:t + 1, b:b + 1], gamma, beta)
    assert np.array_equal(alone[0, 0], a[t, b])


@pytest.mark.parametrize("N", [144, 512])
def test_layernorm_offset_rows(N):
    """x + 1000 (no residual: the fp32 sum x + res would round at that size): a
    one-pass variance fails here (test_attention_cpu.py shows it on the CPU), the
    two-pass form with the refined mean stays within the bound."""
    x, _, gamma, beta = ar.draw_layernorm(N)
    x = (x + 1000).astype(np.float32)
    close(run_ln(x, None, gamma, beta), ar.layernorm_ref(x, None, gamma, beta), f"layernorm offset N={N}")


def test_mask_rows():
    T, B, N = 6, 4, 70
    x = np.random.default_rng(5).uniform(-1, 1, (T, B, N)).astype(np.float32)
    ln = (T, 0, 2, -1)
    d = put(nan_past_lengths(x, ln).reshape(T * B, N), ld=N + 2, fill=SENT)
    asr.mask_rows(d, T, B, N, asr.device_lengths(ln))
    asr.synchronize()
    got = d.toCpu().reshape(T, B, N + 2)
    assert np.all(got[:, :, N:] == SENT)
    for b, n in enumerate(ln):
        n = max(n, 0)
        assert np.array_equal(got[:n, b, :N], x[:n, b]) and not got[n:, b, :N].any()


# --------------------------------------------------------------- from_torch
def torch_masks(T, ln, chunk, left, right):
    """(attn_mask [T][T], key_padding_mask [B][T]) as torch takes them: True = not allowed."""
    allowed = ar.mask_matrix(T, T, T, chunk, left, right)
    kpm = np.arange(T)[None, :] >= np.asarray(ln)[:, None]
    return torch.from_numpy(~allowed), torch.from_numpy(kpm)


def check_valid_rows(got, ref, ln, what):
    """Valid rows under the bound, padding rows exact zeros."""
    B = got.shape[1]
    mask = np.arange(got.shape[0])[:, None] < np.asarray(ln)[None, :]
    assert not got[~mask].any()
    close(got[mask], ref[mask], what)
    assert mask.sum() >= B


@pytest.mark.parametrize("window", [(1, -1, -1), (16, 2, 0)], ids=["full", "chunked"])
def test_from_torch_multihead_attention(window):
    torch.manual_seed(21)
    T, B, E, H = 70, 5, 144, 4
    mha = torch.nn.MultiheadAttention(E, H)
    with torch.no_grad():
        mha.in_proj_bias.uniform_(-0.1, 0.1)
        mha.out_proj.bias.uniform_(-0.1, 0.1)
    layer = asr.MultiheadAttention.from_torch(mha, *window)
    x = np.random.default_rng(6).uniform(-1, 1, (T, B, E)).astype(np.float32)
    ln = ar.ragged_lengths(T, B)
    out = layer.forward(dm(nan_past_lengths(x, ln).reshape(T * B, E)), T, B, lengths=ln)
    asr.synchronize()
    am, kpm = torch_masks(T, ln, *window)
    with torch.no_grad():
        ref, _ = mha.double()(*(torch.from_numpy(x.astype(np.float64)),) * 3, key_padding_mask=kpm, attn_mask=am,
                              need_weights=False)
    check_valid_rows(out.toCpu().reshape(T, B, E), ref.numpy(), ln, f"MultiheadAttention {window}")


@pytest.mark.parametrize("norm_first", [False, True], ids=["post", "pre"])
def test_from_torch_transformer_encoder_layer(norm_first):
    torch.manual_seed(22)
    T, B, E, H, F = 70, 5, 64, 4, 128
    enc = torch.nn.TransformerEncoderLayer(E, H, F, dropout=0.0, norm_first=norm_first)   # train mode: no fused path
    with torch.no_grad():
        for nm in (enc.norm1, enc.norm2):
            nm.weight.uniform_(0.5, 1.5)
            nm.bias.uniform_(-0.1, 0.1)
    layer = asr.TransformerEncoderLayer.from_torch(enc)
    x = np.random.default_rng(7).uniform(-1, 1, (T, B, E)).astype(np.float32)
    ln = ar.ragged_lengths(T, B)
    out = layer.forward(dm(nan_past_lengths(x, ln).reshape(T * B, E)), T, B, lengths=ln)
    asr.synchronize()
    am, kpm = torch_masks(T, ln, 1, -1, -1)
    with torch.no_grad():
        ref = enc.double()(torch.from_numpy(x.astype(np.float64)), src_mask=am, src_key_padding_mask=kpm)
    check_valid_rows(out.toCpu().reshape(T, B, E), ref.numpy(), ln, f"TransformerEncoderLayer norm_first={norm_first}")


def test_conv_then_encoder_layer_then_logsoftmax():
    """Conv1d(stride 2) -> TransformerEncoderLayer -> Linear + log-softmax, the
    conv's out_lengths passed on as a device array; against the torch chain in
    float64 on each utterance's own frames."""
    torch.manual_seed(23)
    T, B, ci, E, H, F, V = 41, 6, 26, 32, 2, 64, 29
    conv = torch.nn.Conv1d(ci, E, 5, stride=2, padding=2)
    enc = torch.nn.TransformerEncoderLayer(E, H, F, dropout=0.0)
    lin = torch.nn.Linear(E, V)
    c1, l2 = asr.Conv1d.from_torch(conv, act="relu"), asr.TransformerEncoderLayer.from_torch(enc)
    x = np.random.default_rng(8).uniform(-1, 1, (T, B, ci)).astype(np.float32)
    ln = (T, 3, 12, 1, 20, 8)
    h, T1, ln1 = c1.forward(dm(nan_past_lengths(x, ln).reshape(T * B, ci)), T, B, lengths=ln)
    y = l2.forward(h, T1, B, lengths=ln1)
    l3 = asr.Linear(T1 * B, E, V, lin.weight.detach().numpy().T.copy(), lin.bias.detach().numpy(),
                    asr.EPI_BIAS_LOGSOFTMAX)
    got = l3.forward(y).toCpu().reshape(T1, B, V)
    asr.synchronize()
    oln = [c1.out_frames(n) for n in ln]
    assert [int(v) for v in asr.device_int32(ln1, B)] == oln and min(oln) >= 1
    cd, ed, ld = conv.double(), enc.double(), lin.double()
    with torch.no_grad():
        for b, n in enumerate(ln):
            f = torch.relu(cd(torch.from_numpy(x[:n, b].astype(np.float64).T.copy())[None]))[0].T   # [n1][E]
            assert f.shape[0] == oln[b]
            ref = torch.log_softmax(ld(ed(f[:, None, :])[:, 0]), dim=1).numpy()
            close(got[:oln[b], b], ref, f"chain utterance {b}")
