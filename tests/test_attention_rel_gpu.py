"""GPU numerics of relative-position self-attention (asr_attention_rel_fwd,
asr.RelPositionMultiheadAttention, a ConformerLayer built with it).

Reference: attention_rel_reference.py (float64).  Bound: the project's bound
for fp32 kernels, |err| <= 2e-5 * (1 + |ref|); the value cases also compute the
error of torch float32 on the CPU for the same formula and take
max(2e-5, 4 x that) if it exceeds 5e-6 (as test_attention_large_logits does).
Inputs: Q, K, V and the table U(+-1), biases U(+-0.5).  The kernel's tiles are
asr_attention_fwd's (attention_reference.ATTN_SHAPES) plus a 128-row ring of
table rows in two halves: (193, 1, 1, 64) walks four key blocks, so both halves
are written twice.  Table rows outside the needed range hold NaN everywhere.
Bit-independence cases compare with np.array_equal.
"""
import copy
import functools

import numpy as np
import pytest
import torch

import attention_reference as ar
import attention_rel_reference as atr
import conformer_reference as cf
from conftest import asr
from test_attention_gpu import ATOL, SENT, View, check_valid_rows, close, dm, fetch, ids, nan_past_lengths, put
from test_attention_gpu import run as run_plain

pytestmark = pytest.mark.gpu
SHAPES = ar.ATTN_SHAPES + [(193, 1, 1, 64)]
PAD = 3                                       # NaN rows on either side of the needed table rows


def run(q, k, v, heads, pos, pos_zero, u=None, bv=None, mask=(1, -1, -1), lengths=None, q_pos0=0, k_pos0=0, ld=None,
        misalign=False, fused=False, rc=False, pad=PAD):
    """asr_attention_rel_fwd on q [Tq][B][E], k, v [Tk][B][E] and the table pos;
    pad NaN rows go around the table.  ld: row stride of q, k, v, out and the
    table; misalign: every buffer 4 bytes past a 16-byte boundary; fused: q, k,
    v as column ranges of one buffer; rc: return the status instead of raising."""
    Tq, B, E = q.shape
    Tk = k.shape[0]
    desc = asr.attn_desc(heads, E // heads, 0.0, *mask)
    if fused:
        buf = put(np.concatenate([q, k, v], axis=2).reshape(Tq * B, 3 * E))
        dq, dk, dv = (asr.ColumnView(buf, E * i) for i in range(3))
    else:
        dq, dk, dv = (put(a.reshape(-1, E), ld, misalign=misalign) for a in (q, k, v))
    nan = np.full((pad, E), np.nan, np.float32)
    dp = put(np.concatenate([nan, pos, nan]), ld, misalign=misalign)
    du, dbv = (None if a is None else put(a.reshape(-1, 1), misalign=misalign) for a in (u, bv))
    ldo = ld or E
    out = put(np.full((Tq * B, ldo), SENT, np.float32), misalign=misalign)
    ln = None if lengths is None else asr.device_lengths(lengths)
    args = (dq, dk, dv, out, Tq, Tk, B, desc, View(dp.ptr, pos.shape[0] + 2 * pad, dp.cols, dp), pos_zero + pad, du, dbv)
    try:
        asr.attention_rel_fwd(*args, lengths=ln, q_pos0=q_pos0, k_pos0=k_pos0)
    except asr.AsrError as e:
        if rc:
            return e.status
        raise
    asr.synchronize()
    got = fetch(out, Tq * B, ldo).reshape(Tq, B, ldo)
    assert np.all(got[:, :, E:] == SENT)
    return got[:, :, :E]


@functools.lru_cache(maxsize=None)
def case(shape, mask="full", lengths=None):
    """(q, k, v, pos, pos_zero, u, bv, float64 reference), read-only."""
    q, k, v = ar.draw_attention(shape)
    pos, pz, u, bv = atr.draw_rel(shape, ar.MASKS[mask])
    ref, _ = atr.attention_rel_ref(q, k, v, shape[2], pos, pz, u, bv, *ar.MASKS[mask], lengths=lengths)
    for a in (q, k, v, pos, u, bv, ref):
        a.setflags(write=False)
    return q, k, v, pos, pz, u, bv, ref


def torch32(q, k, v, heads, pos, pz, u, bv, mask):
    """The formula in torch float32 on the CPU (full buffers, gathered table rows)."""
    T, B, E = q.shape
    t = lambda a: torch.from_numpy(np.array(a))   # noqa: E731
    sp = lambda a: t(a).view(-1, B, heads, E // heads)   # noqa: E731
    allowed = t(ar.mask_matrix(T, T, T, *mask))
    row = (pz - (np.arange(T)[:, None] - np.arange(T)[None, :])).clip(0, pos.shape[0] - 1)
    pg = t(pos).view(-1, heads, E // heads)[t(row)]                                # [T][T][h][d]
    ac = torch.einsum("ibhd,jbhd->bhij", sp(q) + t(u).view(heads, -1), sp(k))
    bd = torch.einsum("ibhd,ijhd->bhij", sp(q) + t(bv).view(heads, -1), pg)
    s = ((ac + bd) / np.sqrt(E // heads)).masked_fill(~allowed, -float("inf"))
    return torch.einsum("bhij,jbhd->ibhd", torch.softmax(s, -1), sp(v)).reshape(T, B, E).numpy()


# ------------------------------------------------------------------ values
@pytest.mark.parametrize("mask", list(ar.MASKS))
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_rel_values(shape, mask):
    q, k, v, pos, pz, u, bv, ref = case(shape, mask)
    e32 = (np.abs(torch32(q, k, v, shape[2], pos, pz, u, bv, ar.MASKS[mask]) - ref) / (1 + np.abs(ref))).max()
    bound = max(ATOL, 4 * e32) if e32 > 5e-6 else ATOL
    print(f"torch float32 (CPU) err / (1 + |ref|) {e32:.3e}, bound {bound:.3e}")
    close(run(q, k, v, shape[2], pos, pz, u, bv, ar.MASKS[mask]), ref, f"rel {ids(shape)} {mask}", atol=bound)


@pytest.mark.parametrize("mask", ["full", "chunked"])
@pytest.mark.parametrize("shape", [ar.ATTN_SHAPES[2], ar.ATTN_SHAPES[3], ar.ATTN_SHAPES[5]], ids=ids)
def test_rel_lengths(shape, mask):
    """Ragged lengths, NaN in every Q / K / V row past its length: exact zeros there."""
    T, B, H, D = shape
    ln = ar.ragged_lengths(T, B)
    q, k, v, pos, pz, u, bv, ref = case(shape, mask, ln)
    got = run(*(nan_past_lengths(a, ln) for a in (q, k, v)), H, pos, pz, u, bv, ar.MASKS[mask], lengths=ln)
    for b, n in enumerate(ln):
        assert not got[n:, b].any(), b
    close(got, ref, f"rel lengths {ids(shape)} {mask}")


# ------------------------------------------------------- bit-independence
BIT = ar.ATTN_SHAPES[2]                        # (70, 3, 2, 36): two blocks, a partial dim tile


@pytest.mark.parametrize("mask", ["full", "causal", "chunked"])
@pytest.mark.parametrize("shape", [ar.ATTN_SHAPES[2], ar.ATTN_SHAPES[3], ar.ATTN_SHAPES[4]], ids=ids)
def test_zero_table_and_null_biases_give_attention_fwd_bits(shape, mask):
    q, k, v, pos, pz, *_ = case(shape, mask)
    ln = ar.ragged_lengths(shape[0], shape[1])
    got = run(q, k, v, shape[2], np.zeros_like(pos), pz, mask=ar.MASKS[mask], lengths=ln)
    assert np.array_equal(got, run_plain(q, k, v, shape[2], ar.MASKS[mask], lengths=ln))


@pytest.mark.parametrize("mask", ["full", "window"])
def test_bits_do_not_depend_on_the_table_size_or_pos_zero(mask):
    q, k, v, pos, pz, u, bv, _ = case(BIT, mask)
    rng = np.random.default_rng(3)
    big = np.concatenate([rng.uniform(-1, 1, (41, pos.shape[1])), pos, rng.uniform(-1, 1, (7, pos.shape[1]))])
    a = run(q, k, v, BIT[2], pos, pz, u, bv, ar.MASKS[mask])
    assert np.array_equal(a, run(q, k, v, BIT[2], big.astype(np.float32), pz + 41, u, bv, ar.MASKS[mask]))


@pytest.mark.parametrize("mask", ["full", "chunked"])
def test_bits_do_not_depend_on_the_batch(mask):
    """One utterance alone (B = 1) == the same utterance inside a ragged batch."""
    T, B, H, D = BIT
    q, k, v, pos, pz, u, bv, _ = case(BIT, mask)
    ln, n = (T, 0, T - 3), T - 3
    got = run(*(nan_past_lengths(a, ln) for a in (q, k, v)), H, pos, pz, u, bv, ar.MASKS[mask], lengths=ln)
    alone = run(*(nan_past_lengths(a[:, 2:3], [n]) for a in (q, k, v)), H, pos, pz, u, bv, ar.MASKS[mask], lengths=(n,))
    assert alone[:n].any() and np.array_equal(got[:, 2], alone[:, 0])


@pytest.mark.parametrize("how", ["strided-misaligned", "fused"])
def test_bits_do_not_depend_on_strides_alignment_or_fused_qkv(how):
    """ld = E + 1 with every pointer 4 bytes past a 16-byte boundary; Q, K, V as column views of one buffer."""
    q, k, v, pos, pz, u, bv, _ = case(BIT, "window")
    ln = ar.ragged_lengths(BIT[0], BIT[1])
    a = run(q, k, v, BIT[2], pos, pz, u, bv, ar.MASKS["window"], lengths=ln)
    kw = dict(fused=True) if how == "fused" else dict(ld=BIT[2] * BIT[3] + 1, misalign=True)
    assert np.array_equal(a, run(q, k, v, BIT[2], pos, pz, u, bv, ar.MASKS["window"], lengths=ln, **kw))


def sub_table(pos, pz, Tq, Tk, mask, q_pos0, k_pos0):
    """The rows of the whole call's table that a call on a slice of the frames needs."""
    dmax, dmin = atr.needed_rows(Tq, Tk, *mask, q_pos0, k_pos0)
    return pos[pz - dmax:pz - dmin + 1], dmax


def test_streaming_chunks_give_the_whole_calls_bits():
    """Mask (chunk 16, left 2, right 0) over T = 150: chunk by chunk on the K / V of
    frames [16 (c - 2), 16 (c + 1)) with each call's minimal table == one call."""
    shape, mask = (150, 3, 2, 36), ar.MASKS["chunked"]
    T, H, ln = shape[0], shape[2], (150, 0, 65)
    q, k, v, pos, pz, u, bv, ref = case(shape, "chunked", ln)
    q, k, v = (nan_past_lengths(a, ln) for a in (q, k, v))
    whole = run(q, k, v, H, pos, pz, u, bv, mask, lengths=ln)
    parts = []
    for q0 in range(0, T, 16):
        q1, k0 = min(q0 + 16, T), max(0, q0 - 32)
        parts.append(run(q[q0:q1], k[k0:q1], v[k0:q1], H, *sub_table(pos, pz, q1 - q0, q1 - k0, mask, q0, k0), u, bv, mask,
                         lengths=ln, q_pos0=q0, k_pos0=k0))
    assert np.array_equal(np.concatenate(parts), whole)
    close(whole, ref, "streaming whole")


def test_positions_q_pos0_differs_from_k_pos0():
    """Queries 77 .. 119 over keys 67 .. 149 (Tq 43, Tk 83, k_pos0 no multiple of 64) under the
    window (1, 10, 3) == those rows of the whole call."""
    shape, mask = (150, 3, 2, 36), ar.MASKS["window"]
    q, k, v, pos, pz, u, bv, _ = case(shape, "window")
    whole = run(q, k, v, shape[2], pos, pz, u, bv, mask)
    part = run(q[77:120], k[67:], v[67:], shape[2], *sub_table(pos, pz, 43, 83, mask, 77, 67), u, bv, mask, q_pos0=77,
               k_pos0=67)
    assert np.array_equal(part, whole[77:120])


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("end", ["top", "bottom"])
def test_a_table_one_row_short_is_refused(end):
    q, k, v, pos, pz, u, bv, _ = case(ar.ATTN_SHAPES[0])
    short, z = (pos[1:], pz - 1) if end == "top" else (pos[:-1], pz)
    assert run(q, k, v, 1, short, z, u, bv, rc=True, pad=0) == asr.ASR_ERR_ARG
    assert run(q, k, v, 1, pos, pz, u, bv, rc=True, pad=0).shape == q.shape


def rel_module(E, heads, seed):
    """atr.RelPositionAttention with drawn parameters (weights U(+-1/sqrt(E)), biases U(+-0.1), u / v U(+-0.5))."""
    m = atr.RelPositionAttention(E, heads).double()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, prm in m.named_parameters():
            a = 0.5 if "pos_bias" in name else 0.1 if name.endswith("bias") else E ** -0.5
            prm.copy_((torch.rand(prm.shape, generator=g, dtype=torch.float64) * 2 - 1) * a)
    return m


LAYER = (70, 3, 72, 2, 96, 7)                  # T, B, E, heads, F, kernel


def conformer_parts(first=False):
    block = cf.make_block(LAYER, convolution_first=first)
    parts = block.explicit_parts()
    parts["attn"] = (parts["attn"][0], rel_module(LAYER[2], LAYER[3], 31))
    return block, parts


@pytest.mark.parametrize("which", ["conformer", "mha", "rel"])
def test_a_short_x_raises_before_any_device_call(which):
    T, B, E, H = LAYER[:4]
    layer = {"conformer": lambda: asr.ConformerLayer.from_torch(**conformer_parts()[1]),
             "mha": lambda: asr.MultiheadAttention(E, H),
             "rel": lambda: asr.RelPositionMultiheadAttention(E, H)}[which]()
    with pytest.raises(ValueError, match="needs"):
        layer.forward(asr.DeviceMatrix((T - 1) * B, E), T, B)
    with pytest.raises(ValueError, match="needs"):
        layer.forward(asr.DeviceMatrix(T * B, E - 1), T, B)


# ----------------------------------------------------------------- classes
def rel_ref(m, x, lengths, window):
    """m (float64) on each utterance's own frames with its own 2 n - 1 table."""
    def fn(xu, n):
        allowed = torch.from_numpy(ar.mask_matrix(n, n, n, *window))
        return m(xu.transpose(0, 1), atr.rel_pos_emb(n, x.shape[2]), allowed).transpose(0, 1)
    return cf.per_utterance(fn, x, lengths, x.shape[2])


@pytest.mark.parametrize("window", [(1, -1, -1), (16, 2, 0)], ids=["full", "chunked"])
def test_from_torch_rel_position_attention(window):
    T, B, E, H = LAYER[:4]
    m = rel_module(E, H, 30)
    layer = asr.RelPositionMultiheadAttention.from_torch(m, *window)
    x, ln = cf.draw_x(T, B, E), ar.ragged_lengths(T, B)
    out = layer.forward(dm(nan_past_lengths(x, ln).reshape(T * B, E)), T, B, lengths=ln)
    asr.synchronize()
    check_valid_rows(out.toCpu().reshape(T, B, E), rel_ref(m, x, ln, window), ln, f"RelPositionMultiheadAttention {window}")
    table = layer._table
    layer.forward(dm(x[:20].reshape(20 * B, E)), 20, B)          # fewer frames: the cached table serves
    assert layer._table is table


def test_conformer_layer_with_rel_position_attention():
    """The block of conformer_reference.py with the stand-in as its attention, composed in float64."""
    T, B, E = LAYER[:3]
    block, parts = conformer_parts()
    layer = asr.ConformerLayer.from_torch(**parts)
    assert isinstance(layer.attn, asr.RelPositionMultiheadAttention)
    b64, m = copy.deepcopy(block).double(), parts["attn"][1]

    def fn(xu, n):
        xu = b64.ffn1(xu) * 0.5 + xu
        nrm = b64.self_attn_layer_norm(xu)
        xu = b64._conv(xu + m(nrm.transpose(0, 1), atr.rel_pos_emb(n, E)).transpose(0, 1))
        return b64.final_layer_norm(b64.ffn2(xu) * 0.5 + xu)

    x, ln = cf.draw_x(T, B, E), ar.ragged_lengths(T, B)
    out = layer.forward(dm(nan_past_lengths(x, ln).reshape(T * B, E)), T, B, lengths=ln)
    asr.synchronize()
    check_valid_rows(out.toCpu().reshape(T, B, E), cf.per_utterance(fn, x, ln, E), ln, "ConformerLayer with rel attention")
