"""CPU checks of the references for relative-position self-attention
(attention_rel_reference.py) and of asr.rel_positional_encoding: the float64
numpy restatement against the literal pad-and-view rel-shift of the toolkits'
formulation and against attention_reference.attention_ref, and the sinusoidal
table against its definition and against the toolkits' pos_emb.  No GPU here."""
import numpy as np
import pytest
import torch

import attention_reference as ar
import attention_rel_reference as rr
from conftest import asr


# ------------------------------------- the reference against the toolkits' form
def close64(got, ref):
    assert np.all(np.abs(got - ref) <= 1e-12 * (1 + np.abs(ref))), np.abs(got - ref).max()


@pytest.mark.parametrize("T", [1, 5, 70])
def test_reference_equals_the_literal_rel_shift(T):
    """Full attention: the numpy restatement (row pos_zero - (p - r) of the
    table) == matrix_ac + rel_shift(matrix_bd) with the pad-and-view shift."""
    B, H, D = 3, 2, 12
    E = H * D
    q, k, v = ar.draw_attention((T, B, H, D), seed=3)
    rng = np.random.default_rng(T)
    pos = rng.uniform(-1, 1, (2 * T - 1, E))
    u, vb = rng.uniform(-0.5, 0.5, E), rng.uniform(-0.5, 0.5, E)
    ref, seen = rr.attention_rel_ref(q, k, v, H, pos, T - 1, u, vb)
    assert seen.all()
    mod = rr.RelPositionAttention(E, H).double()
    with torch.no_grad():
        mod.pos_bias_u.copy_(torch.from_numpy(u.reshape(H, D)))
        mod.pos_bias_v.copy_(torch.from_numpy(vb.reshape(H, D)))
        t = lambda a: torch.from_numpy(np.asarray(a, np.float64)).transpose(0, 1).reshape(B, T, H, D)   # noqa: E731
        got = mod.core(t(q), t(k), t(v), torch.from_numpy(pos).reshape(1, 2 * T - 1, H, D))
    close64(got.transpose(0, 1).numpy(), ref)


@pytest.mark.parametrize("mask", list(ar.MASKS), ids=list(ar.MASKS))
def test_reference_with_zero_table_is_attention_ref(mask):
    shape = (70, 3, 2, 36)
    T, B, H, D = shape
    q, k, v = ar.draw_attention(shape)
    ln = ar.ragged_lengths(T, B)
    pos, pos_zero, _u, _v = rr.draw_rel(shape, ar.MASKS[mask])
    got, seen = rr.attention_rel_ref(q, k, v, H, np.zeros_like(pos), pos_zero, None, np.zeros(H * D), *ar.MASKS[mask],
                                     lengths=ln)
    ref, seen0 = ar.attention_ref(q, k, v, H, *ar.MASKS[mask], lengths=ln)
    assert np.array_equal(seen, seen0)
    assert np.array_equal(got, ref)


def test_reference_offsets_are_a_slice():
    """q_pos0 / k_pos0 and a minimal table: rows of a call on a slice of the frames equal the whole call's rows."""
    shape = (70, 3, 2, 36)
    q, k, v = ar.draw_attention(shape)
    pos, pos_zero, u, vb = rr.draw_rel(shape, (16, 2, 0))
    lengths = (70, 40, 55)
    whole, _ = rr.attention_rel_ref(q, k, v, 2, pos, pos_zero, u, vb, 16, 2, 0, lengths)
    dmax, dmin = rr.needed_rows(16, 48, 16, 2, 0, 48, 16)
    assert (dmax, dmin) == (47, -15)
    small = pos[pos_zero - dmax:pos_zero - dmin + 1]
    part, seen = rr.attention_rel_ref(q[48:64], k[16:64], v[16:64], 2, small, dmax, u, vb, 16, 2, 0, lengths,
                                      q_pos0=48, k_pos0=16)
    assert seen[:, 0].all() and not seen[:, 1].any()
    close64(part, whole[48:64])


# ------------------------------------------------------ the sinusoidal table
@pytest.mark.parametrize("ml,mr,E", [(0, 0, 4), (5, 0, 8), (0, 7, 6), (69, 69, 144), (47, 0, 64)])
def test_rel_positional_encoding_matches_its_definition(ml, mr, E):
    pe = asr.rel_positional_encoding(ml, mr, E)
    assert pe.shape == (ml + mr + 1, E) and pe.dtype == np.float32
    for i in {0, ml, ml + mr, (ml + mr) // 2}:
        delta = ml - i
        for kk in {0, 1, E // 2 - 1}:
            w = 10000.0 ** (-2.0 * kk / E)
            assert pe[i, 2 * kk] == np.float32(np.sin(delta * w)), (i, kk)
            assert pe[i, 2 * kk + 1] == np.float32(np.cos(delta * w)), (i, kk)
    assert np.array_equal(pe[ml, 0::2], np.zeros(E // 2)) and np.array_equal(pe[ml, 1::2], np.ones(E // 2))
    n = min(ml, mr)                                             # delta and -delta: the sines change sign
    for dlt in range(n + 1):
        assert np.array_equal(pe[ml - dlt, 0::2], -pe[ml + dlt, 0::2])
        assert np.array_equal(pe[ml - dlt, 1::2], pe[ml + dlt, 1::2])


def test_rel_positional_encoding_is_the_toolkits_pos_emb():
    T, E = 23, 16
    assert np.array_equal(asr.rel_positional_encoding(T - 1, T - 1, E),
                          rr.rel_pos_emb(T, E)[0].numpy().astype(np.float32))
    for bad in ((-1, 0, 4), (0, -1, 4), (3, 3, 5), (3, 3, 0)):
        with pytest.raises(ValueError):
            asr.rel_positional_encoding(*bad)
