"""The float64 references of tests/gated_rnn_reference.py against torch.nn.LSTM /
torch.nn.GRU in float64, and, on the references alone, the input conditions of
the cases that test_gated_rnn_edges_gpu.py runs: a seed that stops meeting
them fails here, without a GPU.

Bound of the first part: |ref - torch| <= 1e-12 * (1 + |ref|), two float64
evaluations of the same formula in different summation orders.  torch takes
no utterance of length 0, so lengths go through pack_padded_sequence with
every length >= 1 (1 and T among them); reverse is the flipped-input form.
"""
import numpy as np
import pytest
import torch

import gated_rnn_reference as gr

CELLS = ("lstm", "gru")


def lengths_1_T(T, B):
    ln = np.random.default_rng(T + B).integers(1, T + 1, B)
    ln[1], ln[B - 2] = 1, T
    return ln


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
@pytest.mark.parametrize("with_lengths", [False, True], ids=["full", "lengths"])
@pytest.mark.parametrize("use0", [False, True], ids=["zeros", "state"])
@pytest.mark.parametrize("H", [16, 144])
@pytest.mark.parametrize("T", [1, 7])
@pytest.mark.parametrize("cell", CELLS)
def test_reference_is_torch_float64(cell, T, H, use0, with_lengths, reverse):
    B, I = 5, 8
    p = gr.draw(cell, T, B, I, H, seed=100 * H + T)
    ln = lengths_1_T(T, B) if with_lengths else None
    assert ln is None or (1 in ln and T in ln)
    h, hT, cT, z = gr.reference(p, use0, ln, reverse)
    th, thT, tcT = gr.torch_run(p, torch.float64, use0, ln, reverse)
    for name, a, b in (("h", h, th), ("h_T", hT, thT), ("c_T", cT, tcT)):
        if a is not None:
            assert np.all(np.abs(a - b) <= 1e-12 * (1 + np.abs(a))), (name, np.abs(a - b).max())
    if ln is not None:
        for b in range(B):
            assert not h[ln[b]:, b].any()
            assert np.all(np.isnan(z[ln[b]:, b])) and np.all(np.isfinite(z[:ln[b], b]))


@pytest.mark.parametrize("cell", CELLS)
def test_reference_length_zero_and_clamps(cell):
    """What torch cannot run: length 0 keeps h0 / c0 and gives zero rows; -3 is 0 and T + 5 is T; and
    the rows of x at or past a length are never read into a result (NaN there changes nothing)."""
    T, B, I, H = 7, 6, 8, 16
    p = gr.draw(cell, T, B, I, H, seed=5)
    ln = np.array([0, -3, T + 5, 3, 1, T])
    clamped = np.clip(ln, 0, T)
    x = p["x"].copy()
    for b in range(B):
        x[clamped[b]:, b] = np.nan
    for reverse in (False, True):
        a = gr.reference(p, True, ln, reverse)
        b = gr.reference(p, True, clamped, reverse, x=x)
        for u, v in zip(a, b):
            assert u is None or np.array_equal(u, v, equal_nan=True)
        h, hT, cT, _ = a
        assert not h[:, :2].any() and np.array_equal(hT[:2], p["h0"][:2].astype(np.float64))
        assert cT is None or np.array_equal(cT[:2], p["c0"][:2].astype(np.float64))
        full = gr.reference(p, True, None, reverse)
        assert np.array_equal(h[:, 2], full[0][:, 2]) and np.array_equal(hT[2], full[1][2])


def test_reference_given_P():
    """P = x.W_ih given instead of x and W_ih is the same walk."""
    for cell in CELLS:
        p = gr.draw(cell, 4, 3, 8, 16, seed=9)
        P = (p["x"].astype(np.float64).reshape(12, 8) @ p["W_ih"].astype(np.float64)).reshape(4, 3, -1)
        for u, v in zip(gr.reference(p, True, (4, 0, 2), True), gr.reference(p, True, (4, 0, 2), True, P=P)):
            assert u is None or np.array_equal(u, v, equal_nan=True)


# ---------------------------------------------------------------- the GPU cases' input conditions
@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
@pytest.mark.parametrize("T,B,I,H", gr.SATURATED_SHAPES)
@pytest.mark.parametrize("cell", CELLS)
def test_saturated_inputs_saturate(cell, T, B, I, H, reverse):
    """At least 5 % of the walk's gate pre-activations have |z| > 20 and at least 5 % have |z| < 2;
    torch's own float32 stays close enough to float64 for the case's bound to mean something."""
    p = gr.saturated(cell, T, B, I, H)
    h, hT, cT, z = gr.reference(p, True, None, reverse)
    big, small = gr.shares(z)
    th, thT, tcT = gr.torch_run(p, torch.float32, True, None, reverse)
    e32 = max(gr.rel_err(th, h), gr.rel_err(thT, hT), 0.0 if cT is None else gr.rel_err(tcT, cT))
    print(f"{cell} {(T, B, I, H)} reverse={reverse}: |z| > 20 {big:.1%}, |z| < 2 {small:.1%}, max |z| "
          f"{np.nanmax(np.abs(z)):.1f}, torch float32 {e32:.2e}")
    assert big >= 0.05 and small >= 0.05
    assert e32 <= 5e-6          # so that max(2e-5, 4 e32) stays the suite's bound


@pytest.mark.parametrize("H", [32, 144])
@pytest.mark.parametrize("cell", CELLS)
def test_extreme_P_overflows_expf_both_ways(cell, H):
    T, B = 2, 5
    p = gr.draw(cell, T, B, 8, H, seed=4200 + H)
    P = gr.extreme_P(cell, T, B, H)
    assert np.all(np.isfinite(P))
    h, hT, cT, z = gr.reference(p, True, None, False, P=P)
    assert np.all(np.isfinite(h)) and np.all(np.isfinite(hT)) and (cT is None or np.all(np.isfinite(cT)))
    for q in range(gr.NG[cell]):        # every gate sees an overflow of expf(-z) and of expf(z), and moderate values
        zq = z[:, :, q * H:(q + 1) * H]
        assert (zq < -88.73).any() and (zq > 88.73).any() and (np.abs(zq) < 2).any(), q


def test_permutation_moves_tiles_and_lane_groups():
    B = 37
    perm = gr.permutation(B)
    assert sorted(perm) == list(range(B))
    pos = np.argsort(perm)                      # utterance u sits at position pos[u]
    assert pos[0] != 0 and pos[B - 1] != B - 1
    assert pos[0] // 16 != 0 and pos[B - 1] // 16 != (B - 1) // 16      # another row tile
    u = np.arange(B)
    assert np.mean(pos // 16 != u // 16) > 0.5
    assert np.mean((pos % 16) // 4 != (u % 16) // 4) > 0.5
    assert perm[0] != 0 and perm[B - 1] != B - 1    # rows 0 (read by rows past B) and B - 1 (the clamped A row)
    ln = gr.ragged_lengths(6, B, 1)
    assert 0 in ln and 1 in ln and 6 in ln


def test_nan_case_lengths():
    for T, B in ((7, 21),):
        ln = gr.nan_case_lengths(T, B)
        assert {0, 1, T, -3, T + 5} <= set(ln.tolist())
