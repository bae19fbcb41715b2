"""The gated recurrence (csrc/gated_rnn.hip: asr_lstm_fwd / asr_lstm_recur_fwd /
asr_gru_fwd / asr_gru_recur_fwd, asr.GRU) where test_lstm_gpu.py and
test_gru_gpu.py do not look: T = 1, H = 2048, saturated gates, a long
sequence, NaN in the padding, a permuted batch, in-place state carry.

Reference: the float64 walks of tests/gated_rnn_reference.py (checked against
torch in float64 by test_gated_rnn_edges_cpu.py, which also asserts these
cases' input conditions).  Bound, unless a test says otherwise: the suite's
|err| <= 2e-5 * (1 + |ref|) on h, h_T and (LSTM) c_T.  Every case asserts
finiteness and prints its max err / (1 + |ref|).

Forms: 16 <= H <= 128 is the resident kernel (one launch), H > 128 the step
kernel (one launch per frame, four 16-column tiles per workgroup).
"""
import functools

import numpy as np
import pytest
import torch

import gated_rnn_reference as gr
from conftest import asr

pytestmark = pytest.mark.gpu
ATOL = 2e-5
CELLS = ("lstm", "gru")


def dm(a):
    a = np.asarray(a, np.float32)
    return asr.DeviceMatrix.from_numpy(a.reshape(-1, a.shape[-1]) if a.ndim > 1 else a.reshape(-1, 1))


@functools.lru_cache(maxsize=8)
def device_weights(cell, T, B, I, H, seed, w_ih=1.0, bias=0.1):
    """The drawn inputs (gated_rnn_reference.draw) and their four weight matrices on the device."""
    p = gr.draw(cell, T, B, I, H, seed, w_ih, bias)
    return p, [dm(p["W_ih"]), dm(p["W_hh"]), dm(p["b_ih"]), dm(p["b_hh"])]


def run(p, W, use0=True, lengths=None, reverse=False, recur=False, x=None, P=None, hid=None, h0=None, c0=None,
        hT=None, cT=None):
    """One layer and direction on the device: (h [T, B, ldh], h_T [B, H], c_T [B, H] or None).  recur: through
    *_recur_fwd on P (default: asr_linear_fwd's x.W_ih).  hid / h0 / c0 / hT / cT: device matrices to use
    instead of fresh ones (h0 / c0 default to the drawn ones when use0)."""
    T, B, H, lstm = p["T"], p["B"], p["H"], p["cell"] == "lstm"
    G = gr.NG[p["cell"]] * H
    hid = asr.DeviceMatrix(T * B, H) if hid is None else hid
    h0 = (dm(p["h0"]) if use0 else None) if h0 is None else h0
    c0 = (dm(p["c0"]) if use0 and lstm else None) if c0 is None else c0
    hT = asr.DeviceMatrix(B, H) if hT is None else hT
    cT = (asr.DeviceMatrix(B, H) if lstm else None) if cT is None else cT
    ln = None if lengths is None else asr.device_lengths(lengths)
    xd = dm(p["x"] if x is None else x)
    kw = dict(h0=h0, hT=hT, lengths=ln, reverse=reverse)
    if recur or P is not None:
        if P is None:
            Pd = asr.DeviceMatrix(T * B, G)
            asr.linear_fwd(xd, W[0], None, Pd, asr.EPI_NONE)
        else:
            Pd = dm(P)
        if lstm:
            work = asr.DeviceBytes(asr.lstm_workspace_bytes(T, B, H))
            asr.lstm_recur_fwd(Pd, W[1], W[2], W[3], hid, T, B, work, c0=c0, cT=cT, **kw)
        else:
            asr.gru_recur_fwd(Pd, W[1], W[2], W[3], hid, T, B, **kw)
    elif lstm:
        asr.lstm_fwd(xd, *W, hid, T, B, asr.DeviceBytes(asr.lstm_workspace_bytes(T, B, H)), c0=c0, cT=cT, **kw)
    else:
        asr.gru_fwd(xd, *W, hid, T, B, asr.DeviceBytes(asr.gru_workspace_bytes(T, B, H)), **kw)
    asr.synchronize()
    return hid.toCpu().reshape(T, B, hid.cols), hT.toCpu(), cT.toCpu() if lstm else None


def check(got, ref, what, bound=ATOL):
    """Finite, and |got - ref| <= bound * (1 + |ref|) on h, h_T and c_T; returns the max err / (1 + |ref|)."""
    worst = 0.0
    for name, g, r in zip(("h", "h_T", "c_T"), got, ref):
        if r is None:
            continue
        assert np.all(np.isfinite(g)), f"{what} {name}: not finite"
        e = gr.rel_err(g, r)
        worst = max(worst, e)
        assert e <= bound, f"{what} {name}: max err / (1 + |ref|) {e:.3e} > {bound:.3e}"
    print(f"{what}: max err / (1 + |ref|) {worst:.3e} (bound {bound:.1e})")
    return worst


def same_bits(a, b, what):
    for name, u, v in zip(("h", "h_T", "c_T"), a, b):
        if u is not None:
            assert np.array_equal(u.view(np.uint32), v.view(np.uint32)), f"{what}: {name} differs"


# ------------------------------------------------------------------------------------------- T = 1
@pytest.mark.parametrize("B", [1, 17])
@pytest.mark.parametrize("H", [16, 128, 144, 256])
@pytest.mark.parametrize("cell", CELLS)
def test_single_frame(cell, H, B):
    """T = 1, how a streaming caller runs the layer: the resident kernel's first prefetch is also its
    past-the-end one, and the step form's one launch has k == 0 and last == 1 together.  Forward and
    reverse, with and without h0 / c0, without lengths and with lengths that mix 1 and 0, through
    *_fwd and *_recur_fwd; h_T / c_T of a length-0 utterance are h0 / c0 bit for bit (zeros without)."""
    T, I = 1, 8
    p, W = device_weights(cell, T, B, I, H, seed=1100 + H + B)
    mixes = (None, tuple(int(b % 3 != 0) for b in range(B)), tuple(int(b % 3 == 0) for b in range(B)))
    assert {0, 1} == set(mixes[1]) | set(mixes[2]) and (B == 1 or {0, 1} == set(mixes[1]) == set(mixes[2]))
    worst = 0.0
    for reverse in (False, True):
        for use0 in (False, True):
            for ln in mixes:
                ref = gr.reference(p, use0, ln, reverse)[:3]
                for recur in (False, True):
                    what = f"{cell} H={H} B={B} reverse={reverse} use0={use0} lengths={ln is not None} recur={recur}"
                    got = run(p, W, use0, ln, reverse, recur)
                    worst = max(worst, check(got, ref, what))
                    for b in range(B if ln is not None else 0):
                        if ln[b] == 0:
                            assert not got[0][:, b].any(), what
                            for state, init in ((got[1], p["h0"]), (got[2], p["c0"])):
                                if state is not None:
                                    want = init[b] if use0 else np.zeros(H, np.float32)
                                    assert np.array_equal(state[b].view(np.uint32), want.view(np.uint32)), what
    print(f"T=1 {cell} H={H} B={B}: worst of 24 calls {worst:.3e}")


# --------------------------------------------------------------------------------- the upper limit
@pytest.mark.parametrize("cell", CELLS)
def test_H_2048(cell):
    """GR_HMAX: H = 2048 (32 groups of four 16-column tiles, 128 16-k chunks), T = 3, B = 3, lengths
    (3, 0, 2), forward and reverse.  The weights (W_hh is 64 MB for the LSTM) are drawn once."""
    T, B, I, H, ln = 3, 3, 8, 2048, (3, 0, 2)
    p, W = device_weights(cell, T, B, I, H, seed=2048)
    p64 = dict(p, W_hh=p["W_hh"].astype(np.float64))        # one conversion for both directions
    for reverse in (False, True):
        got = run(p, W, True, ln, reverse)
        check(got, gr.reference(p64, True, ln, reverse)[:3], f"{cell} H=2048 reverse={reverse}")
        assert not got[0][:, 1].any() and not got[0][2:, 2].any()
        assert np.array_equal(got[1][1], p["h0"][1])
    device_weights.cache_clear()


# --------------------------------------------------------------------------------- saturated gates
@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
@pytest.mark.parametrize("T,B,I,H", gr.SATURATED_SHAPES)
@pytest.mark.parametrize("cell", CELLS)
def test_saturated_gates(cell, T, B, I, H, reverse):
    """W_ih ~ U(+-120 / sqrt(H)) and biases ~ U(+-10): at least 5 % of the gate pre-activations have |z| > 20
    (sigmoid and tanh in their tails, f = i = 1 chains) and at least 5 % have |z| < 2.  The saturation comes
    from the input side, so the recurrence stays contractive and a bound means something.  Bound:
    max(2e-5, 4 x torch float32's own error on the CPU) * (1 + |ref|), as test_attention_large_logits."""
    p = gr.saturated(cell, T, B, I, H)
    W = [dm(p[k]) for k in ("W_ih", "W_hh", "b_ih", "b_hh")]
    ref = gr.reference(p, True, None, reverse)
    big, small = gr.shares(ref[3])
    assert big >= 0.05 and small >= 0.05
    t32 = gr.torch_run(p, torch.float32, True, None, reverse)
    e32 = max(gr.rel_err(a, b) for a, b in zip(t32, ref[:3]) if b is not None)
    bound = max(ATOL, 4 * e32)
    print(f"{cell} {(T, B, I, H)} reverse={reverse}: |z| > 20 {big:.1%}, |z| < 2 {small:.1%}; bound terms: "
          f"2e-5 and 4 x {e32:.3e} (torch float32 on the CPU)")
    check(run(p, W, True, None, reverse), ref[:3], f"saturated {cell} {(T, B, I, H)} reverse={reverse}", bound)


@pytest.mark.parametrize("H", [32, 144])
@pytest.mark.parametrize("cell", CELLS)
def test_extreme_preactivations(cell, H):
    """*_recur_fwd on a hand-built P whose entries cycle through +-1e4, +-104, +-88, +-20 and U(+-1): expf
    overflows to inf in the sigmoid at z < -88.7, and would in a sigmoid written with expf(z) at z > 88.7."""
    T, B = 2, 5
    p, W = device_weights(cell, T, B, 8, H, seed=4200 + H)
    P = gr.extreme_P(cell, T, B, H)
    ref = gr.reference(p, True, None, False, P=P)
    check(run(p, W, True, None, False, P=P), ref[:3], f"extreme P {cell} H={H}")


# --------------------------------------------------------------------------------- a long sequence
@pytest.mark.parametrize("H", [32, 144])
@pytest.mark.parametrize("cell", CELLS)
def test_long_sequence(cell, H):
    """T = 300 at the suite's ordinary weight scales, lengths (300, 150): the bound holds at every frame
    (torch float32 is 4e-8 to 5e-8 from float64 here, so the error does not grow along the sequence)."""
    T, B, I, ln = 300, 2, 8, (300, 150)
    p, W = device_weights(cell, T, B, I, H, seed=300 + H)
    ref = gr.reference(p, True, ln, False)
    got = run(p, W, True, ln, False)
    check(got, ref[:3], f"long {cell} H={H}")
    assert not got[0][150:, 1].any()
    print(f"long {cell} H={H}: first 50 frames {gr.rel_err(got[0][:50], ref[0][:50]):.3e}, last 50 frames "
          f"{gr.rel_err(got[0][-50:], ref[0][-50:]):.3e}")


# ------------------------------------------------------------------------------ NaN in the padding
@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
@pytest.mark.parametrize("H", [48, 144])
@pytest.mark.parametrize("cell", CELLS)
def test_nan_in_padding(cell, H, reverse):
    """The length mask is a select, not arithmetic: every x row at or past its utterance's length is NaN
    (so those rows of P are NaN too), hid is pre-filled with NaN, ldh = H + 4 with a sentinel in the four
    extra columns.  Valid rows are finite and within the bound, rows past the length exact zeros, the
    sentinel intact, and h, h_T, c_T bit-equal to the same call on zero padding and a zeroed hid."""
    T, B, I, SENT = 7, 21, 8, -12345.0
    p, W = device_weights(cell, T, B, I, H, seed=700 + H)
    ln = gr.nan_case_lengths(T, B)
    assert {0, 1, T, -3, T + 5} <= set(ln.tolist())
    clamped = np.clip(ln, 0, T)
    xs = {}
    for name, fill in (("nan", np.nan), ("zero", 0.0)):
        xs[name] = p["x"].copy()
        for b in range(B):
            xs[name][clamped[b]:, b] = fill
    assert np.isnan(xs["nan"]).any()
    outs = {}
    for name, fill in (("nan", np.nan), ("zero", 0.0)):
        pre = np.full((T * B, H + 4), fill, np.float32)
        pre[:, H:] = SENT
        outs[name] = run(p, W, True, tuple(int(v) for v in ln), reverse, x=xs[name], hid=dm(pre))
    h, hT, cT = outs["nan"]
    assert np.all(h[:, :, H:] == SENT) and np.all(outs["zero"][0][:, :, H:] == SENT)
    for b in range(B):
        assert np.array_equal(h[clamped[b]:, b, :H].view(np.uint32), np.zeros((T - clamped[b], H), np.uint32)), b
    got = (h[:, :, :H], hT, cT)
    check(got, gr.reference(p, True, ln, reverse, x=xs["nan"])[:3], f"NaN padding {cell} H={H} reverse={reverse}")
    same_bits(got, (outs["zero"][0][:, :, :H],) + outs["zero"][1:], "NaN against zero padding")


# ----------------------------------------------------------------- bits do not depend on the row
@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("cell", CELLS)
def test_bits_do_not_depend_on_the_row(cell, H, reverse):
    """B = 37 and the same utterances permuted (x, h0, c0 and lengths together): all but one utterance move
    to another row, most to another row tile and lane group, rows 0 (which rows past B read) and B - 1 (the
    step form's clamped A row) hold other utterances; h, h_T and c_T come out as the same permutation, bit
    for bit."""
    T, B, I = 6, 37, 8
    p, W = device_weights(cell, T, B, I, H, seed=3700 + H)
    perm = gr.permutation(B)
    ln = gr.ragged_lengths(T, B, H)
    assert 0 in ln and perm[0] != 0 and perm[B - 1] != B - 1 and np.sum(perm == np.arange(B)) <= 1
    a = run(p, W, True, tuple(int(v) for v in ln), reverse)
    q = dict(p, x=np.ascontiguousarray(p["x"][:, perm]), h0=p["h0"][perm], c0=p["c0"][perm])
    b = run(q, W, True, tuple(int(v) for v in ln[perm]), reverse)
    check(a, gr.reference(p, True, ln, reverse)[:3], f"permuted {cell} H={H} reverse={reverse}")
    same_bits((a[0][:, perm], a[1][perm], None if a[2] is None else a[2][perm]), b, "permuted batch")


# --------------------------------------------------------------------------------- in-place state
@pytest.mark.parametrize("T,reverse", [(1, False), (5, True)], ids=["T1-forward", "T5-reverse-length1"])
@pytest.mark.parametrize("cell", CELLS)
def test_state_in_place_resident(cell, T, reverse):
    """H = 48 (the resident form): d_hT == d_h0 and d_cT == d_c0 exactly is legal (a lane reads its own
    element first and writes it last) and gives the bits of the call with separate buffers."""
    B, I, H = 20, 8, 48
    p, W = device_weights(cell, T, B, I, H, seed=4800 + T)
    ln = None
    if T > 1:
        ln = [int(v) for v in gr.ragged_lengths(T, B, 48)]
        assert 1 in ln
        ln = tuple(ln)
    apart = run(p, W, True, ln, reverse)
    h0, c0 = dm(p["h0"]), dm(p["c0"]) if cell == "lstm" else None
    inplace = run(p, W, True, ln, reverse, h0=h0, c0=c0, hT=h0, cT=c0)
    check(inplace, gr.reference(p, True, ln, reverse)[:3], f"in place {cell} T={T}")
    same_bits(apart, inplace, "in place against separate buffers")


@pytest.mark.parametrize("cell", CELLS)
def test_state_in_place_refused_in_the_step_form(cell):
    """H = 256: the step form reads whole h0 rows while it stores d_hT in the same launch, so d_hT == d_h0
    is ASR_ERR_ARG (nothing is launched); a partial overlap is refused in both forms."""
    for H in (48, 256):
        p, W = device_weights(cell, 1, 20, 8, H, seed=4900 + H)
        h0 = dm(np.concatenate([p["h0"], p["h0"]]))         # [2B, H]: rows [0, B) as h0, a view B / 2 rows in as hT
        views = [asr._DeviceView(h0, 10, 20)] + ([asr._DeviceView(h0, 0, 20)] if H > 128 else [])
        for hT in views:
            with pytest.raises(asr.AsrError) as e:
                run(p, W, True, None, False, h0=asr._DeviceView(h0, 0, 20), hT=hT)
            assert e.value.status == asr.ASR_ERR_ARG


@pytest.mark.parametrize("H", [48, 256])
def test_gru_class_streams_on_its_own_state(H):
    """asr.GRU, 2 layers, unidirectional, B = 20, ragged lengths: T = 8 run in chunks of (1, 1, 2, 1, 3)
    frames with h0=net.h_n each time and the lengths clipped per chunk equals one T = 8 call bit for bit,
    in the outputs and in the final h_n, and equals the same chain with a host copy of h_n uploaded as a
    fresh h0.  (Two chunks of the same T in a row keep the state matrix: without the second matrix of
    _GatedRNN._forward the step form at H = 256 would be asked to write d_hT over d_h0.)"""
    T, B, I, L, chunks = 8, 20, 8, 2, (1, 1, 2, 1, 3)
    rng = np.random.default_rng(H)
    s = 1 / np.sqrt(H)
    params = [[tuple(rng.uniform(-lim, lim, shape).astype(np.float32) for lim, shape in
                     ((s, (I if l == 0 else H, 3 * H)), (s, (H, 3 * H)), (0.1, 3 * H), (0.1, 3 * H)))]
              for l in range(L)]
    x = rng.uniform(-1, 1, (T, B, I)).astype(np.float32)
    h_init = rng.uniform(-1, 1, (L * B, H)).astype(np.float32)
    ln = gr.ragged_lengths(T, B, H + 1)
    assert 0 in ln and T in ln

    whole = asr.GRU(I, H, L, False, params)
    out = whole.forward(dm(x), T, B, lengths=tuple(int(v) for v in ln), h0=dm(h_init)).toCpu()
    asr.synchronize()
    want_h = whole.h_n.toCpu()
    # one layer-1 utterance against the float64 reference, so that "equal" is not "equally wrong"
    p0 = {"cell": "gru", "x": x, "h0": h_init[:B], "W_ih": params[0][0][0], "W_hh": params[0][0][1],
          "b_ih": params[0][0][2], "b_hh": params[0][0][3]}
    check((whole.outputs[0].toCpu().reshape(T, B, H), want_h[:B]), gr.reference(p0, True, ln)[:2], f"GRU class H={H}")

    for host_copy in (False, True):
        net = asr.GRU(I, H, L, False, params)
        parts, lo, state = [], 0, dm(h_init)
        for n in chunks:
            before = state.toCpu()
            part = net.forward(dm(x[lo:lo + n]), n, B, lengths=tuple(int(v) for v in np.clip(ln - lo, 0, n)), h0=state)
            parts.append(part.toCpu())
            asr.synchronize()
            assert np.array_equal(state.toCpu(), before)         # the caller's h0 keeps its contents
            assert net.h_n is not state
            state = dm(net.h_n.toCpu()) if host_copy else net.h_n
            lo += n
        same_bits((np.concatenate(parts), net.h_n.toCpu()), (out, want_h), f"chunks, host_copy={host_copy}")
