"""GPU numerics of the audio front end on the paths test_fbank_gpu.py does not
reach (fbank_cases.EDGE_CASES): frames past the 64th of an utterance, the log
floor, 128 / 65 / 64 / 1 mel filters and filters without an FFT bin, the DCT
read from global memory and D > 64, hop > win, hop = 1, win = n_fft, an odd
win, win = 2, clamped and absent lengths, int16-scale samples and a tone over
1-LSB dither.

Reference: fbank_cases.features_parts(), float64.  Bound per case, in the
metric of fbank_cases (|err| / (1 + |ref|) for log-mel, |err| / (1 + sum_m
|dct[k, m] e_ref[m]|) for MFCC): max(2e-5, 3.5 E32), E32 being the fp32 CPU
chain's error against float64 on the same input, computed where the test
runs; tests/test_fbank_edges_cpu.py asserts E32 <= 2e-5 / 3.5 on the cases
marked fixed in fbank_cases.py, so there the bound is the project's 2e-5 (and
it came out as 2e-5 to 2.04e-5 on all but the two tone cases, whose fp32
chain is itself 3e-4 to 6e-4 away from float64).  Every MFCC case also
runs its log-mel twin under the unscaled metric, so the scaled one cannot
hide a wrong log-mel.  Bit equalities (shifted copies, batch position, T,
clamped lengths, silence) are exact.

Measured on an MI355X, max err / (1 + scale), kernel (fp32 CPU chain): see
DESIGN.md §13.
"""
import numpy as np
import pytest

import fbank_cases as fc
from fbank_cases import SENT, check_padding, run, waves
from test_fbank_gpu import CASES

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check(name, got, gf, d, twin=False):
    """frames, padding bits, finite, and the case's bound against float64."""
    F = d.ref.shape[2]
    assert np.array_equal(gf, d.frames)
    assert got.shape[:2] == d.ref.shape[:2]
    assert np.all(got[:, :, F:] == SENT)               # the columns past F are not written
    got = got[:, :, :F]
    check_padding(got, d.frames, d.c)
    assert np.isfinite(got).all()
    abs_err, e_gpu = fc.scaled_error(got, d.ref, d.scale)
    e32, tol = fc.e32(name, twin), fc.bound(name, twin)
    print(f"case {name}{' (log-mel twin)' if twin else ''}: max abs err {abs_err:.3e}, E_gpu {e_gpu:.3e}, "
          f"E32 {e32:.3e}, bound {tol:.3e}")
    assert e_gpu <= tol, f"case {name}: E_gpu {e_gpu:.3e} > {tol:.3e} (E32 {e32:.3e})"
    return got


@pytest.mark.parametrize("name", list(fc.EDGE_CASES))
def test_edge_features(name):
    d = fc.edge(name)
    F = d.ref.shape[2]
    got, gf = run(d.c, d.wave, d.ns, ldo=F + 3)
    check(name, got, gf, d)
    if d.c["n_mfcc"]:
        t = fc.edge(name, twin=True)
        got, gf = run(t.c, t.wave, t.ns, ldo=t.ref.shape[2] + 3)
        check(name, got, gf, t, twin=True)


@pytest.mark.parametrize("name", ["shift-p97", "shift-p0"])
def test_shifted_copies_have_the_same_bits(name):
    """A frame's bits depend on its own samples only: rows t >= 1 of the copy
    advanced by k hop samples are rows t + k of the whole waveform, and row 0
    too without pre-emphasis (x[-1] = 0 at an utterance's start is the only
    difference).  k = 1, 63, 64, 65 set every block and every trip of the
    per-wave loop against block 0 and other waves."""
    d = fc.edge(name)
    got, gf = run(d.c, d.wave, d.ns)
    assert np.array_equal(gf, d.frames)
    first = 0 if d.c["preemph"] == 0.0 else 1
    for i, k in enumerate(fc.SHIFTS):
        n = d.frames[1 + i]
        assert n == d.frames[0] - k
        same = bits(got[first:n, 1 + i]) == bits(got[first + k:n + k, 0])
        assert same.all(), f"k = {k}: rows {sorted(set(np.nonzero(~same)[0] + first))} of the copy differ"


def test_silence_is_the_floor_in_identical_bits():
    """Digital silence: every log-mel element is ln(floor), the same bits."""
    d = fc.edge("floor-logmel")
    got, _ = run(d.c, d.wave, d.ns)
    row = bits(got[:d.frames[0], 0])
    assert np.all(row == row.flat[0])
    v = got[0, 0, 0]
    assert np.isfinite(v) and abs(float(v) - np.log(1e-10)) <= fc.ATOL * (1 + abs(np.log(1e-10)))
    # and the frames inside row 1's gap are those bits too
    inside = np.all(d.logmel[:, 1] == np.log(d.c["log_floor"]), axis=1)[:d.frames[1]]
    assert inside.sum() >= 3 and np.all(bits(got[:d.frames[1], 1][inside]) == row.flat[0])
    # the MFCC of silence: the same bits in every frame
    m = fc.edge("floor-mfcc")
    gm, _ = run(m.c, m.wave, m.ns)
    rows = bits(gm[:m.frames[0], 0])
    assert np.all(rows == rows[0])


def test_lengths_are_clamped_and_frames_is_optional():
    """nsamples above S or negative count as S and 0; d_frames = NULL writes
    the same features."""
    c, B, S, _ = CASES["a"]
    wave = waves(16000, B, S)
    plain, pf = run(c, wave, (S, 0, 1200))
    got, gf = run(c, wave, (S + 5, -3, 1200))
    assert np.array_equal(gf, pf) and list(pf) == [11, 0, 6]
    assert np.array_equal(bits(got), bits(plain))
    nof, none = run(c, wave, (S + 5, -3, 1200), want_frames=False)
    assert none is None
    assert np.array_equal(bits(nof), bits(plain))
    # and without context (the main kernel writes the output itself)
    c0 = dict(c, n_context=0)
    plain, pf = run(c0, wave, (S, 0, 1200))
    got, gf = run(c0, wave, (2 ** 31 - 1, -2 ** 31, 1200), want_frames=True)
    assert np.array_equal(gf, pf) and np.array_equal(bits(got), bits(plain))
    nof, _ = run(c0, wave, (S + 5, -3, 1200), want_frames=False)
    assert np.array_equal(bits(nof), bits(plain))
    ref, frames = fc.features(c0, wave, (S, 0, 1200), plain.shape[0])
    assert np.array_equal(frames, pf)
    check_padding(plain, frames, c0)


def test_batch_independent_past_a_block():
    """blocks-512's 129-frame utterance alone (T = 129), alone with T = 129 + 70,
    second of five and last of five (T = 140): the same bits on the common rows."""
    d = fc.edge("blocks-512")
    five, f5 = run(d.c, d.wave, d.ns)
    n = int(d.ns[1])
    assert d.frames[1] == 2 * fc.FRAMES_PER_WG + 1
    alone_wave = np.ascontiguousarray(d.wave[1:2, :n])
    alone, fa = run(d.c, alone_wave)
    assert alone.shape[0] == 129 and list(fa) == [129]
    assert np.array_equal(bits(alone[:, 0]), bits(five[:129, 1]))
    longer, fl = run(d.c, alone_wave, T=129 + 70)
    assert list(fl) == [129]
    assert np.array_equal(bits(longer[:129]), bits(alone)) and not bits(longer[129:]).any()
    # last of five, after utterances of other lengths
    order = [0, 2, 3, 4, 1]
    last, fo = run(d.c, np.ascontiguousarray(d.wave[order]), tuple(d.ns[i] for i in order))
    assert np.array_equal(fo, f5[order])
    assert np.array_equal(bits(last[:, 4]), bits(five[:, 1]))
    assert np.array_equal(bits(last[:, 1]), bits(five[:, 2]))
