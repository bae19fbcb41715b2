"""The one-wave decoder's frame loop after its instruction diet (DESIGN.md §22,
csrc/ctc_wave_kernel.inc, csrc/ctc_wave_select.h: lazily computed best
state, selection passes on the keys' high words, unguarded absent keys, parent links written by the slot
builders).  Every case decodes with the one-wave kernel (waves =
ASR_CTC_WAVES_LIST) through the C ABI's Python mirror and is held to

  * the workgroup kernel (8 waves, untouched) on the same emissions: the full
    ranked beam, labels equal and fp64 scores bit for bit;
  * the CPU oracle: best labels identical, |dlogp| <= 1e-9 * max(1, |logp|).

The beam capacity is given explicitly (64 slots up to beam 56: one row per
lane), so that a tie overflow is an error here and never a silent re-decode on
another kernel.  Shapes are the smallest that reach each changed path."""
import numpy as np
import pytest

from conftest import asr, cpu_threads, oracle

pytestmark = pytest.mark.gpu
LIST = asr.ASR_CTC_WAVES_LIST
TOL = 1e-9
V0, BEAM0, B0, T0 = 29, 50, 24, 48


def _logsoftmax(x):
    x = x - x.max(axis=2, keepdims=True)
    return (x - np.log(np.exp(x).sum(axis=2, keepdims=True))).astype(np.float32)


def _normal(T, B, V, sigma, seed):
    return _logsoftmax(np.random.default_rng(seed).normal(0.0, sigma, (T, B, V)))


def _cap(beam):
    return 64 if beam <= 56 else 128


def _decode(emis, beam, waves, is_log=True, lengths=None, cap=0):
    dec = asr.CTCDecoder(emis.shape[2], beam, 0, max_states=cap or _cap(beam), waves=waves)
    dec.decode(emis, is_log=is_log, lengths=lengths)
    assert dec.config()[1] == waves
    beams = dec.beams(max_hyps=dec.config()[0])
    lab, lp = dec.best()
    dec.close()
    return beams, lab, lp


def _same_bits(a, b, what):
    assert a[1] == b[1], f"{what}: best labels differ"
    assert np.array_equal(a[2], b[2]), f"{what}: best log-probs differ"
    assert len(a[0]) == len(b[0])
    for u, (x, y) in enumerate(zip(a[0], b[0])):
        assert [l for l, _ in x] == [l for l, _ in y], f"{what}: utterance {u} ranked labels differ"
        assert [s for _, s in x] == [s for _, s in y], f"{what}: utterance {u} ranked scores differ"


def _vs_oracle(got, emis, beam, is_log, what, lengths=None):
    T, B, _ = emis.shape
    if lengths is None:
        ref = [r[0] for r in oracle.decode(emis, beam, 0, is_log=is_log, nthreads=cpu_threads(), max_hyps=1)]
    else:
        ref = [oracle.decode(np.ascontiguousarray(emis[:n, b:b + 1, :]), beam, 0, is_log=is_log, max_hyps=1)[0][0]
               if n else ([], 0.0) for b, n in enumerate(lengths)]
    for b in range(B):
        assert got[1][b] == [int(c) for c in ref[b][0]], f"{what}: utterance {b} best labels vs oracle"
        d = abs(got[2][b] - ref[b][1])
        assert d <= TOL * max(1.0, abs(ref[b][1])), f"{what}: utterance {b} logp off by {d}"


def _check(emis, beam=BEAM0, is_log=True, what="", cap=0):
    wave = _decode(emis, beam, LIST, is_log, cap=cap)
    _same_bits(wave, _decode(emis, beam, 8, is_log, cap=cap), what + " vs workgroup kernel")
    _vs_oracle(wave, emis, beam, is_log, what)
    return wave


@pytest.mark.parametrize("T", [1, 2, 3])
def test_fewer_than_k_candidates(T):
    """Nothing is pruned in the first frames: the best state comes from the
    maximum key, now computed in that branch only."""
    _check(_normal(T, B0, V0, 1.0, 100 + T), what=f"T={T}")


def test_guess_above_the_cutoff():
    """Flat and peaked frames alternate: the floor guessed from the last
    frame's cutoff is wrong on most frames, so the second attempt (every
    label, floor 1) runs."""
    rng = np.random.default_rng(7)
    sig = np.where(np.arange(T0) % 2 == 0, 0.1, 8.0)[:, None, None]
    _check(_logsoftmax(rng.normal(0.0, 1.0, (T0, B0, V0)) * sig), what="alternating")


def test_more_live_labels_than_registered():
    """Flat frames: (nearly) every label is live, so most are `rest` labels
    whose keys are regenerated per pass; 48 frames on the one-row instance
    (RPT = 1)."""
    _check(_normal(T0, B0, V0, 0.2, 11), what="sigma 0.2")


def test_exactly_uniform_emissions():
    """Every label equally likely in every frame: all labels live, and whole
    classes of candidates tie.  At V = 29 and beam 50 the second frame alone
    leaves 1 + 28 + 756 = 785 tied survivors, more than any beam capacity
    (256), so that shape cannot decode past one frame.  What runs: one frame
    at V = 29 on the one-row kernel (RPT = 1: 24 `rest` labels, nothing
    pruned), and six frames at V = 4, beam 3, capacity 128 — the two-row
    instance (RPT = 2) with no `rest` labels, which covers the tie exits of the
    selection only.  Many `rest` labels over many frames on the one-row kernel
    are test_more_live_labels_than_registered's."""
    _check(np.full((1, B0, V0), np.log(1.0 / V0), np.float32), what="uniform V=29 T=1")
    T, B, V, beam = 6, 4, 4, 3
    emis = np.full((T, B, V), 1.0 / V, np.float32)
    ref = oracle.decode(emis, beam, 0, max_hyps=4096)
    got = {}
    for w in (LIST, 8):
        dec = asr.CTCDecoder(V, beam, 0, max_states=128, waves=w)
        dec.decode(emis)
        got[w] = (dec.beams(max_hyps=128), *dec.best())
        dec.close()
    _same_bits(got[LIST], got[8], "uniform V=4")
    for b in range(B):
        assert [l for l, _ in got[LIST][0][b]] == [list(l) for l, _ in ref[b]]
        assert all(abs(x - y) <= TOL * max(1.0, abs(y)) for (_, x), (_, y) in zip(got[LIST][0][b], ref[b]))


@pytest.mark.parametrize("sigma,beam,cap", [(12.0, 50, 256), (8.0, 10, 64)])
def test_quantised_emissions_ties(sigma, beam, cap):
    """Log emissions on a grid of 0.25: every score lies on the grid, so whole
    classes of candidates have equal keys, at the cutoff too in every frame
    (the one-value bin and whole-bin exits of the selection).  The ties at
    beam 50 (up to 96 survivors, by the oracle) need capacity 256, the
    four-rows-per-lane instance (RPT = 4); only beam 10 (up to 40 survivors,
    capacity 64) reaches the one-row instance (RPT = 1) that C4 runs."""
    rng = np.random.default_rng(23)
    emis = (np.round(rng.normal(0.0, sigma, (T0, B0, V0)) * 4.0) / 4.0 - 8.0).astype(np.float32)
    _check(emis, beam=beam, what=f"grid 0.25, beam {beam}", cap=cap)


def test_keys_equal_in_the_high_word():
    """Labels in pairs whose probabilities differ by one fp32 ulp: prefixes
    that differ by such a label score within 2^-30 relative of each other
    once |logp| > 64 — keys equal in the high word that only the 64-bit
    passes below sh = 32 tell apart, all along the beam and at its cutoff."""
    rng = np.random.default_rng(31)
    p = np.exp(_logsoftmax(rng.normal(0.0, 1.0, (T0, B0, V0)))).astype(np.float32)
    p[:, :, 2::2] = np.nextafter(p[:, :, 1::2], np.float32(1.0))
    wave = _check(p, is_log=False, what="ulp pairs")
    assert max(wave[2]) < -64.0
    # the pairs are told apart: some ranked neighbours differ below 2^-30 relative
    near = sum(1 for u in wave[0] for (_, x), (_, y) in zip(u, u[1:]) if 0.0 < x - y <= 2.0 ** -30 * abs(x))
    assert near > 0


@pytest.mark.parametrize("V,beam", [(32, 50), (33, 50), (63, 50), (29, 56), (29, 57)])
def test_mask_and_capacity_edges(V, beam):
    """32-bit child masks up to V = 32, 64-bit from 33 to the last vocabulary
    (63); beam 56 is the last one-row-per-lane shape (RPT = 1, capacity 64) and
    57 the first with two (RPT = 2, capacity 128)."""
    _check(_normal(T0, B0, V, 1.0, 1000 + V + beam), beam=beam, what=f"V={V} beam={beam}")


def test_segments_and_frame_parity():
    """Segments [0, 13), [13, 14), [14, 37): a resumed segment starts on an odd
    and on an even frame; utterances of every length class.  Bit-identical to
    the whole decode, which is the workgroup kernel's and the oracle's."""
    T, cuts = 37, [13, 14]
    lengths = [37, 0, 1, 13, 14, 15, 36, 35, 2, 3, 12, 21, 37, 29, 7, 1, 0, 33, 37, 14, 13, 25, 11, 37]
    assert len(lengths) == B0
    emis = _normal(T, B0, V0, 1.0, 41)
    whole = _decode(emis, BEAM0, LIST, lengths=lengths)
    _same_bits(whole, _decode(emis, BEAM0, 8, lengths=lengths), "whole vs workgroup kernel")
    _vs_oracle(whole, emis, BEAM0, True, "whole", lengths=lengths)
    d_em = asr.DeviceMatrix.from_numpy(emis.reshape(T * B0, V0))
    d = asr.CTCDecoder(V0, BEAM0, 0, max_states=64)
    bounds = [0] + cuts + [T]
    for t0, t1 in zip(bounds, bounds[1:]):
        d.decode_segment(d_em.ptr + 4 * t0 * B0 * V0, T, t0, t1, B0, True, lengths=lengths if t0 == 0 else None)
    assert d.config()[1] == LIST
    seg = (d.beams(max_hyps=d.config()[0]), *d.best())
    d.close()
    _same_bits(seg, whole, "segments vs whole")


@pytest.mark.parametrize("B", [32, 64])
def test_pipeline_decode_cus(B):
    """The pipeline at its default decode-CU count (half of the CUs, or 3/8 on
    the fp32 GEMMs) and at a quarter of them: equal results, and those of the
    same production followed by a plain one-wave decode.  At B = 32 the
    pipeline takes the CU-groups schedule (workgroup decoders, no decode
    partition: the two runs differ in nothing, and the case only pins that
    schedule's results to the one-wave kernel's); B = 64 is the smallest batch
    on the chip-filling schedule, whose one-wave decoders run on the decode
    CUs, and there the two counts differ."""
    T, inp, H, V, beam = 40, 48, 64, 29, 50
    rng = np.random.default_rng(5)
    s = 1 / np.sqrt(H)
    host = [rng.uniform(-s, s, (inp, H)), rng.uniform(-s, s, (H, H)), rng.uniform(-0.1, 0.1, (H, 1)),
            rng.uniform(-0.1, 0.1, (H, 1)), rng.uniform(-4 * s, 4 * s, (H, V)), rng.uniform(-0.5, 0.5, (V, 1))]
    W = [asr.DeviceMatrix.from_numpy(np.asarray(a, np.float32)) for a in host]
    x = asr.DeviceMatrix.from_numpy(rng.uniform(-1, 1, (T * B, inp)).astype(np.float32))
    import torch
    quarter = torch.cuda.get_device_properties(0).multi_processor_count // 4
    outs, fused, counts = [], None, []
    for dcus in (0, quarter):
        p = asr.Pipeline(T, B, inp, H, V, beam, W, decode_cus=dcus)
        d = p.describe()
        counts.append(d["decode_cus"])
        if B >= 64:
            assert d["mode"] == "chip-filling batches" and d["decode_waves"] == LIST, d
        fused = d["fused_emission"] if fused is None else fused
        assert d["fused_emission"] == fused
        for _ in range(2):
            p.submit(x)
        while p.pending():
            lab, ln, lp, _ = p.collect()
            outs.append(([lab[b, :ln[b]].tolist() for b in range(B)], lp.copy()))
        p.close()
    if B >= 64:
        assert counts[1] == quarter and counts[0] > quarter, counts
    em = asr.DeviceMatrix(T * B, V)
    asr.model_emissions(x, W, T, B, em, fused, recurrence=d["recurrence"])
    dec = asr.CTCDecoder(V, beam, 0, waves=LIST)
    dec.decode_device(em.ptr, T, B, is_log=True)
    lab, lp = dec.best()
    dec.close()
    for o in outs:
        assert o[0] == lab and np.array_equal(o[1], lp)
