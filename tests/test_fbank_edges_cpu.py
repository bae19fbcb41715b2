"""CPU side of the front end's edge cases (fbank_cases.EDGE_CASES): the host
tables of every new configuration against float64, and the conditions each
case must meet on the references alone before tests/test_fbank_edges_gpu.py
compares the kernel with them: a case that stops reaching its path fails
here.  No GPU: asr_fbank_host_tables is host code and both references run on
the CPU.
"""
import numpy as np
import pytest

import fbank_cases as fc
from test_fbank_cpu import host_tables, one_rounding, ref_dct, ref_mel, ref_window

# the distinct configurations of the cases and of their log-mel twins, by table content
TABLE_KEYS = ("sample_rate", "win_length", "n_fft", "window", "n_mels", "f_min", "f_max", "n_mfcc")
CONFIGS = {}
for _name, _ec in fc.EDGE_CASES.items():
    CONFIGS.setdefault(tuple(_ec.config[k] for k in TABLE_KEYS), (_name, _ec.config))


@pytest.mark.parametrize("name", [n for n, _ in CONFIGS.values()])
def test_host_tables(name):
    cfg = fc.EDGE_CASES[name].config
    win, mel, dct = host_tables(cfg)
    one_rounding(win, ref_window(cfg["window"], cfg["win_length"]))
    rm = ref_mel(cfg["sample_rate"], cfg["n_fft"], cfg["n_mels"], cfg["f_min"], cfg["f_max"])
    one_rounding(mel, rm)
    assert np.array_equal(mel == 0, rm == 0)
    assert np.all((mel != 0).sum(axis=0) <= 2)    # a bin is in at most two filters
    if cfg["n_mfcc"]:
        one_rounding(dct, ref_dct(cfg["n_mfcc"], cfg["n_mels"]))
    else:
        assert np.isnan(dct).all()   # not written for a log-mel output


def test_every_case_has_its_frame_counts():
    assert set(fc.EDGE_FRAMES) == set(fc.EDGE_CASES)
    for name in fc.EDGE_CASES:
        assert list(fc.edge(name).frames) == fc.EDGE_FRAMES[name], name


def test_blocks_cases_span_blocks():
    """Frames past the 64th: a second (and third) workgroup per utterance, and an
    utterance that ends on each side of a block boundary."""
    f = fc.EDGE_FRAMES
    W = fc.FRAMES_PER_WG
    assert f["blocks-512"] == [2 * W + 12, 2 * W + 1, W + 1, W, 0]
    assert fc.edge("blocks-512").T == 2 * W + 12 and fc.edge("blocks-512").c["n_context"] == 1
    assert fc.edge("blocks-2048").c["n_fft"] == 2048 and f["blocks-2048"] == [W + 6, W + 1]
    assert f["win2"][0] == W + 1
    for name in ("shift-p97", "shift-p0"):
        d = fc.edge(name)
        assert d.frames[0] >= 2 * W + 2 and fc.SHIFTS == (1, W - 1, W, W + 1)
        # row i is row 0 advanced by k hop samples
        for i, k in enumerate(fc.SHIFTS):
            n = d.ns[1 + i]
            assert n == fc.S_LONG - k * fc.HOP
            assert np.array_equal(d.wave[1 + i, :n], d.wave[0, k * fc.HOP:])
    assert fc.edge("shift-p0").c["preemph"] == 0.0 and fc.edge("shift-p97").c["preemph"] > 0.9


def test_reference_shift_rows_agree():
    """The property the GPU test asserts as bits holds in the float64 reference:
    rows t >= 1 of the copy advanced by k frames are rows t + k of the whole
    waveform, and row 0 too without pre-emphasis."""
    for name, first in (("shift-p97", 1), ("shift-p0", 0)):
        d = fc.edge(name)
        for i, k in enumerate(fc.SHIFTS):
            n = d.frames[1 + i]
            assert n == d.frames[0] - k
            assert np.array_equal(d.ref[first:n, 1 + i], d.ref[first + k:n + k, 0]), (name, k)
    # x[-1] = 0 at an utterance's start changes frame 0's first sample only (the Hann window's w[0] = 0 hides it
    # from the features, so the pre-emphasised samples are compared)
    d = fc.edge("shift-p97")
    assert fc.preemphasis(d.wave[1], 0.97)[0] != fc.preemphasis(d.wave[0], 0.97)[fc.HOP]


def test_floor_cases_reach_the_floor():
    for name in ("floor-logmel", "floor-mfcc"):
        d = fc.edge(name)
        assert fc.floor_share(name, 0) == 1.0                     # silence: every band at the floor
        assert 0.2 <= fc.floor_share(name, 1) <= 0.8              # the gap
        assert 0.2 <= fc.floor_share(name, 2) <= 0.8              # energies around the floor
        assert fc.floor_share(name, 3) == 0.0
        # frames wholly inside the gap are at the floor, their neighbours are not
        fl = np.log(d.c["log_floor"])
        win, hop = d.c["win_length"], d.c["hop_length"]
        inside = [t for t in range(d.frames[1]) if fc.GAP[0] + 1 <= t * hop and t * hop + win <= fc.GAP[1]]
        assert len(inside) >= 3
        for t in range(d.frames[1]):
            assert np.all(d.logmel[t, 1] == fl) == (t in inside), t
        assert inside[0] > 0 and inside[-1] < d.frames[1] - 1
        # row 2 straddles within frames, not only between them
        at = d.logmel[:, 2] == fl
        assert np.any(at.any(axis=1) & ~at.all(axis=1))
        # int16 scale: integers, several thousand
        assert np.array_equal(d.wave[3], np.round(d.wave[3])) and 8000 < np.abs(d.wave[3]).max() < 32768
        assert not d.wave[0].any()
    for name in ("floor1-logmel", "floor1-mfcc"):
        d = fc.edge(name)
        assert d.c["log_floor"] == 1.0 and 3e-3 < np.abs(d.wave).mean() < 0.5
        assert 0.2 <= fc.floor_share(name) <= 0.8
    assert np.isfinite(fc.edge("floor-mfcc").ref).all()


def test_mel_layout_cases_reach_their_paths():
    e = {n: fc.edge(n).c for n in fc.EDGE_CASES}
    dims = lambda c: c["n_mels"] * (c["n_mfcc"] or c["n_mels"])   # noqa: E731
    # the DCT matrix against the kernel's LDS limit of 4096 floats
    assert dims(e["m128-d40"]) == 5120 and e["m128-d40"]["n_mfcc"]
    assert dims(e["m128-d32"]) == 4096 and e["m128-d32"]["n_mfcc"]
    assert dims(e["m128-8k"]) == 16384 and e["m128-8k"]["n_mfcc"] == 128    # D > 64: the lanes' second trip
    for n in ("blocks-512", "floor-mfcc", "band", "hop-gt-win", "win401"):
        assert e[n]["n_mfcc"] and dims(e[n]) < 4096
    # filters without an FFT bin
    assert fc.empty_filters(e["m128-d40"]) >= 1
    assert fc.empty_filters(e["m128-d32"]) >= 1
    assert fc.empty_filters(e["m128-8k"]) == 6
    for n in ("m128-2048", "m1-2048", "m64", "m65", "band"):
        assert fc.empty_filters(e[n]) == 0
    # an empty filter's energy is the floor in every frame
    d = fc.edge("m128-8k")
    empty = ~fc.host_tables(d.c)[1].any(axis=1)
    assert np.all(d.logmel[:, :, empty] == np.log(d.c["log_floor"]))
    assert (e["m64"]["n_mels"], e["m65"]["n_mels"], e["m1-2048"]["n_mels"], e["m128-2048"]["n_mels"]) == (64, 65, 1, 128)
    # bins in no filter: below f_min and above f_max
    mel = fc.host_tables(e["band"])[1]
    unused = ~mel.any(axis=0)
    assert unused[:9].all() and unused[-19:].all() and not unused[12:100].any()


def test_framing_and_signal_cases_are_what_they_claim():
    e = {n: fc.edge(n) for n in ("hop-gt-win", "hop1-rect", "win401", "win2", "dc", "tone-p97", "tone-p0")}
    c = e["hop-gt-win"].c
    assert c["hop_length"] > c["win_length"]
    c = e["hop1-rect"].c
    assert (c["hop_length"], c["win_length"], c["n_fft"], c["window"]) == (1, 256, 256, fc.asr.FBANK_WIN_RECT)
    assert e["win401"].c["win_length"] % 2 == 1
    c = e["win2"].c
    assert (c["hop_length"], c["win_length"], c["window"]) == (1, 2, fc.asr.FBANK_WIN_RECT)
    assert e["dc"].c["preemph"] == 0.0 and abs(e["dc"].wave.mean() - 0.25) < 1e-3 and e["dc"].wave.std() < 5e-3
    for n in ("tone-p97", "tone-p0"):
        w = e[n].wave
        assert np.array_equal(w, np.round(w)) and 16380 <= np.abs(w).max() <= 16386
        # the spread of band energies within a frame: above 1e6
        spread = e[n].logmel[:e[n].frames[0], 0].max(axis=1) - e[n].logmel[:e[n].frames[0], 0].min(axis=1)
        assert spread.min() > np.log(1e6)


@pytest.mark.parametrize("name", list(fc.EDGE_CASES))
def test_fp32_chain_error(name):
    """The fp32 CPU chain's own error against float64 on each case's input, in
    the case's metric.  Where a case is marked fixed it stays within ATOL / ROOM
    = 5.7e-6, so the GPU test's bound is ATOL itself; elsewhere the bound is
    ROOM times this figure, computed on the same input at run time."""
    d = fc.edge(name)
    assert np.isfinite(d.ref).all() and np.isfinite(d.ref32).all()
    assert np.all(d.scale >= np.abs(d.ref) * (1 - 1e-12))    # the DCT sum's size is at least |c_k|
    e = fc.e32(name)
    line = f"case {name}: fp32 CPU chain max err / (1 + scale) {e:.3e}, bound {fc.bound(name):.3e}"
    if d.c["n_mfcc"]:
        line += f"; log-mel twin {fc.e32(name, True):.3e}, bound {fc.bound(name, True):.3e}"
    print(line)
    if fc.EDGE_CASES[name].fixed:
        assert e <= fc.E32_FIXED
        assert fc.bound(name) == fc.ATOL
