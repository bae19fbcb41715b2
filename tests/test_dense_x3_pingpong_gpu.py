"""The two-phase schedule of the K <= 256 split-bf16 GEMM (csrc/dense_x3.hip,
gemm_x3_kernel<.., PP = true>, the default) against the one-phase loop
(ASR_X3G_PINGPONG=0, read at each launch), bit for bit.

The two halves of the workgroup run half a tile apart (one in its MFMAs, the
other storing C, splitting and staging a coming A tile, loading a later one);
column ownership, chunk order, product order and accumulators are the
one-phase loop's, so every output element goes through the same MFMA sequence
and the raw float32 must be equal.  The shapes walk the schedule's edges: one
partial tile, one and two tiles, an odd tile count, NCH = 1 / 2 / 4 / 8, a
half of the workgroup that owns no columns, persistent workgroups with
unequal tile counts, a second (partial) column block, and the fused
production's fragment-major epilogue on persistent and on short workgroups.
"""
import numpy as np
import pytest

from conftest import asr

pytestmark = pytest.mark.gpu


def dm(a):
    return asr.DeviceMatrix.from_numpy(np.asarray(a, np.float32))


CASES = [
    (5, 256, 256),      # one partial tile
    (16, 256, 256),     # one full tile
    (17, 256, 256),     # two tiles, second partial
    (48, 96, 200),      # three tiles; NCH = 4 with zero-padded k; partial last column wave
    (64, 32, 64),       # NCH = 1; only waves 0-1 own columns, so half 1 has none
    (4144, 64, 256),    # 259 tiles: persistent workgroups with unequal tile counts
    (4112, 256, 300),   # two column blocks, second partial; unequal tile counts
]


@pytest.mark.parametrize("M,K,N", CASES)
def test_linear_fwd_same_bits_as_one_phase(M, K, N, monkeypatch):
    assert asr.get_dense_arith() == asr.DENSE_SPLIT_BF16
    rng = np.random.default_rng(1000 * M + K + N)
    x = dm(rng.uniform(-1, 1, (M, K)))
    W = dm(rng.uniform(-1, 1, (K, N)) / np.sqrt(K))
    b = dm(rng.uniform(-0.5, 0.5, (N, 1)))
    for epi in (asr.EPI_NONE, asr.EPI_BIAS, asr.EPI_BIAS_RELU):
        out = {}
        for pp in ("1", "0"):
            monkeypatch.setenv("ASR_X3G_PINGPONG", pp)
            y = dm(np.full((M, N), np.nan))   # an element not written stays NaN: never equal
            asr.linear_fwd(x, W, b if epi != asr.EPI_NONE else None, y, epi)
            out[pp] = y.toCpu()
        monkeypatch.delenv("ASR_X3G_PINGPONG")
        y = dm(np.full((M, N), np.nan))
        asr.linear_fwd(x, W, b if epi != asr.EPI_NONE else None, y, epi)
        assert not np.isnan(out["0"]).any(), epi
        assert np.array_equal(out["1"], out["0"]), epi
        assert np.array_equal(y.toCpu(), out["0"]), epi   # unset: the two-phase default


def _weights(inp, H, V, seed):
    rng = np.random.default_rng(seed)
    s = 1 / np.sqrt(H)
    host = [rng.uniform(-s, s, (inp, H)), rng.uniform(-s, s, (H, H)), rng.uniform(-0.1, 0.1, (H, 1)),
            rng.uniform(-0.1, 0.1, (H, 1)), rng.uniform(-4 * s, 4 * s, (H, V)), rng.uniform(-0.5, 0.5, (V, 1))]
    return [dm(a) for a in host]


def _emissions(x, W, T, B, inp, H, V, beam):
    p = asr.Pipeline(T, B, inp, H, V, beam, W, segments=2)
    d = p.describe()
    assert d["mode"] == "chip-filling batches" and d["fused_emission"] and d["segments"] == 2, d
    p.submit(x)
    p.collect()
    e = p.peek_emissions()
    p.close()
    return e, d


@pytest.mark.parametrize("gsplit", [None, "0.3"])
def test_fused_production_same_bits_as_one_phase(gsplit, monkeypatch):
    """The fragment-major epilogue in the pipeline's fused production: two
    T-segments of 3 x 304 rows = 57 tiles each (odd), the projection on
    persistent workgroups, and with ASR_PIPELINE_GSPLIT=0.3 part of it on
    short workgroups (tpw > 0)."""
    T, B, inp, H, V, beam = 6, 304, 64, 256, 29, 10
    if gsplit is not None:
        monkeypatch.setenv("ASR_PIPELINE_GSPLIT", gsplit)
    W = _weights(inp, H, V, seed=23)
    x = dm(np.random.default_rng(23).uniform(-1, 1, (T * B, inp)))
    monkeypatch.setenv("ASR_X3G_PINGPONG", "0")
    ref, dref = _emissions(x, W, T, B, inp, H, V, beam)
    monkeypatch.delenv("ASR_X3G_PINGPONG")
    got, d = _emissions(x, W, T, B, inp, H, V, beam)
    if gsplit is not None:
        assert d["decode_cu_gemm_rows"] > 0, d
    assert d["decode_cu_gemm_rows"] == dref["decode_cu_gemm_rows"], (d, dref)
    assert np.isfinite(ref).all()
    assert np.array_equal(got, ref)
