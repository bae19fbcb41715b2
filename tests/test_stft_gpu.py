"""GPU numerics of the torch.stft-style front end (asr_stft_fwd), asr_add_pos_fwd
and the WhisperEncoder chain, against the float64 restatements of
stft_reference.py.  A parity case's bound is 4 x the error of the float32
restatement (float32 framing, torch.fft.rfft, mel product and log) against
float64 on the same input: the margin for a direct fp32 sum of length n_fft
against the FFT's log2 n_fft, and for the MFMA's accumulation order."""
import ctypes
import math

import numpy as np
import pytest
import torch

import stft_reference as sr
from conftest import asr

pytestmark = pytest.mark.gpu
SENT = -12345.0
WHISPER = dict(center=1, log="log10", floor_mode="clamp", floor=1e-10, dyn_range=8.0, shift=4.0, scale=0.25, drop_last=1)
PLAIN = dict(center=0, log="ln", floor_mode="add", floor=1e-5, dyn_range=0.0, shift=0.0, scale=1.0, drop_last=0)
VARIANTS = {"whisper": WHISPER, "plain": PLAIN, "centred-ln": {**PLAIN, "center": 1},
            "uncentred-clamp": {**WHISPER, "center": 0}}
SHAPES = [(400, 400, 160, 80), (400, 400, 160, 128), (512, 400, 160, 64), (30, 30, 7, 5)]


def setup(shape, variant, power=2):
    n_fft, win, hop, n_mels = shape
    c = dict(n_fft=n_fft, win=win, hop=hop, power=power, **variant)
    window = asr.stft_window("hann", win).astype(np.float32)
    mel = asr.mel_filter_bank(n_fft // 2 + 1, n_mels, 0.0, 8000.0, 16000.0, "slaney", "slaney").astype(np.float32)
    cfg = asr.stft_config(n_fft, win, hop, c["center"], power, n_mels, c["log"], c["floor_mode"], c["floor"],
                          c["dyn_range"], c["shift"], c["scale"], c["drop_last"])
    return c, window, mel, asr.StftFrontend(cfg, window, mel)


def run(fe, wave, ns, pad_to=0, T=None, ldw=None, ldo=None):
    """asr_stft_fwd on a sentinel-filled output, NaN in the buffer past each n_b: (out [T, B, ldo], frames [B])."""
    B, S = wave.shape
    ldw, ldo = ldw or S + 3, ldo or fe.cfg.n_mels + 3
    buf = np.full((B, ldw), np.nan, np.float32)
    for b, n in enumerate(ns):
        buf[b, :n] = wave[b, :n]
    T = T or max(1, fe.num_frames(pad_to or S))
    dw, dn = asr.DeviceMatrix.from_numpy(buf), asr.device_lengths(ns)
    out, frames = asr.DeviceMatrix.from_numpy(np.full((T * B, ldo), SENT, np.float32)), asr.DeviceBytes(4 * B)
    work = asr.DeviceBytes(max(16, fe.workspace_bytes(T, B)))
    asr.check(asr.lib().asr_stft_fwd(fe.h, dw.ptr, ldw, dn.ptr, B, S, pad_to, out.ptr, ldo, frames.ptr, work.ptr, T,
                                     None), "asr_stft_fwd")
    return out.toCpu().reshape(T, B, ldo), asr.device_int32(frames, B).tolist()


def check(c, window, mel, fe, wave, ns, pad_to, what):
    got, frames = run(fe, wave, ns, pad_to)
    n_mels = mel.shape[0]
    assert np.all(got[:, :, n_mels:] == SENT)
    refs = [sr.stft_mel_ref(c, window, mel, wave[b], n, pad_to) for b, n in enumerate(ns)]
    r32 = [sr.stft_mel_ref(c, window, mel, wave[b], n, pad_to, np.float32) for b, n in enumerate(ns)]
    bound = 4 * max([np.abs(a - b).max() for a, b in zip(r32, refs) if a.size] + [0.0])
    assert frames == [len(r) for r in refs]
    err = 0.0
    for b, ref in enumerate(refs):
        assert not got[len(ref):, b, :n_mels].any()
        if len(ref):
            err = max(err, np.abs(got[:len(ref), b, :n_mels] - ref).max())
    print(f"{what}: kernel err {err:.3e}, float32 restatement err {bound / 4:.3e}")
    assert np.isfinite(err) and err <= bound, (what, err, bound)


@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("shape", SHAPES)
def test_parity(shape, variant, pad):
    """B = 3 ragged: no frame, exactly 64 frames (one tile), 65 frames; white noise, a 0.5 tone + 1e-4 noise (the
    range clamp bites), all zeros (every feature is the clamped floor)."""
    c, window, mel, fe = setup(shape, VARIANTS[variant])
    n_fft, hop, extra = shape[0], shape[2], c["drop_last"]
    n_of = lambda f: (f + extra - 1) * hop + (0 if c["center"] else n_fft)   # noqa: E731
    ns = [n_fft // 2 if c["center"] else n_fft - 1, n_of(64), n_of(65)]
    S = max(ns)
    assert [sr.num_frames(c, n) for n in ns] == [0, 64, 65]
    rng = np.random.default_rng(sum(shape))
    tone = 0.5 * np.sin(2 * np.pi * 0.06 * np.arange(S)) + 1e-4 * rng.standard_normal((3, S))
    for name, wave in (("noise", rng.standard_normal((3, S))), ("tone", tone), ("zeros", np.zeros((3, S)))):
        check(c, window, mel, fe, wave.astype(np.float32), ns, S + 37 if pad else 0, f"{shape} {variant} {name}")


def test_magnitude_db():
    c, window, mel, fe = setup(SHAPES[0], {**PLAIN, "center": 1, "log": "db", "floor_mode": "clamp"}, power=1)
    wave = np.random.default_rng(1).standard_normal((2, 3000)).astype(np.float32)
    check(c, window, mel, fe, wave, [3000, 1777], 0, "magnitude, dB")


def test_whisper_size():
    c, window, mel, fe = setup(SHAPES[0], WHISPER)
    wave = (0.1 * np.random.default_rng(2).standard_normal((2, 32000))).astype(np.float32)
    check(c, window, mel, fe, wave, [32000, 12345], 480000, "30 s")


@pytest.mark.parametrize("variant", ["whisper", "plain"])
def test_bits_do_not_depend_on_the_batch(variant):
    """Alone, tight T, the 16-byte stores (ldo = n_mels) against row 2 of a batch of 3 with a larger T and an odd ldo."""
    c, window, mel, fe = setup(SHAPES[0], VARIANTS[variant])
    wave = np.random.default_rng(3).standard_normal((3, 12000)).astype(np.float32)
    ns = [12000, 5000, 11111]
    alone, f1 = run(fe, wave[2:, :11111], ns[2:], ldw=11111, ldo=80)
    batch, f3 = run(fe, wave, ns, T=90, ldo=91)
    assert f1[0] == f3[2] > 64 and np.array_equal(alone[:, 0, :80], batch[:f1[0], 2, :80])


@pytest.mark.parametrize("N", [5, 64])
def test_add_pos(N):
    """In place, ragged lengths.  Bound 1.5e-6: erfcf within 4 ulp of a GELU below 3 in size (9.5e-7), the product
    and the sum one rounding each of values below 4 (2 x 2.4e-7)."""
    T, B, ln = 7, 3, (7, 0, 4)
    rng = np.random.default_rng(N)
    x, pos = rng.uniform(-3, 3, (T, B, N)).astype(np.float32), rng.uniform(-1, 1, (T + 2, N)).astype(np.float32)
    gelu = np.vectorize(lambda v: 0.5 * v * (1 + math.erf(v / math.sqrt(2))))
    for act in (None, "gelu"):
        d = asr.DeviceMatrix.from_numpy(x.reshape(T * B, N))
        asr.add_pos_fwd(d, asr.DeviceMatrix.from_numpy(pos), d, T, B, N, act, asr.device_lengths(ln))
        got = d.toCpu().reshape(T, B, N)
        ref = (gelu(x.astype(np.float64)) if act else x.astype(np.float64)) + pos[:T, None, :]
        for b, n in enumerate(ln):
            assert not got[n:, b].any() and np.all(np.abs(got[:n, b] - ref[:n, b]) <= 1.5e-6)


def test_whisper_encoder_chain():
    """WhisperEncoder.from_transformers on the stand-in's weights, one shorter utterance, at the tolerance of the
    Conformer and wav2vec 2.0 layer tests (2e-5 (1 + |ref|))."""
    torch.manual_seed(0)
    m = sr.StandInEncoder(80, 64, 2, 96, 2, 24).double().eval()
    T, B, ln = 48, 2, (48, 31)
    feats = np.random.default_rng(4).uniform(-1, 1, (T, B, 80)).astype(np.float32)
    enc = asr.WhisperEncoder.from_transformers(m)
    got = enc.forward(asr.DeviceMatrix.from_numpy(feats.reshape(T * B, 80)), T, B, ln).toCpu().reshape(24, B, 64)
    assert asr.device_int32(enc.out_lengths, B).tolist() == [24, 16]
    for b, n in enumerate(ln):
        with torch.no_grad():
            ref = m(torch.from_numpy(feats[:n, b].T.astype(np.float64))[None])[0].numpy()
        assert not got[len(ref):, b].any() and np.all(np.abs(got[:len(ref), b] - ref) <= 2e-5 * (1 + np.abs(ref)))
