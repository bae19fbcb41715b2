"""CPU checks of the audio front end (asr_fbank_*): exported, frame counts and
feature dimensions, the host tables against a float64 numpy construction from
the semantics in include/asr_amd.h, and the configuration / argument checks
ahead of any HIP call (no GPU here; the fake device pointers are never
dereferenced on the host)."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import scipy.fft

from conftest import asr

NAMES = ["asr_fbank_num_frames", "asr_fbank_feature_dim", "asr_fbank_host_tables", "asr_fbank_create",
         "asr_fbank_destroy", "asr_fbank_workspace_bytes", "asr_fbank_fwd"]
FAKE = 0x10000   # a non-NULL, 16-byte aligned "device pointer"

BASE = dict(sample_rate=16000.0, win_length=400, hop_length=160, n_fft=512, window=asr.FBANK_WIN_HANN,
            preemph=0.97, n_mels=40, f_min=0.0, f_max=8000.0, log_floor=1e-10, n_mfcc=26, n_context=0)
TABLE_CASES = {
    "16k_hann_mfcc": BASE,
    "8k_hamming_mfcc": dict(BASE, sample_rate=8000.0, win_length=200, hop_length=80, n_fft=256,
                            window=asr.FBANK_WIN_HAMMING, n_mels=23, f_max=4000.0, n_mfcc=13),
    "16k_rect_logmel": dict(BASE, win_length=1024, hop_length=256, n_fft=1024, window=asr.FBANK_WIN_RECT,
                            n_mels=80, n_mfcc=0),
}


def config(**kw):
    return asr.FbankConfig(**dict(BASE, **kw))


# ---- the float64 reference tables, from the text of the semantics
def ref_window(kind, win):
    n = np.arange(win, dtype=np.float64)
    if kind == asr.FBANK_WIN_RECT:
        return np.ones(win)
    c = np.cos(2 * np.pi * n / (win - 1))
    return 0.5 - 0.5 * c if kind == asr.FBANK_WIN_HANN else 0.54 - 0.46 * c


def ref_mel(sample_rate, n_fft, n_mels, f_min, f_max):
    """[n_mels, n_fft/2 + 1]: triangles over n_mels + 2 points equally spaced in
    HTK mel, no area normalisation."""
    mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)   # noqa: E731
    pts = np.linspace(mel(np.float64(f_min)), mel(np.float64(f_max)), n_mels + 2)
    hz = 700.0 * (10.0 ** (pts / 2595.0) - 1.0)
    f = np.arange(n_fft // 2 + 1, dtype=np.float64) * sample_rate / n_fft
    lo, c, hi = hz[:-2, None], hz[1:-1, None], hz[2:, None]
    return np.maximum(0.0, np.minimum((f - lo) / (c - lo), (hi - f) / (hi - c)))


def ref_dct(n_mfcc, n_mels):
    k = np.arange(n_mfcc, dtype=np.float64)[:, None]
    m = np.arange(n_mels, dtype=np.float64)[None, :]
    s = np.where(k == 0, np.sqrt(1.0 / n_mels), np.sqrt(2.0 / n_mels))
    return s * np.cos(np.pi * k * (2 * m + 1) / (2.0 * n_mels))


def one_rounding(got, ref):
    """Every fp32 entry is the float64 value rounded once: within half an fp32
    ulp of it (1e-6 of slack for the last bits of the float64 values themselves,
    whose cos / log10 / pow need not round identically in two libraries)."""
    got = np.asarray(got, np.float64)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(got - ref) <= 0.5 * ulp * (1 + 1e-6)), np.abs(got - ref).max()


def host_tables(cfg):
    c = asr.FbankConfig(**cfg)
    D = c.n_mfcc or c.n_mels
    win = np.zeros(c.win_length, np.float32)
    mel = np.zeros((c.n_mels, c.n_fft // 2 + 1), np.float32)
    dct = np.full((D, c.n_mels), np.nan, np.float32)
    rc = asr.lib().asr_fbank_host_tables(ctypes.byref(c), win.ctypes.data, mel.ctypes.data, dct.ctypes.data)
    assert rc == asr.ASR_OK
    return win, mel, dct


def test_symbols_in_mirror_and_library():
    for n in NAMES:
        assert n in asr.EXPORTS, n
        assert hasattr(asr.lib(), n), n
    out = subprocess.run(["nm", "-D", "--defined-only", str(asr.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (asr_[a-z0-9_]+)$", out, flags=re.M))
    assert set(NAMES) <= exported


def test_num_frames():
    c = config()
    nf = lambda n: asr.lib().asr_fbank_num_frames(ctypes.byref(c), n)   # noqa: E731
    win, hop = c.win_length, c.hop_length
    assert nf(win - 1) == 0
    assert nf(win) == 1
    assert nf(win + hop - 1) == 1
    assert nf(win + hop) == 2
    assert nf(0) == 0
    assert asr.lib().asr_fbank_num_frames(ctypes.byref(config(n_fft=384)), 1000) < 0


def test_feature_dim():
    fd = lambda **kw: asr.lib().asr_fbank_feature_dim(ctypes.byref(config(**kw)))   # noqa: E731
    assert fd() == 26
    assert fd(n_context=2) == 26 * 5
    assert fd(n_mfcc=0) == 40
    assert fd(n_mfcc=0, n_context=2) == 40 * 5
    assert fd(n_mels=129) == 0
    assert fd(n_mfcc=0, n_mels=128, n_context=16) == 0   # F = 4224 > 4096


@pytest.mark.parametrize("name", list(TABLE_CASES))
def test_host_tables(name):
    cfg = TABLE_CASES[name]
    win, mel, dct = host_tables(cfg)
    one_rounding(win, ref_window(cfg["window"], cfg["win_length"]))
    rm = ref_mel(cfg["sample_rate"], cfg["n_fft"], cfg["n_mels"], cfg["f_min"], cfg["f_max"])
    one_rounding(mel, rm)
    assert np.array_equal(mel == 0, rm == 0)
    assert np.all((mel != 0).sum(axis=0) <= 2)    # a bin is in at most two filters
    if cfg["n_mfcc"]:
        rd = ref_dct(cfg["n_mfcc"], cfg["n_mels"])
        eye = np.eye(cfg["n_mels"])
        sp = scipy.fft.dct(eye, type=2, norm="ortho", axis=0)[:cfg["n_mfcc"]]   # column m = DCT of unit vector m
        assert np.abs(rd - sp).max() < 1e-14
        one_rounding(dct, rd)
    else:
        assert np.isnan(dct).all()   # not written for a log-mel output


def test_host_tables_null_pointers_and_bad_config():
    c = config()
    L = asr.lib()
    assert L.asr_fbank_host_tables(ctypes.byref(c), None, None, None) == asr.ASR_OK
    assert L.asr_fbank_host_tables(None, None, None, None) == asr.ASR_ERR_ARG
    assert L.asr_fbank_host_tables(ctypes.byref(config(n_fft=384)), None, None, None) == asr.ASR_ERR_UNSUPPORTED


@pytest.mark.parametrize("bad", [dict(n_fft=384), dict(win_length=513), dict(n_mels=129), dict(n_mfcc=41),
                                 dict(n_context=17), dict(f_max=8000.5), dict(log_floor=0.0),
                                 dict(win_length=1), dict(hop_length=0), dict(window=3), dict(preemph=1.0),
                                 dict(sample_rate=0.0), dict(f_min=8000.0)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_create_unsupported(bad):
    """Decided from the configuration alone: no handle, no HIP call (this
    machine has no GPU, so a HIP call would give ASR_ERR_HIP instead)."""
    h = ctypes.c_void_p()
    assert asr.lib().asr_fbank_create(ctypes.byref(config(**bad)), ctypes.byref(h)) == asr.ASR_ERR_UNSUPPORTED
    assert not h.value
    with pytest.raises(asr.AsrError) as e:
        asr.FeatureFrontend(**dict(BASE, **bad))
    assert e.value.status == asr.ASR_ERR_UNSUPPORTED


def test_create_err_arg():
    h = ctypes.c_void_p()
    assert asr.lib().asr_fbank_create(None, ctypes.byref(h)) == asr.ASR_ERR_ARG
    assert asr.lib().asr_fbank_create(ctypes.byref(config()), None) == asr.ASR_ERR_ARG
    assert asr.lib().asr_fbank_destroy(None) == asr.ASR_ERR_ARG
    assert asr.lib().asr_fbank_workspace_bytes(None, 10, 4) == 0


def test_fwd_null_handle_is_err_arg():
    p = FAKE
    assert asr.lib().asr_fbank_fwd(None, p, 2000, None, 3, 2000, p, 26, None, None, 11, None) == asr.ASR_ERR_ARG
