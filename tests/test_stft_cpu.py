"""CPU checks of the torch.stft-style front end and the Whisper encoder: the
float64 restatements against transformers' WhisperFeatureExtractor and
WhisperEncoder, the host tables, the frame counts, the basis and the refusals
(every call is refused before any HIP call)."""
import ctypes

import numpy as np
import pytest
import torch

import stft_reference as sr
from conftest import asr

WHISPER = dict(n_fft=400, win=400, hop=160, center=1, power=2, log="log10", floor_mode="clamp", floor=1e-10,
               dyn_range=8.0, shift=4.0, scale=0.25, drop_last=1)


@pytest.mark.parametrize("n_mels", [80, 128])
def test_reference_is_the_whisper_extractor(n_mels):
    """Against the extractor's float64 numpy path (with torch installed its __call__ takes the float32 torch.stft
    path, which is 5e-6 from both).  Bound 2.5e-7: that path keeps the spectrum in complex64 (1.2e-7 relative on the
    power: 1.3e-8 after log10 and / 4) and the log-mel in float32, two roundings of a value below 2 (1.2e-7 each)."""
    tf = pytest.importorskip("transformers")
    fe = tf.WhisperFeatureExtractor(feature_size=n_mels)
    rng = np.random.default_rng(n_mels)
    waves = [rng.standard_normal(n).astype(np.float32) * 0.1 for n in (32000, 12345)]
    batch = np.zeros((2, fe.n_samples), np.float32)
    for b, w in enumerate(waves):
        batch[b, :len(w)] = w
    want = fe._np_extract_fbank_features(batch, "cpu")
    mel = asr.mel_filter_bank(201, n_mels, 0.0, 8000.0, 16000.0, "slaney", "slaney")
    assert np.abs(mel - np.asarray(fe.mel_filters, np.float64).T).max() <= 1e-12
    for w, f in zip(waves, want):
        got = sr.stft_mel_ref(WHISPER, asr.stft_window("hann", 400), mel, w, len(w), pad_to=fe.n_samples)
        assert got.shape == (3000, n_mels) and np.abs(got - f.T).max() <= 2.5e-7


def test_standin_is_the_whisper_encoder():
    tf = pytest.importorskip("transformers")
    torch.manual_seed(0)
    cfg = tf.WhisperConfig(d_model=64, encoder_layers=2, encoder_attention_heads=2, encoder_ffn_dim=96,
                           num_mel_bins=80, max_source_positions=24, decoder_layers=1, decoder_attention_heads=2,
                           decoder_ffn_dim=64, vocab_size=60, pad_token_id=0, bos_token_id=1, eos_token_id=2,
                           decoder_start_token_id=1)
    enc = tf.models.whisper.modeling_whisper.WhisperEncoder(cfg).double().eval()
    mine = sr.StandInEncoder(80, 64, 2, 96, 2, 24).double()
    mine.load_state_dict(enc.state_dict())
    x = torch.randn(2, 80, 48, dtype=torch.float64)
    with torch.no_grad():
        assert (mine(x) - enc(x).last_hidden_state).abs().max() <= 1e-12


def test_window_against_the_extractor():
    au = pytest.importorskip("transformers.audio_utils")
    for kind in ("hann", "hamming"):
        assert np.abs(asr.stft_window(kind, 400) - au.window_function(400, kind)).max() <= 1e-12
        assert np.abs(asr.stft_window(kind, 25, False) - au.window_function(25, kind, periodic=False)).max() <= 1e-12
    htk = asr.mel_filter_bank(257, 40, 20.0, 7600.0, 16000.0)
    assert np.abs(htk - au.mel_filter_bank(257, 40, 20.0, 7600.0, 16000, None, "htk").T).max() <= 1e-12


def test_num_frames_edges():
    for center, drop, cases in ((1, 0, {200: 0, 201: 2, 319: 2, 320: 3}), (1, 1, {200: 0, 201: 1, 480000: 3000}),
                                (0, 0, {399: 0, 400: 1, 559: 1, 560: 2}), (0, 1, {400: 0, 560: 1})):
        c = asr.stft_config(400, 400, 160, center, drop_last=drop)
        for n, want in cases.items():
            assert asr.stft_num_frames(c, n) == want == sr.num_frames(dict(n_fft=400, hop=160, center=center,
                                                                           drop_last=drop), n), (center, drop, n)
    assert asr.stft_num_frames(asr.stft_config(15), 100) < 0 and asr.stft_num_frames(asr.stft_config(400), -1) < 0


@pytest.mark.parametrize("n_fft,win", [(400, 400), (512, 400), (30, 30), (31, 8)])
def test_host_basis_against_float64(n_fft, win):
    w = np.random.default_rng(n_fft).uniform(0.1, 1, win).astype(np.float32)
    G = asr.stft_host_basis(asr.stft_config(n_fft, win, 7), w)
    NB, NBp, left = n_fft // 2 + 1, G.shape[1] // 2, (n_fft - win) // 2
    wp = np.zeros(n_fft)
    wp[left:left + win] = w
    ang = 2 * np.pi * np.outer(np.arange(n_fft), np.arange(NB)) / n_fft
    assert NBp % 16 == 0 and not G[:, NB:NBp].any() and not G[:, NBp + NB:].any()
    # one rounding to fp32 of a value below 1, and cos / sin of the unreduced float64 argument (up to 2 pi 500: 4e-13)
    assert np.abs(G[:, :NB] - wp[:, None] * np.cos(ang)).max() <= 6e-8 + 1e-12
    assert np.abs(G[:, NBp:NBp + NB] + wp[:, None] * np.sin(ang)).max() <= 6e-8 + 1e-12


def test_refusals():
    L, p = asr.lib(), ctypes.c_void_p(64)
    assert all(n in asr.EXPORTS for n in ("asr_stft_create", "asr_stft_fwd", "asr_add_pos_fwd", "asr_stft_host_basis"))
    good = asr.stft_config(400, 400, 160, n_mels=80, log="log10")
    h = ctypes.c_void_p()
    assert L.asr_stft_create(None, p, p, ctypes.byref(h)) == asr.ASR_ERR_ARG
    assert L.asr_stft_create(ctypes.byref(good), None, p, ctypes.byref(h)) == asr.ASR_ERR_ARG
    bad = [dict(n_fft=15), dict(n_fft=1025), dict(win_length=401), dict(win_length=1), dict(hop_length=0),
           dict(hop_length=401), dict(power=3), dict(n_mels=0), dict(n_mels=129), dict(log=4), dict(floor=0.0),
           dict(floor_mode=2), dict(dyn_range=-1.0), dict(scale=float("nan")), dict(n_fft=1024, win_length=1024,
                                                                                     hop_length=1024)]
    for kw in bad:       # the last: 63 hops + n_fft samples do not fit in LDS
        c = asr.stft_config(**{**dict(n_fft=400, win_length=400, hop_length=160, log="log10"), **kw})
        assert L.asr_stft_create(ctypes.byref(c), p, p, ctypes.byref(h)) == asr.ASR_ERR_UNSUPPORTED, kw
    assert L.asr_stft_host_basis(ctypes.byref(good), None, p) == asr.ASR_ERR_ARG
    assert L.asr_stft_fwd(None, p, 2000, None, 3, 2000, 0, p, 80, None, None, 13, None) == asr.ASR_ERR_ARG
    assert L.asr_stft_destroy(None) == asr.ASR_ERR_ARG and L.asr_stft_workspace_bytes(None, 5, 5) == 0
    for args in ((None, 8, p, 8, None, p, 8, 4, 2, 8, 0), (p, 8, p, 8, None, p, 8, 0, 2, 8, 0),
                 (p, 7, p, 8, None, p, 8, 4, 2, 8, 0), (p, 8, p, 8, None, p, 8, 4, 2, 8, 2)):
        assert L.asr_add_pos_fwd(*args, None) == asr.ASR_ERR_ARG, args
    assert L.asr_add_pos_fwd(p, 8, p, 8, None, p, 8, 1 << 20, 1 << 12, 8, 1, None) == asr.ASR_ERR_UNSUPPORTED
