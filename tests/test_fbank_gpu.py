"""GPU numerics of the audio front end (asr_fbank_fwd / asr.FeatureFrontend).

Reference: features() of fbank_cases.py, float64 numpy written from the semantics in
include/asr_amd.h (np.fft.rfft per frame, the float64 tables of
test_fbank_cpu.py); its STFT piece is cross-checked against torch.stft
(center=False) in float64 at win == n_fft, where the two conventions coincide.
Bound: the project's bound for fp32 kernels, |err| <= 2e-5 (1 + |ref|).  The
same chain in fp32 on the CPU (torch.fft.rfft float32, fp32 tables and sums)
stays within 5.7e-6 (1 + |ref|) on cases a-e with these inputs, so the bound
leaves about 3.5x for another butterfly order.

Inputs: uniform(-0.5, 0.5) noise plus a 440 Hz tone plus a chirp, so that every
mel band is far above log_floor.  Shapes: the smallest at which each part can
go wrong (CASES).
"""
import copy
import functools

import numpy as np
import pytest
import torch

from conftest import asr, oracle
from fbank_cases import (ATOL, SENT, cfg, check_padding, features, features_fp32, num_frames, poisoned, preemphasis,
                         ref_stft, ref_window, run, waves)

pytestmark = pytest.mark.gpu

# name -> (config, B, S, nsamples)
CASES = {
    # zero-pad to n_fft, lengths, a 0-frame utterance, context edges
    "a": (cfg(16000, 400, 160, 512, 40, 26, 1), 3, 2000, (2000, 1200, 399)),
    # log-mel output, direct write
    "b": (cfg(16000, 400, 160, 512, 40, 0, 0), 2, 1500, (1500, 900)),
    # smallest FFT, C close to the frame count
    "c": (cfg(8000, 200, 80, 256, 23, 13, 2), 2, 900, (900, 540)),
    # win == n_fft
    "d": (cfg(16000, 1024, 256, 1024, 80, 0, 0), 1, 5000, None),
    # largest FFT
    "e": (cfg(16000, 400, 160, 2048, 64, 26, 0), 2, 2100, (2100, 1260)),
    # last-frame boundary (400 + 160 k samples exactly / one short), B not a multiple of the waves of a workgroup
    "f": (cfg(16000, 400, 160, 512, 40, 26, 0), 5, 880, (880, 879, 560, 559, 400)),
    # T = 1
    "f1": (cfg(16000, 400, 160, 512, 40, 26, 0), 5, 400, None),
}


def close(got, ref, what=""):
    err = np.abs(np.asarray(got, np.float64) - ref)
    print(f"{what} max err {err.max():.3e} (max err / (1 + |ref|) {(err / (1 + np.abs(ref))).max():.3e})")
    assert np.all(err <= ATOL * (1.0 + np.abs(ref))), f"{what} max err {err.max()}"


@functools.lru_cache(maxsize=None)
def case(name):
    """(config, wave, nsamples, T, reference out, reference frames); unchanged by the tests."""
    c, B, S, ns = CASES[name]
    wave = waves(int(c["sample_rate"]), B, S)
    T = max(1, num_frames(S, c["win_length"], c["hop_length"]))
    ref, frames = features(c, wave, ns, T)
    ref.setflags(write=False)
    return c, wave, ns, T, ref, frames


def test_reference_stft_matches_torch_stft():
    """win == n_fft: torch.stft(center=False) frames and windows as the reference does."""
    c, wave, _, _, _, _ = case("d")
    y = preemphasis(wave[0], c["preemph"])
    X = ref_stft(y, c)
    tw = torch.from_numpy(ref_window(c["window"], c["win_length"]))
    ts = torch.stft(torch.from_numpy(y), c["n_fft"], hop_length=c["hop_length"], win_length=c["win_length"],
                    window=tw, center=False, return_complex=True).numpy().T
    assert ts.shape == X.shape
    assert np.abs(ts - X).max() <= 1e-10 * np.abs(X).max()


@pytest.mark.parametrize("name", list(CASES))
def test_features(name):
    c, wave, ns, T, ref, frames = case(name)
    got, gf = run(c, wave, ns)
    assert np.array_equal(gf, frames)
    assert got.shape == ref.shape
    check_padding(got, frames, c)
    close(got, ref, f"case {name}")


def test_case_shapes_are_what_they_claim():
    assert list(case("a")[5]) == [11, 6, 0]
    assert list(case("c")[5]) == [9, 5]             # 2C + 1 = 5 context frames
    assert list(case("f")[5]) == [4, 3, 2, 1, 1]
    assert case("f1")[3] == 1 and list(case("f1")[5]) == [1] * 5


def test_strides_sentinel_and_poison():
    """ldw > S, ldo > F: columns >= F keep the sentinel; samples in [S, ldw) and in
    [nsamples_b, S) are 1e30 (run() poisons them) and change nothing."""
    c, wave, ns, T, ref, frames = case("a")
    F = ref.shape[2]
    plain, _ = run(c, wave, ns)
    got, gf = run(c, wave, ns, ldw=wave.shape[1] + 37, ldo=F + 5)
    assert np.array_equal(gf, frames)
    assert np.all(got[:, :, F:] == SENT)
    assert np.array_equal(got[:, :, :F].view(np.uint32), plain.view(np.uint32))
    close(got[:, :, :F], ref, "strided")
    # the same utterances with clean samples past each length: the same bits
    full = wave.copy()
    c0 = dict(c)
    fe = asr.FeatureFrontend(**c0)
    out, fr = fe.forward(full, ns)
    asr.synchronize()
    assert np.array_equal(out.toCpu().reshape(T, -1, F).view(np.uint32), plain.view(np.uint32))
    assert np.array_equal(asr.device_int32(fr, len(ns)), frames)
    fe.close()


def test_batch_independent():
    """An utterance's bits depend on the configuration only: a batch of five,
    its first two alone, one of them last in another batch, and a larger T."""
    c = CASES["a"][0]
    S = 2000
    wave = waves(16000, 5, S)
    ns = (2000, 1200, 399, 1777, 800)
    five, f5 = run(c, wave, ns)
    two, f2 = run(c, wave[:2], ns[:2])
    assert np.array_equal(five[:, :2].view(np.uint32), two.view(np.uint32))
    assert np.array_equal(f5[:2], f2)
    other, fo = run(c, wave[[3, 4, 1]], (ns[3], ns[4], ns[1]))
    assert np.array_equal(other[:, 2].view(np.uint32), five[:, 1].view(np.uint32))
    assert np.array_equal(other[:, 0].view(np.uint32), five[:, 3].view(np.uint32))
    T = five.shape[0]
    longer, fl = run(c, wave, ns, T=T + 7)
    assert np.array_equal(longer[:T].view(np.uint32), five.view(np.uint32))
    assert not longer[T:].view(np.uint32).any()
    assert np.array_equal(fl, f5)


@pytest.mark.parametrize("window", ["hamming", "rect"])
def test_window_kinds(window):
    c, wave, ns, T, _, _ = case("c")
    c = dict(c, window=asr.FBANK_WINDOWS[window])
    ref, frames = features(c, wave, ns, T)
    got, gf = run(c, wave, ns)
    assert np.array_equal(gf, frames)
    check_padding(got, frames, c)
    close(got, ref, window)


def test_no_preemphasis():
    c, wave, ns, T, _, _ = case("b")
    c = dict(c, preemph=0.0)
    ref, frames = features(c, wave, ns, T)
    got, gf = run(c, wave, ns)
    assert np.array_equal(gf, frames)
    close(got, ref, "preemph = 0")


def test_frontend_device_pointer_and_null_lengths():
    """FeatureFrontend.forward on a device pointer; nsamples None = S for all."""
    c, wave, _, T, ref, frames = case("d")
    fe = asr.FeatureFrontend(**c)
    dw = asr.DeviceMatrix.from_numpy(wave)
    out, fr = fe.forward(dw.ptr, B=wave.shape[0], S=wave.shape[1])
    asr.synchronize()
    assert (out.rows, out.cols) == (T * wave.shape[0], fe.feature_dim)
    close(out.toCpu().reshape(ref.shape), ref, "device pointer")
    assert np.array_equal(asr.device_int32(fr, wave.shape[0]), frames)
    fe.close()


def test_fwd_err_arg():
    """With a real handle: every argument error is decided before a launch."""
    c, wave, ns, T, ref, _ = case("a")
    B, S = wave.shape
    F = ref.shape[2]
    fe = asr.FeatureFrontend(**c)
    dw, out = asr.DeviceMatrix.from_numpy(wave), asr.DeviceMatrix(T * B, F)
    work = asr.DeviceBytes(fe.workspace_bytes(T, B))
    assert fe.workspace_bytes(T, B) >= T * B * 26 * 4
    L = asr.lib()

    def fwd(h=fe.h, w=dw.ptr, ldw=S, B=B, S=S, o=out.ptr, ldo=F, wk=work.ptr, T=T):
        return L.asr_fbank_fwd(h, w, ldw, None, B, S, o, ldo, None, wk, T, None)

    assert fwd() == asr.ASR_OK
    asr.synchronize()
    for bad in (dict(w=None), dict(o=None), dict(wk=None), dict(B=0), dict(S=0), dict(T=0), dict(ldw=S - 1),
                dict(ldo=F - 1), dict(T=T - 1)):
        assert fwd(**bad) == asr.ASR_ERR_ARG, bad
    fe.close()
    fe0 = asr.FeatureFrontend(**dict(c, n_context=0))
    assert fe0.workspace_bytes(T, B) == 0
    out0 = asr.DeviceMatrix(T * B, 26)
    assert L.asr_fbank_fwd(fe0.h, dw.ptr, S, None, B, S, out0.ptr, 26, None, None, T, None) == asr.ASR_OK
    asr.synchronize()
    fe0.close()


def test_graph_replay():
    """One asr_fbank_fwd (case a: both kernels) captured into a graph and
    replayed once gives the eager call's bits."""
    c, wave, ns, T, ref, frames = case("a")
    B, S = wave.shape
    F = ref.shape[2]
    fe = asr.FeatureFrontend(**c)
    bufs = (asr.DeviceMatrix.from_numpy(poisoned(wave, ns, S)), asr.device_lengths(ns),
            asr.DeviceMatrix.from_numpy(np.full((T * B, F), SENT, np.float32)), asr.DeviceBytes(4 * B),
            asr.DeviceBytes(fe.workspace_bytes(T, B)))
    dw, dn, out, fr, work = bufs

    def call(stream):
        asr.check(asr.lib().asr_fbank_fwd(fe.h, dw.ptr, S, dn.ptr, B, S, out.ptr, F, fr.ptr, work.ptr, T, stream),
                  "asr_fbank_fwd")

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call(s.cuda_stream)   # eager, on the capture stream (also loads the kernels)
    torch.cuda.synchronize()
    eager = (out.toCpu(), asr.device_int32(fr, B))
    close(eager[0].reshape(ref.shape), ref, "eager")
    for m in (out, fr, work):
        asr.check(asr.lib().asr_memset(m.ptr, 0xFF, m.nbytes, None), "asr_memset")
    asr.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(torch.cuda.current_stream().cuda_stream)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.toCpu().view(np.uint32), eager[0].view(np.uint32))
    assert np.array_equal(asr.device_int32(fr, B), eager[1])
    fe.close()


def test_chain_waveform_to_text():
    """wave -> FeatureFrontend -> Linear (ReLU) -> LSTM (bidirectional, H = 32, the
    front end's d_frames as its lengths) -> Linear (log-softmax, V = 29) ->
    CTCDecoder with the same lengths, on case a's audio.

    The decode equals oracle.decode of the emissions the GPU produced (the
    project's parity rule).  The emissions are compared with the float64 CPU
    chain (reference features -> torch.nn in float64): the same chain on the
    CPU in fp32 is E32 away from it, and the GPU must be within 10 x E32 (it
    adds other summation orders in four stages, nothing of a new kind)."""
    c, wave, ns, T, ref, frames = case("a")
    B, F, H1, H, V, beam = wave.shape[0], ref.shape[2], 48, 32, 29, 20
    torch.manual_seed(1234)
    lin1, lstm, lin2 = torch.nn.Linear(F, H1), torch.nn.LSTM(H1, H, 1, bidirectional=True), torch.nn.Linear(2 * H, V)

    def cpu_chain(feats, dtype):
        with torch.no_grad():
            m1, ml, m2 = (copy.deepcopy(m).to(dtype) for m in (lin1, lstm, lin2))
            x = torch.relu(m1(torch.from_numpy(np.array(feats)).to(dtype)))
            hid = torch.zeros(T, B, 2 * H, dtype=dtype)
            for b in range(B):
                if frames[b]:
                    hid[:frames[b], b:b + 1] = ml(x[:frames[b], b:b + 1])[0]
            return torch.log_softmax(m2(hid), dim=-1).numpy()

    em64 = cpu_chain(ref, torch.float64)
    f32, fr32 = features_fp32(c, wave, ns, T)
    assert np.array_equal(fr32, frames)
    em32 = cpu_chain(f32, torch.float32)

    fe = asr.FeatureFrontend(**c)
    feats, dfr = fe.forward(poisoned(wave, ns, wave.shape[1]), ns)
    w = lambda m: m.weight.detach().numpy().T   # noqa: E731
    L1 = asr.Linear(T * B, F, H1, w(lin1), lin1.bias.detach().numpy(), epilogue=asr.EPI_BIAS_RELU)
    L2 = asr.Linear(T * B, 2 * H, V, w(lin2), lin2.bias.detach().numpy(), epilogue=asr.EPI_BIAS_LOGSOFTMAX)
    net = asr.LSTM.from_torch(lstm)
    hid = asr.DeviceMatrix(T * B, 2 * H)
    work = asr.DeviceBytes(asr.lstm_workspace_bytes(T, B, H))
    x = L1.forward(feats)
    for d, (w_ih, w_hh, b_ih, b_hh) in enumerate(net.layers[0]):
        asr.lstm_fwd(x, w_ih, w_hh, b_ih, b_hh, hid, T, B, work, lengths=dfr, reverse=d == 1, col=d * H)
    em = L2.forward(hid)
    asr.synchronize()
    lens = asr.device_int32(dfr, B)
    assert np.array_equal(lens, frames)
    dec = asr.CTCDecoder(V, beam, 0)
    dec.decode_device(em.ptr, T, B, is_log=True, lengths=lens)
    best, lp = dec.best()
    emg = em.toCpu().reshape(T, B, V)
    for b, n in enumerate(lens):
        r = oracle.decode(np.ascontiguousarray(emg[:n, b:b + 1]), beam, 0, is_log=True)[0][0] if n else ([], 0.0)
        assert best[b] == list(r[0]), f"utterance {b}"
        assert abs(lp[b] - r[1]) <= 1e-9 * max(1.0, abs(r[1])), f"utterance {b}"
    dec.close()
    fe.close()

    e32 = np.abs(em32.astype(np.float64) - em64).max()
    eg = np.abs(emg.astype(np.float64) - em64).max()
    print(f"chain emissions: fp32 CPU chain max err {e32:.3e}, GPU max err {eg:.3e}, ratio {eg / e32:.2f}")
    assert eg <= 10 * e32
