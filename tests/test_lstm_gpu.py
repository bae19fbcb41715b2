"""GPU numerics of the LSTM layer (asr_lstm_fwd / asr_lstm_recur_fwd / asr.LSTM).

Reference: torch.nn.LSTM on the CPU in float64 with the same weights.  Bound:
the project's bound for fp32 kernels (test_dense_gpu.py close(), ATOL = 2e-5):
|err| <= 2e-5 * (1 + |ref|) on h, h_T and c_T.  torch's own fp32 LSTM sits
5e-8 .. 3.2e-7 from the fp64 result at these shapes, so the bound leaves the
summation order and the device's exp / tanh about 60x.

Shapes (T, B, in, H): 16 <= H <= 128 is the one-launch resident kernel (one
wave per 16 hidden columns, 16 utterances per workgroup), H > 128 the
per-frame step kernel.
"""
import copy
import functools

import numpy as np
import pytest
import torch

from conftest import asr

pytestmark = pytest.mark.gpu
ATOL = 2e-5

SHAPES = [(7, 5, 16, 16),      # one wave, partial row tile
          (9, 16, 24, 48),     # exactly one full row tile, odd tile count
          (6, 33, 8, 80),      # two full row tiles plus one row
          (12, 50, 40, 128),   # the resident maximum
          (5, 3, 8, 144),      # the smallest step-form H
          (6, 20, 24, 256),    # step form
          (4, 17, 32, 512),
          (3, 16, 16, 1024)]


def dm(a):
    return asr.DeviceMatrix.from_numpy(np.asarray(a, np.float32))


def close(got, ref, what=""):
    ref = np.asarray(ref, np.float64)
    err = np.abs(np.asarray(got, np.float64) - ref)
    print(f"{what} max err {err.max():.3e} (max err / (1 + |ref|) {(err / (1 + np.abs(ref))).max():.3e})")
    assert np.all(err <= ATOL * (1.0 + np.abs(ref))), f"{what} max err {err.max()}"


@functools.lru_cache(maxsize=None)
def params(T, B, I, H, seed=0):
    """Inputs as test_rnn_forward draws them; two directions' weights."""
    rng = np.random.default_rng(1000 * H + 10 * B + T + seed)
    s = 1 / np.sqrt(H)
    p = {"x": rng.uniform(-1, 1, (T * B, I)).astype(np.float32),
         "h0": rng.uniform(-1, 1, (2, B, H)).astype(np.float32),
         "c0": rng.uniform(-1, 1, (2, B, H)).astype(np.float32)}
    for d in range(2):
        p[d] = (rng.uniform(-s, s, (I, 4 * H)).astype(np.float32), rng.uniform(-s, s, (H, 4 * H)).astype(np.float32),
                rng.uniform(-0.1, 0.1, 4 * H).astype(np.float32), rng.uniform(-0.1, 0.1, 4 * H).astype(np.float32))
    return p


@functools.lru_cache(maxsize=None)
def reference(T, B, I, H, use0, lengths=None):
    """torch.nn.LSTM(bidirectional=True) in float64: (out [T, B, 2H], h_n [2, B, H],
    c_n [2, B, H]); lengths (a tuple) through pack_padded_sequence."""
    p = params(T, B, I, H)
    m = torch.nn.LSTM(I, H, 1, bidirectional=True).double()
    with torch.no_grad():
        for d, sfx in enumerate(("", "_reverse")):
            getattr(m, "weight_ih_l0" + sfx).copy_(torch.from_numpy(p[d][0].T.astype(np.float64)))
            getattr(m, "weight_hh_l0" + sfx).copy_(torch.from_numpy(p[d][1].T.astype(np.float64)))
            getattr(m, "bias_ih_l0" + sfx).copy_(torch.from_numpy(p[d][2].astype(np.float64)))
            getattr(m, "bias_hh_l0" + sfx).copy_(torch.from_numpy(p[d][3].astype(np.float64)))
        x = torch.from_numpy(p["x"].reshape(T, B, I).astype(np.float64))
        st = (torch.from_numpy(p["h0"].astype(np.float64)), torch.from_numpy(p["c0"].astype(np.float64))) if use0 else None
        if lengths is None:
            out, (hn, cn) = m(x, st)
        else:
            pk = torch.nn.utils.rnn.pack_padded_sequence(x, torch.tensor(lengths), enforce_sorted=False)
            out, (hn, cn) = m(pk, st)
            out, _ = torch.nn.utils.rnn.pad_packed_sequence(out, total_length=T)
    return out.numpy(), hn.numpy(), cn.numpy()


def run(T, B, I, H, d, use0, lengths=None, out=None, recur_only=False, stream=0, work=None):
    """Direction d (0 forward, 1 reverse) of the layer on the device into columns
    [d*H', ...) of out (default: an [T*B, H] buffer); returns (out, h_T, c_T) arrays."""
    p = params(T, B, I, H)
    W = [dm(p[d][0]), dm(p[d][1]), dm(p[d][2].reshape(-1, 1)), dm(p[d][3].reshape(-1, 1))]
    h0 = dm(p["h0"][d]) if use0 else None
    c0 = dm(p["c0"][d]) if use0 else None
    hid = out if out is not None else asr.DeviceMatrix(T * B, H)
    col = d * H if hid.cols == 2 * H else 0
    hT, cT = asr.DeviceMatrix(B, H), asr.DeviceMatrix(B, H)
    work = work or asr.DeviceBytes(asr.lstm_workspace_bytes(T, B, H))
    ln = None if lengths is None else asr.device_lengths(lengths)
    if recur_only:
        P = asr.DeviceMatrix(T * B, 4 * H)
        asr.linear_fwd(dm(p["x"]), W[0], None, P, asr.EPI_NONE, stream)
        asr.lstm_recur_fwd(P, W[1], W[2], W[3], hid, T, B, work, h0=h0, c0=c0, hT=hT, cT=cT, lengths=ln,
                           reverse=d == 1, col=col, stream=stream)
    else:
        asr.lstm_fwd(dm(p["x"]), *W, hid, T, B, work, h0=h0, c0=c0, hT=hT, cT=cT, lengths=ln, reverse=d == 1,
                     col=col, stream=stream)
    asr.synchronize()
    return hid.toCpu(), hT.toCpu(), cT.toCpu()


def draw_lengths(T, B):
    ln = np.random.default_rng(T * B).integers(1, T + 1, B)
    ln[1], ln[B - 2] = 1, T    # one utterance of length 1, one of length T
    return tuple(int(v) for v in ln)


@pytest.mark.parametrize("use0", [False, True], ids=["zeros", "h0c0"])
@pytest.mark.parametrize("T,B,I,H", SHAPES)
def test_lstm_forward(T, B, I, H, use0):
    out, hn, cn = reference(T, B, I, H, use0)
    got, hT, cT = run(T, B, I, H, 0, use0)
    close(got, out[:, :, :H].reshape(T * B, H), "h")
    close(hT, hn[0], "h_T")
    close(cT, cn[0], "c_T")


@pytest.mark.parametrize("T,B,I,H", [(7, 5, 16, 16), (12, 50, 40, 128), (5, 3, 8, 144)])
def test_lstm_reverse(T, B, I, H):
    """reverse=1 equals torch's forward LSTM on the time-flipped input, flipped back."""
    p = params(T, B, I, H)
    m = torch.nn.LSTM(I, H, 1).double()
    with torch.no_grad():
        for name, a in zip(("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"), p[1]):
            getattr(m, name).copy_(torch.from_numpy((a.T if a.ndim == 2 else a).astype(np.float64)))
        x = torch.from_numpy(p["x"].reshape(T, B, I).astype(np.float64)).flip(0)
        out, (hn, cn) = m(x, (torch.from_numpy(p["h0"][1:2].astype(np.float64)),
                              torch.from_numpy(p["c0"][1:2].astype(np.float64))))
        out = out.flip(0)
    got, hT, cT = run(T, B, I, H, 1, True)
    close(got, out.numpy().reshape(T * B, H), "h")
    close(hT, hn[0].numpy(), "h_T")
    close(cT, cn[0].numpy(), "c_T")


@pytest.mark.parametrize("d", [0, 1], ids=["forward", "reverse"])
@pytest.mark.parametrize("T,B,I,H", [(12, 50, 40, 128), (6, 20, 24, 256)])
def test_lstm_lengths(T, B, I, H, d):
    """d_lengths is pack_padded_sequence / pad_packed_sequence: zeros past each
    length, h_n / c_n after each utterance's last valid frame."""
    ln = draw_lengths(T, B)
    out, hn, cn = reference(T, B, I, H, True, ln)
    got, hT, cT = run(T, B, I, H, d, True, lengths=ln)
    got = got.reshape(T, B, H)
    for b in range(B):
        assert not got[ln[b]:, b].any(), b
    close(got, out[:, :, d * H:(d + 1) * H], "h")
    close(hT, hn[d], "h_T")
    close(cT, cn[d], "c_T")


@pytest.mark.parametrize("d", [0, 1], ids=["forward", "reverse"])
@pytest.mark.parametrize("T,B,I,H", [(7, 5, 16, 16), (5, 3, 8, 144)])
def test_lstm_length_zero(T, B, I, H, d):
    """An utterance of length 0: all-zero rows, h_T == h0 and c_T == c0 bit for
    bit; the other utterances are what they are without it (a negative length
    clamps to 0)."""
    p = params(T, B, I, H)
    ln = [T] * B
    ln[0], ln[B - 1] = 0, -3
    got, hT, cT = run(T, B, I, H, d, True, lengths=tuple(ln))
    full, hfull, cfull = run(T, B, I, H, d, True)
    got, full = got.reshape(T, B, H), full.reshape(T, B, H)
    for b in (0, B - 1):
        assert not got[:, b].any()
        assert np.array_equal(hT[b], p["h0"][d][b])
        assert np.array_equal(cT[b], p["c0"][d][b])
    assert np.array_equal(got[:, 1:B - 1], full[:, 1:B - 1])
    assert np.array_equal(hT[1:B - 1], hfull[1:B - 1])
    assert np.array_equal(cT[1:B - 1], cfull[1:B - 1])


@pytest.mark.parametrize("H", [48, 144])
def test_lstm_streaming_carry(H):
    """Forward, T = 12 in one call == frames [0, 5) then [5, 12) with the first
    call's d_hT / d_cT as the second's d_h0 / d_c0, bit for bit (how a streaming
    caller runs an LSTM; also the carried registers / rows against the stored
    ones)."""
    T, T1, B, I = 12, 5, 5, 24
    p = params(T, B, I, H)
    W = [dm(p[0][0]), dm(p[0][1]), dm(p[0][2].reshape(-1, 1)), dm(p[0][3].reshape(-1, 1))]
    h0, c0 = dm(p["h0"][0]), dm(p["c0"][0])
    whole, hT, cT = asr.DeviceMatrix(T * B, H), asr.DeviceMatrix(B, H), asr.DeviceMatrix(B, H)
    asr.lstm_fwd(dm(p["x"]), *W, whole, T, B, asr.DeviceBytes(asr.lstm_workspace_bytes(T, B, H)), h0=h0, c0=c0,
                 hT=hT, cT=cT)
    asr.synchronize()
    parts, hc, cc = [], h0, c0
    for lo, hi in ((0, T1), (T1, T)):
        n = hi - lo
        hid, hn, cn = asr.DeviceMatrix(n * B, H), asr.DeviceMatrix(B, H), asr.DeviceMatrix(B, H)
        asr.lstm_fwd(dm(p["x"][lo * B:hi * B]), *W, hid, n, B, asr.DeviceBytes(asr.lstm_workspace_bytes(n, B, H)),
                     h0=hc, c0=cc, hT=hn, cT=cn)
        asr.synchronize()
        parts.append(hid.toCpu())
        hc, cc = hn, cn
    assert np.array_equal(np.concatenate(parts), whole.toCpu())
    assert np.array_equal(hc.toCpu(), hT.toCpu())
    assert np.array_equal(cc.toCpu(), cT.toCpu())
    assert np.array_equal(hT.toCpu(), whole.toCpu()[(T - 1) * B:])


@pytest.mark.parametrize("T,B,I,H", [(9, 16, 24, 48), (6, 20, 24, 256)])
def test_lstm_ldh_two_halves(T, B, I, H):
    """ldh = 2H: a forward and a reverse call fill the two halves of one buffer
    (torch's bidirectional output); a single direction leaves the other half alone."""
    SENT = -12345.0
    out, _, _ = reference(T, B, I, H, True)
    buf = dm(np.full((T * B, 2 * H), SENT, np.float32))
    got, _, _ = run(T, B, I, H, 0, True, out=buf)
    assert np.all(got[:, H:] == SENT)
    close(got[:, :H], out.reshape(T * B, 2 * H)[:, :H], "forward half")
    got, _, _ = run(T, B, I, H, 1, True, out=buf)
    close(got, out.reshape(T * B, 2 * H), "both halves")
    buf2 = dm(np.full((T * B, 2 * H), SENT, np.float32))
    got2, _, _ = run(T, B, I, H, 1, True, out=buf2)
    assert np.all(got2[:, :H] == SENT)
    assert np.array_equal(got2[:, H:], got[:, H:])


@pytest.mark.parametrize("T,B,I,H", [(12, 50, 40, 128), (6, 20, 24, 256)])
def test_lstm_fwd_is_gemm_then_recurrence(T, B, I, H):
    """asr_lstm_fwd == asr_linear_fwd(EPI_NONE) + asr_lstm_recur_fwd, bit for bit."""
    ln = draw_lengths(T, B)
    a = run(T, B, I, H, 0, True, lengths=ln)
    b = run(T, B, I, H, 0, True, lengths=ln, recur_only=True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("H", [128, 256])
def test_lstm_batch_independent(H):
    """An utterance's bits do not depend on its batch: B = 37, then its first 5
    utterances as a batch of 5."""
    T, B, I, b = 6, 37, 24, 5
    p = params(T, B, I, H)
    W = [dm(p[0][0]), dm(p[0][1]), dm(p[0][2].reshape(-1, 1)), dm(p[0][3].reshape(-1, 1))]
    outs = []
    for nb in (B, b):
        x = np.ascontiguousarray(p["x"].reshape(T, B, I)[:, :nb]).reshape(T * nb, I)
        hid, hT, cT = asr.DeviceMatrix(T * nb, H), asr.DeviceMatrix(nb, H), asr.DeviceMatrix(nb, H)
        asr.lstm_fwd(dm(x), *W, hid, T, nb, asr.DeviceBytes(asr.lstm_workspace_bytes(T, nb, H)),
                     h0=dm(p["h0"][0][:nb]), c0=dm(p["c0"][0][:nb]), hT=hT, cT=cT)
        asr.synchronize()
        outs.append((hid.toCpu().reshape(T, nb, H)[:, :b], hT.toCpu()[:b], cT.toCpu()[:b]))
    for x, y in zip(*outs):
        assert np.array_equal(x, y)


def test_lstm_class_from_torch():
    """asr.LSTM.from_torch on a 2-layer bidirectional nn.LSTM(24, 48) with lengths."""
    T, B, I, H = 9, 16, 24, 48
    torch.manual_seed(48)
    m = torch.nn.LSTM(I, H, 2, bidirectional=True)
    ln = draw_lengths(T, B)
    x = np.random.default_rng(9).uniform(-1, 1, (T, B, I)).astype(np.float32)
    with torch.no_grad():
        pk = torch.nn.utils.rnn.pack_padded_sequence(torch.from_numpy(x.astype(np.float64)), torch.tensor(ln),
                                                     enforce_sorted=False)
        out, (hn, cn) = copy.deepcopy(m).double()(pk)
        out, _ = torch.nn.utils.rnn.pad_packed_sequence(out, total_length=T)
    net = asr.LSTM.from_torch(m)
    got = net.forward(dm(x.reshape(T * B, I)), T, B, lengths=ln).toCpu()
    close(got, out.numpy().reshape(T * B, 2 * H), "h")
    close(net.h_n.toCpu(), hn.numpy().reshape(4 * B, H), "h_n")
    close(net.c_n.toCpu(), cn.numpy().reshape(4 * B, H), "c_n")


def test_lstm_step_form_graph_replay():
    """The per-frame launches of the step form (H > 128) captured into a graph
    and replayed once give the eager call's bits."""
    T, B, I, H = 6, 20, 24, 256
    p = params(T, B, I, H)
    W = [dm(p[0][0]), dm(p[0][1]), dm(p[0][2].reshape(-1, 1)), dm(p[0][3].reshape(-1, 1))]
    h0, c0 = dm(p["h0"][0]), dm(p["c0"][0])
    ln = asr.device_lengths(draw_lengths(T, B))
    P, hid = asr.DeviceMatrix(T * B, 4 * H), asr.DeviceMatrix(T * B, H)
    hT, cT = asr.DeviceMatrix(B, H), asr.DeviceMatrix(B, H)
    work = asr.DeviceBytes(asr.lstm_workspace_bytes(T, B, H))
    asr.linear_fwd(dm(p["x"]), W[0], None, P, asr.EPI_NONE)
    asr.synchronize()

    def call(stream):
        asr.lstm_recur_fwd(P, W[1], W[2], W[3], hid, T, B, work, h0=h0, c0=c0, hT=hT, cT=cT, lengths=ln,
                           stream=stream)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call(s.cuda_stream)   # eager, on the capture stream (also loads the kernel)
    torch.cuda.synchronize()
    eager = (hid.toCpu(), hT.toCpu(), cT.toCpu())
    for m in (hid, hT, cT):
        asr.check(asr.lib().asr_memset(m.ptr, 0xFF, m.nbytes, None), "asr_memset")
    asr.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(torch.cuda.current_stream().cuda_stream)
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip((hid.toCpu(), hT.toCpu(), cT.toCpu()), eager):
        assert np.array_equal(x, y)
