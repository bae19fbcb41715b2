"""The audio front end's references and test cases, shared by
tests/test_fbank_gpu.py, tests/test_fbank_edges_gpu.py and
tests/test_fbank_edges_cpu.py.

References: features(), float64 numpy written from the semantics in
include/asr_amd.h (np.fft.rfft per frame, the float64 tables of
test_fbank_cpu.py), and features_fp32(), the same chain in fp32 on the CPU
(torch.fft.rfft float32, fp32 sums) on the library's own fp32 tables, which
asr_fbank_host_tables builds on the host: neither needs a GPU.

EDGE_CASES: the smallest inputs that reach the paths of csrc/fbank.hip that
CASES of test_fbank_gpu.py does not: frames past the 64th of an utterance
(a second and third workgroup per utterance, the per-wave loop to its last
trip), the log floor, 128 / 65 / 64 / 1 mel filters, filters without an FFT
bin, the DCT read from global memory and D > 64, hop > win, hop = 1, win =
n_fft, an odd win, win = 2, int16-scale samples and a tone 84 dB over dither.
edge(name) computes a case's input and both references once per process;
nothing is drawn again, and the arrays are read-only.

Metric: scale = |ref| for a log-mel output; for an MFCC output the size of the
DCT sum, sum_m |dct[k, m] e_ref[m]| (e near ln(1e-10) = -23 makes c_k a sum
with heavy cancellation, so |c_k| says nothing about its rounding error).  An
output element is in bound when |err| <= tol (1 + scale).
"""
import ctypes
import functools
from collections import namedtuple

import numpy as np
import torch

from conftest import asr
from test_fbank_cpu import BASE, ref_dct, ref_mel, ref_window

ATOL = 2e-5
ROOM = 3.5              # what the bound leaves over the fp32 CPU chain for another butterfly order
E32_FIXED = ATOL / ROOM   # 5.7e-6: below it the bound is ATOL itself
SENT = -12345.0
POISON = 1e30
FRAMES_PER_WG = 64      # FB_FRAMES_PER_WG of csrc/fbank.hip


def cfg(sr, win, hop, n_fft, mels, mfcc, C, **kw):
    return dict(BASE, sample_rate=float(sr), win_length=win, hop_length=hop, n_fft=n_fft, n_mels=mels,
                f_max=sr / 2.0, n_mfcc=mfcc, n_context=C, **kw)


def synth(sr, S, seed):
    t = np.arange(S, dtype=np.float64) / sr
    x = np.random.default_rng(seed).uniform(-0.5, 0.5, S)
    x = x + 0.3 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * (1000 + 1500 * t) * t)
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def waves(sr, B, S, seed0=0):
    w = np.stack([synth(sr, S, seed0 + b) for b in range(B)])
    w.setflags(write=False)
    return w


def num_frames(n, win, hop):
    return 0 if n < win else 1 + (n - win) // hop


def stack_context(base, frames, C):
    """base [T, B, D] -> [T, B, D (2C+1)]: frames t-C .. t+C, zeros outside
    [0, frames_b) and in rows t >= frames_b."""
    T, B, D = base.shape
    out = np.zeros((T, B, D * (2 * C + 1)), base.dtype)
    for b in range(B):
        for t in range(frames[b]):
            for c in range(-C, C + 1):
                if 0 <= t + c < frames[b]:
                    out[t, b, (c + C) * D:(c + C + 1) * D] = base[t + c, b]
    return out


def ref_stft(y, c):
    """Frames of the (pre-emphasised) float64 signal y: [frames, n_fft/2 + 1] complex."""
    win, hop, n_fft = c["win_length"], c["hop_length"], c["n_fft"]
    w = ref_window(c["window"], win)
    nf = num_frames(len(y), win, hop)
    return np.stack([np.fft.rfft(y[t * hop:t * hop + win] * w, n=n_fft) for t in range(nf)]) if nf else \
        np.zeros((0, n_fft // 2 + 1), complex)


def preemphasis(x, a):
    y = np.asarray(x, np.float64).copy()
    y[1:] -= a * np.asarray(x, np.float64)[:-1]
    return y


def lengths(wave, nsamples):
    """The lengths the kernel uses: nsamples clamped to [0, S], S for all when None."""
    B, S = wave.shape
    return [S] * B if nsamples is None else [min(max(int(n), 0), S) for n in nsamples]


def features_parts(c, wave, nsamples, T):
    """The float64 reference and what the checks need beside it:
    (out [T, B, F], frames [B], scale [T, B, F], logmel [T, B, n_mels] of the
    frames inside each utterance, zeros elsewhere)."""
    B, S = wave.shape
    ns = lengths(wave, nsamples)
    mel = ref_mel(c["sample_rate"], c["n_fft"], c["n_mels"], c["f_min"], c["f_max"])
    dct = ref_dct(c["n_mfcc"], c["n_mels"]) if c["n_mfcc"] else None
    D = c["n_mfcc"] or c["n_mels"]
    base, scale, logmel = np.zeros((T, B, D)), np.zeros((T, B, D)), np.zeros((T, B, c["n_mels"]))
    frames = []
    for b in range(B):
        X = ref_stft(preemphasis(wave[b, :ns[b]], c["preemph"]), c)
        P = X.real ** 2 + X.imag ** 2
        e = np.log(np.maximum(P @ mel.T, c["log_floor"]))
        logmel[:len(e), b] = e
        scale[:len(e), b] = np.abs(e) @ np.abs(dct).T if c["n_mfcc"] else np.abs(e)
        if c["n_mfcc"]:
            e = e @ dct.T
        base[:len(e), b] = e
        frames.append(len(e))
    return (stack_context(base, frames, c["n_context"]), np.asarray(frames, np.int32),
            stack_context(scale, frames, c["n_context"]), logmel)


def features(c, wave, nsamples, T):
    """The float64 reference: (out [T, B, F], frames [B])."""
    return features_parts(c, wave, nsamples, T)[:2]


def host_tables(c):
    """(window, mel, dct or None): the fp32 tables the device uses, from
    asr_fbank_host_tables (host only: no handle, no HIP call)."""
    fc = asr.FbankConfig(**c)
    win = np.zeros(fc.win_length, np.float32)
    mel = np.zeros((fc.n_mels, fc.n_fft // 2 + 1), np.float32)
    dct = np.zeros((fc.n_mfcc, fc.n_mels), np.float32) if fc.n_mfcc else None
    asr.check(asr.lib().asr_fbank_host_tables(ctypes.byref(fc), win.ctypes.data, mel.ctypes.data,
                                              dct.ctypes.data if fc.n_mfcc else None), "asr_fbank_host_tables")
    return win, mel, dct


def features_fp32(c, wave, nsamples, T):
    """The same chain in fp32 on the CPU: torch.fft.rfft float32, the library's
    fp32 tables, fp32 sums."""
    win, mel, dct = (None if a is None else torch.from_numpy(a) for a in host_tables(c))
    B, S = wave.shape
    ns = lengths(wave, nsamples)
    D = c["n_mfcc"] or c["n_mels"]
    base = np.zeros((T, B, D), np.float32)
    frames = []
    x = torch.from_numpy(np.array(wave))
    for b in range(B):
        nf = num_frames(ns[b], c["win_length"], c["hop_length"])
        frames.append(nf)
        if not nf:
            continue
        y = x[b, :ns[b]].clone()
        y[1:] -= np.float32(c["preemph"]) * x[b, :ns[b] - 1]
        fr = y.unfold(0, c["win_length"], c["hop_length"])[:nf] * win
        X = torch.fft.rfft(fr, n=c["n_fft"])
        e = torch.log(torch.clamp((X.real ** 2 + X.imag ** 2) @ mel.T, min=c["log_floor"]))
        if c["n_mfcc"]:
            e = e @ dct.T
        base[:nf, b] = e.numpy()
    return stack_context(base, frames, c["n_context"]), np.asarray(frames, np.int32)


def poisoned(wave, nsamples, ldw):
    """wave in a [B, ldw] buffer; everything an utterance does not own is 1e30."""
    B, S = wave.shape
    buf = np.full((B, ldw), POISON, np.float32)
    for b, n in enumerate(lengths(wave, nsamples)):
        buf[b, :n] = wave[b, :n]
    return buf


def run(c, wave, nsamples=None, T=None, ldw=None, ldo=None, stream=0, fe=None, bufs=None, want_frames=True):
    """asr_fbank_fwd on a sentinel-filled output: (out [T, B, ldo], frames [B]);
    want_frames False: d_frames = NULL, frames None."""
    own = fe is None
    fe = fe or asr.FeatureFrontend(**c)
    B, S = wave.shape
    ldw = ldw or S
    T = T or max(1, fe.num_frames(S))
    F = fe.feature_dim
    ldo = ldo or F
    if bufs is None:
        dw = asr.DeviceMatrix.from_numpy(poisoned(wave, nsamples, ldw))
        dn = None if nsamples is None else asr.device_lengths(nsamples)
        out = asr.DeviceMatrix.from_numpy(np.full((T * B, ldo), SENT, np.float32))
        frames = asr.DeviceBytes(4 * B)
        work = asr.DeviceBytes(max(16, fe.workspace_bytes(T, B)))
        bufs = (dw, dn, out, frames, work)
    dw, dn, out, frames, work = bufs
    asr.check(asr.lib().asr_fbank_fwd(fe.h, dw.ptr, ldw, dn.ptr if dn else None, B, S, out.ptr, ldo,
                                      frames.ptr if want_frames else None, work.ptr, T, stream), "asr_fbank_fwd")
    asr.synchronize()
    got = out.toCpu().reshape(T, B, ldo), asr.device_int32(frames, B) if want_frames else None
    if own:
        fe.close()
    return got


def check_padding(got, frames, c):
    """Rows t >= frames_b and context blocks outside the utterance are zero bits."""
    D, C = c["n_mfcc"] or c["n_mels"], c["n_context"]
    bits = np.ascontiguousarray(got).view(np.uint32)
    T, B, _ = got.shape
    for b in range(B):
        assert not bits[frames[b]:, b].any(), b
        for t in range(frames[b]):
            for k in range(-C, C + 1):
                if not 0 <= t + k < frames[b]:
                    assert not bits[t, b, (k + C) * D:(k + C + 1) * D].any(), (t, b, k)


def scaled_error(got, ref, scale):
    """(max |err|, max |err| / (1 + scale))."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    return float(err.max()), float((err / (1.0 + scale)).max())


# ------------------------------------------------------------------ the cases
STD = dict(sr=16000, win=400, hop=160)
HOP = 160
S_LONG = 22640      # 140 frames at win 400, hop 160
SHIFTS = (1, 63, 64, 65)

# name -> (config, signal, B, S, nsamples, fixed)
#   signal: the key of SIGNALS that draws the [B, S] input
#   fixed: the fp32 CPU chain stays within E32_FIXED on this case (asserted on the CPU), so the bound is ATOL.
#   torch.fft.rfft's fp32 error depends on the host CPU's code path (the same case gave 3.1e-6 on one host and
#   5.8e-6 on another), so a case is marked fixed only where the chain measured at most half of E32_FIXED on both;
#   the others take their bound from the chain's error where the test runs.
Edge = namedtuple("Edge", "config signal B S nsamples fixed")


def _e(config, signal, B, S, nsamples=None, fixed=True):
    return Edge(config, signal, B, S, None if nsamples is None else tuple(nsamples), fixed)


C512 = cfg(16000, 400, 160, 512, 40, 0, 0)
SHIFT_NS = (S_LONG,) + tuple(S_LONG - k * HOP for k in SHIFTS)
EDGE_CASES = {
    # ---- blocks: frames past the 64th
    # 140, 129, 65, 64, 0 frames: blocks 1 and 2, one frame alone in a block, an exactly full block, whole blocks of
    # zero rows, context rows across the 63 / 64 boundary
    "blocks-512": _e(cfg(16000, 400, 160, 512, 40, 26, 1), "std", 5, S_LONG, (22640, 20880, 10640, 10480, 399)),
    # 2 waves per workgroup, 32 trips per wave: 70 and 65 frames
    "blocks-2048": _e(cfg(16000, 400, 160, 2048, 64, 0, 0), "std", 2, 11440, (11440, 10640), fixed=False),
    # the 140-frame waveform and the same advanced by k hop samples
    "shift-p97": _e(C512, "shift", 5, S_LONG, SHIFT_NS, fixed=False),
    "shift-p0": _e(dict(C512, preemph=0.0), "shift", 5, S_LONG, SHIFT_NS),
    # ---- the floor and amplitude classes: silence, a gap, energies around the floor, int16 scale
    "floor-logmel": _e(C512, "floor", 4, 3440, fixed=False),
    "floor-mfcc": _e(dict(C512, n_mfcc=26), "floor", 4, 3440),
    "floor1-logmel": _e(dict(C512, log_floor=1.0), "floor1", 1, 3440),
    "floor1-mfcc": _e(dict(C512, log_floor=1.0, n_mfcc=26), "floor1", 1, 3440),
    # ---- mel layouts and the DCT
    "m128-d40": _e(cfg(16000, 400, 160, 512, 128, 40, 0), "std", 2, 1040),    # DCT from global, an empty filter
    "m128-d32": _e(cfg(16000, 400, 160, 512, 128, 32, 0), "std", 2, 1040),    # 4096 floats: the LDS limit
    "m128-8k": _e(cfg(8000, 200, 80, 256, 128, 128, 0), "std", 2, 1040),      # D > 64, six empty filters
    "m128-2048": _e(cfg(16000, 400, 160, 2048, 128, 0, 0), "std", 2, 1040, fixed=False),   # the largest packed table
    "m1-2048": _e(cfg(16000, 400, 160, 2048, 1, 0, 0), "std", 2, 1040),                    # one filter cut into 64 items
    "m64": _e(cfg(16000, 400, 160, 512, 64, 0, 0), "std", 2, 1040, fixed=False),           # one item per lane
    "m65": _e(cfg(16000, 400, 160, 512, 65, 0, 0), "std", 2, 1040, fixed=False),           # two
    "band": _e(dict(cfg(8000, 200, 80, 256, 23, 13, 0), f_min=300.0, f_max=3400.0), "std", 2, 1040),
    # ---- framing
    "hop-gt-win": _e(cfg(16000, 200, 300, 256, 23, 13, 1), "std", 2, 1040, (1040, 500)),
    "hop1-rect": _e(cfg(16000, 256, 1, 256, 23, 0, 0, window=asr.FBANK_WIN_RECT), "std", 2, 300, (300, 256),
                    fixed=False),
    "win401": _e(cfg(16000, 401, 160, 512, 40, 26, 0), "std", 2, 1040),
    "win2": _e(cfg(16000, 2, 1, 256, 23, 0, 0, window=asr.FBANK_WIN_RECT), "std", 2, 66, (66, 65)),
    "dc": _e(dict(C512, preemph=0.0), "dc", 2, 1040, fixed=False),
    # ---- a full-scale tone over 1-LSB dither
    "tone-p97": _e(C512, "tone", 2, 1040, fixed=False),
    "tone-p0": _e(dict(C512, preemph=0.0), "tone", 2, 1040, fixed=False),
}
# The frame counts each case must have (asserted on the CPU).
EDGE_FRAMES = {
    "blocks-512": [140, 129, 65, 64, 0], "blocks-2048": [70, 65], "shift-p97": [140, 139, 77, 76, 75],
    "shift-p0": [140, 139, 77, 76, 75], "floor-logmel": [20] * 4, "floor-mfcc": [20] * 4, "floor1-logmel": [20],
    "floor1-mfcc": [20], "m128-d40": [5, 5], "m128-d32": [5, 5], "m128-8k": [11, 11], "m128-2048": [5, 5],
    "m1-2048": [5, 5], "m64": [5, 5], "m65": [5, 5], "band": [11, 11], "hop-gt-win": [3, 2], "hop1-rect": [45, 1],
    "win401": [4, 4], "win2": [65, 64], "dc": [5, 5], "tone-p97": [5, 5], "tone-p0": [5, 5],
}
GAP = (1000, 2500)   # floor row 1: samples zeroed


def _sig_std(sr, B, S):
    return np.array(waves(sr, B, S))


def _sig_shift(sr, B, S):
    w = np.zeros((B, S), np.float32)
    w[0] = synth(sr, S, 0)
    for i, k in enumerate(SHIFTS):
        w[1 + i, :S - k * HOP] = w[0, k * HOP:]
    return w


def _near_floor(S, seed):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, S) * np.linspace(0.0, 3.0, S)


def _sig_floor(sr, B, S):
    w = np.zeros((4, S), np.float32)                       # row 0: digital silence
    w[1] = synth(sr, S, 1)
    w[1, GAP[0]:GAP[1]] = 0.0                              # row 1: a gap of zeros inside the usual signal
    w[2] = (3e-6 * _near_floor(S, 2)).astype(np.float32)   # row 2: band energies around 1e-10
    t = np.arange(S) / sr                                  # row 3: int16 scale, integers
    rng = np.random.default_rng(3)
    w[3] = np.round(8000 * rng.uniform(-1, 1, S) + 3000 * np.sin(2 * np.pi * 440 * t) +
                    3000 * np.sin(2 * np.pi * (1000 + 1500 * t) * t))
    return w


def _sig_floor1(sr, B, S):
    # row 2's shape at 1e5 times its scale (|x| about 0.1): band energies around a floor of 1.0
    return (0.3 * _near_floor(S, 2)).astype(np.float32)[None]


def _sig_dc(sr, B, S):
    return np.stack([(0.25 + 0.01 * np.random.default_rng(10 + b).uniform(-0.5, 0.5, S)).astype(np.float32)
                     for b in range(B)])


def _sig_tone(sr, B, S):
    t = np.arange(S) / sr
    return np.stack([np.round(16384 * np.sin(2 * np.pi * 1000 * t) + np.random.default_rng(20 + b).uniform(-1, 1, S))
                     .astype(np.float32) for b in range(B)])


SIGNALS = {"std": _sig_std, "shift": _sig_shift, "floor": _sig_floor, "floor1": _sig_floor1, "dc": _sig_dc,
           "tone": _sig_tone}

def logmel_twin(c):
    """The configuration's log-mel output without context: what an MFCC case's
    looser metric must not hide."""
    return dict(c, n_mfcc=0, n_context=0)


EdgeData = namedtuple("EdgeData", "c wave ns T ref frames scale logmel ref32")


@functools.lru_cache(maxsize=None)
def edge(name, twin=False):
    """A case's input, float64 reference (with the metric's scale and the
    log-mel energies) and fp32 CPU chain; computed once, read-only.  twin: the
    same input through the case's log-mel twin (logmel_twin)."""
    ec = EDGE_CASES[name]
    c = logmel_twin(ec.config) if twin else ec.config
    wave = np.ascontiguousarray(SIGNALS[ec.signal](int(c["sample_rate"]), ec.B, ec.S), dtype=np.float32)
    assert wave.shape == (ec.B, ec.S)
    T = max(1, num_frames(ec.S, c["win_length"], c["hop_length"]))
    ref, frames, scale, logmel = features_parts(c, wave, ec.nsamples, T)
    ref32, frames32 = features_fp32(c, wave, ec.nsamples, T)
    assert np.array_equal(frames, frames32)
    for a in (wave, ref, frames, scale, logmel, ref32):
        a.setflags(write=False)
    return EdgeData(c, wave, ec.nsamples, T, ref, frames, scale, logmel, ref32)


def e32(name, twin=False):
    """The fp32 CPU chain's max |err| / (1 + scale) against float64 on the case's input."""
    d = edge(name, twin)
    return scaled_error(d.ref32, d.ref, d.scale)[1]


def bound(name, twin=False):
    """The tolerance of a case: ATOL where the fp32 CPU chain leaves ROOM below it
    (the cases marked fixed: test_fbank_edges_cpu.py asserts that it does), else
    ROOM times the chain's own error on this input."""
    return max(ATOL, ROOM * e32(name, twin))


def floor_share(name, row=None):
    """Share of the reference's log-mel elements (inside the utterances; of one
    batch row when given) that sit at ln(log_floor)."""
    d = edge(name)
    rows = range(len(d.frames)) if row is None else [row]
    e = np.concatenate([d.logmel[:d.frames[b], b].ravel() for b in rows])
    return float(np.mean(e == np.log(d.c["log_floor"])))


def empty_filters(c):
    """Filters of the library's fp32 mel table without a non-zero weight."""
    return int((~host_tables(c)[1].any(axis=1)).sum())
