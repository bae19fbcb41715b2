"""The transducer test cases shared by tests/test_rnnt_cpu.py and
tests/test_rnnt_gpu.py: random models with fixed seeds, their float64
reference decodes (computed once per process) and the conditions each case
must meet on the reference before anything is compared with it.

A randomly drawn transducer emits all blanks or always hits the cap, so every
case scales W_out (out_scale) and sets b_out[blank] (blank_bias) so that its
walk mixes frames without an emission, with one, with several, and frames
that hit the cap.  The seeds were searched for on the CPU (torch's CPU
generator) until both conditions below held; nothing is drawn again at run
time, and a seed that breaks a condition fails the test.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

from rnnt_reference import Reference

# shape = (T, B, E, D, Hp, J, V, L)
Case = namedtuple("Case", "name shape blank max_symbols act lengths seed out_scale blank_bias")


def _c(name, shape, blank_last, ms, act, lengths, seed, out_scale, blank_bias):
    return Case(name, shape, shape[6] - 1 if blank_last else 0, ms, act, tuple(lengths), seed, out_scale, blank_bias)


S1 = (1, 1, 8, 16, 16, 16, 2, 1)
S2 = (9, 5, 24, 16, 48, 32, 17, 1)
S3 = (7, 3, 8, 32, 16, 48, 33, 2)
L2, L3 = [9, 0, 4, 9, 7], [7, 0, 5]

# name, shape, blank at V - 1, max_symbols, activation, lengths, seed, out_scale, blank_bias
SMALL_CASES = [
    _c("s1-b0-m1", S1, False, 1, "relu", [1], 0, 4.0, 0.0),
    _c("s1-bl-m1", S1, True, 1, "relu", [1], 1, 4.0, 0.0),
    _c("s1-b0-m3", S1, False, 3, "relu", [1], 2, 4.0, 0.0),
    _c("s1-bl-m3", S1, True, 3, "relu", [1], 3, 4.0, 0.0),
    _c("s2-b0-m1", S2, False, 1, "relu", L2, 0, 4.0, 2.0),
    _c("s2-bl-m1", S2, True, 1, "relu", L2, 0, 4.0, 2.0),
    _c("s2-b0-m3", S2, False, 3, "relu", L2, 0, 4.0, 2.0),
    _c("s2-bl-m3", S2, True, 3, "relu", L2, 0, 4.0, 4.0),
    _c("s3-b0-m1", S3, False, 1, "tanh", L3, 0, 4.0, 3.0),
    _c("s3-bl-m1", S3, True, 1, "tanh", L3, 0, 4.0, 2.0),
    _c("s3-b0-m3", S3, False, 3, "tanh", L3, 1, 4.0, 2.0),
    _c("s3-bl-m3", S3, True, 3, "tanh", L3, 2, 4.0, 5.0),
]
# GPU only: two row tiles (the second with one row), the required upper range, two layers at 320, and 28 column tiles
# of J and V (waves 0-3 take four tiles in one product, waves 4-7 three single ones; the last V tile is partial and
# holds the blank, 436)
MIXED = (6, 3, 8, 16, 16, 448, 437, 1)
LARGE_CASES = [
    _c("tiles", (6, 17, 16, 16, 16, 16, 17, 1), False, 3, "relu",
       [6, 0, 3, 6, 5, 6, 2, 6, 6, 1, 6, 4, 6, 6, 0, 6, 6], 0, 4.0, 4.0),
    _c("c640", (12, 5, 64, 640, 640, 640, 1025, 1), True, 3, "relu", [12, 0, 7, 12, 9], 0, 4.0, 6.0),
    _c("l2-320", (8, 4, 16, 320, 320, 320, 257, 2), False, 2, "tanh", [8, 0, 8, 5], 0, 4.0, 5.0),
    _c("mixed", MIXED, True, 3, "relu", [6, 0, 4], 2, 4.0, 4.0),
]


def _uniform(gen, shape, bound):
    return ((torch.rand(shape, generator=gen, dtype=torch.float32) * 2 - 1) * bound).numpy()


def make_model(case):
    """(weights dict of float32 arrays in [in][out] layout, enc [T, B, E] float32)."""
    T, B, E, D, Hp, J, V, L = case.shape
    gen = torch.Generator().manual_seed(case.seed)
    k = Hp ** -0.5
    w = {"emb": _uniform(gen, (V, D), 1.0), "w_ih": [], "w_hh": [], "b_ih": [], "b_hh": []}
    for l in range(L):
        w["w_ih"].append(_uniform(gen, (Hp if l else D, 4 * Hp), k))
        w["w_hh"].append(_uniform(gen, (Hp, 4 * Hp), k))
        w["b_ih"].append(_uniform(gen, (4 * Hp,), k))
        w["b_hh"].append(_uniform(gen, (4 * Hp,), k))
    w["w_enc"], w["b_enc"] = _uniform(gen, (E, J), (3.0 / E) ** 0.5), _uniform(gen, (J,), 0.1)
    w["w_pred"], w["b_pred"] = _uniform(gen, (Hp, J), (3.0 / Hp) ** 0.5 * 4.0), _uniform(gen, (J,), 0.1)
    w["w_out"] = _uniform(gen, (J, V), (3.0 / J) ** 0.5 * case.out_scale)
    w["b_out"] = _uniform(gen, (V,), 0.1)
    w["b_out"][case.blank] = case.blank_bias
    enc = _uniform(gen, (T, B, E), 1.0)
    return w, enc


@functools.lru_cache(maxsize=None)
def reference(case):
    """(weights, enc, the reference's decode of the case), computed once and not to be changed."""
    w, enc = make_model(case)
    ref = Reference(w, case.blank, case.act, case.max_symbols).decode(enc, case.lengths)
    return w, enc, ref


def check_conditions(case, ref):
    """The conditions on the inputs, asserted on the reference alone.

    1. Exact token parity only means something away from near-ties: the
       smallest top-2 logit gap of the walk is at least 1e-3 * (1 + max|logit|),
       about a thousand fp32 roundings of a logit.
    2. The walk mixes its paths: a frame without an emission, one with exactly
       one, one with two or more (possible only for max_symbols >= 2), and for
       max_symbols > 1 a frame that hits the cap.  A case of fewer than four
       frames in all (T = B = 1) cannot hold four kinds of frame; it is held
       to the first condition only.
    """
    gap = min(ref["gap"])
    assert gap >= 1e-3 * (1.0 + ref["max_abs_logit"]), (case.name, gap, ref["max_abs_logit"])
    frames = [n for f in ref["frames"] for n in f]
    if len(frames) < 4:
        return
    assert any(n == 0 for n in frames), (case.name, frames)
    assert any(n == 1 for n in frames), (case.name, frames)
    if case.max_symbols > 1:
        assert any(n >= 2 for n in frames), (case.name, frames)
        assert any(n == case.max_symbols for n in frames), (case.name, frames)


def make_decoder(asr, case, w=None):
    T, B, E, D, Hp, J, V, L = case.shape
    if w is None:
        w = make_model(case)[0]
    return asr.TransducerDecoder(asr.rnnt_desc(V, case.blank, E, D, Hp, L, J, case.act, case.max_symbols), w)


def lengths_of(case):
    return np.asarray(case.lengths, np.int32)
