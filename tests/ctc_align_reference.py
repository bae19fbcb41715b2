"""fp64 reference for asr_ctc_align: the CTC forward log-likelihood and the
Viterbi forced alignment of one target against one utterance, in plain numpy.

Exactly the recurrences of include/asr_amd.h over the extended target ext
(S = 2L+1 states, ext[2i] = blank, ext[2i+1] = target[i]):

    frame 0:  a[0] = lp(0, blank), a[1] = lp(0, ext[1]), other states -inf
    forward:  a_t[s] = lse(lse(a[s], a[s-1]), a[s-2] if skip(s)) + lp(t, ext[s])
    Viterbi:  the same with max; ties take the smallest jump (stay, s-1, s-2);
              the final state is S-1 unless v[S-2] > v[S-1] strictly

with skip(s) = ext[s] != blank and ext[s] != ext[s-2], and lse(a, b) =
max + log1p(exp(-|a - b|)) (the oracle's formula).  The states of one frame
are updated as numpy vectors; nothing else is vectorised.

Checked on the CPU (tests/test_ctc_align_cpu.py) against torch's ctc_loss in
float64, against brute-force enumeration of all V^T alignments, and against
the project's oracle prefix scores with a beam that holds every prefix.
"""
from typing import NamedTuple, Sequence

import numpy as np

NINF = -np.inf


class AlignRef(NamedTuple):
    score: float        # forward log-likelihood (-inf: infeasible)
    vscore: float       # log-probability of the best alignment
    path: np.ndarray    # int32 [frames]: label per frame, blank included; all -1 when infeasible
    spans: np.ndarray   # int32 [L, 2]: first frame, one past the last frame; (-1, -1) when infeasible
    gap: float          # smallest best - second best over all Viterbi decisions with two finite candidates


def log_emissions(emis: np.ndarray, is_log: bool) -> np.ndarray:
    """fp64 log-probabilities of fp32 emissions, as the kernel converts them."""
    e = np.asarray(emis, dtype=np.float32).astype(np.float64)
    if is_log:
        return e
    with np.errstate(divide="ignore"):
        return np.log(e)


def lse(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        r = np.maximum(a, b) + np.log1p(np.exp(-np.abs(a - b)))
    return np.where(a == NINF, b, np.where(b == NINF, a, r))


def _shift(x: np.ndarray, k: int) -> np.ndarray:
    return np.concatenate([np.full(k, NINF), x[:len(x) - k]]) if k <= len(x) else np.full(len(x), NINF)


def _infeasible(frames: int, L: int) -> AlignRef:
    return AlignRef(NINF, NINF, np.full(frames, -1, np.int32), np.full((L, 2), -1, np.int32), np.inf)


def ctc_reference(lp: np.ndarray, target: Sequence[int], blank: int = 0) -> AlignRef:
    """lp: fp64 [frames][V] log-probabilities of the utterance's own frames."""
    lp = np.asarray(lp, dtype=np.float64)
    frames, V = lp.shape
    target = [int(c) for c in target]
    L = len(target)
    if any(c == blank or c < 0 or c >= V for c in target):
        return _infeasible(frames, L)
    if frames == 0:
        if L:
            return _infeasible(frames, L)
        return AlignRef(0.0, 0.0, np.zeros(0, np.int32), np.zeros((0, 2), np.int32), np.inf)
    S = 2 * L + 1
    ext = np.full(S, blank, np.int64)
    ext[1::2] = target
    skip = np.zeros(S, bool)
    skip[3::2] = ext[3::2] != ext[1:S - 2:2]

    a = np.full(S, NINF)
    a[0] = lp[0, blank]
    if S > 1:
        a[1] = lp[0, ext[1]]
    v = a.copy()
    bp = np.zeros((frames, S), np.int8)
    gap = np.inf
    for t in range(1, frames):
        e = lp[t, ext]
        a = lse(lse(a, _shift(a, 1)), np.where(skip, _shift(a, 2), NINF)) + e
        cand = np.stack([v, _shift(v, 1), np.where(skip, _shift(v, 2), NINF)])
        bp[t] = np.argmax(cand, axis=0)          # first maximum: the smallest jump
        top = np.sort(cand, axis=0)[::-1]
        two = top[1] > NINF
        if two.any():
            gap = min(gap, float((top[0][two] - top[1][two]).min()))
        v = top[0] + e
    score = float(lse(a[S - 1:S], a[S - 2:S - 1])[0]) if L else float(a[0])
    s = S - 1
    if L and v[S - 2] > v[S - 1]:
        s = S - 2
    if L and v[S - 1] > NINF and v[S - 2] > NINF:
        gap = min(gap, float(abs(v[S - 1] - v[S - 2])))
    vscore = float(v[s])
    if vscore == NINF:
        return AlignRef(score, NINF, np.full(frames, -1, np.int32), np.full((L, 2), -1, np.int32), gap)
    states = np.zeros(frames, np.int64)
    for t in range(frames - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    path = ext[states].astype(np.int32)
    spans = np.full((L, 2), -1, np.int32)
    for i in range(L):
        at = np.nonzero(states == 2 * i + 1)[0]
        spans[i] = (at[0], at[-1] + 1)
    return AlignRef(score, vscore, path, spans, gap)
