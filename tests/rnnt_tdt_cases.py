"""The token-and-duration transducer's test cases, shared by
tests/test_rnnt_tdt_cpu.py and tests/test_rnnt_tdt_gpu.py: rnnt_cases.py's random
models (same generator, same scaling) plus a duration head drawn after them,
their float64 reference decodes (computed once per process) and the conditions
every case must meet on the reference before anything is compared with it.

Every seed is the first in 0..199 at which the conditions below held, searched
with the reference alone on the CPU; nothing is drawn again at run time, and a
seed that breaks a condition fails the test.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

import rnnt_cases as rc
from rnnt_tdt_reference import TdtReference

# shape = (T, B, E, D_emb, Hp, J, V, L); the first nine fields are rnnt_cases.Case's, which make_model reads
Case = namedtuple("Case", "name shape blank max_symbols act lengths seed out_scale blank_bias durations dur_scale")
KINDS = ("blank>1", "blank0", "token0", "token>0", "cap", "skip")

D5 = (0, 1, 2, 3, 4)
L9, L7, L6 = (9, 0, 4, 9, 7), (7, 0, 5), (6, 0, 4)
CASES = [
    # tokens and durations in one tile
    Case("1-one-tile", (1, 1, 8, 16, 16, 16, 2, 1), 1, 1, "relu", (1,), 0, 4.0, 0.0, (0, 1), 4.0),
    # the duration columns open a tile of their own
    Case("2-own-tile", (9, 5, 24, 16, 48, 32, 16, 1), 15, 2, "relu", L9, 0, 4.0, 2.0, D5, 4.0),
    # the duration columns straddle two tiles
    Case("3-straddle", (9, 5, 24, 16, 48, 32, 14, 1), 13, 3, "relu", L9, 2, 4.0, 2.0, D5, 4.0),    # seeds 0, 1: 3 kinds
    # an unordered table, blank 0
    Case("4-unordered", (9, 5, 24, 16, 48, 32, 17, 1), 0, 2, "relu", L9, 0, 4.0, 2.0, (1, 0, 4, 2), 4.0),
    # two layers, tanh, the blank in the middle
    Case("5-blank-mid", (7, 3, 8, 32, 16, 48, 33, 2), 16, 2, "tanh", L7, 4, 4.0, 2.0, D5, 4.0),   # seeds 0-3: 2 or 3 kinds
    # columns 510 .. 514 cross the 32-tile group boundary: tile 31 is wave 7's, tile 32 wave 0's, and waves 0-6
    # sweep their token tiles by the four-tile product
    Case("6-group-edge", (6, 3, 8, 16, 16, 16, 510, 1), 509, 2, "relu", L6, 0, 4.0, 4.0, D5, 4.0),
    # a second workgroup with one row
    Case("7-two-groups", (6, 17, 16, 16, 16, 16, 17, 1), 16, 3, "relu",
         (6, 0, 3, 6, 5, 6, 2, 6, 6, 1, 6, 4, 6, 6, 0, 6, 6), 0, 4.0, 4.0, (0, 1, 2), 4.0),
    # the LDS limit's end of the range
    Case("8-c640", (12, 5, 64, 640, 640, 640, 1025, 1), 1024, 3, "relu", (12, 0, 7, 12, 9), 0, 4.0, 6.0, D5, 4.0),
]


def by_name(name):
    return next(c for c in CASES if c.name == name)


def make_model(case):
    """rnnt_cases.make_model's weights and enc, then w_dur [J, D], b_dur [D] from a generator of their own."""
    w, enc = rc.make_model(case)
    J, nd = case.shape[5], len(case.durations)
    gen = torch.Generator().manual_seed(1000 + case.seed)
    w["w_dur"] = rc._uniform(gen, (J, nd), (3.0 / J) ** 0.5 * case.dur_scale)
    w["b_dur"] = rc._uniform(gen, (nd,), 0.1)
    return w, enc


def make_reference(case, w):
    return TdtReference(w, case.durations, case.blank, case.act, case.max_symbols)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(weights, enc, the reference's decode of the case), computed once and not to be changed."""
    w, enc = make_model(case)
    return w, enc, make_reference(case, w).decode(enc, case.lengths)


def kinds_of(ref):
    return set().union(*ref["kinds"])


def check_conditions(case, ref):
    """Asserted on the reference alone.  1. Token and duration parity only mean something away from near-ties: the
    smallest top-2 gap of either head is at least 1e-3 * (1 + max|logit|); never waived.  2. Cases 2 to 5 each hold
    at least four of the six kinds of step (test_the_table_holds_every_kind_of_step has the table's union)."""
    floor = 1e-3 * (1.0 + ref["max_abs_logit"])
    assert min(ref["gap"]) >= floor and min(ref["dgap"]) >= floor, (case.name, min(ref["gap"]), min(ref["dgap"]), floor)
    if case.name[0] in "2345":
        assert len(kinds_of(ref) & set(KINDS)) >= 4, (case.name, kinds_of(ref))


def make_decoder(asr, case, w=None):
    T, B, E, D, Hp, J, V, L = case.shape
    if w is None:
        w = make_model(case)[0]
    return asr.TransducerDecoder.tdt(asr.rnnt_desc(V, case.blank, E, D, Hp, L, J, case.act, case.max_symbols), w,
                                     case.durations)


def lengths_of(case):
    return np.asarray(case.lengths, np.int32)


def compare_exact(case, res, state, cnt, ref):
    """Tokens, timesteps, durations, counts and skip_out equal the reference's."""
    assert cnt.tolist() == ref["count"], case.name
    assert state[1].tolist() == ref["skip"], case.name
    for b, r in enumerate(res):
        assert (r[0], r[1], r[4]) == (ref["tokens"][b], ref["timesteps"][b], ref["durations"][b]), (case.name, b)


def check_chunked(decode, enc, ln, cuts=(5, 4, 3)):
    """decode(enc, lengths, state) -> (results, state, counts): the chunks, with the state and the frame skip
    passed on and the frame offset added to the timesteps, give the whole decode's outputs bit for bit; at least
    one cut falls inside a jump."""
    whole, wstate, wcnt = decode(enc, ln, None)
    state, t0, inside = None, 0, False
    parts = [([], [], [], 0.0, []) for _ in whole]
    cnt = np.zeros_like(wcnt)
    for T in cuts:
        res, state, c = decode(np.ascontiguousarray(enc[t0:t0 + T]), np.clip(ln - t0, 0, T).astype(np.int32), state)
        inside |= t0 + T < enc.shape[0] and bool((state[1] > 0).any())
        parts = [(p[0] + r[0], p[1] + [t + t0 for t in r[1]], p[2] + r[2].tolist(), p[3] + r[3], p[4] + r[4])
                 for p, r in zip(parts, res)]
        cnt, t0 = cnt + c, t0 + T
    assert inside and cnt.tolist() == wcnt.tolist() and int(cnt.sum()) > 0
    assert np.array_equal(state[0], wstate[0]) and state[1].tolist() == wstate[1].tolist()
    for p, r in zip(parts, whole):
        assert (p[0], p[1], p[2], p[4]) == (r[0], r[1], r[2].tolist(), r[4])
