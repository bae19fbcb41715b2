"""The transducer lattice-scoring cases shared by tests/test_rnnt_align_cpu.py
and tests/test_rnnt_align_gpu.py: rnnt_cases' random models with fixed seeds,
target lists drawn from a generator with a fixed seed of its own, their float64
references (computed once per process, not to be changed) and the condition
each case must meet on the reference before frames are compared with it.

The seeds were searched for on the CPU with the reference until the condition
held for every target of the case in both topologies; nothing is drawn again at
run time, and a seed that breaks the condition fails the test.
"""
import functools
from collections import namedtuple

import torch

import rnnt_beam_cases as bc
import rnnt_cases as rc
from rnnt_align_reference import AlignReference

# spec: one (utterance, target length) per target; greedy: the labels are the model's own greedy walk of the
# utterance under that max_symbols (cut to the length) instead of random ones
AlignCase = namedtuple("AlignCase", "name model spec tseed greedy")

TOPOLOGIES = ("standard", "one_per_frame")
REL = 2e-5          # the kernel's bound per summed term: test_rnnt_gpu.py's bound for totals


def _a(name, shape, act, lengths, seed, blank_bias, spec, tseed, greedy=0, out_scale=4.0):
    return AlignCase(name, rc.Case(name, shape, 0, 1, act, tuple(lengths), seed, out_scale, blank_bias), tuple(spec),
                     tseed, greedy)


# S2: T = 9, lengths [9, 0, 4, 9, 7]; target lengths 0, 1, = len, > len, > T; a zero-frame utterance with U = 0 and U > 0
SPEC_S2 = [(0, 0), (0, 1), (0, 9), (0, 5), (2, 4), (2, 5), (3, 12), (4, 7), (4, 3), (1, 0), (1, 2)]
# S3: T = 7, lengths [7, 0, 5]
SPEC_S3 = [(0, 0), (0, 1), (0, 7), (0, 3), (2, 5), (2, 6), (2, 9), (1, 0), (1, 1)]
SMALL_CASES = [
    _a("s2", rc.S2, "relu", rc.L2, 0, 2.0, SPEC_S2, 0),
    _a("s3", rc.S3, "tanh", rc.L3, 0, 3.0, SPEC_S3, 0),
]
# An n-best list: N = B * K targets, utt[n] = n / K (K = 2)
NBEST_CASE = _a("s2-nbest", rc.S2, "relu", rc.L2, 0, 2.0, [(n // 2, 2 + n % 4) for n in range(10)], 1)
# GPU only.  U = 70 and U = 130 over 6 and 5 frames (426 and 655 nodes, no multiple of the 48-row tile).  The lattice
# kernel's states per lane follow the call's max_target_len (1 below 64, 2 below 128, else 4), so a call with all
# three targets runs with four; the tests also score the U = 70 target in a call of its own (two states per lane).
# A random transcript of 130 labels over 6 frames has a log-probability near -400, whose rounding bound is wider
# than the gaps of its lattice; the model's own greedy walk (blank made rare) is a transcript with a decisive best
# path.
LONG_CASE = _a("long", (6, 2, 16, 16, 16, 16, 17, 1), "relu", [6, 5], 1, -2.0, [(0, 70), (1, 130), (1, 3)], 0,
               greedy=40, out_scale=8.0)
# V = 257 (two layers, 320) and V = 1025 (640: the LDS limit, V no multiple of 16, three column sweeps), T <= 12, U <= 6;
# V = 437 (rnnt_cases.MIXED: 28 column tiles, waves on both paths of the sweep at once)
UPPER_CASES = [
    AlignCase("l2-320", bc.UPPER_CASES[1].model, ((0, 6), (0, 0), (2, 3), (3, 5), (3, 1), (1, 0)), 0, 0),
    AlignCase("c640", bc.UPPER_CASES[0].model, ((0, 6), (2, 4), (3, 1), (4, 5), (0, 0)), 0, 0),
    _a("mixed", rc.MIXED, "relu", [6, 0, 4], 0, 2.0, [(0, 4), (0, 0), (2, 3), (2, 1), (0, 6), (1, 0)], 0),
]
# The joint kernel takes three row tiles of 16 nodes up to J = 816, two from J = 832 and one from J = 1264 (what
# fits in LDS): the smallest J of the other two kernels, at a small V and T; 36 nodes are more than one workgroup of either
SPEC_WIDE = [(0, 8), (0, 0), (1, 2), (1, 4), (0, 3)]
WIDE_J_CASES = [
    _a("j832", (4, 2, 16, 16, 16, 832, 17, 1), "relu", [4, 3], 0, 2.0, SPEC_WIDE, 0),
    _a("j1264", (4, 2, 16, 16, 16, 1264, 17, 1), "relu", [4, 3], 0, 2.0, SPEC_WIDE, 0),
]
# The search is the lattice when nothing is pruned: V = 2 (one label), T = 8, K = 16
NOPRUNE_MODEL = rc.Case("noprune", (8, 3, 8, 16, 16, 16, 2, 1), 0, 1, "relu", (8, 5, 0), 0, 4.0, 0.5)
# Greedy is one alignment: max_symbols (24) so high that the walk never reaches it.  A random transducer either
# emits blanks only or repeats a label up to any cap (rnnt_cases), so these seeds were searched until the walk
# ended every frame on a blank, with several emissions in some frame (about one seed in twenty)
GREEDY_MODELS = [rc.Case("s2-greedy", rc.S2, 0, 24, "relu", tuple(rc.L2), 17, 4.0, 4.0),
                 rc.Case("s3-greedy", rc.S3, 0, 24, "tanh", tuple(rc.L3), 39, 4.0, 4.0)]


def targets_of(case):
    """(targets, utt) of a case: label lists and the utterance of each."""
    V = case.model.shape[6]
    utt = [b for b, _u in case.spec]
    if case.greedy:
        w, enc = rc.make_model(case.model)
        walk = AlignReference(w, case.model.blank, case.model.act, case.greedy).decode(enc, case.model.lengths)
        targets = []
        for b, U in case.spec:
            assert len(walk["tokens"][b]) >= U, (case.name, b, len(walk["tokens"][b]), U)
            targets.append(list(walk["tokens"][b][:U]))
        return targets, utt
    gen = torch.Generator().manual_seed(1000 + case.tseed)
    targets = []
    for _b, U in case.spec:
        labels = torch.randint(0, V - 1, (U,), generator=gen).tolist()
        targets.append([y if y < case.model.blank else y + 1 for y in labels])      # never the blank
    return targets, utt


@functools.lru_cache(maxsize=None)
def reference(case, topology):
    """(weights, enc, targets, utt, the reference's result per target), computed once and not to be changed."""
    w, enc = rc.make_model(case.model)
    targets, utt = targets_of(case)
    ref = AlignReference(w, case.model.blank, case.model.act, 1).align(enc, targets, case.model.lengths, utt, topology)
    return w, enc, targets, utt, ref


def bound(value, terms):
    """|gpu - ref| <= REL * (1 + |ref|) * terms, terms = the summed log-probabilities (len_b + U_n for a score)."""
    return REL * (1.0 + abs(value)) * max(terms, 1)


def frames_comparable(r):
    """A target's frames are compared only when every decision of its best path
    is clear of rounding: at each node (t, u) of the path the gap between the
    two candidates is at least twice the bound of a value of t + u terms."""
    return all(gap >= 2.0 * bound(value, t + u) for t, u, value, gap in r["cells"])


def check_conditions(case, ref):
    """No target of any case is left out of the frames comparison."""
    for n, r in enumerate(ref):
        assert frames_comparable(r), (case.name, n, min((g / bound(v, t + u), t, u) for t, u, v, g in r["cells"]))
