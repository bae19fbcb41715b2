"""GPU checks of the transducer lattice scorer (asr_rnnt_align): the fused joint
kernel and the lattice kernel against tests/rnnt_align_reference.py and the
host twin.  Scores and Viterbi scores within test_rnnt_gpu.py's bound for
totals per summed term, |gpu - ref| <= 2e-5 * (1 + |ref|) * (len_b + U_n);
emission frames equal to the reference's and the twin's for every target (the
cases' seeds keep every decision of every best path at least twice the bound
apart, which is asserted); independence of N, position, max_target_len and of
the outputs asked for, bit for bit; rescore on beam_search output; infeasible
targets and zero-length utterances.

Measured on an MI355X (max over the case of |gpu - ref| / ((1 + |ref|) *
(len_b + U_n))) are in DESIGN.md §28; the bound is 2e-5."""
import math

import numpy as np
import pytest

import rnnt_align_cases as ac
import rnnt_beam_cases as bc
import rnnt_cases as rc
from conftest import asr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    asr.set_device(0)


def compare(name, got, ref, host=None):
    score, vscore, frames = got
    err = 0.0
    for n, r in enumerate(ref):
        for g, want in ((score[n], r["score"]), (vscore[n], r["vscore"])):
            if math.isinf(want):
                assert g == want, (name, n, g, want)
            else:
                err = max(err, abs(g - want) / ((1.0 + abs(want)) * max(r["terms"], 1)))
    print(f"rnnt align {name}: max score err per term {err:.3e} (bound {ac.REL:.0e})")
    for n, r in enumerate(ref):
        for g, want in ((score[n], r["score"]), (vscore[n], r["vscore"])):
            assert math.isinf(want) or abs(g - want) <= ac.bound(want, r["terms"]), (name, n, g, want)
        assert ac.frames_comparable(r), (name, n)           # no target is left out
        assert frames[n].tolist() == r["frames"], (name, n, frames[n].tolist(), r["frames"])
        if host is not None:
            assert frames[n].tolist() == host[2][n].tolist(), (name, n)
        if math.isfinite(r["score"]):
            assert score[n] >= vscore[n]


def run_case(case, topology):
    w, enc, targets, utt, ref = ac.reference(case, topology)
    ac.check_conditions(case, ref)
    dec = rc.make_decoder(asr, case.model, w)
    ln = rc.lengths_of(case.model)
    got = dec.align(enc, targets, ln, utt, topology)
    host = dec.align_host(enc, targets, ln, utt, topology)
    compare(f"{case.name}/{topology}", got, ref, host)
    return dec, enc, targets, utt, ln, got


@pytest.mark.parametrize("topology", ac.TOPOLOGIES)
@pytest.mark.parametrize("case", ac.SMALL_CASES + [ac.NBEST_CASE, ac.LONG_CASE], ids=lambda c: c.name)
def test_kernel_matches_reference(case, topology):
    dec, enc, targets, utt, ln, got = run_case(case, topology)
    if case is ac.LONG_CASE:
        assert [len(t) for t in targets][:2] == [70, 130]      # max_target_len = 130: four states per lane
    if case is ac.NBEST_CASE:
        assert utt == [n // 2 for n in range(len(targets))]    # N = B K, utt[n] = n / K
    dec.close()


@pytest.mark.parametrize("topology", ac.TOPOLOGIES)
@pytest.mark.parametrize("case", ac.UPPER_CASES, ids=lambda c: c.name)
def test_upper_range(case, topology):
    T, V = case.model.shape[0], case.model.shape[6]
    assert T <= 12 and max(U for _b, U in case.spec) <= 6 and V in (257, 437, 1025)
    dec = run_case(case, topology)[0]
    dec.close()


@pytest.mark.parametrize("topology", ac.TOPOLOGIES)
@pytest.mark.parametrize("case", ac.WIDE_J_CASES, ids=lambda c: c.name)
def test_joint_kernels_of_two_and_one_row_tiles(case, topology):
    """J = 832 and J = 1264: the joint kernel with 32 and with 16 nodes per workgroup, more than one workgroup each."""
    J = case.model.shape[5]
    assert J in (832, 1264) and max(ln * (U + 1) for (b, U), ln in
                                    ((s, case.model.lengths[s[0]]) for s in case.spec)) > 32
    dec = run_case(case, topology)[0]
    dec.close()


@pytest.mark.parametrize("topology", ac.TOPOLOGIES)
def test_states_per_lane(topology):
    """The lattice kernel takes 1, 2 or 4 states per lane by the call's max_target_len (< 64, < 128, else).  The
    U = 70 target in a call of its own runs with two: against the reference and the twin, and with the bits of
    the four-state run; the U = 3 target with one, two and four."""
    case = ac.LONG_CASE
    w, enc, targets, utt, ref = ac.reference(case, topology)
    ac.check_conditions(case, ref)
    assert [len(t) for t in targets] == [70, 130, 3]
    dec = rc.make_decoder(asr, case.model, w)
    ln = rc.lengths_of(case.model)
    four = dec.align(enc, targets, ln, utt, topology)                           # max_target_len = 130
    two = dec.align(enc, targets[:1], ln, utt[:1], topology)                    # max_target_len = 70
    host = dec.align_host(enc, targets[:1], ln, utt[:1], topology)
    compare(f"long U = 70 alone/{topology}", two, ref[:1], host)
    wide = dec._align(enc, targets[:1], ln, utt[:1], topology, 0, (True, True, True), max_target_len=127)

    def same(a, n, b):
        assert a[0][0].tobytes() == b[0][n].tobytes() and a[1][0].tobytes() == b[1][n].tobytes()
        assert a[2][0].tolist() == b[2][n].tolist()

    same(two, 0, four)
    same(wide, 0, four)
    for mtl in (3, 63, 64, 127, 128):                                           # one, one, two, two, four
        got = dec._align(enc, targets[2:], ln, utt[2:], topology, 0, (True, True, True), max_target_len=mtl)
        same(got, 2, four)
    compare(f"long U = 3 alone/{topology}", dec.align(enc, targets[2:], ln, utt[2:], topology), ref[2:])
    dec.close()


@pytest.mark.parametrize("topology", ac.TOPOLOGIES)
@pytest.mark.parametrize("case", [ac.SMALL_CASES[0], ac.SMALL_CASES[1], ac.LONG_CASE], ids=lambda c: c.name)
def test_independence(case, topology):
    """A target's bits depend on its own frames, labels and lengths only."""
    w, enc, targets, utt, _ref = ac.reference(case, topology)
    dec = rc.make_decoder(asr, case.model, w)
    ln = rc.lengths_of(case.model)
    score, vscore, frames = dec.align(enc, targets, ln, utt, topology)

    def same(got, idx):
        s, v, f = got
        for k, n in enumerate(idx):
            if s is not None:
                assert s[k].tobytes() == score[n].tobytes(), (case.name, n)
            if v is not None:
                assert v[k].tobytes() == vscore[n].tobytes(), (case.name, n)
            if f is not None:
                assert f[k].tolist() == frames[n].tolist(), (case.name, n)

    first = list(range(min(3, len(targets))))
    same(dec.align(enc, [targets[n] for n in first], ln, [utt[n] for n in first], topology), first)     # N, alone
    perm = [(5 * n + 2) % len(targets) for n in range(len(targets))]          # N = 11, 9, 3: coprime to 5
    assert sorted(perm) == list(range(len(targets)))
    same(dec.align(enc, [targets[n] for n in perm], ln, [utt[n] for n in perm], topology), perm)       # shuffled order
    mtl = max(len(t) for t in targets)
    everyone = list(range(len(targets)))
    same(dec._align(enc, targets, ln, utt, topology, 0, (True, True, True), max_target_len=mtl + 37), everyone)
    same(dec._align(enc, targets, ln, utt, topology, 0, (True, False, False)), everyone)               # each output alone
    same(dec._align(enc, targets, ln, utt, topology, 0, (False, True, False)), everyone)
    same(dec._align(enc, targets, ln, utt, topology, 0, (False, False, True)), everyone)
    # T: the same utterances inside a longer, padded batch
    pad = np.concatenate([enc, np.ones((5,) + enc.shape[1:], np.float32)], axis=0)
    same(dec.align(pad, targets, ln, utt, topology), everyone)
    dec.close()


def test_rescore_of_a_beam_search():
    case = next(c for c in bc.SMALL_CASES if c.name == "s2-k4-a")
    w, enc = rc.make_model(case.model)
    dec = bc.make_decoder(asr, case, w)
    ln = rc.lengths_of(case.model)
    nbest = dec.beam_search(enc, ln, beam=case.beam)
    res = dec.rescore(nbest, enc, ln)
    targets = [h[0] for u in nbest for h in u]
    utt = [b for b, u in enumerate(nbest) for _ in u]
    exact = dec.score(enc, targets, ln, utt, "one_per_frame")
    k = 0
    for b, (u, r) in enumerate(zip(nbest, res)):
        assert len(r) == len(u)
        by_tokens = {tuple(h[0]): float(exact[k + j]) for j, h in enumerate(u)}
        search = {tuple(h[0]): h[2] for h in u}
        for tok, s, e in r:
            assert np.float64(e).tobytes() == np.float64(by_tokens[tuple(tok)]).tobytes(), b      # bit for bit
            assert s == search[tuple(tok)]
            assert e >= s - ac.bound(s, int(ln[b]) + len(tok)), (b, tok, e, s)
        assert [e for _t, _s, e in r] == sorted((e for _t, _s, e in r), reverse=True)
        # equal exact scores keep the search order
        order = sorted(range(len(u)), key=lambda j: -float(exact[k + j]))
        assert [t for t, _s, _e in r] == [u[j][0] for j in order]
        k += len(u)
    # the exact scores feed nbest_mbr as they are
    lists = [[t for t, _s, _e in r] for r in res]
    weights = [[e for _t, _s, e in r] for r in res]
    asr.nbest_mbr(lists, log_weights_per_utt=weights)
    dec.close()


def test_infeasible_targets_and_zero_length_utterances():
    case = ac.SMALL_CASES[0]                   # S2: T = 9, lengths [9, 0, 4, 9, 7], blank 0, V = 17
    w, enc = rc.make_model(case.model)
    dec = rc.make_decoder(asr, case.model, w)
    ln = rc.lengths_of(case.model)
    good = [3, 5, 7]
    targets = [good, [3, 0, 7], [3, 17, 7], [3, -1, 7], good, good, [], good, good, [1, 2, 3, 4, 5]]
    utt = [0, 0, 0, 0, -1, 5, 1, 1, 2, 2]
    for topology in ac.TOPOLOGIES:
        score, vscore, frames = dec.align(enc, targets, ln, utt, topology)
        hs, hv, hf = dec.align_host(enc, targets, ln, utt, topology)
        for n in (1, 2, 3, 4, 5, 7):
            assert score[n] == -math.inf and vscore[n] == -math.inf and frames[n].tolist() == [-1, -1, -1], (topology, n)
        assert score[6] == 0.0 and vscore[6] == 0.0
        assert (score[9] == -math.inf) == (topology == "one_per_frame")
        for n in range(len(targets)):
            assert math.isinf(hs[n]) == math.isinf(score[n]) and frames[n].tolist() == hf[n].tolist(), (topology, n)
            if math.isfinite(hs[n]):
                assert abs(score[n] - hs[n]) <= ac.bound(hs[n], int(ln[utt[n]]) + len(targets[n]))
    dec.close()
