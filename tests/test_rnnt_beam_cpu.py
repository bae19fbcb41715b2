"""CPU checks of the transducer beam search (asr_rnnt_beam*): the fp64 host twin
asr_rnnt_beam_host against tests/rnnt_beam_reference.py, K = 1 against the
greedy twin, truncation at max_out, the n-best through nbest_mbr and every
refusal.  No GPU is needed or used."""
import numpy as np
import pytest

import rnnt_beam_cases as bc
import rnnt_cases as rc
from conftest import asr

REL = 1e-9   # the project's oracle bound: both sides are fp64 and differ in summation order only


def close(a, b):
    return abs(a - b) <= REL * (1.0 + abs(b))


def test_the_suite_has_a_deep_merge_and_a_short_frame():
    bc.check_suite(bc.SMALL_CASES)


@pytest.mark.parametrize("case", bc.OPTION_CASES, ids=lambda c: c.name)
def test_option_twin_matches_reference(case):
    """The blank in the middle and at V - 1, K > V and V < 16: the twin against the reference."""
    w, enc, ref = bc.reference(case)
    bc.check_conditions(case, ref, need_merge=bc.OPTION_NEEDS_MERGE[case.name])
    bc.check_option(case, ref)
    dec = bc.make_decoder(asr, case, w)
    res, margin = dec.beam_search_host(enc, rc.lengths_of(case.model), beam=case.beam, margins=True)
    assert [len(u) for u in res] == [len(u) for u in ref["hyps"]]
    for b, (got, want) in enumerate(zip(res, ref["hyps"])):
        for (tok, ts, score), (rtok, rts, rscore) in zip(got, want):
            assert tok == rtok and ts == rts, b
            assert close(score, rscore), (b, score, rscore)
        assert (np.isinf(margin[b]) and np.isinf(ref["margin"][b])) or \
            abs(margin[b] - ref["margin"][b]) <= 1e-9 * (1 + abs(ref["margin"][b])) + 1e-9 * ref["max_abs_logit"]
    for b, n in enumerate(case.model.lengths):
        if n == 0:
            assert res[b] == [([], [], 0.0)]
    dec.close()


def test_lengths_are_clamped_and_optional():
    """lengths = NULL is every length T; a length above T is T and a negative one 0."""
    case = bc.OPTION_CASES[0]   # s2-bl-k4
    w, enc, _ref = bc.reference(case)
    dec = bc.make_decoder(asr, case, w)
    T, K = enc.shape[0], case.beam
    assert dec.beam_search_host(enc, None, beam=K) == dec.beam_search_host(enc, [T] * enc.shape[1], beam=K)
    wild = dec.beam_search_host(enc, [T + 5, -3, 4, T, 7], beam=K)
    assert wild == dec.beam_search_host(enc, [T, 0, 4, T, 7], beam=K)
    assert wild[1] == [([], [], 0.0)] and max(len(h[0]) for h in wild[0]) > 0
    dec.close()


@pytest.mark.parametrize("case", bc.SMALL_CASES, ids=lambda c: c.name)
def test_twin_matches_reference(case):
    w, enc, ref = bc.reference(case)
    bc.check_conditions(case, ref)
    dec = bc.make_decoder(asr, case, w)
    res, margin = dec.beam_search_host(enc, rc.lengths_of(case.model), beam=case.beam, margins=True)
    assert [len(u) for u in res] == [len(u) for u in ref["hyps"]]
    for b, (got, want) in enumerate(zip(res, ref["hyps"])):
        for (tok, ts, score), (rtok, rts, rscore) in zip(got, want):
            assert tok == rtok and ts == rts, b
            assert close(score, rscore), (b, score, rscore)
        assert (np.isinf(margin[b]) and np.isinf(ref["margin"][b])) or \
            abs(margin[b] - ref["margin"][b]) <= 1e-9 * (1 + abs(ref["margin"][b])) + 1e-9 * ref["max_abs_logit"]
    # a zero-length utterance: one empty hypothesis with score 0
    b0 = case.model.lengths.index(0)
    assert res[b0] == [([], [], 0.0)]
    dec.close()


def test_beam_one_is_greedy_with_one_symbol_per_frame():
    case = bc.SMALL_CASES[0]
    w, enc = rc.make_model(case.model)
    dec = bc.make_decoder(asr, case, w)          # max_symbols = 1
    ln = rc.lengths_of(case.model)
    greedy, _state, cnt = dec.decode_host(enc, ln)
    beam = dec.beam_search_host(enc, ln, beam=1)
    assert int(cnt.sum()) > 0
    for b in range(enc.shape[1]):
        assert len(beam[b]) == 1
        assert beam[b][0][0] == greedy[b][0] and beam[b][0][1] == greedy[b][1]
        assert close(beam[b][0][2], greedy[b][3])
    dec.close()


def test_truncation_at_max_out_and_nbest():
    case = bc.SMALL_CASES[3]   # s2-k4-a
    w, enc, ref = bc.reference(case)
    dec = bc.make_decoder(asr, case, w)
    ln = rc.lengths_of(case.model)
    full = dec.beam_search_host(enc, ln, beam=case.beam)
    assert max(n for u in ref["lens"] for n in u) > 2
    for max_out in (0, 2):
        res = dec.beam_search_host(enc, ln, beam=case.beam, max_out=max_out)
        for b in range(len(res)):
            assert len(res[b]) == len(full[b])
            for (tok, ts, score), (ftok, fts, fscore) in zip(res[b], full[b]):
                assert tok == ftok[:max_out] and ts == fts[:max_out] and score == fscore
    two = dec.beam_search_host(enc, ln, beam=case.beam, nbest=2)
    assert [u for u in two] == [u[:2] for u in full]
    # the uncut lengths through the C ABI
    T, B = enc.shape[0], enc.shape[1]
    K = case.beam
    tok, ts = np.zeros((B, K, 2), np.int32), np.zeros((B, K, 2), np.int32)
    hl, sc, nh = np.zeros((B, K), np.int32), np.zeros((B, K), np.float64), np.zeros(B, np.int32)
    p = asr._ptr
    assert asr.lib().asr_rnnt_beam_host(dec.h, p(np.ascontiguousarray(enc, np.float32)), p(ln), T, B, K, K, 2, p(tok),
                                        p(ts), p(hl), p(sc), p(nh), None) == asr.ASR_OK
    assert [hl[b, :nh[b]].tolist() for b in range(B)] == ref["lens"]
    dec.close()


def test_nbest_goes_through_mbr_and_edit_distance():
    case = bc.SMALL_CASES[4]
    w, enc, _ref = bc.reference(case)
    dec = bc.make_decoder(asr, case, w)
    res = dec.beam_search_host(enc, rc.lengths_of(case.model), beam=case.beam)
    lists = [[tok for tok, _ts, _s in u] for u in res]
    weights = [[s for _tok, _ts, s in u] for u in res]
    risks, best, dist = asr.nbest_mbr(lists, weights, host=True)
    assert len(risks) == len(res) and all(len(r) == len(u) for r, u in zip(risks, res))
    assert all(0 <= best[b] < len(res[b]) for b in range(len(res)))
    b = max(range(len(res)), key=lambda i: len(res[i]))
    d = asr.edit_distance([lists[b][0]] * len(lists[b]), lists[b], host=True)
    assert d[0] == 0 and d.tolist() == dist[b][0].tolist()
    dec.close()


def test_refusals():
    case = bc.SMALL_CASES[0]
    w = rc.make_model(case.model)[0]
    T, B, E, D, Hp, J, V, L = case.model.shape
    dec = bc.make_decoder(asr, case, w)
    lib = asr.lib()
    assert lib.asr_rnnt_beam_workspace_bytes(None, 1, 1, 1) == 0
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 17), (1 << 30, 4, 1), (1 << 30, 1, 16)):
        assert dec.beam_workspace_bytes(*bad) == 0, bad
    # f, the slices of ceil(B / (16 / R)) workgroups, the node tables
    assert dec.beam_workspace_bytes(3, 17, 1) == 4 * (3 * 17 * J + 2 * 16 * (2 * L * Hp + J + V)) + 16 * 17 * (3 + 1)
    assert dec.beam_workspace_bytes(3, 5, 3) == 4 * (3 * 5 * J + 2 * 16 * (2 * L * Hp + J + V)) + 16 * 5 * (9 + 1)
    assert dec.beam_workspace_bytes(3, 5, 9) == 4 * (3 * 5 * J + 5 * 16 * (2 * L * Hp + J + V)) + 16 * 5 * (27 + 1)
    enc = np.zeros((2, 2, E), np.float32)
    i32, f64 = np.zeros(64, np.int32), np.zeros(64, np.float64)
    p = asr._ptr
    #       h      enc     len   T  B  K  nbest max_out tokens timesteps len   score   nhyp
    good = [dec.h, p(enc), None, 2, 2, 4, 2, 3, p(i32), p(i32), p(i32), p(f64), p(i32)]

    def both(i, value, want):
        a = list(good)
        a[i] = value
        assert lib.asr_rnnt_beam_host(*a, None) == want, (i, value)
        assert lib.asr_rnnt_beam(*a, p(f64), None) == want, (i, value)    # refused before any HIP call

    for i in (0, 1, 8, 9, 10, 11, 12):
        both(i, None, asr.ASR_ERR_ARG)
    both(3, 0, asr.ASR_ERR_ARG)
    both(4, 0, asr.ASR_ERR_ARG)
    both(5, 0, asr.ASR_ERR_ARG)
    both(5, 17, asr.ASR_ERR_ARG)
    both(6, 0, asr.ASR_ERR_ARG)
    both(6, 5, asr.ASR_ERR_ARG)          # nbest > K
    both(7, -1, asr.ASR_ERR_ARG)
    both(3, 1 << 30, asr.ASR_ERR_UNSUPPORTED)       # T * B and T * K + 1
    a = list(good)
    a[7], a[8], a[9] = 0, None, None                # max_out = 0 needs no token arrays
    assert lib.asr_rnnt_beam_host(*a, None) == asr.ASR_OK
    assert lib.asr_rnnt_beam(*good, None, None) == asr.ASR_ERR_ARG          # no workspace
    assert lib.asr_rnnt_beam(*good, p(f64), None) == asr.ASR_ERR_STATE      # not uploaded
    assert lib.asr_rnnt_beam_host(*good, None) == asr.ASR_OK
    with pytest.raises(ValueError):
        dec.beam_search_host(np.zeros((2, 2, E + 1), np.float32))
    dec.close()
    # the search kernel's LDS limit, 64 * (2 L (Hp + 4) + (J + 4)) + 8192 <= 160 KiB, is the call's to refuse:
    # Hp = J = 816 can be created (the greedy limit) and searched on the host, not on the device
    big = rc.Case("big", (1, 1, 8, 16, 816, 816, 3, 1), 0, 1, "relu", (1,), 0, 1.0, 0.0)
    dec = rc.make_decoder(asr, big)
    enc = np.zeros((1, 1, 8), np.float32)
    args = [dec.h, p(enc), None, 1, 1, 1, 1, 1, p(i32), p(i32), p(i32), p(f64), p(i32)]
    assert lib.asr_rnnt_beam(*args, p(f64), None) == asr.ASR_ERR_UNSUPPORTED
    assert lib.asr_rnnt_beam_host(*args, None) == asr.ASR_OK
    dec.close()
