"""The token-and-duration transducer's host twin (asr_rnnt_greedy_tdt_host)
against the float64 reference of rnnt_tdt_cases.py, and the refusals of the
asr_rnnt_*tdt* entry points and of the entry points that take no TDT handle.
No GPU."""
import numpy as np
import pytest

import asr_amd as asr
import rnnt_cases as rc
import rnnt_tdt_cases as tc

TIGHT = 1e-9     # fp64 twin against fp64 reference, relative to 1 + |ref|


@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c.name)
def test_twin_matches_reference(case):
    w, enc, ref = tc.reference(case)
    tc.check_conditions(case, ref)
    dec = tc.make_decoder(asr, case, w)
    assert dec.durations == list(case.durations)
    res, state, cnt, gaps = dec.decode_host(enc, tc.lengths_of(case), gaps=True)
    tc.compare_exact(case, res, state, cnt, ref)
    assert np.allclose(state[0], ref["state"][0], rtol=0, atol=TIGHT)
    for b, (_tok, _ts, lp, total, _dur) in enumerate(res):
        assert np.allclose(lp, ref["logps"][b], rtol=0, atol=TIGHT * (1 + np.abs(ref["logps"][b]).max(initial=0)))
        assert abs(total - ref["total"][b]) <= TIGHT * (1 + abs(ref["total"][b])) * max(2 * ref["evals"][b], 1)
        for got, want in ((gaps[0, b], ref["gap"][b]), (gaps[1, b], ref["dgap"][b])):
            assert got == want if np.isinf(want) else abs(got - want) <= TIGHT * (1 + ref["max_abs_logit"])


def test_the_table_holds_every_kind_of_step():
    """A blank with dur > 1, a blank with dur = 0, a token with dur = 0, one with dur > 0, a frame that hits
    max_symbols and a walk that ends past its utterance: each occurs in some case's reference walk."""
    seen = set().union(*(tc.kinds_of(tc.reference(c)[2]) for c in tc.CASES if c.name != "8-c640"))
    assert seen >= set(tc.KINDS), set(tc.KINDS) - seen


def test_chunked_twin_equals_whole():
    """Case 4 at T = 12 cut 5 + 4 + 3, the state and the skip passed on: every output equals the whole decode's."""
    case = tc.by_name("4-unordered")._replace(shape=(12,) + tc.by_name("4-unordered").shape[1:], lengths=(12, 0, 7, 12, 10))
    w, enc = tc.make_model(case)
    dec, ln = tc.make_decoder(asr, case, w), tc.lengths_of(case)
    tc.check_chunked(lambda e, n, st: dec.decode_host(e, n, state=st), enc, ln)


@pytest.mark.parametrize("durations", [[], list(range(17)), [0, 0], [0, -1], [1, 32768]])
def test_a_bad_duration_table_is_refused(durations):
    case = tc.by_name("1-one-tile")._replace(durations=tuple(durations))
    w = tc.make_model(case._replace(durations=tuple(durations) or (0,)))[0]
    if not durations:
        w["w_dur"], w["b_dur"] = w["w_dur"][:, :0], w["b_dur"][:0]
    with pytest.raises(asr.AsrError) as e:
        tc.make_decoder(asr, case, w)
    assert e.value.status == asr.ASR_ERR_ARG


def test_a_handle_of_the_wrong_kind_is_refused():
    """ASR_ERR_UNSUPPORTED before any HIP call, both ways round: the entry points of the one-softmax lattice on a
    TDT handle, and the TDT pair on an LSTM and on a stateless handle."""
    case = tc.by_name("4-unordered")
    w, enc = tc.make_model(case)
    dec, ln = tc.make_decoder(asr, case, w), tc.lengths_of(case)
    plain = rc.make_decoder(asr, case, {k: v for k, v in w.items() if k not in ("w_dur", "b_dur")})
    x, buf = np.zeros(64, np.float64), np.zeros(16, np.int32)
    p = asr._ptr(x)
    lib = asr.lib()
    assert lib.asr_rnnt_tdt_durations(dec.h, asr._ptr(buf)) == 4 and buf[:4].tolist() == [1, 0, 4, 2]
    assert lib.asr_rnnt_tdt_durations(plain.h, None) == 0 and lib.asr_rnnt_tdt_durations(None, None) == 0
    assert dec.workspace_bytes(9, 5) == plain.workspace_bytes(9, 5) > 0
    head = (p, None, 1, 1, 1, None, None)
    assert lib.asr_rnnt_greedy(dec.h, *head, p, p, p, p, p, p, None) == asr.ASR_ERR_UNSUPPORTED
    assert lib.asr_rnnt_greedy_host(dec.h, *head, p, p, p, p, p, None) == asr.ASR_ERR_UNSUPPORTED
    assert lib.asr_rnnt_greedy_stateless(dec.h, *head, p, p, p, p, p, p, None) == asr.ASR_ERR_UNSUPPORTED
    assert lib.asr_rnnt_greedy_tdt(plain.h, *head, None, None, p, p, p, p, p, p, p, None) == asr.ASR_ERR_UNSUPPORTED
    assert lib.asr_rnnt_greedy_tdt_host(plain.h, *head, None, None, p, p, p, p, p, p, None, None) == \
        asr.ASR_ERR_UNSUPPORTED
    assert lib.asr_rnnt_greedy_tdt(dec.h, *head, None, None, p, p, None, p, p, p, p, None) == asr.ASR_ERR_ARG
    assert lib.asr_rnnt_greedy_tdt(dec.h, *head, None, None, p, p, p, p, p, p, p, None) == asr.ASR_ERR_STATE
    for call in (lambda: dec.beam_search_host(enc, ln, beam=2), lambda: dec.score_host(enc, [[1]], ln, [0]),
                 lambda: dec.align_host(enc, [[1]], ln, [0], "standard")):
        with pytest.raises(asr.AsrError) as e:
            call()
        assert e.value.status == asr.ASR_ERR_UNSUPPORTED
