"""GPU checks of the transducer decode kernel (asr_rnnt_greedy) against
tests/rnnt_reference.py: tokens, timesteps and counts exactly, log-probs within
the LSTM tests' bound; exact ties, batch independence, streaming, zero-length
utterances and truncation.

Measured on an MI355X (max over the case of |gpu - ref| / (1 + |ref|) per token
log-prob, and of |gpu - ref| / ((1 + |ref|) * terms) for the totals) are in
DESIGN.md §24; the bound is 2e-5."""
import numpy as np
import pytest

import rnnt_cases as rc
from conftest import asr
from rnnt_reference import Reference

pytestmark = pytest.mark.gpu

TOL = 2e-5    # the LSTM tests' bound: |gpu - ref| <= TOL * (1 + |ref|)


@pytest.fixture(scope="module", autouse=True)
def _device():
    asr.set_device(0)


def terms_of(case, ref, b):
    """Joint evaluations summed into utterance b's total: its emissions, and one
    blank for every frame that did not hit the cap."""
    return ref["count"][b] + sum(1 for n in ref["frames"][b] if n < case.max_symbols)


@pytest.mark.parametrize("case", rc.SMALL_CASES + rc.LARGE_CASES, ids=lambda c: c.name)
def test_kernel_matches_reference(case):
    w, enc, ref = rc.reference(case)
    rc.check_conditions(case, ref)
    dec = rc.make_decoder(asr, case, w)
    ln = rc.lengths_of(case)
    res, state, cnt = dec.decode(enc, ln)
    host, _hs, hcnt = dec.decode_host(enc, ln)
    err_lp = err_total = 0.0
    for b, (tok, ts, lp, total) in enumerate(res):
        rl = np.asarray(ref["logps"][b], np.float64)
        if len(lp) == len(rl) and len(lp):
            err_lp = max(err_lp, float(np.max(np.abs(lp - rl) / (1 + np.abs(rl)))))
        err_total = max(err_total, abs(total - ref["total"][b]) /
                        ((1 + abs(ref["total"][b])) * max(terms_of(case, ref, b), 1)))
    print(f"rnnt {case.name}: max logp err {err_lp:.3e}, max total err per term {err_total:.3e} (bound {TOL:.0e})")
    assert cnt.tolist() == ref["count"]
    for b, (tok, ts, lp, total) in enumerate(res):
        assert tok == ref["tokens"][b] and ts == ref["timesteps"][b], b
        assert tok == host[b][0] and ts == host[b][1], b       # decode matches decode_host in tokens
    assert hcnt.tolist() == cnt.tolist()
    assert err_lp <= TOL and err_total <= TOL
    assert np.all(np.abs(state - ref["state"]) <= TOL * (1 + np.abs(ref["state"])))
    dec.close()


SMALL = (8, 5, 12, 16, 32, 32, 17, 1)    # T, B, E, D, Hp, J, V, L


def _tie_case(blank, src, dup):
    case = rc.Case("tie", SMALL, blank, 3, "relu", (8, 8, 5, 8, 3), 10, 4.0, 1.5)
    w, enc = rc.make_model(case)
    w["w_out"][:, dup] = w["w_out"][:, src]
    w["b_out"][dup] = w["b_out"][src]
    return case, w, enc


@pytest.mark.parametrize("blank,src,dup,winner,loser", [
    (8, 8, 12, 8, 12),     # blank tied with a token above it: blank wins
    (8, 8, 3, 3, 8),       # blank tied with a token below it: the token wins
    (8, 2, 14, 2, 14),     # two tokens
    (0, 0, 16, 0, 16),     # blank at 0 against the last column
    (16, 16, 0, 0, 16),    # blank last against column 0
])
def test_exact_tie_goes_to_the_lower_index(blank, src, dup, winner, loser):
    case, w, enc = _tie_case(blank, src, dup)
    ref = Reference(w, blank, case.act, case.max_symbols).decode(enc, case.lengths)
    assert min(ref["gap"]) == 0.0           # the tied pair was the maximum somewhere on the reference's walk
    # every other choice of the walk is away from a near-tie: the same model with the losing column pushed down
    w2 = dict(w, b_out=w["b_out"].copy())
    w2["b_out"][loser] -= 30.0
    ref2 = Reference(w2, blank, case.act, case.max_symbols).decode(enc, case.lengths)
    assert ref2["tokens"] == ref["tokens"] and min(ref2["gap"]) >= 1e-3 * (1 + ref["max_abs_logit"])
    dec = rc.make_decoder(asr, case, w)
    res, _state, cnt = dec.decode(enc, rc.lengths_of(case))
    assert cnt.tolist() == ref["count"]
    seen = set()
    for b, (tok, ts, _lp, _total) in enumerate(res):
        assert tok == ref["tokens"][b] and ts == ref["timesteps"][b]
        seen.update(tok)
    assert loser == blank or loser not in seen
    if winner != blank:
        assert winner in seen
    else:
        assert any(n < case.max_symbols for f in ref["frames"] for n in f)   # blank did win
    dec.close()


def _model(shape, seed, blank=0, ms=3, act="relu", bias=3.0, lengths=None):
    T, B = shape[0], shape[1]
    case = rc.Case("adhoc", shape, blank, ms, act, tuple(lengths) if lengths is not None else (T,) * B, seed, 4.0, bias)
    w, enc = rc.make_model(case)
    return case, w, enc


def test_batch_independent():
    """37 utterances, then the first 5 alone: equal bits."""
    case, w, enc = _model((6, 37, 12, 16, 48, 32, 19, 2), 3, act="tanh", bias=2.0)
    dec = rc.make_decoder(asr, case, w)
    ln = np.array([6, 0, 3, 6, 5] + [6] * 32, np.int32)
    r37, s37, c37 = dec.decode(enc, ln)
    r5, s5, c5 = dec.decode(np.ascontiguousarray(enc[:, :5]), ln[:5])
    assert c37[:5].tolist() == c5.tolist() and int(c5.sum()) > 0
    for b in range(5):
        assert r37[b][0] == r5[b][0] and r37[b][1] == r5[b][1]
        assert np.array_equal(r37[b][2], r5[b][2]) and r37[b][3] == r5[b][3]
    assert np.array_equal(s37[:, :, :5], s5)
    dec.close()


@pytest.mark.parametrize("shape,act", [((12, 5, 12, 16, 48, 32, 19, 2), "tanh"), ((12, 18, 8, 16, 32, 48, 33, 1), "relu")])
def test_streaming_equals_whole(shape, act):
    """T = 12 cut as 5 + 4 + 3 with the state carried: the whole decode bit for bit."""
    T, B = shape[0], shape[1]
    ln = np.array(([12, 0, 7, 12, 9] * 4)[:B], np.int32)
    case, w, enc = _model(shape, 4, blank=shape[6] - 1, act=act, bias=2.0, lengths=ln)
    dec = rc.make_decoder(asr, case, w)
    whole, wstate, wcnt = dec.decode(enc, ln)
    assert 0 < int(wcnt.sum()) < T * B * case.max_symbols
    state, parts, totals = None, [([], [], []) for _ in range(B)], np.zeros(B)
    for t0, t1 in ((0, 5), (5, 9), (9, 12)):
        res, state, _c = dec.decode(np.ascontiguousarray(enc[t0:t1]), np.clip(ln - t0, 0, t1 - t0), state=state)
        for b, (tok, ts, lp, total) in enumerate(res):
            parts[b][0].extend(tok), parts[b][1].extend(t + t0 for t in ts), parts[b][2].extend(lp.tolist())
            totals[b] += total
    for b in range(B):
        assert parts[b][0] == whole[b][0] and parts[b][1] == whole[b][1]
        assert parts[b][2] == whole[b][2].tolist()
        assert abs(totals[b] - whole[b][3]) <= 1e-12 * (1 + abs(whole[b][3]))   # fp64 sums of the same fp32 terms
    assert np.array_equal(state, wstate)
    dec.close()


def test_zero_length_utterance_keeps_the_start_state():
    case, w, enc = _model((5, 4, 12, 16, 32, 32, 17, 2), 6, act="tanh", bias=2.0)
    dec = rc.make_decoder(asr, case, w)
    ln = np.array([5, 0, 5, 0], np.int32)
    res, state, cnt = dec.decode(enc, ln)
    assert cnt[1] == 0 and cnt[3] == 0 and cnt[0] + cnt[2] > 0
    assert res[1] == ([], [], res[1][2], 0.0) and len(res[1][2]) == 0
    # the start state: zeros, then one predictor step on Emb[blank]
    ref = Reference(w, case.blank, case.act, case.max_symbols).decode(enc, ln)
    assert np.all(np.abs(state[:, :, 1] - ref["state"][:, :, 1]) <= TOL * (1 + np.abs(ref["state"][:, :, 1])))
    assert np.array_equal(state[:, :, 1], state[:, :, 3])
    _r, alone, _c = dec.decode(enc, np.zeros(4, np.int32))
    assert np.array_equal(alone[:, :, 0], state[:, :, 1])
    assert np.any(state[:, :, 1] != 0)
    dec.close()


def test_truncation_at_max_out():
    case = rc.SMALL_CASES[6]   # s2-b0-m3
    w, enc, ref = rc.reference(case)
    dec = rc.make_decoder(asr, case, w)
    ln = rc.lengths_of(case)
    full, state, cnt = dec.decode(enc, ln)
    assert cnt.tolist() == ref["count"] and max(ref["count"]) > 2
    for max_out in (0, 2):
        res, st, c = dec.decode(enc, ln, max_out=max_out)
        assert c.tolist() == ref["count"] and any(x > max_out for x in c)   # the count goes on
        for b in range(len(res)):
            n = min(max_out, ref["count"][b])
            assert res[b][0] == ref["tokens"][b][:n] and res[b][1] == ref["timesteps"][b][:n]
            assert np.array_equal(res[b][2], full[b][2][:n])
            assert res[b][3] == full[b][3]
        assert np.array_equal(st, state)    # the walk and the state went on
    dec.close()
