"""The stateless-predictor transducer's kernels (asr_rnnt_greedy_stateless and the
RT_PRED_CTX forms of asr_rnnt_beam / asr_rnnt_beam_lm / asr_rnnt_align) against
the float64 references of rnnt_stateless_cases.py, and the invariants between
the kernels.  Bounds: test_rnnt_gpu.py's, test_rnnt_beam_gpu.py's and
rnnt_align_cases.py's, unchanged (the joint is the same arithmetic and a context
table is one more fp32-accurate GEMM)."""
import math

import numpy as np
import pytest

import asr_amd as asr
import rnnt_align_cases as ac
import rnnt_cases as rc
import rnnt_lm_cases as lc
import rnnt_stateless_cases as sc

pytestmark = pytest.mark.gpu
TOL = 2e-5    # test_rnnt_gpu.py's: |gpu - ref| <= TOL * (1 + |ref|), per term for a total


@pytest.fixture(autouse=True)
def _device():
    asr.set_device(0)


@pytest.mark.parametrize("case", sc.GREEDY_CASES, ids=lambda c: c.name)
def test_greedy_kernel_matches_reference(case):
    w, enc, ref = sc.reference(case)
    rc.check_conditions(case, ref)
    dec = sc.make_decoder(asr, case, w)
    res, ctx, cnt = dec.decode(enc, sc.lengths_of(case))
    assert cnt.tolist() == ref["count"]
    assert np.array_equal(ctx, sc._ref(sc.StatelessReference, case, w, 1).context_of(ref["state"]))
    err_lp = err_total = 0.0
    for b, (tok, ts, lp, total) in enumerate(res):
        assert tok == ref["tokens"][b] and ts == ref["timesteps"][b], (case.name, b)
        want = np.asarray(ref["logps"][b], np.float64)
        if len(want):
            err_lp = max(err_lp, float(np.max(np.abs(lp - want) / (1 + np.abs(want)))))
        terms = max(sum(ref["frames"][b]) + len(ref["frames"][b]), 1)
        err_total = max(err_total, abs(total - ref["total"][b]) / ((1 + abs(ref["total"][b])) * terms))
    print(f"rnnt stateless greedy {case.name}: max logp err {err_lp:.3e}, total err per term {err_total:.3e}")
    assert err_lp <= TOL and err_total <= TOL


@pytest.mark.parametrize("name,beam", sc.BEAMS)
def test_beam_kernel_matches_reference(name, beam):
    case, w, enc, ref = sc.beam_reference(name, beam)
    sc.check_beam_conditions(name, beam, ref)
    res = sc.make_decoder(asr, case, w).beam_search(enc, sc.lengths_of(case), beam=beam)
    assert [[(h[0], h[1]) for h in u] for u in res] == [[(h[0], h[1]) for h in u] for u in ref["hyps"]]
    err = max((abs(h[2] - r[2]) / ((1 + abs(r[2])) * max(frames, 1))
               for u, ru, frames in zip(res, ref["hyps"], ref["frames"]) for h, r in zip(u, ru)), default=0.0)
    print(f"rnnt stateless beam {name} K={beam}: max score err per frame {err:.3e}")
    assert err <= TOL


@pytest.mark.parametrize("topology", ac.TOPOLOGIES)
@pytest.mark.parametrize("name", sorted(sc.ALIGN_SPEC))
def test_align_kernels_match_reference(name, topology):
    case, w, enc, targets, utt, ref = sc.align_reference(name, topology)
    score, vscore, frames = sc.make_decoder(asr, case, w).align(enc, targets, sc.lengths_of(case), utt, topology)
    for n, r in enumerate(ref):
        assert ac.frames_comparable(r), (name, n)
        for g, want in ((score[n], r["score"]), (vscore[n], r["vscore"])):
            assert g == want if math.isinf(want) else abs(g - want) <= ac.bound(want, r["terms"]), (name, n, g, want)
        assert frames[n].tolist() == r["frames"], (name, n)


def test_lm_fused_beam_kernel_matches_reference():
    """Non-zero weights: test_rnnt_lm_gpu.py's comparison and bound, and the twin's bits for the LM parts."""
    case, w, enc, ref = sc.lm_reference()
    dec, lm, ln = sc.make_decoder(asr, case.model, w), lc.make_lm(asr, case), sc.lengths_of(case.model)
    res = dec.beam_search(enc, ln, lm=lm, **lc.search_kwargs(case))
    lc.compare("stateless " + case.name, res, ref, lambda g, r, frames: abs(g - r) / ((1 + abs(r)) * max(frames, 1)), TOL)
    host = dec.beam_search_host(enc, ln, lm=lm, **lc.search_kwargs(case))
    for got, want in zip(res, host):
        assert [(g[0], g[1], g[4], g[5]) for g in got] == [(h[0], h[1], h[4], h[5]) for h in want]


def test_infeasible_targets_and_zero_length_utterances():
    """test_rnnt_align_gpu.py's case on a stateless handle: a blank, an out-of-range and a negative label, an
    utterance outside [0, B), a zero-length utterance, and U > len in the one-per-frame lattice."""
    case = sc.by_name("ragged-c2")      # T = 9, lengths [9, 0, 4, 9, 7], blank 0, V = 17
    w, enc = sc.make_model(case)
    dec, ln = sc.make_decoder(asr, case, w), sc.lengths_of(case)
    good = [3, 5, 7]
    targets = [good, [3, 0, 7], [3, 17, 7], [3, -1, 7], good, good, [], good, good, [1, 2, 3, 4, 5]]
    utt = [0, 0, 0, 0, -1, 5, 1, 1, 2, 2]
    for topology in ac.TOPOLOGIES:
        score, vscore, frames = dec.align(enc, targets, ln, utt, topology)
        hs, _hv, hf = dec.align_host(enc, targets, ln, utt, topology)
        for n in (1, 2, 3, 4, 5, 7):
            assert score[n] == -math.inf and vscore[n] == -math.inf and frames[n].tolist() == [-1, -1, -1], (topology, n)
        assert score[6] == 0.0 and vscore[6] == 0.0 and math.isfinite(score[0])
        assert (score[9] == -math.inf) == (topology == "one_per_frame")
        for n in range(len(targets)):
            assert math.isinf(hs[n]) == math.isinf(score[n]) and frames[n].tolist() == hf[n].tolist(), (topology, n)
            if math.isfinite(hs[n]):
                assert abs(score[n] - hs[n]) <= ac.bound(hs[n], int(ln[utt[n]]) + len(targets[n]))


def test_beam_one_is_the_greedy_kernel():
    case = sc.by_name("ragged-c2")._replace(max_symbols=1)
    w, enc = sc.make_model(case)
    dec, ln = sc.make_decoder(asr, case, w), sc.lengths_of(case)
    res, _ctx, cnt = dec.decode(enc, ln)
    beam = dec.beam_search(enc, ln, beam=1)
    assert int(cnt.sum()) > 0
    for (tok, ts, _lp, total), u in zip(res, beam):
        assert u[0][0] == tok and u[0][1] == ts and u[0][2] == total     # equal bits


def test_chunked_decode_equals_whole():
    case = sc.by_name("ragged-c2")
    w, enc = sc.make_model(case)
    dec = sc.make_decoder(asr, case, w)
    sc.check_chunked(lambda e, ln, st: dec.decode(e, ln, state=st), case, enc)


def test_batch_independent():
    """37 utterances, then the first 5 alone: equal bits."""
    case = sc.by_name("ragged-c2")._replace(shape=(9, 37) + sc.RAGGED[2:], lengths=tuple([9, 0, 4, 9, 7] * 7 + [9, 3]))
    w, enc = sc.make_model(case)
    dec, ln = sc.make_decoder(asr, case, w), sc.lengths_of(case)
    r37, c37, n37 = dec.decode(enc, ln)
    r5, c5, n5 = dec.decode(np.ascontiguousarray(enc[:, :5]), ln[:5])
    assert n37[:5].tolist() == n5.tolist() and int(n5.sum()) > 0 and np.array_equal(c37[:5], c5)
    for x, y in zip(r37[:5], r5):
        assert x[0] == y[0] and x[1] == y[1] and np.array_equal(x[2], y[2]) and x[3] == y[3]
    b37, b5 = dec.beam_search(enc, ln, beam=3), dec.beam_search(np.ascontiguousarray(enc[:, :5]), ln[:5], beam=3)
    assert b37[:5] == b5


def test_zero_lm_weights_give_the_unfused_beam():
    """A stateless handle fused with an LM at alpha = beta = 0: the unfused search byte for byte."""
    lm_case = lc.SMALL_CASES[0]
    case = sc.by_name("ragged-c2")
    w, enc = sc.make_model(case)
    dec, ln = sc.make_decoder(asr, case, w), sc.lengths_of(case)
    lm = lc.make_lm(asr, lm_case)
    V = case.shape[6]
    tok = [-1 if v == case.blank else v % 5 for v in range(V)]
    plain = dec.beam_search(enc, ln, beam=4)
    fused = dec.beam_search(enc, ln, beam=4, lm=lm, alpha=0.0, beta=0.0, tok_of_label=tok, bos=False, eos=False)
    assert sum(len(h[0]) for u in plain for h in u) > 0
    assert [[(h[0], h[1], h[2]) for h in u] for u in fused] == [[(h[0], h[1], h[2]) for h in u] for u in plain]
    assert all(h[3] == h[2] for u in fused for h in u)      # am = total


@pytest.mark.parametrize("blank_last", [False, True])
def test_exact_logit_tie_goes_to_the_lower_index(blank_last):
    """Label 5 is label 3's copy (equal W_out columns and biases), lifted so the pair is the maximum: 3 wins."""
    case = sc.by_name("ragged-c2")._replace(blank=16 if blank_last else 0)
    w, enc = sc.make_model(case)
    w["w_out"][:, 5], w["b_out"][5] = w["w_out"][:, 3], 3.0
    w["b_out"][3] = 3.0
    ref = sc._ref(sc.StatelessReference, case, w, 3).decode(enc, case.lengths)
    assert min(ref["gap"]) == 0.0 and any(3 in t for t in ref["tokens"])
    res, _ctx, cnt = sc.make_decoder(asr, case, w).decode(enc, sc.lengths_of(case))
    assert cnt.tolist() == ref["count"]
    assert [r[0] for r in res] == ref["tokens"] and not any(5 in r[0] for r in res)
