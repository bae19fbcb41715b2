"""CPU checks of the LM-fused transducer beam search (asr_rnnt_lm_*,
asr_rnnt_beam_lm*): the fp64 host twin asr_rnnt_beam_lm_host against
tests/rnnt_lm_reference.py, zero weights against asr_rnnt_beam_host, K = 1
against the greedy twin, truncation, every refusal in its order, the Python
keywords and lm_rescore against asr_lm_score_host.  No GPU is needed or used."""
import numpy as np
import pytest

import rnnt_cases as rc
import rnnt_lm_cases as lc
from conftest import asr

REL = 1e-9   # the project's oracle bound: both sides are fp64 and differ in summation order only


def rel(got, want, _frames):
    return abs(got - want) / (1.0 + abs(want))


def test_the_suite_meets_its_conditions():
    lc.check_suite(lc.SMALL_CASES)


@pytest.mark.parametrize("case", lc.SMALL_CASES, ids=lambda c: c.name)
def test_twin_matches_reference(case):
    w, enc, ref, _plain = lc.reference(case)
    lc.check_conditions(case, ref)
    dec = lc.make_decoder(asr, case, w)
    lm = lc.make_lm(asr, case)
    res, margin = dec.beam_search_host(enc, rc.lengths_of(case.model), margins=True, lm=lm, **lc.search_kwargs(case))
    lc.compare(case.name, res, ref, rel, REL)
    for b in range(len(res)):
        assert (np.isinf(margin[b]) and np.isinf(ref["margin"][b])) or \
            abs(margin[b] - ref["margin"][b]) <= 1e-9 * (1 + abs(ref["margin"][b])) + 1e-9 * ref["max_abs_logit"]
    # a zero-length utterance: one empty hypothesis with am = 0 and total 0 or the </s> term
    b0 = case.model.lengths.index(0)
    assert len(res[b0]) == 1
    tok, ts, total, am, lml, n = res[b0][0]
    assert (tok, ts, am, n) == ([], [], 0.0, 0)
    if case.eos:
        v_eos = lm.score([[]], bos=case.bos, eos=True, host=True)[0][0]
        assert lml == v_eos and total == 0.0 + (float(np.float32(case.alpha)) * 2.302585092994046) * v_eos
    else:
        assert total == 0.0 and lml == 0.0
    dec.close()


@pytest.mark.parametrize("case", lc.OPTION_CASES, ids=lambda c: c.name)
def test_option_twin_matches_reference(case):
    """The moved blank, both flags and neither, beta < 0, a zero weight, K > V and the order-8 model: the twin
    against the reference."""
    w, enc, ref, _plain = lc.reference(case)
    lc.check_conditions(case, ref, need_merge=lc.OPTION_NEEDS_MERGE[case.name])
    lc.check_option(case)
    dec = lc.make_decoder(asr, case, w)
    lm = lc.make_lm(asr, case)
    res, margin = dec.beam_search_host(enc, rc.lengths_of(case.model), margins=True, lm=lm, **lc.search_kwargs(case))
    lc.compare(case.name, res, ref, rel, REL)
    for b in range(len(res)):
        assert (np.isinf(margin[b]) and np.isinf(ref["margin"][b])) or \
            abs(margin[b] - ref["margin"][b]) <= 1e-9 * (1 + abs(ref["margin"][b])) + 1e-9 * ref["max_abs_logit"]
    assert [[len(h[0]) for h in u] for u in res] == ref["lens"]
    dec.close()


def _raw_host(dec, fuse, enc, ln, K, nbest, max_out):
    """Every output array of asr_rnnt_beam_lm_host (fuse) or asr_rnnt_beam_host (None)."""
    enc = np.ascontiguousarray(enc, np.float32)
    T, B = enc.shape[0], enc.shape[1]
    mo = max(max_out, 1)
    tok, ts = np.zeros((B, nbest, mo), np.int32), np.zeros((B, nbest, mo), np.int32)
    hl, nh, nt = np.zeros((B, nbest), np.int32), np.zeros(B, np.int32), np.zeros((B, nbest), np.int32)
    tot, am, lml = (np.zeros((B, nbest), np.float64) for _ in range(3))
    p = asr._ptr
    if fuse is None:
        rc_ = asr.lib().asr_rnnt_beam_host(dec.h, p(enc), p(ln), T, B, K, nbest, max_out, p(tok), p(ts), p(hl), p(tot),
                                           p(nh), None)
    else:
        rc_ = asr.lib().asr_rnnt_beam_lm_host(fuse, p(enc), p(ln), T, B, K, nbest, max_out, p(tok), p(ts), p(hl),
                                              p(tot), p(am), p(lml), p(nt), p(nh), None)
    assert rc_ == asr.ASR_OK
    return tok, ts, hl, tot, nh, am, lml, nt


@pytest.mark.parametrize("case", [lc.SMALL_CASES[1], lc.SMALL_CASES[3]], ids=lambda c: c.name)
def test_zero_weights_are_the_unfused_search(case):
    w, enc, _ref, _plain = lc.reference(case)
    dec = lc.make_decoder(asr, case, w)
    lm = lc.make_lm(asr, case)
    ln = rc.lengths_of(case.model)
    fuse = dec._lm_handle(lm, 0.0, 0.0, lc.tok_of_label(case), case.bos, False)
    K, T = case.beam, enc.shape[0]
    fused, plain = _raw_host(dec, fuse, enc, ln, K, K, T), _raw_host(dec, None, enc, ln, K, K, T)
    assert int(plain[4].sum()) > enc.shape[1]
    for i in range(5):
        assert np.array_equal(fused[i], plain[i]), i
    assert np.array_equal(fused[5], plain[3]) and np.array_equal(fused[7], plain[2])
    dec.close()


def test_beam_one_is_greedy_under_a_zero_lm():
    case = lc.SMALL_CASES[0]
    w, enc = rc.make_model(case.model)
    dec = lc.make_decoder(asr, case, w)          # max_symbols = 1
    lm = lc.make_lm(asr, case)
    ln = rc.lengths_of(case.model)
    greedy, _state, cnt = dec.decode_host(enc, ln)
    beam = dec.beam_search_host(enc, ln, beam=1, lm=lm, alpha=0.0, beta=0.0, tok_of_label=lc.tok_of_label(case))
    assert int(cnt.sum()) > 0
    for b in range(enc.shape[1]):
        assert len(beam[b]) == 1
        assert beam[b][0][0] == greedy[b][0] and beam[b][0][1] == greedy[b][1]
        assert abs(beam[b][0][2] - greedy[b][3]) <= REL * (1 + abs(greedy[b][3])) and beam[b][0][2] == beam[b][0][3]
    dec.close()


def test_truncation_at_max_out_and_nbest():
    case = lc.SMALL_CASES[1]   # a-k4
    w, enc, ref, _plain = lc.reference(case)
    dec = lc.make_decoder(asr, case, w)
    lm = lc.make_lm(asr, case)
    ln = rc.lengths_of(case.model)
    kw = lc.search_kwargs(case)
    full = dec.beam_search_host(enc, ln, lm=lm, **kw)
    assert max(n for u in ref["lens"] for n in u) > 2
    for max_out in (0, 2):
        res = dec.beam_search_host(enc, ln, max_out=max_out, lm=lm, **kw)
        for b in range(len(res)):
            assert len(res[b]) == len(full[b])
            for got, want in zip(res[b], full[b]):
                assert got[0] == want[0][:max_out] and got[1] == want[1][:max_out] and got[2:] == want[2:]
    two = dec.beam_search_host(enc, ln, nbest=2, lm=lm, **kw)
    assert [u for u in two] == [u[:2] for u in full]
    # the uncut lengths through the C ABI, and the optional arrays left out
    fuse = dec._lm_handle(lm, case.alpha, case.beta, lc.tok_of_label(case), case.bos, case.eos)
    out = _raw_host(dec, fuse, enc, ln, case.beam, case.beam, 2)
    assert [out[2][b, :out[4][b]].tolist() for b in range(enc.shape[1])] == ref["lens"]
    T, B, K = enc.shape[0], enc.shape[1], case.beam
    p = asr._ptr
    i32, tot, nh = np.zeros((B, K, 2), np.int32), np.zeros((B, K), np.float64), np.zeros(B, np.int32)
    assert asr.lib().asr_rnnt_beam_lm_host(fuse, p(np.ascontiguousarray(enc, np.float32)), p(ln), T, B, K, K, 2, p(i32),
                                           p(i32.copy()), p(np.zeros((B, K), np.int32)), p(tot), None, None, None,
                                           p(nh), None) == asr.ASR_OK
    assert np.array_equal(tot, out[3])
    dec.close()


def test_refusals_in_their_order():
    case = lc.SMALL_CASES[3]          # b-k4: a model with <s> and </s>
    w = rc.make_model(case.model)[0]
    T, B, E, D, Hp, J, V, L = case.model.shape
    dec = lc.make_decoder(asr, case, w)
    lm = lc.make_lm(asr, case)
    bare = asr.NGramLM.from_string("\\data\\\nngram 1=1\n\n\\1-grams:\n-1.0\ta\n\n\\end\\\n")   # no <s>, no </s>
    lib, p = asr.lib(), asr._ptr
    tok = np.asarray(lc.tok_of_label(case), np.int32)
    z = asr._vp()
    ref_ = asr.ctypes.byref(z)
    # asr_rnnt_lm_create: out; the handles and the map; the weights; the flags; a flag without its token
    assert lib.asr_rnnt_lm_create(dec.h, lm.h, p(tok), 0.5, 0.5, 0, None) == asr.ASR_ERR_ARG
    for args in ((None, lm.h, p(tok), 0.5, 0.5, 0), (dec.h, None, p(tok), 0.5, 0.5, 0), (dec.h, lm.h, None, 0.5, 0.5, 0),
                 (dec.h, lm.h, p(tok), -0.5, 0.5, 0), (dec.h, lm.h, p(tok), float("inf"), 0.5, 0),
                 (dec.h, lm.h, p(tok), float("nan"), 0.5, 0), (dec.h, lm.h, p(tok), 0.5, float("nan"), 0),
                 (dec.h, lm.h, p(tok), 0.5, float("-inf"), 0), (dec.h, lm.h, p(tok), 0.5, 0.5, 4),
                 (dec.h, bare.h, p(tok), 0.5, 0.5, asr.ASR_LM_BOS), (dec.h, bare.h, p(tok), 0.5, 0.5, asr.ASR_LM_EOS),
                 (None, lm.h, p(tok), -0.5, 0.5, 4)):
        z.value = 1
        assert lib.asr_rnnt_lm_create(*args, ref_) == asr.ASR_ERR_ARG, args
        assert not z.value
    assert lib.asr_rnnt_lm_create(dec.h, bare.h, p(tok), 0.0, -1.0, 0, ref_) == asr.ASR_OK
    assert lib.asr_rnnt_lm_destroy(z) == asr.ASR_OK
    assert lib.asr_rnnt_lm_destroy(None) == asr.ASR_ERR_ARG
    fuse = dec._lm_handle(lm, 0.5, 0.5, tok, True, True)
    # the workspace: asr_rnnt_beam's plus the LM rows [16][V] of doubles per workgroup
    assert lib.asr_rnnt_beam_lm_workspace_bytes(None, 1, 1, 1) == 0
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 17), (1 << 30, 4, 1), (1 << 30, 1, 16)):
        assert dec.beam_lm_workspace_bytes(fuse, *bad) == 0, bad
    assert dec.beam_lm_workspace_bytes(fuse, 3, 17, 1) == dec.beam_workspace_bytes(3, 17, 1) + 2 * 16 * V * 8
    assert dec.beam_lm_workspace_bytes(fuse, 3, 5, 9) == dec.beam_workspace_bytes(3, 5, 9) + 5 * 16 * V * 8
    enc = np.zeros((2, 2, E), np.float32)
    i32, f64 = np.zeros(64, np.int32), np.zeros(64, np.float64)
    #       z     enc     len   T  B  K  nbest max_out tokens timesteps len  total   am    lm    ntok  nhyp
    good = [fuse, p(enc), None, 2, 2, 4, 2, 3, p(i32), p(i32), p(i32), p(f64), None, None, None, p(i32)]

    def both(changes, want):
        a = list(good)
        for i, value in changes:
            a[i] = value
        assert lib.asr_rnnt_beam_lm_host(*a, None) == want, changes
        assert lib.asr_rnnt_beam_lm(*a, p(f64), None) == want, changes    # refused before any HIP call

    for i in (0, 1, 8, 9, 10, 11, 15):
        both([(i, None)], asr.ASR_ERR_ARG)
    both([(3, 0)], asr.ASR_ERR_ARG)
    both([(4, 0)], asr.ASR_ERR_ARG)
    both([(5, 0)], asr.ASR_ERR_ARG)
    both([(5, 17)], asr.ASR_ERR_ARG)
    both([(6, 0)], asr.ASR_ERR_ARG)
    both([(6, 5)], asr.ASR_ERR_ARG)          # nbest > K
    both([(7, -1)], asr.ASR_ERR_ARG)
    both([(3, 1 << 30)], asr.ASR_ERR_UNSUPPORTED)       # T * B and T * K + 1
    both([(3, 1 << 30), (5, 17)], asr.ASR_ERR_ARG)      # the argument errors come first
    both([(3, 1 << 30), (7, -1)], asr.ASR_ERR_ARG)
    a = list(good)
    a[7], a[8], a[9] = 0, None, None                # max_out = 0 needs no token arrays
    assert lib.asr_rnnt_beam_lm_host(*a, None) == asr.ASR_OK
    assert lib.asr_rnnt_beam_lm(*good, None, None) == asr.ASR_ERR_ARG          # no workspace
    assert lib.asr_rnnt_beam_lm(*good, p(f64), None) == asr.ASR_ERR_STATE      # nothing uploaded
    assert lib.asr_rnnt_beam_lm_host(*good, None) == asr.ASR_OK
    dec.close()
    # the LDS limit is the device call's to refuse, and it comes before the state
    big = rc.Case("big", (1, 1, 8, 16, 816, 816, V, 1), 0, 1, "relu", (1,), 0, 1.0, 0.0)
    dec = rc.make_decoder(asr, big)
    fuse = dec._lm_handle(lm, 0.5, 0.5, tok, True, False)
    enc = np.zeros((1, 1, 8), np.float32)
    args = [fuse, p(enc), None, 1, 1, 1, 1, 1, p(i32), p(i32), p(i32), p(f64), None, None, None, p(i32)]
    assert lib.asr_rnnt_beam_lm(*args, p(f64), None) == asr.ASR_ERR_UNSUPPORTED
    assert lib.asr_rnnt_beam_lm_host(*args, None) == asr.ASR_OK
    dec.close()


def test_keywords_labels_and_lm_rescore():
    case = lc.SMALL_CASES[1]   # a-k4
    w, enc, ref, plain = lc.reference(case)
    lm = lc.make_lm(asr, case)
    ln = rc.lengths_of(case.model)
    T, B, E, D, Hp, J, V, L = case.model.shape
    labels = [""] + ["w%d" % (v - 1) for v in range(1, V)]
    desc = asr.rnnt_desc(V, 0, E, D, Hp, L, J, case.model.act, 1)
    named, bare = asr.TransducerDecoder(desc, w, labels=labels), asr.TransducerDecoder(desc, w)
    assert named.lm_tokens(lm).tolist() == list(lc.tok_of_label(case))
    with pytest.raises(ValueError):
        bare.beam_search_host(enc, ln, lm=lm, alpha=0.5)           # no labels: tok_of_label is required
    with pytest.raises(ValueError):
        bare.beam_search_host(enc, ln, lm=lm, tok_of_label=[0] * (V - 1))
    by_name = named.beam_search_host(enc, ln, beam=case.beam, lm=lm, alpha=case.alpha, beta=case.beta)
    by_map = bare.beam_search_host(enc, ln, lm=lm, **lc.search_kwargs(case))
    assert by_name == by_map
    assert len(named._fuse) == 1
    named.beam_search_host(enc, ln, beam=case.beam, lm=lm, alpha=case.alpha, beta=case.beta)
    assert len(named._fuse) == 1                                   # the handle is kept
    assert bare.beam_search_host(enc, ln, beam=case.beam) == bare.beam_search_host(enc, ln, beam=case.beam, lm=None)
    # eos and bos reach the library
    with_eos = named.beam_search_host(enc, ln, beam=case.beam, lm=lm, alpha=case.alpha, beta=case.beta, eos=True)
    no_bos = named.beam_search_host(enc, ln, beam=case.beam, lm=lm, alpha=case.alpha, beta=case.beta, bos=False)
    assert with_eos != by_name and no_bos != by_name
    # lm_rescore of the unfused n-best: asr_lm_score_host's values, ctcdecode's combination, a stable order
    unfused = bare.beam_search_host(enc, ln, beam=case.beam)
    ranked = named.lm_rescore(unfused, lm, case.alpha, case.beta, host=True)
    tok = lc.tok_of_label(case)
    for u, r in zip(unfused, ranked):
        assert sorted(h[0] for h in u) == sorted(h[0] for h in r)
        assert [h[2] for h in r] == sorted((h[2] for h in r), reverse=True)
        for ys, _ts, total, am, lml, n in r:
            want, counts = lm.score([[tok[y] for y in ys]], bos=True, eos=False, host=True)
            assert lml == want[0] and n == counts[0][0] == len(ys)
            assert total == asr.lm_total(am, lml, n, case.alpha, case.beta)
            assert am in [h[2] for h in u if h[0] == ys]
    # what fusion adds: somewhere its best is not the best of the re-ranked unfused K-best
    fused_best = [u[0][0] if u else None for u in by_map]
    assert any(f != (r[0][0] if r else None) for f, r in zip(fused_best, ranked))
    named.close()
    bare.close()
