"""CPU checks of the LM-fused CTC beam search (asr_ctc_lm_*): the
Python reference against the oracle and against exhaustive enumeration, the
library's host twin against the reference, ties and overflow, the worked
example, every documented refusal, and CTCBeamDecoder's model_path paths.  No
GPU call is made."""
import ctypes
import itertools
import math

import numpy as np
import pytest

from conftest import asr, oracle
from ctc_lm_cases import (HOST_CASES, MIN_GAP, TOL, WIDE_OPTION_CASES, WORKED_ARPA, WORKED_BEST, WORKED_CTC,
                          WORKED_EMIS, WORKED_LABELS, WORKED_LM10, WORKED_TOTAL, Case, assert_same_beams, close,
                          tie_case, wide_reference)
from ctc_lm_reference import LN10, FusedSearch
from lm_reference import BOS, ArpaModel

FAKE = ctypes.c_void_p(0x1000)   # never dereferenced: every refusal comes first


# ---- 1. the reference at alpha = beta = 0 is the plain search -----------------
@pytest.mark.parametrize("T,V,beam,blank,seed", [(30, 6, 4, 0, 1), (30, 6, 4, 2, 2), (12, 29, 8, 0, 3),
                                                  (12, 29, 8, 28, 4), (20, 9, 3, 0, 5)])
def test_reference_without_lm_is_the_oracle(T, V, beam, blank, seed):
    c = Case(seed, T, 3, V, beam, order=2, alpha=0.0, beta=0.0, blank=blank, is_log=False)
    ref, _ = c.reference()
    want = oracle.decode(c.emis, beam, blank, is_log=False)
    for b in range(c.B):
        assert [h[0] for h in ref[b]] == [list(map(int, lab)) for lab, _ in want[b]], b
        for h, (_, lp) in zip(ref[b], want[b]):
            assert close(h[1], lp) and close(h[2], lp) and h[4] == len(h[0]), (b, h, lp)


# ---- 2. a beam wider than the state space: exact sums over all alignments -----
def _collapse(path, blank):
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return tuple(out)


@pytest.mark.parametrize("T,V,blank,seed", [(5, 3, 0, 11), (4, 4, 0, 12), (4, 4, 2, 13), (5, 3, 1, 14)])
def test_reference_exhaustive(T, V, blank, seed):
    c = Case(seed, T, 1, V, 10_000, order=3, alpha=0.8, beta=-0.25, blank=blank, is_log=False)
    ref, _ = c.reference()
    prob = c.emis[:, 0].astype(np.float64)
    exact = {}
    for path in itertools.product(range(V), repeat=T):
        q = _collapse(path, blank)
        exact[q] = exact.get(q, 0.0) + math.prod(prob[t, v] for t, v in enumerate(path))
    model = ArpaModel(c.text)
    tok = [model.ids.get(s, -1) if s != "" else -1 for s in c.labels]
    aln10 = float(np.float32(c.alpha)) * LN10
    beta = float(np.float32(c.beta))
    assert {tuple(h[0]) for h in ref[0]} == set(exact)
    for labels, total, ctc, L, n in ref[0]:
        W = 0.0
        for i in range(len(labels)):
            W = W + ((aln10 * model.score([tok[x] for x in labels[:i + 1]], BOS)[2][-1]) + beta)
        assert close(ctc, math.log(exact[tuple(labels)])), labels
        assert close(total, math.log(exact[tuple(labels)]) + W), labels
        assert n == len(labels)


# ---- 3. the host twin against the reference -----------------------------------
def check_host(c, ref, gap, name):
    assert gap >= MIN_GAP, gap
    lm = c.lm()
    dec = c.decoder(lm)
    got, host_gap = c.host(dec)
    assert_same_beams(got, ref, name)
    assert host_gap == pytest.approx(gap, rel=1e-6)   # the twin's own gap report is the reference's
    labels, totals = dec.best()
    assert labels == [list(u[0][0]) for u in ref]
    assert all(close(t, u[0][1]) for t, u in zip(totals, ref))
    dec.close()


@pytest.mark.parametrize("name", sorted(HOST_CASES))
def test_host_twin_matches_reference(name):
    c = Case(**HOST_CASES[name])
    ref, gap = c.reference()
    check_host(c, ref, gap, name)


@pytest.mark.parametrize("name", sorted(WIDE_OPTION_CASES))
def test_host_twin_matches_reference_on_wide_option_cases(name):
    """The table test_ctc_lm_gpu.py runs on the device: a failure there with
    this one passing is the kernel's."""
    check_host(*wide_reference(name), name)


def test_host_twin_without_lm_weight_is_the_oracle():
    c = Case(120, 25, 3, 9, 5, order=3, alpha=0.0, beta=0.0, is_log=False)
    lm = c.lm()
    dec = c.decoder(lm)
    got, _ = c.host(dec)
    want = oracle.decode(c.emis, c.beam, c.blank, is_log=False)
    for b in range(c.B):
        assert [h[0] for h in got[b]] == [list(map(int, lab)) for lab, _ in want[b]]
        assert all(close(h[1], lp) and h[1] == h[2] for h, (_, lp) in zip(got[b], want[b]))


# ---- 4. ties and overflow ---------------------------------------------------------
def test_ties_all_survive():
    text, labels, emis = tie_case(V=5, beam=2, T=3)
    lm = asr.NGramLM.from_string(text)
    model = ArpaModel(text)
    tok = [model.ids.get(s, -1) if s != "" else -1 for s in labels]
    ref, _ = FusedSearch(model, 5, 2, 0, tok, 0.5, 0.0, bos=True).decode(emis[:, 0], is_log=False)
    assert len(ref) > 3   # more than beam + 1 hypotheses: whole tie classes survived
    dec = asr.CTCLMDecoder(5, 2, lm, lm.label_tokens(labels), 0.5, 0.0)
    dec.decode_host(emis, is_log=False)
    assert_same_beams(dec.beams(256), [ref])


def test_tie_overflow_is_reported():
    text, labels, emis = tie_case(V=40, beam=2, T=2)   # 39 tied states at frame 0
    lm = asr.NGramLM.from_string(text)
    dec = asr.CTCLMDecoder(40, 2, lm, lm.label_tokens(labels), 0.5, 0.0, max_states=3)   # capacity 32
    dec.decode_host(emis, is_log=False)
    with pytest.raises(asr.AsrError) as e:
        dec.beams(8)
    assert e.value.status == asr.ASR_ERR_BEAM_OVERFLOW
    with pytest.raises(asr.AsrError) as e:
        dec.best()
    assert e.value.status == asr.ASR_ERR_BEAM_OVERFLOW
    auto = asr.CTCLMDecoder(40, 2, lm, lm.label_tokens(labels), 0.5, 0.0)   # automatic capacity: no re-decode either
    auto.decode_host(emis, is_log=False)
    with pytest.raises(asr.AsrError) as e:
        auto.beams(8)
    assert e.value.status == asr.ASR_ERR_BEAM_OVERFLOW


def test_capacity_exactly_full_and_one_state_more():
    """32 tied states in 32 slots decode, 33 are an overflow."""
    text, labels, emis = tie_case(V=32, beam=2, T=1)
    lm = asr.NGramLM.from_string(text)
    model = ArpaModel(text)
    tok = [model.ids.get(s, -1) if s != "" else -1 for s in labels]
    ref, _ = FusedSearch(model, 32, 2, 0, tok, 0.5, 0.0, bos=True).decode(emis[:, 0], is_log=False)
    assert len(ref) == 32
    dec = asr.CTCLMDecoder(32, 2, lm, lm.label_tokens(labels), 0.5, 0.0)
    dec.decode_host(emis, is_log=False)
    assert_same_beams(dec.beams(256), [ref])
    text, labels, emis = tie_case(V=33, beam=2, T=1)
    lm = asr.NGramLM.from_string(text)
    dec = asr.CTCLMDecoder(33, 2, lm, lm.label_tokens(labels), 0.5, 0.0)
    dec.decode_host(emis, is_log=False)
    with pytest.raises(asr.AsrError) as e:
        dec.beams(256)
    assert e.value.status == asr.ASR_ERR_BEAM_OVERFLOW


# ---- 5. the worked example (every number is in ctc_lm_cases.py) -------------------
def test_worked_example_fusion_keeps_what_the_plain_search_pruned():
    lm = asr.NGramLM.from_string(WORKED_ARPA)
    dec = asr.CTCLMDecoder(3, 1, lm, lm.label_tokens(WORKED_LABELS), 1.0, 0.0)
    dec.decode_host(WORKED_EMIS, is_log=False)
    beams = dec.beams(8)[0]
    assert [h[0] for h in beams] == [WORKED_BEST, []]
    labels, total, ctc, lm10, n = beams[0]
    assert total == pytest.approx(WORKED_TOTAL, abs=1e-6) and total == pytest.approx(-2.0715, abs=1e-4)
    assert ctc == pytest.approx(WORKED_CTC, abs=1e-6) and lm10 == pytest.approx(WORKED_LM10, abs=1e-6) and n == 2
    assert beams[1][1] == pytest.approx(math.log(0.07), abs=1e-6)
    model = ArpaModel(WORKED_ARPA)
    ref, _ = FusedSearch(model, 3, 1, 0, [-1, model.ids["a"], model.ids["b"]], 1.0, 0.0).decode(WORKED_EMIS[:, 0], False)
    assert_same_beams([beams], [ref])
    # the plain search dropped "b" at frame 0: its final beam is ["a"], and no
    # re-ranking of that beam (lm_rescore) can return "ba"
    plain = oracle.decode(WORKED_EMIS, 1, 0, is_log=False)[0]
    assert [list(map(int, lab)) for lab, _ in plain] == [[1]]
    assert plain[0][1] == pytest.approx(math.log(0.605), abs=1e-6)


# ---- 6. refusals, each before any HIP call ------------------------------------------
@pytest.fixture(scope="module")
def small():
    lm = asr.NGramLM.from_string(WORKED_ARPA)
    tok = lm.label_tokens(WORKED_LABELS)
    return lm, tok


def _create(lm, tok, V=3, beam=2, blank=0, max_states=0, alpha=0.5, beta=0.0, flags=1, top_n=0, codes=None,
            out=True, lm_null=False, tok_null=False):
    h = ctypes.c_void_p()
    c = None if codes is None else np.asarray(codes, np.int32)
    rc = asr.lib().asr_ctc_lm_create(None if c is None else c.ctypes.data, V, beam, blank, max_states,
                                     None if lm_null else lm.h, None if tok_null else tok.ctypes.data, alpha, beta,
                                     flags, top_n, ctypes.byref(h) if out else None)
    if rc == asr.ASR_OK:
        asr.lib().asr_ctc_lm_destroy(h.value)
    else:
        assert h.value is None
    return rc


CREATE_REFUSALS = {
    "out_null": (dict(out=False), asr.ASR_ERR_ARG),
    "lm_null": (dict(lm_null=True), asr.ASR_ERR_ARG),
    "tok_null": (dict(tok_null=True), asr.ASR_ERR_ARG),
    "V_small": (dict(V=1), asr.ASR_ERR_ARG),
    "beam_zero": (dict(beam=0), asr.ASR_ERR_ARG),
    "blank_negative": (dict(blank=-1), asr.ASR_ERR_ARG),
    "blank_past_V": (dict(blank=3), asr.ASR_ERR_ARG),
    "alpha_negative": (dict(alpha=-0.5), asr.ASR_ERR_ARG),
    "alpha_nan": (dict(alpha=float("nan")), asr.ASR_ERR_ARG),
    "alpha_inf": (dict(alpha=float("inf")), asr.ASR_ERR_ARG),
    "beta_inf": (dict(beta=float("-inf")), asr.ASR_ERR_ARG),
    "flags_unknown_bit": (dict(flags=4), asr.ASR_ERR_ARG),
    "top_n_negative": (dict(top_n=-1), asr.ASR_ERR_ARG),
    "max_states_negative": (dict(max_states=-1), asr.ASR_ERR_ARG),
    "codes_equal": (dict(codes=[5, 6, 5]), asr.ASR_ERR_ARG),
    "max_states_below_beam": (dict(beam=4, max_states=4), asr.ASR_ERR_ARG),
    "capacity_above_256": (dict(beam=250), asr.ASR_ERR_UNSUPPORTED),
}


@pytest.mark.parametrize("name", sorted(CREATE_REFUSALS))
def test_create_refusals(small, name):
    kw, status = CREATE_REFUSALS[name]
    assert _create(*small, **kw) == status
    assert _create(*small) == asr.ASR_OK


def test_create_refusals_that_need_other_shapes(small):
    lm, _ = small
    big = np.full(5000, -1, np.int32)
    assert _create(lm, big, V=4097) == asr.ASR_ERR_UNSUPPORTED
    assert _create(lm, big, V=300) == asr.ASR_ERR_UNSUPPORTED             # 299 candidate labels
    assert _create(lm, big, V=300, top_n=256) == asr.ASR_ERR_UNSUPPORTED
    assert _create(lm, big, V=300, top_n=255) == asr.ASR_OK
    no_eos = asr.NGramLM.from_string("\n\\data\\\nngram 1=2\n\n\\1-grams:\n-1\t<s>\n-1\ta\n\n\\end\\\n")
    tok = np.array([-1, 1], np.int32)
    assert _create(no_eos, tok, V=2, flags=asr.ASR_LM_EOS) == asr.ASR_ERR_ARG   # a flag whose token is absent
    assert _create(no_eos, tok, V=2, flags=asr.ASR_LM_BOS) == asr.ASR_OK
    no_bos = asr.NGramLM.from_string("\n\\data\\\nngram 1=2\n\n\\1-grams:\n-1\t</s>\n-1\ta\n\n\\end\\\n")
    assert _create(no_bos, tok, V=2, flags=asr.ASR_LM_BOS) == asr.ASR_ERR_ARG


def test_decode_and_fetch_refusals(small):
    lm, tok = small
    L = asr.lib()
    dec = asr.CTCLMDecoder(3, 2, lm, tok, 0.5, 0.0)
    one = np.array([1], np.int32)
    for fn, tail in ((L.asr_ctc_lm_decode, (None,)), (L.asr_ctc_lm_decode_host, ())):
        assert fn(None, FAKE, 2, 1, 3, 3, None, 0, *tail) == asr.ASR_ERR_ARG
        assert fn(dec.h, None, 2, 1, 3, 3, None, 0, *tail) == asr.ASR_ERR_ARG
        assert fn(dec.h, FAKE, 0, 1, 3, 3, None, 0, *tail) == asr.ASR_ERR_ARG
        assert fn(dec.h, FAKE, 2, 0, 3, 3, None, 0, *tail) == asr.ASR_ERR_ARG
        assert fn(dec.h, FAKE, 2, 1, 0, 3, None, 0, *tail) == asr.ASR_ERR_ARG
        assert fn(dec.h, FAKE, 2, 1, 3, 0, None, 0, *tail) == asr.ASR_ERR_ARG
        for bad in (0, 3, -1):   # lengths are in [1, T]
            assert fn(dec.h, FAKE, 2, 1, 3, 3, np.array([bad], np.int32).ctypes.data, 0, *tail) == asr.ASR_ERR_ARG
    # the LM was never uploaded: refused before any HIP call
    assert L.asr_ctc_lm_decode(dec.h, FAKE, 2, 1, 3, 3, one.ctypes.data, 0, None) == asr.ASR_ERR_STATE
    # fetches: arguments first, then "no decode yet"
    i32 = np.zeros(8, np.int32)
    p = i32.ctypes.data
    assert L.asr_ctc_lm_get_beams(None, 1, 1, p, p, p, None, None, None, None) == asr.ASR_ERR_ARG
    assert L.asr_ctc_lm_get_beams(dec.h, 0, 1, p, p, p, None, None, None, None) == asr.ASR_ERR_ARG
    assert L.asr_ctc_lm_get_beams(dec.h, 1, 0, p, p, p, None, None, None, None) == asr.ASR_ERR_ARG
    assert L.asr_ctc_lm_get_beams(dec.h, 1, 1, None, p, p, None, None, None, None) == asr.ASR_ERR_ARG
    assert L.asr_ctc_lm_get_beams(dec.h, 1, 1, p, None, p, None, None, None, None) == asr.ASR_ERR_ARG
    assert L.asr_ctc_lm_get_beams(dec.h, 1, 1, p, p, None, None, None, None, None) == asr.ASR_ERR_ARG
    assert L.asr_ctc_lm_get_beams(dec.h, 1, 1, p, p, p, None, None, None, None) == asr.ASR_ERR_STATE
    assert L.asr_ctc_lm_get_best(None, p, 1, p, None) == asr.ASR_ERR_ARG
    assert L.asr_ctc_lm_get_best(dec.h, None, 1, p, None) == asr.ASR_ERR_ARG
    assert L.asr_ctc_lm_get_best(dec.h, p, 0, p, None) == asr.ASR_ERR_ARG
    assert L.asr_ctc_lm_get_best(dec.h, p, 1, None, None) == asr.ASR_ERR_ARG
    assert L.asr_ctc_lm_get_best(dec.h, p, 1, p, None) == asr.ASR_ERR_STATE
    gap = np.zeros(4)
    assert L.asr_ctc_lm_host_gaps(None, gap.ctypes.data) == asr.ASR_ERR_ARG
    assert L.asr_ctc_lm_host_gaps(dec.h, None) == asr.ASR_ERR_ARG
    assert L.asr_ctc_lm_host_gaps(dec.h, gap.ctypes.data) == asr.ASR_ERR_STATE
    assert L.asr_ctc_lm_destroy(None) == asr.ASR_ERR_ARG
    # a refused decode leaves the handle usable
    dec.decode_host(WORKED_EMIS, is_log=False)
    assert len(dec.beams(4)[0]) >= 1
    assert dec.host_gaps().shape == (1,)


# ---- 7. the Python mirror -----------------------------------------------------------
def test_label_tokens(small):
    lm, _ = small
    assert lm.label_tokens(["", "a", "b", "zz", "<s>"]).tolist() == [-1, lm.token_id("a"), lm.token_id("b"), -1,
                                                                       lm.token_id("<s>")]
    assert lm.label_tokens(["a"]).dtype == np.int32


def test_beam_decoder_without_model_is_unchanged(monkeypatch):
    made = []

    class Plain:   # stands in for CTCDecoder, whose constructor needs a GPU
        def __init__(self, *args):
            made.append(args)

        def set_timesteps(self, on):
            made.append(("timesteps", on))

    monkeypatch.setattr(asr, "CTCDecoder", Plain)
    d = asr.CTCBeamDecoder(["_", "a", "b"], beam_width=4, cutoff_top_n=1, alpha=3.0, beta=2.0, cutoff_prob=0.5)
    assert made == [(3, 4, 0), ("timesteps", True)]   # the plain decoder, every LM argument ignored
    assert isinstance(d._dec, Plain) and d._fused is None and d._lm is None


def test_beam_decoder_model_path_errors(tmp_path):
    path = tmp_path / "lm.arpa"
    path.write_text(WORKED_ARPA)
    with pytest.raises(NotImplementedError):
        asr.CTCBeamDecoder(["_", "a", "b"], model_path=str(path), cutoff_prob=0.9)
    with pytest.raises(ValueError, match="lm_rescore"):
        asr.CTCBeamDecoder(["_", "x", "y"], model_path=str(path))       # no label is a token: a word-level LM
    with pytest.raises(ValueError, match="lm_rescore"):
        asr.CTCBeamDecoder(["a", "x", "y"], model_path=str(path), blank_id=0)   # only the blank's string is one
    d = asr.CTCBeamDecoder(["_", "a", "b"], model_path=str(path), alpha=1.0, beta=0.0, beam_width=1, cutoff_top_n=40)
    assert isinstance(d._fused, asr.CTCLMDecoder) and d._dec is None
    d._fused.decode_host(WORKED_EMIS, is_log=False)   # the same search the device decode runs
    assert d._fused.beams(4)[0][0][0] == WORKED_BEST
