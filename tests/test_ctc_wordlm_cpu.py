"""CPU checks of the word mode of the LM-fused CTC beam search (asr_lexicon_*,
asr_ctc_lm_create_word): the library's host twin against the Python
reference of ctc_wordlm_reference.py, the structural cases of a lexicon, the
worked example, every documented refusal and CTCBeamDecoder's lexicon paths.
No GPU call is made."""
import ctypes
import math

import numpy as np
import pytest

from conftest import asr, oracle
from ctc_lm_cases import MIN_GAP, assert_same_beams, close
from ctc_lm_reference import LN10, FusedSearch
from ctc_wordlm_cases import (HOST_CASES, WIDE_OPTION_CASES, WORKED_ARPA, WORKED_BEAM, WORKED_BEST, WORKED_CTC,
                              WORKED_EMIS, WORKED_LABELS, WORKED_LM10, WORKED_PLAIN, WORKED_RANKED, WORKED_TOTAL,
                              WordCase, wide_reference)
from ctc_wordlm_reference import WordFusedSearch
from lm_reference import ArpaModel


def check_hypotheses(c, lm, beams):
    """Every returned hypothesis: lm_log10 is the LM score of its words (a
    left-to-right sum here, a tree there: 1e-9), n its word count, and total is
    ctc + aln10 L + beta n (1e-12)."""
    mapper = lm.label_mapper(c.labels, mode="word")
    aln10 = float(np.float32(c.alpha)) * LN10
    beta = float(np.float32(c.beta))
    for u in beams:
        rows = [mapper(h[0]) for h in u]
        logp, counts = lm.score(rows, bos=c.bos, eos=c.eos, host=True)
        for h, row, want in zip(u, rows, logp):
            labels, total, ctc, L, n = h
            assert n == len(row), h
            assert abs(L - want) <= 1e-9 * max(1.0, abs(want)), (h, want)
            model = ctc + aln10 * L + beta * n
            assert abs(total - model) <= 1e-12 * max(1.0, abs(model)), (h, model)


def run_host(c, name="", reference=None):
    """Host twin against the reference ((beams, gap) where the caller has it
    already); -> (beams, reference, lm)."""
    ref, gap = reference or c.reference()
    assert gap >= MIN_GAP, gap
    lm = c.lm()
    lex = c.lexicon(lm)
    dec = c.decoder(lm, lex)
    got, host_gap = c.host(dec)
    assert_same_beams(got, ref, name)
    assert host_gap == pytest.approx(gap, rel=1e-6)   # the twin's own gap report is the reference's
    labels, totals = dec.best()
    assert labels == [list(u[0][0]) for u in ref]
    assert all(close(t, u[0][1]) for t, u in zip(totals, ref))
    check_hypotheses(c, lm, got)
    dec.close()
    lex.close()
    return got, ref, lm


# ---- 1. the host twin against the reference -----------------------------------
@pytest.mark.parametrize("name", sorted(HOST_CASES))
def test_host_twin_matches_reference(name):
    run_host(WordCase(**HOST_CASES[name]), name)


@pytest.mark.parametrize("name", sorted(WIDE_OPTION_CASES))
def test_host_twin_matches_reference_on_wide_option_cases(name):
    """The table test_ctc_wordlm_gpu.py runs on the device: a failure there with
    this one passing is the kernel's."""
    c, ref, gap = wide_reference(name)
    run_host(c, name, reference=(ref, gap))


def test_context_window_shifts_past_seven_words():
    for name in ("nine_words", "nine_words_closed"):
        c = WordCase(**HOST_CASES[name])
        ref, _ = c.reference()
        assert max(h[4] for u in ref for h in u) >= 9, name   # more words than the longest context


# ---- 2. structural cases --------------------------------------------------------
# Labels of V = 6: 0 blank, 1 a, 2 b, 3 c, 4 d, 5 space; V = 5 has no d and the space is 4.
def test_word_that_is_a_prefix_of_another():
    c = WordCase(seed=31, T=6, B=2, V=6, beam=6, words=["a", "ab", "abc"], order=2,
                 peak=([1, 2, 5, 1, 2, 3], 5.0))
    c.emis[1, 1] = c.emis[2, 1]   # utterance 1: a space instead of the first b, "a abc"
    got, _, lm = run_host(c)
    tok = {w: lm.token_id(w) for w in c.words}
    mapper = lm.label_mapper(c.labels, mode="word")
    assert (tok["ab"], tok["abc"]) in {tuple(mapper(h[0])) for h in got[0]}
    assert (tok["a"], tok["abc"]) in {tuple(mapper(h[0])) for h in got[1]}


def test_oov_word_in_open_mode():
    c = WordCase(seed=32, T=5, B=2, V=6, beam=4, words=["ab", "c"], order=2, oov=-2.0,
                 peak=([4, 1, 5, 3, 5], 14.0))
    got, _, lm = run_host(c)
    for u in got:
        assert u[0][0] == [4, 1, 5, 3, 5] and u[0][4] == 2          # "da c ": da is no word
        assert lm.label_mapper(c.labels, mode="word")(u[0][0]) == [-1, lm.token_id("c")]


def test_leading_doubled_and_trailing_spaces():
    c = WordCase(seed=33, T=7, B=2, V=5, beam=4, words=["a", "b"], order=2, peak=([4, 1, 4, 0, 4, 2, 4], 14.0))
    got, ref, _ = run_host(c)
    for u in got:
        assert u[0][0] == [4, 1, 4, 4, 2, 4] and u[0][4] == 2       # " a  b ": two words, no pending word
    search = c.search()
    memo = {}
    assert search.word_terms((4,), memo) == (0.0, 0.0, 0, ())       # a leading space scores nothing
    assert search.word_terms((4, 1, 4, 4), memo) == search.word_terms((4, 1, 4), memo)   # nor a doubled one
    assert search.partial((4, 1, 4, 4, 2, 4)) == ()


@pytest.mark.parametrize("closed", [False, True])
def test_pending_final_word_terminal_and_not(closed):
    # "ab" is a word, "a" is only its prefix: utterance 0 ends in "c ab", utterance 1 in "c a"
    c = WordCase(seed=37, T=5, B=2, V=5, beam=4, words=["ab", "c"], order=2, closed=closed, oov=-2.0,
                 peak=([3, 4, 1, 0, 2], 14.0))
    c.emis[4, 1] = c.emis[3, 1]   # utterance 1: a blank instead of the b
    got, _, lm = run_host(c)
    assert got[0][0][0] == [3, 4, 1, 2] and got[0][0][4] == 2
    assert got[1][0][0] == [3, 4, 1] and got[1][0][4] == 2          # the unfinished "a" is counted, as an OOV
    mapper = lm.label_mapper(c.labels, mode="word")
    assert mapper(got[0][0][0]) == [lm.token_id("c"), lm.token_id("ab")]
    assert mapper(got[1][0][0]) == [lm.token_id("c"), -1]


def test_closed_mode_dead_end():
    # the emissions favour d (label 4), which no word contains: closed mode never returns it
    c = WordCase(seed=35, T=6, B=2, V=6, beam=5, words=["ab", "ca", "b"], order=2, closed=True,
                 peak=([4, 4, 1, 4, 5, 4], 6.0))
    got, _, _ = run_host(c)
    assert all(4 not in h[0] for u in got for h in u)
    index = {s: i for i, s in enumerate(c.labels)}
    spelled = {tuple(index[ch] for ch in w) for w in c.words}
    for u in got:
        for h in u:   # every finished word is a lexicon word, no leading or doubled space
            words = "".join(c.labels[x] for x in h[0]).split(" ")
            assert all(tuple(index[ch] for ch in w) in spelled for w in words[:-1]), h
    open_case = WordCase(seed=35, T=6, B=2, V=6, beam=5, words=["ab", "ca", "b"], order=2, closed=False,
                         peak=([4, 4, 1, 4, 5, 4], 6.0))
    ref, _ = open_case.reference()
    assert any(4 in h[0] for u in ref for h in u)   # the open search does go there


def test_closed_mode_state_space_smaller_than_the_beam():
    c = WordCase(seed=36, T=3, B=2, V=5, beam=200, words=["a", "bc"], order=2, closed=True)
    got, _, _ = run_host(c)
    # every label string of at most 3 labels the two words allow, the empty one included
    want = {(), (1,), (2,), (2, 3), (1, 4), (1, 4, 1), (1, 4, 2), (2, 3, 4)}
    for u in got:
        assert {tuple(h[0]) for h in u} == want


# ---- 3. open mode without an LM weight is the plain search ---------------------
@pytest.mark.parametrize("T,V,beam,seed", [(20, 6, 4, 41), (12, 9, 5, 42)])
def test_open_mode_without_lm_weight_is_the_plain_search(T, V, beam, seed):
    c = WordCase(seed, T, 3, V, beam, order=2, alpha=0.0, beta=0.0, is_log=False)
    ref, _ = c.reference()
    model = ArpaModel(c.text)
    plain = FusedSearch(model, V, beam, 0, [-1] * V, 0.0, 0.0)
    lm = c.lm()
    lex = c.lexicon(lm)
    dec = c.decoder(lm, lex)
    got, _ = c.host(dec)
    tokens = asr.CTCLMDecoder(V, beam, lm, np.full(V, -1, np.int32), 0.0, 0.0)
    tokens.decode_host(c.emis, is_log=False)
    twin = tokens.beams(256)
    want = oracle.decode(c.emis, beam, 0, is_log=False)
    for b in range(c.B):
        base, _ = plain.decode(c.emis[:, b], is_log=False)
        # bit for bit: the word-mode reference and the token-mode reference, the two host twins
        assert [(h[0], h[1], h[2]) for h in ref[b]] == [(h[0], h[1], h[2]) for h in base]
        assert [(h[0], h[1], h[2]) for h in got[b]] == [(h[0], h[1], h[2]) for h in twin[b]]
        assert all(h[1] == h[2] for h in got[b])   # W is exactly 0.0
        assert [h[0] for h in got[b]] == [list(map(int, lab)) for lab, _ in want[b]]
        assert [h[2] for h in ref[b]] == [lp for _, lp in want[b]]   # the oracle's fp64 sums, bit for bit
        assert all(close(h[1], lp) for h, (_, lp) in zip(got[b], want[b]))


# ---- 4. the worked example (every number is in ctc_wordlm_cases.py) --------------
def test_worked_example_word_lm_keeps_what_the_plain_search_pruned():
    lm = asr.NGramLM.from_string(WORKED_ARPA)
    lex = asr.Lexicon.from_lm(lm, WORKED_LABELS)
    assert lex.skipped == 0 and lex.info()["words"] == 3
    dec = asr.CTCLMDecoder.word(5, WORKED_BEAM, lm, lex, 1.0, 0.0)
    dec.decode_host(WORKED_EMIS, is_log=False)
    beams = dec.beams(8)[0]
    assert [h[0] for h in beams] == WORKED_RANKED
    labels, total, ctc, lm10, n = beams[0]
    assert labels == WORKED_BEST
    assert total == pytest.approx(WORKED_TOTAL, abs=1e-6) and total == pytest.approx(math.log(0.108), abs=1e-4)
    assert ctc == pytest.approx(WORKED_CTC, abs=1e-6) and lm10 == pytest.approx(WORKED_LM10, abs=1e-6) and n == 1
    assert beams[1][1] == pytest.approx(math.log(0.0071), abs=1e-4) and beams[1][4] == 1   # the pending "a"
    assert beams[2][1] == pytest.approx(math.log(0.005325), abs=1e-4)
    model = ArpaModel(WORKED_ARPA)
    words = {(1,): model.ids["a"], (2,): model.ids["b"], (3,): model.ids["c"]}
    ref, _ = WordFusedSearch(model, 5, WORKED_BEAM, 0, 4, words, 1.0, 0.0).decode(WORKED_EMIS[:, 0], False)
    assert_same_beams([beams], [ref])
    # the plain search of the same width dropped "c " and "c$" at frame 1: no
    # re-ranking of its final beam (lm_rescore with mode="word") can return "c "
    plain = oracle.decode(WORKED_EMIS, WORKED_BEAM, 0, is_log=False)[0]
    assert [list(map(int, lab)) for lab, _ in plain] == WORKED_PLAIN
    assert WORKED_BEST not in WORKED_PLAIN


# ---- 5. refusals, each before any HIP call ------------------------------------------
def _lexicon(spell=(1, 2, 3), offsets=(0, 2, 3), tok=(2, 3), n_words=2, V=5, space=4, out=True, null=None):
    s, o, t = np.asarray(spell, np.int32), np.asarray(offsets, np.int64), np.asarray(tok, np.int32)
    h = ctypes.c_void_p()
    rc = asr.lib().asr_lexicon_create(None if null == "spell" else s.ctypes.data,
                                      None if null == "offsets" else o.ctypes.data,
                                      None if null == "tok" else t.ctypes.data, n_words, V, space,
                                      ctypes.byref(h) if out else None)
    if rc == asr.ASR_OK:
        asr.lib().asr_lexicon_destroy(h.value)
    else:
        assert h.value is None
    return rc


LEXICON_REFUSALS = {
    "out_null": dict(out=False),
    "spell_null": dict(null="spell"),
    "offsets_null": dict(null="offsets"),
    "tok_null": dict(null="tok"),
    "V_small": dict(V=1),
    "no_words": dict(n_words=0),
    "space_negative": dict(space=-1),
    "space_past_V": dict(space=5),
    "offsets_not_from_zero": dict(offsets=(1, 2, 3)),
    "offsets_decreasing": dict(offsets=(0, 3, 2)),
    "label_negative": dict(spell=(1, -1, 3)),
    "label_past_V": dict(spell=(1, 5, 3)),
    "label_is_the_space": dict(spell=(1, 4, 3)),
    "empty_word": dict(offsets=(0, 3, 3)),
    "token_negative": dict(tok=(2, -1)),
    "one_spelling_two_tokens": dict(spell=(1, 2, 1, 2), offsets=(0, 2, 4), tok=(2, 3)),
}


@pytest.mark.parametrize("name", sorted(LEXICON_REFUSALS))
def test_lexicon_create_refusals(name):
    assert _lexicon(**LEXICON_REFUSALS[name]) == asr.ASR_ERR_ARG
    assert _lexicon() == asr.ASR_OK


def test_lexicon_info_and_duplicates():
    assert _lexicon(spell=(1, 2, 1, 2), offsets=(0, 2, 4), tok=(3, 3)) == asr.ASR_OK   # the same word twice: once
    lex = asr.Lexicon([[1, 2], [1, 2], [1], [1, 3], [2]], [3, 3, 7, 8, 9], 5, 4)
    assert lex.info() == {"words": 4, "nodes": 5, "max_children": 2, "space_label": 4, "table_bytes": 4 * (6 + 5 + 5)}
    L = asr.lib()
    assert L.asr_lexicon_get_info(None, ctypes.byref(asr.LexiconInfo())) == asr.ASR_ERR_ARG
    assert L.asr_lexicon_get_info(lex.h, None) == asr.ASR_ERR_ARG
    assert L.asr_lexicon_upload(None) == asr.ASR_ERR_ARG
    assert L.asr_lexicon_destroy(None) == asr.ASR_ERR_ARG
    lex.close()
    with pytest.raises(ValueError):
        asr.Lexicon([[1]], [1, 2], 5, 4)


@pytest.fixture(scope="module")
def small():
    lm = asr.NGramLM.from_string(WORKED_ARPA)
    return lm, asr.Lexicon.from_lm(lm, WORKED_LABELS)


def _create(lm, lex, V=5, beam=2, blank=0, max_states=0, alpha=0.5, beta=0.0, flags=1, top_n=0, mode=0, codes=None,
            out=True, lm_null=False, lex_null=False):
    h = ctypes.c_void_p()
    c = None if codes is None else np.asarray(codes, np.int32)
    rc = asr.lib().asr_ctc_lm_create_word(None if c is None else c.ctypes.data, V, beam, blank, max_states,
                                          None if lm_null else lm.h, None if lex_null else lex.h, alpha, beta, flags,
                                          top_n, mode, ctypes.byref(h) if out else None)
    if rc == asr.ASR_OK:
        asr.lib().asr_ctc_lm_destroy(h.value)
    else:
        assert h.value is None
    return rc


CREATE_REFUSALS = {
    "out_null": (dict(out=False), asr.ASR_ERR_ARG),
    "lm_null": (dict(lm_null=True), asr.ASR_ERR_ARG),
    "lex_null": (dict(lex_null=True), asr.ASR_ERR_ARG),
    "V_small": (dict(V=1), asr.ASR_ERR_ARG),
    "beam_zero": (dict(beam=0), asr.ASR_ERR_ARG),
    "blank_negative": (dict(blank=-1), asr.ASR_ERR_ARG),
    "blank_past_V": (dict(blank=5), asr.ASR_ERR_ARG),
    "alpha_negative": (dict(alpha=-0.5), asr.ASR_ERR_ARG),
    "alpha_nan": (dict(alpha=float("nan")), asr.ASR_ERR_ARG),
    "beta_inf": (dict(beta=float("inf")), asr.ASR_ERR_ARG),
    "flags_unknown_bit": (dict(flags=4), asr.ASR_ERR_ARG),
    "top_n_negative": (dict(top_n=-1), asr.ASR_ERR_ARG),
    "max_states_negative": (dict(max_states=-1), asr.ASR_ERR_ARG),
    "lexicon_V_differs": (dict(V=6), asr.ASR_ERR_ARG),
    "spelling_uses_the_blank": (dict(blank=2), asr.ASR_ERR_ARG),
    "space_is_the_blank": (dict(blank=4), asr.ASR_ERR_ARG),
    "mode_unknown": (dict(mode=2), asr.ASR_ERR_ARG),
    "mode_negative": (dict(mode=-1), asr.ASR_ERR_ARG),
    "codes_equal": (dict(codes=[5, 6, 5, 7, 8]), asr.ASR_ERR_ARG),
    "max_states_below_beam": (dict(beam=4, max_states=4), asr.ASR_ERR_ARG),
    "capacity_above_256": (dict(beam=250), asr.ASR_ERR_UNSUPPORTED),
}


@pytest.mark.parametrize("name", sorted(CREATE_REFUSALS))
def test_create_word_refusals(small, name):
    kw, status = CREATE_REFUSALS[name]
    assert _create(*small, **kw) == status
    assert _create(*small) == asr.ASR_OK and _create(*small, mode=1) == asr.ASR_OK


def test_create_word_refusals_that_need_other_shapes(small):
    lm, _ = small
    wide = asr.Lexicon([[1]], [2], 300, 2)
    assert _create(lm, wide, V=300) == asr.ASR_ERR_UNSUPPORTED             # 299 candidate labels
    assert _create(lm, wide, V=300, top_n=255) == asr.ASR_OK
    huge = asr.Lexicon([[1]], [2], 4097, 2)
    assert _create(lm, huge, V=4097, top_n=40) == asr.ASR_ERR_UNSUPPORTED
    no_eos = asr.NGramLM.from_string("\n\\data\\\nngram 1=2\n\n\\1-grams:\n-1\t<s>\n-1\ta\n\n\\end\\\n")
    lex = asr.Lexicon([[1]], [1], 3, 2)
    assert _create(no_eos, lex, V=3, flags=asr.ASR_LM_EOS) == asr.ASR_ERR_ARG   # a flag whose token is absent
    assert _create(no_eos, lex, V=3, flags=asr.ASR_LM_BOS) == asr.ASR_OK


def test_word_handle_decode_before_upload_and_fetch_states(small):
    lm, lex = small
    dec = asr.CTCLMDecoder.word(5, 2, lm, lex, 0.5, 0.0)
    fake = ctypes.c_void_p(0x1000)   # never dereferenced: the refusal comes first
    assert asr.lib().asr_ctc_lm_decode(dec.h, fake, 2, 1, 5, 5, None, 0, None) == asr.ASR_ERR_STATE
    with pytest.raises(asr.AsrError) as e:
        dec.beams(4)
    assert e.value.status == asr.ASR_ERR_STATE
    dec.decode_host(WORKED_EMIS, is_log=False)
    assert len(dec.beams(4)[0]) == 3 and dec.host_gaps().shape == (1,)


# ---- 6. the Python mirror -----------------------------------------------------------
def test_lexicon_from_lm_skips_what_the_labels_cannot_spell():
    text = ("\n\\data\\\nngram 1=7\n\n\\1-grams:\n-9\t<s>\n-1\t</s>\n-1\t<unk>\n-1\tab\n-1\tax\n-1\tb\n-1\tba\n"
            "\n\\end\\\n")
    lm = asr.NGramLM.from_string(text)
    lex = asr.Lexicon.from_lm(lm, ["", "a", "b", " "])
    assert lex.skipped == 1 and lex.info()["words"] == 3 and lex.space == 3   # "ax" has a letter that is no label
    assert asr.Lexicon.from_lm(lm, ["x", "a", "b", " "]).skipped == 0
    assert asr.Lexicon.from_lm(lm, ["x", "a", "b", " "], blank_id=0).skipped == 1   # the blank's string spells nothing
    with pytest.raises(ValueError):
        asr.Lexicon.from_lm(lm, ["", "a", "b", "_"])   # the space is no label


def test_beam_decoder_with_a_word_level_model(tmp_path):
    path = tmp_path / "words.arpa"
    path.write_text(WORKED_ARPA.replace("\ta\t", "\tab\t").replace("<s> a", "<s> ab"))   # "ab", "b", "c"
    labels = ["_", "a", "b", "c", " "]
    with pytest.raises(ValueError, match="lm_rescore"):
        asr.CTCBeamDecoder(["_", "x", "y", "z", " "], model_path=str(path))   # lexicon=None: as before
    with pytest.raises(ValueError, match="space"):
        asr.CTCBeamDecoder(labels, model_path=str(path), lexicon="open", space="|")
    with pytest.raises(ValueError):
        asr.CTCBeamDecoder(labels, model_path=str(path), lexicon="both")
    with pytest.raises(ValueError):
        asr.CTCBeamDecoder(labels, lexicon="open")
    with pytest.raises(NotImplementedError):
        asr.CTCBeamDecoder(labels, model_path=str(path), lexicon="open", cutoff_prob=0.9)
    for mode in ("open", "closed"):
        d = asr.CTCBeamDecoder(labels, model_path=str(path), alpha=1.0, beta=0.0, beam_width=WORKED_BEAM,
                               cutoff_top_n=40, lexicon=mode)
        assert isinstance(d._fused, asr.CTCLMDecoder) and d._dec is None and d._lex.info()["words"] == 3
        d._fused.decode_host(WORKED_EMIS, is_log=False)   # the same search the device decode runs
        best = d._fused.beams(4)[0][0]
        assert best[0] == WORKED_BEST and best[4] == 1
