"""GPU checks of the word mode of the LM-fused CTC beam search (the lexicon trie
on the device): the device against the library's host twin on the
same handle and against the Python reference (labels, ranks and word counts
identical, scores to 1e-9), at every shape and under every option; every
compared case asserts the smallest gap first (seeds chosen on the CPU so that a
rank difference cannot be rounding)."""
import numpy as np
import pytest

from conftest import asr
from ctc_lm_cases import MIN_GAP, assert_same_beams, batch_independence, close, largest_difference
from ctc_wordlm_cases import (HOST_CASES, WIDE_OPTION_CASES, WORKED_ARPA, WORKED_BEAM, WORKED_BEST, WORKED_EMIS,
                              WORKED_LABELS, WordCase, letter, wide_reference)
from ctc_wordlm_reference import WordFusedSearch
from lm_reference import ArpaModel

pytestmark = pytest.mark.gpu


def handles(case):
    lm = case.lm()
    lm.upload()
    lex = case.lexicon(lm)
    lex.upload()
    return lm, lex, case.decoder(lm, lex)


def run(case, reference=None, what=""):
    """Device against the host twin, then against the Python reference:
    `reference` is (beams, gap) where the caller has it already."""
    lm, lex, dec = handles(case)
    host, gap = case.host(dec)
    assert gap >= MIN_GAP, gap
    dev = case.device(dec)
    assert_same_beams(dev, host, "device vs host twin")
    ref, ref_gap = reference or case.reference()
    assert ref_gap >= MIN_GAP, ref_gap
    print("%s: reference gap %.3g, largest |device - reference| %.3g" % (what, ref_gap, largest_difference(dev, ref)))
    assert_same_beams(dev, ref, "device vs reference")
    dec.close()
    lex.close()
    return dev


def all_letters(V, extra):
    """Every letter as a one-letter word (the root has V - 2 children) and a few longer words."""
    one = [letter(i, V) for i in range(V - 2)]
    return one + [one[i] + one[j] for i, j in extra]


# (T, B, V, beam) in both lexicon modes: one frame; a few frames; several blocks of
# pairs; order 5 with a wide beam and peaked emissions; more than 7 words; the
# widest sibling search (a root with 63 and with 64 children, across the wave
# width); capacities 64 and 256; a large vocabulary with the label cutoff; more
# utterances than CUs.
SHAPES = {
    "t1_open": dict(seed=401, T=1, B=3, V=5, beam=2),
    "t1_closed": dict(seed=402, T=1, B=3, V=5, beam=2, closed=True),
    "t8_open": dict(seed=403, T=8, B=4, V=5, beam=3),
    "t8_closed": dict(seed=404, T=8, B=4, V=5, beam=3, closed=True),
    "t40_v29_open": dict(seed=405, T=40, B=8, V=29, beam=8, n_words=60, max_word=4, n_letters=8, oov=-4.0,
                         boost=3.0),
    "t40_v29_closed": dict(seed=1406, T=40, B=8, V=29, beam=8, n_words=60, max_word=4, n_letters=8, closed=True),
    "t64_beam50_order5_open": dict(seed=10407, T=64, B=5, V=29, beam=50, order=5, sigma=8.0, n_words=200, max_word=3,
                                   n_letters=12, oov=-4.0),
    "t64_beam50_order5_closed": dict(seed=23408, T=64, B=5, V=29, beam=50, order=5, sigma=8.0, n_words=200, max_word=3,
                                     n_letters=12, closed=True),
    "nine_words": HOST_CASES["nine_words"],
    "nine_words_closed": HOST_CASES["nine_words_closed"],
    "v65_root63_open": dict(seed=409, T=12, B=2, V=65, beam=8, oov=-4.0, n_letters=10, boost=3.0,
                           words=all_letters(65, [(0, 1), (62, 0), (5, 5)])),
    "v65_root63_closed": dict(seed=410, T=12, B=2, V=65, beam=8, closed=True, n_letters=10, boost=3.0,
                              words=all_letters(65, [(0, 1), (62, 0), (5, 5)])),
    "v66_root64_open": dict(seed=411, T=12, B=2, V=66, beam=8, oov=-4.0, n_letters=10, boost=3.0,
                           words=all_letters(66, [(0, 1), (63, 0), (63, 63)])),
    "v66_root64_closed": dict(seed=412, T=12, B=2, V=66, beam=8, closed=True, n_letters=10, boost=3.0,
                              words=all_letters(66, [(0, 1), (63, 0), (63, 63)])),
    "capacity64": dict(seed=413, T=16, B=2, V=12, beam=40, max_states=64, n_words=30, n_letters=5, sigma=8.0,
                       oov=-4.0),
    "capacity256_closed": dict(seed=414, T=16, B=2, V=12, beam=200, n_words=30, n_letters=5, closed=True,
                               sigma=8.0),
    "capacity256_open": dict(seed=415, T=12, B=2, V=8, beam=220, max_states=256, n_words=12, n_letters=4,
                             sigma=8.0, oov=-4.0),
    "v1000_top40_closed": dict(seed=416, T=24, B=2, V=1000, beam=20, top_n=40, closed=True, n_words=200, max_word=3,
                               n_letters=28, boost=6.0),
    "b300_open": dict(seed=1417, T=8, B=300, V=6, beam=3),
    "b300_closed": dict(seed=418, T=8, B=300, V=6, beam=3, closed=True),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_device_matches_host_twin(name):
    """... and the Python reference, at every shape."""
    run(WordCase(**SHAPES[name]), what=name)


@pytest.mark.parametrize("name", sorted(WIDE_OPTION_CASES))
def test_device_wide_option_cases(name):
    """Every option at a width of more than one wave of pairs, in one lexicon
    mode or the other: device, host twin and reference agree
    (test_ctc_wordlm_cpu.py runs the twin against the reference on the same
    table)."""
    case, ref, gap = wide_reference(name)
    run(case, reference=(ref, gap), what=name)


def test_widest_sibling_runs():
    for V, n in ((65, 63), (66, 64)):
        c = WordCase(**SHAPES["v%d_root%d_open" % (V, n)])
        lm = c.lm()
        assert c.lexicon(lm).info()["max_children"] == n


@pytest.mark.parametrize("name", ["bos_off_eos_on_closed", "beta_neg", "unk", "top3_closed", "lengths_closed",
                                  "batch_major", "probabilities"])
def test_device_small_cases(name):
    run(WordCase(**HOST_CASES[name]), what=name)


@pytest.mark.parametrize("kw", [dict(seed=421, T=40, B=8, V=29, beam=8, n_words=40, n_letters=8),
                                dict(seed=422, T=16, B=3, V=65, beam=8, n_words=40, n_letters=8)])
def test_open_mode_without_lm_weight_is_the_plain_decoder(kw):
    c = WordCase(alpha=0.0, beta=0.0, is_log=False, **kw)
    lm, lex, dec = handles(c)
    got = c.device(dec)
    plain = asr.CTCDecoder(c.V, c.beam, c.blank)
    plain.decode(c.emis, is_log=False)
    want = plain.beams(256)
    for b in range(c.B):
        assert [h[0] for h in got[b]] == [lab for lab, _ in want[b]], b
        for h, (_, lp) in zip(got[b], want[b]):
            assert close(h[1], lp) and h[1] == h[2]
    plain.close()
    dec.close()


def tie_case(V, T):
    """Uniform emissions, every letter a word of the same unigram probability:
    whole classes of states tie at every prune."""
    names = [letter(i, V) for i in range(V - 2)]
    text = "\n\\data\\\nngram 1=%d\n\n\\1-grams:\n" % (len(names) + 2)
    text += "-99\t<s>\n-1\t</s>\n" + "".join("-1\t%s\n" % n for n in names) + "\n\\end\\\n"
    return text, [""] + names + [" "], np.full((T, 1, V), 1.0 / V, np.float32)


def test_ties_and_overflow_on_the_device():
    text, labels, emis = tie_case(V=5, T=3)
    lm = asr.NGramLM.from_string(text)
    lm.upload()
    lex = asr.Lexicon.from_lm(lm, labels)
    lex.upload()
    model = ArpaModel(text)
    words = {(i + 1,): model.ids[labels[i + 1]] for i in range(3)}
    for closed, frames in ((False, 3), (True, 1)):   # 13 and 4 hypotheses, the one-letter words tied
        emis = np.full((frames, 1, 5), 0.2, np.float32)
        ref, _ = WordFusedSearch(model, 5, 2, 0, 4, words, 0.5, 0.0, closed=closed).decode(emis[:, 0], is_log=False)
        totals = [h[1] for h in ref]
        assert len(ref) > 3 and max(totals.count(x) for x in totals) >= 3
        dec = asr.CTCLMDecoder.word(5, 2, lm, lex, 0.5, 0.0, closed=closed)
        dec.decode(emis, is_log=False)
        got = dec.beams(256)
        assert len(got[0]) > 3   # more than beam + 1 hypotheses: whole tie classes survived
        assert_same_beams(got, [ref])
        dec.close()
    text, labels, emis = tie_case(V=40, T=2)
    lm40 = asr.NGramLM.from_string(text)
    lm40.upload()
    lex40 = asr.Lexicon.from_lm(lm40, labels)
    lex40.upload()
    for max_states in (3, 0):   # explicit and automatic capacity: both 32 slots, 40 states tie at frame 0
        d = asr.CTCLMDecoder.word(40, 2, lm40, lex40, 0.5, 0.0, max_states=max_states)
        both = np.concatenate([emis, emis], axis=1)
        both[:, 1, 1:] *= np.linspace(1.0, 0.5, 39, dtype=np.float32)   # the second utterance has no ties
        d.decode(both, is_log=False)
        with pytest.raises(asr.AsrError) as e:
            d.beams(8)
        assert e.value.status == asr.ASR_ERR_BEAM_OVERFLOW
        d.decode(both[:, 1:], is_log=False)   # the handle goes on working
        assert len(d.beams(8)[0]) >= 1
        d.close()


@pytest.mark.parametrize("closed", [False, True])
def test_results_do_not_depend_on_the_batch(closed):
    c = WordCase(seed=431, T=12, B=6, V=7, beam=5, n_words=12, closed=closed)
    lm, lex, dec = handles(c)
    u = c.emis[:, 2:3]
    dec.decode(u, is_log=True)
    alone = dec.beams(64)[0]
    first = c.emis.copy()
    first[:, 0] = u[:, 0]
    last = c.emis.copy()
    last[:, -1] = u[:, 0]
    big = np.ascontiguousarray(np.tile(c.emis, (1, 50, 1)))   # 300 utterances, the one at row 299
    big[:, -1] = u[:, 0]
    outs = []
    dec.decode(first, is_log=True)
    outs.append(dec.beams(64)[0])
    dec.decode(last, is_log=True)
    outs.append(dec.beams(64)[-1])
    dec.decode(np.ascontiguousarray(last.transpose(1, 0, 2)), is_log=True, batch_major=True)
    outs.append(dec.beams(64)[-1])
    dec.decode(big, is_log=True)
    outs.append(dec.beams(64)[-1])
    for o in outs:
        assert o == alone   # bit-identical: labels, ranks and every fp64 score
    dec.close()


def test_results_do_not_depend_on_the_batch_with_the_label_cutoff():
    """Closed mode with 20 of 64 candidate labels a frame, lengths on every row."""
    c = WordCase(seed=436, T=12, B=6, V=65, beam=8, top_n=20, closed=True, n_words=40, n_letters=8, boost=3.0)
    lm, lex, dec = handles(c)
    batch_independence(dec, c.emis, 2, 9)
    dec.close()
    lex.close()


def test_workspace_reuse_across_decodes_of_different_T():
    small = WordCase(seed=432, T=5, B=2, V=6, beam=4)
    large = WordCase(seed=432, T=20, B=9, V=6, beam=4)   # the same lexicon and model (same seed and V)
    assert small.text == large.text and small.words == large.words
    lm, lex, dec = handles(small)
    for c in (small, large, small, large):
        host, gap = c.host(dec)
        assert gap >= MIN_GAP, gap
        assert_same_beams(c.device(dec), host)
    dec.close()


def test_decode_before_upload_is_refused():
    c = WordCase(seed=433, T=4, B=1, V=5, beam=2)
    lm = c.lm()
    lex = c.lexicon(lm)
    dec = c.decoder(lm, lex)
    for step in (lm.upload, lex.upload):   # refused until both are on the device
        with pytest.raises(asr.AsrError) as e:
            dec.decode(c.emis, is_log=True)
        assert e.value.status == asr.ASR_ERR_STATE
        step()
    dec.decode(c.emis, is_log=True)
    assert len(dec.beams(4)[0]) >= 1
    dec.close()


def test_token_and_word_handles_decode_alternately():
    c = WordCase(seed=434, T=10, B=3, V=6, beam=4, n_words=8)
    lm, lex, word = handles(c)
    tok = np.array([-1] + [lm.token_id(s) for s in c.labels[1:]], np.int32)   # one-letter words are tokens too
    token = asr.CTCLMDecoder(c.V, c.beam, lm, tok, c.alpha, c.beta)
    token.decode_host(c.emis, is_log=True)
    token_host = token.beams(256)
    word_host, gap = c.host(word)
    assert gap >= MIN_GAP and float(token.host_gaps().min()) >= MIN_GAP
    for _ in range(2):
        token.decode(c.emis, is_log=True)
        word.decode(c.emis, is_log=True)
        assert_same_beams(token.beams(256), token_host, "token mode")
        assert_same_beams(word.beams(256), word_host, "word mode")
    token.close()
    word.close()


def test_worked_example_on_the_device():
    lm = asr.NGramLM.from_string(WORKED_ARPA)
    lm.upload()
    lex = asr.Lexicon.from_lm(lm, WORKED_LABELS)
    lex.upload()
    for closed in (False, True):
        dec = asr.CTCLMDecoder.word(5, WORKED_BEAM, lm, lex, 1.0, 0.0, closed=closed)
        dec.decode_host(WORKED_EMIS, is_log=False)
        host = dec.beams(8)
        dec.decode(WORKED_EMIS, is_log=False)
        dev = dec.beams(8)
        assert_same_beams(dev, host)
        assert dev[0][0][0] == WORKED_BEST and dec.best()[0] == [WORKED_BEST]
        dec.close()
    # the plain decoder pruned "c " at frame 1; re-ranking its beam with the same LM cannot bring it back
    plain = asr.CTCDecoder(5, WORKED_BEAM, 0)
    plain.decode(WORKED_EMIS, is_log=False)
    rescored = plain.lm_rescore(8, lm, 1.0, 0.0, lm.label_mapper(WORKED_LABELS, mode="word"), bos=True, eos=False)
    assert WORKED_BEST not in [r[0] for r in rescored[0]]
    plain.close()


def test_beam_decoder_with_a_closed_lexicon(tmp_path):
    import torch
    c = WordCase(seed=435, T=10, B=3, V=7, beam=4, n_words=10, alpha=0.6, beta=0.4, closed=True)
    path = tmp_path / "words.arpa"
    path.write_text(c.text)
    labels = ["_"] + c.labels[1:]   # ctcdecode style: the blank has a string of its own
    probs = np.ascontiguousarray(c.emis.transpose(1, 0, 2))   # [B][T][V] log-probabilities
    lens = np.array([10, 4, 7], np.int32)
    bd = asr.CTCBeamDecoder(labels, model_path=str(path), alpha=0.6, beta=0.4, cutoff_top_n=40, beam_width=4,
                            log_probs_input=True, lexicon="closed")
    lm = c.lm()
    lm.upload()
    lex = asr.Lexicon.from_lm(lm, labels)
    lex.upload()
    dec = asr.CTCLMDecoder.word(7, 4, lm, lex, 0.6, 0.4, bos=True, eos=False, top_n=40, closed=True)
    dec.decode(probs, is_log=True, lengths=lens, batch_major=True)
    want = dec.beams(256)
    for feed in (probs, torch.from_numpy(probs).cuda()):
        res, scores, ts, out_lens = bd.decode(feed, torch.from_numpy(lens))
        assert res.shape == (3, 4, 10) and (ts == -1).all()
        for b in range(3):
            for k in range(4):
                if k < len(want[b]):
                    assert res[b, k, :out_lens[b, k]].tolist() == want[b][k][0]
                    assert scores[b, k] == np.float32(-want[b][k][1])
                else:
                    assert out_lens[b, k] == 0 and np.isinf(scores[b, k])
    dec.close()
