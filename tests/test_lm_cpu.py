"""CPU checks of the back-off n-gram language model (asr_lm_*): the ARPA loader,
the exact table and the host scorer against the pure-Python reference of
tests/lm_reference.py, every refusal of the parser and of asr_lm_score (decided
before any HIP call: the fake device pointers are never dereferenced), the label
mapper and the combination formula of CTCDecoder.lm_rescore.  No GPU here."""
import ctypes
import math
import re
import subprocess

import numpy as np
import pytest

from conftest import asr
import lm_reference as R

NAMES = ["asr_lm_create_arpa", "asr_lm_create_arpa_mem", "asr_lm_destroy", "asr_lm_get_info", "asr_lm_token_id",
         "asr_lm_token_string", "asr_lm_score_host", "asr_lm_upload", "asr_lm_score"]
FAKE = 0x10000   # a non-NULL, 16-byte aligned "device pointer"
BOS, EOS = R.BOS, R.EOS


def test_symbols_in_mirror_and_library():
    for n in NAMES:
        assert n in asr.EXPORTS, n
        assert hasattr(asr.lib(), n), n
    out = subprocess.run(["nm", "-D", "--defined-only", str(asr.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (asr_[a-z0-9_]+)$", out, flags=re.M))
    assert set(NAMES) <= exported
    assert asr.ASR_LM_MAX_ORDER == 8 and (asr.ASR_LM_BOS, asr.ASR_LM_EOS) == (1, 2)


# ------------------------------------------------------- the worked example
# Every value is a multiple of 1/16, so every sum below is exact in fp64.
# ids: <s> 0, </s> 1, a 2, b 3, c 4 (and <unk> 5 in HAND_UNK).
HAND = """
\\data\\
ngram 1=5
ngram 2=5
ngram 3=3

\\1-grams:
-99\t<s>\t-0.5
-1.0\t</s>
-1.5\ta\t-0.25
-2.0 b -0.75
-2.5\tc\t-0.125

\\2-grams:
-0.5\t<s> a\t-0.375
-0.625\ta b\t-0.25
-0.875\tb c
-1.125\tc </s>
-1.25\ta a\t-1.0

\\3-grams:
-0.125\t<s> a b
-0.25\ta b c
-0.0625\tb a c

\\end\\
"""
HAND_UNK = (HAND.replace("ngram 1=5", "ngram 1=6").replace("ngram 2=5", "ngram 2=6")
            .replace("-2.5\tc\t-0.125\n", "-2.5\tc\t-0.125\n-3.0\t<unk>\t-0.5\n")
            .replace("-1.25\ta a\t-1.0\n", "-1.25\ta a\t-1.0\n-0.375\t<unk> b\n"))
A, B_, C = 2, 3, 4


@pytest.fixture(scope="module")
def hand():
    lm = asr.NGramLM.from_string(HAND, oov_log10=-7.0)
    yield lm
    lm.close()


def one(lm, tokens, bos, eos):
    logp, counts, tl, to = lm.score([tokens], bos=bos, eos=eos, detail=True, host=True)
    return float(logp[0]), counts[0].tolist(), tl[0].tolist(), to[0].tolist()


def test_hand_model_ids_and_info(hand):
    assert (hand.order, hand.vocab_size) == (3, 5)
    assert (hand.bos_id, hand.eos_id, hand.unk_id) == (0, 1, -1)
    assert [hand.token_id(t) for t in ("<s>", "</s>", "a", "b", "c", "d", "")] == [0, 1, 2, 3, 4, -1, -1]
    assert [hand.token_string(i) for i in range(5)] == ["<s>", "</s>", "a", "b", "c"]
    info = hand.info()
    assert info["ngrams"] == [5, 5, 3]
    # (b a c) sits on the path c, a, b: the node (c, a) = the bigram "a c" is not in the model
    assert info["nodes_inserted"] == 1
    # level 1: 6 nodes; level 2: 5 + 1 inserted, +1 sentinel; level 3: 3 + 1; 12-byte nodes, 4-byte words
    assert info["table_bytes"] == 6 * 12 + (6 * 4 + 7 * 12) + (3 * 4 + 4 * 12)


def test_hand_matched_trigram_and_eos(hand):
    # <s> a b c </s>
    #   a | <s>      : bigram (<s> a)            = -0.5     order 2
    #   b | <s> a    : trigram (<s> a b)         = -0.125   order 3
    #   c | a b      : trigram (a b c)           = -0.25    order 3
    #   </s> | b c   : (b c </s>) absent, bo(b c) = 0 (no field); bigram (c </s>) = -1.125, order 2
    total, counts, v, o = one(hand, [A, B_, C], True, True)
    assert v == [-0.5, -0.125, -0.25, -1.125] and o == [2, 3, 3, 2]
    assert total == -2.0 and counts == [4, 0]


def test_hand_backoff_through_two_levels(hand):
    # a a c, no <s>, no </s>
    #   a | -        : P(a)                      = -1.5     order 1
    #   a | a        : bigram (a a)              = -1.25    order 2
    #   c | a a      : (a a c) absent, bo(a a) = -1.0; (a c) absent, bo(a) = -0.25; P(c) = -2.5
    #                  -1.0 + -0.25 + -2.5       = -3.75    order 1
    total, counts, v, o = one(hand, [A, A, C], False, False)
    assert v == [-1.5, -1.25, -3.75] and o == [1, 2, 1]
    assert total == -6.5 and counts == [3, 0]


def test_hand_context_absent_from_the_model(hand):
    # <s> c c
    #   c | <s>      : (<s> c) absent, bo(<s>) = -0.5; P(c) = -2.5           = -3.0    order 1
    #   c | <s> c    : (<s> c c) absent, context (<s> c) not in the model: 0;
    #                  (c c) absent, bo(c) = -0.125; P(c) = -2.5             = -2.625  order 1
    total, counts, v, o = one(hand, [C, C], True, False)
    assert v == [-3.0, -2.625] and o == [1, 1]
    assert total == -5.625 and counts == [2, 0]


def test_hand_ngram_present_whose_suffix_is_absent(hand):
    # b a c
    #   b | -        : P(b)                                  = -2.0     order 1
    #   a | b        : (b a) absent, bo(b) = -0.75; P(a) -1.5 = -2.25    order 1
    #   c | b a      : trigram (b a c) present (its suffix (a c) is not) = -0.0625  order 3
    total, counts, v, o = one(hand, [B_, A, C], False, False)
    assert v == [-2.0, -2.25, -0.0625] and o == [1, 1, 3]
    assert total == -4.3125
    # the node inserted for (a c) is no match:  c | a = bo(a) + P(c) = -0.25 + -2.5, order 1;
    # c | c a: context (c a) absent: 0, then the same
    assert one(hand, [A, C], False, False)[2:] == ([-1.5, -2.75], [1, 1])
    assert one(hand, [C, A, C], False, False)[2:] == ([-2.5, -1.625, -2.75], [1, 1, 1])


def test_hand_empty_hypothesis(hand):
    # </s> | <s>: (<s> </s>) absent, bo(<s>) = -0.5; P(</s>) = -1.0
    assert one(hand, [], True, True) == (-1.5, [1, 0], [-1.5], [1])
    assert one(hand, [], False, True) == (-1.0, [1, 0], [-1.0], [1])
    assert one(hand, [], True, False) == (0.0, [0, 0], [], [])


def test_hand_oov_without_unk_cuts_the_context(hand):
    # <s> a ? b c </s>, oov_log10 = -7
    #   a | <s> = -0.5 (2);  ? = -7.0 (order 0);  b | - = P(b) = -2.0 (1): nothing at or before ? is seen;
    #   c | b = (b c) = -0.875 (2);  </s> | b c = 0 + (c </s>) = -1.125 (2)
    for bad in (99, 5, -1):
        total, counts, v, o = one(hand, [A, bad, B_, C], True, True)
        assert v == [-0.5, -7.0, -2.0, -0.875, -1.125] and o == [2, 0, 1, 2, 2]
        assert total == -11.5 and counts == [5, 1]


def test_hand_oov_with_unk():
    lm = asr.NGramLM.from_string(HAND_UNK, oov_log10=-7.0)
    assert lm.unk_id == 5 and lm.vocab_size == 6
    # a ? b
    #   a = -1.5 (1);  <unk> | a: (a <unk>) absent, bo(a) = -0.25; P(<unk>) = -3.0  = -3.25 (1)
    #   b | a <unk>: (a <unk> b) absent, context (a <unk>) absent: 0; bigram (<unk> b) = -0.375 (2)
    total, counts, v, o = one(lm, [A, -1, B_], False, False)
    assert v == [-1.5, -3.25, -0.375] and o == [1, 1, 2]
    assert total == -5.125 and counts == [3, 1]
    assert one(lm, [A, 5, B_], False, False)[2] == v          # the id of <unk> itself is no OOV
    assert one(lm, [A, 5, B_], False, False)[1] == [3, 0]
    lm.close()


def test_reference_agrees_on_the_hand_model(hand):
    ref = R.ArpaModel(HAND)
    for toks, flags in [([A, B_, C], 3), ([A, A, C], 0), ([C, C], 1), ([B_, A, C], 0), ([A, 99, B_, C], 3), ([], 3)]:
        total, counts, v, o = ref.score(toks, flags, oov_log10=-7.0)
        assert (total, counts, v, o) == one(hand, toks, bool(flags & BOS), bool(flags & EOS))


# ------------------------------------------- host scorer against the reference
LENGTHS = [0, 1, 2, 63, 64, 65, 200]


def compare_with_reference(text, hyps, flags, oov_log10=-100.0):
    ref = R.ArpaModel(text)
    lm = asr.NGramLM.from_string(text, oov_log10=oov_log10)
    logp, counts, tl, to = lm.score(hyps, bos=bool(flags & BOS), eos=bool(flags & EOS), detail=True, host=True)
    for n, h in enumerate(hyps):
        want, wc, wv, wo = ref.score(h, flags, oov_log10)
        assert counts[n].tolist() == wc, (n, counts[n], wc)
        assert to[n].tolist() == wo, (n, flags)
        assert tl[n].tolist() == wv, (n, flags)                       # bit-equal
        assert abs(logp[n] - want) <= 1e-9 * sum(abs(x) for x in wv), (n, logp[n], want)
    info = lm.info()
    lm.close()
    return ref, info


@pytest.mark.parametrize("order,vocab", [(1, 3), (2, 5), (3, 11), (5, 23), (8, 40)])
def test_host_scorer_equals_reference_on_random_models(order, vocab):
    rng = np.random.default_rng(1000 * order + vocab)
    text = R.random_arpa(rng, vocab, order, [4 * vocab + 10 * k for k in range(2, order + 1)])
    inserted = 0
    for flags in (0, BOS, EOS, BOS | EOS):
        hyps = R.random_hypotheses(rng, vocab + 2, LENGTHS)
        ref, info = compare_with_reference(text, hyps, flags)
        inserted = info["nodes_inserted"]
        assert info["order"] == ref.order and info["ngrams"] == [ref.counts[k] for k in range(1, ref.order + 1)]
    if order >= 3:
        assert inserted > 0   # the generator's models are not suffix-closed


@pytest.mark.parametrize("unk", [False, True])
def test_host_scorer_equals_reference_with_oovs(unk):
    rng = np.random.default_rng(77 + unk)
    text = R.random_arpa(rng, 9, 4, [40, 60, 60], unk=unk)
    for flags in (0, BOS | EOS):
        hyps = R.random_hypotheses(rng, 12, [0, 1, 2, 7, 65, 130], oov_rate=0.2)
        compare_with_reference(text, hyps, flags, oov_log10=-3.5)


def test_results_do_not_depend_on_the_batch():
    rng = np.random.default_rng(5)
    text = R.random_arpa(rng, 12, 3, [60, 80])
    lm = asr.NGramLM.from_string(text)
    hyps = R.random_hypotheses(rng, 14, [3, 70, 0, 129])
    all_, _ = lm.score(hyps, host=True)
    for n, h in enumerate(hyps):
        alone, _ = lm.score([h], host=True)
        assert alone[0] == all_[n]
    rev, _ = lm.score(hyps[::-1], host=True)
    assert rev[::-1].tolist() == all_.tolist()
    lm.close()


def test_ids_and_info_follow_the_unigram_order():
    rng = np.random.default_rng(11)
    text = R.random_arpa(rng, 17, 3, [30, 30], unk=True)
    ref = R.ArpaModel(text)
    lm = asr.NGramLM.from_string(text)
    assert lm.vocab_size == ref.vocab == 20 and lm.order == 3
    assert (lm.bos_id, lm.eos_id, lm.unk_id) == (ref.bos, ref.eos, ref.unk)
    for i, t in enumerate(ref.tokens):
        assert lm.token_id(t) == i and lm.token_string(i) == t
    assert lm.token_id("nope") == -1
    s = ctypes.c_char_p()
    assert asr.lib().asr_lm_token_string(lm.h, 20, ctypes.byref(s)) == asr.ASR_ERR_ARG
    assert asr.lib().asr_lm_token_string(lm.h, -1, ctypes.byref(s)) == asr.ASR_ERR_ARG
    assert lm.info()["ngrams"] == [20, 30, 30]
    lm.close()


def test_from_arpa_reads_a_file(tmp_path):
    p = tmp_path / "hand.arpa"
    p.write_text(HAND)
    lm = asr.NGramLM.from_arpa(p, oov_log10=-7.0)
    assert one(lm, [A, B_, C], True, True)[0] == -2.0
    lm.close()


# ------------------------------------------------------------------ the parser
def create(text, oov=-100.0):
    data = text.encode() if isinstance(text, str) else text
    h = ctypes.c_void_p()
    rc = asr.lib().asr_lm_create_arpa_mem(data, len(data), oov, ctypes.byref(h))
    if rc == asr.ASR_OK:
        asr.lib().asr_lm_destroy(h)
    else:
        assert not h.value
    return rc


SMALL = "\\data\\\nngram 1=2\nngram 2=1\n\n\\1-grams:\n-1 a -0.5\n-2 b\n\n\\2-grams:\n-0.5 a b\n\n\\end\\\n"


def test_parser_accepts_the_small_model_and_its_variants():
    assert create(SMALL) == asr.ASR_OK
    assert create("some header\n\n" + SMALL + "trailing text\n") == asr.ASR_OK
    assert create(SMALL.replace("\n", "\r\n")) == asr.ASR_OK
    assert create(SMALL.replace("-1 a -0.5", "-99  \t a \t\t 0.25  ")) == asr.ASR_OK   # -99, a positive back-off
    assert create(SMALL.replace("-2 b", "-2e0 b").replace("-0.5 a b", "-5E-1 a b")) == asr.ASR_OK


def test_parser_unreadable_file(tmp_path):
    h = ctypes.c_void_p()
    rc = asr.lib().asr_lm_create_arpa(str(tmp_path / "missing.arpa").encode(), -100.0, ctypes.byref(h))
    assert rc == asr.ASR_ERR_ARG and not h.value


def test_parser_missing_data_marker():
    assert create(SMALL.replace("\\data\\\n", "")) == asr.ASR_ERR_ARG
    assert create("") == asr.ASR_ERR_ARG


def test_parser_missing_end_marker():
    assert create(SMALL.replace("\\end\\\n", "")) == asr.ASR_ERR_ARG
    assert create(SMALL[:SMALL.index("\\2-grams")]) == asr.ASR_ERR_ARG


def test_parser_section_count_differs_from_its_header():
    assert create(SMALL.replace("ngram 1=2", "ngram 1=3")) == asr.ASR_ERR_ARG
    assert create(SMALL.replace("ngram 1=2", "ngram 1=1")) == asr.ASR_ERR_ARG
    assert create(SMALL.replace("ngram 2=1", "ngram 2=2")) == asr.ASR_ERR_ARG
    assert create(SMALL.replace("-0.5 a b\n", "")) == asr.ASR_ERR_ARG
    assert create(SMALL.replace("\\2-grams:\n-0.5 a b\n", "")) == asr.ASR_ERR_ARG      # a section missing


@pytest.mark.parametrize("bad", ["x", "nan", "inf", "-inf", "-1e999", "-0x1p3", "--1", "-1.0.0", "1e", "-"])
def test_parser_non_numeric_nan_or_infinite_value(bad):
    assert create(SMALL.replace("-2 b", bad + " b")) == asr.ASR_ERR_ARG
    assert create(SMALL.replace("-1 a -0.5", "-1 a " + bad)) == asr.ASR_ERR_ARG


def test_parser_probability_above_zero():
    assert create(SMALL.replace("-2 b", "0.001 b")) == asr.ASR_ERR_ARG
    assert create(SMALL.replace("-0.5 a b", "1 a b")) == asr.ASR_ERR_ARG
    assert create(SMALL.replace("-2 b", "0 b")) == asr.ASR_OK
    assert create(SMALL.replace("-2 b", "-0.0 b")) == asr.ASR_OK


def test_parser_token_without_a_unigram():
    assert create(SMALL.replace("-0.5 a b", "-0.5 a c")) == asr.ASR_ERR_ARG
    assert create(SMALL.replace("-0.5 a b", "-0.5 c b")) == asr.ASR_ERR_ARG


def test_parser_duplicate_ngram():
    assert create(SMALL.replace("-2 b", "-2 a")) == asr.ASR_ERR_ARG
    dup = SMALL.replace("ngram 2=1", "ngram 2=2").replace("-0.5 a b\n", "-0.5 a b\n-0.25 a b\n")
    assert create(dup) == asr.ASR_ERR_ARG
    assert create(dup.replace("-0.25 a b", "-0.25 b a")) == asr.ASR_OK


def test_parser_wrong_number_of_fields():
    assert create(SMALL.replace("-2 b", "-2")) == asr.ASR_ERR_ARG
    assert create(SMALL.replace("-2 b", "-2 b -0.5 -0.5")) == asr.ASR_ERR_ARG
    assert create(SMALL.replace("-0.5 a b", "-0.5 a")) == asr.ASR_ERR_ARG
    assert create(SMALL.replace("-0.5 a b", "-0.5 a b -1 -1")) == asr.ASR_ERR_ARG


def test_parser_bad_oov_value():
    for oov in (0.5, float("nan"), float("-inf")):
        assert create(SMALL, oov) == asr.ASR_ERR_ARG
    assert create(SMALL, 0.0) == asr.ASR_OK


def test_parser_unsupported_order():
    nine = "\\data\\\n" + "".join("ngram %d=1\n" % k for k in range(1, 10))
    nine += "".join("\n\\%d-grams:\n-1 %s\n" % (k, " ".join(["a"] * k)) for k in range(1, 10)) + "\n\\end\\\n"
    assert create(nine) == asr.ASR_ERR_UNSUPPORTED
    eight = nine.replace("ngram 9=1\n", "").replace("\n\\9-grams:\n-1 " + " ".join(["a"] * 9) + "\n", "")
    assert create(eight) == asr.ASR_OK


def test_parser_unsupported_count():
    assert create(SMALL.replace("ngram 2=1", "ngram 2=2147483648")) == asr.ASR_ERR_UNSUPPORTED
    assert create(SMALL.replace("ngram 2=1", "ngram 2=99999999999999999")) == asr.ASR_ERR_UNSUPPORTED
    assert create(SMALL.replace("ngram 2=1", "ngram 2=2147483647")) == asr.ASR_ERR_ARG   # supported, but a lie


# ------------------------------------------------------ asr_lm_score's refusals
@pytest.fixture(scope="module")
def handles():
    with_all = ctypes.c_void_p()
    bare = ctypes.c_void_p()
    assert asr.lib().asr_lm_create_arpa_mem(HAND.encode(), len(HAND.encode()), -7.0, ctypes.byref(with_all)) == 0
    assert asr.lib().asr_lm_create_arpa_mem(SMALL.encode(), len(SMALL.encode()), -7.0, ctypes.byref(bare)) == 0
    yield with_all, bare
    asr.lib().asr_lm_destroy(with_all)
    asr.lib().asr_lm_destroy(bare)


def score(h, tokens=FAKE, ldt=8, lengths=FAKE, N=4, max_len=8, flags=3, logp=FAKE, counts=FAKE, tok_logp=FAKE,
          tok_order=FAKE, ldd=9):
    return asr.lib().asr_lm_score(h, tokens, ldt, lengths, N, max_len, flags, logp, counts, tok_logp, tok_order,
                                  ldd, None)


def test_score_err_arg(handles):
    h, bare = handles
    E = asr.ASR_ERR_ARG
    assert score(None) == E
    assert score(h, tokens=None) == E
    assert score(h, N=0) == E
    assert score(h, N=-2) == E
    assert score(h, ldt=7) == E
    assert score(h, ldd=8) == E
    assert score(h, ldd=8, tok_logp=None) == E
    assert score(h, ldd=8, tok_order=None) == E
    assert score(h, logp=None, counts=None, tok_logp=None, tok_order=None) == E
    assert score(bare, flags=1) == E        # no <s> in the model
    assert score(bare, flags=2) == E        # no </s>
    assert score(bare, flags=3) == E


def test_score_err_unsupported(handles):
    h, _ = handles
    U = asr.ASR_ERR_UNSUPPORTED
    assert score(h, max_len=65537, ldt=65537, ldd=65538) == U
    assert score(h, max_len=-1) == U
    assert score(h, max_len=1 << 30, ldt=1 << 30, ldd=(1 << 30) + 1) == U


def test_score_err_state_when_not_uploaded(handles):
    h, bare = handles
    S = asr.ASR_ERR_STATE
    assert score(h) == S
    assert score(h, lengths=None, ldd=0, tok_logp=None, tok_order=None) == S    # ldd is unused without detail
    assert score(h, max_len=65536, ldt=65536, ldd=65537) == S
    assert score(h, max_len=0, ldt=0, ldd=1) == S
    assert score(bare, flags=0) == S
    # the order of the checks: ARG before UNSUPPORTED before STATE
    assert score(h, max_len=65537, ldt=8) == asr.ASR_ERR_ARG
    assert score(h, max_len=65537, ldt=65537, ldd=65538) == asr.ASR_ERR_UNSUPPORTED


def test_score_host_shares_the_checks(handles):
    h, bare = handles
    tok = np.zeros((2, 4), np.int32)
    out = np.zeros(2, np.float64)

    def host(hh, tokens=tok.ctypes.data, ldt=4, N=2, max_len=4, flags=0, logp=out.ctypes.data, ldd=5):
        return asr.lib().asr_lm_score_host(hh, tokens, ldt, None, N, max_len, flags, logp, None, None, None, ldd)

    assert host(h) == asr.ASR_OK
    assert host(None) == asr.ASR_ERR_ARG
    assert host(h, tokens=None) == asr.ASR_ERR_ARG
    assert host(h, N=0) == asr.ASR_ERR_ARG
    assert host(h, ldt=3) == asr.ASR_ERR_ARG
    assert host(h, logp=None) == asr.ASR_ERR_ARG
    assert host(bare, flags=1) == asr.ASR_ERR_ARG
    assert host(h, max_len=-1) == asr.ASR_ERR_UNSUPPORTED


# ------------------------------------------------------------ the label mapper
def test_label_mapper_char(hand):
    labels = ["", "a", "b", "c", " ", "z"]                     # label 0: the blank, an empty string
    m = hand.label_mapper(labels, mode="char")
    assert m([1, 2, 3]) == [A, B_, C]
    assert m([0, 1, 0, 0, 3]) == [A, C]                        # empty strings are dropped
    assert m([1, 4, 5]) == [A, -1, -1]                         # " " and "z" are no tokens of the model
    assert m([]) == []


def test_label_mapper_word():
    text = "\\data\\\nngram 1=3\n\n\\1-grams:\n-1 ab\n-1 c\n-1 </s>\n\n\\end\\\n"
    lm = asr.NGramLM.from_string(text)
    labels = ["", "a", "b", "c", " ", "|"]
    m = lm.label_mapper(labels, mode="word")
    assert m([1, 2, 4, 3]) == [0, 1]                           # "ab c"
    assert m([4, 4, 1, 2, 4, 4, 3, 4]) == [0, 1]               # empty words are dropped
    assert m([3, 1]) == [-1]                                   # "ca": unknown
    assert m([1, 0, 2]) == [0]                                 # the blank joins nothing
    assert m([]) == []
    bar = lm.label_mapper(labels, mode="word", space="|")
    assert bar([1, 2, 5, 3]) == [0, 1]
    assert bar([1, 2, 4, 3]) == [-1]                           # "ab c" is one unknown word
    with pytest.raises(ValueError):
        lm.label_mapper(labels, mode="bpe")
    lm.close()


# -------------------------------------------------- lm_rescore's combination
class StubLM:
    def __init__(self, values):
        self.values = values
        self.calls = []

    def score(self, token_lists, bos=True, eos=True, detail=False, host=False, stream=0):
        self.calls.append((token_lists, bos, eos))
        lp = np.array([self.values[tuple(t)] for t in token_lists], np.float64)
        counts = np.array([[len(t) + (1 if eos else 0), 0] for t in token_lists], np.int32)
        return lp, counts


def stub_decoder(monkeypatch, beams, exact):
    dec = object.__new__(asr.CTCDecoder)
    dec.h = None
    dec.T, dec.B, dec.V, dec.blank = 5, len(beams), 4, 0
    dec._last = (FAKE, dec.B * 4, 4, None, True)
    dec.beams = lambda max_hyps: [u[:max_hyps] for u in beams]
    monkeypatch.setattr(asr, "ctc_score", lambda emis, targets, **kw: np.array([exact[tuple(t)] for t in targets]))
    return dec


def test_lm_rescore_formula_and_stable_order(monkeypatch):
    beams = [[([1, 2], -1.0), ([1], -1.5), ([2, 2, 3], -2.0), ([3], -2.5)],
             [([2], -0.5)],
             []]
    exact = {(1, 2): -0.9, (1,): -1.4, (2, 2, 3): -1.9, (3,): -1.4, (2,): -0.4}
    lmv = {(1, 2): -3.0, (1,): -1.0, (2, 2, 3): -0.5, (3,): -1.0, (2,): -2.0}
    lm = StubLM(lmv)
    dec = stub_decoder(monkeypatch, beams, exact)
    alpha, beta = 0.7, 0.25
    out = dec.lm_rescore(10, lm, alpha, beta, mapper=lambda lab: list(lab), bos=True, eos=True)
    assert lm.calls == [([[1, 2], [1], [2, 2, 3], [3], [2]], True, True)]       # one call for the whole batch
    assert [len(u) for u in out] == [4, 1, 0]
    for u in out:
        for labels, total, ex, ll, nt in u:
            assert ex == exact[tuple(labels)] and ll == lmv[tuple(labels)] and nt == len(labels)   # </s> not counted
            assert total == ex + alpha * math.log(10.0) * ll + beta * nt
        assert [r[1] for r in u] == sorted((r[1] for r in u), reverse=True)
    # (1,) and (3,) have equal totals: they keep their beam order
    order = [tuple(r[0]) for r in out[0]]
    assert order.index((1,)) + 1 == order.index((3,))
    assert out[0][order.index((1,))][1] == out[0][order.index((3,))][1]
    # alpha = beta = 0: the exact-score ranking of rescore()
    zero = dec.lm_rescore(10, lm, 0.0, 0.0, mapper=lambda lab: list(lab), eos=False)
    assert [tuple(r[0]) for r in zero[0]] == [(1, 2), (1,), (3,), (2, 2, 3)]
    assert all(r[1] == r[2] for u in zero for r in u)
    assert lm.calls[-1][2] is False and all(r[4] == len(r[0]) for u in zero for r in u)
    assert [len(u) for u in dec.lm_rescore(2, lm, alpha, beta, mapper=lambda lab: list(lab))] == [2, 1, 0]


def test_lm_rescore_needs_a_whole_utterance_decode():
    dec = object.__new__(asr.CTCDecoder)
    dec.h = None
    dec._last = None
    with pytest.raises(asr.AsrError) as e:
        dec.lm_rescore(5, None, 1.0, 0.0, mapper=None)
    assert e.value.status == asr.ASR_ERR_STATE
