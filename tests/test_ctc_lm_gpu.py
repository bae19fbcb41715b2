"""GPU checks of the LM-fused CTC beam search (asr_ctc_lm_decode): the
device against the library's host twin on the same handle and against the Python
reference (labels, ranks and n_tokens identical, scores to 1e-9), at every shape
and under every option; every randomised case asserts the smallest gap first (a
seed chosen so that a rank difference cannot be rounding)."""
import numpy as np
import pytest

from conftest import asr
from ctc_lm_cases import (HOST_CASES, MIN_GAP, WIDE_OPTION_CASES, WORKED_ARPA, WORKED_BEST, WORKED_EMIS, WORKED_LABELS,
                          Case, assert_same_beams, batch_independence, close, largest_difference, tie_case,
                          wide_reference)
from ctc_lm_reference import FusedSearch
from lm_reference import ArpaModel

pytestmark = pytest.mark.gpu


def run(case, reference=None, what=""):
    """Device against the host twin, then against the Python reference:
    `reference` is (beams, gap) where the caller has it already."""
    lm = case.lm()
    lm.upload()
    dec = case.decoder(lm)
    host, gap = case.host(dec)
    assert gap >= MIN_GAP, gap
    dev = case.device(dec)
    assert_same_beams(dev, host, "device vs host twin")
    ref, ref_gap = reference or case.reference()
    assert ref_gap >= MIN_GAP, ref_gap
    print("%s: reference gap %.3g, largest |device - reference| %.3g" % (what, ref_gap, largest_difference(dev, ref)))
    assert_same_beams(dev, ref, "device vs reference")
    dec.close()
    return dev


# (T, B, V, beam): one frame; a few frames; several blocks of pairs; order 5 with a
# wide beam; V and beam + 1 across a wave boundary; more utterances than CUs; a
# large vocabulary with the label cutoff.
SHAPES = {
    "t1": dict(seed=201, T=1, B=3, V=5, beam=2),
    "t6": dict(seed=202, T=6, B=4, V=5, beam=3),
    "t40_v29": dict(seed=305, T=40, B=8, V=29, beam=8),
    "t64_beam50_order5": dict(seed=601, T=64, B=5, V=29, beam=50, order=5, sigma=8.0),
    "v63": dict(seed=205, T=16, B=2, V=63, beam=8),
    "v64": dict(seed=206, T=16, B=2, V=64, beam=8),
    "v65": dict(seed=207, T=16, B=2, V=65, beam=8),
    "beam62": dict(seed=208, T=16, B=2, V=12, beam=62),
    "beam63": dict(seed=302, T=16, B=2, V=12, beam=63),
    "beam64": dict(seed=210, T=16, B=2, V=12, beam=64),
    "b300": dict(seed=211, T=8, B=300, V=6, beam=3),
    "v1000_top40": dict(seed=302, T=24, B=2, V=1000, beam=20, top_n=40),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_device_matches_host_twin(name):
    """... and the Python reference, at every shape."""
    run(Case(**SHAPES[name]), what=name)


@pytest.mark.parametrize("name", sorted(WIDE_OPTION_CASES))
def test_device_wide_option_cases(name):
    """Every option at a width of more than one wave of pairs or on a limit:
    device, host twin and reference agree (test_ctc_lm_cpu.py runs the twin
    against the reference on the same table)."""
    case, ref, gap = wide_reference(name)
    run(case, reference=(ref, gap), what=name)


@pytest.mark.parametrize("name", sorted(HOST_CASES))
def test_device_small_cases(name):
    """OOV with and without <unk>, <s> / </s> on and off, beta of both signs,
    the label cutoff on quantised emissions, lengths 1 .. T, batch-major
    strides, probabilities, a non-zero blank with codes: device, host twin and
    reference agree."""
    run(Case(**HOST_CASES[name]), what=name)


@pytest.mark.parametrize("kw", [dict(seed=221, T=40, B=8, V=29, beam=8), dict(seed=222, T=16, B=3, V=65, beam=8),
                                dict(seed=223, T=20, B=4, V=9, beam=20, blank=4)])
def test_device_without_lm_weight_is_the_plain_decoder(kw):
    c = Case(alpha=0.0, beta=0.0, is_log=False, **kw)
    lm = c.lm()
    lm.upload()
    dec = c.decoder(lm)
    got = c.device(dec)
    plain = asr.CTCDecoder(c.V, c.beam, c.blank)
    plain.decode(c.emis, is_log=False)
    want = plain.beams(256)
    for b in range(c.B):
        assert [h[0] for h in got[b]] == [lab for lab, _ in want[b]], b
        for h, (_, lp) in zip(got[b], want[b]):
            assert close(h[1], lp) and h[1] == h[2] and h[4] == len(h[0])
    plain.close()
    dec.close()


def test_ties_and_overflow_on_the_device():
    text, labels, emis = tie_case(V=5, beam=2, T=3)
    lm = asr.NGramLM.from_string(text)
    lm.upload()
    model = ArpaModel(text)
    tok = [model.ids.get(s, -1) if s != "" else -1 for s in labels]
    ref, _ = FusedSearch(model, 5, 2, 0, tok, 0.5, 0.0, bos=True).decode(emis[:, 0], is_log=False)
    dec = asr.CTCLMDecoder(5, 2, lm, lm.label_tokens(labels), 0.5, 0.0)
    dec.decode(emis, is_log=False)
    got = dec.beams(256)
    assert len(got[0]) > 3
    assert_same_beams(got, [ref])
    text, labels, emis = tie_case(V=40, beam=2, T=2)
    lm40 = asr.NGramLM.from_string(text)
    lm40.upload()
    for max_states in (3, 0):   # explicit and automatic capacity: both 32 slots, 40 states tie
        d = asr.CTCLMDecoder(40, 2, lm40, lm40.label_tokens(labels), 0.5, 0.0, max_states=max_states)
        both = np.concatenate([emis, emis], axis=1)
        both[:, 1, 1:] *= np.linspace(1.0, 0.5, 39, dtype=np.float32)   # the second utterance has no ties
        d.decode(both, is_log=False)
        with pytest.raises(asr.AsrError) as e:
            d.beams(8)
        assert e.value.status == asr.ASR_ERR_BEAM_OVERFLOW
        d.decode(both[:, 1:], is_log=False)   # the handle goes on working
        assert len(d.beams(8)[0]) >= 1
        d.close()


def test_capacity_exactly_full_and_one_state_more():
    """32 tied states in 32 slots decode, 33 are an overflow: the kernel's
    comparison with the capacity, pinned from both sides."""
    text, labels, emis = tie_case(V=32, beam=2, T=1)
    lm = asr.NGramLM.from_string(text)
    lm.upload()
    model = ArpaModel(text)
    tok = [model.ids.get(s, -1) if s != "" else -1 for s in labels]
    ref, _ = FusedSearch(model, 32, 2, 0, tok, 0.5, 0.0, bos=True).decode(emis[:, 0], is_log=False)
    assert len(ref) == 32
    for max_states in (3, 0):   # explicit and automatic capacity: both 32 slots
        dec = asr.CTCLMDecoder(32, 2, lm, lm.label_tokens(labels), 0.5, 0.0, max_states=max_states)
        dec.decode(emis, is_log=False)
        got = dec.beams(256)
        assert len(got[0]) == 32
        assert_same_beams(got, [ref])
        dec.close()
    text, labels, emis = tie_case(V=33, beam=2, T=1)
    lm33 = asr.NGramLM.from_string(text)
    lm33.upload()
    untied = emis.copy()
    untied[:, 0, 1:] *= np.linspace(1.0, 0.5, 32, dtype=np.float32)
    model = ArpaModel(text)
    tok = [model.ids.get(s, -1) if s != "" else -1 for s in labels]
    ref33, _ = FusedSearch(model, 33, 2, 0, tok, 0.5, 0.0, bos=True).decode(untied[:, 0], is_log=False)
    assert len(ref33) == 3
    for max_states in (3, 0):
        dec = asr.CTCLMDecoder(33, 2, lm33, lm33.label_tokens(labels), 0.5, 0.0, max_states=max_states)
        dec.decode(emis, is_log=False)
        with pytest.raises(asr.AsrError) as e:
            dec.beams(256)
        assert e.value.status == asr.ASR_ERR_BEAM_OVERFLOW
        dec.decode(untied, is_log=False)   # the handle goes on working
        assert_same_beams(dec.beams(256), [ref33])
        dec.close()


def test_results_do_not_depend_on_the_batch():
    c = Case(seed=231, T=12, B=6, V=9, beam=5, order=3)
    lm = c.lm()
    lm.upload()
    dec = c.decoder(lm)
    u = c.emis[:, 2:3]
    dec.decode(u, is_log=True)
    alone = dec.beams(64)[0]
    first = c.emis.copy()
    first[:, 0] = u[:, 0]
    last = c.emis.copy()
    last[:, -1] = u[:, 0]
    outs = [alone]
    dec.decode(first, is_log=True)
    outs.append(dec.beams(64)[0])
    dec.decode(last, is_log=True)
    outs.append(dec.beams(64)[-1])
    dec.decode(np.ascontiguousarray(last.transpose(1, 0, 2)), is_log=True, batch_major=True)
    outs.append(dec.beams(64)[-1])
    dec.decode(np.ascontiguousarray(first.transpose(1, 0, 2)), is_log=True, batch_major=True)
    outs.append(dec.beams(64)[0])
    for o in outs[1:]:
        assert o == alone   # bit-identical: labels, ranks and every fp64 score
    dec.close()


def test_results_do_not_depend_on_the_batch_with_the_label_cutoff():
    """The candidate labels of a frame are read at an index that depends on the
    utterance's row and on T: 20 of 64 labels, lengths on every row."""
    c = Case(seed=235, T=12, B=6, V=65, beam=8, top_n=20)
    lm = c.lm()
    lm.upload()
    dec = c.decoder(lm)
    batch_independence(dec, c.emis, 2, 9)
    dec.close()


def test_workspace_reuse_growing_then_shrinking():
    small = Case(seed=232, T=5, B=2, V=7, beam=4)
    large = Case(seed=232, T=20, B=9, V=7, beam=4)   # the same model (same seed and V), more frames and rows
    assert small.text == large.text
    lm = small.lm()
    lm.upload()
    dec = small.decoder(lm)
    for c in (small, large, small, large):
        host, gap = c.host(dec)
        assert gap >= MIN_GAP, gap
        assert_same_beams(c.device(dec), host)
    dec.close()


def test_workspace_reuse_with_the_label_cutoff():
    """A longer decode leaves candidate rows behind: the shorter one after it
    must read none of them."""
    small = Case(seed=236, T=5, B=2, V=12, beam=4, top_n=4)
    large = Case(seed=236, T=20, B=9, V=12, beam=4, top_n=4)   # the same model (same seed and V)
    assert small.text == large.text
    lm = small.lm()
    lm.upload()
    dec = small.decoder(lm)
    for c in (large, small, large, small):
        host, gap = c.host(dec)
        assert gap >= MIN_GAP, gap
        assert_same_beams(c.device(dec), host)
    ref, ref_gap = small.reference()
    assert ref_gap >= MIN_GAP, ref_gap
    assert_same_beams(small.device(dec), ref)
    dec.close()


def test_decode_before_upload_is_refused():
    c = Case(seed=233, T=4, B=1, V=5, beam=2)
    lm = c.lm()
    dec = c.decoder(lm)
    with pytest.raises(asr.AsrError) as e:
        dec.decode(c.emis, is_log=True)
    assert e.value.status == asr.ASR_ERR_STATE
    lm.upload()
    dec.decode(c.emis, is_log=True)
    assert len(dec.beams(4)[0]) >= 1
    dec.close()


def test_worked_example_on_the_device():
    lm = asr.NGramLM.from_string(WORKED_ARPA)
    lm.upload()
    dec = asr.CTCLMDecoder(3, 1, lm, lm.label_tokens(WORKED_LABELS), 1.0, 0.0)
    dec.decode_host(WORKED_EMIS, is_log=False)
    host = dec.beams(8)
    dec.decode(WORKED_EMIS, is_log=False)
    dev = dec.beams(8)
    assert_same_beams(dev, host)
    assert dev[0][0][0] == WORKED_BEST and dec.best()[0] == [WORKED_BEST]
    # the plain decoder pruned "b" at frame 0; re-ranking its beam with the same LM cannot bring "ba" back
    plain = asr.CTCDecoder(3, 1, 0)
    plain.decode(WORKED_EMIS, is_log=False)
    rescored = plain.lm_rescore(8, lm, 1.0, 0.0, lm.label_mapper(WORKED_LABELS), bos=True, eos=False)
    assert [r[0] for r in rescored[0]] == [[1]]
    plain.close()
    dec.close()


def test_beam_decoder_with_model_path(tmp_path):
    import torch
    c = Case(seed=234, T=10, B=3, V=7, beam=4, order=3, alpha=0.6, beta=0.4)
    path = tmp_path / "model.arpa"
    path.write_text(c.text)
    labels = ["_"] + c.labels[1:]   # ctcdecode style: the blank has a string of its own
    probs = np.ascontiguousarray(c.emis.transpose(1, 0, 2))   # [B][T][V] log-probabilities
    lens = np.array([10, 4, 7], np.int32)
    bd = asr.CTCBeamDecoder(labels, model_path=str(path), alpha=0.6, beta=0.4, cutoff_top_n=40, beam_width=4,
                            log_probs_input=True)
    lm = c.lm()
    lm.upload()
    dec = asr.CTCLMDecoder(7, 4, lm, lm.label_tokens(labels), 0.6, 0.4, bos=True, eos=False, top_n=40)
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
