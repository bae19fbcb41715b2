"""The stateless-predictor transducer's host twins (asr_rnnt_greedy_stateless_host
and the dual-kind asr_rnnt_beam_host / asr_rnnt_align_host) against the float64
references, and TransducerDecoder.from_icefall against torch's own forward of
the stand-in modules.  No GPU."""
import math

import numpy as np
import pytest
import torch

import asr_amd as asr
import rnnt_align_cases as ac
import rnnt_cases as rc
import rnnt_lm_cases as lc
import rnnt_stateless_cases as sc

TIGHT = 1e-9     # fp64 twin against fp64 reference, relative to 1 + |ref|
SMALL = [c for c in sc.GREEDY_CASES if c.name != "limit-c2"]


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_greedy_twin_matches_reference(case):
    w, enc, ref = sc.reference(case)
    rc.check_conditions(case, ref)
    dec = sc.make_decoder(asr, case, w)
    assert dec.context == case.context and dec.info()["L"] == 0 and dec.state_shape(3) == (3, case.context)
    res, ctx, cnt = dec.decode_host(enc, sc.lengths_of(case))
    assert cnt.tolist() == ref["count"]
    assert np.array_equal(ctx, sc._ref(sc.StatelessReference, case, w, 1).context_of(ref["state"]))
    for b, (tok, ts, lp, total) in enumerate(res):
        assert tok == ref["tokens"][b] and ts == ref["timesteps"][b]
        assert np.allclose(lp, ref["logps"][b], rtol=0, atol=TIGHT * (1 + np.abs(ref["logps"][b]).max(initial=0)))
        assert abs(total - ref["total"][b]) <= TIGHT * (1 + abs(ref["total"][b])) * max(len(ref["frames"][b]), 1)


def test_chunked_twin_equals_whole():
    case = sc.by_name("ragged-c2")
    w, enc = sc.make_model(case)
    dec = sc.make_decoder(asr, case, w)
    sc.check_chunked(lambda e, ln, st: dec.decode_host(e, ln, state=st), case, enc)


@pytest.mark.parametrize("name,beam", sc.BEAMS)
def test_beam_twin_matches_reference(name, beam):
    case, w, enc, ref = sc.beam_reference(name, beam)
    sc.check_beam_conditions(name, beam, ref)
    res = sc.make_decoder(asr, case, w).beam_search_host(enc, sc.lengths_of(case), beam=beam)
    assert [[(h[0], h[1]) for h in u] for u in res] == [[(h[0], h[1]) for h in u] for u in ref["hyps"]]
    for u, r, frames in zip(res, ref["hyps"], ref["frames"]):
        for h, want in zip(u, r):
            assert abs(h[2] - want[2]) <= TIGHT * (1 + abs(want[2])) * max(frames, 1)


def test_lm_fused_beam_twin_matches_reference():
    case, w, enc, ref = sc.lm_reference()
    res = sc.make_decoder(asr, case.model, w).beam_search_host(enc, sc.lengths_of(case.model),
                                                              lm=lc.make_lm(asr, case), **lc.search_kwargs(case))
    lc.compare("stateless twin " + case.name, res, ref, lambda g, r, frames: abs(g - r) / ((1 + abs(r)) * max(frames, 1)),
               TIGHT)


@pytest.mark.parametrize("topology", ac.TOPOLOGIES)
def test_align_twin_matches_reference(topology):
    case, w, enc, targets, utt, ref = sc.align_reference("ragged-c2", topology)
    score, vscore, frames = sc.make_decoder(asr, case, w).align_host(enc, targets, sc.lengths_of(case), utt, topology)
    for n, r in enumerate(ref):
        assert ac.frames_comparable(r)
        for g, want in ((score[n], r["score"]), (vscore[n], r["vscore"])):
            assert g == want if math.isinf(want) else abs(g - want) <= TIGHT * (1 + abs(want)) * max(r["terms"], 1)
        assert frames[n].tolist() == r["frames"]


@pytest.mark.parametrize("groups", [1, 4, 16])
def test_from_icefall_reproduces_the_modules(groups):
    """The expanded w_ctx against torch's forward of the stand-in decoder in float64: embedding, grouped Conv1d over
    the context, ReLU (icefall's Decoder.forward with need_pad = False)."""
    case = sc.by_name("ragged-c2")._replace(groups=groups if groups > 1 else 0, bias=True, context=3)
    w, _enc = sc.make_model(case)
    dmod, jmod = sc.standin(case, w)
    dec = asr.TransducerDecoder.from_icefall(dmod, jmod)
    assert dec.context == 3 and dec.desc.start_fill == -1 and dec.desc.blank == case.blank
    assert np.array_equal(dec.weights["w_ctx"], w["w_ctx"])
    ys = torch.tensor([[3, 0, 16], [5, 5, 1]])
    want = torch.relu(dmod.double().conv(dmod.embedding(ys).permute(0, 2, 1))[:, :, 0]).detach().numpy()
    e = w["emb"].astype(np.float64)
    got = np.maximum(sum(e[ys[:, i].numpy()] @ dec.weights["w_ctx"][i].astype(np.float64) for i in range(3))
                     + dec.weights["b_ctx"], 0)
    assert np.allclose(got, want, rtol=0, atol=1e-12)
    padded = sc.standin(case._replace(fill_blank=True), w)
    assert asr.TransducerDecoder.from_icefall(*padded).desc.start_fill == case.blank


def test_a_handle_of_the_wrong_kind_is_refused_by_the_four_greedy_entry_points():
    """ASR_ERR_UNSUPPORTED before any HIP call: the device entry points get pointers they never follow."""
    case = sc.by_name("one-c2")
    sl, lstm = sc.make_decoder(asr, case), rc.make_decoder(asr, rc.SMALL_CASES[0])
    x = np.zeros(64, np.float64)
    p = asr._ptr(x)
    tail = (p, None, 1, 1, 1, None, None, p, p, p, p, p)
    lib = asr.lib()
    assert lib.asr_rnnt_context(sl.h) == case.context and lib.asr_rnnt_context(lstm.h) == 0
    assert lib.asr_rnnt_context(None) == 0
    assert lib.asr_rnnt_greedy(sl.h, *tail, p, None) == asr.ASR_ERR_UNSUPPORTED
    assert lib.asr_rnnt_greedy_host(sl.h, *tail, None) == asr.ASR_ERR_UNSUPPORTED
    assert lib.asr_rnnt_greedy_stateless(lstm.h, *tail, p, None) == asr.ASR_ERR_UNSUPPORTED
    assert lib.asr_rnnt_greedy_stateless_host(lstm.h, *tail, None) == asr.ASR_ERR_UNSUPPORTED
