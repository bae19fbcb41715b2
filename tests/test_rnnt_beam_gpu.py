"""GPU checks of the transducer beam-search kernel (asr_rnnt_beam) against
tests/rnnt_beam_reference.py and the host twin: tokens, timesteps, lengths and
hypothesis counts exactly, scores within test_rnnt_gpu.py's bound for totals;
K = 1 against the greedy kernel, batch independence, exact token ties, the
upper range of shapes and zero-length utterances.

Measured on an MI355X (max over the case of |gpu - ref| / ((1 + |ref|) * frames
walked)) are in DESIGN.md §25; the bound is 2e-5."""
import numpy as np
import pytest

import rnnt_beam_cases as bc
import rnnt_cases as rc
from conftest import asr
from rnnt_beam_reference import BeamReference

pytestmark = pytest.mark.gpu

TOL = 2e-5    # test_rnnt_gpu.py's bound for totals: |gpu - ref| <= TOL * (1 + |ref|) * frames walked


@pytest.fixture(scope="module", autouse=True)
def _device():
    asr.set_device(0)


def compare(name, res, ref, host=None):
    err = 0.0
    for b, (got, want) in enumerate(zip(res, ref["hyps"])):
        for (_tok, _ts, score), (_rt, _rs, rscore) in zip(got, want):
            err = max(err, abs(score - rscore) / ((1 + abs(rscore)) * max(ref["frames"][b], 1)))
    print(f"rnnt beam {name}: max score err per frame {err:.3e} (bound {TOL:.0e})")
    assert [len(u) for u in res] == [len(u) for u in ref["hyps"]]
    for b, (got, want) in enumerate(zip(res, ref["hyps"])):
        for j, ((tok, ts, _s), (rtok, rts, _rs)) in enumerate(zip(got, want)):
            assert tok == rtok and ts == rts, (b, j)
            if host is not None:
                assert tok == host[b][j][0] and ts == host[b][j][1], (b, j)
    assert err <= TOL


def test_the_suite_has_a_deep_merge_and_a_short_frame():
    bc.check_suite(bc.SMALL_CASES + bc.WIDE_CASES)


@pytest.mark.parametrize("case", bc.SMALL_CASES + bc.WIDE_CASES, ids=lambda c: c.name)
def test_kernel_matches_reference(case):
    w, enc, ref = bc.reference(case)
    bc.check_conditions(case, ref)
    dec = bc.make_decoder(asr, case, w)
    ln = rc.lengths_of(case.model)
    res = dec.beam_search(enc, ln, beam=case.beam)
    host = dec.beam_search_host(enc, ln, beam=case.beam)
    assert [len(u) for u in host] == [len(u) for u in res]
    compare(case.name, res, ref, host)
    # the uncut lengths, and nbest < K
    two = dec.beam_search(enc, ln, beam=case.beam, nbest=2, max_out=1)
    for b in range(len(res)):
        assert [(t[:1], s[:1], sc) for t, s, sc in res[b][:2]] == two[b]
    dec.close()


@pytest.mark.parametrize("case", bc.UPPER_CASES, ids=lambda c: c.name)
def test_upper_range(case):
    w, enc, ref = bc.reference(case)
    bc.check_conditions(case, ref, need_merge=bc.UPPER_NEEDS_MERGE[case.name])
    dec = bc.make_decoder(asr, case, w)
    res = dec.beam_search(enc, rc.lengths_of(case.model), beam=case.beam)
    compare(case.name, res, ref)
    dec.close()


@pytest.mark.parametrize("case", [bc.SMALL_CASES[0], bc.SMALL_CASES[6]], ids=lambda c: c.name)
def test_beam_one_is_the_greedy_kernel(case):
    """K = 1 against asr_rnnt_greedy on a max_symbols = 1 handle of the same weights."""
    w, enc = rc.make_model(case.model)
    dec = bc.make_decoder(asr, case, w)          # max_symbols = 1
    ln = rc.lengths_of(case.model)
    greedy, _state, cnt = dec.decode(enc, ln)
    beam = dec.beam_search(enc, ln, beam=1)
    assert int(cnt.sum()) > 0
    for b in range(enc.shape[1]):
        assert len(beam[b]) == 1
        assert beam[b][0][0] == greedy[b][0] and beam[b][0][1] == greedy[b][1]
        total = greedy[b][3]
        assert abs(beam[b][0][2] - total) <= TOL * (1 + abs(total)) * max(int(ln[b]), 1)
    dec.close()


def test_batch_independent():
    """S2 at K = 3: five utterances span two workgroups; the first two alone give equal bits."""
    case = bc.SMALL_CASES[2]
    w, enc, _ref = bc.reference(case)
    dec = bc.make_decoder(asr, case, w)
    ln = rc.lengths_of(case.model)
    T, B, K = enc.shape[0], enc.shape[1], case.beam

    def raw(e, lens):
        """Every output array of one asr_rnnt_beam call, downloaded as it is."""
        e = np.ascontiguousarray(e, np.float32)
        nb = e.shape[1]
        dec.upload()
        d_enc, d_ln = asr._upload(e, 0), asr._upload(np.ascontiguousarray(lens, np.int32), 0)
        outs = [asr.DeviceBytes(4 * nb * K * T), asr.DeviceBytes(4 * nb * K * T), asr.DeviceBytes(4 * nb * K),
                asr.DeviceBytes(8 * nb * K), asr.DeviceBytes(max(4 * nb, 16))]
        for o in outs:      # the same bytes under every entry the kernel leaves unwritten
            asr.check(asr.lib().asr_memset(o.ptr, 0, o.nbytes, None), "asr_memset")
        work = asr.DeviceBytes(dec.beam_workspace_bytes(T, nb, K))
        dec.beam_search_device(d_enc.ptr, T, nb, K, K, T, outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr,
                               outs[4].ptr, work.ptr, d_ln.ptr)
        asr.check(asr.lib().asr_stream_sync(None), "asr_stream_sync")
        return (asr._download(outs[0], (nb, K, T), np.int32, 0), asr._download(outs[1], (nb, K, T), np.int32, 0),
                asr._download(outs[2], (nb, K), np.int32, 0), asr._download(outs[3], (nb, K), np.float64, 0),
                asr._download(outs[4], (nb,), np.int32, 0))

    all5 = raw(enc, ln)
    first2 = raw(enc[:, :2], ln[:2])
    assert int(all5[4].sum()) > B - 1
    for a, f in zip(all5, first2):
        assert np.array_equal(a[:2], f)
    dec.close()


SMALL = (4, 3, 12, 16, 32, 32, 17, 1)    # T, B, E, D, Hp, J, V, L


def _tie_case(blank, src, dup, seed):
    case = rc.Case("tie", SMALL, blank, 1, "relu", (4, 4, 2), seed, 4.0, 1.5)
    w, enc = rc.make_model(case)
    w["w_out"][:, dup] = w["w_out"][:, src]
    w["b_out"][dup] = w["b_out"][src] = 4.0     # the pair leads at every frame
    return case, w, enc


def tie_references(blank, src, dup, seed):
    """The tie case with its conditions, asserted on the reference alone.
    Two columns of W_out are equal and lead every frame, so at K = 1 the walk
    emits one of the two at every frame, and at K = 2 the beam is, after every
    frame, one hypothesis extended by both: an exact tie, kept whole."""
    case, w, enc = _tie_case(blank, src, dup, seed)
    lo, hi = min(src, dup), max(src, dup)
    ref1 = BeamReference(w, blank, case.act, 1).search(enc, case.lengths, beam=1)
    ref2 = BeamReference(w, blank, case.act, 1).search(enc, case.lengths, beam=2)
    bound = 1e-3 * (1 + ref2["max_abs_logit"])
    # K = 1: the tie is the top of every frame (margin 0), the lower index wins, and every other choice is away
    # from a near-tie: the same model with the higher column pushed down walks the same way with a margin
    assert min(ref1["margin"]) == 0.0
    assert all(u[0][0] == [lo] * n for u, n in zip(ref1["hyps"], case.lengths))
    w2 = dict(w, b_out=w["b_out"].copy())
    w2["b_out"][hi] -= 30.0
    clean = BeamReference(w2, blank, case.act, 1).search(enc, case.lengths, beam=1)
    assert [u[0][0] for u in clean["hyps"]] == [u[0][0] for u in ref1["hyps"]] and min(clean["margin"]) >= bound
    # K = 2: both kept, in token order, with equal scores; what is decided beside the ties has a margin
    for u, n in zip(ref2["hyps"], case.lengths):
        assert len(u) == 2 and u[0][2] == u[1][2] and len(u[0][0]) == n
        assert u[0][0][:-1] == u[1][0][:-1] and u[0][0][-1] == lo and u[1][0][-1] == hi
    assert min(ref2["margin"]) == 0.0 and min(ref2["margin_nonzero"]) >= bound
    return case, w, enc, ref1, ref2


@pytest.mark.parametrize("blank,src,dup,seed", [(8, 2, 14, 2), (0, 5, 16, 27), (16, 0, 9, 1)])
def test_exact_token_tie(blank, src, dup, seed):
    """At K = 1 the lower index wins; at K = 2 with both kept, they come out in token order."""
    case, w, enc, ref1, ref2 = tie_references(blank, src, dup, seed)
    dec = rc.make_decoder(asr, case, w)
    ln = rc.lengths_of(case)
    got1 = dec.beam_search(enc, ln, beam=1)
    got2 = dec.beam_search(enc, ln, beam=2)
    for b in range(enc.shape[1]):
        assert [(h[0], h[1]) for h in got1[b]] == [(h[0], h[1]) for h in ref1["hyps"][b]]
        assert [(h[0], h[1]) for h in got2[b]] == [(h[0], h[1]) for h in ref2["hyps"][b]]
        assert got2[b][0][2] == got2[b][1][2]       # equal bits: the same row and equal logits
    dec.close()


def test_zero_length_among_others():
    case = bc.SMALL_CASES[3]
    w, enc, ref = bc.reference(case)
    dec = bc.make_decoder(asr, case, w)
    ln = np.array([9, 0, 0, 9, 0], np.int32)
    res = dec.beam_search(enc, ln, beam=case.beam)
    for b in (1, 2, 4):
        assert res[b] == [([], [], 0.0)]
    for b in (0, 3):
        assert [h[0] for h in res[b]] == [h[0] for h in ref["hyps"][b]]
    every = dec.beam_search(enc, np.zeros(5, np.int32), beam=case.beam)
    assert every == [[([], [], 0.0)]] * 5
    dec.close()
