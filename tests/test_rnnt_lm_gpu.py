"""GPU checks of the LM-fused transducer beam search (asr_rnnt_beam_lm) against
tests/rnnt_lm_reference.py and the host twin: tokens, timesteps, lengths,
counts, n_tokens and lm_log10 exactly, the LM part of the total bit for bit, am
and total within test_rnnt_beam_gpu.py's bound; zero weights against
asr_rnnt_beam, batch independence, a second call on the same workspace, and the
refusals that come before a launch.

Measured on an MI355X (max over the case of |gpu - ref| / ((1 + |ref|) * frames
walked)) are in DESIGN.md §26; the bound is 2e-5."""
import numpy as np
import pytest

import rnnt_cases as rc
import rnnt_lm_cases as lc
from conftest import asr

pytestmark = pytest.mark.gpu

TOL = 2e-5    # |gpu - ref| <= TOL * (1 + |ref|) * frames walked


def per_frame(got, want, frames):
    return abs(got - want) / ((1 + abs(want)) * max(frames, 1))


@pytest.fixture(scope="module", autouse=True)
def _device():
    asr.set_device(0)


def test_the_suite_meets_its_conditions():
    lc.check_suite(lc.SMALL_CASES + lc.WIDE_CASES)


def run_case(case, need_merge=True, twin=True):
    w, enc, ref, _plain = lc.reference(case)
    lc.check_conditions(case, ref, need_merge)
    dec = lc.make_decoder(asr, case, w)
    lm = lc.make_lm(asr, case)
    ln = rc.lengths_of(case.model)
    res = dec.beam_search(enc, ln, lm=lm, **lc.search_kwargs(case))
    lc.compare(case.name, res, ref, per_frame, TOL)
    if twin:   # lm_log10 and the LM part of the total are the twin's bits
        host = dec.beam_search_host(enc, ln, lm=lm, **lc.search_kwargs(case))
        for b, (got, want) in enumerate(zip(res, host)):
            assert [(g[0], g[1], g[4], g[5]) for g in got] == [(h[0], h[1], h[4], h[5]) for h in want], b
    b0 = case.model.lengths.index(0)
    assert len(res[b0]) == 1 and res[b0][0][0] == [] and res[b0][0][3] == 0.0 and res[b0][0][5] == 0
    dec.close()
    return res


@pytest.mark.parametrize("case", lc.SMALL_CASES + lc.WIDE_CASES, ids=lambda c: c.name)
def test_kernel_matches_reference(case):
    run_case(case)


@pytest.mark.parametrize("case", lc.UPPER_CASES, ids=lambda c: c.name)
def test_upper_range(case):
    run_case(case, need_merge=lc.UPPER_NEEDS_MERGE[case.name], twin=False)


def raw(dec, fuse, e, lens, K, work=None, calls=1):
    """Every output array of asr_rnnt_beam_lm (fuse) or asr_rnnt_beam (fuse None), downloaded as it is."""
    e = np.ascontiguousarray(e, np.float32)
    T, nb = e.shape[0], e.shape[1]
    dec.upload()
    d_enc, d_ln = asr._upload(e, 0), asr._upload(np.ascontiguousarray(lens, np.int32), 0)
    sizes = [4 * nb * K * T, 4 * nb * K * T, 4 * nb * K, 8 * nb * K, max(4 * nb, 16), 8 * nb * K, 8 * nb * K, 4 * nb * K]
    out = []
    for _ in range(calls):
        o = [asr.DeviceBytes(n) for n in sizes]
        for x in o:      # the same bytes under every entry the kernel leaves unwritten
            asr.check(asr.lib().asr_memset(x.ptr, 0, x.nbytes, None), "asr_memset")
        if fuse is None:
            work = work or asr.DeviceBytes(dec.beam_workspace_bytes(T, nb, K))
            dec.beam_search_device(d_enc.ptr, T, nb, K, K, T, o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr, o[4].ptr, work.ptr,
                                   d_ln.ptr)
        else:
            work = work or asr.DeviceBytes(dec.beam_lm_workspace_bytes(fuse, T, nb, K))
            dec.beam_search_lm_device(fuse, d_enc.ptr, T, nb, K, K, T, o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr, o[4].ptr,
                                      work.ptr, o[5].ptr, o[6].ptr, o[7].ptr, d_ln.ptr)
        asr.check(asr.lib().asr_stream_sync(None), "asr_stream_sync")
        shapes = [((nb, K, T), np.int32), ((nb, K, T), np.int32), ((nb, K), np.int32), ((nb, K), np.float64),
                  ((nb,), np.int32), ((nb, K), np.float64), ((nb, K), np.float64), ((nb, K), np.int32)]
        out.append([asr._download(x, sh, dt, 0) for x, (sh, dt) in zip(o, shapes)])
    return out if calls > 1 else out[0]


@pytest.mark.parametrize("case", [lc.SMALL_CASES[1], lc.SMALL_CASES[3]], ids=lambda c: c.name)
def test_zero_weights_give_the_unfused_bytes(case):
    """alpha = beta = 0 without </s>: tokens, timesteps, lengths, scores and counts of asr_rnnt_beam."""
    w, enc, _ref, _plain = lc.reference(case)
    dec = lc.make_decoder(asr, case, w)
    lm = lc.make_lm(asr, case)
    lm.upload()
    ln = rc.lengths_of(case.model)
    fuse = dec._lm_handle(lm, 0.0, 0.0, lc.tok_of_label(case), case.bos, False)
    fused, plain = raw(dec, fuse, enc, ln, case.beam), raw(dec, None, enc, ln, case.beam)
    assert int(plain[4].sum()) > enc.shape[1]
    for i in range(5):
        assert np.array_equal(fused[i], plain[i]), i
    assert np.array_equal(fused[5], plain[3])       # am = total
    dec.close()


def test_batch_independent_and_repeatable():
    """S2 at K = 4: five utterances span two workgroups; the first two alone give equal bits, and so does a second
    call on the same workspace."""
    case = lc.SMALL_CASES[1]
    w, enc, _ref, _plain = lc.reference(case)
    dec = lc.make_decoder(asr, case, w)
    lm = lc.make_lm(asr, case)
    lm.upload()
    ln = rc.lengths_of(case.model)
    fuse = dec._lm_handle(lm, case.alpha, case.beta, lc.tok_of_label(case), case.bos, case.eos)
    work = asr.DeviceBytes(dec.beam_lm_workspace_bytes(fuse, enc.shape[0], enc.shape[1], case.beam))
    first, second = raw(dec, fuse, enc, ln, case.beam, work=work, calls=2)
    first2 = raw(dec, fuse, enc[:, :2], ln[:2], case.beam)
    assert int(first[4].sum()) > enc.shape[1] - 1
    for a, b, f in zip(first, second, first2):
        assert np.array_equal(a, b)
        assert np.array_equal(a[:2], f)
    dec.close()


def test_refusals_before_a_launch():
    case = lc.SMALL_CASES[0]
    w = rc.make_model(case.model)[0]
    lib, p = asr.lib(), asr._ptr
    E = case.model.shape[2]
    enc = np.zeros((2, 2, E), np.float32)
    i32, f64 = np.zeros(64, np.int32), np.zeros(64, np.float64)
    tail = [p(enc), None, 2, 2, 4, 2, 3, p(i32), p(i32), p(i32), p(f64), None, None, None, p(i32), p(f64), None]
    # the model not uploaded, then the LM not uploaded
    dec = lc.make_decoder(asr, case, w)
    lm = lc.make_lm(asr, case)
    fuse = dec._lm_handle(lm, 0.5, 0.5, lc.tok_of_label(case), True, False)
    assert lib.asr_rnnt_beam_lm(fuse, *tail) == asr.ASR_ERR_STATE
    dec.upload()
    assert lib.asr_rnnt_beam_lm(fuse, *tail) == asr.ASR_ERR_STATE
    dec.close()
    # beyond the LDS limit
    big = rc.Case("big", (1, 1, 8, 16, 816, 816, 17, 1), 0, 1, "relu", (1,), 0, 1.0, 0.0)
    dec = rc.make_decoder(asr, big)
    lm.upload()
    fuse = dec._lm_handle(lm, 0.5, 0.5, lc.tok_of_label(case), True, False)
    enc = np.zeros((1, 1, 8), np.float32)
    args = [fuse, p(enc), None, 1, 1, 1, 1, 1, p(i32), p(i32), p(i32), p(f64), None, None, None, p(i32), p(f64), None]
    assert lib.asr_rnnt_beam_lm(*args) == asr.ASR_ERR_UNSUPPORTED
    dec.close()
