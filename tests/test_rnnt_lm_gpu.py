"""GPU checks of the LM-fused transducer beam search (asr_rnnt_beam_lm) against
tests/rnnt_lm_reference.py and the host twin: tokens, timesteps, lengths,
counts, n_tokens and lm_log10 exactly, the LM part of the total bit for bit, am
and total within test_rnnt_beam_gpu.py's bound; zero weights against
asr_rnnt_beam, batch independence, a second call on the same workspace, and the
refusals that come before a launch; the option table (a moved blank, both flags
and neither, beta < 0, a zero weight, K > V, an order-8 model) and what only the
device can show: nothing written beyond the counts, the optional outputs left
out, and a workspace that holds another search.

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


def raw(dec, fuse, e, lens, K, work=None, calls=1, nbest=None, max_out=None, fill=0, arrays=True, extras=True,
        zero_work=False):
    """Every output array of asr_rnnt_beam_lm (fuse) or asr_rnnt_beam (fuse None), downloaded as it is: tokens and
    timesteps [B][nbest][max_out], lengths and totals [B][nbest], counts [B], am, lm_log10 and n_tokens [B][nbest].
    The arrays hold the byte `fill` before the call; arrays False passes no token and timestep arrays (max_out = 0),
    extras False no am, lm_log10 and n_tokens; zero_work clears a workspace made here."""
    e = np.ascontiguousarray(e, np.float32)
    T, nb = e.shape[0], e.shape[1]
    nbest = K if nbest is None else nbest
    max_out = T if max_out is None else max_out
    mo = max(max_out, 1)
    dec.upload()
    d_enc, d_ln = asr._upload(e, 0), asr._upload(np.ascontiguousarray(lens, np.int32), 0)
    sizes = [4 * nb * nbest * mo, 4 * nb * nbest * mo, 4 * nb * nbest, 8 * nb * nbest, max(4 * nb, 16), 8 * nb * nbest,
             8 * nb * nbest, 4 * nb * nbest]
    out = []
    for _ in range(calls):
        o = [asr.DeviceBytes(n) for n in sizes]
        for x in o:      # the same bytes under every entry the kernel leaves unwritten
            asr.check(asr.lib().asr_memset(x.ptr, fill, x.nbytes, None), "asr_memset")
        if work is None:
            work = asr.DeviceBytes(dec.beam_workspace_bytes(T, nb, K) if fuse is None else
                                   dec.beam_lm_workspace_bytes(fuse, T, nb, K))
            if zero_work:
                asr.check(asr.lib().asr_memset(work.ptr, 0, work.nbytes, None), "asr_memset")
        tk, ts = (o[0].ptr, o[1].ptr) if arrays else (0, 0)
        if fuse is None:
            dec.beam_search_device(d_enc.ptr, T, nb, K, nbest, max_out, tk, ts, o[2].ptr, o[3].ptr, o[4].ptr, work.ptr,
                                   d_ln.ptr)
        else:
            am, lml, nt = (o[5].ptr, o[6].ptr, o[7].ptr) if extras else (0, 0, 0)
            dec.beam_search_lm_device(fuse, d_enc.ptr, T, nb, K, nbest, max_out, tk, ts, o[2].ptr, o[3].ptr, o[4].ptr,
                                      work.ptr, am, lml, nt, d_ln.ptr)
        asr.check(asr.lib().asr_stream_sync(None), "asr_stream_sync")
        shapes = [((nb, nbest, mo), np.int32), ((nb, nbest, mo), np.int32), ((nb, nbest), np.int32),
                  ((nb, nbest), np.float64), ((nb,), np.int32), ((nb, nbest), np.float64), ((nb, nbest), np.float64),
                  ((nb, nbest), np.int32)]
        out.append([asr._download(x, sh, dt, 0) for x, (sh, dt) in zip(o, shapes)])
    return out if calls > 1 else out[0]


def untouched(a, written, fill=0x5A):
    """Every entry of `a` outside the mask `written` still holds the fill byte."""
    return bool((a.view(np.uint8).reshape(a.shape + (a.itemsize,))[~written] == fill).all())


def fuse_of(dec, lm, case):
    lm.upload()
    return dec._lm_handle(lm, case.alpha, case.beta, lc.tok_of_label(case), case.bos, case.eos)


@pytest.mark.parametrize("case", lc.OPTION_CASES, ids=lambda c: c.name)
def test_option_kernel_matches_reference(case):
    """The moved blank, both flags and neither, beta < 0, a zero weight, K > V and the order-8 model whose contexts
    are cut to seven tokens: the kernel against the reference and the twin."""
    w, enc, ref, _plain = lc.reference(case)
    lc.check_conditions(case, ref, need_merge=lc.OPTION_NEEDS_MERGE[case.name])
    lc.check_option(case)
    res = run_case(case, need_merge=lc.OPTION_NEEDS_MERGE[case.name])
    assert [[len(h[0]) for h in u] for u in res] == ref["lens"]
    if case.name == "f-a0":     # alpha = 0: another model over the same tokens gives the same tokens and totals
        other = case._replace(lm=lc.BI16)
        dec, lm = lc.make_decoder(asr, other, w), lc.make_lm(asr, other)
        again = dec.beam_search(enc, rc.lengths_of(other.model), lm=lm, **lc.search_kwargs(other))
        assert [[(h[0], h[1], h[2], h[3], h[5]) for h in u] for u in again] == \
            [[(h[0], h[1], h[2], h[3], h[5]) for h in u] for u in res]
        dec.close()


def test_nothing_is_written_beyond_the_counts():
    """f-bm-k8 (both flags: the </s> term reorders a list within its first two) at nbest = 2 < K and max_out = 2
    below a length: what lies below the counts and the cut lengths is the full call's and the reference's, the
    lengths are the uncut ones, and every other byte of every array is as it was."""
    case = next(c for c in lc.OPTION_CASES if c.name == "f-bm-k8")
    w, enc, ref, _plain = lc.reference(case)
    lc.check_option(case)
    assert max(n for u in ref["lens"] for n in u) > 2
    dec, lm = lc.make_decoder(asr, case, w), lc.make_lm(asr, case)
    fuse = fuse_of(dec, lm, case)
    ln = rc.lengths_of(case.model)
    K, B = case.beam, enc.shape[1]
    full = raw(dec, fuse, enc, ln, K)
    for max_out in (2, 0):
        cut = raw(dec, fuse, enc, ln, K, nbest=2, max_out=max_out, fill=0x5A, arrays=max_out > 0)
        tok, ts, hl, tot, nh, am, lml, nt = cut
        assert nh.tolist() == [min(len(u), 2) for u in ref["hyps"]] == np.minimum(full[4], 2).tolist()
        wrote3, wrote2 = np.zeros(tok.shape, bool), np.zeros(hl.shape, bool)
        for b in range(B):
            for j in range(nh[b]):
                n = min(int(hl[b, j]), max_out)
                wrote2[b, j] = True
                wrote3[b, j, :n] = True
                assert hl[b, j] == full[2][b, j] == ref["lens"][b][j] == nt[b, j]
                assert (tot[b, j], am[b, j], lml[b, j]) == (full[3][b, j], full[5][b, j], full[6][b, j])
                assert lml[b, j] == ref["hyps"][b][j][4]
                assert tok[b, j, :n].tolist() == full[0][b, j, :n].tolist() == ref["hyps"][b][j][0][:n]
                assert ts[b, j, :n].tolist() == full[1][b, j, :n].tolist() == ref["hyps"][b][j][1][:n]
        assert not wrote2[1, 1:].any() and nh[1] == 1      # the zero-length utterance: one empty hypothesis
        assert untouched(tok, wrote3) and untouched(ts, wrote3)
        assert all(untouched(a, wrote2) for a in (hl, tot, am, lml, nt))
    dec.close()


def test_optional_outputs_left_out():
    """f-bm-k8 without am, lm_log10 and n_tokens: the other arrays hold the bytes of the call that passes them, and
    the three left out are not touched."""
    case = next(c for c in lc.OPTION_CASES if c.name == "f-bm-k8")
    w, enc, _ref, _plain = lc.reference(case)
    dec, lm = lc.make_decoder(asr, case, w), lc.make_lm(asr, case)
    fuse = fuse_of(dec, lm, case)
    ln = rc.lengths_of(case.model)
    full = raw(dec, fuse, enc, ln, case.beam)
    bare = raw(dec, fuse, enc, ln, case.beam, extras=False)
    assert int(full[4].sum()) > enc.shape[1]
    for i in range(5):
        assert np.array_equal(full[i], bare[i]), i
    for i in (5, 6, 7):
        assert not bare[i].any() and full[i].any(), i
    dec.close()


def test_a_workspace_that_holds_another_search():
    """f-o8 (T = 12, K = 4), then f-v3 (T = 6, K = 16, another model and LM), then f-bm-k8 in one workspace sized for
    the largest: each finds the node table, the c slices, the logits and the LM rows of another search, and gives
    the bytes of its own run in a zeroed workspace.  (test_rnnt_beam_gpu.py does the same for asr_rnnt_beam.)"""
    runs = []
    for name in ("f-o8", "f-v3", "f-bm-k8"):
        case = next(c for c in lc.OPTION_CASES if c.name == name)
        w, enc, _ref, _plain = lc.reference(case)
        dec, lm = lc.make_decoder(asr, case, w), lc.make_lm(asr, case)
        runs.append((case, enc, dec, fuse_of(dec, lm, case)))
    work = asr.DeviceBytes(max(d.beam_lm_workspace_bytes(f, e.shape[0], e.shape[1], c.beam) for c, e, d, f in runs))
    asr.check(asr.lib().asr_memset(work.ptr, 0, work.nbytes, None), "asr_memset")
    for case, enc, dec, fuse in runs:
        ln = rc.lengths_of(case.model)
        shared = raw(dec, fuse, enc, ln, case.beam, work=work)
        fresh = raw(dec, fuse, enc, ln, case.beam, zero_work=True)
        assert int(fresh[4].sum()) > enc.shape[1]
        for a, b in zip(shared, fresh):
            assert np.array_equal(a, b), case.name
    for _c, _e, dec, _f in runs:
        dec.close()


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
