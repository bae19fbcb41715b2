"""The token-and-duration transducer's kernel (asr_rnnt_greedy_tdt) against the
float64 reference of rnnt_tdt_cases.py and the host twin, and the invariants of
the kernel.  Bound: test_rnnt_gpu.py's, 2e-5 * (1 + |ref|) per token log-prob
and per summed term of a total; an evaluation sums two terms here."""
import numpy as np
import pytest

import asr_amd as asr
import rnnt_cases as rc
import rnnt_tdt_cases as tc

pytestmark = pytest.mark.gpu
TOL = 2e-5
CASE4 = tc.by_name("4-unordered")


@pytest.fixture(autouse=True)
def _device():
    asr.set_device(0)


@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c.name)
def test_kernel_matches_reference_and_twin(case):
    w, enc, ref = tc.reference(case)
    tc.check_conditions(case, ref)
    dec, ln = tc.make_decoder(asr, case, w), tc.lengths_of(case)
    res, state, cnt = dec.decode(enc, ln)
    tc.compare_exact(case, res, state, cnt, ref)
    host, hstate, hcnt = dec.decode_host(enc, ln)
    assert hcnt.tolist() == cnt.tolist() and hstate[1].tolist() == state[1].tolist()
    assert [(r[0], r[1], r[4]) for r in res] == [(r[0], r[1], r[4]) for r in host]
    err_lp = err_total = err_state = 0.0
    for b, (_tok, _ts, lp, total, _dur) in enumerate(res):
        want = np.asarray(ref["logps"][b], np.float64)
        if len(want):
            err_lp = max(err_lp, float(np.max(np.abs(lp - want) / (1 + np.abs(want)))))
        terms = max(2 * ref["evals"][b], 1)
        err_total = max(err_total, abs(total - ref["total"][b]) / ((1 + abs(ref["total"][b])) * terms))
    err_state = float(np.max(np.abs(state[0] - ref["state"][0])))
    print(f"rnnt tdt {case.name}: max logp err {err_lp:.3e}, total err per term {err_total:.3e}, "
          f"state err {err_state:.3e}")
    assert err_lp <= TOL and err_total <= TOL


def test_durations_of_one_walk_as_the_plain_kernel():
    """durations = [1] on case 4's shape: every evaluation moves one frame, asr_rnnt_greedy's walk at
    max_symbols = 1 on the same weights; the duration softmax over one column adds exactly 0."""
    case = CASE4._replace(durations=(1,), max_symbols=1)
    w, enc = tc.make_model(case)
    ln = tc.lengths_of(case)
    res, _state, cnt = tc.make_decoder(asr, case, w).decode(enc, ln)
    plain, _st, pcnt = rc.make_decoder(asr, case, {k: v for k, v in w.items() if k[2:] != "dur"}).decode(enc, ln)
    assert cnt.tolist() == pcnt.tolist() and int(cnt.sum()) > 0
    bits = True
    for r, q, frames in zip(res, plain, ln):     # one evaluation per frame: the totals sum `frames` terms
        assert r[0] == q[0] and r[1] == q[1] and r[4] == [1] * len(r[0])
        assert np.all(np.abs(r[2] - q[2]) <= TOL * (1 + np.abs(q[2])))
        assert abs(r[3] - q[3]) <= TOL * (1 + abs(q[3])) * max(int(frames), 1)
        bits &= np.array_equal(r[2], q[2]) and r[3] == q[3]
    print(f"rnnt tdt durations of one: bits equal to asr_rnnt_greedy's: {bits}")


def test_chunked_decode_equals_whole():
    """Case 4 at T = 12 cut 5 + 4 + 3, the state and the skip passed on: every output array bit for bit."""
    case = CASE4._replace(shape=(12,) + CASE4.shape[1:], lengths=(12, 0, 7, 12, 10))
    w, enc = tc.make_model(case)
    dec = tc.make_decoder(asr, case, w)
    tc.check_chunked(lambda e, n, st: dec.decode(e, n, state=st), enc, tc.lengths_of(case))


def test_batch_independent():
    """37 utterances of case 4's shape, then the first 5 alone: equal bytes."""
    case = CASE4._replace(shape=(9, 37) + CASE4.shape[2:], lengths=tuple([9, 0, 4, 9, 7] * 7 + [9, 3]))
    w, enc = tc.make_model(case)
    dec, ln = tc.make_decoder(asr, case, w), tc.lengths_of(case)
    r37, s37, n37 = dec.decode(enc, ln)
    r5, s5, n5 = dec.decode(np.ascontiguousarray(enc[:, :5]), ln[:5])
    assert n37[:5].tolist() == n5.tolist() and int(n5.sum()) > 0
    assert np.array_equal(s37[0][:, :, :5], s5[0]) and np.array_equal(s37[1][:5], s5[1])
    for x, y in zip(r37[:5], r5):
        assert x[0] == y[0] and x[1] == y[1] and np.array_equal(x[2], y[2]) and x[3] == y[3] and x[4] == y[4]


def test_nothing_is_written_beyond_the_counts():
    """Case 4 at max_out = 2 into arrays of 0x5A: the records below min(count, 2) are the reference's, the counts
    are the uncut ones and every other byte is as it was."""
    w, enc, ref = tc.reference(CASE4)
    assert max(ref["count"]) > 2
    dec = tc.make_decoder(asr, CASE4, w)
    dec.upload()
    T, B, mo = enc.shape[0], enc.shape[1], 2
    shapes = [((B, mo), np.int32)] * 3 + [((B, mo), np.float64)]
    outs = [asr.DeviceBytes(int(np.prod(sh)) * np.dtype(dt).itemsize) for sh, dt in shapes]
    d_cnt, d_tot, work = asr.DeviceBytes(4 * B), asr.DeviceBytes(8 * B), asr.DeviceBytes(dec.workspace_bytes(T, B))
    for o in outs:
        asr.check(asr.lib().asr_memset(o.ptr, 0x5A, o.nbytes, None), "asr_memset")
    d_enc, d_ln = asr._upload(enc, 0), asr._upload(tc.lengths_of(CASE4), 0)
    dec.decode_device(d_enc.ptr, T, B, mo, outs[0].ptr, outs[1].ptr, outs[3].ptr, d_cnt.ptr, d_tot.ptr, work.ptr,
                      d_ln.ptr, d_durations=outs[2].ptr)
    asr.check(asr.lib().asr_stream_sync(None), "asr_stream_sync")
    tok, ts, dur, lp = (asr._download(o, sh, dt, 0) for o, (sh, dt) in zip(outs, shapes))
    cnt = asr._download(d_cnt, (B,), np.int32, 0)
    assert cnt.tolist() == ref["count"]
    written = np.arange(mo)[None, :] < np.minimum(cnt, mo)[:, None]
    for a, want in ((tok, "tokens"), (ts, "timesteps"), (dur, "durations")):
        assert a[written].tolist() == [x for b in range(B) for x in ref[want][b][:mo]]
    for a in (tok, ts, dur, lp):
        assert bool((a.view(np.uint8).reshape(a.shape + (a.itemsize,))[~written] == 0x5A).all())
