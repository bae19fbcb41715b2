"""GPU checks of asr_edit_distance and asr_nbest_mbr (csrc/edit.hip): the device
against the host twins on the same arrays (integers equal; risks within 1e-12 *
max(1, risk): all terms are non-negative, so at most 256 products and adds plus
one exp each leave well under 1e-13 relative; bit-equal with uniform weights),
the edges of the lane layout and of the token chunks, the independence promise,
untouched memory, one ragged call of 64 groups and CTCDecoder.mbr_rescore after
a real decode."""
import math

import numpy as np
import pytest

from conftest import asr, oracle
import edit_reference as R

pytestmark = pytest.mark.gpu

SENT_I = -77
SENT_F = -12345.678
REF_LENS = [1, 63, 64, 65, 128, 1024]        # the chunk edges of the reference-token reads
KS = [1, 2, 4, 8, 16]


@pytest.fixture(scope="module", autouse=True)
def device():
    asr.set_device(0)


def table(rows, ld=None, fill=1):
    """Token lists as ([n][ld] int32, lengths); the padding holds a token the rows
    use too, so reading it as a token would change a result."""
    ld = max([len(r) for r in rows] + [1]) if ld is None else ld
    tab = np.full((len(rows), ld), fill, np.int32)
    for n, r in enumerate(rows):
        tab[n, :len(r)] = r
    return tab, np.array([len(r) for r in rows], np.int32)


def ptr(a):
    return None if a is None else a.ctypes.data


def host_ed(ref, rl, hyp, hl, max_ref, max_hyp, ri, hi, P):
    dist, ops = np.full(P, SENT_I, np.int32), np.full((P, 4), SENT_I, np.int32)
    asr.check(asr.lib().asr_edit_distance_host(ptr(ref), ref.shape[1], ptr(rl), ref.shape[0], max_ref, ptr(hyp),
                                               hyp.shape[1], ptr(hl), hyp.shape[0], max_hyp, ptr(ri), ptr(hi), P,
                                               ptr(dist), ptr(ops)), "asr_edit_distance_host")
    return dist, ops


def device_ed(ref, rl, hyp, hl, max_ref, max_hyp, ri, hi, P, want=("dist", "ops"), pad=3):
    """One asr_edit_distance; the outputs are pre-filled with a sentinel and have
    `pad` extra rows, which must come back untouched."""
    up = lambda a: None if a is None else asr._upload(a)
    d_ref, d_rl, d_hyp, d_hl, d_ri, d_hi = (up(a) for a in (ref, rl, hyp, hl, ri, hi))
    dp = lambda d: None if d is None else d.ptr
    bufs = {"dist": np.full(P + pad, SENT_I, np.int32), "ops": np.full((P + pad, 4), SENT_I, np.int32)}
    dev = {k: asr._upload(v) for k, v in bufs.items() if k in want}
    asr.check(asr.lib().asr_edit_distance(d_ref.ptr, ref.shape[1], dp(d_rl), ref.shape[0], max_ref, d_hyp.ptr,
                                          hyp.shape[1], dp(d_hl), hyp.shape[0], max_hyp, dp(d_ri), dp(d_hi), P,
                                          dp(dev.get("dist")), dp(dev.get("ops")), None), "asr_edit_distance")
    asr.synchronize()
    out = {}
    for k in bufs:
        if k not in dev:
            out[k] = None
            continue
        got = asr._download(dev[k], bufs[k].shape, np.int32)
        assert (got[P:] == SENT_I).all(), k
        out[k] = got[:P]
    return out["dist"], out["ops"]


def cross(n_ref, n_hyp):
    ri, hi = np.meshgrid(np.arange(n_ref, dtype=np.int32), np.arange(n_hyp, dtype=np.int32), indexing="ij")
    return np.ascontiguousarray(ri.reshape(-1)), np.ascontiguousarray(hi.reshape(-1))


def assert_device_equals_host(ref, rl, hyp, hl, max_ref, max_hyp, ri, hi, P):
    h_dist, h_ops = host_ed(ref, rl, hyp, hl, max_ref, max_hyp, ri, hi, P)
    d_dist, d_ops = device_ed(ref, rl, hyp, hl, max_ref, max_hyp, ri, hi, P)
    assert (d_dist == h_dist).all(), np.nonzero(d_dist != h_dist)[0][:8]
    assert (d_ops == h_ops).all(), np.nonzero((d_ops != h_ops).any(axis=1))[0][:8]
    ok = h_dist >= 0
    assert (h_ops[ok, 1:].sum(axis=1) == h_dist[ok]).all()
    return h_dist, h_ops


@pytest.mark.parametrize("K", KS)
def test_every_k_at_its_column_and_chunk_edges(K):
    """A call with max_hyp_len = 64 K runs K columns per lane: hypothesis lengths
    0, 1, 64 K - 1, 64 K (and 32 K + 1, one past the K / 2 layout) against every
    reference length; a call with max_hyp_len = 64 K + 1 runs the next layout."""
    rng = np.random.default_rng(100 + K)
    refs = [rng.integers(0, 3, L).tolist() for L in REF_LENS] + [[]]
    ref, rl = table(refs, ld=1027)
    lens = [0, 1, 64 * K - 1, 64 * K] + ([32 * K + 1] if K > 1 else [])
    hyp, hl = table([rng.integers(0, 3, L).tolist() for L in lens], ld=64 * K + 5)
    ri, hi = cross(len(refs), len(lens))
    h_dist, _ = assert_device_equals_host(ref, rl, hyp, hl, 1024, 64 * K, ri, hi, len(ri))
    small = [p for p in range(len(ri)) if rl[ri[p]] <= 65 and hl[hi[p]] <= 65]
    for p in small:      # and the host twin against the literal reference where that is quick
        assert h_dist[p] == R.distance_two_rows(refs[ri[p]], hyp[hi[p], :hl[hi[p]]].tolist())
    if K < 16:
        lens = [64 * K + 1, 64 * K, 1]
        hyp, hl = table([rng.integers(0, 3, L).tolist() for L in lens])
        ri, hi = cross(len(refs), len(lens))
        assert_device_equals_host(ref, rl, hyp, hl, 1024, 64 * K + 1, ri, hi, len(ri))


def test_equal_disjoint_and_repeated_sequences():
    rng = np.random.default_rng(7)
    lens = [1, 63, 64, 65, 128, 1024]
    seqs = [rng.integers(0, 5, L).tolist() for L in lens]
    ref, rl = table(seqs + [[7] * L for L in lens], fill=7)
    hyp, hl = table(seqs + [[7] * L for L in lens] + [rng.integers(10, 15, L).tolist() for L in lens], fill=7)
    n = len(lens)
    # equal sequences: row p against row p
    dist, ops = assert_device_equals_host(ref, rl, hyp, hl, 1024, 1024, None, None, 2 * n)
    assert (dist == 0).all() and (ops[:, 0] == rl).all() and (ops[:, 1:] == 0).all()
    # one repeated token, every length against every length: |la - lb| and min(la, lb) hits
    ri, hi = cross(n, n)
    ri, hi = ri + n, hi + n
    dist, ops = assert_device_equals_host(ref, rl, hyp, hl, 1024, 1024, ri, hi, len(ri))
    la, lb = rl[ri], hl[hi]
    assert (dist == abs(la - lb)).all() and (ops[:, 0] == np.minimum(la, lb)).all() and (ops[:, 1] == 0).all()
    # no token in common: max(la, lb), no hit
    ri, hi = cross(n, n)
    hi = hi + 2 * n
    dist, ops = assert_device_equals_host(ref, rl, hyp, hl, 1024, 1024, ri, hi, len(ri))
    la, lb = rl[ri], hl[hi]
    assert (dist == np.maximum(la, lb)).all() and (ops[:, 0] == 0).all() and (ops[:, 1] == np.minimum(la, lb)).all()


def test_worked_examples_and_extreme_tokens_on_the_device():
    c = lambda s: [ord(x) for x in s]
    lo, hi_ = -(1 << 31), (1 << 31) - 1
    refs = [c("kitten"), c("ab"), c("abcd"), [lo, -1, hi_], []]
    hyps = [c("sitting"), c("ba"), c("bcde"), [hi_, -1, lo], []]
    dist, ops = asr.edit_distance(refs, hyps, detail=True)
    assert dist.tolist() == [3, 2, 2, 2, 0]
    assert ops.tolist() == [[4, 2, 0, 1], [0, 2, 0, 0], [3, 0, 1, 1], [1, 2, 0, 0], [0, 0, 0, 0]]
    assert asr.wer(refs, hyps) == asr.wer(refs, hyps, host=True)


def test_clamped_lengths_null_lengths_and_bad_indices():
    rng = np.random.default_rng(8)
    ref, hyp = rng.integers(0, 3, (9, 80)).astype(np.int32), rng.integers(0, 3, (7, 140)).astype(np.int32)
    rl = np.array([0, -3, 5, 70, 71, 1000, -(1 << 31), (1 << 31) - 1, 64], np.int32)
    hl = np.array([130, -1, 129, 3, (1 << 31) - 1, 0, 64], np.int32)
    ri, hi = cross(9, 7)
    assert_device_equals_host(ref, rl, hyp, hl, 70, 129, ri, hi, len(ri))
    assert_device_equals_host(ref, None, hyp, None, 70, 129, ri, hi, len(ri))
    assert_device_equals_host(ref, rl, hyp, None, 80, 64, None, None, 7)
    bad_r = np.array([0, 9, -1, 1, (1 << 31) - 1, 2, 8], np.int32)
    bad_h = np.array([0, 0, 0, 7, 1, -(1 << 31), 6], np.int32)
    dist, ops = assert_device_equals_host(ref, rl, hyp, hl, 70, 129, bad_r, bad_h, 7)
    assert dist[1:6].tolist() == [-1] * 5 and (ops[1:6] == -1).all() and dist[0] >= 0 and dist[6] >= 0


def test_independence():
    rng = np.random.default_rng(9)
    lens = [0, 1, 5, 33, 63, 64]
    refs = [rng.integers(0, 3, L).tolist() for L in lens for _ in range(3)]
    hyps = [rng.integers(0, 3, L).tolist() for L in lens for _ in range(3)]
    ref, rl = table(refs)
    hyp, hl = table(hyps)
    ri, hi = cross(len(refs), len(hyps))
    P = len(ri)
    base_d, base_o = device_ed(ref, rl, hyp, hl, 64, 64, ri, hi, P)
    # another order and another P
    perm = rng.permutation(P).astype(np.int32)
    d, o = device_ed(ref, rl, hyp, hl, 64, 64, ri[perm], hi[perm], P)
    assert d.tobytes() == base_d[perm].tobytes() and o.tobytes() == base_o[perm].tobytes()
    d, o = device_ed(ref, rl, hyp, hl, 64, 64, ri[:37].copy(), hi[:37].copy(), 37)
    assert d.tobytes() == base_d[:37].tobytes() and o.tobytes() == base_o[:37].tobytes()
    d, o = device_ed(ref, rl, hyp, hl, 64, 64, ri[P - 1:].copy(), hi[P - 1:].copy(), 1)
    assert d.tobytes() == base_d[P - 1:].tobytes() and o.tobytes() == base_o[P - 1:].tobytes()
    # other leading dimensions and maximum lengths: 2, 4 and 16 columns per lane
    for max_ref, max_hyp, ldr, ldh in [(64, 70, 64, 70), (200, 256, 333, 256), (1024, 1024, 1030, 1024)]:
        ref_w, _ = table(refs, ld=ldr)
        hyp_w, _ = table(hyps, ld=ldh)
        d, o = device_ed(ref_w, rl, hyp_w, hl, max_ref, max_hyp, ri, hi, P)
        assert d.tobytes() == base_d.tobytes() and o.tobytes() == base_o.tobytes(), (max_ref, max_hyp)
    # each output alone
    d, o = device_ed(ref, rl, hyp, hl, 64, 64, ri, hi, P, want=("dist",))
    assert o is None and d.tobytes() == base_d.tobytes()
    d, o = device_ed(ref, rl, hyp, hl, 64, 64, ri, hi, P, want=("ops",))
    assert d is None and o.tobytes() == base_o.tobytes()
    # and the mirror's own path
    d, o = asr.edit_distance(refs, hyps, pairs=np.stack([ri, hi], axis=1), detail=True)
    assert d.tobytes() == base_d.tobytes() and o.tobytes() == base_o.tobytes()


# ------------------------------------------------------------------------ MBR
def host_mbr(tok, ln, gs, max_hyps, w, ldm, max_len):
    N, G = tok.shape[0], len(gs) - 1
    dist = np.full((N, ldm), SENT_I, np.int32)
    risk, best = np.full(N, SENT_F, np.float64), np.full(G, SENT_I, np.int32)
    asr.check(asr.lib().asr_nbest_mbr_host(ptr(tok), tok.shape[1], ptr(ln), N, max_len, ptr(gs), G, max_hyps, ptr(w),
                                           ptr(dist), ldm, ptr(risk), ptr(best)), "asr_nbest_mbr_host")
    return dist, risk, best


def device_mbr(tok, ln, gs, max_hyps, w, ldm, max_len, want=("risk", "best"), pad=2):
    N, G = tok.shape[0], len(gs) - 1
    up = lambda a: None if a is None else asr._upload(a)
    dp = lambda d: None if d is None else d.ptr
    d_tok, d_ln, d_gs, d_w = up(tok), up(ln), up(gs), up(w)
    bufs = {"dist": np.full((N + pad, ldm), SENT_I, np.int32), "risk": np.full(N + pad, SENT_F, np.float64),
            "best": np.full(G + pad, SENT_I, np.int32)}
    dev = {k: asr._upload(v) for k, v in bufs.items() if k == "dist" or k in want}
    asr.check(asr.lib().asr_nbest_mbr(d_tok.ptr, tok.shape[1], dp(d_ln), N, max_len, d_gs.ptr, G, max_hyps, dp(d_w),
                                      dev["dist"].ptr, ldm, dp(dev.get("risk")), dp(dev.get("best")), None),
              "asr_nbest_mbr")
    asr.synchronize()
    out = {}
    for k, n in (("dist", N), ("risk", N), ("best", G)):
        if k not in dev:
            out[k] = None
            continue
        got = asr._download(dev[k], bufs[k].shape, bufs[k].dtype)
        assert (got[n:] == bufs[k][n:]).all(), k
        out[k] = got[:n]
    return out["dist"], out["risk"], out["best"]


def distinct_groups(rng, sizes, vocab, lo, hi):
    """Groups of distinct hypotheses (equal ones have equal risks; ties are tested apart)."""
    out = []
    for n in sizes:
        seen = set()
        while len(seen) < n:
            seen.add(tuple(rng.integers(0, vocab, rng.integers(lo, hi + 1)).tolist()))
        out.append([list(t) for t in sorted(seen, key=lambda t: rng.random())])
    return out


def pack_groups(groups, ld=None):
    tok, ln = table([h for g in groups for h in g], ld=ld)
    gs = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    return tok, ln, gs


def assert_mbr_device_equals_host(tok, ln, gs, max_hyps, w, ldm=None, max_len=None, uniform=False):
    ldm = max_hyps if ldm is None else ldm
    max_len = tok.shape[1] if max_len is None else max_len
    h_dist, h_risk, h_best = host_mbr(tok, ln, gs, max_hyps, w, ldm, max_len)
    if w is not None and not uniform:
        # no near-tie in the comparator, so that `best` is decided beyond the tolerance
        for g in range(len(gs) - 1):
            r = np.sort(h_risk[gs[g]:gs[g] + min(gs[g + 1] - gs[g], max_hyps)])
            if len(r) > 1:
                assert r[1] - r[0] >= 1e-9 * max(1.0, r[0]), (g, r[:2])
    d_dist, d_risk, d_best = device_mbr(tok, ln, gs, max_hyps, w, ldm, max_len)
    assert (d_dist == h_dist).all()                                   # sentinels included: same entries written
    written = h_risk != SENT_F
    assert ((d_risk != SENT_F) == written).all()
    if w is None or uniform:
        assert d_risk.tobytes() == h_risk.tobytes()
    else:
        assert (np.abs(d_risk - h_risk)[written] <= 1e-12 * np.maximum(1.0, h_risk[written])).all()
    assert (d_best == h_best).all()
    return h_dist, h_risk, h_best


@pytest.mark.parametrize("max_len,lo,hi", [(12, 0, 12), (100, 60, 100)])
def test_mbr_device_equals_host(max_len, lo, hi):
    rng = np.random.default_rng(20 + max_len)
    sizes = [1, 2, 5, 63, 64, 65, 130, 256, 0, 3] if max_len == 12 else [1, 7, 65, 0, 20]
    groups = distinct_groups(rng, sizes, 4, lo, hi)
    tok, ln, gs = pack_groups(groups, ld=max_len + 3)
    w = rng.uniform(-30.0, 0.0, tok.shape[0])
    h_dist, h_risk, h_best = assert_mbr_device_equals_host(tok, ln, gs, max(sizes), w, max_len=max_len)
    assert_mbr_device_equals_host(tok, ln, gs, max(sizes), None, max_len=max_len)
    empty = sizes.index(0)
    assert h_best[empty] == -1 and h_best[0] == 0 and h_risk[0] == 0.0
    # the host twin against the literal reference on the small groups
    for g, n in enumerate(sizes):
        if 0 < n <= 7:
            want_r, want_b, want_d = R.mbr(groups[g], w[gs[g]:gs[g + 1]].tolist())
            assert (h_dist[gs[g]:gs[g + 1], :n] == want_d).all() and h_best[g] == want_b
            assert all(abs(h_risk[gs[g] + k] - want_r[k]) <= 1e-12 * max(1.0, want_r[k]) for k in range(n))


def test_mbr_weight_edge_cases_and_ties():
    rng = np.random.default_rng(31)
    nan, inf = math.nan, math.inf
    # no usable weight: e_j = 1 for every j, so bit-equal, and the lowest row decides a tie
    flat = [[-inf] * 6, [nan] * 6, [nan, -inf, nan, -inf, -inf, nan]]
    groups = distinct_groups(rng, [6] * len(flat), 4, 6, 12)
    tok, ln, gs = pack_groups(groups)
    w = np.array([x for c in flat for x in c], np.float64)
    _, h_risk, _ = assert_mbr_device_equals_host(tok, ln, gs, 6, w, uniform=True)
    assert h_risk.tobytes() == host_mbr(tok, ln, gs, 6, None, 6, tok.shape[1])[1].tobytes()
    cases = [[0.0, nan, -1.0, -inf, -2.5, nan], [0.0, inf, -1.0, 5.0, -inf, nan],
             [-1e308, 1e308, 0.0, 1e307, -inf, nan], [700.0, -700.0, 1.0, 2.0, 3.0, 4.0]]
    groups = distinct_groups(rng, [6] * len(cases), 4, 6, 12)
    tok, ln, gs = pack_groups(groups)
    w = np.array([x for c in cases for x in c], np.float64)
    h_dist, h_risk, h_best = assert_mbr_device_equals_host(tok, ln, gs, 6, w)
    assert np.isfinite(h_risk).all()
    assert h_best.tolist()[1:] == [1, 1, 0]                           # the +inf / the overwhelming weight decide
    assert h_risk[6:12].tolist() == h_dist[6:12, 1].astype(np.float64).tolist()
    # duplicate hypotheses, uniform weights: the lowest row alone decides
    dup = [[[1, 2, 3], [1, 2], [1, 2, 3], [1, 2]], [[5], [1, 2], [1, 2], [7, 7, 7, 7]], [[4, 4]] * 70]
    tok, ln, gs = pack_groups(dup)
    _, h_risk, h_best = assert_mbr_device_equals_host(tok, ln, gs, 70, None)
    assert h_best.tolist() == [0, 1, 0]
    _, _, h_best = assert_mbr_device_equals_host(tok, ln, gs, 70, np.zeros(tok.shape[0]), uniform=True)
    assert h_best.tolist() == [0, 1, 0]


def test_mbr_untouched_memory_and_group_bounds():
    rng = np.random.default_rng(32)
    N, L, max_hyps, ldm = 40, 9, 5, 8
    tok = rng.integers(0, 3, (N, L + 2)).astype(np.int32)
    ln = rng.integers(0, L + 1, N).astype(np.int32)
    # valid, empty, oversize (5 of 12 rows), beyond N, negative start, reversed, valid again
    gs_list = [[0, 3], [3, 3], [3, 15], [36, 41], [-1, 2], [9, 5], [38, 40]]
    for lo, hi in gs_list:
        gs = np.array([lo, hi], np.int32)
        h_dist, h_risk, h_best = host_mbr(tok, ln, gs, max_hyps, None, ldm, L)
        d_dist, d_risk, d_best = device_mbr(tok, ln, gs, max_hyps, None, ldm, L)
        valid = 0 <= lo <= hi <= N
        n = min(hi - lo, max_hyps) if valid else 0
        touched = np.zeros((N, ldm), bool)
        touched[max(lo, 0):max(lo, 0) + n, :n] = True
        assert (d_dist[~touched] == SENT_I).all() and (d_dist[touched] >= 0).all()
        rows = touched.any(axis=1)
        assert (d_risk[~rows] == SENT_F).all() and (d_risk[rows] != SENT_F).all()
        assert (d_dist == h_dist).all() and (d_best == h_best).all() and (d_best[0] == -1) == (n == 0)
        assert d_risk.tobytes() == h_risk.tobytes()                   # uniform weights: bit-equal
    # several groups at once, each output alone
    w = rng.uniform(-3.0, 0.0, N)
    gs = np.array([0, 3, 3, 15, 40], np.int32)
    dist, risk, best = device_mbr(tok, ln, gs, max_hyps, w, ldm, L)
    d2, r2, b2 = device_mbr(tok, ln, gs, max_hyps, w, ldm, L, want=("risk",))
    d3, r3, b3 = device_mbr(tok, ln, gs, max_hyps, w, ldm, L, want=("best",))
    assert b2 is None and r3 is None
    assert d2.tobytes() == dist.tobytes() == d3.tobytes()
    assert r2.tobytes() == risk.tobytes() and b3.tobytes() == best.tobytes()
    assert best[1] == -1 and (risk[8:15] == SENT_F).all() and (risk[20:] == SENT_F).all()


def test_mbr_independence():
    rng = np.random.default_rng(33)
    groups = distinct_groups(rng, [9, 1, 30, 4], 4, 3, 40)
    tok, ln, gs = pack_groups(groups)
    w = rng.uniform(-10.0, 0.0, tok.shape[0])
    base_d, base_r, base_b = device_mbr(tok, ln, gs, 30, w, 30, tok.shape[1])
    # one group alone, as group 0 of its own call, with other leading dimensions and maxima (4 columns per lane)
    for g in range(4):
        t, l, s = pack_groups([groups[g]], ld=250)
        n = len(groups[g])
        d, r, b = device_mbr(t, l, s, 256, w[gs[g]:gs[g + 1]].copy(), 256, 200)
        assert d[:, :n].tobytes() == base_d[gs[g]:gs[g + 1], :n].tobytes()
        assert r.tobytes() == base_r[gs[g]:gs[g + 1]].tobytes() and b[0] == base_b[g]
    # the groups in another order
    order = [2, 0, 3, 1]
    t, l, s = pack_groups([groups[g] for g in order])
    wp = np.concatenate([w[gs[g]:gs[g + 1]] for g in order])
    d, r, b = device_mbr(t, l, s, 30, wp, 30, t.shape[1])
    assert b.tolist() == [base_b[g] for g in order]
    assert r.tobytes() == np.concatenate([base_r[gs[g]:gs[g + 1]] for g in order]).tobytes()
    # and the mirror's own path
    risks, best, dists = asr.nbest_mbr(groups, [w[gs[g]:gs[g + 1]] for g in range(4)])
    assert best.tolist() == base_b.tolist()
    for g in range(4):
        n = len(groups[g])
        assert risks[g].tobytes() == base_r[gs[g]:gs[g + 1]].tobytes()
        assert dists[g].tobytes() == np.ascontiguousarray(base_d[gs[g]:gs[g + 1], :n]).tobytes()


def test_mbr_64_ragged_groups():
    rng = np.random.default_rng(34)
    sizes = rng.integers(0, 257, 64).tolist()
    sizes[0], sizes[1], sizes[2], sizes[63] = 0, 256, 1, 255
    groups = distinct_groups(rng, sizes, 4, 6, 14)
    tok, ln, gs = pack_groups(groups)
    w = rng.uniform(-20.0, 0.0, tok.shape[0])
    _, _, h_best = assert_mbr_device_equals_host(tok, ln, gs, 256, w)
    assert h_best[0] == -1 and (h_best[1:] >= 0).all()


# ----------------------------------------------------------------- end to end
def test_mbr_rescore_after_a_real_decode():
    T, B, V, beam = 40, 4, 6, 8
    emis = oracle.synthetic_emissions(T, B, V, seed0=99)
    dec = asr.CTCDecoder(V, beam, 0)
    dec.decode(emis)
    plain = dec.rescore(beam)
    for scale in (1.0, 0.1):
        out = dec.mbr_rescore(beam, scale=scale)
        assert [len(u) for u in out] == [len(u) for u in plain]
        for b in range(B):
            ranked = [lab for lab, _, _ in plain[b]]
            exact = {tuple(lab): ex for lab, ex, _ in plain[b]}
            want, _, _ = R.mbr(ranked, [scale * exact[tuple(lab)] for lab in ranked])
            assert sorted(tuple(r[0]) for r in out[b]) == sorted(exact)
            for lab, risk, total in out[b]:
                assert total == exact[tuple(lab)]
                k = ranked.index(lab)
                assert abs(risk - want[k]) <= 1e-12 * max(1.0, want[k])
            keys = [(r[1], ranked.index(r[0])) for r in out[b]]
            assert keys == sorted(keys)                    # risk ascending, equal risks in rescore()'s order
    # scale = 1e6.  Once the best exact score leads by more than ln(4 T beam) / scale = 7.2e-6,
    # every other e_j is below 1 / (4 T beam); a distance is at most T, so the top hypothesis'
    # risk is below beam T / (4 T beam) = 0.25, while every other risk is at least
    # d(k, top) e_top / Z >= 1 / (1 + beam / (4 T beam)) > 0.99: rescore()'s first comes first.
    scale = 1e6
    for b in range(B):
        if len(plain[b]) > 1:
            assert scale * (plain[b][0][1] - plain[b][1][1]) > math.log(4 * T * beam)
    top = dec.mbr_rescore(beam, scale=scale)
    assert [u[0][0] for u in top] == [u[0][0] for u in plain]
    # distances over words instead of labels
    labels = ["", "a", "b", " ", "c", "d"]
    ids = {}

    def words_of(lab):      # one dictionary for the whole batch, as word_tokens keeps within a call
        return [ids.setdefault(x, len(ids)) for x in "".join(labels[c] for c in lab).split(" ") if x != ""]

    words = dec.mbr_rescore(beam, tokens=words_of)
    for b in range(B):
        ranked = [lab for lab, _, _ in plain[b]]
        assert asr.word_tokens(ranked, labels) == asr.word_tokens(ranked, labels, " ")
        want, _, _ = R.mbr([words_of(lab) for lab in ranked], [ex for _, ex, _ in plain[b]])
        for lab, risk, _ in words[b]:
            assert abs(risk - want[ranked.index(lab)]) <= 1e-12 * max(1.0, want[ranked.index(lab)])
    dec.close()
