"""CPU checks of edit distance, WER counts and n-best MBR rescoring (asr_edit_* /
asr_nbest_mbr*): the host twins against the literal Python reference of
tests/edit_reference.py, every refusal of the four entry points (decided before
any HIP call: the fake device pointers are never dereferenced), the Python
helpers and CTCDecoder.mbr_rescore on a stubbed decoder.  No GPU here."""
import math
import re
import subprocess

import numpy as np
import pytest

from conftest import asr
import edit_reference as R

NAMES = ["asr_edit_distance", "asr_edit_distance_host", "asr_nbest_mbr", "asr_nbest_mbr_host"]
FAKE = 0x10000   # a non-NULL, 16-byte aligned "device pointer"
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def test_symbols_in_mirror_and_library():
    for n in NAMES:
        assert n in asr.EXPORTS, n
        assert hasattr(asr.lib(), n), n
    out = subprocess.run(["nm", "-D", "--defined-only", str(asr.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (asr_[a-z0-9_]+)$", out, flags=re.M))
    assert set(NAMES) <= exported
    assert asr.ASR_EDIT_MAX_LEN == 1024 and asr.ASR_MBR_MAX_HYPS == 256


def chars(s):
    return [ord(c) for c in s]


WORKED = [("kitten", "sitting", 3, (4, 2, 0, 1)), ("ab", "ba", 2, (0, 2, 0, 0)), ("abcd", "bcde", 2, (3, 0, 1, 1))]


def test_worked_examples():
    refs, hyps = [chars(a) for a, _, _, _ in WORKED], [chars(b) for _, b, _, _ in WORKED]
    dist, ops = asr.edit_distance(refs, hyps, detail=True, host=True)
    for n, (a, b, d, c) in enumerate(WORKED):
        assert R.align(chars(a), chars(b)) == (d, c)
        assert dist[n] == d and tuple(ops[n]) == c, (a, b)
    assert (asr.edit_distance(refs, hyps, host=True) == dist).all()


def test_host_equals_reference_on_random_pairs():
    """Alphabets of 2 to 4 tokens: ties at nearly every cell."""
    rng = np.random.default_rng(18)
    refs, hyps = [], []
    for n in range(3000):
        v = 2 + n % 3
        refs.append(rng.integers(0, v, rng.integers(0, 41)).tolist())
        hyps.append(rng.integers(0, v, rng.integers(0, 41)).tolist())
    dist, ops = asr.edit_distance(refs, hyps, detail=True, host=True)
    for n in range(3000):
        d, c = R.align(refs[n], hyps[n])
        assert dist[n] == d and tuple(ops[n]) == c, n
        assert dist[n] == R.distance_two_rows(refs[n], hyps[n])
        h, s, de, i = (int(x) for x in ops[n])
        assert s + de + i == dist[n] and h + s + de == len(refs[n]) and h + s + i == len(hyps[n])
        assert min(h, s, de, i) >= 0


def test_extreme_token_values():
    vals = [I32_MIN, -1, I32_MAX, 0]
    rng = np.random.default_rng(3)
    refs = [[vals[i] for i in rng.integers(0, 4, 12)] for _ in range(50)]
    hyps = [[vals[i] for i in rng.integers(0, 4, 11)] for _ in range(50)]
    refs.append([I32_MIN, -1, I32_MAX])
    hyps.append([I32_MAX, -1, I32_MIN])
    dist, ops = asr.edit_distance(refs, hyps, detail=True, host=True)
    for n in range(len(refs)):
        assert (dist[n], tuple(ops[n])) == R.align(refs[n], hyps[n])
    assert dist[-1] == 2 and tuple(ops[-1]) == (1, 2, 0, 0)


def host_call(ref, ref_len, hyp, hyp_len, max_ref, max_hyp, ref_idx=None, hyp_idx=None, P=None):
    ref, hyp = np.ascontiguousarray(ref, np.int32), np.ascontiguousarray(hyp, np.int32)
    arr = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)
    ref_len, hyp_len, ref_idx, hyp_idx = arr(ref_len), arr(hyp_len), arr(ref_idx), arr(hyp_idx)
    if P is None:
        P = len(ref_idx) if ref_idx is not None else len(hyp_idx) if hyp_idx is not None else len(ref)
    dist, ops = np.full(P, -99, np.int32), np.full((P, 4), -99, np.int32)
    p = lambda a: None if a is None else a.ctypes.data
    asr.check(asr.lib().asr_edit_distance_host(p(ref), ref.shape[1], p(ref_len), ref.shape[0], max_ref, p(hyp),
                                               hyp.shape[1], p(hyp_len), hyp.shape[0], max_hyp, p(ref_idx), p(hyp_idx),
                                               P, p(dist), p(ops)), "asr_edit_distance_host")
    return dist, ops


def test_lengths_are_clamped_and_null_lengths_mean_the_maximum():
    rng = np.random.default_rng(5)
    ref, hyp = rng.integers(0, 3, (6, 12)), rng.integers(0, 3, (6, 15))
    rl, hl = [0, -3, 5, 9, 10, 1000], [7, I32_MIN, 11, 3, I32_MAX, -1]
    dist, ops = host_call(ref, rl, hyp, hl, 9, 11)
    for n in range(6):
        a = ref[n, :min(max(rl[n], 0), 9)].tolist()
        b = hyp[n, :min(max(hl[n], 0), 11)].tolist()
        assert (dist[n], tuple(ops[n])) == R.align(a, b)
    dist, ops = host_call(ref, None, hyp, None, 9, 11)
    for n in range(6):
        assert (dist[n], tuple(ops[n])) == R.align(ref[n, :9].tolist(), hyp[n, :11].tolist())


def test_index_arrays_duplicates_permutation_and_bad_indices():
    rng = np.random.default_rng(6)
    ref, hyp = rng.integers(0, 3, (5, 8)), rng.integers(0, 3, (7, 8))
    rl, hl = rng.integers(0, 9, 5), rng.integers(0, 9, 7)
    ri = [0, 0, 4, 2, 2, 2, 3, 1, 4]
    hi = [6, 6, 0, 5, 1, 5, 2, 3, 4]
    dist, ops = host_call(ref, rl, hyp, hl, 8, 8, ri, hi)
    for p in range(len(ri)):
        want = R.align(ref[ri[p], :rl[ri[p]]].tolist(), hyp[hi[p], :hl[hi[p]]].tolist())
        assert (dist[p], tuple(ops[p])) == want
    # only one index array: the other side is row p
    perm = rng.permutation(5)
    dist, _ = host_call(ref, rl, hyp, hl, 8, 8, ref_idx=perm)
    for p in range(5):
        assert dist[p] == R.align(ref[perm[p], :rl[perm[p]]].tolist(), hyp[p, :hl[p]].tolist())[0]
    # an index outside its table: -1 everywhere, the others unharmed
    dist, ops = host_call(ref, rl, hyp, hl, 8, 8, [0, 5, -1, 1, I32_MAX, 2], [0, 0, 0, 7, 1, I32_MIN])
    assert dist.tolist()[1:] == [-1] * 5 and (ops[1:] == -1).all()
    assert dist[0] == R.align(ref[0, :rl[0]].tolist(), hyp[0, :hl[0]].tolist())[0]
    # the mirror's pairs argument
    d2 = asr.edit_distance([r.tolist() for r in ref], [h.tolist() for h in hyp], pairs=[(4, 6), (0, 0), (9, 0)],
                           host=True)
    assert d2[0] == R.distance_two_rows(ref[4].tolist(), hyp[6].tolist()) and d2[2] == -1


def test_longest_and_empty_sequences():
    rng = np.random.default_rng(7)
    a, b = rng.integers(0, 4, 1024).tolist(), rng.integers(0, 4, 1024).tolist()
    dist, ops = asr.edit_distance([a, a, [], [], a], [b, [], b, [], a], detail=True, host=True)
    assert dist[0] == R.distance_two_rows(a, b)
    assert int(ops[0, 1:].sum()) == dist[0] and int(ops[0, :3].sum()) == 1024 and ops[0, 0] + ops[0, 1] + ops[0, 3] == 1024
    assert tuple(ops[1]) == (0, 0, 1024, 0) and tuple(ops[2]) == (0, 0, 0, 1024)
    assert dist[3] == 0 and tuple(ops[3]) == (0, 0, 0, 0)
    assert dist[4] == 0 and tuple(ops[4]) == (1024, 0, 0, 0)


# ------------------------------------------------------------------ refusals
def dev_ed(ref=FAKE, ldr=8, ref_len=FAKE, n_ref=4, max_ref=8, hyp=FAKE, ldh=8, hyp_len=FAKE, n_hyp=4, max_hyp=8,
           ref_idx=FAKE, hyp_idx=FAKE, P=4, dist=FAKE, ops=FAKE):
    return asr.lib().asr_edit_distance(ref, ldr, ref_len, n_ref, max_ref, hyp, ldh, hyp_len, n_hyp, max_hyp, ref_idx,
                                       hyp_idx, P, dist, ops, None)


def host_ed(ref=FAKE, ldr=8, ref_len=FAKE, n_ref=4, max_ref=8, hyp=FAKE, ldh=8, hyp_len=FAKE, n_hyp=4, max_hyp=8,
            ref_idx=FAKE, hyp_idx=FAKE, P=4, dist=FAKE, ops=FAKE):
    return asr.lib().asr_edit_distance_host(ref, ldr, ref_len, n_ref, max_ref, hyp, ldh, hyp_len, n_hyp, max_hyp,
                                            ref_idx, hyp_idx, P, dist, ops)


@pytest.mark.parametrize("call", [dev_ed, host_ed])
def test_edit_distance_refusals(call):
    E, U = asr.ASR_ERR_ARG, asr.ASR_ERR_UNSUPPORTED
    assert call(ref=None) == E
    assert call(hyp=None) == E
    for bad in (0, -1):
        assert call(P=bad) == E
        assert call(n_ref=bad) == E
        assert call(n_hyp=bad) == E
    assert call(ldr=7) == E
    assert call(ldh=7) == E
    assert call(dist=None, ops=None) == E
    assert call(ref_idx=None, P=5) == E
    assert call(hyp_idx=None, P=5) == E
    assert call(ref_idx=None, hyp_idx=None, n_ref=9, P=5) == E
    assert call(max_ref=1025, ldr=1025) == U
    assert call(max_hyp=1025, ldh=1025) == U
    assert call(max_ref=-1) == U
    assert call(max_hyp=-1) == U
    # the order of the checks: ARG before UNSUPPORTED
    assert call(max_ref=1025, ldr=1025, dist=None, ops=None) == E
    assert call(max_hyp=1025, ldh=8) == E


def dev_mbr(tokens=FAKE, ldt=8, lengths=FAKE, N=6, max_len=8, gs=FAKE, G=2, max_hyps=3, weight=FAKE, dist=FAKE, ldm=3,
            risk=FAKE, best=FAKE):
    return asr.lib().asr_nbest_mbr(tokens, ldt, lengths, N, max_len, gs, G, max_hyps, weight, dist, ldm, risk, best,
                                   None)


def host_mbr(tokens=FAKE, ldt=8, lengths=FAKE, N=6, max_len=8, gs=FAKE, G=2, max_hyps=3, weight=FAKE, dist=FAKE,
             ldm=3, risk=FAKE, best=FAKE):
    return asr.lib().asr_nbest_mbr_host(tokens, ldt, lengths, N, max_len, gs, G, max_hyps, weight, dist, ldm, risk,
                                        best)


@pytest.mark.parametrize("call", [dev_mbr, host_mbr])
def test_nbest_mbr_refusals(call):
    E, U = asr.ASR_ERR_ARG, asr.ASR_ERR_UNSUPPORTED
    assert call(tokens=None) == E
    assert call(gs=None) == E
    assert call(dist=None) == E
    for bad in (0, -1):
        assert call(N=bad) == E
        assert call(G=bad) == E
        assert call(max_hyps=bad) == E
    assert call(ldt=7) == E
    assert call(ldm=2) == E
    assert call(risk=None, best=None) == E
    assert call(max_len=1025, ldt=1025) == U
    assert call(max_len=-1) == U
    assert call(max_hyps=257, ldm=257) == U
    assert call(max_hyps=257, ldm=256) == E
    assert call(max_len=1025, ldt=1025, risk=None, best=None) == E


# ------------------------------------------------------------------------ MBR
def host_mbr_arrays(tok, ln, gs, max_hyps, w, ldm=None, max_len=None, want_risk=True, want_best=True):
    tok = np.ascontiguousarray(tok, np.int32)
    N = tok.shape[0]
    max_len = tok.shape[1] if max_len is None else max_len
    ldm = max_hyps if ldm is None else ldm
    gs = np.ascontiguousarray(gs, np.int32)
    G = len(gs) - 1
    ln = None if ln is None else np.ascontiguousarray(ln, np.int32)
    w = None if w is None else np.ascontiguousarray(w, np.float64)
    dist = np.full((N, ldm), -99, np.int32)
    risk, best = np.full(N, -99.0, np.float64), np.full(G, -99, np.int32)
    p = lambda a: None if a is None else a.ctypes.data
    asr.check(asr.lib().asr_nbest_mbr_host(p(tok), tok.shape[1], p(ln), N, max_len, p(gs), G, max_hyps, p(w), p(dist),
                                           ldm, p(risk) if want_risk else None, p(best) if want_best else None),
              "asr_nbest_mbr_host")
    return dist, risk, best


def random_groups(rng, sizes, vocab=4, max_len=10):
    """Groups of distinct hypotheses (equal ones have equal risks: the tie cases are tested apart)."""
    out = []
    for n in sizes:
        seen = set()
        while len(seen) < n:
            seen.add(tuple(rng.integers(0, vocab, rng.integers(0, max_len + 1)).tolist()))
        out.append([list(t) for t in sorted(seen, key=lambda t: rng.random())])
    return out


def close(got, want):
    return abs(got - want) <= 1e-12 * max(1.0, abs(want))


def test_mbr_host_equals_reference():
    rng = np.random.default_rng(11)
    sizes = [1, 2, 5, 64, 65, 130, 0, 256, 3]
    groups = random_groups(rng, sizes)
    weights = [rng.uniform(-30.0, 0.0, n).tolist() for n in sizes]
    risks, best, dists = asr.nbest_mbr(groups, weights, host=True)
    uni_r, uni_b, uni_d = asr.nbest_mbr(groups, None, host=True)
    for g, n in enumerate(sizes):
        want_r, want_b, want_d = R.mbr(groups[g], weights[g])
        assert (dists[g] == want_d).all() and (uni_d[g] == want_d).all()
        assert (dists[g] == dists[g].T).all() and (np.diag(dists[g]) == 0).all()
        assert all(close(risks[g][k], want_r[k]) for k in range(n)), g
        if n > 1:
            two = sorted(want_r)[:2]
            assert two[1] - two[0] >= 1e-9 * max(1.0, two[0]), g     # the seed leaves no near-tie
        assert best[g] == want_b
        z = R.tree_sum([1.0] * n)
        want_u = [R.tree_sum([float(x) for x in want_d[k]]) / z for k in range(n)]
        assert uni_r[g].tolist() == want_u                           # bit-equal: every e_j is 1
        assert uni_b[g] == (min(range(n), key=lambda k: (want_u[k], k)) if n else -1)
    assert best[6] == -1 and len(risks[6]) == 0
    assert risks[0].tolist() == [0.0] and best[0] == 0               # n = 1


def test_mbr_weight_edge_cases():
    rng = np.random.default_rng(12)
    hyps = random_groups(rng, [6])[0]
    nan, inf = math.nan, math.inf
    cases = [[-inf] * 6, [nan] * 6, [nan, -inf, nan, -inf, -inf, nan], [0.0, nan, -1.0, -inf, -2.0, nan],
             [0.0, inf, -1.0, 5.0, inf, nan], [inf] * 6, [-1e308, 1e308, 0.0, 1e308, -inf, nan], [700.0, -700.0] * 3]
    uniform = asr.nbest_mbr([hyps], None, host=True)
    for w in cases:
        risks, best, dists = asr.nbest_mbr([hyps], [w], host=True)
        want_r, want_b, want_d = R.mbr(hyps, w)
        assert (dists[0] == want_d).all()
        assert all(close(risks[0][k], want_r[k]) for k in range(6)), w
        assert best[0] == want_b
        assert all(math.isfinite(r) for r in risks[0])
    for w in cases[:3]:                                              # no usable weight: uniform, bit for bit
        assert asr.nbest_mbr([hyps], [w], host=True)[0][0].tobytes() == uniform[0][0].tobytes()
    # one +inf: the risk is the distance to that hypothesis
    risks, best, dists = asr.nbest_mbr([hyps], [[0.0, -1.0, inf, 3.0, nan, -inf]], host=True)
    assert risks[0].tolist() == dists[0][:, 2].astype(np.float64).tolist() and best[0] == 2


def test_mbr_ties_take_the_lowest_row():
    hyps = [[1, 2, 3], [1, 2], [1, 2, 3], [1, 2]]
    risks, best, _ = asr.nbest_mbr([hyps], None, host=True)
    assert risks[0].tolist() == [0.5, 0.5, 0.5, 0.5] and best[0] == 0
    risks, best, _ = asr.nbest_mbr([[[5], [1, 2], [1, 2], [7, 7, 7, 7]]], None, host=True)
    assert best[0] == 1 and risks[0][1] == risks[0][2]


def test_mbr_empty_invalid_and_oversize_groups():
    rng = np.random.default_rng(13)
    N, L, max_hyps, ldm = 20, 6, 4, 7
    tok = rng.integers(0, 3, (N, L))
    ln = rng.integers(0, L + 1, N)
    w = rng.uniform(-5, 0, N)
    #      valid   empty   oversize  invalid: beyond N, negative start, reversed
    gs_list = [[0, 3], [3, 3], [3, 12], [15, 21], [-1, 2], [9, 5]]
    for lo, hi in gs_list:
        dist, risk, best = host_mbr_arrays(tok, ln, [lo, hi], max_hyps, w, ldm=ldm)
        valid = 0 <= lo <= hi <= N
        n = min(hi - lo, max_hyps) if valid else 0
        touched = np.zeros((N, ldm), bool)
        touched[lo:lo + n, :n] = True
        assert (dist[~touched] == -99).all() and (dist[touched] >= 0).all()
        rows = np.zeros(N, bool)
        rows[lo:lo + n] = True
        assert (risk[~rows] == -99.0).all()
        if n == 0:
            assert best[0] == -1
            continue
        hyps = [tok[r, :ln[r]].tolist() for r in range(lo, lo + n)]
        want_r, want_b, want_d = R.mbr(hyps, w[lo:lo + n].tolist())
        assert (dist[lo:lo + n, :n] == want_d).all() and best[0] == want_b
        assert all(close(risk[lo + k], want_r[k]) for k in range(n))
    # several groups in one call, each output alone, NULL lengths
    gs = [0, 3, 3, 7, 20]
    dist, risk, best = host_mbr_arrays(tok, None, gs, max_hyps, w)
    d2, r2, _ = host_mbr_arrays(tok, None, gs, max_hyps, w, want_best=False)
    d3, _, b3 = host_mbr_arrays(tok, None, gs, max_hyps, w, want_risk=False)
    assert d2.tobytes() == dist.tobytes() == d3.tobytes()
    assert r2.tobytes() == risk.tobytes() and b3.tobytes() == best.tobytes()
    assert best[1] == -1 and (risk[11:] == -99.0).all()              # rows 11.. are beyond the first max_hyps
    for g in (0, 2, 3):
        n = min(gs[g + 1] - gs[g], max_hyps)
        want_r, want_b, _ = R.mbr([tok[r].tolist() for r in range(gs[g], gs[g] + n)], w[gs[g]:gs[g] + n].tolist())
        assert best[g] == want_b and all(close(risk[gs[g] + k], want_r[k]) for k in range(n))


# ------------------------------------------------------------- Python helpers
def test_wer_and_word_tokens():
    labels = ["", "a", "b", "c", " ", "|"]
    refs = [[1, 2, 4, 3], [3, 4, 3, 4, 1], []]
    hyps = [[1, 2, 4, 4, 2], [3, 4, 1], [2]]
    toks = asr.word_tokens(refs + hyps, labels)
    assert toks == [[0, 1], [1, 1, 2], [], [0, 3], [1, 2], [3]]       # ab c / c c a / - / ab b / c a / b
    out = asr.wer(toks[:3], toks[3:], host=True)
    assert out == {"errors": 3, "ref_tokens": 5, "hits": 3, "sub": 1, "del": 1, "ins": 1, "wer": 0.6}
    cer = asr.wer(refs, hyps, host=True)
    assert cer["errors"] == cer["sub"] + cer["del"] + cer["ins"] and cer["ref_tokens"] == 9
    assert asr.word_tokens([[1, 5, 2]], labels, space="|") == [[0, 1]]
    assert asr.word_tokens([[4, 4, 0]], labels) == [[]]
    assert asr.wer([[]], [[1]], host=True)["wer"] == math.inf
    assert asr.wer([[]], [[]], host=True)["wer"] == 0.0
    assert asr.wer([], [], host=True)["wer"] == 0.0
    with pytest.raises(ValueError):
        asr.edit_distance([[1]], [[1], [2]], host=True)


# ------------------------------------------------------------- mbr_rescore
def stub_decoder(monkeypatch, beams, exact):
    dec = object.__new__(asr.CTCDecoder)
    dec.h = None
    dec.T, dec.B, dec.V, dec.blank = 5, len(beams), 4, 0
    dec._last = (FAKE, dec.B * 4, 4, None, True)
    dec.beams = lambda max_hyps: [u[:max_hyps] for u in beams]
    monkeypatch.setattr(asr, "ctc_score", lambda emis, targets, **kw: np.array([exact[tuple(t)] for t in targets]))
    device = asr.nbest_mbr
    monkeypatch.setattr(asr, "nbest_mbr", lambda toks, w, host=False, stream=0: device(toks, w, host=True))
    return dec


class StubLM:
    def __init__(self, values):
        self.values = values

    def score(self, token_lists, bos=True, eos=True, detail=False, host=False, stream=0):
        lp = np.array([self.values[tuple(t)] for t in token_lists], np.float64)
        return lp, np.array([[len(t) + (1 if eos else 0), 0] for t in token_lists], np.int32)


def test_mbr_rescore_formula_and_stable_order(monkeypatch):
    beams = [[([1, 2], -1.0), ([1], -1.5), ([2, 2, 3], -2.0), ([3], -2.5), ([1, 2, 3], -3.0)],
             [([2], -0.5)],
             [],
             [([1, 2], -1.0), ([2, 1], -1.0), ([1, 2], -1.0)]]
    exact = {(1, 2): -0.9, (1,): -1.4, (2, 2, 3): -1.9, (3,): -1.4, (2,): -0.4, (1, 2, 3): -2.5, (2, 1): -0.9}
    dec = stub_decoder(monkeypatch, beams, exact)
    plain = dec.rescore(10)
    for scale in (1.0, 0.25, 0.0):
        out = dec.mbr_rescore(10, scale=scale)
        assert [len(u) for u in out] == [5, 1, 0, 3]
        for b, u in enumerate(out):
            ranked = [lab for lab, _, _ in plain[b]]
            want, _, _ = R.mbr(ranked, [scale * exact[tuple(lab)] for lab in ranked])
            for lab, risk, total in u:
                assert total == exact[tuple(lab)]
                assert close(risk, want[ranked.index(lab)])
            assert [r[1] for r in u] == sorted(r[1] for r in u)
    # utterance 3, uniform weights: (1, 2) twice and (2, 1): the two equal hypotheses have
    # the smaller, equal risk and keep rescore()'s order; the stub cannot tell them apart,
    # so check that on the risks
    tie = dec.mbr_rescore(10, scale=0.0)[3]
    assert [tuple(r[0]) for r in tie] == [(1, 2), (1, 2), (2, 1)] and tie[0][1] == tie[1][1] < tie[2][1]
    # equal risks keep the order of the ranking they came from: (1,) before (3,) in rescore()'s order
    eq = dec.mbr_rescore(10, scale=0.0)[0]
    order = [tuple(r[0]) for r in eq]
    r1, r3 = eq[order.index((1,))][1], eq[order.index((3,))][1]
    assert r1 == r3 and order.index((1,)) < order.index((3,))
    assert [len(u) for u in dec.mbr_rescore(2)] == [2, 1, 0, 2]
    # distances over tokens(labels): every hypothesis maps to the same token list -> every risk 0
    flat = dec.mbr_rescore(10, tokens=lambda lab: [7])
    assert all(r[1] == 0.0 for u in flat for r in u)
    assert [[r[0] for r in u] for u in flat] == [[r[0] for r in u] for u in plain]
    # with a language model: the weights are scale * lm_rescore()'s totals
    lmv = {k: -0.5 * len(k) for k in exact}
    lm = StubLM(lmv)
    alpha, beta = 0.7, 0.25
    ranked = dec.lm_rescore(10, lm, alpha, beta, mapper=lambda lab: list(lab))
    out = dec.mbr_rescore(10, scale=0.5, lm=lm, alpha=alpha, beta=beta, mapper=lambda lab: list(lab))
    for b, u in enumerate(out):
        labs = [r[0] for r in ranked[b]]
        want, _, _ = R.mbr(labs, [0.5 * r[1] for r in ranked[b]])
        for lab, risk, total in u:
            # (1, 2) occurs twice in utterance 3 with one total; index() finds either
            assert total == ranked[b][labs.index(lab)][1] and close(risk, want[labs.index(lab)])


def test_mbr_rescore_needs_a_whole_utterance_decode():
    dec = object.__new__(asr.CTCDecoder)
    dec.h = None
    dec._last = None
    with pytest.raises(asr.AsrError) as e:
        dec.mbr_rescore(5)
    assert e.value.status == asr.ASR_ERR_STATE
