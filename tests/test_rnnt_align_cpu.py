"""CPU checks of the transducer lattice scorer (asr_rnnt_align*): the reference
tests/rnnt_align_reference.py against its own enumeration of every alignment,
the fp64 host twin asr_rnnt_align_host against the reference, the beam search
as the one-per-frame lattice when nothing is pruned, the lattice as an upper
bound of every search score, the greedy walk as one alignment of the standard
lattice, infeasible targets, clamping and every refusal.  No GPU is needed or
used.  test_reference_matches_its_enumeration checks the Python reference
alone, so it is the one test here that does not need the library's new symbols;
every other test of the file calls them."""
import itertools
import math

import numpy as np
import pytest
import torch

import rnnt_align_cases as ac
import rnnt_beam_cases as bc
import rnnt_cases as rc
from conftest import asr
from rnnt_align_reference import AlignReference, brute_force, lattice

REL = 1e-9   # the project's oracle bound: both sides are fp64 and differ in summation order only


def close(a, b):
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= REL * (1.0 + abs(b))


@pytest.mark.parametrize("topology", [0, 1])
def test_reference_matches_its_enumeration(topology):
    case = ac.SMALL_CASES[0]
    w, enc = rc.make_model(case.model)
    ref = AlignReference(w, case.model.blank, case.model.act, 1)
    gen = torch.Generator().manual_seed(7)
    checked = 0
    for ln, U in itertools.product(range(1, 6), range(0, 4)):
        tgt = [1 + int(x) for x in torch.randint(0, 16, (U,), generator=gen)]
        lpb, lpy = ref.grid(torch.as_tensor(enc[:ln, 0], dtype=torch.float64), tgt)
        total, best = brute_force(lpb, lpy, topology)
        if topology == 1 and U > ln:
            assert total == -math.inf
            continue
        got = lattice(lpb, lpy, topology)
        assert close(got["score"], total) and close(got["vscore"], best), (ln, U, got["score"], total)
        # the frames describe an alignment of that probability
        fr = got["frames"]
        assert all(a <= b if topology == 0 else a < b for a, b in zip(fr, fr[1:])), fr
        lp, u = 0.0, 0
        for t in range(ln):
            emitted = 0
            while u < U and fr[u] == t and not (topology and emitted):
                lp += lpy[t][u]
                u, emitted = u + 1, 1
            if not (topology and emitted):
                lp += lpb[t][u]
        assert u == U and close(lp, best), (ln, U, fr)
        checked += 1
    assert checked >= 14


@pytest.mark.parametrize("topology", ac.TOPOLOGIES)
@pytest.mark.parametrize("case", ac.SMALL_CASES + [ac.NBEST_CASE] + ac.WIDE_J_CASES, ids=lambda c: c.name)
def test_twin_matches_reference(case, topology):
    w, enc, targets, utt, ref = ac.reference(case, topology)
    ac.check_conditions(case, ref)
    # the mix of target lengths: 0, 1, = len, > len, > T
    if case in ac.SMALL_CASES:
        T, lens = case.model.shape[0], case.model.lengths
        kinds = {(U == 0, U == 1, U == lens[b] > 0, U > lens[b] > 0, U > T) for b, U in case.spec}
        assert all(any(k[i] for k in kinds) for i in range(5)), kinds
    dec = rc.make_decoder(asr, case.model, w)
    score, vscore, frames = dec.align_host(enc, targets, rc.lengths_of(case.model), utt, topology)
    for n, r in enumerate(ref):
        assert close(score[n], r["score"]) and close(vscore[n], r["vscore"]), (n, score[n], r["score"])
        assert frames[n].tolist() == r["frames"], n
    # score_host is the same call with one output: equal bits
    assert dec.score_host(enc, targets, rc.lengths_of(case.model), utt, topology).tobytes() == score.tobytes()
    dec.close()


def test_the_search_is_the_lattice_when_nothing_is_pruned():
    """V = 2 (one label), T <= 8, K = 16: asr_rnnt_beam keeps min(K, |A| V)
    candidates and |A| <= t + 1 at frame t, so 2 (t + 1) <= 16 for t <= 7 and no
    candidate is ever dropped: every hypothesis's search score is the
    one-per-frame lattice's score of its tokens."""
    model = ac.NOPRUNE_MODEL
    assert model.shape == (8, 3, 8, 16, 16, 16, 2, 1) and model.lengths == (8, 5, 0)
    w, enc = rc.make_model(model)
    dec = rc.make_decoder(asr, model, w)
    ln = rc.lengths_of(model)
    nbest = dec.beam_search_host(enc, ln, beam=16)
    for b, hyps in enumerate(nbest):
        assert sorted(h[0] for h in hyps) == [[1] * k for k in range(model.lengths[b] + 1)], b
    targets = [h[0] for u in nbest for h in u]
    utt = [b for b, u in enumerate(nbest) for _ in u]
    exact = dec.score_host(enc, targets, ln, utt, "one_per_frame")
    for k, (tgt, s) in enumerate(zip(targets, (h[2] for u in nbest for h in u))):
        assert close(s, exact[k]), (k, tgt, s, exact[k])
    dec.close()


@pytest.mark.parametrize("case", bc.SMALL_CASES, ids=lambda c: c.name)
def test_the_lattice_is_an_upper_bound_of_the_search(case):
    w, enc, ref = bc.reference(case)
    dec = bc.make_decoder(asr, case, w)
    targets = [tok for u in ref["hyps"] for tok, _ts, _s in u]
    utt = [b for b, u in enumerate(ref["hyps"]) for _ in u]
    exact = dec.score_host(enc, targets, rc.lengths_of(case.model), utt, "one_per_frame")
    k = 0
    for u in ref["hyps"]:
        for _tok, _ts, s in u:
            assert exact[k] >= s - 1e-9 * (1.0 + abs(s)), (case.name, k, exact[k], s)
            k += 1
    # TransducerDecoder.rescore on the host scores: per utterance a permutation of the n-best, by exact score
    # descending, equal scores in search order, each hypothesis with its own search and exact score
    res = dec.rescore(ref["hyps"], enc, rc.lengths_of(case.model), host=True)
    assert len(res) == len(ref["hyps"])
    k = 0
    for u, r in zip(ref["hyps"], res):
        mine = {tuple(tok): (s, float(exact[k + j])) for j, (tok, _ts, s) in enumerate(u)}
        assert len(mine) == len(u) == len(r)
        assert sorted(tuple(t) for t, _s, _e in r) == sorted(mine)
        for tok, s, e in r:
            assert (s, e) == mine[tuple(tok)]
        pos = {tuple(tok): j for j, (tok, _ts, _s) in enumerate(u)}
        keys = [(-e, pos[tuple(t)]) for t, _s, e in r]
        assert keys == sorted(keys)
        k += len(u)
    dec.close()


@pytest.mark.parametrize("model", ac.GREEDY_MODELS, ids=lambda m: m.name)
def test_greedy_is_one_alignment_of_the_standard_lattice(model):
    w, enc, ref = rc.reference(model)
    assert max(n for f in ref["frames"] for n in f) < model.max_symbols     # the walk never reaches the cap
    assert sum(ref["count"]) > 0 and any(n >= 2 for f in ref["frames"] for n in f)
    dec = rc.make_decoder(asr, model, w)
    score, vscore, _frames = dec.align_host(enc, ref["tokens"], rc.lengths_of(model), None, "standard")
    for b, total in enumerate(ref["total"]):
        assert vscore[b] >= total - 1e-9 * (1.0 + abs(total)), (b, vscore[b], total)
        assert score[b] >= vscore[b], b
    dec.close()


def test_infeasible_targets_zero_frames_and_clamping():
    case = ac.SMALL_CASES[0]                   # S2: T = 9, lengths [9, 0, 4, 9, 7], blank 0, V = 17
    w, enc = rc.make_model(case.model)
    dec = rc.make_decoder(asr, case.model, w)
    ln = rc.lengths_of(case.model)
    good = [3, 5, 7]
    targets = [good, [3, 0, 7], [3, 17, 7], [3, -1, 7], good, good, [], good, good]
    utt = [0, 0, 0, 0, -1, 5, 1, 1, 2]
    for topology in ac.TOPOLOGIES:
        score, vscore, frames = dec.align_host(enc, targets, ln, utt, topology)
        for n in (1, 2, 3, 4, 5, 7):           # the blank, V, a negative label, utt outside [0, B), no frames with U > 0
            assert score[n] == -math.inf and vscore[n] == -math.inf and frames[n].tolist() == [-1, -1, -1], (topology, n)
        assert score[6] == 0.0 and vscore[6] == 0.0          # no frames, U = 0
        assert math.isfinite(score[0]) and math.isfinite(score[8]) and score[0] >= vscore[0]
        assert all(0 <= f < 9 for f in frames[0]) and all(0 <= f < 4 for f in frames[8])
    # U > len under one_per_frame only
    s0 = dec.score_host(enc, [[1, 2, 3, 4, 5]], ln, [2], "standard")
    s1 = dec.score_host(enc, [[1, 2, 3, 4, 5]], ln, [2], "one_per_frame")
    assert math.isfinite(s0[0]) and s1[0] == -math.inf
    # lengths are clamped to [0, T]; utt NULL is utterance n
    a = dec.score_host(enc, [good] * 5, [12, -3, 4, 9, 7])
    b = dec.score_host(enc, [good] * 5, [9, 0, 4, 9, 7], [0, 1, 2, 3, 4])
    assert a.tobytes() == b.tobytes() and a[1] == -math.inf
    # target lengths are clamped to [0, max_target_len]: the raw call
    tg = np.array([[3, 5, 7, 9]], np.int32)
    out = np.zeros((3, 1), np.float64)
    fr = np.full((3, 4), -5, np.int32)
    for i, tl in enumerate((3, 7, -2)):
        rc_ = asr.lib().asr_rnnt_align_host(dec.h, enc.ctypes.data, None, 9, 5, tg.ctypes.data, 4,
                                           np.array([tl], np.int32).ctypes.data, None, 1, 3, 0,
                                           out[i].ctypes.data, None, fr[i].ctypes.data)
        assert rc_ == asr.ASR_OK
    assert out[0, 0] == out[1, 0] == score_of(dec, enc, ln, good)
    assert out[2, 0] == score_of(dec, enc, ln, [])
    assert fr[0].tolist() == fr[1].tolist() and fr[0, 3] == -5 and all(x >= 0 for x in fr[0, :3])
    assert fr[2].tolist() == [-1, -1, -1, -5]              # beyond max_target_len: not touched
    dec.close()


def score_of(dec, enc, ln, target):
    return float(dec.score_host(enc, [target], ln, [0])[0])


def test_every_refusal_returns_its_status_without_a_hip_call():
    case = ac.SMALL_CASES[0]
    w, enc = rc.make_model(case.model)
    dec = rc.make_decoder(asr, case.model, w)             # never uploaded
    L = asr.lib()
    T, B = enc.shape[0], enc.shape[1]
    tg = np.array([[1, 2], [3, 4]], np.int32)
    tl = np.array([2, 1], np.int32)
    ut = np.array([0, 1], np.int32)
    sc, vs, fr = np.zeros(2), np.zeros(2), np.zeros((2, 2), np.int32)
    work = np.zeros(4)
    base = dict(h=dec.h, enc=enc.ctypes.data, T=T, B=B, tg=tg.ctypes.data, ldt=2, tl=tl.ctypes.data, ut=ut.ctypes.data,
                N=2, mtl=2, topo=0, sc=sc.ctypes.data, vs=vs.ctypes.data, fr=fr.ctypes.data)

    def both(**kw):
        a = {**base, **kw}
        host = L.asr_rnnt_align_host(a["h"], a["enc"], None, a["T"], a["B"], a["tg"], a["ldt"], a["tl"], a["ut"], a["N"],
                                     a["mtl"], a["topo"], a["sc"], a["vs"], a["fr"])
        dev = L.asr_rnnt_align(a["h"], a["enc"], None, a["T"], a["B"], a["tg"], a["ldt"], a["tl"], a["ut"], a["N"],
                               a["mtl"], a["topo"], a["sc"], a["vs"], a["fr"], work.ctypes.data, None)
        # the device entry refuses the same way; what the host accepts ends at "not uploaded", before any HIP call
        assert dev == (asr.ASR_ERR_STATE if host == asr.ASR_OK else host), (kw, host, dev)
        return host

    assert both() == asr.ASR_OK
    for kw in (dict(h=None), dict(enc=None), dict(tg=None), dict(tl=None), dict(T=0), dict(B=0), dict(N=0), dict(mtl=-1),
               dict(ldt=1), dict(sc=None, vs=None, fr=None), dict(topo=2), dict(topo=-1), dict(ut=None, B=1)):
        assert both(**kw) == asr.ASR_ERR_ARG, kw
    for kw in (dict(mtl=256, ldt=256), dict(T=1 << 30, B=4), dict(T=1 << 30, B=1, N=1), dict(N=1 << 30),
               dict(T=1 << 20, B=1, N=1 << 20), dict(N=1 << 24, mtl=0)):
        assert both(**kw) == asr.ASR_ERR_UNSUPPORTED, kw
    assert L.asr_rnnt_align(dec.h, enc.ctypes.data, None, T, B, tg.ctypes.data, 2, tl.ctypes.data, ut.ctypes.data, 2, 2,
                            0, sc.ctypes.data, None, None, None, None) == asr.ASR_ERR_ARG      # no workspace
    assert dec.align_workspace_bytes(T, B, 2, 256) == 0 and dec.align_workspace_bytes(0, B, 2, 2) == 0
    d = case.model.shape
    Hp, J = d[4], d[5]
    assert dec.align_workspace_bytes(T, B, 2, 2) == \
        4 * (T * B * J + 3 * 2 * (4 * Hp + Hp + J) + 2 * Hp + 2 * ((2 * T * 3 + 3) // 4 * 4) + 4) + 64 * 2 * (T + 3)
    assert not dec.info()["uploaded"]
    dec.close()
