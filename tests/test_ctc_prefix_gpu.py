"""GPU numerics of the CTC prefix scorer (asr_ctc_prefix_begin / _score /
_advance, asr.CTCPrefixScorer) and of joint CTC / attention decoding
(TransformerDecoder.beam_search with ctc) against ctc_prefix_reference.py
(float64).  Bounds: deltas and joint rows |err| <= 2e-5 * (1 + |ref|), the
project's fp32 bound, -inf exactly where the reference has it; the fp64 state
1e-9 * (1 + |ref|).  Each case prints its max error.  B = 3 utterances with
lengths (T, ceil(T / 2), 1); V = 5, 70, 300 around a wave's 64 and a workgroup's
256 tokens; T = 1, 2, 63, 64, 65, 130 around the 64-frame stage and its chunks
of eight.  The slots cycle through a random prefix, the empty prefix, one token,
a repeated token, three tokens (too long for T_b <= 2; every prefix of two is
too long in utterance 2), a finished slot and an empty slot whose state is NaN.
"""
import functools
import types

import numpy as np
import pytest
import torch  # noqa: F401  (one HIP runtime per process: conftest.py)

import attention_decode_reference as adref
import attention_decoder_reference as adr
import ctc_prefix_reference as cpr
from conftest import asr

pytestmark = pytest.mark.gpu
ATOL, ATOL64, SENT, B, NEG = adr.ATOL, 1e-9, -12345.0, 3, -np.inf
CASES = [(V, T, K, bl) for V in (5, 70, 300) for T in (1, 2, 63, 64, 65, 130) for K in (1, 4, 16) for bl in (0, V - 2)]
KINDS = ("random", "empty_prefix", "one", "repeat", "three", "finished", "empty_slot")
case_id = lambda c: "x".join(map(str, c))   # noqa: E731
lengths = lambda T: (T, (T + 1) // 2, 1)   # noqa: E731


def close(got, want, what, atol=ATOL):
    """-inf and NaN (an untouched empty slot) exactly where want has them, the rest inside atol * (1 + |want|)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(got == NEG, want == NEG) and np.array_equal(np.isnan(got), np.isnan(want)), what
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin]) / (1 + np.abs(want[fin]))
    print(f"{what}: max err / (1 + |ref|) {err.max() if err.size else 0.0:.3e}")
    assert np.all(np.isfinite(got[fin])) and np.all(err <= atol), what


@functools.lru_cache(maxsize=None)
def problem(case):
    """x [T][B][V] float32 with a few -inf entries; per slot the state after its prefix (rn, rb [T][N], psi, last;
    NaN past T_b and in empty slots), scores, flags, and the reference deltas [N][V] (SENT: a row not to touch)."""
    V, T, K, blank = case
    eos, N = V - 1, B * K
    rng = np.random.default_rng(1000 * V + 10 * T + K + blank)
    x = cpr.log_softmax_emissions(T, B, V, seed=V + T)
    x[rng.random(x.shape) < 0.02] = NEG
    toks = [c for c in range(V) if c not in (blank, eos)]
    rn, rb = np.full((T, N), np.nan), np.full((T, N), np.nan)
    psi, last = np.full(N, np.nan), np.full(N, -7, np.int32)
    scores, fin, want = -rng.uniform(0, 5, N), np.zeros(N, np.int32), np.full((N, V), SENT)
    for b, Tb in enumerate(lengths(T)):
        xb, sl = x[:Tb, b].astype(np.float64), slice(b * K, (b + 1) * K)
        kinds = [KINDS[(T + b * K + k) % len(KINDS)] for k in range(K)]
        a, r = rng.choice(toks), rng.choice(toks, 3)
        prefix = {"random": [r[0], r[1]], "empty_prefix": [], "one": [a], "repeat": [a, a], "three": list(r),
                  "finished": [a], "empty_slot": []}
        st = cpr.begin(xb, blank, K)
        for i in range(3):                           # eos pads the shorter prefixes: the state passes through
            st = cpr.advance(xb, st, np.arange(K), [(prefix[kd] + [eos] * 3)[i] for kd in kinds], blank, eos)
        rn[:Tb, sl], rb[:Tb, sl], psi[sl], last[sl] = st
        d = cpr.score(xb, st, blank, eos)
        for k, kd in enumerate(kinds):
            n = b * K + k
            fin[n] = kd == "finished"
            if kd == "empty_slot":
                scores[n], psi[n], last[n] = NEG, np.nan, -7
                rn[:, n] = rb[:, n] = np.nan
            if kd not in ("finished", "empty_slot"):
                want[n] = d[k]
    for a in (x, rn, rb, psi, last, scores, fin, want):
        a.setflags(write=False)
    return x, (rn, rb, psi, last), scores, fin, want


def fill(d, a):
    a = np.ascontiguousarray(a)
    asr.check(asr.lib().asr_memcpy_h2d(d.ptr, a.ctypes.data, a.nbytes, None), "asr_memcpy_h2d")


def put(a2d, pad=0, misalign=False, fill_with=np.nan):
    """a2d on the device at row stride cols + pad (fill_with in the padding), 4 bytes past a 16-byte boundary if
    asked."""
    h = np.full((a2d.shape[0], a2d.shape[1] + pad), fill_with, np.float32)
    h[:, :a2d.shape[1]] = a2d
    off = int(misalign)
    flat = np.concatenate([np.zeros(off, np.float32), h.reshape(-1), np.zeros(4 - off, np.float32)])
    base = asr.DeviceMatrix.from_numpy(flat.reshape(-1, 1))
    assert base.ptr % 16 == 0
    return types.SimpleNamespace(ptr=base.ptr + 4 * off, rows=h.shape[0], cols=h.shape[1], nbytes=h.nbytes, keep=base)


def run(x, lens, K, state, scores, fin, blank, att=None, w=0.0, bonus=0.0, moves=(), pad=0, misalign=False):
    """One score (out [N][V]; rows and padding start as SENT) and then one advance per (parent, token) of moves
    (the states [(rn, rb, psi, last)], each written into buffers full of SENT) on x [T][B][V] with NaN past each
    length."""
    T, nb, V = x.shape
    N = nb * K
    x = x.copy()
    for b, Tb in enumerate(lens):
        x[Tb:, b] = np.nan
    sc = asr.CTCPrefixScorer(put(x.reshape(T * nb, V), pad, misalign), T, nb, lens, K, blank, V - 1, V=V)
    for d, a in zip((sc.rn[0], sc.rb[0], sc.psi[0], sc.last[0]), state):
        fill(d, a)
    st = types.SimpleNamespace(cur=0, scores=[asr._upload(scores)], fin=[asr._upload(fin)])
    out = put(np.full((N, V), SENT, np.float32), pad, misalign, SENT)
    d_att = None if att is None else put(att, pad, misalign)
    sc.score(st, d_att, out, w, bonus)
    got = asr._download(out, (N, V + pad), np.float32)
    assert np.all(got[:, V:] == SENT)
    states = []
    for parent, token in moves:
        st.parent, st.token = asr._upload(np.asarray(parent, np.int32)), asr._upload(np.asarray(token, np.int32))
        for d, a in zip((sc.rn[1 - sc.cur], sc.rb[1 - sc.cur], sc.psi[1 - sc.cur], sc.last[1 - sc.cur]), state):
            fill(d, np.full(a.shape, SENT, a.dtype))
        sc.advance(st)
        c = sc.cur
        states.append((asr._download(sc.rn[c], (T, N), np.float64), asr._download(sc.rb[c], (T, N), np.float64),
                       asr._download(sc.psi[c], N, np.float64), asr._download(sc.last[c], N, np.int32)))
    return got[:, :V], states


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_deltas_and_joint_rows(case):
    V, T, K, blank = case
    x, state, scores, fin, want = problem(case)
    got, _ = run(x, lengths(T), K, state, scores, fin, blank, pad=3)
    keep = want[:, 0] == SENT
    assert np.all(got[keep] == SENT)                 # finished and empty slots: not touched
    close(got[~keep], want[~keep], f"deltas {case}")
    att = np.log(np.random.default_rng(V + T + K).dirichlet(np.ones(V), B * K)).astype(np.float32)
    got, _ = run(x, lengths(T), K, state, scores, fin, blank, att, 0.3, 0.25)
    assert np.all(got[keep] == SENT)
    close(got[~keep], 0.7 * att[~keep].astype(np.float64) + 0.3 * want[~keep] + 0.25, f"joint rows {case}")


def moves_of(case, steps=3):
    """steps x (parent [N], token [N]) as a prune could give them, and the reference states after each."""
    V, T, K, blank = case
    x, state, scores, fin, _ = problem(case)
    eos, N = V - 1, B * K
    rng = np.random.default_rng(7 * V + T + K)
    toks = np.array([c for c in range(V) if c not in (blank, eos)] + [eos])
    alive, done, moves, refs = scores > NEG, fin.astype(bool), [], []
    for _ in range(steps):
        parent, token = np.arange(N), np.full(N, eos)
        for n in range(N):
            pool = np.flatnonzero(alive[n // K * K:(n // K + 1) * K]) + n // K * K
            if len(pool):                            # no live slot: the empty slot itself with eos, as the prune says
                parent[n] = rng.choice(pool)
                token[n] = eos if done[parent[n]] else rng.choice(toks)
        new = [np.full_like(a, SENT) for a in state]                 # rows past T_b: not touched
        for b, Tb in enumerate(lengths(T)):
            sl = slice(b * K, (b + 1) * K)
            st = cpr.advance(x[:Tb, b].astype(np.float64), tuple(a[:Tb, sl] if a.ndim == 2 else a[sl] for a in state),
                             parent[sl] - b * K, token[sl], blank, eos)
            for a, v in zip(new, st):
                a[(slice(0, Tb), sl) if a.ndim == 2 else sl] = v
        state, alive, done = tuple(new), alive[parent], done[parent] | (token == eos)
        moves.append((parent, token))
        refs.append(state)
    return moves, refs


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_three_chained_advances(case):
    V, T, K, blank = case
    x, state, scores, fin, _ = problem(case)
    moves, refs = moves_of(case)
    _, got = run(x, lengths(T), K, state, scores, fin, blank, moves=moves)
    for i, (g, w) in enumerate(zip(got, refs)):
        assert np.array_equal(g[3], w[3])
        for name, a, r in zip(("rn", "rb", "psi"), g, w):
            close(a, r, f"advance {case} step {i} {name}", ATOL64)


@pytest.mark.parametrize("case", [(70, 65, 4, 0), (300, 130, 4, 298)], ids=case_id)
def test_a_row_and_a_state_depend_only_on_their_own_inputs(case):
    """Utterance 1's K = 4 slots: among the others, alone, in another slot order, at K = 16 between empty slots, and
    with padded strides behind a misaligned base pointer."""
    V, T, K, blank = case
    x, state, scores, fin, _ = problem(case)
    att = np.log(np.random.default_rng(5).dirichlet(np.ones(V), B * K)).astype(np.float32)
    (parent, token), lens, sl = moves_of(case, 1)[0][0], lengths(T), slice(K, 2 * K)
    base, (bst,) = run(x, lens, K, state, scores, fin, blank, att, 0.3, 0.1, [(parent, token)])
    base, bst = base[sl], [a[..., sl] for a in bst]
    one = [a[..., sl] for a in state]

    def same(got, st, where, what):
        assert np.array_equal(got[where], base), what
        assert all(np.array_equal(a[..., where][:lens[1]], r[:lens[1]]) if a.ndim == 2 else
                   np.array_equal(a[where], r) for a, r in zip(st, bst)), what

    move = [(parent[sl] - K, token[sl])]
    got, (st,) = run(x[:, 1:2], lens[1:2], K, one, scores[sl], fin[sl], blank, att[sl], 0.3, 0.1, move)
    same(got, st, slice(0, K), "alone")
    got, (st,) = run(x[:, 1:2], lens[1:2], K, one, scores[sl], fin[sl], blank, att[sl], 0.3, 0.1, move, 5, True)
    same(got, st, slice(0, K), "padded strides, misaligned")
    perm = np.array([2, 0, 3, 1])
    got, (st,) = run(x[:, 1:2], lens[1:2], K, [a[..., perm] for a in one], scores[sl][perm], fin[sl][perm], blank,
                     att[sl][perm], 0.3, 0.1, [(np.argsort(perm)[move[0][0][perm]], move[0][1][perm])])
    same(got, st, np.argsort(perm), "another slot order")
    at = np.array([3, 7, 8, 15])
    wide = [np.full(a.shape[:-1] + (16,), np.nan if a.dtype == np.float64 else -7, a.dtype) for a in one]
    for a, o in zip(wide, one):
        a[..., at] = o
    sc16, fin16, att16 = np.full(16, NEG), np.zeros(16, np.int32), np.zeros((16, V), np.float32)
    sc16[at], fin16[at], att16[at] = scores[sl], fin[sl], att[sl]
    par16, tok16 = np.arange(16), np.full(16, V - 1)
    par16[at], tok16[at] = at[move[0][0]], move[0][1]
    got, (st,) = run(x[:, 1:2], lens[1:2], 16, wide, sc16, fin16, blank, att16, 0.3, 0.1, [(par16, tok16)])
    same(got, st, at, "K = 16")


@functools.lru_cache(maxsize=None)
def search_reference(case):
    K, w, bonus, max_len, seed = case
    c = adref.SEARCH
    memory, modules = adref.search_model(seed, 0.0)
    emis = cpr.log_softmax_emissions(c["T"], c["B"], c["V"], 700 + seed)
    want, worst = cpr.joint_beam_search_ref(modules, memory, emis, c["enc_lengths"], K, max_len, 10, 10, w, 0, bonus)
    return memory, modules, emis, want, worst


@pytest.mark.parametrize("case", cpr.SEARCH_CASES, ids=case_id)
def test_joint_search_equals_the_float64_joint_search(case):
    K, w, bonus, max_len, seed = case
    c = adref.SEARCH
    memory, modules, emis, want, worst = search_reference(case)
    print(f"case {case}: margin {worst:.2f}")
    assert worst >= 2, worst                         # the reference keeps its margin at every prune
    dec = asr.TransformerDecoder.from_torch(*modules)
    T, nb, E = memory.shape
    d_mem, d_emis = (asr.DeviceMatrix.from_numpy(a.reshape(T * nb, -1)) for a in (memory, emis))
    args = dict(max_len=max_len, sos=10, eos=10, ctc=d_emis, ctc_weight=w, blank=0, length_bonus=bonus)
    got = dec.beam_search(d_mem, T, nb, c["enc_lengths"], beam=K, **args)
    assert [[y for y, _ in u] for u in got] == [[y for y, _ in u] for u in want]
    for (y, s), (_, r) in ((g, h) for u, v in zip(got, want) for g, h in zip(u, v)):
        assert abs(s - r) <= adr.score_bound(len(y) + (len(y) < max_len), r), (y, s, r)
    if K == 1:
        assert dec.greedy(d_mem, T, nb, c["enc_lengths"], **args) == got
    plain = dec.beam_search(d_mem, T, nb, c["enc_lengths"], beam=K, max_len=max_len, sos=10, eos=10)
    assert plain == dec.beam_search(d_mem, T, nb, c["enc_lengths"], beam=K, **{**args, "ctc_weight": 0.0})
    if w == 0.7:                                     # a weight at which CTC changes what the search returns
        assert [[y for y, _ in u] for u in got] != [[y for y, _ in u] for u in plain]


@pytest.mark.parametrize("kw,match", [(dict(ctc_weight=1.5), "ctc_weight"), (dict(ctc_weight=-0.1), "ctc_weight"),
                                      (dict(blank=10), "blank"), (dict(blank=11), "blank"), (dict(blank=-1), "blank"),
                                      (dict(length_bonus=np.inf), "length_bonus"), (dict(rows=1), "ctc is"),
                                      (dict(cols=1), "ctc is")])
def test_beam_search_refuses(kw, match):
    c = adref.SEARCH
    memory, modules = adref.search_model(0, 0.0)
    dec = asr.TransformerDecoder.from_torch(*modules)
    T, nb, V = c["T"], c["B"], c["V"]
    kw = dict(kw)
    ctc = asr.DeviceMatrix(T * nb + kw.pop("rows", 0), V + kw.pop("cols", 0))
    with pytest.raises(ValueError, match=match):
        dec.beam_search(asr.DeviceMatrix.from_numpy(memory.reshape(T * nb, -1)), T, nb, beam=2, max_len=3, sos=10,
                        eos=10, **{"ctc": ctc, "ctc_weight": 0.5, **kw})
