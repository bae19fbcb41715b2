"""CPU checks of attention-decoder beam search (asr_decode_attention_fwd,
asr_embed_fwd, asr_attn_beam_step, asr_attn_beam_step_host and the step /
begin / beam_search layer of asr_amd.py): exported, every refusal ahead of any
HIP call and in the documented order (the fake device pointers are never
dereferenced on the host), the host twin of the prune against the numpy rule
with np.array_equal, the float64 references of attention_decode_reference.py
against each other (a decoder stepping on a cache through an ancestry table,
random forced reorders included, against a from-scratch recompute), the margin
of the search cases' seeds, and the Python shape checks.  No GPU here."""
import ctypes

import numpy as np
import pytest

import attention_decode_reference as ref
import attention_decoder_reference as adr
from conftest import asr

NAMES = ["asr_decode_attention_fwd", "asr_embed_fwd", "asr_attn_beam_step", "asr_attn_beam_step_host"]
FAKE, FAKE2 = 0x10000, 0x20000   # non-NULL, 16-byte aligned "device pointers"
INT_MAX = 2 ** 31 - 1
ARG, UNSUP = asr.ASR_ERR_ARG, asr.ASR_ERR_UNSUPPORTED


def test_exported():
    assert all(n in asr.EXPORTS for n in NAMES)
    assert all(hasattr(asr.lib(), n) for n in NAMES)


# ------------------------------------------------------------------ refusals
def datt(heads=4, head_dim=16, scale=0.0, N=6, Tk=8, S=6, ldc=6, ld=None, lds=None, null=None):
    p = {"q": FAKE, "k": FAKE, "v": FAKE, "out": FAKE, "cols": FAKE}
    if null in p:
        p[null] = None
    d = asr.XAttnDesc(heads, head_dim, scale)
    l4 = lds or (heads * head_dim if ld is None else ld,) * 4
    return asr.lib().asr_decode_attention_fwd(None if null == "desc" else ctypes.byref(d), p["q"], l4[0], p["k"],
                                              l4[1], p["v"], l4[2], p["cols"], ldc, FAKE, p["out"], l4[3], N, Tk, S,
                                              None)


def test_decode_attention_refusals_in_order():
    for null in ("desc", "q", "k", "v", "out", "cols"):
        assert datt(null=null) == ARG, null
    for kw in (dict(N=0), dict(N=-1), dict(Tk=0), dict(Tk=-8), dict(S=0), dict(S=-1), dict(heads=0, ld=64),
               dict(head_dim=0, ld=64), dict(head_dim=-16, ld=64)):
        assert datt(**kw) == ARG, kw
    for ldc in (1, 5, -1, -6, -2 ** 40):             # not in {0} or [N, inf)
        assert datt(ldc=ldc) == ARG, ldc
    for lds in ((63, 64, 64, 64), (64, 63, 64, 64), (64, 64, 0, 64), (64, 64, 64, -64)):
        assert datt(lds=lds) == ARG, lds
    for scale in (-1.0, float("inf"), float("nan")):
        assert datt(scale=scale) == ARG, scale
    # ARG comes before UNSUPPORTED
    assert datt(head_dim=18, ldc=3) == ARG
    assert datt(head_dim=256, scale=float("nan")) == ARG
    assert datt(Tk=1 << 20, S=1 << 12, ldc=2) == ARG
    for kw in (dict(head_dim=18), dict(head_dim=2, ldc=0), dict(head_dim=132), dict(heads=33, head_dim=128),
               dict(heads=65536, head_dim=4), dict(Tk=1 << 20, S=1 << 12), dict(Tk=INT_MAX, S=INT_MAX, ldc=0)):
        assert datt(**kw) == UNSUP, kw


def emb(R=6, E=32, V=11, P=8, lds=None, scale=2.0, null=None, pe=FAKE, pos=FAKE):
    p = {"emb": FAKE, "tok": FAKE, "out": FAKE}
    if null in p:
        p[null] = None
    l3 = lds or (E, E, E)
    return asr.lib().asr_embed_fwd(p["emb"], l3[0], pe, l3[1], p["tok"], pos, scale, p["out"], l3[2], R, E, V, P, None)


def test_embed_refusals_in_order():
    for null in ("emb", "tok", "out"):
        assert emb(null=null) == ARG, null
    assert emb(pos=None) == ARG                       # a table without positions
    for kw in (dict(R=0), dict(R=-6), dict(E=0), dict(V=0), dict(P=0), dict(P=-1), dict(lds=(31, 32, 32)),
               dict(lds=(32, 31, 32)), dict(lds=(32, 32, 8)), dict(scale=float("nan")), dict(scale=float("inf"))):
        assert emb(**kw) == ARG, kw
    assert emb(R=1 << 20, E=1 << 12, lds=(1 << 12, 1 << 12, 31)) == ARG          # before UNSUPPORTED
    assert emb(R=1 << 20, E=1 << 12) == UNSUP
    assert emb(R=1 << 20, E=1 << 12, pe=None, pos=None, P=0, lds=(1 << 12, 0, 1 << 12)) == UNSUP   # no table: P, ldp unused


BEAM_PTRS = ["logp", "scores", "finished", "tokens_in", "anc_in", "scores_out", "finished_out", "parent", "token",
             "tokens_out", "anc_out", "all_finished"]


def beam(host, B=3, K=4, V=11, max_len=8, step=2, eos=10, ld=None, null=None, same=None):
    p = {n: FAKE2 if n in ("tokens_out", "anc_out") else FAKE for n in BEAM_PTRS}
    if null in p:
        p[null] = None
    if same:
        p[same + "_out"] = p[same + "_in"]
    d = asr.AttnBeamDesc(B, K, V, max_len, step, eos)
    args = [None if null == "desc" else ctypes.byref(d), p["logp"], V if ld is None else ld] + [p[n] for n in
                                                                                                 BEAM_PTRS[1:]]
    if host:
        return asr.lib().asr_attn_beam_step_host(*args)
    return asr.lib().asr_attn_beam_step(*args, None)


@pytest.mark.parametrize("host", [False, True])
def test_beam_step_refusals_in_order(host):
    for null in ["desc"] + BEAM_PTRS:
        assert beam(host, null=null) == ARG, null
    for kw in (dict(B=0), dict(K=0), dict(K=17), dict(K=-1), dict(V=0, ld=11), dict(max_len=0), dict(step=-1),
               dict(step=8), dict(eos=-1), dict(eos=11), dict(ld=10), dict(same="tokens"), dict(same="anc")):
        assert beam(host, **kw) == ARG, kw
    assert beam(host, B=1 << 28, K=16, ld=10) == ARG                              # before UNSUPPORTED
    assert beam(host, B=1 << 28, K=16) == UNSUP
    assert beam(host, B=1 << 20, max_len=1 << 12) == UNSUP


# --------------------------------------------- the host twin against the rule
@pytest.mark.parametrize("kind", ref.BEAM_KINDS)
@pytest.mark.parametrize("V,K", ref.BEAM_SHAPES)
def test_beam_step_host_equals_the_rule(kind, V, K):
    B, L = ref.BEAM_B, ref.BEAM_MAX_LEN
    logp, scores, fin, tin, ain, step = ref.beam_case(kind, V, K)
    eos = V - 1
    want = ref.beam_step_ref(logp, scores, fin, tin, ain, B, K, V, L, step, eos)
    got = asr.attn_beam_step_host(asr.attn_beam_desc(B, K, V, L, step, eos), logp, scores, fin, tin, ain)
    for name, g, w in zip(("scores", "finished", "parent", "token", "tokens_out", "anc_out", "live"), got, want):
        assert np.array_equal(g, w), (name, g, w)
    if kind in ("ties_tokens", "ties_parents"):       # the case does plant ties among the kept
        so = got[0].reshape(B, K)
        assert K == 1 or np.any(so[:, :-1] == so[:, 1:])
    if kind == "few":
        assert np.isinf(got[0][2 * K:]).all() and got[6] <= (K if V > 1 else 0)


def test_beam_step_host_wide_row_stride_and_shape_errors():
    B, K, V, L = ref.BEAM_B, 4, 5, ref.BEAM_MAX_LEN
    logp, scores, fin, tin, ain, step = ref.beam_case("mixed", V, K)
    d = asr.attn_beam_desc(B, K, V, L, step, V - 1)
    wide = np.full((B * K, V + 3), 9.0, np.float32)   # columns past V would win if they were read
    wide[:, :V] = logp
    a, b = asr.attn_beam_step_host(d, logp, scores, fin, tin, ain), asr.attn_beam_step_host(d, wide, scores, fin,
                                                                                            tin, ain)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for bad in (dict(logp=logp[:-1]), dict(logp=logp[:, :-1]), dict(scores=scores[:-1]), dict(fin=fin[1:]),
                dict(tin=tin[:-1]), dict(ain=ain[:, :-1])):
        kw = dict(logp=logp, scores=scores, fin=fin, tin=tin, ain=ain)
        kw.update(bad)
        with pytest.raises(ValueError, match="attn_beam_step_host"):
            asr.attn_beam_step_host(d, kw["logp"], kw["scores"], kw["fin"], kw["tin"], kw["ain"])


# ------------------------------------------------ reference against reference
@pytest.mark.parametrize("norm_first", [True, False])
def test_cached_ancestry_reference_equals_recompute(norm_first):
    """The float64 decoder stepping on a K/V cache through the ancestry table,
    under random forced reorders, against decoder_ref on every slot's
    reconstructed prefix, recomputed from scratch."""
    c, K, steps, sos = ref.SEARCH, 3, 7, 10
    memory, modules = ref.search_model(7, 0.0, norm_first)
    memory = memory[:12]                              # T = 12 keeps the recompute small
    enc = (12, 5, 9)
    B, N = c["B"], c["B"] * K
    rng = np.random.default_rng(5)
    cached = ref.CachedDecoderRef(*modules, memory, enc, K, steps)
    prefixes, tokens = [[] for _ in range(N)], np.full(N, sos)
    for s in range(steps):
        got = cached.step(tokens)
        want = ref.prefix_logp_ref(modules, prefixes, np.arange(N) // K, memory, enc, sos)
        assert np.all(np.abs(got - want) <= 1e-12 * (1 + np.abs(want))), (s, np.abs(got - want).max())
        parents = (np.arange(N) // K) * K + rng.integers(0, K, N)
        tokens = rng.integers(0, c["V"] - 1, N)
        cached.reorder(parents)
        prefixes = [prefixes[p] + [int(t)] for p, t in zip(parents, tokens)]


def test_decode_attention_ref_is_softmax_attention():
    heads, D, Tk = 2, 8, 9
    q, k, v, table, col = ref.draw_decode(heads, D, Tk)
    ln = ref.dattn_lengths(Tk)
    got = ref.decode_attention_ref(q, k, v, heads, table, ln)
    for n in range(q.shape[0]):
        kk = np.stack([k[j, table[j, n]] for j in range(ln[n])]) if ln[n] else np.zeros((0, heads * D))
        vv = np.stack([v[j, table[j, n]] for j in range(ln[n])]) if ln[n] else np.zeros((0, heads * D))
        for h in range(heads):
            sl = slice(h * D, (h + 1) * D)
            w = np.exp(kk[:, sl].astype(np.float64) @ q[n, sl].astype(np.float64) / np.sqrt(D))
            want = (w / w.sum()) @ vv[:, sl] if ln[n] else np.zeros(D)
            assert np.allclose(got[n, sl], want, rtol=0, atol=1e-13)
    one = ref.decode_attention_ref(q, k, v, heads, col, ln)
    assert np.array_equal(one, ref.decode_attention_ref(q, k, v, heads, np.tile(col, (Tk, 1)), ln))


@pytest.mark.parametrize("case", ref.SEARCH_CASES)
def test_search_seeds_keep_their_margin(case):
    K, bias, max_len, seed = case
    memory, modules = ref.search_model(seed, bias)
    res, worst = ref.beam_search_ref(modules, memory, ref.SEARCH["enc_lengths"], K, max_len, 10, 10)
    assert worst >= 2, worst
    lens = {len(y) for u in res for y, _ in u}
    if bias > 0:
        assert len(lens) > 2 and min(lens) < max_len          # hypotheses end at different steps
    if bias < 0:
        assert lens == {max_len}                              # none ends before max_len


# ----------------------------------------------------- Python shape checks
class Buf:
    """A stand-in for a device matrix: the shape checks run before any device call."""

    def __init__(self, rows, cols):
        self.ptr, self.rows, self.cols = FAKE, rows, cols


class Ints:
    def __init__(self, n):
        self.ptr, self.nbytes = FAKE, 4 * n


def test_decode_attention_fwd_shape_checks_raise():
    d = asr.xattn_desc(2, 8)
    N, Tk, S, E = 3, 5, 4, 16
    ok = dict(q=Buf(N, E), k=Buf(Tk * S, E), v=Buf(Tk * S, E), out=Buf(N, E))
    table = np.zeros((Tk, N), int)
    for name, bad in (("q", Buf(N - 1, E)), ("k", Buf(Tk * S - 1, E)), ("v", Buf(Tk * S, E - 1)),
                      ("out", Buf(N, E - 4))):
        a = dict(ok, **{name: bad})
        with pytest.raises(ValueError, match=f"decode_attention_fwd: {name}"):
            asr.decode_attention_fwd(a["q"], a["k"], a["v"], a["out"], N, Tk, S, d, table, ldc=N)
    call = lambda cols, ldc, **kw: asr.decode_attention_fwd(ok["q"], ok["k"], ok["v"], ok["out"], N, Tk, S, d,   # noqa: E731
                                                            cols, ldc=ldc, **kw)
    with pytest.raises(ValueError, match="ldc"):
        call(table, 2)
    with pytest.raises(ValueError, match="cols is required"):
        call(None, 0)
    with pytest.raises(ValueError, match="cols: shape"):
        call(table[:-1], N)
    with pytest.raises(ValueError, match="cols: shape"):
        call(np.zeros(N + 1, int), 0)
    for bad in (S, -1):
        t = table.copy()
        t[2, 1] = bad
        with pytest.raises(ValueError, match="cols: a value outside"):
            call(t, N)
        with pytest.raises(ValueError, match="cols: a value outside"):
            call(t[2], 0)
    with pytest.raises(ValueError, match="cols"):
        call(Ints(Tk * N - 1), N)
    with pytest.raises(ValueError, match="lengths"):
        call(table, N, lengths=[1, 2])
    with pytest.raises(ValueError, match="lengths"):
        call(table, N, lengths=Ints(N - 1))


def test_embed_and_beam_step_shape_checks_raise():
    with pytest.raises(ValueError, match="embed_fwd: emb"):
        asr.embed_fwd(Buf(10, 8), None, [0, 1], None, Buf(2, 8), 2, 8, 11)
    with pytest.raises(ValueError, match="embed_fwd: out"):
        asr.embed_fwd(Buf(11, 8), None, [0, 1], None, Buf(1, 8), 2, 8, 11)
    with pytest.raises(ValueError, match="tokens"):
        asr.embed_fwd(Buf(11, 8), None, [0, 1, 2], None, Buf(2, 8), 2, 8, 11)
    with pytest.raises(ValueError, match="tokens is required"):
        asr.embed_fwd(Buf(11, 8), None, None, None, Buf(2, 8), 2, 8, 11)
    with pytest.raises(ValueError, match="pe needs"):
        asr.embed_fwd(Buf(11, 8), Ints(2 * 4 * 8 - 1), [0, 1], [0, 1], Buf(2, 8), 2, 8, 11, P=4)
    with pytest.raises(ValueError, match="pe needs pos"):
        asr.embed_fwd(Buf(11, 8), Ints(2 * 4 * 8), [0, 1], None, Buf(2, 8), 2, 8, 11, P=4)
    with pytest.raises(ValueError, match="pos"):
        asr.embed_fwd(Buf(11, 8), Ints(2 * 4 * 8), [0, 1], [0], Buf(2, 8), 2, 8, 11, P=4)
    B, K, V, L = 2, 3, 5, 4
    N = B * K
    d = asr.attn_beam_desc(B, K, V, L, 1, 4)
    ok = dict(logp=Buf(N, V), scores=Ints(2 * N), finished=Ints(N), tokens_in=Ints(L * N), anc_in=Ints(L * N),
              scores_out=Ints(2 * N), finished_out=Ints(N), parent=Ints(N), token=Ints(N), tokens_out=Ints(L * N),
              anc_out=Ints(L * N), all_finished=Ints(1))
    small = dict(logp=Buf(N - 1, V), scores=Ints(2 * N - 1), finished=Ints(N - 1), tokens_in=Ints(L * N - 1),
                 anc_in=Ints(L * N - 1), scores_out=Ints(2 * N - 1), finished_out=Ints(N - 1), parent=Ints(N - 1),
                 token=Ints(N - 1), tokens_out=Ints(L * N - 1), anc_out=Ints(L * N - 1), all_finished=Ints(0))
    for name in ok:
        with pytest.raises(ValueError, match=f"attn_beam_step: {name}"):
            asr.attn_beam_step(d, **dict(ok, **{name: small[name]}))


def test_layer_step_shape_checks_raise():
    E, N, T, B = 16, 4, 5, 2
    mha, ca = object.__new__(asr.MultiheadAttention), object.__new__(asr.CrossAttention)
    mha.E = ca.E = E
    mha.heads = ca.heads = 2
    mha.desc = asr.attn_desc(2, E // 2, 0.0, 1, -1, 0)
    cache, x, kv = Buf(3 * N, 3 * E), Buf(N, E), Buf(T * B, 2 * E)
    for window in ((1, 8, 0), (1, -1, 2), (4, -1, 0), (1, -1, -1)):      # forward()'s window is not the cache's
        lim = object.__new__(asr.MultiheadAttention)
        lim.E, lim.heads, lim.desc = E, 2, asr.attn_desc(2, E // 2, 0.0, *window)
        with pytest.raises(ValueError, match="must be causal"):
            lim.step(x, N, cache, 0, Ints(N))
    with pytest.raises(ValueError, match="MultiheadAttention.step: anc"):      # a host table, before any allocation
        mha.step(x, N, cache, 1, np.full((2, N), N))
    with pytest.raises(ValueError, match="MultiheadAttention.step: out"):
        mha.step(x, N, cache, 0, Ints(N), out=Buf(N - 1, E))
    with pytest.raises(ValueError, match="MultiheadAttention.step: x"):
        mha.step(Buf(N - 1, E), N, cache, 0, Ints(N))
    with pytest.raises(ValueError, match="MultiheadAttention.step: cache"):
        mha.step(x, N, cache, 3, Ints(4 * N))
    with pytest.raises(ValueError, match="MultiheadAttention.step: cache"):
        mha.step(x, N, Buf(3 * N, 2 * E), 0, Ints(N))
    with pytest.raises(ValueError, match="MultiheadAttention.step: anc"):
        mha.step(x, N, cache, 2, Ints(3 * N - 1))
    with pytest.raises(ValueError, match="CrossAttention.step: x"):
        ca.step(Buf(N, E + 1), N, kv, T, B, [0, 2, 4])
    with pytest.raises(ValueError, match="CrossAttention.step: kv"):
        ca.step(x, N, Buf(T * B - 1, 2 * E), T, B, [0, 2, 4])
    with pytest.raises(ValueError, match="CrossAttention.step: out"):
        ca.step(x, N, kv, T, B, [0, 2, 4], out=Buf(N, E - 1))
    with pytest.raises(ValueError, match="hyp_offsets is required"):
        ca.step(x, N, kv, T, B, None)
    with pytest.raises(ValueError, match="CrossAttention.step: 2 hyp_offsets"):
        ca.step(x, N, kv, T, B, [0, 4])
    with pytest.raises(ValueError, match="CrossAttention.step: hyp_offsets"):
        ca.step(x, N, kv, T, B, Ints(B))
    with pytest.raises(ValueError, match="CrossAttention.step: 3 k_lengths"):
        ca.step(x, N, kv, T, B, [0, 2, 4], k_lengths=[5, 5, 5])
