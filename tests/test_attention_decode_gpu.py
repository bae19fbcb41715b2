"""GPU numerics of attention-decoder beam search (asr_decode_attention_fwd,
asr_embed_fwd, asr_attn_beam_step, and the step / begin / beam_search layer of
asr.TransformerDecoder).

References: attention_decode_reference.py (float64; checked against each other
in test_attention_decode_cpu.py).  Bound: the project's bound for fp32 kernels,
|err| <= 2e-5 * (1 + |ref|); a hypothesis score, a sum of per-token log-probs,
gets attention_decoder_reference.score_bound.  Inputs as in
test_attention_decoder_gpu.py: Q, K, V and the memory U(+-1), weights
U(+-1/sqrt(fan-in)), biases U(+-0.1), LayerNorm gamma U(0.5, 1.5).  Each case
prints its max error.  Bit-equality cases compare with np.array_equal.

The kernel walks 64-key blocks with a key per lane, so Tk = 1, 63, 64, 65 and
130 are one key, the block edge on both sides and a third block of 2; N = 7
hypotheses over S = 3 columns with lengths that include 0 and Tk.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (one HIP runtime per process: conftest.py)

import attention_decode_reference as ref
import attention_decoder_reference as adr
from conftest import asr

pytestmark = pytest.mark.gpu
ATOL = ref.ATOL
SENT = -12345.0
N, S = ref.DATTN_N, ref.DATTN_S
CASES = [(h, d, tk) for h, d in ref.DATTN_DIMS for tk in ref.DATTN_TK]
case_id = lambda c: "x".join(map(str, c))   # noqa: E731


class View:
    """rows x cols floats at a device address that something else owns."""

    def __init__(self, ptr, rows, cols, keep):
        self.ptr, self.rows, self.cols, self._keep = ptr, rows, cols, keep


def dm(a):
    return asr.DeviceMatrix.from_numpy(np.asarray(a, np.float32))


def close(got, want, what="", atol=ATOL):
    want = np.asarray(want, np.float64)
    err = np.abs(np.asarray(got, np.float64) - want)
    print(f"{what} max err {err.max():.3e} (max err / (1 + |ref|) {(err / (1 + np.abs(want))).max():.3e})")
    assert np.all(np.isfinite(got))
    assert np.all(err <= atol * (1.0 + np.abs(want))), f"{what} max err {err.max()}"


def put(a2d, ld=None, fill=np.nan, misalign=False):
    """a2d [rows][n] on the device with row stride ld (extra columns hold fill);
    misalign: the buffer starts 4 bytes past a 16-byte boundary."""
    rows, n = a2d.shape
    ld = ld or n
    h = np.full((rows, ld), fill, np.float32)
    h[:, :n] = a2d
    if not misalign:
        d = dm(h)
        assert d.ptr % 16 == 0
        return d
    base = dm(np.concatenate([np.zeros(1, np.float32), h.reshape(-1), np.zeros(3, np.float32)]).reshape(-1, 1))
    v = View(base.ptr + 4, rows, ld, base)
    assert v.ptr % 16 == 4
    return v


def fetch(view, rows, ld):
    out = np.empty((rows, ld), np.float32)
    asr.check(asr.lib().asr_memcpy_d2h(out.ctypes.data, view.ptr, out.nbytes, None), "asr_memcpy_d2h")
    return out


def run(q, k, v, heads, cols, lengths=None, ld=None, ldo=None, misalign=False, fused_kv=False):
    """asr_decode_attention_fwd on q [N][E], k, v [Tk][S][E]; cols [Tk][N] (a
    table, ldc = N) or [N] (ldc = 0), uploaded as they are; returns out
    [N][ldo], every element a sentinel before the call.  ld: row stride of q, k
    and v (extra columns NaN); ldo: of out; misalign: all buffers 4 bytes past a
    16-byte boundary; fused_kv: k and v as the column ranges of one [Tk*S, 2E]
    buffer."""
    n, E = q.shape
    Tk, s_cols, _ = k.shape
    desc = asr.xattn_desc(heads, E // heads)
    dq = put(q, ld, misalign=misalign)
    if fused_kv:
        assert ld is None
        buf = put(np.concatenate([k, v], axis=2).reshape(Tk * s_cols, 2 * E), misalign=misalign)
        dk, dv = View(buf.ptr, Tk * s_cols, 2 * E, buf), View(buf.ptr + 4 * E, Tk * s_cols, 2 * E, buf)
        ldk = ldv = 2 * E
    else:
        dk, dv = (put(a.reshape(-1, E), ld, misalign=misalign) for a in (k, v))
        ldk = ldv = None
    ldo = ldo or E
    out = put(np.full((n, ldo), SENT, np.float32), misalign=misalign)
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    d_len = None if lengths is None else asr.device_lengths(lengths)
    asr.decode_attention_fwd(dq, dk, dv, out, n, Tk, s_cols, desc, asr.device_lengths(cols.reshape(-1)),
                             ldc=n if cols.ndim == 2 else 0, lengths=d_len, ldk=ldk, ldv=ldv, ldo=ldo)
    asr.synchronize()
    return fetch(out, n, ldo)


@functools.lru_cache(maxsize=None)
def inputs(case):
    heads, D, Tk = case
    a = ref.draw_decode(heads, D, Tk)
    for x in a:
        x.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(case, table):
    q, k, v, tab, col = inputs(case)
    out = ref.decode_attention_ref(q, k, v, case[0], tab if table else col, ref.dattn_lengths(case[2]))
    out.setflags(write=False)
    return out


def poisoned(case, table):
    """The case's K and V with NaN in every row past the lengths and every (key, column) the table does not name."""
    q, k, v, tab, col = inputs(case)
    t = tab if table else np.tile(col, (case[2], 1))
    ln = ref.dattn_lengths(case[2])
    return ref.nan_unnamed(k, t, ln), ref.nan_unnamed(v, t, ln)


# ------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("table", [False, True], ids=["ldc0", "ancestry"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_decode_attention_values(case, table):
    """N = 7 over S = 3 columns, one column per hypothesis (ldc = 0) or a random
    ancestry table; lengths with 0 and Tk; NaN in every K / V row past the
    lengths and in every slot the table does not name; a sentinel beyond column
    E of out."""
    heads, D, Tk = case
    q, _, _, tab, col = inputs(case)
    k, v = poisoned(case, table)
    E, ln = heads * D, ref.dattn_lengths(Tk)
    out = run(q, k, v, heads, tab if table else col, ln, ldo=E + 3)
    assert np.all(out[:, E:] == SENT)
    assert np.all(out[ln == 0, :E] == 0)
    close(out[:, :E], reference(case, table), f"decode attention {case} table {table}")


def test_decode_attention_without_lengths_and_explicit_scale():
    heads, D, Tk = 2, 16, 65
    q, k, v, tab, _ = inputs((heads, D, Tk))
    desc = asr.xattn_desc(heads, D, 0.37)
    out = asr.DeviceMatrix(N, heads * D)
    asr.decode_attention_fwd(dm(q), dm(k.reshape(-1, heads * D)), dm(v.reshape(-1, heads * D)), out, N, Tk, S, desc,
                             tab, ldc=N)            # a host table: validated and uploaded by the wrapper
    close(out.toCpu(), ref.decode_attention_ref(q, k, v, heads, tab, None, 0.37), "no lengths, scale 0.37")


# ----------------------------------------------------------- 2. bit equality
BIT_CASES = [(2, 20, 130), (2, 64, 65), (1, 128, 64), (2, 4, 63)]


@pytest.mark.parametrize("case", BIT_CASES, ids=case_id)
def test_rows_do_not_depend_on_where_the_keys_lie(case):
    """The indirect table against the same keys gathered into a contiguous
    cache read with the identity table; ldc = 0 against a full table holding
    the same column in every row."""
    heads, D, Tk = case
    q, k, v, tab, col = inputs(case)
    ln = ref.dattn_lengths(Tk)
    base = run(q, k, v, heads, tab, ln)
    j = np.arange(Tk)[:, None]
    gathered = run(q, k[j, tab], v[j, tab], heads, np.tile(np.arange(N), (Tk, 1)), ln)       # S = N columns
    assert np.array_equal(base, gathered)
    one = run(q, k, v, heads, col, ln)
    assert np.array_equal(one, run(q, k, v, heads, np.tile(col, (Tk, 1)), ln))


@pytest.mark.parametrize("case", BIT_CASES, ids=case_id)
def test_rows_do_not_depend_on_the_slot_or_on_n(case):
    """The hypotheses permuted, and N doubled (every hypothesis twice)."""
    heads, D, Tk = case
    q, k, v, tab, _ = inputs(case)
    ln = ref.dattn_lengths(Tk)
    base = run(q, k, v, heads, tab, ln)
    perm = np.array([3, 6, 0, 5, 1, 4, 2])
    assert np.array_equal(base[perm], run(q[perm], k, v, heads, tab[:, perm], ln[perm]))
    twice = np.concatenate([np.arange(N), perm])
    assert np.array_equal(base[twice], run(q[twice], k, v, heads, tab[:, twice], ln[twice]))


@pytest.mark.parametrize("case", BIT_CASES, ids=case_id)
def test_rows_do_not_depend_on_strides_alignment_or_a_fused_kv_buffer(case):
    heads, D, Tk = case
    q, k, v, tab, _ = inputs(case)
    E, ln = heads * D, ref.dattn_lengths(Tk)
    base = run(q, k, v, heads, tab, ln)
    assert np.array_equal(base, run(q, k, v, heads, tab, ln, ld=E + 1, ldo=E + 1)[:, :E])
    assert np.array_equal(base, run(q, k, v, heads, tab, ln, misalign=True))
    assert np.array_equal(base, run(q, k, v, heads, tab, ln, fused_kv=True))


# ---------------------------------------------------------------- 3. the clamp
def test_a_garbage_table_is_clamped():
    """Columns outside [0, S) are clamped, tested without leaving any
    allocation: the K / V allocations hold S slots in front of the Tk*S slots
    the call sees and S behind them (the base pointer passed is S slots into
    the allocation), each slot 2E floats wide (ld = 2E) with NaN in its upper
    half, NaN in the 2S extra slots and in every slot no live (j, n) names.
    The table holds values in [S, 2S) and negative ones down to -S: unclamped
    they would address another slot INSIDE the allocation (the next key's, the
    one before, or an extra one).  The output must be finite and equal the call
    with the clamped table."""
    heads, D, Tk = 2, 20, 65
    E = heads * D
    q, k, v, tab, _ = inputs((heads, D, Tk))
    ln = ref.dattn_lengths(Tk)
    first = S
    slots = np.full((Tk * S + 2 * S, 2 * E), np.nan, np.float32)
    kslots, vslots = slots.copy(), slots.copy()
    kslots[first:first + Tk * S, :E] = k.reshape(Tk * S, E)
    vslots[first:first + Tk * S, :E] = v.reshape(Tk * S, E)
    # NaN where no live (j, n) names the slot, also inside the call's range
    named = ~np.isnan(ref.nan_unnamed(k, np.clip(tab, 0, S - 1), ln).reshape(Tk * S, E)[:, 0])
    kslots[first:first + Tk * S][~named] = np.nan
    vslots[first:first + Tk * S][~named] = np.nan

    def call(table):
        dq, dk, dv, out = dm(q), dm(kslots), dm(vslots), dm(np.full((N, E), SENT, np.float32))
        d_cols = asr.device_lengths(np.ascontiguousarray(table, np.int32).reshape(-1))
        d_len, desc = asr.device_lengths(ln), asr.xattn_desc(heads, D)
        asr.check(asr.lib().asr_decode_attention_fwd(
            ctypes.byref(desc), dq.ptr, E, dk.ptr + 4 * first * 2 * E, 2 * E, dv.ptr + 4 * first * 2 * E, 2 * E,
            d_cols.ptr, N, d_len.ptr, out.ptr, E, N, Tk, S, None), "asr_decode_attention_fwd")
        asr.synchronize()                            # every buffer above lives until here
        return out.toCpu()

    # columns in [S, 2S) where the clamped value is S - 1, negative ones (down to -S) where it is 0
    wild = np.where(tab == S - 1, tab + 1 + (np.arange(Tk)[:, None] % S), np.where(tab == 0, -1 - (np.arange(N) % S),
                                                                                   tab))
    assert (wild >= S).any() and (wild < 0).any() and wild.max() < 2 * S and wild.min() >= -S
    assert np.array_equal(np.clip(wild, 0, S - 1), tab)
    got, want = call(wild), call(tab)
    assert np.all(np.isfinite(got))
    assert np.array_equal(got, want)
    close(want, ref.decode_attention_ref(q, k, v, heads, tab, ln), "clamped table")


# ------------------------------------------------------------- 4. embedding
@pytest.mark.parametrize("E", [32, 36])
def test_embed_equals_the_host_gather(E):
    V, U, Nh = 11, 9, 5
    rng = np.random.default_rng(E)
    emb = rng.uniform(-1, 1, (V, E)).astype(np.float32)
    w = rng.uniform(-1, 1, (E, V)).astype(np.float32)
    layer = asr.TransformerDecoderLayer(asr.MultiheadAttention(E, 1, chunk=1, left=-1, right=0),
                                        asr.CrossAttention(E, 1), asr.LayerNorm(E), asr.LayerNorm(E), asr.LayerNorm(E),
                                        np.zeros((E, 8)), np.zeros(8), np.zeros((8, E)), np.zeros(E))
    for pos_enc, scale in ((True, True), (False, True), (True, False)):
        dec = asr.TransformerDecoder(emb, [layer], w, scale_embedding=scale, positional_encoding=pos_enc)
        tokens = rng.integers(0, V, (U, Nh))
        want = dec.embed(tokens)
        out = asr.DeviceMatrix(U * Nh, E + 2)
        out.toGpu(np.full((U * Nh, E + 2), SENT, np.float32))
        pos = np.repeat(np.arange(U), Nh)
        asr.embed_fwd(dm(emb), dec._pe_dev(U), tokens.reshape(-1), pos if pos_enc else None, out, U * Nh, E, V, U,
                      dec.emb_scale)
        got = out.toCpu()
        assert np.array_equal(got[:, :E], want) and np.all(got[:, E:] == SENT)
    # a token or a position outside its table: a zero row
    tokens = np.array([0, V, -1, 3, 4], np.int32)
    pos = np.array([0, 1, 2, U, -1], np.int32)
    dec = asr.TransformerDecoder(emb, [layer], w)
    out = asr.DeviceMatrix(5, E)
    asr.embed_fwd(dm(emb), dec._pe_dev(U), tokens, pos, out, 5, E, V, U, dec.emb_scale)
    got = out.toCpu()
    assert np.array_equal(got[0], dec.embed(np.array([[0]]))[0]) and np.all(got[1:] == 0)


# ------------------------------------------------------------- 5. beam step
@pytest.mark.parametrize("kind", ref.BEAM_KINDS)
@pytest.mark.parametrize("V,K", ref.BEAM_SHAPES)
def test_beam_step_equals_the_host_twin(kind, V, K):
    B, L = ref.BEAM_B, ref.BEAM_MAX_LEN
    Nn = B * K
    logp, scores, fin, tin, ain, step = ref.beam_case(kind, V, K)
    d = asr.attn_beam_desc(B, K, V, L, step, V - 1)
    want = asr.attn_beam_step_host(d, logp, scores, fin, tin, ain)
    up = asr._upload
    so, fo, par, tok, live = (asr.DeviceBytes(8 * Nn), asr.DeviceBytes(4 * Nn), asr.DeviceBytes(4 * Nn),
                              asr.DeviceBytes(4 * Nn), up(np.array([77], np.int32)))
    tout, aout = up(tin), up(ain)                   # the twin's out tables start as copies too
    asr.attn_beam_step(d, put(logp, V + 3), up(scores), up(fin), up(tin), up(ain), so, fo, par, tok, tout, aout,
                       live)
    dl = asr._download
    got = (dl(so, Nn, np.float64), dl(fo, Nn, np.int32), dl(par, Nn, np.int32), dl(tok, Nn, np.int32),
           dl(tout, (L, Nn), np.int32), dl(aout, (L, Nn), np.int32), int(dl(live, 1, np.int32)[0]))
    for name, g, w in zip(("scores", "finished", "parent", "token", "tokens_out", "anc_out", "live"), got, want):
        assert np.array_equal(g, w), (name, g, w)


# ------------------------------------------------------- 6. stepwise parity
STEP = dict(E=32, heads=2, F=64, V=11, B=3, K=4, T=70, enc=(70, 33, 0), steps=70, at=(0, 1, 63, 64, 69))


def toolkit_decoder(normalize_before):
    c = STEP
    layers = [adr.make_toolkit_layer(normalize_before, c["E"], c["heads"], c["F"], seed=10 * i) for i in range(2)]
    torch.manual_seed(4000 + int(normalize_before))
    emb = torch.nn.Embedding(c["V"], c["E"])
    out = torch.nn.Linear(c["E"], c["V"])
    norm = torch.nn.LayerNorm(c["E"])
    with torch.no_grad():
        emb.weight.uniform_(-1, 1).mul_(1.0 / np.sqrt(c["E"]))
        out.weight.uniform_(-1, 1).mul_(1.0 / np.sqrt(c["E"]))
        norm.weight.uniform_(0.5, 1.5)
    w, b = asr._torch_linear(out)
    return asr.TransformerDecoder(emb.weight.detach().numpy(),
                                  [asr.TransformerDecoderLayer.from_linears(**l.parts()) for l in layers], w, b,
                                  asr.LayerNorm.from_torch(norm) if normalize_before else None)


def torch_decoder(norm_first):
    c = STEP
    return asr.TransformerDecoder.from_torch(*adr.make_decoder(norm_first, seed=20, E=c["E"], heads=c["heads"],
                                                               F=c["F"], layers=2, V=c["V"]))


@pytest.mark.parametrize("norm_first", [True, False], ids=["pre", "post"])
@pytest.mark.parametrize("layout", ["torch", "toolkit"])
def test_steps_on_the_cache_equal_the_teacher_forced_decoder(layout, norm_first):
    """70 steps of step() driven with random tokens and random parents from a
    fixed seed (the self-attention cache crosses 64 keys); at steps 0, 1, 63, 64
    and 69 the log-probs of every slot equal log_probs() on that slot's
    reconstructed prefix, within the bound.  Encoder lengths (70, 33, 0)."""
    c = STEP
    dec = torch_decoder(norm_first) if layout == "torch" else toolkit_decoder(norm_first)
    B, K, T, V = c["B"], c["K"], c["T"], c["V"]
    Nn, sos = B * K, V - 1
    memory = dm(adr.draw_memory(T, B, c["E"], seed=9).reshape(T * B, c["E"]))
    rng = np.random.default_rng(11)
    state = dec.begin(memory, T, B, c["enc"], beam=K, max_len=c["steps"], sos=sos)
    prefixes, tokens, parents = [[] for _ in range(Nn)], None, None
    utt = (np.arange(Nn) // K).tolist()
    for s in range(c["steps"]):
        logp = dec.step(state, tokens, parents)
        if s in c["at"]:
            got = logp.toCpu()
            tin = np.full((s + 1, Nn), sos, np.int32)
            for n, p in enumerate(prefixes):
                tin[1:, n] = p
            full, _, _ = dec.log_probs(tin, [s + 1] * Nn, utt, memory, T, B, c["enc"])
            want = full.toCpu().reshape(s + 1, Nn, V)[s]
            close(got, want, f"{layout} norm_first {norm_first} step {s}")
        if s == c["steps"] - 1:
            break
        parents = (np.arange(Nn) // K) * K + rng.integers(0, K, Nn)
        tokens = rng.integers(0, V, Nn)
        prefixes = [prefixes[p] + [int(t)] for p, t in zip(parents, tokens)]
    tok, _, _, _ = state.tables()                    # the state's token table is the prefixes
    assert tok.shape[0] == c["steps"] - 1 and [tok[:, n].tolist() for n in range(Nn)] == prefixes


# --------------------------------------------------------- 7. search parity
@functools.lru_cache(maxsize=None)
def search_reference(case):
    K, bias, max_len, seed = case
    memory, modules = ref.search_model(seed, bias)
    res, worst = ref.beam_search_ref(modules, memory, ref.SEARCH["enc_lengths"], K, max_len, 10, 10)
    return memory, modules, res, worst


@pytest.mark.parametrize("case", ref.SEARCH_CASES, ids=case_id)
def test_beam_search_equals_the_float64_recompute_search(case):
    K, bias, max_len, seed = case
    c = ref.SEARCH
    memory, modules, want, worst = search_reference(case)
    assert worst >= 2, worst                         # the reference keeps its margin at every prune
    dec = asr.TransformerDecoder.from_torch(*modules)
    T, B, E = memory.shape
    d_mem = dm(memory.reshape(T * B, E))
    got = dec.beam_search(d_mem, T, B, c["enc_lengths"], beam=K, max_len=max_len, sos=10, eos=10)
    print(f"case {case}: margin {worst:.2f}, lengths {[[len(y) for y, _ in u] for u in got]}")
    assert [[y for y, _ in u] for u in got] == [[y for y, _ in u] for u in want]
    flat = [(y, s, w) for u, uw in zip(got, want) for (y, s), (_, w) in zip(u, uw)]
    hyps, utt = [y for u in got for y, _ in u], [b for b, u in enumerate(got) for _ in u]
    # a hypothesis that has not ended is scored without its eos term: compare only the ended ones with score()
    forced = dec.score(hyps, utt, d_mem, T, B, c["enc_lengths"], sos=10, eos=10)
    for (y, s, w), f in zip(flat, forced):
        ended = len(y) < max_len                     # a hypothesis of max_len tokens has not ended: no eos term
        assert abs(s - w) <= adr.score_bound(len(y) + ended, w), (y, s, w)
        if ended:                                    # the cache path against the teacher-forced path
            assert abs(s - f) <= adr.score_bound(len(y) + 1, f), (y, s, f)
    if K == 1:
        assert dec.greedy(d_mem, T, B, c["enc_lengths"], max_len=max_len, sos=10, eos=10) == got


def test_an_utterance_without_frames_returns_the_empty_hypothesis():
    K, bias, max_len, seed = ref.SEARCH_CASES[1]
    memory, modules = ref.search_model(seed, bias)
    dec = asr.TransformerDecoder.from_torch(*modules)
    T, B, E = memory.shape
    d_mem = dm(memory.reshape(T * B, E))
    enc = (70, 0, 5)
    got = dec.beam_search(d_mem, T, B, enc, beam=K, max_len=6, sos=10, eos=10, nbest=2)
    assert len(got) == B and all(len(u) <= 2 for u in got) and [y for y, _ in got[1]] == [[]]
    want = dec.score([[]], [1], d_mem, T, B, enc, sos=10, eos=10)[0]
    assert abs(got[1][0][1] - want) <= adr.score_bound(1, want)
    full = dec.beam_search(d_mem, T, B, (70, 33, 5), beam=K, max_len=6, sos=10, eos=10)
    assert got[0] == full[0][:2] and got[2] == full[2][:2]      # the other utterances do not notice
    # its slots leave the search after step 0, so they hold no one up: with every utterance empty the loop is over
    # after the second step although no hypothesis has emitted eos
    state = dec.begin(d_mem, T, B, (0, 0, 0), beam=K, max_len=6, sos=10)
    assert dec.prune(state, dec.step(state), 10) > 0
    state.drop_utterances([0, 1, 2])
    assert dec.prune(state, dec.step(state), 10) == 0 and np.isinf(state.tables()[2]).all()
    assert dec.beam_search(d_mem, T, B, (0, 0, 0), beam=K, max_len=6, sos=10, eos=10) == [got[1]] * B


# ----------------------------------------------------------- 8. shape errors
def test_steps_refuse_buffers_smaller_than_the_call():
    """Every new step / forward over more rows than its input has: ValueError before any device call."""
    c = STEP
    E, T, B, K = c["E"], 5, 2, 2
    Nn = B * K
    modules = adr.make_decoder(True, seed=20, E=E, heads=c["heads"], F=c["F"], layers=2, V=c["V"])
    dec = asr.TransformerDecoder.from_torch(*modules)
    layer = dec.layers[0]
    x, small = asr.DeviceMatrix(Nn, E), asr.DeviceMatrix(Nn - 1, E)
    cache, kv = asr.DeviceMatrix(3 * Nn, 3 * E), asr.DeviceMatrix(T * B, 2 * E)
    anc = np.tile(np.arange(Nn), (3, 1))
    off = [0, 2, 4]
    with pytest.raises(ValueError, match="MultiheadAttention.step: x"):
        layer.self_attn.step(small, Nn, cache, 0, anc)
    with pytest.raises(ValueError, match="MultiheadAttention.step: cache"):
        layer.self_attn.step(x, Nn, cache, 3, anc)
    with pytest.raises(ValueError, match="MultiheadAttention.step: anc"):
        layer.self_attn.step(x, Nn, cache, 1, np.full((2, Nn), Nn))
    with pytest.raises(ValueError, match="CrossAttention.step: x"):
        layer.cross_attn.step(small, Nn, kv, T, B, off)
    with pytest.raises(ValueError, match="CrossAttention.step: kv"):
        layer.cross_attn.step(x, Nn, kv, T + 1, B, off)
    with pytest.raises(ValueError, match="CrossAttention.step: .*hyp_offsets"):
        layer.cross_attn.step(x, Nn, kv, T, B, [0, 2])
    with pytest.raises(ValueError, match="CrossAttention.step: .*k_lengths"):
        layer.cross_attn.step(x, Nn, kv, T, B, off, k_lengths=[5])
    with pytest.raises(ValueError, match="TransformerDecoderLayer.step: x"):
        layer.step(small, Nn, cache, 0, anc, kv, T, B, off)
    with pytest.raises(ValueError, match="TransformerDecoderLayer.step: kv"):
        layer.step(x, Nn, cache, 0, anc, kv, T + 1, B, off)
    with pytest.raises(ValueError, match="TransformerDecoderLayer.step: cache"):
        layer.step(x, Nn, cache, 3, anc, kv, T, B, off)
    with pytest.raises(ValueError, match="TransformerDecoderLayer.step: out"):
        layer.step(x, Nn, cache, 0, anc, kv, T, B, off, out=small)
    memory = asr.DeviceMatrix(T * B, E)
    with pytest.raises(ValueError, match="begin: memory"):
        dec.begin(memory, T + 1, B)
    with pytest.raises(ValueError, match="beam"):
        dec.begin(memory, T, B, beam=17)
    with pytest.raises(ValueError, match="enc_lengths"):
        dec.begin(memory, T, B, [5])
    state = dec.begin(memory, T, B, beam=K, max_len=2)
    with pytest.raises(ValueError, match="come together"):
        dec.step(state, tokens=[1] * Nn)
    with pytest.raises(ValueError, match="decide a step"):
        dec.step(state, [1] * Nn, [0, 1, 2, 3])
    dec.step(state)
    with pytest.raises(ValueError, match="not decided"):
        dec.step(state)
    with pytest.raises(ValueError, match="parent outside"):
        dec.step(state, [1] * Nn, [2, 1, 2, 3])
    with pytest.raises(ValueError, match="token outside"):
        dec.step(state, [c["V"]] * Nn, [0, 1, 2, 3])
    with pytest.raises(ValueError, match="tokens .* not"):
        dec.step(state, [1] * (Nn - 1), [0, 1, 2])
    dec.step(state, [1] * Nn, [0, 0, 3, 3])
    with pytest.raises(ValueError, match="used up"):
        dec.step(state, [1] * Nn, [0, 1, 2, 3])
