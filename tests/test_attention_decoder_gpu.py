"""GPU numerics of attention-decoder rescoring (asr_cross_attention_fwd,
asr_token_score, asr.CrossAttention, asr.TransformerDecoderLayer,
asr.TransformerDecoder, asr.CTCDecoder.attention_rescore).

References: attention_decoder_reference.py (float64; checked against torch in
test_attention_decoder_cpu.py).  Bound: the project's bound for fp32 kernels,
|err| <= 2e-5 * (1 + |ref|) (test_attention_gpu.py, and what test_conformer_gpu.py
uses for a layer against its float64 block); a hypothesis score, a sum of at
most U + 1 per-token log-probs, gets (U + 1) times that.  Inputs: Q, K, V, x and
the memory U(+-1), weights U(+-1/sqrt(fan-in)), biases U(+-0.1), LayerNorm gamma
U(0.5, 1.5).  Each case prints its max error.

The kernel's tiles are the ones attention_decoder_reference.XATTN_CASES were
chosen for: 64 flat queries per workgroup, token-major over the hypotheses of
one utterance (5 hypotheses x 13 tokens = 65: a second tile with one live lane),
64-key blocks (T = 70: a second block of 6 keys), one instantiation per
ceil(head_dim / 16).  Bit-equality cases compare with np.array_equal.
"""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (one HIP runtime per process: conftest.py)

import attention_decoder_reference as adr
from conftest import asr

pytestmark = pytest.mark.gpu
ATOL = adr.ATOL
SENT = -12345.0
case_id = lambda c: "x".join(map(str, c))   # noqa: E731


class View:
    """rows x cols floats at a device address that something else owns."""

    def __init__(self, ptr, rows, cols, keep):
        self.ptr, self.rows, self.cols, self._keep = ptr, rows, cols, keep


def dm(a):
    return asr.DeviceMatrix.from_numpy(np.asarray(a, np.float32))


def close(got, ref, what="", atol=ATOL):
    ref = np.asarray(ref, np.float64)
    err = np.abs(np.asarray(got, np.float64) - ref)
    print(f"{what} max err {err.max():.3e} (max err / (1 + |ref|) {(err / (1 + np.abs(ref))).max():.3e})")
    assert np.all(np.isfinite(got))
    assert np.all(err <= atol * (1.0 + np.abs(ref))), f"{what} max err {err.max()}"


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


def run(q, k, v, heads, off, max_hyps, qlen=None, klen=None, ld=None, ldo=None, misalign=False, fused_kv=False):
    """asr_cross_attention_fwd on q [U][N][E], k, v [T][B][E]; returns out
    [U][N][ldo], every element a sentinel before the call.  ld: row stride of q,
    k and v (extra columns NaN); ldo: of out; misalign: all buffers 4 bytes past
    a 16-byte boundary; fused_kv: k and v as the column ranges of one [T*B, 2E]
    buffer."""
    Uq, N, E = q.shape
    T, B, _ = k.shape
    desc = asr.xattn_desc(heads, E // heads)
    dq = put(q.reshape(-1, E), ld, misalign=misalign)
    if fused_kv:
        assert ld is None
        buf = put(np.concatenate([k, v], axis=2).reshape(T * B, 2 * E), misalign=misalign)
        dk, dv = View(buf.ptr, T * B, 2 * E, buf), View(buf.ptr + 4 * E, T * B, 2 * E, buf)
        ldk = ldv = 2 * E
    else:
        dk, dv = (put(a.reshape(-1, E), ld, misalign=misalign) for a in (k, v))
        ldk = ldv = None
    ldo = ldo or E
    out = put(np.full((Uq * N, ldo), SENT, np.float32), misalign=misalign)
    asr.cross_attention_fwd(dq, dk, dv, out, Uq, N, T, B, desc, [int(x) for x in off], max_hyps,
                            None if qlen is None else [int(x) for x in qlen],
                            None if klen is None else [int(x) for x in klen], ldk=ldk, ldv=ldv, ldo=ldo)
    asr.synchronize()
    return fetch(out, Uq * N, ldo).reshape(Uq, N, ldo)


@functools.lru_cache(maxsize=None)
def inputs(case):
    heads, D, T = case
    qkv = adr.draw_cross(heads, D, T)
    for a in qkv:
        a.setflags(write=False)
    return qkv


@functools.lru_cache(maxsize=None)
def reference(case, klen):
    q, k, v = inputs(case)
    ref = adr.cross_attention_ref(q, k, v, case[0], adr.COUNTS, adr.QLEN, klen)
    ref.setflags(write=False)
    return ref


def poisoned(case, klen):
    """The case's Q, K, V with NaN in every row past its length."""
    q, k, v = inputs(case)
    return adr.nan_past(q, adr.QLEN), adr.nan_past(k, klen), adr.nan_past(v, klen)


# ------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("case", adr.XATTN_CASES, ids=case_id)
def test_cross_attention_values(case):
    """B = 3 with (5, 0, 2) hypotheses, U = 13, ragged qlen with 0 and U, ragged
    klen with 0 and T, NaN past every length, a sentinel beyond column E and in
    the rows of hypotheses no utterance covers."""
    heads, D, T = case
    E, N = heads * D, sum(adr.COUNTS)
    klen = adr.klen_for(T)
    assert 0 in adr.QLEN and adr.U in adr.QLEN and 0 in klen and T in klen and len(adr.QLEN) == N
    q, k, v = poisoned(case, klen)
    ref = reference(case, klen)
    off = adr.offsets(adr.COUNTS)
    got = run(q, k, v, heads, off, max(adr.COUNTS), adr.QLEN, klen, ldo=E + 3)
    assert np.all(got[:, :, E:] == SENT)
    for n, (b, m) in enumerate(zip(adr.utt_of(adr.COUNTS), adr.QLEN)):
        assert not got[m:, n, :E].any(), n                       # exact zeros past the hypothesis's length
        if klen[b] == 0:
            assert not got[:, n, :E].any(), n                    # and for an utterance without frames
    close(got[:, :, :E], ref, f"cross-attention {case_id(case)}")
    # the last utterance's hypotheses taken out of the map: their rows are not written, the others' bits stay
    cut = run(q, k, v, heads, [0, 5, 5, 5], 5, adr.QLEN, klen, ldo=E + 3)
    assert np.all(cut[:, 5:] == SENT) and np.all(cut[:, :, E:] == SENT)
    assert np.array_equal(cut[:, :5, :E], got[:, :5, :E])


def test_cross_attention_without_lengths_and_explicit_scale():
    case = adr.XATTN_CASES[3]
    heads = case[0]
    q, k, v = inputs(case)
    got = run(q, k, v, heads, adr.offsets(adr.COUNTS), 5)
    close(got, adr.cross_attention_ref(q, k, v, heads, adr.COUNTS), "no lengths")
    E, T, B = q.shape[2], k.shape[0], k.shape[1]
    out = asr.DeviceMatrix(q.shape[0] * q.shape[1], E)
    asr.cross_attention_fwd(dm(q.reshape(-1, E)), dm(k.reshape(-1, E)), dm(v.reshape(-1, E)), out, q.shape[0],
                            q.shape[1], T, B, asr.xattn_desc(heads, E // heads, 0.37), adr.offsets(adr.COUNTS).tolist(),
                            5)
    asr.synchronize()
    close(out.toCpu().reshape(q.shape), adr.cross_attention_ref(q, k, v, heads, adr.COUNTS, scale=0.37), "scale 0.37")


# ---------------------------------------------------------- 2. bit equality
BIT_CASES = [adr.XATTN_CASES[0], adr.XATTN_CASES[3], adr.XATTN_CASES[4], adr.XATTN_CASES[6]]


def bit_klen(T):
    return (T - 3, T, 6)     # every utterance has frames, so every hypothesis with tokens has a row to compare


@functools.lru_cache(maxsize=None)
def grouped(case):
    heads, D, T = case
    klen = bit_klen(T)
    q, k, v = poisoned(case, klen)
    out = run(q, k, v, heads, adr.offsets(adr.COUNTS), max(adr.COUNTS), adr.QLEN, klen)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("case", BIT_CASES, ids=case_id)
def test_rows_equal_self_attention_kernel_on_the_hypothesis_alone(case):
    """asr_attention_fwd with B = 1 on hypothesis n alone: pointers offset to its
    column, strides N*ld / B*ld, Tq = qlen, Tk = klen, no window, no lengths."""
    heads, D, T = case
    E, N, B = heads * D, sum(adr.COUNTS), len(adr.COUNTS)
    klen = bit_klen(T)
    q, k, v = poisoned(case, klen)
    got = grouped(case)
    dq, dk, dv = (dm(a.reshape(-1, E)) for a in (q, k, v))
    desc = asr.attn_desc(heads, D)
    compared = 0
    for n, b in enumerate(adr.utt_of(adr.COUNTS)):
        nq, nk = adr.QLEN[n], klen[b]
        if nq == 0:
            assert not got[:, n].any()
            continue
        out = asr.DeviceMatrix(nq, E)
        asr.attention_fwd(View(dq.ptr + 4 * E * n, nq, N * E, dq), View(dk.ptr + 4 * E * b, nk, B * E, dk),
                          View(dv.ptr + 4 * E * b, nk, B * E, dv), out, nq, nk, 1, desc)
        asr.synchronize()
        assert np.array_equal(out.toCpu(), got[:nq, n]), (n, b)
        compared += 1
    assert compared == N - 1


def regroup(case, spec):
    """The case's hypotheses and memories rearranged as spec says (adr.REGROUPS)."""
    klen = bit_klen(case[2])
    q, k, v = poisoned(case, klen)
    perm = [n for _, hyps in spec for n in hyps]
    assert sorted(perm) == list(range(q.shape[1]))
    old_utt = adr.utt_of(adr.COUNTS)
    assert all(old_utt[n] == b for b, hyps in spec for n in hyps)
    src = [b for b, _ in spec]
    counts = [len(hyps) for _, hyps in spec]
    return (np.ascontiguousarray(q[:, perm]), np.ascontiguousarray(k[:, src]), np.ascontiguousarray(v[:, src]),
            counts, [adr.QLEN[n] for n in perm], [klen[b] for b in src], perm)


@pytest.mark.parametrize("spec", adr.REGROUPS, ids=["permuted", "empties", "split"])
@pytest.mark.parametrize("case", BIT_CASES[1:3], ids=case_id)
def test_rows_do_not_depend_on_the_grouping(case, spec):
    base = grouped(case)
    q, k, v, counts, qlen, klen, perm = regroup(case, spec)
    got = run(q, k, v, case[0], adr.offsets(counts), max(counts), qlen, klen)
    assert np.array_equal(got, base[:, perm])
    more = run(q, k, v, case[0], adr.offsets(counts), len(perm), qlen, klen)        # max_hyps = N: a larger grid
    assert np.array_equal(more, base[:, perm])


@pytest.mark.parametrize("case", BIT_CASES, ids=case_id)
def test_rows_do_not_depend_on_strides_alignment_or_a_fused_kv_buffer(case):
    heads, D, T = case
    E = heads * D
    base = grouped(case)
    klen = bit_klen(T)
    q, k, v = poisoned(case, klen)
    off, mh = adr.offsets(adr.COUNTS), max(adr.COUNTS)
    odd = run(q, k, v, heads, off, mh, adr.QLEN, klen, ld=E + 1, ldo=E + 1)
    assert np.array_equal(odd[:, :, :E], base) and np.all(odd[:, :, E:] == SENT)
    assert np.array_equal(run(q, k, v, heads, off, mh, adr.QLEN, klen, misalign=True), base)
    assert np.array_equal(run(q, k, v, heads, off, mh, adr.QLEN, klen, fused_kv=True), base)
    assert np.array_equal(run(q, k, v, heads, off, mh, adr.QLEN, klen, fused_kv=True, misalign=True), base)


# ------------------------------------------------------- 3. a garbage map
def test_a_garbage_map_is_clamped():
    """Offsets (0, 9, 3, N) with max_hyps = 2.  The clamps make it: utterance 0
    cnt = min(9, 2) = 2 from hypothesis 0; utterance 1 cnt = max(3 - 9, 0) = 0;
    utterance 2 cnt = min(N - 3, 2) = 2 from hypothesis min(3, N - 2) = 3.  Every
    access stays inside the buffers by construction; asserted: the call returns
    and the rows of hypotheses 2, 5 and 6, which no clamped range covers, keep
    their sentinel."""
    case = adr.XATTN_CASES[1]
    heads, D, T = case
    q, k, v = inputs(case)
    N = q.shape[1]
    got = run(q, k, v, heads, [0, 9, 3, N], 2)
    assert np.all(got[:, [2, 5, 6]] == SENT)
    assert np.all(np.isfinite(got))


# ------------------------------------------------------- 4. token scores
@pytest.mark.parametrize("V", [5, 70])
def test_token_score_is_exact(V):
    """Against numpy float64 in the same order of summation: equal, not close."""
    Uq, N = 9, 6
    rng = np.random.default_rng(V)
    z = rng.normal(0, 2, (Uq, N, V))
    logp = (z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(np.float32)
    tok = rng.integers(0, V, (Uq, N))
    ln = [9, 0, 4, 1, 9, 7]
    for ld in (V, V + 3):
        got = asr.token_score(put(logp.reshape(Uq * N, V), ld), tok, ln, Uq, N, V, ld=ld)
        ref = adr.token_score_ref(logp, tok, ln)
        assert np.array_equal(got, ref) and got[1] == 0.0 and np.all(np.isfinite(got))
    bad = tok.copy()
    bad[2, 4], bad[5, 2], bad[0, 0] = V, -1, V + 1000     # (5, 2) is past hypothesis 2's length: not counted
    got = asr.token_score(dm(logp.reshape(Uq * N, V)), bad, ln, Uq, N, V)
    ref = adr.token_score_ref(logp, bad, ln)
    assert got[4] == -np.inf and got[0] == -np.inf and np.isfinite(got[2])
    assert np.array_equal(got, ref)
    assert np.array_equal(asr.token_score(dm(logp.reshape(Uq * N, V)), tok, None, Uq, N, V),
                          adr.token_score_ref(logp, tok, [Uq] * N))


# ------------------------------------------ 5. the decoder layer and decoder
def dec_batch():
    hyps = [y for u in adr.DEC_HYPS for y in u]
    utt = [b for b, u in enumerate(adr.DEC_HYPS) for _ in u]
    return hyps, utt, [len(y) + 1 for y in hyps]


def check_layer(layer, torch_layer, what):
    E = adr.DEC["E"]
    hyps, utt, ln = dec_batch()
    Uq, N, T, B = max(ln), len(hyps), adr.DEC_T, len(adr.DEC_HYPS)
    x = np.random.default_rng(5).uniform(-1, 1, (Uq, N, E)).astype(np.float32)
    mem = adr.draw_memory(T, B, E)
    ref = adr.layer_ref(torch_layer, x, ln, utt, mem, adr.DEC_ENC_LENGTHS)
    off, mh = asr.TransformerDecoder._group(utt, B)
    kv = layer.cross_attn.project_memory(dm(adr.nan_past(mem, adr.DEC_ENC_LENGTHS).reshape(T * B, E)), T, B)
    out = layer.forward(dm(adr.nan_past(x, ln).reshape(Uq * N, E)), Uq, N, kv, T, B, ln, list(adr.DEC_ENC_LENGTHS),
                        off.tolist(), mh)
    asr.synchronize()
    assert (out.rows, out.cols) == (Uq * N, E)
    got = out.toCpu().reshape(Uq, N, E)
    mask = np.arange(Uq)[:, None] < np.asarray(ln)[None, :]
    assert not got[~mask].any()
    close(got[mask], ref[mask], what)


@pytest.mark.parametrize("norm_first", [False, True], ids=["post-norm", "pre-norm"])
def test_decoder_layer_from_torch(norm_first):
    _, dec, _ = adr.make_decoder(norm_first)
    layer = asr.TransformerDecoderLayer.from_torch(dec.layers[0])
    assert layer.norm_first is norm_first
    check_layer(layer, dec.layers[0], f"TransformerDecoderLayer norm_first={norm_first}")


@pytest.mark.parametrize("normalize_before", [True, False], ids=["pre-norm", "post-norm"])
def test_decoder_layer_from_the_toolkit_stand_in(normalize_before):
    tk = adr.make_toolkit_layer(normalize_before)
    layer = asr.TransformerDecoderLayer.from_linears(**tk.parts())
    check_layer(layer, tk, f"toolkit DecoderLayer normalize_before={normalize_before}")


@pytest.mark.parametrize("norm_first", [False, True], ids=["post-norm", "pre-norm"])
def test_decoder_score(norm_first):
    """E = 32, 4 heads, F = 64, 2 layers, V = 11: per-token log-probs at the layer
    bound, hypothesis scores at (U + 1) x it."""
    E, V = adr.DEC["E"], adr.DEC["V"]
    modules = adr.make_decoder(norm_first)
    dec = asr.TransformerDecoder.from_torch(*modules)
    assert len(dec.layers) == adr.DEC["layers"] and dec.final_norm is not None
    hyps, utt, _ = dec_batch()
    T, B, eos = adr.DEC_T, len(adr.DEC_HYPS), V - 1
    mem = adr.draw_memory(T, B, E)
    d_mem = dm(adr.nan_past(mem, adr.DEC_ENC_LENGTHS).reshape(T * B, E))
    tin, tgt, ln = adr.teacher_forcing(hyps, eos, eos)
    ref_logp, ref_score = adr.decoder_ref(*modules, tin, tgt, ln, utt, mem, adr.DEC_ENC_LENGTHS)
    logp, Uq, N = dec.log_probs(tin, ln, utt, d_mem, T, B, adr.DEC_ENC_LENGTHS)
    asr.synchronize()
    got = logp.toCpu().reshape(Uq, N, V)
    mask = np.arange(Uq)[:, None] < np.asarray(ln)[None, :]
    close(got[mask], ref_logp[mask], f"decoder log-probs norm_first={norm_first}")
    score = dec.score(hyps, utt, d_mem, T, B, adr.DEC_ENC_LENGTHS)          # sos = eos = V - 1 by default
    err = np.abs(score - ref_score)
    print(f"decoder scores norm_first={norm_first}: max err {err.max():.3e}, bound "
          f"{adr.score_bound(Uq, ref_score).min():.3e}")
    assert np.all(err <= adr.score_bound(Uq, ref_score))
    # the device's gather of its own log-probs is exact
    assert np.array_equal(score, adr.token_score_ref(got, tgt, ln))
    assert dec.score([], [], d_mem, T, B).shape == (0,)


# -------------------------------------------------------- 6. end to end
def test_ctc_decoder_attention_rescore_end_to_end():
    """CTC beam search -> attention_rescore on the tiny random model of
    attention_decoder_reference.e2e_model (seed E2E_SEED): att against
    decoder_ref, exact_ctc against rescore(), the order wherever the float64
    totals are more than 100 x the score bound apart (every utterance at this
    seed); ctc_weight 0 gives att's order, ctc_weight 1 the order of att +
    rescore()'s exact score, and the CTC term alone rescore()'s own order."""
    c = adr.E2E
    T, B, V, E = c["T"], c["B"], c["V"], c["E"]
    emis, memory, modules = adr.e2e_model()
    dec = asr.TransformerDecoder.from_torch(*modules)
    d_mem = dm(memory.reshape(T * B, E))
    ctc = asr.CTCDecoder(V, c["beam"], 0)
    ctc.decode(emis)
    beams = ctc.beams(c["max_hyps"])
    assert all(len(u) == c["max_hyps"] for u in beams)
    ref_att, ref_ctc = adr.e2e_reference(beams, emis, memory, modules)
    nmax = max(len(h[0]) for u in beams for h in u) + 1
    exact = {(b, tuple(lab)): ex for b, u in enumerate(ctc.rescore(c["max_hyps"])) for lab, ex, _ in u}
    for w in adr.E2E_WEIGHTS:
        assert adr.smallest_gap_ratio(beams, ref_att, ref_ctc, w) > 1.0        # every utterance qualifies
        got = ctc.attention_rescore(c["max_hyps"], dec, d_mem, T, ctc_weight=w)
        k, worst = 0, 0.0
        for b, (u, rows) in enumerate(zip(beams, got)):
            want = {tuple(lab): (ref_att[k + j], ref_ctc[k + j]) for j, (lab, _) in enumerate(u)}
            k += len(u)
            assert sorted(tuple(r[0]) for r in rows) == sorted(want)
            for lab, total, att, ex in rows:
                ra, rc = want[tuple(lab)]
                worst = max(worst, abs(att - ra) / adr.score_bound(nmax, ra))
                assert abs(att - ra) <= adr.score_bound(nmax, ra), (b, lab, att, ra)
                assert ex == exact[(b, tuple(lab))] and abs(ex - rc) <= 1e-9 * abs(rc)
                assert total == att + w * ex
            order = [tuple(r[0]) for r in rows]
            assert order == sorted(want, key=lambda y: -(want[y][0] + w * want[y][1])), (b, w)
            if w == 0.0:        # the order of att alone
                assert order == [tuple(r[0]) for r in sorted(rows, key=lambda r: -r[2])]
            if w == 1.0:        # att + rescore()'s exact scores, unweighted
                assert order == [tuple(r[0]) for r in sorted(rows, key=lambda r: -(r[2] + exact[(b, tuple(r[0]))]))]
        print(f"attention_rescore ctc_weight {w}: max att err / score bound {worst:.3e}")
    # with att taken out, ctc_weight = 1 is rescore()'s order; the function form gives the method's rows
    resc = ctc.rescore(c["max_hyps"])
    zero = asr.attention_combine(beams, np.zeros(len(ref_att)), [exact[(b, tuple(h[0]))] for b, u in enumerate(beams)
                                                                  for h in u], 1.0)
    assert [[r[0] for r in u] for u in zero] == [[r[0] for r in u] for u in resc]
    fn = asr.attention_rescore(beams, dec, d_mem, T, B, ctc_scores=[[exact[(b, tuple(h[0]))] for h in u]
                                                                    for b, u in enumerate(beams)], ctc_weight=0.5)
    assert fn == ctc.attention_rescore(c["max_hyps"], dec, d_mem, T, ctc_weight=0.5)
    # an utterance with an empty beam gives []
    assert asr.attention_rescore([beams[0], [], beams[2]], dec, d_mem, T, B)[1] == []
    ctc.close()


# ------------------------------------------------ the forwards' shape checks
def test_forwards_refuse_buffers_smaller_than_the_call():
    """Every new forward checks rows and columns before any device call: a layer
    run over more rows than its input has raises ValueError."""
    E = adr.DEC["E"]
    _, dec, _ = adr.make_decoder(True)
    layer = asr.TransformerDecoderLayer.from_torch(dec.layers[0])
    ca = layer.cross_attn
    Uq, N, T, B = 4, 3, 5, 2
    x, mem = asr.DeviceMatrix(Uq * N, E), asr.DeviceMatrix(T * B, E)
    kv = ca.project_memory(mem, T, B)
    assert (kv.rows, kv.cols) == (T * B, 2 * E)
    off = [0, 2, 3]
    with pytest.raises(ValueError, match="project_memory: memory"):
        ca.project_memory(mem, T + 1, B)
    with pytest.raises(ValueError, match="CrossAttention.forward: x"):
        ca.forward(x, Uq + 1, N, kv, T, B, hyp_offsets=off)
    with pytest.raises(ValueError, match="CrossAttention.forward: kv"):
        ca.forward(x, Uq, N, kv, T, B + 1, hyp_offsets=off + [3])
    with pytest.raises(ValueError, match="kv"):
        ca.forward(x, Uq, N, mem, T, B, hyp_offsets=off)                  # E columns, not 2E
    with pytest.raises(ValueError, match="q_lengths"):
        ca.forward(x, Uq, N, kv, T, B, q_lengths=[1, 2], hyp_offsets=off)
    with pytest.raises(ValueError, match="hyp_offsets"):
        ca.forward(x, Uq, N, kv, T, B, hyp_offsets=[0, 3])
    with pytest.raises(ValueError, match="TransformerDecoderLayer.forward: x"):
        layer.forward(x, Uq, N + 1, kv, T, B, hyp_offsets=off)
    with pytest.raises(ValueError, match="TransformerDecoderLayer.forward: kv"):
        layer.forward(x, Uq, N, mem, T, B, hyp_offsets=off)
    with pytest.raises(ValueError, match="must not be x"):
        layer.forward(x, Uq, N, kv, T, B, hyp_offsets=off, out=x)
    modules = adr.make_decoder(True)
    d = asr.TransformerDecoder.from_torch(*modules)
    with pytest.raises(ValueError, match="memory"):
        d.score([[1, 2]], [0], mem, T + 1, B)
    with pytest.raises(ValueError, match="non-decreasing"):
        d.score([[1], [2]], [1, 0], mem, T, B)
    with pytest.raises(ValueError, match="token outside"):
        d.score([[1, 99]], [0], mem, T, B)
