"""CPU checks of attention-decoder rescoring (asr_cross_attention_fwd,
asr_token_score, asr.CrossAttention, asr.TransformerDecoderLayer,
asr.TransformerDecoder, asr.attention_rescore): exported, every refusal ahead of
any HIP call and in the documented order (the fake device pointers are never
dereferenced on the host), the float64 references of
attention_decoder_reference.py against torch in float64, the from_torch
packers (layouts, refusals, the toolkit stand-in), the Python shape checks, the
ordering and tie rule of the combination, and that the end-to-end case's seed
separates the totals of every utterance.  No GPU here."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import attention_decoder_reference as adr
from conftest import asr, oracle

NAMES = ["asr_cross_attention_fwd", "asr_token_score"]
FAKE = 0x10000   # a non-NULL, 16-byte aligned "device pointer"
INT_MAX = 2 ** 31 - 1
ARG, UNSUP = asr.ASR_ERR_ARG, asr.ASR_ERR_UNSUPPORTED


def xatt(heads=4, head_dim=16, scale=0.0, U=8, N=6, T=8, B=2, max_hyps=3, ld=None, lds=None, null=None):
    """asr_cross_attention_fwd with fake pointers; null: the pointer passed as NULL."""
    p = {"q": FAKE, "k": FAKE, "v": FAKE, "out": FAKE, "off": FAKE}
    if null in p:
        p[null] = None
    d = asr.XAttnDesc(heads, head_dim, scale)
    l4 = lds or (heads * head_dim if ld is None else ld,) * 4
    return asr.lib().asr_cross_attention_fwd(None if null == "desc" else ctypes.byref(d), p["q"], l4[0], p["k"],
                                             l4[1], p["v"], l4[2], FAKE, FAKE, p["off"], max_hyps, p["out"], l4[3],
                                             U, N, T, B, None)


def tsc(U=8, N=6, V=11, ld=None, logp=FAKE, tok=FAKE, out=FAKE):
    return asr.lib().asr_token_score(logp, V if ld is None else ld, tok, FAKE, out, U, N, V, None)


def test_symbols_in_mirror_and_library():
    for n in NAMES:
        assert n in asr.EXPORTS, n
        assert hasattr(asr.lib(), n), n
    out = subprocess.run(["nm", "-D", "--defined-only", str(asr.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    assert set(NAMES) <= set(re.findall(r" T (asr_[a-z0-9_]+)$", out, flags=re.M))


def test_desc_mirrors_the_header_struct():
    assert ctypes.sizeof(asr.XAttnDesc) == 3 * 4
    assert [f[0] for f in asr.XAttnDesc._fields_] == ["heads", "head_dim", "scale"]
    d = asr.xattn_desc(4, 36)
    assert (d.heads, d.head_dim, d.scale) == (4, 36, 0.0)


# --------------------------------------------------------------- refusals
@pytest.mark.parametrize("null", ["desc", "q", "k", "v", "out", "off"])
def test_cross_attention_err_arg_null(null):
    assert xatt(null=null) == ARG


@pytest.mark.parametrize("kw", [dict(U=0), dict(U=-1), dict(N=0), dict(N=-3), dict(T=0), dict(T=-5), dict(B=0),
                                dict(B=-2), dict(heads=0), dict(heads=-4, ld=64), dict(head_dim=0),
                                dict(head_dim=-16, ld=64), dict(max_hyps=0), dict(max_hyps=-1), dict(max_hyps=7),
                                dict(ld=63), dict(lds=(64, 63, 64, 64)), dict(lds=(64, 64, 0, 64)),
                                dict(lds=(64, 64, 64, -64)), dict(scale=-1.0), dict(scale=float("inf")),
                                dict(scale=float("nan"))],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_cross_attention_err_arg(kw):
    assert xatt(**kw) == ARG


@pytest.mark.parametrize("kw", [
    dict(head_dim=18), dict(head_dim=2), dict(head_dim=132), dict(heads=33, head_dim=128),     # E = 4224
    dict(heads=65536, head_dim=4, ld=2 ** 40), dict(B=65536),
    dict(U=1 << 20, N=1 << 12, max_hyps=1), dict(T=1 << 20, B=1 << 12),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_cross_attention_err_unsupported(kw):
    assert xatt(**kw) == UNSUP


def test_cross_attention_flat_query_bound():
    """U*max_hyps > INT_MAX - 64 is refused (a tile's last flat query 64 x + 63 stays an int)."""
    assert xatt(U=INT_MAX - 63, N=1, max_hyps=1) == UNSUP
    assert xatt(U=1 << 16, N=1 << 15, max_hyps=1 << 15) == UNSUP        # U*N = 2^31 as well


def test_cross_attention_refusals_in_order():
    assert xatt(head_dim=18, null="out") == ARG                    # NULL before unsupported
    assert xatt(head_dim=18, U=0) == ARG                           # sizes before unsupported
    assert xatt(head_dim=18, max_hyps=0) == ARG
    assert xatt(head_dim=18, max_hyps=7) == ARG                    # max_hyps > N
    assert xatt(heads=65536, head_dim=4, ld=8) == ARG              # the stride, before the grid limit
    assert xatt(head_dim=256, ld=1024, scale=float("nan")) == ARG  # the scale, before head_dim > 128
    assert xatt(U=INT_MAX, N=INT_MAX, B=70000, T=-1) == ARG
    assert xatt(B=65536, max_hyps=100) == ARG                      # max_hyps > N before the grid limit


def test_token_score_refusals_in_order():
    assert tsc(logp=None) == ARG
    assert tsc(tok=None) == ARG
    assert tsc(out=None) == ARG
    for kw in (dict(U=0), dict(U=-1), dict(N=0), dict(N=-2), dict(V=0), dict(V=-1, ld=4), dict(ld=10)):
        assert tsc(**kw) == ARG, kw
    assert tsc(U=1 << 20, N=1 << 12, ld=10) == ARG                 # both: ARG
    assert tsc(U=1 << 20, N=1 << 12) == UNSUP
    assert tsc(U=INT_MAX, N=INT_MAX) == UNSUP


# -------------------------------------------- the references against torch
def close64(got, ref):
    assert np.all(np.abs(got - ref) <= 1e-12 * (1 + np.abs(ref))), np.abs(got - ref).max()


@pytest.mark.parametrize("case", adr.XATTN_CASES[:4] + adr.XATTN_CASES[-1:], ids=lambda c: "x".join(map(str, c)))
def test_cross_attention_reference_equals_torch_on_repeated_memory(case):
    """torch.nn.MultiheadAttention in float64 with identity projections, the
    memory repeated per hypothesis (repeat_interleave) and a key-padding mask."""
    heads, D, T = case
    E = heads * D
    q, k, v = adr.draw_cross(heads, D, T)
    qlen, klen = adr.QLEN, adr.klen_for(T)
    ref = adr.cross_attention_ref(q, k, v, heads, adr.COUNTS, qlen, klen)
    mha = torch.nn.MultiheadAttention(E, heads, bias=False).double()
    with torch.no_grad():
        mha.in_proj_weight.copy_(torch.eye(E, dtype=torch.float64).repeat(3, 1))
        mha.out_proj.weight.copy_(torch.eye(E, dtype=torch.float64))
    utt = adr.utt_of(adr.COUNTS)
    counts = torch.tensor(adr.COUNTS)
    t64 = lambda a: torch.from_numpy(a.astype(np.float64))   # noqa: E731
    kr, vr = (torch.repeat_interleave(t64(a), counts, dim=1) for a in (k, v))
    live = [n for n in range(len(utt)) if klen[utt[n]] > 0]     # torch gives NaN for a fully masked row
    pad = torch.from_numpy(np.arange(T)[None, :] >= np.asarray(klen)[utt][:, None])
    with torch.no_grad():
        got, _ = mha(t64(q)[:, live], kr[:, live], vr[:, live], key_padding_mask=pad[live], need_weights=False)
    got = got.numpy()
    assert len(live) == 5
    for i, n in enumerate(live):
        close64(got[:qlen[n], i], ref[:qlen[n], n])
        assert not ref[qlen[n]:, n].any()
    for n in range(len(utt)):
        if n not in live:
            assert not ref[:, n].any()


def test_token_score_reference():
    logp = np.log(np.random.default_rng(0).uniform(0.1, 1, (3, 2, 5)))
    tok = np.array([[1, 4], [0, 9], [2, 2]])
    got = adr.token_score_ref(logp, tok, (3, 1))
    assert got[0] == (logp[0, 0, 1] + logp[1, 0, 0]) + logp[2, 0, 2] and got[1] == logp[0, 1, 4]
    assert adr.token_score_ref(logp, tok, (0, 2)).tolist() == [0.0, -np.inf]


def test_positional_encoding_is_the_toolkits():
    assert np.array_equal(asr.sinusoidal_positional_encoding(9, 32), adr.positional_encoding(9, 32).numpy())


@pytest.mark.parametrize("normalize_before", [True, False])
def test_toolkit_stand_in_equals_the_torch_layer(normalize_before):
    """The stand-in's forward is torch.nn.TransformerDecoderLayer's once the weights are copied over."""
    E, heads, F = adr.DEC["E"], adr.DEC["heads"], adr.DEC["F"]
    tk = adr.make_toolkit_layer(normalize_before)
    tl = torch.nn.TransformerDecoderLayer(E, heads, F, dropout=0.0, norm_first=normalize_before,
                                          layer_norm_eps=1e-12).eval()
    with torch.no_grad():
        for mha, att in ((tl.self_attn, tk.self_attn), (tl.multihead_attn, tk.src_attn)):
            mha.in_proj_weight.copy_(torch.cat([att.linear_q.weight, att.linear_k.weight, att.linear_v.weight]))
            mha.in_proj_bias.copy_(torch.cat([att.linear_q.bias, att.linear_k.bias, att.linear_v.bias]))
            mha.out_proj.load_state_dict(att.linear_out.state_dict())
        tl.linear1.load_state_dict(tk.feed_forward.w_1.state_dict())
        tl.linear2.load_state_dict(tk.feed_forward.w_2.state_dict())
        for a, b in ((tl.norm1, tk.norm1), (tl.norm2, tk.norm2), (tl.norm3, tk.norm3)):
            a.load_state_dict(b.state_dict())
    hyps = [y for u in adr.DEC_HYPS for y in u]
    utt = [b for b, u in enumerate(adr.DEC_HYPS) for _ in u]
    ln = [len(y) + 1 for y in hyps]
    x = np.random.default_rng(3).uniform(-1, 1, (13, len(hyps), E))
    mem = adr.draw_memory(adr.DEC_T, 3, E)
    a = adr.layer_ref(tk, x, ln, utt, mem, adr.DEC_ENC_LENGTHS)
    b = adr.layer_ref(tl, x, ln, utt, mem, adr.DEC_ENC_LENGTHS)
    for n, m in enumerate(ln):
        assert np.all(np.abs(a[:m, n] - b[:m, n]) <= 1e-11 * (1 + np.abs(b[:m, n])))


# ---------------------------------------------------------------- packing
def test_pack_cross_attention_from_torch():
    torch.manual_seed(1)
    E, H = 24, 2
    mha = torch.nn.MultiheadAttention(E, H)
    with torch.no_grad():
        mha.in_proj_bias.uniform_(-0.1, 0.1)
        mha.out_proj.bias.uniform_(-0.1, 0.1)
    w_q, b_q, w_kv, b_kv, w_out, b_out = asr.CrossAttention.pack_torch(mha)
    assert (w_q.shape, b_q.shape, w_kv.shape, b_kv.shape, w_out.shape, b_out.shape) == (
        (E, E), (E,), (E, 2 * E), (2 * E,), (E, E), (E,))
    assert all(a.dtype == np.float32 and a.flags.c_contiguous for a in (w_q, b_q, w_kv, b_kv, w_out, b_out))
    x = torch.randn(5, E)
    qkv = torch.nn.functional.linear(x, mha.in_proj_weight, mha.in_proj_bias).detach().numpy()
    assert np.allclose(x.numpy() @ w_q + b_q, qkv[:, :E], atol=1e-5)
    assert np.allclose(x.numpy() @ w_kv + b_kv, qkv[:, E:], atol=1e-5)
    assert np.allclose(x.numpy() @ w_out + b_out, mha.out_proj(x).detach().numpy(), atol=1e-5)


def test_cross_attention_refusals_are_multihead_attentions():
    pack = asr.CrossAttention.pack_torch
    with pytest.raises(ValueError, match="kdim"):
        pack(torch.nn.MultiheadAttention(24, 2, kdim=16, vdim=24))
    with pytest.raises(ValueError, match="bias_k"):
        pack(torch.nn.MultiheadAttention(24, 2, add_bias_kv=True))
    with pytest.raises(ValueError, match="add_zero_attn"):
        pack(torch.nn.MultiheadAttention(24, 2, add_zero_attn=True))
    for E, H in ((36, 6), (18, 1), (1024, 4)):
        with pytest.raises(ValueError, match="head_dim"):
            asr.CrossAttention(E, H)
    with pytest.raises(ValueError, match="embed_dim"):
        asr.CrossAttention(4224, 33)


def test_pack_linears_of_the_toolkit_stand_in():
    tk = adr.make_toolkit_layer(True)
    a = tk.src_attn
    w_q, b_q, w_kv, b_kv, w_out, b_out = asr.CrossAttention.pack_linears(a.linear_q, a.linear_k, a.linear_v,
                                                                         a.linear_out)
    E = adr.DEC["E"]
    x = torch.randn(5, E)
    assert np.allclose(x.numpy() @ w_q + b_q, a.linear_q(x).detach().numpy(), atol=1e-5)
    assert np.allclose(x.numpy() @ w_kv[:, :E] + b_kv[:E], a.linear_k(x).detach().numpy(), atol=1e-5)
    assert np.allclose(x.numpy() @ w_kv[:, E:] + b_kv[E:], a.linear_v(x).detach().numpy(), atol=1e-5)
    assert np.allclose(x.numpy() @ w_out + b_out, a.linear_out(x).detach().numpy(), atol=1e-5)
    with pytest.raises(ValueError, match="E -> E"):
        asr.CrossAttention.pack_linears(a.linear_q, torch.nn.Linear(E, 2 * E), a.linear_v, a.linear_out)


def test_decoder_layer_refusals():
    mk = torch.nn.TransformerDecoderLayer
    with pytest.raises(ValueError, match="gelu"):
        asr.TransformerDecoderLayer.from_torch(mk(16, 2, 32, activation="gelu"))
    with pytest.raises(ValueError, match="ReLU only"):
        asr.TransformerDecoderLayer.from_torch(mk(16, 2, 32, activation=torch.nn.SiLU()))
    with pytest.raises(ValueError, match="head_dim"):
        asr.TransformerDecoderLayer.from_torch(mk(36, 6, 32))


# ----------------------------------------------------- Python shape checks
class Buf:
    """A stand-in for a device matrix: the shape checks run before any device call."""

    def __init__(self, rows, cols):
        self.ptr, self.rows, self.cols = FAKE, rows, cols


def test_cross_attention_fwd_shape_checks_raise():
    d = asr.xattn_desc(2, 8)
    U, N, T, B, E = 4, 3, 5, 2, 16
    ok = dict(q=Buf(U * N, E), k=Buf(T * B, E), v=Buf(T * B, E), out=Buf(U * N, E))
    for name, bad in (("q", Buf(U * N - 1, E)), ("k", Buf(T * B - 1, E)), ("v", Buf(T * B, E - 1)),
                      ("out", Buf(U * N, E - 4))):
        a = dict(ok, **{name: bad})
        with pytest.raises(ValueError, match=f"cross_attention_fwd: {name}"):
            asr.cross_attention_fwd(a["q"], a["k"], a["v"], a["out"], U, N, T, B, d, [0, 2, 3], 2)
    kv = Buf(T * B, 2 * E)
    with pytest.raises(ValueError, match="cross_attention_fwd: v"):      # V's columns would run past the row
        asr.cross_attention_fwd(ok["q"], asr.ColumnView(kv, 0), asr.ColumnView(kv, E + 4), ok["out"], U, N, T, B, d,
                                [0, 2, 3], 2)
    with pytest.raises(ValueError, match="hyp_offsets"):
        asr.cross_attention_fwd(ok["q"], ok["k"], ok["v"], ok["out"], U, N, T, B, d, [0, 3], 2)
    with pytest.raises(ValueError, match="hyp_offsets"):
        asr.cross_attention_fwd(ok["q"], ok["k"], ok["v"], ok["out"], U, N, T, B, d, None, 2)


def test_token_score_shape_checks_raise():
    with pytest.raises(ValueError, match="token_score: logp"):
        asr.token_score(Buf(11, 5), np.zeros((4, 3), int), None, 4, 3, 5)
    with pytest.raises(ValueError, match="tokens"):
        asr.token_score(Buf(12, 5), np.zeros((4, 2), int), None, 4, 3, 5)
    with pytest.raises(ValueError, match="lengths"):
        asr.token_score(Buf(12, 5), np.zeros((4, 3), int), [1, 2], 4, 3, 5)


def test_decoder_grouping_and_teacher_forcing():
    off, mh = asr.TransformerDecoder._group([0, 0, 2, 2, 2], 4)
    assert off.tolist() == [0, 2, 2, 5, 5] and mh == 3
    with pytest.raises(ValueError, match="non-decreasing"):
        asr.TransformerDecoder._group([0, 2, 1], 3)
    with pytest.raises(ValueError, match="non-decreasing"):
        asr.TransformerDecoder._group([0, 3], 3)
    hyps = [[1, 2], [], [3]]
    tin, tgt, ln = asr.TransformerDecoder.teacher_forcing(hyps, 9, 8)
    rin, rgt, rln = adr.teacher_forcing(hyps, 9, 8)
    assert np.array_equal(tin, rin) and np.array_equal(tgt, rgt) and ln.tolist() == rln.tolist() == [3, 1, 2]
    assert tin[:, 0].tolist() == [9, 1, 2] and tgt[:, 0].tolist() == [1, 2, 8] and tgt[0, 1] == 8


# ------------------------------------------------- ordering and the tie rule
def test_attention_combine_orders_by_total_and_keeps_ties_in_beam_order():
    nbest = [[([1], -1.0), ([2], -2.0), ([3], -3.0), ([4], -4.0)], [], [([5], -0.5)]]
    att = [-4.0, -2.0, -3.0, -1.0, -7.0]
    ctc = [-1.0, -2.0, -1.0, -3.0, -0.5]
    out = asr.attention_combine(nbest, att, ctc, 0.5)
    assert out[1] == [] and out[2] == [([5], -7.25, -7.0, -0.5)]
    # totals: -4.5, -3.0, -3.5, -2.5
    assert [r[0] for r in out[0]] == [[4], [2], [3], [1]]
    assert [r[1] for r in out[0]] == [-2.5, -3.0, -3.5, -4.5]
    assert out[0][0] == ([4], -2.5, -1.0, -3.0)
    # weight 0: att's order; weight 1 with equal totals: the beam order stays
    assert [r[0] for r in asr.attention_combine(nbest, att, ctc, 0.0)[0]] == [[4], [2], [3], [1]]
    tie = asr.attention_combine([[([1], 0), ([2], 0), ([3], 0)]], [-2.0, -1.0, -2.0], [-1.0, -2.0, -1.0], 1.0)
    assert [r[0] for r in tie[0]] == [[1], [2], [3]] and {r[1] for r in tie[0]} == {-3.0}


def test_attention_rescore_checks_its_arguments_and_takes_an_empty_nbest():
    assert asr.attention_rescore([[], []], None, None, 5, 2) == [[], []]
    with pytest.raises(ValueError, match="n-best lists"):
        asr.attention_rescore([[]], None, None, 5, 2)
    with pytest.raises(ValueError, match="ctc_scores"):
        asr.attention_rescore([[([1], -1.0)], []], None, None, 5, 2, ctc_scores=[[], []])


# ------------------------------------------------- the end-to-end case's seed
def test_e2e_seed_separates_every_utterances_totals():
    """With the oracle's n-best and the float64 references alone: at seed
    E2E_SEED every utterance has a full beam and neighbouring totals more than
    100 x the score bound apart at every ctc_weight of the GPU test."""
    c = adr.E2E
    emis, memory, modules = adr.e2e_model()
    nbest = oracle.decode(emis, c["beam"], 0, max_hyps=c["max_hyps"])
    assert all(len(u) == c["max_hyps"] for u in nbest)
    att, ctc = adr.e2e_reference(nbest, emis, memory, modules)
    assert np.all(np.isfinite(att)) and np.all(np.isfinite(ctc))
    for w in adr.E2E_WEIGHTS:
        ratio = adr.smallest_gap_ratio(nbest, att, ctc, w)
        print(f"seed {adr.E2E_SEED} ctc_weight {w}: smallest gap / (100 x bound) = {ratio:.2f}")
        assert ratio > 1.0, (w, ratio)
