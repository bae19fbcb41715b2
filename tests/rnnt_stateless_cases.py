"""The stateless-transducer test cases shared by tests/test_rnnt_stateless_cpu.py
and _gpu.py, in the manner of rnnt_cases.py: fixed seeds (searched for on the CPU
until the conditions on the reference held; one that breaks them fails the
test), W_out scaled and b_out[blank] set so that the walks mix their paths.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

import rnnt_beam_cases as rbc
import rnnt_cases as rc
import rnnt_lm_cases as lc
from rnnt_stateless_reference import (StatelessAlignReference, StatelessBeamReference, StatelessLmBeamReference,
                                      StatelessReference)

# shape = (T, B, E, D, Hp, J, V); context 1 with conv False: no W_ctx (D = Hp); groups > 0: a block-diagonal W_ctx,
# the decoder made by from_icefall from a grouped stand-in conv; fill_blank: start_fill = blank, else -1
Case = namedtuple("Case", "name shape blank max_symbols act lengths seed out_scale blank_bias context conv bias "
                          "groups fill_blank")


def _c(name, shape, blank_last, ms, act, lengths, seed, blank_bias, context, conv=True, bias=True, groups=0,
       fill_blank=False):
    return Case(name, shape, shape[6] - 1 if blank_last else 0, ms, act, tuple(lengths), seed, 4.0, blank_bias,
                context, conv, bias, groups, fill_blank)


ONE = (1, 1, 8, 16, 16, 16, 2)            # one k chunk, below the ring depth
RAGGED = (9, 5, 24, 16, 48, 32, 17)       # a partial row tile, a zero length, a partial last V tile
TILES = (6, 17, 16, 16, 16, 16, 17)       # a second workgroup with one row
MIXED = (6, 3, 8, 32, 16, 448, 437)       # 28 column tiles: four-tile products and single tiles; the blank in the last
LIMIT = (3, 2, 16, 16, 1232, 1232, 17)    # the documented LDS limit's Hp = J
L17 = [6, 0, 3, 6, 5, 6, 2, 6, 6, 1, 6, 4, 6, 6, 0, 6, 6]
CASES = [
    _c("one-c1", ONE, False, 1, "relu", [1], 0, 0.0, 1, conv=False, bias=False),
    _c("one-c2", ONE, True, 3, "tanh", [1], 1, 0.0, 2, fill_blank=True),
    _c("ragged-c2", RAGGED, False, 3, "tanh", rc.L2, 4, 2.0, 2, bias=False),
    _c("ragged-c3-grouped", RAGGED, True, 1, "relu", rc.L2, 8, 2.0, 3, groups=4, fill_blank=True),
    _c("tiles-c1", TILES, False, 3, "relu", L17, 11, 5.0, 1, conv=False),
    _c("mixed-c2", MIXED, True, 3, "relu", [6, 0, 4], 9, 8.0, 2),
    _c("limit-c2", LIMIT, False, 1, "tanh", [3, 2], 0, 2.0, 2, bias=False),
]
# beam only: K = 16 (an utterance fills the 16-row tile: every context is permuted by parent row), and the LM case
CASES += [_c("wide-c2", RAGGED, False, 1, "relu", [3, 0, 2, 3, 1], 16, 2.0, 2, fill_blank=True),
          _c("lm-c2", RAGGED, False, 1, "relu", rc.L2, 33, 2.0, 2)]
GREEDY_CASES = CASES[:-2]
BEAMS = [("ragged-c2", 1), ("ragged-c2", 3), ("ragged-c3-grouped", 4), ("tiles-c1", 4), ("mixed-c2", 4),
         ("wide-c2", 16)]
# a trigram over the 16 labels fused at alpha = beta = 0.5 with <s>, K = 4 (rnnt_lm_cases' a-k4 on this predictor)
LM_CASE = lc.LmCase("lm-c2", None, 4, lc.TRI16, True, False, 0.5, 0.5, ())
ALIGN_SPEC = {"ragged-c2": [(0, 3), (2, 0), (3, 5), (4, 2), (1, 0)], "mixed-c2": [(0, 4), (2, 1)]}


def by_name(name):
    return next(c for c in CASES if c.name == name)


def make_model(case):
    """(weights dict of float32 arrays in [in][out] layout, None where the model has none; enc [T, B, E])."""
    T, B, E, D, Hp, J, V = case.shape
    gen = torch.Generator().manual_seed(case.seed)
    C = case.context
    w = {"emb": rc._uniform(gen, (V, D), 1.0), "w_ctx": None, "b_ctx": None}
    if case.conv:
        w["w_ctx"] = rc._uniform(gen, (C, D, Hp), (3.0 / (D * C)) ** 0.5 * 2.0)
        if case.groups:     # block-diagonal: the channels of a group see only their own
            g = case.groups
            mask = np.kron(np.eye(g, dtype=np.float32), np.ones((D // g, Hp // g), np.float32))
            w["w_ctx"] = w["w_ctx"] * mask
    if case.bias:
        w["b_ctx"] = rc._uniform(gen, (Hp,), 0.1)
    w["w_enc"], w["b_enc"] = rc._uniform(gen, (E, J), (3.0 / E) ** 0.5), rc._uniform(gen, (J,), 0.1)
    w["w_pred"], w["b_pred"] = rc._uniform(gen, (Hp, J), (3.0 / Hp) ** 0.5 * 4.0), rc._uniform(gen, (J,), 0.1)
    w["w_out"] = rc._uniform(gen, (J, V), (3.0 / J) ** 0.5 * case.out_scale)
    w["b_out"] = rc._uniform(gen, (V,), 0.1)
    w["b_out"][case.blank] = case.blank_bias
    return w, rc._uniform(gen, (T, B, E), 1.0)


def start_fill(case):
    return case.blank if case.fill_blank else -1


def _ref(cls, case, w, ms):
    return cls(w, case.blank, case.act, ms, case.context, start_fill(case))


@functools.lru_cache(maxsize=None)
def reference(case):
    """(weights, enc, the reference's greedy decode), computed once and not to be changed."""
    w, enc = make_model(case)
    return w, enc, _ref(StatelessReference, case, w, case.max_symbols).decode(enc, case.lengths)


@functools.lru_cache(maxsize=None)
def beam_reference(name, beam):
    case = by_name(name)
    w, enc = make_model(case)
    return case, w, enc, _ref(StatelessBeamReference, case, w, 1).search(enc, case.lengths, beam=beam)


@functools.lru_cache(maxsize=None)
def align_reference(name, topology):
    """Targets: the first U labels of a long greedy walk of the utterance (likely labels keep the lattice's
    decisions clear of rounding), as rnnt_align_cases' greedy cases do."""
    case = by_name(name)
    w, enc = make_model(case)
    ref = _ref(StatelessAlignReference, case, w, 24)
    walk = ref.decode(enc, case.lengths)
    utt = [b for b, _u in ALIGN_SPEC[name]]
    targets = [list(walk["tokens"][b][:U]) for b, U in ALIGN_SPEC[name]]
    assert all(len(t) == U for t, (_b, U) in zip(targets, ALIGN_SPEC[name])), name
    return case, w, enc, targets, utt, ref.align(enc, targets, case.lengths, utt, topology)


@functools.lru_cache(maxsize=None)
def lm_reference():
    """(LmCase with the model filled in, weights, enc, the reference's fused search), computed once."""
    case = LM_CASE._replace(model=by_name(LM_CASE.name))
    w, enc = make_model(case.model)
    r = _ref(StatelessLmBeamReference, case.model, w, 1)
    r.lm_setup(lc.lm_model(case), lc.tok_of_label(case), case.alpha, case.beta, lc.flags_of(case), case.lm[5])
    ref = r.search_lm(enc, case.model.lengths, beam=case.beam)
    lc.check_conditions(case._replace(name="sl-" + case.name), ref)      # the margins, and a merge
    return case, w, enc, ref


def check_chunked(decode, case, enc):
    """decode(enc, lengths, state) -> (results, context, counts): cut at frame 4 with the context carried equals the
    whole decode, bit for bit."""
    ln = lengths_of(case)
    whole, wctx, wcnt = decode(enc, ln, None)
    a, ctx, ca = decode(enc[:4], np.minimum(ln, 4), None)
    b, ctx, cb = decode(enc[4:], np.maximum(ln - 4, 0), ctx)
    assert np.array_equal(ctx, wctx) and (ca + cb).tolist() == wcnt.tolist() and int(cb.sum()) > 0
    for u, x, y in zip(whole, a, b):
        assert u[0] == x[0] + y[0] and u[1] == x[1] + [t + 4 for t in y[1]]
        assert np.array_equal(u[2], np.concatenate([x[2], y[2]]))


def check_beam_conditions(name, beam, ref):
    """Every decision margin of the reference's search is at least 1e-3 * (1 + max |logit|)."""
    assert min(ref["margin"]) >= rbc.margin_bound(ref), (name, beam, min(ref["margin"]), ref["max_abs_logit"])


def standin(case, w):
    """Stand-in modules with icefall's attribute names, holding the case's weights."""
    T, B, E, D, Hp, J, V = case.shape
    C, g = case.context, max(case.groups, 1)
    dec, joi = torch.nn.Module(), torch.nn.Module()
    dec.context_size, dec.blank_id = C, case.blank
    dec.embedding = torch.nn.Embedding(V, D, padding_idx=case.blank if case.fill_blank else None)
    dec.embedding.weight.data = torch.from_numpy(w["emb"]).clone()
    if case.conv:
        dec.conv = torch.nn.Conv1d(D, Hp, C, groups=g, bias=case.bias)
        cw = np.zeros((Hp, D // g, C), np.float32)
        for gi in range(g):
            blk = w["w_ctx"][:, gi * (D // g):(gi + 1) * (D // g), gi * (Hp // g):(gi + 1) * (Hp // g)]
            cw[gi * (Hp // g):(gi + 1) * (Hp // g)] = blk.transpose(2, 1, 0)
        dec.conv.weight.data = torch.from_numpy(cw)
        if case.bias:
            dec.conv.bias.data = torch.from_numpy(w["b_ctx"]).clone()
    for name, key, shape in (("encoder_proj", "enc", (E, J)), ("decoder_proj", "pred", (Hp, J)),
                             ("output_linear", "out", (J, V))):
        lin = torch.nn.Linear(*shape)
        lin.weight.data = torch.from_numpy(np.ascontiguousarray(w["w_" + key].T))
        lin.bias.data = torch.from_numpy(w["b_" + key]).clone()
        setattr(joi, name, lin)
    return dec, joi


def make_decoder(asr, case, w=None):
    T, B, E, D, Hp, J, V = case.shape
    if w is None:
        w = make_model(case)[0]
    if case.groups:
        return asr.TransducerDecoder.from_icefall(*standin(case, w), activation=case.act,
                                                  max_symbols=case.max_symbols)
    return asr.TransducerDecoder.stateless(
        asr.rnnt_stateless_desc(V, case.blank, E, D, Hp, J, case.act, case.max_symbols, case.context,
                                start_fill(case)), w)


def lengths_of(case):
    return np.asarray(case.lengths, np.int32)
