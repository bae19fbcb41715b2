"""The cases of the LM-fused transducer beam search shared by
tests/test_rnnt_lm_cpu.py and tests/test_rnnt_lm_gpu.py: rnnt_cases' random
models and lm_reference's random ARPA models, both from fixed seeds, their
float64 reference searches (computed once per process, not to be changed) and
the conditions each case and the suite must meet on the reference before
anything is compared with it.

The seeds were searched for on the CPU with the reference alone (model seeds
0..199 per case; about one in ten qualifies at V = 17, and seed 165 alone of
the sixty tried at V = 1025 has both the margin and a merge) and pinned; nothing is drawn again at run time, and
a seed that breaks a condition fails the test.
"""
import functools
from collections import namedtuple

import numpy as np

import rnnt_cases as rc
from lm_reference import BOS, EOS, ArpaModel, random_arpa, windowed_arpa
from rnnt_beam_reference import BeamReference
from rnnt_lm_reference import LmBeamReference

# lm = (order, n-grams of order 2.., ordinary tokens, <unk> present, seed, oov_log10); oov: labels mapped to -1
LmCase = namedtuple("LmCase", "name model beam lm bos eos alpha beta oov")
C640 = (12, 5, 64, 640, 640, 640, 1025, 1)


def _l(name, shape, act, lengths, seed, blank_bias, beam, lm, bos, eos, alpha, beta, oov=()):
    return LmCase(name, rc.Case(name, shape, 0, 1, act, tuple(lengths), seed, 4.0, blank_bias), beam, lm, bos, eos,
                  alpha, beta, tuple(oov))


TRI16 = (3, (40, 60), 16, False, 7, -100.0)           # a trigram over the 16 labels
FOUR32 = (4, (80, 80, 80), 32, False, 11, -1.0)      # a 4-gram, no <unk>: a mild OOV value, so that OOVs are kept
FOUR32U = (4, (80, 80, 80), 32, True, 11, -100.0)      # the same draw with <unk>
BI16 = (2, (60,), 16, False, 5, -100.0)
TRI1024 = (3, (3000, 3000), 1024, False, 3, -100.0)    # sparse: almost every lookup backs off

SMALL_CASES = [
    _l("a-k2", rc.S2, "relu", rc.L2, 20, 2.0, 2, TRI16, True, False, 0.5, 0.5),
    _l("a-k4", rc.S2, "relu", rc.L2, 4, 2.0, 4, TRI16, True, False, 0.5, 0.5),
    _l("a-k8", rc.S2, "relu", rc.L2, 12, 2.0, 8, TRI16, True, False, 0.5, 0.5),
    _l("b-k4", rc.S3, "tanh", rc.L3, 2, 3.0, 4, FOUR32, False, True, 0.4, 0.3, (5, 9)),
    _l("b-k4-unk", rc.S3, "tanh", rc.L3, 1, 3.0, 4, FOUR32U, False, True, 0.4, 0.3, (5, 9)),
]
# GPU only (the twin and the reference run them too): R = 16, and R = 8 with three dead rows
WIDE_CASES = [
    _l("c-k16", rc.S2, "relu", [3, 0, 2, 3, 1], 4, 2.0, 16, BI16, True, False, 0.5, 0.5),
    _l("d-k5", rc.S2, "relu", rc.L2, 29, 2.0, 5, TRI16, True, False, 0.5, 0.5),
]
# The LDS limit, V no multiple of 16, the LM rows at their upper shape.
UPPER_CASES = [
    _l("e-c640-k4", C640, "relu", [12, 0, 7, 12, 9], 165, 6.0, 4, TRI1024, True, False, 0.3, 0.5),
]
UPPER_NEEDS_MERGE = {"e-c640-k4": True}


def _o(name, shape, blank, act, lengths, seed, blank_bias, beam, lm, bos, eos, alpha, beta, oov=()):
    return LmCase(name, rc.Case(name, shape, blank, 1, act, tuple(lengths), seed, 4.0, blank_bias), beam, lm, bos, eos,
                  alpha, beta, tuple(oov))


TRI436 = (3, (1500, 1500), 436, False, 3, -100.0)      # sparse over MIXED's 436 labels
BI2 = (2, (4,), 2, False, 5, -100.0)                   # a bigram over the two labels of the V = 3 shape
# order 8 over 16 tokens: a seventh field makes lm_text build the model from the windows of the case's own unfused
# K-best (lm_reference.windowed_arpa), with (30,) * 7 random n-grams beside them
O8 = (8, (30,) * 7, 16, False, 21, -100.0, "windows")
V3 = (6, 3, 8, 16, 16, 16, 3, 1)
S12 = (12, 3, 24, 16, 48, 32, 17, 1)
# The options the cases above leave alone: the blank in the middle and at V - 1, both flags together and neither,
# beta < 0, alpha = 0, beta = 0, K > V, and an order-8 model whose context is cut to its last seven tokens.  Model
# seeds 0..199 were tried per case with the reference alone; the first that meets the margin, a merge and the case's
# own condition (check_option) is pinned.  Of the 200 the margin holds at 78 (f-bl-k4), 26 (f-bm-k8), 88, 101, 38,
# 101, 121 (f-mixed, 33 with a kept label >= 432), 143 (f-v3) and 100 (f-o8, 58 with its four conditions; at a blank
# bias of 1.0 instead of 0.0: 117 and 45).  No merge condition was waived.
OPTION_CASES = [
    _o("f-bl-k4", rc.S2, 16, "relu", rc.L2, 3, 2.0, 4, TRI16, True, False, 0.5, 0.5),
    _o("f-bm-k8", rc.S2, 8, "relu", rc.L2, 5, 2.0, 8, TRI16, True, True, 0.5, 0.5),
    _o("f-s3-bl", rc.S3, 32, "tanh", rc.L3, 4, 3.0, 4, FOUR32U, False, False, 0.4, 0.3, (5, 9)),
    _o("f-neg", rc.S2, 0, "relu", rc.L2, 4, 2.0, 4, TRI16, True, False, 0.5, -0.7),
    _o("f-a0", rc.S2, 0, "relu", rc.L2, 13, 2.0, 4, TRI16, True, False, 0.0, 0.6),
    _o("f-b0", rc.S2, 16, "relu", rc.L2, 0, 2.0, 4, TRI16, False, True, 0.5, 0.0),
    _o("f-mixed", rc.MIXED, 436, "relu", [6, 0, 4], 62, 6.0, 4, TRI436, True, False, 0.3, 0.5),
    _o("f-v3", V3, 2, "relu", [6, 0, 4], 0, 1.0, 16, BI2, True, True, 0.5, 0.5),
    _o("f-o8", S12, 0, "relu", [12, 0, 10], 29, 0.0, 4, O8, True, True, 0.5, 0.5),
]
OPTION_NEEDS_MERGE = {c.name: True for c in OPTION_CASES}


@functools.lru_cache(maxsize=None)
def lm_text(case):
    order, ngrams, vocab, unk, seed, _oov = case.lm[:6]
    if len(case.lm) > 6:     # the windows of the case's own unfused K-best, as LM tokens (the indices of w0..)
        w, enc = rc.make_model(case.model)
        plain = BeamReference(w, case.model.blank, case.model.act, 1).search(enc, case.model.lengths, beam=case.beam)
        seqs = [[_w_index(case, y) for y in ys] for u in plain["hyps"] for ys, _ts, _s in u]
        return windowed_arpa(np.random.default_rng(seed), vocab, order, seqs, list(ngrams))
    return random_arpa(np.random.default_rng(seed), vocab, order, list(ngrams), bos=True, eos=True, unk=unk)


def _w_index(case, v):
    """Label v is the model's token w<this>: the non-blank labels in label order."""
    return v - (1 if v > case.model.blank else 0)


@functools.lru_cache(maxsize=None)
def lm_model(case):
    return ArpaModel(lm_text(case))


def flags_of(case):
    return (BOS if case.bos else 0) | (EOS if case.eos else 0)


@functools.lru_cache(maxsize=None)
def tok_of_label(case):
    """The blank and the labels in case.oov map to -1, the other labels to the model's tokens w0, w1, ... in label
    order (an OOV label keeps its place in the count): with the blank at 0, label v > 0 is w(v-1)."""
    m = lm_model(case)
    V = case.model.shape[6]
    return tuple(-1 if v == case.model.blank or v in case.oov else m.ids["w%d" % _w_index(case, v)] for v in range(V))


@functools.lru_cache(maxsize=None)
def reference(case):
    """(weights, enc, the reference's fused search, its unfused search), computed once and not to be changed."""
    w, enc = rc.make_model(case.model)
    r = LmBeamReference(w, case.model.blank, case.model.act, 1)
    r.lm_setup(lm_model(case), tok_of_label(case), case.alpha, case.beta, flags_of(case), case.lm[5])
    ref = r.search_lm(enc, case.model.lengths, beam=case.beam)
    plain = BeamReference(w, case.model.blank, case.model.act, 1).search(enc, case.model.lengths, beam=case.beam)
    return w, enc, ref, plain


def margin_bound(ref):
    """The project's near-tie bound: 1e-3 * (1 + max |logit|)."""
    return 1e-3 * (1.0 + ref["max_abs_logit"])


def rescored_best(case, w, plain):
    """Per utterance the best tokens of the unfused K-best re-ranked by total = am + W (+ the </s> term)."""
    r = LmBeamReference(w, case.model.blank, case.model.act, 1)
    r.lm_setup(lm_model(case), tok_of_label(case), case.alpha, case.beta, flags_of(case), case.lm[5])
    best = []
    for u in plain["hyps"]:
        rows = []
        for ys, _ts, am in u:
            L = sum(r._value(tuple(ys[:i + 1]))[0] for i in range(len(ys)))
            total = am + r.aln10 * L + r.beta * len(ys)
            if case.eos:
                total += r.aln10 * r._value(tuple(ys), eos=True)[0]
            rows.append((total, ys))
        best.append(max(rows, key=lambda x: x[0])[1] if rows else None)
    return best


def facts(case):
    """What the suite-level conditions count, from the reference alone."""
    w, _enc, ref, plain = reference(case)
    fused_best = [u[0][0] if u else None for u in ref["hyps"]]
    plain_best = [u[0][0] if u else None for u in plain["hyps"]]
    return {"deep": ref["deep_merges"], "short": ref["short_frames"], "backoffs": dict(ref["backoffs"]),
            "oov": ref["oov"], "vs_plain": sum(a != b for a, b in zip(fused_best, plain_best)),
            "vs_rescore": sum(a != b for a, b in zip(fused_best, rescored_best(case, w, plain)))}


def check_conditions(case, ref, need_merge=True):
    """Asserted on the reference alone: every decision margin (over fused scores
    and totals) is at least the bound, and for K >= 2 the search merged."""
    assert min(ref["margin"]) >= margin_bound(ref), (case.name, min(ref["margin"]), ref["max_abs_logit"])
    if case.beam >= 2 and need_merge:
        assert ref["merges"] >= 1, case.name
    if case.name.startswith("a-"):     # lookups that back off by one and by two orders
        assert ref["backoffs"].get(1, 0) >= 1 and ref["backoffs"].get(2, 0) >= 1, (case.name, ref["backoffs"])
    if case.oov:
        assert ref["oov"] >= 1, case.name


def check_option(case):
    """The option case's own condition, asserted on the reference alone, after check_conditions."""
    _w, _enc, ref, plain = reference(case)
    V, K, name = case.model.shape[6], case.beam, case.name
    if name == "f-bl-k4":      # lookups that back off by one and by two orders
        assert ref["backoffs"].get(1, 0) >= 1 and ref["backoffs"].get(2, 0) >= 1, ref["backoffs"]
    if name == "f-bm-k8":      # the </s> term reorders a final list, and within its first two
        assert any(r[:2] != [0, 1] for r in ref["pre_eos_rank"] if len(r) >= 2), ref["pre_eos_rank"]
    if name == "f-neg":        # the fused best is not the unfused best
        assert any(f and f[0][0] != u[0][0] for f, u in zip(ref["hyps"], plain["hyps"]))
    if name == "f-a0":         # alpha = 0: any other model over the same tokens gives the same search
        other = reference(case._replace(lm=BI16))[2]
        assert [[(h[0], h[1], h[2], h[5]) for h in u] for u in other["hyps"]] == \
            [[(h[0], h[1], h[2], h[5]) for h in u] for u in ref["hyps"]]
        assert any(h[4] != o[4] for u, v in zip(ref["hyps"], other["hyps"]) for h, o in zip(u, v))   # not the same LM
    if name == "f-mixed":      # a kept label in the partial last column tile, beside the blank
        assert any(432 <= v < V and v != case.model.blank for v in ref["kept_labels"]), sorted(ref["kept_labels"])
    if name == "f-v3":
        assert V < K and ref["short_frames"] >= 1
    if name == "f-o8":
        assert lm_model(case).order == 8
        assert ref["max_len"] >= 9                  # a context was cut to its last 7 tokens
        assert ref["max_order"] == 8                # a lookup answered at order 8, without backing off
        assert ref["full_ctx_backoffs"] >= 1        # a lookup that backed off from a 7-token context
        assert ref["eos_full_ctx"] >= 1             # a final hypothesis's </s> term looked up with a full context


def check_suite(cases):
    """Over the cases: a deep merge, a frame short of K, a backed-off lookup, an
    OOV, an utterance whose fused best is not the unfused best, and one whose
    fused best is not the best of the re-ranked unfused K-best (what fusion is
    for)."""
    fs = [facts(c) for c in cases]
    assert any(f["deep"] >= 1 for f in fs)
    assert any(f["short"] >= 1 for f in fs)
    assert any(sum(f["backoffs"].values()) >= 1 for f in fs)
    assert any(f["oov"] >= 1 for f in fs)
    assert any(f["vs_plain"] >= 1 for f in fs)
    assert any(f["vs_rescore"] >= 1 for f in fs)


def make_decoder(asr, case, w=None):
    return rc.make_decoder(asr, case.model, w)


def make_lm(asr, case):
    return asr.NGramLM.from_string(lm_text(case), oov_log10=case.lm[5])


def search_kwargs(case):
    return dict(beam=case.beam, alpha=case.alpha, beta=case.beta, tok_of_label=tok_of_label(case), bos=case.bos,
                eos=case.eos)


def compare(name, res, ref, err_of, bound):
    """res against the reference: tokens, timesteps, counts and n_tokens equal;
    lm_log10 equal bit for bit; the LM part of total equal bit for bit, taken as
    total == (am + W) [+ the </s> term] with res's own am and the reference's W
    (total - am itself is rounded at total's size, so it moves with the last
    place of am); am and total within bound under err_of(got, want, frames).
    Returns the largest error."""
    assert [len(u) for u in res] == [len(u) for u in ref["hyps"]], name
    err = 0.0
    for b, (got, want) in enumerate(zip(res, ref["hyps"])):
        for j, (g, r) in enumerate(zip(got, want)):
            assert g[0] == r[0] and g[1] == r[1] and g[5] == r[5], (name, b, j)
            assert g[4] == r[4], (name, b, j, g[4], r[4])
            total = g[3] + ref["weights"][b][j]
            if ref["eos_terms"][b][j] != 0.0:
                total = total + ref["eos_terms"][b][j]
            assert g[2] == total, (name, b, j, g[2], total)
            err = max(err, err_of(g[3], r[3], ref["frames"][b]), err_of(g[2], r[2], ref["frames"][b]))
    print(f"rnnt lm {name}: max error {err:.3e} (bound {bound:.0e})")
    assert err <= bound, (name, err)
    return err
