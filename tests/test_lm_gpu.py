"""GPU checks of asr_lm_score (csrc/lm.hip): the device against asr_lm_score_host
on the same handle (matched orders and counts equal, per-token values bit-equal,
totals within 1e-9 of the sum of |terms|), the edges of the table walk, the
independence promise, untouched memory, and CTCDecoder.lm_rescore after a real
decode."""
import math

import numpy as np
import pytest

from conftest import asr, oracle
import lm_reference as R

pytestmark = pytest.mark.gpu

BOS, EOS = R.BOS, R.EOS
LENGTHS = [0, 1, 2, 63, 64, 65, 200, 130, 1000]
SENT_F = -12345.678
SENT_I = -77


@pytest.fixture(scope="module", autouse=True)
def device():
    asr.set_device(0)


def pack(hyps, ldt=None, max_len=None):
    max_len = max([len(h) for h in hyps] + [0]) if max_len is None else max_len
    ldt = max(max_len, 1) if ldt is None else ldt
    tok = np.full((len(hyps), ldt), 3, np.int32)     # a valid id in the padding: it must never be read as a token
    for n, h in enumerate(hyps):
        tok[n, :len(h)] = h
    return tok, np.array([len(h) for h in hyps], np.int32), max_len


def host_score(lm, tok, lengths, max_len, flags):
    N, ldt = tok.shape
    ldd = max_len + 1
    logp, counts = np.zeros(N, np.float64), np.zeros((N, 2), np.int32)
    tl, to = np.full((N, ldd), SENT_F, np.float64), np.full((N, ldd), SENT_I, np.int32)
    asr.check(asr.lib().asr_lm_score_host(lm.h, tok.ctypes.data, ldt, None if lengths is None else lengths.ctypes.data,
                                          N, max_len, flags, logp.ctypes.data, counts.ctypes.data, tl.ctypes.data,
                                          to.ctypes.data, ldd), "asr_lm_score_host")
    return logp, counts, tl, to


def device_score(lm, tok, lengths, max_len, flags, want=("logp", "counts", "tl", "to"), ldd=None, pad=3):
    """One asr_lm_score; every output buffer is pre-filled with a sentinel and has
    `pad` extra rows.  Returns the four arrays (None where not asked for)."""
    N, ldt = tok.shape
    ldd = max_len + 1 if ldd is None else ldd
    d_tok = asr._upload(tok)
    d_len = None if lengths is None else asr._upload(lengths)
    bufs = {"logp": np.full(N + pad, SENT_F, np.float64), "counts": np.full((N + pad, 2), SENT_I, np.int32),
            "tl": np.full((N + pad, ldd), SENT_F, np.float64), "to": np.full((N + pad, ldd), SENT_I, np.int32)}
    dev = {k: asr._upload(v) for k, v in bufs.items() if k in want}
    ptr = {k: (dev[k].ptr if k in dev else None) for k in bufs}
    asr.check(asr.lib().asr_lm_score(lm.h, d_tok.ptr, ldt, None if d_len is None else d_len.ptr, N, max_len, flags,
                                     ptr["logp"], ptr["counts"], ptr["tl"], ptr["to"], ldd, None), "asr_lm_score")
    asr.synchronize()
    out = {k: (asr._download(dev[k], bufs[k].shape, bufs[k].dtype) if k in dev else None) for k in bufs}
    for k in dev:   # the rows past N are never written
        assert (out[k][N:] == bufs[k][N:]).all(), k
        out[k] = out[k][:N]
    return out["logp"], out["counts"], out["tl"], out["to"]


def assert_device_equals_host(lm, hyps, flags, ldt=None, lengths="given", max_len=None):
    tok, ln, max_len = pack(hyps, ldt, max_len)
    if lengths is None:
        ln = None
    elif lengths != "given":
        ln = np.asarray(lengths, np.int32)
    h_logp, h_counts, h_tl, h_to = host_score(lm, tok, ln, max_len, flags)
    d_logp, d_counts, d_tl, d_to = device_score(lm, tok, ln, max_len, flags)
    assert (d_counts == h_counts).all()
    assert (d_to == h_to).all()
    assert (d_tl.view(np.int64) == h_tl.view(np.int64)).all()            # bit-equal, sentinels included
    mask = np.arange(max_len + 1)[None, :] < h_counts[:, :1]
    scale = np.where(mask, np.abs(h_tl), 0.0).sum(axis=1)
    assert (np.abs(d_logp - h_logp) <= 1e-9 * scale).all()
    # entries past the scored ones keep the sentinel
    assert (d_tl[~mask] == SENT_F).all() and (d_to[~mask] == SENT_I).all()
    return h_logp, h_counts, h_tl, h_to


def hyps_of(rng, vocab, N, lengths=LENGTHS, oov_rate=0.0):
    return R.random_hypotheses(rng, vocab, [lengths[n % len(lengths)] for n in range(N)], oov_rate)


@pytest.fixture(scope="module")
def models():
    rng = np.random.default_rng(2026)
    made = {}
    for name, (vocab, order, unk) in {"uni": (7, 1, False), "tri": (12, 3, False), "tri_unk": (12, 3, True),
                                      "oct": (9, 8, False)}.items():
        text = R.random_arpa(rng, vocab, order, [50 + 25 * k for k in range(2, order + 1)], unk=unk)
        lm = asr.NGramLM.from_string(text, oov_log10=-4.5)
        lm.upload()
        made[name] = lm
    yield made
    for lm in made.values():
        lm.close()


@pytest.mark.parametrize("name", ["uni", "tri", "oct"])
@pytest.mark.parametrize("N", [1, 63, 257])
def test_device_equals_host(models, name, N):
    lm = models[name]
    assert lm.order == {"uni": 1, "tri": 3, "oct": 8}[name]
    rng = np.random.default_rng(N)
    lengths = LENGTHS if N > 1 else [1000]
    for flags in (0, BOS, EOS, BOS | EOS):
        assert_device_equals_host(lm, hyps_of(rng, lm.vocab_size, N, lengths), flags)


def test_single_hypotheses_of_every_length(models):
    lm = models["tri"]
    rng = np.random.default_rng(9)
    for L in LENGTHS:
        assert_device_equals_host(lm, hyps_of(rng, lm.vocab_size, 1, [L]), BOS | EOS)


def test_ldt_beyond_max_len_and_lengths_variants(models):
    lm = models["tri"]
    rng = np.random.default_rng(3)
    hyps = hyps_of(rng, lm.vocab_size, 63, [5, 64, 70, 0, 33])
    # NULL lengths: every row has max_len tokens (the padding id is then a token like any other)
    assert_device_equals_host(lm, hyps, BOS | EOS, ldt=97, lengths=None)
    assert_device_equals_host(lm, hyps, 0, ldt=70, lengths=None)
    # given lengths, beyond max_len and negative: clamped to [0, max_len]
    ln = [len(h) for h in hyps]
    ln[0], ln[1], ln[2], ln[3] = 1000, -5, 71, -(1 << 31)
    h_logp, h_counts, _, _ = assert_device_equals_host(lm, hyps, BOS | EOS, ldt=97, lengths=ln)
    assert h_counts[0, 0] == 71 and h_counts[1, 0] == 1 and h_counts[2, 0] == 71 and h_counts[3, 0] == 1
    assert_device_equals_host(lm, hyps, EOS, ldt=128, lengths=ln, max_len=80)


def test_every_output_alone_and_all_together(models):
    lm = models["oct"]
    rng = np.random.default_rng(4)
    tok, ln, max_len = pack(hyps_of(rng, lm.vocab_size, 63, [0, 3, 64, 129]))
    full = device_score(lm, tok, ln, max_len, BOS | EOS)
    names = ("logp", "counts", "tl", "to")
    for i, k in enumerate(names):
        alone = device_score(lm, tok, ln, max_len, BOS | EOS, want=(k,))
        assert [x is not None for x in alone] == [j == i for j in range(4)]
        assert alone[i].tobytes() == full[i].tobytes(), k
    pair = device_score(lm, tok, ln, max_len, BOS | EOS, want=("logp", "to"))
    assert pair[0].tobytes() == full[0].tobytes() and pair[3].tobytes() == full[3].tobytes()


EDGE = """
\\data\\
ngram 1=12
ngram 2=4
ngram 3=1

\\1-grams:
-1.0\t<s>\t-0.5
-1.0\t</s>
-1.0\tw0\t-0.25
-1.0\tw1\t-0.25
-1.0\tw2\t-0.25
-1.0\tw3\t-0.25
-1.0\tw4\t-0.25
-1.0\tw5\t-0.25
-1.0\tw6\t-0.25
-1.0\tw7\t-0.25
-1.0\tw8\t-0.25
-1.0\tw9\t-0.25

\\2-grams:
-0.5\tw0 w5\t-0.125
-0.5\tw3 w5
-0.5\tw9 w5
-0.5\tw2 w7

\\3-grams:
-0.25\tw1 w0 w5

\\end\\
"""


def test_child_range_edges():
    """w5 has the children w0, w3, w9 (hits on the first and the last of a range,
    misses below, between and above); w7 has one child; (w5, w0) has one child."""
    lm = asr.NGramLM.from_string(EDGE)
    lm.upload()
    w = lambda i: i + 2
    cases = [([w(0), w(5)], 2), ([w(9), w(5)], 2), ([w(3), w(5)], 2), ([w(4), w(5)], 1), ([w(1), w(5)], 1),
             ([1, w(5)], 1), ([w(2), w(7)], 2), ([w(1), w(7)], 1), ([w(8), w(7)], 1), ([w(1), w(0), w(5)], 3),
             ([w(2), w(0), w(5)], 2), ([w(0), w(0), w(5)], 2), ([w(1), w(3), w(5)], 2), ([w(6), w(6)], 1)]
    hyps = [c for c, _ in cases]
    _, _, h_tl, h_to = assert_device_equals_host(lm, hyps, 0)
    ref = R.ArpaModel(EDGE)
    for n, (c, q) in enumerate(cases):
        assert h_to[n, len(c) - 1] == q, c
        _, _, v, o = ref.score(c, 0)
        assert h_tl[n, :len(c)].tolist() == v and h_to[n, :len(c)].tolist() == o
    lm.close()


@pytest.mark.parametrize("name", ["tri", "tri_unk"])
def test_out_of_vocabulary_ids(models, name):
    lm = models[name]
    rng = np.random.default_rng(6)
    V = lm.vocab_size
    hyps = hyps_of(rng, V, 63, [1, 2, 9, 65, 130], oov_rate=0.25)
    hyps += [[-1], [V], [V + 1000, 2, 3], [2, -1, -1, 3, 4, 5], [-1] * 70, [1 << 30, -(1 << 31), 3]]
    for flags in (0, BOS | EOS):
        _, counts, tl, to = assert_device_equals_host(lm, hyps, flags)
        n = len(hyps) - 2                                  # seventy OOVs
        assert counts[n, 1] == 70
        if lm.unk_id < 0:
            assert (to[n, :70] == 0).all() and (tl[n, :70] == np.float32(-4.5)).all()
        else:
            assert (to[n, :70] >= 1).all()


def big_arpa(rng, V, per_order):
    """vocab V (ids 0 and 1 are <s> and </s>), per_order n-grams of each order 2..4."""
    names = ["<s>", "</s>"] + ["w%d" % i for i in range(V - 2)]
    levels = [np.arange(V, dtype=np.int64)[:, None]]
    for _ in range(3):
        prev = levels[-1][levels[-1][:, -1] != 1]
        cand = np.concatenate([prev[rng.integers(0, len(prev), per_order)],
                               rng.integers(1, V, per_order)[:, None]], axis=1)
        levels.append(np.unique(cand, axis=0))
    out = ["\\data\\"] + ["ngram %d=%d" % (k + 1, len(lv)) for k, lv in enumerate(levels)]
    for k, lv in enumerate(levels):
        p = rng.uniform(-4.0, 0.0, len(lv)).astype(np.float32)
        b = rng.uniform(-1.0, 0.25, len(lv)).astype(np.float32)
        out += ["", "\\%d-grams:" % (k + 1)]
        out += ["%.9g\t%s\t%.9g" % (p[i], " ".join(names[j] for j in g), b[i]) for i, g in enumerate(lv.tolist())]
    return "\n".join(out + ["", "\\end\\", ""]), levels


def test_larger_model_against_the_host_scorer():
    rng = np.random.default_rng(8)
    text, levels = big_arpa(rng, 2000, 70000)
    assert 1.9e5 <= sum(len(lv) for lv in levels[1:]) <= 2.1e5
    lm = asr.NGramLM.from_string(text)
    lm.upload()
    info = lm.info()
    assert info["order"] == 4 and info["nodes_inserted"] > 0
    N = 4096
    lens = rng.integers(0, 81, N)
    lens[:4] = [80, 0, 1, 79]
    # random ids over 2000 words nearly always back off to the unigram, so three
    # quarters of the hypotheses are chains of the model's own 4-grams
    hyps = []
    for n, L in enumerate(lens):
        if n % 4 == 0:
            hyps.append(rng.integers(0, 2000, L).tolist())
        else:
            rows = levels[3][rng.integers(0, len(levels[3]), L // 4 + 1)]
            hyps.append(rows.reshape(-1)[:L].tolist())
    _, _, _, h_to = assert_device_equals_host(lm, hyps, BOS | EOS)
    assert (h_to == 4).sum() > N and (h_to == 1).sum() > N     # deep matches and full back-offs both occur
    lm.close()


def test_independence(models):
    lm = models["oct"]
    rng = np.random.default_rng(10)
    hyps = hyps_of(rng, lm.vocab_size, 130, [0, 1, 64, 65, 130, 200, 7], oov_rate=0.05)
    tok, ln, max_len = pack(hyps)
    base = device_score(lm, tok, ln, max_len, BOS | EOS)[0]
    # another row order
    perm = rng.permutation(len(hyps))
    tok_p, ln_p, _ = pack([hyps[i] for i in perm])
    assert device_score(lm, tok_p, ln_p, max_len, BOS | EOS)[0].tobytes() == base[perm].tobytes()
    # another N
    assert device_score(lm, tok[:37], ln[:37], max_len, BOS | EOS)[0].tobytes() == base[:37].tobytes()
    one = device_score(lm, tok[129:], ln[129:], max_len, BOS | EOS)[0]
    assert one.tobytes() == base[129:].tobytes()
    # another ldt and max_len
    tok_w, ln_w, ml_w = pack(hyps, ldt=333, max_len=301)
    assert device_score(lm, tok_w, ln_w, ml_w, BOS | EOS)[0].tobytes() == base.tobytes()
    # with and without the detail outputs
    assert device_score(lm, tok, ln, max_len, BOS | EOS, want=("logp",))[0].tobytes() == base.tobytes()
    assert device_score(lm, tok, ln, max_len, BOS | EOS, want=("logp", "tl"))[0].tobytes() == base.tobytes()
    # and the mirror's own path
    assert lm.score(hyps)[0].tobytes() == base.tobytes()


def test_untouched_memory(models):
    lm = models["tri"]
    rng = np.random.default_rng(12)
    hyps = hyps_of(rng, lm.vocab_size, 63, [0, 1, 5, 64, 65])
    tok, ln, max_len = pack(hyps, ldt=80)
    ldd = max_len + 9
    for flags in (0, EOS):
        logp, counts, tl, to = device_score(lm, tok, ln, max_len, flags, ldd=ldd)
        scored = np.arange(ldd)[None, :] < counts[:, :1]
        assert (counts[:, 0] == ln + (1 if flags & EOS else 0)).all()
        assert (tl[~scored] == SENT_F).all() and (to[~scored] == SENT_I).all()     # columns beyond max_len + 1 too
        assert (tl[scored] != SENT_F).all() and (to[scored] >= 1).all()
        assert (logp != SENT_F).all()


def test_lm_rescore_after_a_real_decode(models):
    T, B, V, beam = 40, 4, 6, 8
    lm = models["tri"]
    labels = ["", lm.token_string(2), lm.token_string(5), lm.token_string(7), lm.token_string(9), "not-a-token"]
    mapper = lm.label_mapper(labels, mode="char")
    emis = oracle.synthetic_emissions(T, B, V, seed0=99)
    dec = asr.CTCDecoder(V, beam, 0)
    dec.decode(emis)
    plain = dec.rescore(beam)
    beams = dec.beams(beam)
    alpha, beta = 0.8, 0.3
    out = dec.lm_rescore(beam, lm, alpha, beta, mapper)
    assert [len(u) for u in out] == [len(u) for u in plain]
    for b in range(B):
        exact = {tuple(lab): ex for lab, ex, _ in plain[b]}
        rank = {tuple(lab): i for i, (lab, _) in enumerate(beams[b])}
        assert sorted(tuple(r[0]) for r in out[b]) == sorted(exact)
        for lab, total, ex, ll, nt in out[b]:
            assert ex == exact[tuple(lab)]
            toks = mapper(lab)
            want, counts = lm.score([toks], host=True)
            assert ll == want[0] and nt == len(toks) == counts[0, 0] - 1
            assert total == ex + alpha * math.log(10.0) * ll + beta * nt
        keys = [(-r[1], rank[tuple(r[0])]) for r in out[b]]
        assert keys == sorted(keys)                       # total descending, equal totals in beam order
    zero = dec.lm_rescore(beam, lm, 0.0, 0.0, mapper)
    assert [[r[0] for r in u] for u in zero] == [[r[0] for r in u] for u in plain]
    dec.close()
