"""GPU checks of asr_ctc_align (CTC forced alignment and exact transcript
scoring) against the fp64 numpy reference of tests/ctc_align_reference.py.

Tolerances: scores within 1e-9 relative (the decoder's own parity bound: fp64
error accumulated over ~1000 additions of magnitude <= 5000 is ~1e-9), -inf
exactly; paths and spans equal, which needs every Viterbi decision of the
reference to be decided by more than the arithmetic's error: every case
asserts that the reference's smallest decision gap is >= 1e-6 (no case is
excluded), except the tie-rule cases, whose uniform emissions make the ties
exact on both sides and whose paths the tie rule alone decides."""
import numpy as np
import pytest

from conftest import asr, oracle
import ctc_align_reference as R

pytestmark = pytest.mark.gpu

SENT = 7777          # fills the padding that a call must leave alone
REL = 1e-9
MIN_GAP = 1e-6
_refs = {}


def reference(emis, b, frames, target, is_log, blank):
    """Reference of one target against frames [0, frames) of utterance b, cached."""
    rows = np.ascontiguousarray(emis[:frames, b])
    key = (rows.tobytes(), rows.shape, tuple(target), bool(is_log), blank)
    if key not in _refs:
        _refs[key] = R.ctc_reference(R.log_emissions(rows, is_log), target, blank)
    return _refs[key]


def gpu_align(emis, targets, lengths=None, utt=None, is_log=False, blank=0, batch_major=False, mtl=None,
              ldt=None, ldp=None, want=("score", "vscore", "path", "spans")):
    """One asr_ctc_align call over time-major numpy emissions [T][B][V]; the
    path and spans buffers are sentinel-filled first."""
    T, B, V = emis.shape
    N = len(targets)
    mtl = max([len(t) for t in targets] + [0]) if mtl is None else mtl
    ldt = max(mtl, 1) if ldt is None else ldt
    ldp = T if ldp is None else ldp
    if batch_major:
        dev, fs, us = np.ascontiguousarray(emis.transpose(1, 0, 2)), V, T * V
    else:
        dev, fs, us = np.ascontiguousarray(emis), B * V, V
    tg = np.full((N, ldt), SENT, np.int32)
    for n, t in enumerate(targets):
        tg[n, :len(t)] = t
    tl = np.array([len(t) for t in targets], np.int32)
    d_emis, d_tg, d_tl = asr._upload(dev.astype(np.float32)), asr._upload(tg), asr._upload(tl)
    d_len = asr._upload(np.asarray(lengths, np.int32)) if lengths is not None else None
    d_utt = asr._upload(np.asarray(utt, np.int32)) if utt is not None else None
    d_score = asr._upload(np.full(N, 123.0)) if "score" in want else None
    d_vscore = asr._upload(np.full(N, 123.0)) if "vscore" in want else None
    d_path = asr._upload(np.full((N, ldp), SENT, np.int32)) if "path" in want else None
    d_spans = asr._upload(np.full((N, ldt, 2), SENT, np.int32)) if "spans" in want else None
    d_work = None
    if d_path or d_spans:
        d_work = asr.DeviceBytes(max(asr.ctc_align_workspace_bytes(T, N, mtl), 16))
    ptr = lambda d: d.ptr if d is not None else 0
    asr.ctc_align_device(d_emis.ptr, T, B, V, fs, us, ptr(d_len), is_log, blank, d_tg.ptr, ldt, d_tl.ptr,
                         ptr(d_utt), N, mtl, ptr(d_score), ptr(d_vscore), ptr(d_path), ldp, ptr(d_spans),
                         ptr(d_work))
    asr.synchronize()
    out = dict(T=T, mtl=mtl, ldt=ldt, ldp=ldp)
    if d_score:
        out["score"] = asr._download(d_score, N, np.float64)
    if d_vscore:
        out["vscore"] = asr._download(d_vscore, N, np.float64)
    if d_path:
        out["path"] = asr._download(d_path, (N, ldp), np.int32)
    if d_spans:
        out["spans"] = asr._download(d_spans, (N, ldt, 2), np.int32)
    return out


def close(got, want):
    if want == -np.inf:
        return got == -np.inf
    return bool(np.isfinite(got)) and abs(got - want) <= REL * abs(want)


def check(res, emis, targets, lengths=None, utt=None, is_log=False, blank=0, ties=False):
    """Every output present in res equals the reference of every target."""
    T, B, _ = emis.shape
    refs = []
    for n, target in enumerate(targets):
        b = utt[n] if utt is not None else n
        L = len(target)
        if 0 <= b < B:
            frames = T if lengths is None else max(0, min(int(lengths[b]), T))
            ref = reference(emis, b, frames, target, is_log, blank)
        else:
            frames, ref = 0, R._infeasible(0, L)
        refs.append(ref)
        if not ties:
            assert ref.gap >= MIN_GAP, (n, ref.gap)
        if "score" in res:
            assert close(res["score"][n], ref.score), (n, res["score"][n], ref.score)
        if "vscore" in res:
            assert close(res["vscore"][n], ref.vscore), (n, res["vscore"][n], ref.vscore)
        if "path" in res:
            row = res["path"][n]
            assert row[:frames].tolist() == ref.path.tolist(), (n, row[:frames], ref.path)
            assert (row[frames:T] == -1).all(), n
            assert (row[T:] == SENT).all(), n
        if "spans" in res:
            sp = res["spans"][n]
            assert sp[:L].tolist() == ref.spans.tolist(), (n, sp[:L], ref.spans)
            assert (sp[L:res["mtl"]] == -1).all(), n
            assert (sp[res["mtl"]:] == SENT).all(), n
    return refs


def repeats(target):
    return sum(1 for i in range(1, len(target)) if target[i] == target[i - 1])


def random_targets(rng, N, L, V, blank=0):
    labels = [c for c in range(V) if c != blank]
    return [[labels[int(i)] for i in rng.integers(0, len(labels), L)] for _ in range(N)]


# ---------------------------------------------------- K and lane boundaries
@pytest.mark.parametrize("is_log", [False, True])
@pytest.mark.parametrize("L", [0, 1, 31, 32, 63, 64, 127, 128, 255, 256, 511])
def test_lane_layouts_and_tight_lengths(L, is_log):
    """Every K with its largest and smallest L; T = L + repeats + {0, 1, 5}
    (the tightest leaves a single alignment) and one frame too few."""
    V, N = 5, 3
    rng = np.random.default_rng(100 + L)
    targets = random_targets(rng, N, L, V)
    need = [L + repeats(t) for t in targets]
    emis = oracle.synthetic_emissions(max(need) + 5, N, V, seed0=9000 + L, log=is_log)
    for d in (0, 1, 5) + ((-1,) if L >= 1 else ()):
        lengths = [x + d for x in need]
        e = emis[:max(max(lengths), 1)]
        res = gpu_align(e, targets, lengths=lengths, is_log=is_log)
        refs = check(res, e, targets, lengths=lengths, is_log=is_log)
        for ref in refs:
            assert (ref.score == -np.inf) == (d < 0)
        if d == 0 and L >= 1:
            for n in range(N):   # a single alignment: the forward score is the Viterbi score
                assert close(res["score"][n], res["vscore"][n])


@pytest.mark.parametrize("T", [1, 2, 3])
def test_short_sequences_below_the_prefetch_depth(T):
    V = 5
    targets = [[], [1], [2], [1, 2], [2, 2], [4, 3]]
    emis = oracle.synthetic_emissions(T, 2, V, seed0=9100 + T)
    utt = [0, 1, 0, 1, 0, 1]
    check(gpu_align(emis, targets, utt=utt), emis, targets, utt=utt)


@pytest.mark.parametrize("T", [79, 80, 90])
def test_single_label_vocabulary(T):
    """V = 2: every label is an adjacent repeat; L = 40 needs 79 frames."""
    targets = [[1] * 40]
    emis = oracle.synthetic_emissions(T, 1, 2, seed0=9200)
    refs = check(gpu_align(emis, targets), emis, targets)
    assert refs[0].score > -np.inf


@pytest.mark.parametrize("blank", [0, 28, 13])
def test_blank_position(blank):
    V, T, N = 29, 40, 3
    rng = np.random.default_rng(300 + blank)
    targets = random_targets(rng, N, 12, V, blank)
    targets[1][5] = targets[1][4]   # an adjacent repeat
    emis = oracle.synthetic_emissions(T, N, V, seed0=9300)
    check(gpu_align(emis, targets, blank=blank), emis, targets, blank=blank)


# ------------------------------------------------------------- ragged batch
@pytest.mark.parametrize("batch_major", [False, True])
def test_ragged_batch_strides_and_padding(batch_major):
    T, B, V = 50, 7, 29
    lengths = [T, 0, 1, T - 1, 5, T, 2]
    rng = np.random.default_rng(400)
    targets = [random_targets(rng, 1, L, V)[0] for L in (12, 0, 1, 20, 3, 30, 2)]
    targets[6] = [4, 4]              # 2 frames, needs 3
    targets.append([2])              # against the utterance with no frames
    utt = [0, 1, 2, 3, 4, 5, 6, 1]
    emis = oracle.synthetic_emissions(T, B, V, seed0=9400)
    mtl = 30
    res = gpu_align(emis, targets, lengths=lengths, utt=utt, batch_major=batch_major, mtl=mtl, ldt=mtl + 2,
                    ldp=T + 3)
    refs = check(res, emis, targets, lengths=lengths, utt=utt)
    assert refs[1].score == 0.0 and res["score"][1] == 0.0 and res["vscore"][1] == 0.0
    assert (res["path"][1, :T] == -1).all()
    for n in (6, 7):
        assert refs[n].score == -np.inf
        assert (res["spans"][n, :mtl] == -1).all()
    # the same call without d_utt (target n against utterance n)
    res2 = gpu_align(emis, targets[:7], lengths=lengths, batch_major=batch_major, mtl=mtl, ldt=mtl + 2,
                     ldp=T + 3)
    for k in ("score", "vscore", "path", "spans"):
        assert res2[k].tobytes() == res[k][:7].tobytes(), k


# ----------------------------------------------------------- n-best mapping
def test_nbest_mapping():
    T, B, V, N = 30, 4, 29, 12
    rng = np.random.default_rng(500)
    targets = [random_targets(rng, 1, int(L), V)[0] for L in rng.integers(0, 12, N)]
    targets[4] = list(targets[3])    # a duplicate hypothesis of utterance 1
    utt = [n // 3 for n in range(N)]
    emis = oracle.synthetic_emissions(T, B, V, seed0=9500)
    res = gpu_align(emis, targets, utt=utt, mtl=11)
    check(res, emis, targets, utt=utt)
    assert res["score"][4] == res["score"][3] and res["path"][4].tolist() == res["path"][3].tolist()
    perm = rng.permutation(N)
    res_p = gpu_align(emis, [targets[i] for i in perm], utt=[utt[i] for i in perm], mtl=11)
    for k in ("score", "vscore", "path", "spans"):
        assert res_p[k].tobytes() == res[k][perm].tobytes(), k


# -------------------------------------------------------- probability zeros
def test_probability_zeros():
    T, B, V = 12, 2, 5
    emis = oracle.synthetic_emissions(T, B, V, seed0=9600).copy()
    emis[:, 0, 3] = 0.0              # label 3 never possible in utterance 0
    emis[4, 0, 0] = 0.0              # no blank at frame 4
    emis[2:5, 1, 1] = 0.0
    emis[7, 1, [0, 1, 3, 4]] = 0.0   # utterance 1: frame 7 can only be label 2
    targets = [[1, 2, 4], [1, 3, 2], [3], [], [1, 1, 2], [2], [1, 4]]
    utt = [0, 0, 0, 0, 1, 1, 1]
    res = gpu_align(emis, targets, utt=utt)
    refs = check(res, emis, targets, utt=utt)
    # [] in utterance 0 needs the blank at frame 4; [1, 4] in utterance 1 cannot emit the 2 at frame 7
    assert [r.score == -np.inf for r in refs] == [False, True, True, True, False, False, True]
    for k in ("score", "vscore"):
        assert not np.isnan(res[k]).any()


# ---------------------------------------------------------- invalid content
def test_invalid_content_is_infeasible():
    T, B, V = 20, 2, 6
    emis = oracle.synthetic_emissions(T, B, V, seed0=9700)
    targets = [[1, 0, 2], [1, V], [-1, 2], [1, 2], [3, 4, 5], [1, 2 ** 30], [5, -2 ** 31]]
    utt = [0, 0, 1, B, 1, 0, 1]
    res = gpu_align(emis, targets, utt=utt)
    refs = check(res, emis, targets, utt=utt)
    assert [r.score == -np.inf for r in refs] == [True, True, True, True, False, True, True]
    res = gpu_align(emis, targets, utt=[0, 0, 1, -1, 1, 0, 1])
    check(res, emis, targets, utt=[0, 0, 1, -1, 1, 0, 1])


# ------------------------------------------------------------------ tie rule
def test_tie_rule():
    T, V = 7, 4
    emis = np.full((T, 1, V), 0.25, np.float32)
    targets = [[1, 1, 2], [], [3], [1, 2, 3], [2, 2, 2, 2]]
    utt = [0] * len(targets)
    for is_log in (False, True):
        e = np.log(emis) if is_log else emis
        res = gpu_align(e, targets, utt=utt, is_log=is_log)
        check(res, e, targets, utt=utt, is_log=is_log, ties=True)
        assert res["path"][0].tolist() == [1, 0, 1, 2, 0, 0, 0]
        assert res["spans"][0, :3].tolist() == [[0, 1], [2, 3], [3, 4]]
        assert res["path"][1].tolist() == [0] * T
        assert res["path"][4].tolist() == [2, 0, 2, 0, 2, 0, 2]


# ------------------------------------------------- outputs in any combination
def test_outputs_in_any_combination_are_bit_identical():
    T, B, V = 45, 3, 29
    rng = np.random.default_rng(800)
    targets = [random_targets(rng, 1, L, V)[0] for L in (9, 40, 17)]
    emis = oracle.synthetic_emissions(T, B, V, seed0=9800)
    full = gpu_align(emis, targets)
    check(full, emis, targets)
    for want in (("score",), ("vscore",), ("path",), ("spans",), ("score", "vscore"), ("vscore", "path"),
                 ("score", "spans")):
        part = gpu_align(emis, targets, want=want)
        assert sorted(k for k in part if k in ("score", "vscore", "path", "spans")) == sorted(want)
        for k in want:
            assert part[k].tobytes() == full[k].tobytes(), (want, k)


# ---------------------------------------------------------- bit independence
def test_bit_independence_of_batch_position_and_layout():
    V, L, frames = 29, 37, 60
    rng = np.random.default_rng(900)
    target = random_targets(rng, 1, L, V)[0]
    emis = oracle.synthetic_emissions(90, 9, V, seed0=9900)
    alone_e = np.ascontiguousarray(emis[:frames, 5:6])
    alone = gpu_align(alone_e, [target])                       # N = 1, max_target_len = L, T = 60
    check(alone, alone_e, [target])
    others = [random_targets(rng, 1, int(x), V)[0] for x in rng.integers(0, 60, 9)]
    others[5] = target
    lengths = [90, 70, 90, 33, 90, frames, 90, 1, 90]
    crowd = gpu_align(emis, others, lengths=lengths, mtl=511)  # position 5 of 9, K = 16, T = 90
    check(crowd, emis, others, lengths=lengths)
    assert crowd["score"][5:6].tobytes() == alone["score"].tobytes()
    assert crowd["vscore"][5:6].tobytes() == alone["vscore"].tobytes()
    assert crowd["path"][5, :frames].tolist() == alone["path"][0].tolist()
    assert crowd["spans"][5, :L].tolist() == alone["spans"][0, :L].tolist()
    for mtl in (63, 100, 200):                                 # K = 2, 4, 8
        mid = gpu_align(alone_e, [target], mtl=mtl)
        assert mid["score"].tobytes() == alone["score"].tobytes(), mtl
        assert mid["vscore"].tobytes() == alone["vscore"].tobytes(), mtl
        assert mid["path"].tolist() == alone["path"].tolist(), mtl


# ------------------------------------------------------------ long sequences
@pytest.mark.parametrize("T,V,L,B", [(1000, 29, 100, 4), (600, 29, 511, 1), (300, 1000, 255, 1)])
def test_long_sequences(T, V, L, B):
    rng = np.random.default_rng(T + L)
    targets = random_targets(rng, B, L, V)
    emis = oracle.synthetic_emissions(T, B, V, seed0=10000 + L, log=True)
    refs = check(gpu_align(emis, targets, is_log=True), emis, targets, is_log=True)
    assert all(r.score > -np.inf for r in refs)


# --------------------------------------------------------- against the decoder
def test_full_beam_scores_are_exact_and_rescore_keeps_the_order():
    """A beam that holds every prefix prunes nothing: its scores are the exact ones."""
    T, B, V, beam = 5, 6, 3, 200
    emis = oracle.synthetic_emissions(T, B, V, seed0=11000)
    dec = asr.CTCDecoder(V, beam, 0)
    dec.decode(emis)
    hyps = dec.beams(beam)
    targets = [lab for u in hyps for lab, _ in u]
    utt = [b for b, u in enumerate(hyps) for _ in u]
    beam_scores = np.array([lp for u in hyps for _, lp in u])
    exact = asr.ctc_score(emis, targets, utt=utt)
    assert len(targets) > B * 20
    assert np.all(np.abs(exact - beam_scores) <= REL * np.abs(beam_scores))
    rescored = dec.rescore(beam)
    for b in range(B):
        assert [lab for lab, _, _ in rescored[b]] == [lab for lab, _ in hyps[b]]
        for (lab, ex, bs), (_, lp) in zip(rescored[b], hyps[b]):
            assert bs == lp and abs(ex - lp) <= REL * abs(lp)
    dec.close()


def test_exact_score_bounds_a_pruned_beam_score():
    T, B, V, beam = 60, 4, 29, 5
    emis = oracle.synthetic_emissions(T, B, V, seed0=11100)
    dec = asr.CTCDecoder(V, beam, 0)
    dec.decode(emis)
    rescored = dec.rescore(beam)
    assert all(len(u) >= 1 for u in rescored)
    for u in rescored:
        assert [ex for _, ex, _ in u] == sorted((ex for _, ex, _ in u), reverse=True)
        for lab, ex, bs in u:
            assert ex >= bs - REL * abs(bs), (lab, ex, bs)
    # and the exact scores are the reference's
    b = 0
    for lab, ex, _ in rescored[b]:
        assert close(ex, reference(emis, b, T, lab, False, 0).score)
    dec.close()


def test_python_conveniences():
    T, B, V = 25, 3, 7
    emis = oracle.synthetic_emissions(T, B, V, seed0=11200)
    lengths = [25, 11, 4]
    targets = [[1, 2, 2, 6], [3], [5, 5, 5, 5]]     # the last needs 7 frames, has 4
    score = asr.ctc_score(emis, targets, lengths=lengths)
    vscore, paths, spans = asr.ctc_align(np.ascontiguousarray(emis.transpose(1, 0, 2)), targets, lengths=lengths,
                                         batch_major=True)
    for n in range(B):
        ref = reference(emis, n, lengths[n], targets[n], False, 0)
        assert ref.gap >= MIN_GAP
        assert close(score[n], ref.score) and close(vscore[n], ref.vscore)
        assert spans[n].tolist() == ref.spans.tolist()
        assert paths[n].tolist() == (ref.path.tolist() if ref.score > -np.inf else [])
