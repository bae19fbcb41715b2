"""CPU checks of CTC forced alignment / exact scoring (asr_ctc_align): the
numpy reference of tests/ctc_align_reference.py against torch's ctc_loss in
float64, brute-force enumeration and the oracle's prefix scores; then the
entry points themselves: exported, sized and argument-checked before any HIP
call (no GPU here; the fake device pointers are never dereferenced)."""
import itertools
import re
import subprocess

import numpy as np
import pytest

import torch

from conftest import asr, oracle
import ctc_align_reference as R

NAMES = ["asr_ctc_align_workspace_bytes", "asr_ctc_align"]
FAKE = 0x10000   # a non-NULL, 16-byte aligned "device pointer"


def random_log_probs(rng, T, V):
    z = rng.normal(0.0, 3.0, size=(T, V))
    return z - np.log(np.exp(z).sum(axis=1, keepdims=True))


# ------------------------------------------------------------- the reference
def test_reference_forward_equals_torch_ctc_loss_fp64():
    rng = np.random.default_rng(20261019)
    worst = 0.0
    for case in range(200):
        V = int(rng.integers(2, 6))
        blank = int(rng.integers(0, V))
        labels = [c for c in range(V) if c != blank]
        L = int(rng.integers(0, 7))
        target = [labels[int(rng.integers(0, min(len(labels), 2)))] for _ in range(L)]   # heavy repeats
        T = int(rng.integers(1, 14))
        lp = random_log_probs(rng, T, V)
        ref = R.ctc_reference(lp, target, blank)
        loss = torch.nn.functional.ctc_loss(
            torch.from_numpy(lp).unsqueeze(1), torch.tensor([target], dtype=torch.long).reshape(1, L),
            torch.tensor([T]), torch.tensor([L]), blank=blank, reduction="none", zero_infinity=False)
        want = -float(loss[0])
        if np.isinf(want):
            assert ref.score == -np.inf, (case, ref.score)
            assert ref.vscore == -np.inf and (ref.path == -1).all()
        else:
            worst = max(worst, abs(ref.score - want) / abs(want))
    assert worst <= 1e-13, worst


def collapse(align, blank):
    out, prev = [], None
    for c in align:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out


@pytest.mark.parametrize("T,V,blank,target", [(6, 4, 0, [1, 1, 2]), (6, 3, 2, [0, 1, 0]), (5, 4, 1, [3]),
                                              (4, 4, 0, []), (6, 2, 0, [1, 1, 1]), (3, 3, 0, [1, 1, 2]),
                                              (5, 3, 1, [0, 0])])
def test_reference_equals_brute_force(T, V, blank, target):
    rng = np.random.default_rng(1000 * T + 10 * V + blank)
    lp = random_log_probs(rng, T, V)
    total, best = [], -np.inf
    for align in itertools.product(range(V), repeat=T):
        if collapse(align, blank) == target:
            x = float(sum(lp[t, c] for t, c in enumerate(align)))
            total.append(x)
            best = max(best, x)
    ref = R.ctc_reference(lp, target, blank)
    if not total:
        assert ref.score == -np.inf and ref.vscore == -np.inf
        return
    m = max(total)
    want = m + np.log(np.sum(np.exp(np.array(total) - m)))
    assert abs(ref.score - want) <= 1e-13 * max(1.0, abs(want))
    assert abs(ref.vscore - best) <= 1e-13 * max(1.0, abs(best))
    # the path is an alignment of the target with the best score
    assert collapse(ref.path.tolist(), blank) == target
    assert abs(sum(lp[t, c] for t, c in enumerate(ref.path)) - best) <= 1e-13 * max(1.0, abs(best))
    for i, (lo, hi) in enumerate(ref.spans):
        assert (ref.path[lo:hi] == target[i]).all() and lo < hi


def test_reference_tie_rule_worked_example():
    lp = np.full((7, 4), np.log(0.25))
    ref = R.ctc_reference(lp, [1, 1, 2], 0)
    assert ref.path.tolist() == [1, 0, 1, 2, 0, 0, 0]
    assert ref.spans.tolist() == [[0, 1], [2, 3], [3, 4]]
    assert ref.gap == 0.0
    assert ref.vscore == pytest.approx(7 * np.log(0.25), rel=1e-15)
    empty = R.ctc_reference(lp, [], 0)
    assert empty.path.tolist() == [0] * 7 and empty.spans.shape == (0, 2)
    assert empty.score == empty.vscore


def test_reference_invalid_content_and_no_frames():
    lp = np.full((4, 3), np.log(1.0 / 3))
    for bad in ([0], [3], [-1], [1, 0, 2]):
        ref = R.ctc_reference(lp, bad, 0)
        assert ref.score == -np.inf and ref.vscore == -np.inf
        assert (ref.path == -1).all() and (ref.spans == -1).all()
    assert R.ctc_reference(lp[:0], [], 0).score == 0.0
    assert R.ctc_reference(lp[:0], [1], 0).score == -np.inf
    assert R.ctc_reference(lp[:2], [1, 1], 0).score == -np.inf   # needs 3 frames


@pytest.mark.parametrize("T,V,beam", [(5, 3, 200), (4, 4, 250)])
def test_reference_equals_oracle_prefix_scores_with_a_full_beam(T, V, beam):
    """With a beam that holds every prefix nothing is pruned, so the oracle's
    score of a hypothesis is the sum over all its alignments."""
    B = 3
    emis = oracle.synthetic_emissions(T, B, V, seed0=77 + T)
    hyps = oracle.decode(emis, beam, 0, nthreads=1, max_hyps=beam)
    n = 0
    for b in range(B):
        lp = R.log_emissions(emis[:, b], False)
        for labels, score in hyps[b]:
            ref = R.ctc_reference(lp, labels, 0)
            assert abs(ref.score - score) <= 1e-12 * abs(score), (b, labels, ref.score, score)
            n += 1
    assert n > B * 20


# ---------------------------------------------------------- the entry points
def test_symbols_in_mirror_and_library():
    for n in NAMES:
        assert n in asr.EXPORTS, n
        assert hasattr(asr.lib(), n), n
    out = subprocess.run(["nm", "-D", "--defined-only", str(asr.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (asr_[a-z0-9_]+)$", out, flags=re.M))
    assert set(NAMES) <= exported


MTLS = [0, 1, 31, 32, 63, 64, 127, 128, 255, 256, 511]


def test_workspace_bytes_properties():
    ws = asr.ctc_align_workspace_bytes
    for T, N in [(1, 1), (7, 3), (1000, 2048), (50, 9)]:
        prev = 0
        for mtl in MTLS:
            n = ws(T, N, mtl)
            assert n > 0 and n % 16 == 0
            assert n <= N * T * 64 * 4 + 4096
            if mtl <= 63:
                assert n <= (N * T * 64 * 4 + 4096) // 4
            assert n >= N * T * (2 * mtl + 1) * 2 // 8     # 2 bits per state and frame
            assert n >= prev                               # non-decreasing in max_target_len
            prev = n
    for mtl in (0, 40, 300):
        sizes = [ws(T, 5, mtl) for T in (1, 2, 3, 10, 100, 1001)]
        assert sizes == sorted(sizes)
        sizes = [ws(33, N, mtl) for N in (1, 2, 3, 10, 100, 1001)]
        assert sizes == sorted(sizes)
    assert ws(1 << 20, 1 << 11, 511) == (1 << 31) * 256   # no 32-bit overflow


def test_workspace_bytes_invalid_shape():
    ws = asr.ctc_align_workspace_bytes
    assert ws(0, 4, 10) == 0
    assert ws(-1, 4, 10) == 0
    assert ws(4, 0, 10) == 0
    assert ws(4, 4, -1) == 0
    assert ws(4, 4, 512) == 0


def align(emis=FAKE, T=10, B=2, V=5, lengths=FAKE, is_log=0, blank=0, targets=FAKE, ldt=4, tlen=FAKE,
          utt=FAKE, N=2, mtl=4, score=FAKE, vscore=FAKE, path=FAKE, ldp=10, spans=FAKE, work=FAKE):
    return asr.lib().asr_ctc_align(emis, T, B, V, B * V, V, lengths, is_log, blank, targets, ldt, tlen, utt, N,
                                   mtl, score, vscore, path, ldp, spans, work, None)


def test_err_arg():
    E = asr.ASR_ERR_ARG
    assert align(emis=None) == E
    assert align(targets=None) == E
    assert align(tlen=None) == E
    for name in ("T", "B", "V", "N"):
        assert align(**{name: 0}) == E, name
        assert align(**{name: -3}) == E, name
    assert align(blank=-1) == E
    assert align(blank=5) == E
    assert align(ldt=3) == E
    assert align(ldp=9) == E
    assert align(score=None, vscore=None, path=None, spans=None) == E
    assert align(work=None) == E                               # a path and spans wanted
    assert align(work=None, path=None) == E                    # spans alone
    assert align(work=None, spans=None) == E                   # a path alone
    assert align(utt=None, N=3) == E                           # N > B without d_utt


@pytest.mark.parametrize("kw", [dict(mtl=512, ldt=512), dict(mtl=-1), dict(V=4097), dict(mtl=100000, ldt=100000)])
def test_err_unsupported(kw):
    assert align(**kw) == asr.ASR_ERR_UNSUPPORTED


def test_python_mirror_decides_errors_before_any_device_call():
    with pytest.raises(asr.AsrError) as e:
        asr.ctc_align_device(FAKE, 4, 2, 5, 10, 5, 0, False, 7, FAKE, 4, FAKE, 0, 2, 4, d_score=FAKE)
    assert e.value.status == asr.ASR_ERR_ARG
