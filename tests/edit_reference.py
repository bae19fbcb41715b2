"""The edit-distance and MBR semantics of include/asr_amd.h written literally in
Python: the full DP table with forward-carried counts and the tie rule
(diagonal, then up, then left), the weights with their edge cases, and the two
sums in the fixed 64-partial tree.  Slow and obvious; the comparator of
tests/test_edit_cpu.py."""
import math

import numpy as np

INF = math.inf


def align(a, b):
    """(distance, (H, S, D, I)) of reference a against hypothesis b."""
    la, lb = len(a), len(b)
    # a cell: (distance, H, S, D, I)
    D = [[None] * (lb + 1) for _ in range(la + 1)]
    for i in range(la + 1):
        D[i][0] = (i, 0, 0, i, 0)
    for j in range(lb + 1):
        D[0][j] = (j, 0, 0, 0, j)
    for i in range(1, la + 1):
        for j in range(1, lb + 1):
            ne = a[i - 1] != b[j - 1]
            d, h, s, de, ins = D[i - 1][j - 1]
            cand = (d + 1, h, s + 1, de, ins) if ne else (d, h + 1, s, de, ins)
            d, h, s, de, ins = D[i - 1][j]
            if d + 1 < cand[0]:
                cand = (d + 1, h, s, de + 1, ins)
            d, h, s, de, ins = D[i][j - 1]
            if d + 1 < cand[0]:
                cand = (d + 1, h, s, de, ins + 1)
            D[i][j] = cand
    c = D[la][lb]
    return c[0], c[1:]


def distance_two_rows(a, b):
    """The distance alone, by an independent two-row DP over min()."""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j - 1] + (x != y), prev[j] + 1, cur[j - 1] + 1))
        prev = cur
    return prev[len(b)]


def weights(w):
    """e_j of one group's log weights."""
    w = [-INF if (x != x) else float(x) for x in w]
    m = max(w)
    if m == -INF:
        return [1.0] * len(w)
    if m == INF:
        return [1.0 if x == INF else 0.0 for x in w]
    return [math.exp(x - m) for x in w]


def tree_sum(terms):
    """Partial l: terms l, l + 64, .. in increasing order from 0.0; then
    partial[l] += partial[l + 32], + 16, .. + 1."""
    part = [0.0] * 64
    for j, t in enumerate(terms):
        part[j % 64] += t
    off = 32
    while off >= 1:
        for l in range(off):
            part[l] += part[l + off]
        off //= 2
    return part[0]


def mbr(hyps, w=None):
    """(risks, best, distance matrix) of one group; w None: uniform."""
    n = len(hyps)
    if n == 0:
        return [], -1, np.zeros((0, 0), np.int32)
    d = np.zeros((n, n), np.int32)
    for k in range(n):
        for j in range(k + 1, n):
            d[k, j] = d[j, k] = align(hyps[k], hyps[j])[0]
    e = [1.0] * n if w is None else weights(w)
    z = tree_sum(e)
    risks = [tree_sum([e[j] * float(d[k, j]) for j in range(n)]) / z for k in range(n)]
    best = min(range(n), key=lambda k: (risks[k], k))
    return risks, best, d
