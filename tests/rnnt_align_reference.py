"""RNN-T lattice scoring and forced alignment restated in plain torch float64
on top of rnnt_reference.Reference, independent of the library: the reference
of tests/test_rnnt_align_cpu.py and tests/test_rnnt_align_gpu.py.

Target y_1 .. y_U against an utterance of len frames.  The predictor is
teacher-forced (h = c = 0, one step on Emb[blank], then one step per label),
g_u = h_top(u).W_pred + b_pred, and the joint is evaluated over the whole grid:
lp = log_softmax(act(f_t + g_u).W_out + b_out), lpb(t, u) = lp[blank],
lpy(t, u) = lp[y_{u+1}] for u < U.

Topology 0 ("standard", a label arc stays in the frame), node by node:
    a(0, 0) = 0;  a(t, u) = lse(a(t-1, u) + lpb(t-1, u), a(t, u-1) + lpy(t, u-1))
    score = a(len-1, U) + lpb(len-1, U)
Topology 1 ("one_per_frame", a label arc consumes the frame):
    a(0, 0) = 0;  a(t, u) = lse(a(t-1, u) + lpb(t-1, u), a(t-1, u-1) + lpy(t-1, u-1))
    score = a(len, U), infeasible when U > len
Viterbi is the same with max; on exactly equal candidates the blank
predecessor wins.  frames[i] is the frame whose label arc emits label i.
"""
import itertools
import math

import torch

from rnnt_reference import F64, Reference, _t

NINF = -math.inf
TOPOLOGIES = {"standard": 0, "one_per_frame": 1}


def lse(a, b):
    if a == NINF:
        return b
    if b == NINF:
        return a
    return max(a, b) + math.log1p(math.exp(-abs(a - b)))


def lattice(lpb, lpy, topology):
    """lpb, lpy: lists [len][U + 1] (lpy[t][U] unused), len >= 1.  Returns score,
    vscore, frames and cells: for every node of the best path that has a
    predecessor, (t, u, value, gap) with gap = |blank candidate - label
    candidate| (inf where one of them does not exist)."""
    ln, U = len(lpb), len(lpb[0]) - 1
    rows = ln if topology == 0 else ln + 1
    a = [[NINF] * (U + 1) for _ in range(rows)]
    v = [[NINF] * (U + 1) for _ in range(rows)]
    bp = [[0] * (U + 1) for _ in range(rows)]
    gap = [[math.inf] * (U + 1) for _ in range(rows)]
    a[0][0] = v[0][0] = 0.0
    for t in range(rows):
        for u in range(U + 1):
            if t == 0 and u == 0:
                continue
            if topology == 0:
                ab = a[t - 1][u] + lpb[t - 1][u] if t >= 1 else NINF
                ay = a[t][u - 1] + lpy[t][u - 1] if u >= 1 else NINF
                vb = v[t - 1][u] + lpb[t - 1][u] if t >= 1 else NINF
                vy = v[t][u - 1] + lpy[t][u - 1] if u >= 1 else NINF
            else:
                ab = a[t - 1][u] + lpb[t - 1][u] if t >= 1 else NINF
                ay = a[t - 1][u - 1] + lpy[t - 1][u - 1] if t >= 1 and u >= 1 else NINF
                vb = v[t - 1][u] + lpb[t - 1][u] if t >= 1 else NINF
                vy = v[t - 1][u - 1] + lpy[t - 1][u - 1] if t >= 1 and u >= 1 else NINF
            a[t][u] = lse(ab, ay)
            label = vy > vb                     # equal: the blank predecessor
            v[t][u] = vy if label else vb
            bp[t][u] = 1 if label else 0
            if vb != NINF and vy != NINF:
                gap[t][u] = abs(vb - vy)
    if topology == 0:
        score, vscore = a[ln - 1][U] + lpb[ln - 1][U], v[ln - 1][U] + lpb[ln - 1][U]
    else:
        score, vscore = a[ln][U], v[ln][U]
    frames, cells = [-1] * U, []
    if vscore != NINF:
        t, u = rows - 1, U
        while (t, u) != (0, 0):
            cells.append((t, u, v[t][u], gap[t][u]))
            if bp[t][u]:
                if topology == 0:
                    frames[u - 1] = t
                else:
                    frames[u - 1] = t - 1
                    t -= 1
                u -= 1
            else:
                t -= 1
    return {"score": score, "vscore": vscore, "frames": frames, "cells": cells}


def brute_force(lpb, lpy, topology):
    """(log of the summed probability of every alignment, log-probability of the
    best one) by enumeration: for tiny grids only."""
    ln, U = len(lpb), len(lpb[0]) - 1
    logps = []
    if topology == 0:
        # labels emitted at non-decreasing frames e_1 <= .. <= e_U; one blank leaves every frame
        for e in itertools.combinations_with_replacement(range(ln), U):
            lp = 0.0
            for i, t in enumerate(e):
                lp += lpy[t][i]
            for t in range(ln):
                lp += lpb[t][sum(1 for x in e if x <= t)]
            logps.append(lp)
    else:
        for e in itertools.combinations(range(ln), U):
            lp, u = 0.0, 0
            for t in range(ln):
                if u < U and e[u] == t:
                    lp += lpy[t][u]
                    u += 1
                else:
                    lp += lpb[t][u]
            logps.append(lp)
    if not logps:
        return NINF, NINF
    m = max(logps)
    return m + math.log(sum(math.exp(x - m) for x in logps)), m


class AlignReference(Reference):
    def predictor(self, target):
        """g_u for u = 0 .. U: [U + 1, J]."""
        h = [torch.zeros(self.Hp, dtype=F64) for _ in range(self.L)]
        c = [torch.zeros(self.Hp, dtype=F64) for _ in range(self.L)]
        rows = []
        for u in range(len(target) + 1):
            self._step(self.blank if u == 0 else int(target[u - 1]), h, c)
            rows.append(h[self.L - 1] @ self.w["w_pred"] + self.w["b_pred"])
        return torch.stack(rows)

    def grid(self, enc_b, target):
        """enc_b [len, E].  (lpb, lpy) as lists [len][U + 1]; lpy[t][U] = -inf."""
        U = len(target)
        f = enc_b @ self.w["w_enc"] + self.w["b_enc"]
        x = f[:, None, :] + self.predictor(target)[None, :, :]
        z = torch.tanh(x) if self.act == "tanh" else torch.clamp(x, min=0.0)
        lp = torch.log_softmax(z @ self.w["w_out"] + self.w["b_out"], dim=-1)     # [len, U + 1, V]
        lpb = lp[:, :, self.blank]
        lpy = torch.full_like(lpb, NINF)
        if U:
            idx = torch.as_tensor(list(target), dtype=torch.long)
            lpy[:, :U] = lp[:, :U, :].gather(2, idx[None, :, None].expand(lp.shape[0], U, 1))[:, :, 0]
        return lpb.tolist(), lpy.tolist()

    def align(self, enc, targets, lengths=None, utt=None, topology="standard", max_target_len=None):
        """Per target a dict: score, vscore, frames (list of U_n, -1 when
        infeasible), cells (see lattice), terms (len_b + U_n)."""
        topo = TOPOLOGIES[topology] if isinstance(topology, str) else int(topology)
        enc = _t(enc)
        T, B = enc.shape[0], enc.shape[1]
        V = self.w["b_out"].shape[0]
        out = []
        for n, tgt in enumerate(targets):
            tgt = list(tgt) if max_target_len is None else list(tgt)[:max_target_len]
            U = len(tgt)
            b = n if utt is None else int(utt[n])
            ok = 0 <= b < B
            ln = 0 if not ok else T if lengths is None else max(0, min(int(lengths[b]), T))
            bad = any(y < 0 or y >= V or y == self.blank for y in tgt)
            res = {"score": NINF, "vscore": NINF, "frames": [-1] * U, "cells": [], "terms": ln + U}
            if not ok or bad or (ln == 0 and U > 0) or (topo == 1 and U > ln):
                pass
            elif ln == 0:
                res["score"] = res["vscore"] = 0.0
            else:
                lpb, lpy = self.grid(enc[:ln, b], tgt)
                res.update(lattice(lpb, lpy, topo))
            out.append(res)
        return out
