"""The transducer beam search (one symbol per frame) restated in plain torch
float64 on top of rnnt_reference.Reference, independent of the library: the
reference of tests/test_rnnt_beam_cpu.py and tests/test_rnnt_beam_gpu.py.

Search of one utterance with beam width K (length clamped to [0, T]).  A
hypothesis is (ys, one timestep per token, score, predictor state after ys);
the beam A is ordered by rank and starts as the empty hypothesis with score 0
and the start state (h = c = 0, one predictor step on Emb[blank]).  Each frame
t: lp_i = log_softmax(joint(f_t, h_top_i)) for every hypothesis i; candidate
(i, v) scores s_i + lp_i[v]; the best min(K, |A| V) are kept in the order score
descending, i ascending, v ascending, a NaN after every number; (i, blank) is
hypothesis i with the new score, (i, v) is ys_i + [v] at timestep t with the
state stepped on Emb[v]; kept candidates with equal token sequences (compared
as sequences) merge: score logaddexp, timesteps of the higher score, the
earlier candidate on equal scores; the new A is the merged set by score
descending, ties by the position of the earlier constituent.
"""
import math

import torch

from rnnt_reference import F64, Reference, _t


def _key(score, idx):
    """Sort key of the candidate order: a NaN after every number."""
    return (1, 0.0, idx) if score != score else (0, -score, idx)


class _Hyp:
    __slots__ = ("ys", "ts", "score", "h", "c", "node", "pnode")

    def __init__(self, ys, ts, score, h, c, node, pnode):
        self.ys, self.ts, self.score, self.h, self.c = ys, ts, score, h, c
        # node: the extension (an id unique in the utterance) that created the hypothesis, kept while blanks keep
        # it alive; pnode: the node of the hypothesis that extension extended.  A prefix that was pruned and made
        # again has a new node, so a merge of A + blank with B + v is "deep" when A's pnode is not B's node.
        self.node, self.pnode = node, pnode


class BeamReference(Reference):
    def search(self, enc, lengths=None, beam=4, nbest=None, max_out=None):
        """enc [T, B, E].  Returns a dict: hyps (per utterance a list of (tokens,
        timesteps, score), best first, at most nbest, cut at max_out), lens
        (the uncut lengths), margin [B] (the smallest of: the last kept
        candidate's score minus the best rejected one's, the score difference
        of the two constituents of a merge, the gaps between neighbouring final
        scores; inf when none occurred), margin_nonzero (the same over the non-zero
        ones: what is left beside exact ties), max_abs_logit, merges, deep_merges
        (constituents whose creating nodes have different parents), short_frames (frames
        that end with fewer than `beam` hypotheses), frames (frames walked per
        utterance) and greedy (per utterance the K = 1 tokens, when beam > 1).
        For the option cases also: frame_sizes (per utterance, per frame, (candidates
        kept, hypotheses left after merging)), kept_labels (the non-blank labels
        of kept candidates), cut_margin [B] (the smallest kept-against-rejected
        margin alone, inf when nothing was rejected) and tied_neighbours
        (neighbours of a final list with equal scores that were extended from
        different parents)."""
        enc = _t(enc)
        T, B = enc.shape[0], enc.shape[1]
        K = int(beam)
        nbest = K if nbest is None else int(nbest)
        max_out = T if max_out is None else int(max_out)
        V = self.w["b_out"].shape[0]
        out = {"hyps": [], "lens": [], "margin": [], "margin_nonzero": [], "frames": [], "merges": 0, "deep_merges": 0,
               "short_frames": 0, "frame_sizes": [], "kept_labels": set(), "cut_margin": [], "tied_neighbours": 0}
        max_abs = 0.0
        for b in range(B):
            h = [torch.zeros(self.Hp, dtype=F64) for _ in range(self.L)]
            c = [torch.zeros(self.Hp, dtype=F64) for _ in range(self.L)]
            self._step(self.blank, h, c)
            A = [_Hyp((), (), 0.0, h, c, 0, None)]
            nodes = 0
            ln = T if lengths is None else max(0, min(int(lengths[b]), T))
            margins, cuts, sizes = [], [], []
            for t in range(ln):
                f = enc[t, b] @ self.w["w_enc"] + self.w["b_enc"]
                cands = []
                for i, hyp in enumerate(A):
                    logit = self._joint(f, hyp.h[self.L - 1])
                    max_abs = max(max_abs, float(logit.abs().max()))
                    lp = (logit - torch.logsumexp(logit, 0)).tolist()
                    cands.extend((hyp.score + lp[v], i, v) for v in range(V))
                cands.sort(key=lambda x: _key(x[0], x[1] * V + x[2]))
                nk = min(K, len(cands))
                if len(cands) > nk:
                    margins.append(cands[nk - 1][0] - cands[nk][0])
                    cuts.append(cands[nk - 1][0] - cands[nk][0])
                ent = []
                for pos, (s, i, v) in enumerate(cands[:nk]):
                    hyp = A[i]
                    if v != self.blank:
                        out["kept_labels"].add(v)
                    if v == self.blank:
                        ent.append(dict(score=s, ys=hyp.ys, ts=hyp.ts, src=hyp, tok=None, pos=pos, node=hyp.node,
                                        pnode=hyp.pnode))
                    else:
                        ent.append(dict(score=s, ys=hyp.ys + (v,), ts=hyp.ts + (t,), src=hyp, tok=v, pos=pos,
                                        node=None, pnode=hyp.node))
                merged = []
                for e in ent:
                    for m in merged:
                        if m["ys"] == e["ys"]:       # equal token sequences: m came earlier in candidate order
                            out["merges"] += 1
                            if m["pnode"] != e["pnode"]:
                                out["deep_merges"] += 1
                            margins.append(abs(m["score"] - e["score"]))
                            if e["score"] > m["score"]:      # timesteps (and the node) of the higher score
                                m["ts"], m["node"], m["pnode"] = e["ts"], e["node"], e["pnode"]
                            if m["tok"] is not None:         # the state of the constituent that needs no step
                                m["src"], m["tok"] = e["src"], e["tok"]
                            hi, lo = max(m["score"], e["score"]), min(m["score"], e["score"])
                            m["score"] = hi + math.log1p(math.exp(lo - hi))
                            break
                    else:
                        merged.append(e)
                merged.sort(key=lambda x: _key(x["score"], x["pos"]))
                if len(merged) < K:
                    out["short_frames"] += 1
                sizes.append((nk, len(merged)))
                new = []
                for e in merged:
                    src = e["src"]
                    if e["node"] is None:
                        nodes += 1
                        e["node"] = nodes
                    if e["tok"] is None:
                        new.append(_Hyp(e["ys"], e["ts"], e["score"], src.h, src.c, e["node"], e["pnode"]))
                    else:
                        h2, c2 = [x.clone() for x in src.h], [x.clone() for x in src.c]
                        self._step(e["tok"], h2, c2)
                        new.append(_Hyp(e["ys"], e["ts"], e["score"], h2, c2, e["node"], e["pnode"]))
                A = new
            for x, y in zip(A, A[1:]):
                margins.append(x.score - y.score)
                out["tied_neighbours"] += int(x.score == y.score and x.pnode != y.pnode)
            out["frame_sizes"].append(sizes)
            out["cut_margin"].append(min(cuts, default=math.inf))
            out["hyps"].append([(list(x.ys[:max_out]), list(x.ts[:max_out]), x.score) for x in A[:nbest]])
            out["lens"].append([len(x.ys) for x in A[:nbest]])
            out["margin"].append(min(margins, default=math.inf))
            out["margin_nonzero"].append(min((x for x in margins if x != 0.0), default=math.inf))
            out["frames"].append(ln)
        out["max_abs_logit"] = max_abs
        if K > 1:
            out["greedy"] = [u[0][0] for u in self.search(enc, lengths, beam=1)["hyps"]]
        return out
