"""float64 references for attention-decoder rescoring (no device code), shared
by test_attention_decoder_cpu.py and test_attention_decoder_gpu.py:

- cross_attention_ref: asr_cross_attention_fwd in numpy, per hypothesis on its
  own utterance's keys, in attention_reference.attention_ref's operation order;
- decoder_ref: a float64 torch.nn.TransformerDecoder on memory.repeat_interleave
  with a causal tgt_mask and key-padding masks (what the toolkits run), giving
  the per-token log-probs and the per-hypothesis score;
- ToolkitDecoderLayer: a stand-in for ESPnet's / WeNet's DecoderLayer (separate
  linear_q / linear_k / linear_v / linear_out, normalize_before either way),
  written from their published forward; the toolkits themselves are not here;
- the shapes and draws of the GPU cases, and the tiny end-to-end model."""
import copy

import numpy as np
import torch

# ---------------------------------------------------------------- the kernel
# The kernel's tiles: 64 flat queries per workgroup (token-major over the
# hypotheses of one utterance), 64-key blocks, one instantiation per
# ceil(head_dim / 16).  (heads, head_dim, T): one case per instantiation met in
# models (1, 2, 3, 4, 8 tiles); T = 70 is a second key block of 6 keys, T = 130 a
# third of 2.
XATTN_CASES = [(2, 4, 70), (2, 16, 70), (2, 20, 70), (2, 36, 70), (2, 64, 70), (1, 128, 70), (2, 36, 130)]
COUNTS = (5, 0, 2)     # hypotheses per utterance: B = 3, N = 7
U = 13                 # tokens: 5 hypotheses x 13 = 65 flat queries, a second tile with one live lane
QLEN = (13, 0, 7, 1, 12, 13, 5)        # ragged, with 0 and U
# other groupings of the same seven hypotheses: per new utterance (the utterance of COUNTS whose memory it
# has, the hypotheses of COUNTS it holds, in their new order)
REGROUPS = [
    [(2, [5, 6]), (0, [0, 1, 2, 3, 4])],                    # utterances permuted, the empty one dropped
    [(1, []), (0, [0, 1, 2, 3, 4]), (1, []), (2, [5, 6])],  # two empty utterances
    [(0, [0, 1]), (0, [2, 3, 4]), (2, [6, 5])],             # other counts: utterance 0 twice; two hypotheses swapped
]


def klen_for(T):
    """Ragged frames per utterance with T (the utterance of 5 hypotheses: its last key block is partial
    whenever T % 64 != 0) and 0 (the utterance of 2 hypotheses)."""
    return (T, T - 3, 0)


def offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def utt_of(counts):
    return np.repeat(np.arange(len(counts)), counts).tolist()


def draw_cross(heads, head_dim, T, counts=COUNTS, u=U, seed=0):
    """q [U][N][E], k, v [T][B][E] float32, U(+-1)."""
    E, N, B = heads * head_dim, int(sum(counts)), len(counts)
    rng = np.random.default_rng(100000 * head_dim + 1000 * heads + 10 * T + N + seed)
    return (rng.uniform(-1, 1, (u, N, E)).astype(np.float32), rng.uniform(-1, 1, (T, B, E)).astype(np.float32),
            rng.uniform(-1, 1, (T, B, E)).astype(np.float32))


def nan_past(x, lengths):
    x = x.copy()
    for b, n in enumerate(lengths):
        x[max(int(n), 0):, b] = np.nan
    return x


def cross_attention_ref(q, k, v, heads, counts, qlen=None, klen=None, scale=0.0):
    """out [U][N][E] float64: hypothesis n attends to the first klen[b] frames of
    its utterance b; rows u >= qlen[n], and every row when klen[b] == 0, are
    zeros.  The operations of attention_reference.attention_ref, per hypothesis."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    Uq, N, E = q.shape
    T = k.shape[0]
    D = E // heads
    sc = scale if scale else 1.0 / np.sqrt(D)
    out = np.zeros((Uq, N, E))
    for n, b in enumerate(utt_of(counts)):
        nq = Uq if qlen is None else min(max(int(qlen[n]), 0), Uq)
        nk = T if klen is None else min(max(int(klen[b]), 0), T)
        if nq == 0 or nk == 0:
            continue
        for h in range(heads):
            sl = slice(h * D, (h + 1) * D)
            s = q[:nq, n, sl] @ k[:nk, b, sl].T * sc
            s -= s.max(1, keepdims=True)
            pr = np.exp(s)
            pr /= pr.sum(1, keepdims=True)
            out[:nq, n, sl] = pr @ v[:nk, b, sl]
    return out


# ------------------------------------------------------------ token scores
def token_score_ref(logp, tokens, lengths):
    """fp64 [N]: sum over u < lengths[n], ascending, of logp[u][n][tokens[u][n]];
    a token outside [0, V) adds -inf."""
    Uq, N, V = logp.shape
    out = np.zeros(N, np.float64)
    for n in range(N):
        s = np.float64(0.0)
        for u in range(min(max(int(lengths[n]), 0), Uq)):
            t = int(tokens[u][n])
            s = s + (np.float64(logp[u, n, t]) if 0 <= t < V else -np.inf)
        out[n] = s
    return out


# -------------------------------------------------------------- the decoder
DEC = dict(E=32, heads=4, F=64, layers=2, V=11)


def positional_encoding(length, E):
    """The toolkits' PositionalEncoding table, float64 [length, E]."""
    pe = torch.zeros(length, E, dtype=torch.float64)
    pos = torch.arange(0, length, dtype=torch.float64).unsqueeze(1)
    div = torch.exp(torch.arange(0, E, 2, dtype=torch.float64) * -(np.log(10000.0) / E))
    pe[:, 0::2] = torch.sin(pos * div)
    pe[:, 1::2] = torch.cos(pos * div)
    return pe


def make_decoder(norm_first, seed=0, final_norm=True, E=DEC["E"], heads=DEC["heads"], F=DEC["F"],
                 layers=DEC["layers"], V=DEC["V"]):
    """(embedding, torch.nn.TransformerDecoder, output Linear) in float32, eval
    mode, every bias and LayerNorm parameter drawn away from its default."""
    torch.manual_seed(1000 + 10 * seed + int(norm_first))
    emb = torch.nn.Embedding(V, E)
    layer = torch.nn.TransformerDecoderLayer(E, heads, F, dropout=0.0, norm_first=norm_first)
    dec = torch.nn.TransformerDecoder(layer, layers, norm=torch.nn.LayerNorm(E) if final_norm else None)
    out = torch.nn.Linear(E, V)
    with torch.no_grad():
        for m in list(dec.modules()) + [out]:
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.1, 0.1)
            elif isinstance(m, torch.nn.Linear):
                m.weight.uniform_(-1, 1).mul_(1.0 / np.sqrt(m.in_features))
                m.bias.uniform_(-0.1, 0.1)
            elif isinstance(m, torch.nn.MultiheadAttention):
                m.in_proj_weight.uniform_(-1, 1).mul_(1.0 / np.sqrt(E))
                m.in_proj_bias.uniform_(-0.1, 0.1)
        emb.weight.uniform_(-1, 1).mul_(1.0 / np.sqrt(E))      # * sqrt(E) in the decoder: U(+-1) again
    return emb.eval(), dec.eval(), out.eval()


def masks(Uq, lengths, utt, T, enc_lengths):
    """(causal [U][U], tgt padding [N][U], memory padding [N][T]) bool, True = masked."""
    causal = torch.triu(torch.ones(Uq, Uq, dtype=torch.bool), diagonal=1)
    tpad = torch.from_numpy(np.arange(Uq)[None, :] >= np.asarray(lengths)[:, None])
    el = np.full(int(max(utt)) + 1 if len(utt) else 0, T) if enc_lengths is None else np.asarray(enc_lengths)
    mpad = torch.from_numpy(np.arange(T)[None, :] >= el[np.asarray(utt)][:, None])
    return causal, tpad, mpad


def decoder_ref(emb, dec, out, tokens_in, targets, lengths, utt, memory, enc_lengths=None):
    """(logp [U][N][V] float64, score [N] float64): the float64 torch decoder on
    tokens_in [U][N] (lengths[n] of them real) against memory [T][B][E] repeated
    per hypothesis (memory.repeat_interleave over the utterance axis), a causal
    tgt_mask and key-padding masks; score[n] = sum over u < lengths[n] of
    logp[u][n][targets[u][n]].  Rows of logp past lengths[n] mean nothing."""
    emb, dec, out = (copy.deepcopy(m).double() for m in (emb, dec, out))
    tokens_in = np.asarray(tokens_in)
    Uq, N = tokens_in.shape
    T, B, E = memory.shape
    counts = np.bincount(np.asarray(utt), minlength=B)
    assert np.all(np.diff(utt) >= 0)
    with torch.no_grad():
        x = emb(torch.from_numpy(tokens_in.astype(np.int64))) * np.sqrt(E) + positional_encoding(Uq, E)[:, None, :]
        mem = torch.repeat_interleave(torch.from_numpy(np.asarray(memory, np.float64)), torch.from_numpy(counts),
                                      dim=1)
        causal, tpad, mpad = masks(Uq, lengths, utt, T, enc_lengths)
        y = dec(x, mem, tgt_mask=causal, tgt_key_padding_mask=tpad, memory_key_padding_mask=mpad)
        logp = torch.log_softmax(out(y), dim=-1).numpy()
    return logp, token_score_ref(logp, targets, lengths)


def layer_ref(layer, x, lengths, utt, memory, enc_lengths=None):
    """One float64 torch.nn.TransformerDecoderLayer (or ToolkitDecoderLayer) on x [U][N][E]."""
    layer = copy.deepcopy(layer).double()
    Uq, N, E = x.shape
    T, B, _ = memory.shape
    counts = np.bincount(np.asarray(utt), minlength=B)
    with torch.no_grad():
        mem = torch.repeat_interleave(torch.from_numpy(np.asarray(memory, np.float64)), torch.from_numpy(counts),
                                      dim=1)
        causal, tpad, mpad = masks(Uq, lengths, utt, T, enc_lengths)
        return layer(torch.from_numpy(np.asarray(x, np.float64)), mem, tgt_mask=causal,
                     tgt_key_padding_mask=tpad, memory_key_padding_mask=mpad).numpy()


def teacher_forcing(hyps, sos, eos):
    """(tokens_in [U][N], targets [U][N], lengths [N]): sos + y and y + eos, padded with eos."""
    N = len(hyps)
    Uq = max([len(y) for y in hyps] + [0]) + 1
    tin, tgt = np.full((Uq, N), eos, np.int64), np.full((Uq, N), eos, np.int64)
    for n, y in enumerate(hyps):
        tin[0, n] = sos
        tin[1:len(y) + 1, n] = y
        tgt[:len(y), n] = y
    return tin, tgt, np.array([len(y) + 1 for y in hyps])


# The decoder cases: hypotheses per utterance, with an utterance of none and lengths 0 (only sos) to 12
DEC_HYPS = [
    [[1, 2, 3], [4, 4, 9, 1, 2, 8, 8, 3, 5, 6, 7, 1], []],
    [],
    [[5], [9, 8, 7, 6, 5, 4, 3, 2]],
]
DEC_T, DEC_ENC_LENGTHS = 9, (9, 4, 6)


def draw_memory(T, B, E, seed=0):
    return np.random.default_rng(77 + seed).uniform(-1, 1, (T, B, E)).astype(np.float32)


# ------------------------------------------------ the toolkits' decoder layer
class ToolkitAttention(torch.nn.Module):
    """ESPnet's / WeNet's MultiHeadedAttention, batch-major: four Linears, the
    mask (True = keep) applied with masked_fill before and after the softmax."""

    def __init__(self, heads, E):
        super().__init__()
        self.h, self.d_k = heads, E // heads
        self.linear_q, self.linear_k, self.linear_v, self.linear_out = (torch.nn.Linear(E, E) for _ in range(4))

    def forward(self, query, key, value, mask):
        nb = query.size(0)
        q = self.linear_q(query).view(nb, -1, self.h, self.d_k).transpose(1, 2)
        k = self.linear_k(key).view(nb, -1, self.h, self.d_k).transpose(1, 2)
        v = self.linear_v(value).view(nb, -1, self.h, self.d_k).transpose(1, 2)
        scores = torch.matmul(q, k.transpose(-2, -1)) / np.sqrt(self.d_k)
        keep = mask.unsqueeze(1)
        scores = scores.masked_fill(~keep, float(torch.finfo(scores.dtype).min))
        attn = torch.softmax(scores, dim=-1).masked_fill(~keep, 0.0)
        x = torch.matmul(attn, v).transpose(1, 2).contiguous().view(nb, -1, self.h * self.d_k)
        return self.linear_out(x)


class ToolkitFeedForward(torch.nn.Module):
    def __init__(self, E, F):
        super().__init__()
        self.w_1, self.w_2 = torch.nn.Linear(E, F), torch.nn.Linear(F, E)

    def forward(self, x):
        return self.w_2(torch.relu(self.w_1(x)))


class ToolkitDecoderLayer(torch.nn.Module):
    """The toolkits' DecoderLayer (concat_after False), called with torch's
    time-major arguments so that layer_ref serves both kinds."""

    def __init__(self, E, heads, F, normalize_before=True):
        super().__init__()
        self.self_attn, self.src_attn = ToolkitAttention(heads, E), ToolkitAttention(heads, E)
        self.feed_forward = ToolkitFeedForward(E, F)
        self.norm1, self.norm2, self.norm3 = (torch.nn.LayerNorm(E, eps=1e-12) for _ in range(3))
        self.normalize_before = normalize_before
        self.heads = heads

    def forward(self, tgt, memory, tgt_mask, tgt_key_padding_mask, memory_key_padding_mask):
        x, mem = tgt.transpose(0, 1), memory.transpose(0, 1)                 # batch-major, as the toolkits
        tmask = (~tgt_mask)[None, :, :] & (~tgt_key_padding_mask)[:, None, :]
        mmask = (~memory_key_padding_mask)[:, None, :]
        nb = self.normalize_before
        residual = x
        if nb:
            x = self.norm1(x)
        x = residual + self.self_attn(x, x, x, tmask)
        if not nb:
            x = self.norm1(x)
        residual = x
        if nb:
            x = self.norm2(x)
        x = residual + self.src_attn(x, mem, mem, mmask)
        if not nb:
            x = self.norm2(x)
        residual = x
        if nb:
            x = self.norm3(x)
        x = residual + self.feed_forward(x)
        if not nb:
            x = self.norm3(x)
        return x.transpose(0, 1)

    def parts(self):
        """The arguments of asr.TransformerDecoderLayer.from_linears."""
        four = lambda a: (a.linear_q, a.linear_k, a.linear_v, a.linear_out)   # noqa: E731
        return dict(heads=self.heads, self_attn=four(self.self_attn), src_attn=four(self.src_attn),
                    norm1=self.norm1, norm2=self.norm2, norm3=self.norm3, w_1=self.feed_forward.w_1,
                    w_2=self.feed_forward.w_2, normalize_before=self.normalize_before)


def make_toolkit_layer(normalize_before, E=DEC["E"], heads=DEC["heads"], F=DEC["F"], seed=0):
    torch.manual_seed(2000 + seed + int(normalize_before))
    layer = ToolkitDecoderLayer(E, heads, F, normalize_before)
    with torch.no_grad():
        for m in layer.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.1, 0.1)
            elif isinstance(m, torch.nn.Linear):
                m.weight.uniform_(-1, 1).mul_(1.0 / np.sqrt(m.in_features))
                m.bias.uniform_(-0.1, 0.1)
    return layer.eval()


# ------------------------------------------------------ the end-to-end model
# CTC labels 1 .. 6 (blank 0) over V = 7 emission columns; the decoder's vocabulary
# has one entry more, the shared <sos/eos> = 7.  E2E_SEED is the seed at which the
# float64 totals of neighbouring hypotheses of EVERY utterance differ by more than
# 100 x the score bound at ctc_weight 0, 0.5 and 1 (test_attention_decoder_cpu.py
# checks that with the oracle's n-best and the references alone).
E2E = dict(T=12, B=3, V=7, beam=4, max_hyps=4, E=32, heads=4, F=64, layers=2)
E2E_SEED = 140   # the first of seeds 0 .. 299 that qualifies (smallest gap 1.16 x the required one)
E2E_WEIGHTS = (0.0, 0.5, 1.0)
ATOL = 2e-5        # the project's bound for fp32 kernels: |err| <= ATOL * (1 + |ref|)


def e2e_model(seed=E2E_SEED):
    """(emissions [T][B][V] float32 probabilities, memory [T][B][E] float32, the decoder's three torch modules)."""
    from conftest import oracle
    c = E2E
    emis = oracle.synthetic_emissions(c["T"], c["B"], c["V"], seed0=52000 + 100 * seed, sigma=1.0)
    memory = draw_memory(c["T"], c["B"], c["E"], seed=seed)
    return emis, memory, make_decoder(True, seed=50 + seed, E=c["E"], heads=c["heads"], F=c["F"],
                                      layers=c["layers"], V=c["V"] + 1)


def e2e_reference(nbest, emis, memory, modules):
    """(att, ctc) float64, flat over nbest (per utterance [(labels, ...)]): decoder_ref and the exact CTC score."""
    import ctc_align_reference as car
    hyps = [list(h[0]) for u in nbest for h in u]
    utt = [b for b, u in enumerate(nbest) for _ in u]
    eos = E2E["V"]
    tin, tgt, ln = teacher_forcing(hyps, eos, eos)
    _, att = decoder_ref(*modules, tin, tgt, ln, utt, memory)
    lp = car.log_emissions(emis, False)
    ctc = np.array([car.ctc_reference(lp[:, b], y, 0).score for y, b in zip(hyps, utt)])
    return att, ctc


def score_bound(n_tokens_max, ref):
    """(U + 1) x the layer bound, U + 1 = the longest hypothesis's len(y) + 1 terms."""
    return n_tokens_max * ATOL * (1.0 + np.abs(ref))


def smallest_gap_ratio(nbest, att, ctc, weight):
    """min over utterances and neighbouring totals (sorted) of gap / (100 x the larger score bound)."""
    worst, k = np.inf, 0
    nmax = max(len(h[0]) for u in nbest for h in u) + 1
    for u in nbest:
        tot = att[k:k + len(u)] + weight * ctc[k:k + len(u)]
        k += len(u)
        s = np.sort(tot)
        for a, b in zip(s[:-1], s[1:]):
            bound = max(score_bound(nmax, a), score_bound(nmax, b)) * (1 + abs(weight))
            worst = min(worst, (b - a) / (100 * bound))
    return worst
