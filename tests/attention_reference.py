"""float64 restatement of asr_attention_fwd and asr_layernorm_fwd in the
library's layout (no device code), computed per utterance on its own frames
with explicit masks.  Shared by test_attention_cpu.py (which checks it against
torch.nn.functional.scaled_dot_product_attention / layer_norm in float64) and
test_attention_gpu.py (which checks the device against it)."""
import numpy as np

# (T, B, heads, head_dim): the smallest shapes that straddle the kernel's 64-row
# query tile, 64-key block, 16-column MFMA tile and 4-wide contraction.
ATTN_SHAPES = [
    (5, 2, 1, 4),
    (64, 1, 1, 16),
    (70, 3, 2, 36),
    (130, 2, 4, 64),
    (65, 2, 1, 128),
    (129, 33, 2, 20),
]
# (chunk, left, right)
MASKS = {"full": (1, -1, -1), "causal": (1, -1, 0), "window": (1, 10, 3), "chunked": (16, 2, 0)}
# LayerNorm: N (rows: LN_T x LN_B)
LN_SIZES = [1, 4, 63, 64, 65, 144, 512, 4096]
LN_T, LN_B = 8, 5


def visible(p, r, chunk=1, left=-1, right=-1):
    """Query position(s) p see key position(s) r, lengths aside (broadcasts)."""
    pc, rc = np.asarray(p) // chunk, np.asarray(r) // chunk
    ok = np.ones(np.broadcast(pc, rc).shape, bool)
    if left >= 0:
        ok &= rc >= pc - left
    if right >= 0:
        ok &= rc <= pc + right
    return ok


def mask_matrix(Tq, Tk, n, chunk=1, left=-1, right=-1, q_pos0=0, k_pos0=0):
    """[Tq][Tk] bool: query row i (frame q_pos0 + i) sees key row j (frame
    k_pos0 + j) of an utterance of n frames; rows of queries past n are all False."""
    p = q_pos0 + np.arange(Tq)[:, None]
    r = k_pos0 + np.arange(Tk)[None, :]
    return visible(p, r, chunk, left, right) & (r < n) & (p < n)


def draw_attention(shape, seed=0):
    """Q, K, V [T][B][heads*head_dim] float32, U(+-1)."""
    T, B, H, D = shape
    rng = np.random.default_rng(1000 * D + 100 * H + 10 * B + T + seed)
    return tuple(rng.uniform(-1, 1, (T, B, H * D)).astype(np.float32) for _ in range(3))


def ragged_lengths(T, B):
    """(T, 0, 1, 63, 64, 65, ...) capped at T and cut to B; past the list, drawn in [1, T]."""
    base = [T, 0, 1, 63, 64, 65]
    extra = np.random.default_rng(T * 31 + B).integers(1, T + 1, max(B - len(base), 0))
    return tuple(min(int(v), T) for v in (base + list(extra))[:B])


def attention_ref(q, k, v, heads, chunk=1, left=-1, right=-1, lengths=None, scale=0.0, q_pos0=0, k_pos0=0):
    """(out [Tq][B][E] float64, seen [Tq][B] bool): softmax(q k^T scale) v per
    head over the keys each query sees; zeros for queries past the length and
    for queries that see no key (seen False)."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    Tq, B, E = q.shape
    Tk = k.shape[0]
    D = E // heads
    sc = scale if scale else 1.0 / np.sqrt(D)
    out = np.zeros((Tq, B, E))
    seen = np.zeros((Tq, B), bool)
    for b in range(B):
        n = 2 ** 40 if lengths is None else max(int(lengths[b]), 0)
        m = mask_matrix(Tq, Tk, n, chunk, left, right, q_pos0, k_pos0)
        rows = m.any(1)
        seen[:, b] = rows
        if not rows.any():
            continue
        for h in range(heads):
            sl = slice(h * D, (h + 1) * D)
            qq, kk, vv = q[rows, b, sl], k[:, b, sl], v[:, b, sl]
            cols = m.any(0)                                    # keys nobody sees may hold NaN
            s = np.full((qq.shape[0], Tk), -np.inf)
            s[:, cols] = qq @ kk[cols].T * sc
            s[~m[rows]] = -np.inf
            s -= s.max(1, keepdims=True)
            pr = np.exp(s)
            pr /= pr.sum(1, keepdims=True)
            out[rows, b, sl] = pr[:, cols] @ vv[cols]
    return out, seen


def draw_layernorm(N, T=LN_T, B=LN_B, seed=0):
    """x, res [T][B][N] U(+-1), gamma U(0.5, 1.5), beta U(+-0.1); float32."""
    rng = np.random.default_rng(7 * N + seed)
    x = rng.uniform(-1, 1, (T, B, N)).astype(np.float32)
    res = rng.uniform(-1, 1, (T, B, N)).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, N).astype(np.float32)
    beta = rng.uniform(-0.1, 0.1, N).astype(np.float32)
    return x, res, gamma, beta


def layernorm_ref(x, res=None, gamma=None, beta=None, eps=1e-5, lengths=None):
    """[T][B][N] float64, two-pass biased variance; rows t >= len_b are zeros."""
    x = np.asarray(x)
    T, B, N = x.shape
    out = np.zeros((T, B, N))
    for b in range(B):
        n = T if lengths is None else min(max(int(lengths[b]), 0), T)
        v = x[:n, b].astype(np.float64)
        if res is not None:
            v = v + np.asarray(res)[:n, b].astype(np.float64)
        mean = v.sum(1, keepdims=True) / N
        d = v - mean
        var = (d * d).sum(1, keepdims=True) / N
        y = d * (1.0 / np.sqrt(var + eps))
        if gamma is not None:
            y = y * np.asarray(gamma, np.float64)
        if beta is not None:
            y = y + np.asarray(beta, np.float64)
        out[:n, b] = y
    return out
