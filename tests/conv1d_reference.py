"""float64 restatement of asr_conv1d_fwd in the library's layout (no device
code): x [T][B][c_in] time-major, W [k][c_in/groups][c_out], bias [c_out] or
None, lengths [B] or None, act None / 'relu' / 'clip'.  Shared by
test_conv1d_cpu.py (which checks it against torch.nn.functional.conv1d) and
test_conv1d_gpu.py (which checks the device against it)."""
import numpy as np

# (T, B, c_in, c_out, k, s, d, pl, pr): the smallest shapes at which each
# mechanism of the dense kernel (128-row x 64-column tiles, 32-channel stages)
# can go wrong.
DENSE_SHAPES = [
    (9, 3, 4, 16, 3, 1, 1, 1, 1),         # one partial row tile
    (12, 5, 13, 20, 5, 2, 1, 2, 2),       # stride 2, c_in % 4 != 0, partial column tile
    (14, 33, 8, 48, 3, 1, 2, 4, 0),       # dilation, causal padding, several row tiles
    (10, 16, 24, 64, 1, 1, 1, 0, 0),      # pointwise
    (11, 7, 161, 32, 11, 2, 1, 5, 5),     # a DS2-like first layer
    (40, 16, 256, 256, 11, 2, 1, 5, 5),   # K = 2816, several column tiles
    (6, 17, 64, 80, 3, 3, 1, 0, 1),       # stride = k
    (8, 4, 1, 1, 2, 1, 1, 0, 0),          # everything minimal
    (30, 6, 32, 130, 7, 4, 3, 9, 9),      # padding wider than a tap step, c_out just past a tile multiple
]
# (T, B, C, k, s, d, pl, pr)
DEPTHWISE_SHAPES = [
    (40, 3, 19, 33, 1, 1, 16, 16),
    (50, 5, 64, 33, 2, 1, 16, 16),
    (20, 9, 130, 5, 1, 2, 8, 0),
    # 63 s + (k-1) d + 1 = 277 input frames per 64 output frames: more than the
    # depthwise kernel stages in LDS, so the variant that reads x from memory per tap
    (30, 4, 70, 9, 4, 3, 12, 12),
]


def as_dense(shape):
    """A depthwise shape as the 10-tuple (T, B, c_in, c_out, k, s, d, pl, pr, groups)."""
    T, B, C, k, s, d, pl, pr = shape
    return (T, B, C, C, k, s, d, pl, pr, C)


ALL_SHAPES = [sh + (1,) for sh in DENSE_SHAPES] + [as_dense(sh) for sh in DEPTHWISE_SHAPES]


def out_frames(n, k, s, d, pl, pr):
    if n <= 0 or n + pl + pr < d * (k - 1) + 1:
        return 0
    return (n + pl + pr - d * (k - 1) - 1) // s + 1


def draw(shape, seed=0, bias=True):
    """Inputs as the recurrent-layer tests draw them: x U(+-1), W U(+-1/sqrt(k c_in / groups))
    (torch's default initialisation scale), b U(+-0.1); float32."""
    T, B, ci, co, k, s, d, pl, pr, g = shape
    rng = np.random.default_rng(1000 * ci + 100 * k + 10 * B + T + seed)
    cg = ci // g
    sc = 1.0 / np.sqrt(k * cg)
    x = rng.uniform(-1, 1, (T, B, ci)).astype(np.float32)
    W = rng.uniform(-sc, sc, (k, cg, co)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, co).astype(np.float32) if bias else None
    return x, W, b


def ragged_lengths(shape):
    """Lengths that include 0, 1, T and (B >= 4; at B = 3 the 1 is that value) the
    largest count below the receptive field d (k-1) + 1; the rest drawn in [1, T]."""
    T, B, ci, co, k, s, d, pl, pr, g = shape
    assert B >= 3
    ln = np.random.default_rng(T * B + k).integers(1, T + 1, B)
    if B >= 4:
        ln[1] = max(1, min(T, d * (k - 1)))
    ln[0], ln[B // 2], ln[B - 1] = 0, 1, T
    return tuple(int(v) for v in ln)


def activation(v, act, clip):
    if act == "relu":
        return np.maximum(v, 0.0)
    if act == "clip":
        return np.minimum(np.maximum(v, 0.0), clip)
    assert act is None, act
    return v


def conv1d_ref(x, W, b, k, s, d, pl, pr, groups=1, act=None, clip=20.0, lengths=None):
    """(out [T_out][B][c_out] float64, out_lengths [B]): rows past
    out_frames(len_b) are zeros; frames of x at or past len_b are never read."""
    x = np.asarray(x)
    T, B, ci = x.shape
    W = np.asarray(W, np.float64)
    co = W.shape[2]
    assert W.shape[0] == k and W.shape[1] == ci // groups and (groups == 1 or groups == ci == co)
    T_out = out_frames(T, k, s, d, pl, pr)
    out = np.zeros((T_out, B, co), np.float64)
    oln = np.zeros(B, np.int64)
    for bi in range(B):
        n = T if lengths is None else min(max(int(lengths[bi]), 0), T)
        no = out_frames(n, k, s, d, pl, pr)
        oln[bi] = no
        if no == 0:
            continue
        span = (no - 1) * s + d * (k - 1) + 1
        xp = np.zeros((max(span, pl + n), ci), np.float64)
        xp[pl:pl + n] = x[:n, bi].astype(np.float64)
        acc = np.zeros((no, co), np.float64)
        for j in range(k):
            rows = xp[j * d:j * d + (no - 1) * s + 1:s]          # [no][ci]
            acc += rows * W[j, 0] if groups != 1 else rows @ W[j]
        if b is not None:
            acc += np.asarray(b, np.float64)
        out[:no, bi] = activation(acc, act, clip)
    return out, oln
