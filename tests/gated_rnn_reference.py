"""Plain float64 references of one LSTM / GRU layer and direction in the
library's layout (csrc/gated_rnn.hip), shared by test_gated_rnn_edges_cpu.py
(which checks them against torch.nn.LSTM / torch.nn.GRU in float64) and
test_gated_rnn_edges_gpu.py.

Layout: W_ih [in][NG*H], W_hh [H][NG*H], gate q of hidden unit j at column
q*H + j (LSTM: i, f, g, o; GRU: r, z, n); b_ih, b_hh [NG*H]; x [T, B, in]
time-major.  `reverse` walks the frames T-1 .. 0; `lengths` (B counts, clamped
to [0, T]) is pack_padded_sequence / pad_packed_sequence: at frames t >= len_b
utterance b's state is carried unchanged and its output row is zeros, so in
reverse it starts from h0 / c0 at its own last frame.  Rows of x at or past an
utterance's length are never read into a result (they may hold NaN).

Each reference returns (h [T, B, H], h_T [B, H], c_T [B, H] or None, z
[T, B, NG*H]): z holds every gate pre-activation of the walk (NaN where the
utterance is not active); for the GRU's candidate gate it is the argument of
the tanh, (P_n + b_in) + r * (a_n + b_hn).

Instead of x and W_ih a caller may give P [T, B, NG*H] = x.W_ih itself (the
*_recur_fwd entry points).
"""
import numpy as np


def _sigmoid(z):
    """1 / (1 + exp(-z)) without overflow at either end."""
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _setup(x, W_ih, W_hh, b_ih, b_hh, h0, lengths, P, ng):
    W_hh = np.asarray(W_hh, np.float64)
    H = W_hh.shape[0]
    assert W_hh.shape == (H, ng * H)
    if P is None:
        x = np.asarray(x, np.float64)
        T, B = x.shape[:2]
        # rows past a length may be NaN: they are computed and never selected
        with np.errstate(invalid="ignore"):
            P = x.reshape(T * B, -1) @ np.asarray(W_ih, np.float64)
    P = np.asarray(P, np.float64)
    T, B = P.shape[:2] if P.ndim == 3 else (x.shape[0], x.shape[1])
    P = P.reshape(T, B, ng * H)
    ln = np.full(B, T) if lengths is None else np.clip(np.asarray(lengths, np.int64), 0, T)
    h = np.zeros((B, H)) if h0 is None else np.array(h0, np.float64)
    return P, W_hh, np.asarray(b_ih, np.float64), np.asarray(b_hh, np.float64), T, B, H, ln, h


def lstm_ref(x, W_ih, W_hh, b_ih, b_hh, h0=None, c0=None, lengths=None, reverse=False, P=None):
    P, W_hh, b_ih, b_hh, T, B, H, ln, h = _setup(x, W_ih, W_hh, b_ih, b_hh, h0, lengths, P, 4)
    c = np.zeros((B, H)) if c0 is None else np.array(c0, np.float64)
    out, zs = np.zeros((T, B, H)), np.full((T, B, 4 * H), np.nan)
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        act = (t < ln)[:, None]
        with np.errstate(invalid="ignore", over="ignore"):
            z = P[t] + h @ W_hh + (b_ih + b_hh)
            i, f, o = _sigmoid(z[:, :H]), _sigmoid(z[:, H:2 * H]), _sigmoid(z[:, 3 * H:])
            cn = f * c + i * np.tanh(z[:, 2 * H:3 * H])
            hn = o * np.tanh(cn)
        c, h = np.where(act, cn, c), np.where(act, hn, h)
        out[t] = np.where(act, hn, 0.0)
        zs[t] = np.where(act, z, np.nan)
    return out, h, c, zs


def gru_ref(x, W_ih, W_hh, b_ih, b_hh, h0=None, c0=None, lengths=None, reverse=False, P=None):
    assert c0 is None
    P, W_hh, b_ih, b_hh, T, B, H, ln, h = _setup(x, W_ih, W_hh, b_ih, b_hh, h0, lengths, P, 3)
    out, zs = np.zeros((T, B, H)), np.full((T, B, 3 * H), np.nan)
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        act = (t < ln)[:, None]
        with np.errstate(invalid="ignore", over="ignore"):
            a = h @ W_hh
            zr = P[t, :, :H] + a[:, :H] + (b_ih[:H] + b_hh[:H])
            zz = P[t, :, H:2 * H] + a[:, H:2 * H] + (b_ih[H:2 * H] + b_hh[H:2 * H])
            zn = (P[t, :, 2 * H:] + b_ih[2 * H:]) + _sigmoid(zr) * (a[:, 2 * H:] + b_hh[2 * H:])
            n, u = np.tanh(zn), _sigmoid(zz)
            hn = (1.0 - u) * n + u * h
        h = np.where(act, hn, h)
        out[t] = np.where(act, hn, 0.0)
        zs[t] = np.where(act, np.concatenate([zr, zz, zn], 1), np.nan)
    return out, h, None, zs


REFS = {"lstm": lstm_ref, "gru": gru_ref}
NG = {"lstm": 4, "gru": 3}


def draw(cell, T, B, I, H, seed, w_ih=1.0, bias=0.1, w_hh=1.0):
    """float32 inputs of one layer and direction: W_ih ~ U(+-w_ih / sqrt(H)), W_hh ~ U(+-w_hh / sqrt(H)), both
    biases ~ U(+-bias), x, h0 and c0 ~ U(+-1).  The defaults are the scales of test_lstm_gpu.py / test_gru_gpu.py."""
    rng = np.random.default_rng(seed)
    G, s = NG[cell] * H, 1 / np.sqrt(H)
    f = lambda lim, *shape: rng.uniform(-lim, lim, shape).astype(np.float32)   # noqa: E731
    return {"cell": cell, "T": T, "B": B, "I": I, "H": H, "x": f(1, T, B, I), "h0": f(1, B, H), "c0": f(1, B, H),
            "W_ih": f(w_ih * s, I, G), "W_hh": f(w_hh * s, H, G), "b_ih": f(bias, G), "b_hh": f(bias, G)}


def reference(p, use0=True, lengths=None, reverse=False, P=None, x=None):
    """The float64 reference of the drawn inputs p: (h, h_T, c_T, z)."""
    lstm = p["cell"] == "lstm"
    return REFS[p["cell"]](p["x"] if x is None else x, p["W_ih"], p["W_hh"], p["b_ih"], p["b_hh"],
                           p["h0"] if use0 else None, p["c0"] if use0 and lstm else None, lengths, reverse, P)


def torch_run(p, dtype, use0=True, lengths=None, reverse=False):
    """torch.nn.LSTM / torch.nn.GRU on the CPU in `dtype` on the drawn inputs p: (h [T, B, H], h_T, c_T or None)
    as float64 arrays.  reverse is the flipped-input form (per utterance: each one's own valid frames reversed,
    which is what pack_padded_sequence gives the reverse direction); lengths must all be >= 1 (torch refuses 0)
    and go through pack_padded_sequence."""
    import torch
    T, B, I, H, lstm = p["T"], p["B"], p["I"], p["H"], p["cell"] == "lstm"
    m = (torch.nn.LSTM if lstm else torch.nn.GRU)(I, H, 1).to(dtype)
    x = np.array(p["x"])
    ln = np.full(B, T) if lengths is None else np.asarray(lengths)
    assert ln.min() >= 1 and ln.max() <= T
    if reverse:
        for b in range(B):
            x[:ln[b], b] = x[:ln[b], b][::-1]
    with torch.no_grad():
        for name, a in (("weight_ih_l0", p["W_ih"].T), ("weight_hh_l0", p["W_hh"].T), ("bias_ih_l0", p["b_ih"]),
                        ("bias_hh_l0", p["b_hh"])):
            getattr(m, name).copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dtype))
        st = None
        if use0:
            st = torch.from_numpy(p["h0"][None]).to(dtype)
            st = (st, torch.from_numpy(p["c0"][None]).to(dtype)) if lstm else st
        xin = torch.from_numpy(x).to(dtype)
        if lengths is not None:
            xin = torch.nn.utils.rnn.pack_padded_sequence(xin, torch.tensor(ln), enforce_sorted=False)
        out, hn = m(xin, st)
        if lengths is not None:
            out, _ = torch.nn.utils.rnn.pad_packed_sequence(out, total_length=T)
    out = out.double().numpy().copy()
    if reverse:
        for b in range(B):
            out[:ln[b], b] = out[:ln[b], b][::-1]
    hn, cn = (hn[0][0], hn[1][0]) if lstm else (hn[0], None)
    return out, hn.double().numpy(), None if cn is None else cn.double().numpy()


def rel_err(got, ref):
    """max |got - ref| / (1 + |ref|), NaN-propagating."""
    ref = np.asarray(ref, np.float64)
    e = np.abs(np.asarray(got, np.float64) - ref) / (1.0 + np.abs(ref))
    return float(np.max(e)) if np.all(np.isfinite(e)) else float("nan")


def shares(z):
    """The shares of the walk's gate pre-activations with |z| > 20 and with |z| < 2."""
    v = np.abs(z[np.isfinite(z)])
    return float(np.mean(v > 20)), float(np.mean(v < 2))


# The cases whose input conditions test_gated_rnn_edges_cpu.py asserts on the reference alone and
# test_gated_rnn_edges_gpu.py runs.
SATURATED_SHAPES = [(8, 5, 8, 32), (8, 5, 8, 144), (1, 5, 8, 32), (1, 5, 8, 144)]   # (T, B, I, H)


def saturated(cell, T, B, I, H):
    """Saturation from the input side: W_ih ~ U(+-120 / sqrt(H)), both biases ~ U(+-10), W_hh ~ U(+-1 / sqrt(H))."""
    return draw(cell, T, B, I, H, seed=7000 + 10 * H + T + (cell == "gru"), w_ih=120.0, bias=10.0)


def extreme_P(cell, T, B, H):
    """A hand-built P [T, B, NG*H] for *_recur_fwd: its entries cycle through +-1e4, +-104, +-88, +-20 and
    U(+-1), so that expf overflows in both directions (|z| > 88.7) and every gate also sees moderate values."""
    G = NG[cell] * H
    rng = np.random.default_rng(4100 + H + (cell == "gru"))
    small = rng.uniform(-1, 1, (T * B, G))
    cyc = np.array([1e4, -1e4, 104, -104, 88, -88, 20, -20, np.nan])
    # entry (row, column) takes value (column + 4 row) mod 9: a column meets all nine over nine rows, and the
    # gates of one hidden unit (columns j + q H) differ
    v = cyc[(np.arange(G)[None, :] + 4 * np.arange(T * B)[:, None]) % 9]
    return np.where(np.isnan(v), small, v).astype(np.float32).reshape(T, B, G)


def permutation(B=37):
    """A fixed permutation of B = 37 utterances: position i of the permuted batch holds utterance perm[i].  It
    moves utterance 0 and utterance B - 1, and most utterances change their row tile (16 rows) and their lane
    group within it (4 rows)."""
    return (10 * np.arange(B) + 20) % B


def ragged_lengths(T, B, seed):
    """Lengths in [1, T] with a 0, a 1 and a T among them."""
    ln = np.random.default_rng(seed).integers(1, T + 1, B)
    ln[B // 2], ln[1], ln[B - 2] = 0, 1, T
    return ln


def nan_case_lengths(T, B):
    """The NaN-in-the-padding case's lengths: 0, 1, T, -3 and T + 5 among ragged ones."""
    ln = np.random.default_rng(31 * T + B).integers(1, T + 1, B)
    ln[[0, 3, 7, B - 1, B - 2]] = [0, 1, T, -3, T + 5]
    return ln
