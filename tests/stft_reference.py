"""Float64 restatements for the torch.stft-style front end and the Whisper
encoder: stft_mel_ref states asr_stft_fwd's semantics (include/asr_amd.h) with
np.pad and np.fft.rfft (dtype float32: the same steps in float32 on
torch.fft.rfft, whose error against float64 sets the kernel's bound), and
StandInEncoder is Whisper's encoder in torch under transformers' attribute
names, for WhisperEncoder.from_transformers."""
import numpy as np
import torch

def num_frames(c, n):
    f = (0 if n <= c["n_fft"] // 2 else 1 + n // c["hop"]) if c["center"] else (
        0 if n < c["n_fft"] else 1 + (n - c["n_fft"]) // c["hop"])
    return max(f - 1, 0) if c["drop_last"] else f


def stft_mel_ref(c, window, mel, wave, n, pad_to=0, dtype=np.float64):
    """Features [frames, n_mels] of the first n samples of wave; c: n_fft, win,
    hop, center, power, log, floor_mode, floor, dyn_range, shift, scale,
    drop_last."""
    N, hop = c["n_fft"], c["hop"]
    x = np.zeros(max(pad_to, n), dtype)
    x[:n] = wave[:n]
    T = num_frames(c, len(x))
    if T == 0:
        return np.zeros((0, mel.shape[0]))
    if c["center"]:
        x = np.pad(x, N // 2, mode="reflect")
    left = (N - c["win"]) // 2
    w = np.zeros(N, dtype)
    w[left:left + c["win"]] = window
    fr = np.stack([x[t * hop:t * hop + N] for t in range(T)]) * w
    X = np.fft.rfft(fr, axis=1) if dtype == np.float64 else torch.fft.rfft(torch.from_numpy(fr), dim=1).numpy()
    P = np.abs(X).astype(dtype) if c["power"] == 1 else (X.real ** 2 + X.imag ** 2).astype(dtype)
    v = P @ mel.astype(dtype).T
    if c["log"] != "none":
        fl = dtype(c["floor"])
        v = np.maximum(v, fl) if c["floor_mode"] == "clamp" else v + fl
        v = {"ln": np.log, "log10": np.log10, "db": lambda u: dtype(10) * np.log10(u)}[c["log"]](v)
    if c["dyn_range"] > 0:
        v = np.maximum(v, v.max() - dtype(c["dyn_range"]))
    return (v + dtype(c["shift"])) * dtype(c["scale"])


class _Attn(torch.nn.Module):
    def __init__(self, E, H):
        super().__init__()
        self.num_heads = H
        self.q_proj, self.v_proj, self.out_proj = (torch.nn.Linear(E, E) for _ in range(3))
        self.k_proj = torch.nn.Linear(E, E, bias=False)

    def forward(self, x):                                   # [B, T, E]
        B, T, E = x.shape
        sp = lambda y: y.view(B, T, self.num_heads, -1).transpose(1, 2)   # noqa: E731
        q, k, v = sp(self.q_proj(x)), sp(self.k_proj(x)), sp(self.v_proj(x))
        a = torch.softmax(q @ k.transpose(-1, -2) / (E // self.num_heads) ** 0.5, -1) @ v
        return self.out_proj(a.transpose(1, 2).reshape(B, T, E))


class _Layer(torch.nn.Module):
    def __init__(self, E, H, F):
        super().__init__()
        self.self_attn, self.self_attn_layer_norm = _Attn(E, H), torch.nn.LayerNorm(E)
        self.fc1, self.fc2, self.final_layer_norm = torch.nn.Linear(E, F), torch.nn.Linear(F, E), torch.nn.LayerNorm(E)

    def forward(self, x):
        x = x + self.self_attn(self.self_attn_layer_norm(x))
        return x + self.fc2(torch.nn.functional.gelu(self.fc1(self.final_layer_norm(x))))


class StandInEncoder(torch.nn.Module):
    """transformers' WhisperEncoder: features [B, n_mels, T] -> [B, T/2, E]."""

    def __init__(self, n_mels, E, H, F, n_layers, positions):
        super().__init__()
        self.conv1 = torch.nn.Conv1d(n_mels, E, 3, padding=1)
        self.conv2 = torch.nn.Conv1d(E, E, 3, stride=2, padding=1)
        self.embed_positions = torch.nn.Embedding(positions, E)
        self.layers = torch.nn.ModuleList(_Layer(E, H, F) for _ in range(n_layers))
        self.layer_norm = torch.nn.LayerNorm(E)

    def forward(self, feats):
        g = torch.nn.functional.gelu
        x = g(self.conv2(g(self.conv1(feats)))).permute(0, 2, 1)
        x = x + self.embed_positions.weight[:x.shape[1]]
        for layer in self.layers:
            x = layer(x)
        return self.layer_norm(x)
