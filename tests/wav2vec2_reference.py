"""Float64 restatements of asr_grouped_conv1d_fwd, asr_wave_conv_fwd and
asr_layernorm_gelu_fwd, and a compact stand-in for transformers'
Wav2Vec2Model / HubertModel (+ ForCTC) with their attribute names, state-dict
keys and config fields, so that the GPU tests need no transformers.  Every
function works on one utterance's own frames: that is the library's contract
(and, for feat_extract_norm="group", not what transformers computes on a
zero-padded batch)."""
from types import SimpleNamespace

import numpy as np
import torch
from torch import nn

F = torch.nn.functional


def t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def gelu_ref(v):
    return F.gelu(t64(v)).numpy()


def grouped_conv_ref(x, W, b, groups, pl, pr, lengths):
    """x [T, B, c_in], W [k][c_in/g][c_out], b [c_out] -> the pre-activation
    conv + b [T_out, B, c_out] in float64, zeros past out_frames(len_b)."""
    T, B, _ = x.shape
    k, _, c_out = W.shape
    out = np.zeros((max(T + pl + pr - k + 1, 0), B, c_out))
    for bi, n in enumerate(lengths):
        n = min(max(int(n), 0), T)
        if n == 0 or n + pl + pr - k + 1 <= 0:
            continue
        y = F.conv1d(F.pad(t64(x[:n, bi]).T[None], (pl, pr)), t64(W).permute(2, 1, 0).contiguous(), t64(b),
                     groups=groups)[0].T
        out[:y.shape[0], bi] = y.numpy()
    return out


def wave_frames(n, k, s):
    return 0 if n < k else (n - k) // s + 1


def wave_conv_pre(wave, nsamples, W, b, s):
    """wave [B, S], W [k, C] -> (v = conv + b [T1, B, C] float64 with zeros past
    each count, the counts)."""
    B, S = wave.shape
    k, C = W.shape
    counts = [wave_frames(min(max(int(n), 0), S), k, s) for n in nsamples]
    v = np.zeros((wave_frames(S, k, s), B, C))
    for bi, f in enumerate(counts):
        if f:
            x = t64(wave[bi, :(f - 1) * s + k])[None, None]
            v[:f, bi] = F.conv1d(x, t64(W).T[:, None, :].contiguous(), t64(b), stride=s)[0].T.numpy()
    return v, counts


def wave_norm_ref(v, counts, mode, gamma, beta, eps):
    """gelu(norm(v)) of wave_conv_pre's v: mode "none", "layer" (over channels)
    or "group" (per channel over the utterance's own frames, biased variance)."""
    out = np.zeros_like(v)
    for bi, f in enumerate(counts):
        y = v[:f, bi]
        if f and mode != "none":
            ax = 1 if mode == "layer" else 0
            y = (y - y.mean(ax, keepdims=True)) / np.sqrt(y.var(ax, keepdims=True) + eps) * gamma + beta
        out[:f, bi] = gelu_ref(y)
    return out


def ln_ref(x, gamma, beta, eps):
    x = np.asarray(x, np.float64)
    return (x - x.mean(-1, keepdims=True)) / np.sqrt(x.var(-1, keepdims=True) + eps) * gamma + beta


# --------------------------------------------------------------- stand-in
class _FeatLayer(nn.Module):
    def __init__(self, c_in, c_out, k, s, bias, norm):
        super().__init__()
        self.conv = nn.Conv1d(c_in, c_out, k, s, bias=bias)
        if norm == "group":
            self.layer_norm = nn.GroupNorm(c_out, c_out, affine=True)
        elif norm == "layer":
            self.layer_norm = nn.LayerNorm(c_out)
        self.norm = norm

    def forward(self, x):                                   # [1, C, T]
        x = self.conv(x)
        if self.norm == "group":
            x = self.layer_norm(x)
        elif self.norm == "layer":
            x = self.layer_norm(x.transpose(1, 2)).transpose(1, 2)
        return F.gelu(x)


class _Attention(nn.Module):
    def __init__(self, E, heads):
        super().__init__()
        self.num_heads = heads
        self.q_proj, self.k_proj, self.v_proj, self.out_proj = (nn.Linear(E, E) for _ in range(4))

    def forward(self, x):                                   # [T, E]
        T, E = x.shape
        sp = lambda y: y.view(T, self.num_heads, -1).transpose(0, 1)   # noqa: E731
        q, k, v = sp(self.q_proj(x)), sp(self.k_proj(x)), sp(self.v_proj(x))
        p = torch.softmax(q @ k.transpose(1, 2) / np.sqrt(E // self.num_heads), -1)
        return self.out_proj((p @ v).transpose(0, 1).reshape(T, E))


class _EncLayer(nn.Module):
    def __init__(self, E, heads, inter, stable):
        super().__init__()
        self.attention, self.layer_norm, self.final_layer_norm = _Attention(E, heads), nn.LayerNorm(E), nn.LayerNorm(E)
        self.feed_forward = nn.Module()
        self.feed_forward.intermediate_dense, self.feed_forward.output_dense = nn.Linear(E, inter), nn.Linear(inter, E)
        self.stable = stable

    def ff(self, x):
        return self.feed_forward.output_dense(F.gelu(self.feed_forward.intermediate_dense(x)))

    def forward(self, x):
        if self.stable:
            x = x + self.attention(self.layer_norm(x))
            return x + self.ff(self.final_layer_norm(x))
        x = self.layer_norm(x + self.attention(x))
        return self.final_layer_norm(x + self.ff(x))


class StandIn(nn.Module):
    """Wav2Vec2Model / HubertModel (vocab None) or their ForCTC head (vocab V:
    forward then returns log-softmax), one unpadded utterance at a time."""

    def __init__(self, mode="group", stable=False, conv_dim=(32, 32, 32), conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2),
                 hidden=48, heads=4, layers=2, inter=96, pos_k=16, pos_groups=4, vocab=None, conv_bias=True,
                 feat_proj_layer_norm=True, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        self.config = SimpleNamespace(feat_extract_norm=mode, feat_extract_activation="gelu", hidden_act="gelu",
                                      do_stable_layer_norm=stable, add_adapter=False)
        self.feature_extractor = nn.Module()
        dims = (1,) + tuple(conv_dim)
        self.feature_extractor.conv_layers = nn.ModuleList(
            _FeatLayer(dims[i], dims[i + 1], conv_kernel[i], conv_stride[i], conv_bias,
                       "layer" if mode == "layer" else "group" if i == 0 else None) for i in range(len(conv_dim)))
        self.feature_projection = nn.Module()
        self.feature_projection.feat_proj_layer_norm = feat_proj_layer_norm
        if feat_proj_layer_norm:
            self.feature_projection.layer_norm = nn.LayerNorm(conv_dim[-1])
        self.feature_projection.projection = nn.Linear(conv_dim[-1], hidden)
        self.encoder = nn.Module()
        self.encoder.pos_conv_embed = nn.Module()
        self.encoder.pos_conv_embed.conv = nn.utils.parametrizations.weight_norm(
            nn.Conv1d(hidden, hidden, pos_k, padding=pos_k // 2, groups=pos_groups), name="weight", dim=2)
        self.encoder.layer_norm = nn.LayerNorm(hidden)
        self.encoder.layers = nn.ModuleList(_EncLayer(hidden, heads, inter, stable) for _ in range(layers))
        self.lm_head = nn.Linear(hidden, vocab) if vocab else None
        with torch.no_grad():                                # norms away from (1, 0), so that a swapped pair shows
            for m in self.modules():
                if isinstance(m, (nn.LayerNorm, nn.GroupNorm)):
                    m.weight.uniform_(0.5, 1.5)
                    m.bias.uniform_(-0.2, 0.2)
        self.eval()

    @torch.no_grad()
    def forward(self, wave):                                 # [S] -> [T, E or V]
        x = wave[None, None]
        for layer in self.feature_extractor.conv_layers:
            x = layer(x)
        x = x[0].T
        if self.feature_projection.feat_proj_layer_norm:
            x = self.feature_projection.layer_norm(x)
        x = self.feature_projection.projection(x)
        pos = self.encoder.pos_conv_embed.conv(x.T[None])
        if self.encoder.pos_conv_embed.conv.kernel_size[0] % 2 == 0:
            pos = pos[:, :, :-1]
        x = x + F.gelu(pos)[0].T
        if not self.config.do_stable_layer_norm:
            x = self.encoder.layer_norm(x)
        for layer in self.encoder.layers:
            x = layer(x)
        if self.config.do_stable_layer_norm:
            x = self.encoder.layer_norm(x)
        return x if self.lm_head is None else torch.log_softmax(self.lm_head(x), -1)
