"""CPU checks of the wav2vec 2.0 / HuBERT additions: the stand-in of
wav2vec2_reference.py against the real transformers models (float64, single
unpadded utterances), Wav2Vec2Encoder.pack_transformers against the module it
read, and every refusal of asr_wave_conv_fwd, asr_grouped_conv1d_fwd and
asr_layernorm_gelu_fwd ahead of any HIP call (the fake device pointers are never
dereferenced on the host).  No GPU here."""
import ctypes

import numpy as np
import pytest
import torch

import wav2vec2_reference as w2v
from conftest import asr

FAKE, FAKE2 = 0x10000, 0x20000
INT_MAX = 2 ** 31 - 1
ARG, UNS = asr.ASR_ERR_ARG, asr.ASR_ERR_UNSUPPORTED
ids = lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()) or "ok"   # noqa: E731


# ------------------------------------------------ stand-in vs transformers
@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("mode", ["group", "layer"])
@pytest.mark.parametrize("family", ["Wav2Vec2", "Hubert"])
def test_stand_in_matches_transformers(family, mode, stable):
    tf = pytest.importorskip("transformers")
    cfg = getattr(tf, family + "Config")(
        hidden_size=48, num_hidden_layers=2, num_attention_heads=4, intermediate_size=96, conv_dim=(32, 32, 32),
        conv_stride=(5, 2, 2), conv_kernel=(10, 3, 2), num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4,
        feat_extract_norm=mode, do_stable_layer_norm=stable, conv_bias=True, vocab_size=20)
    torch.manual_seed(3)
    real = getattr(tf, family + "ForCTC")(cfg).double().eval()
    mine = w2v.StandIn(mode, stable, vocab=20).double()
    base = getattr(real, "wav2vec2", None) or real.hubert
    sd = {**base.state_dict(), **{"lm_head." + k: v for k, v in real.lm_head.state_dict().items()}}
    missing, unexpected = mine.load_state_dict(sd, strict=False)
    assert not missing and all(k.startswith("masked_spec_embed") for k in unexpected), (missing, unexpected)
    rng = np.random.default_rng(5)
    for n in (700, 400):
        wave = torch.from_numpy(rng.standard_normal(n))
        with torch.no_grad():
            ref = torch.log_softmax(real(wave[None]).logits[0], -1)
        got = mine(wave)
        assert got.shape == ref.shape and (got - ref).abs().max() <= 1e-12, (got - ref).abs().max()


# ----------------------------------------------------------------- packing
@pytest.mark.parametrize("mode,stable,fpln", [("group", False, True), ("layer", True, False)])
def test_pack_transformers(mode, stable, fpln):
    m = w2v.StandIn(mode, stable, vocab=20, conv_bias=mode == "layer", feat_proj_layer_norm=fpln)
    p = asr.Wav2Vec2Encoder.pack_transformers(m)
    assert (p["mode"], p["stable"], p["fp_norm"] is None) == (mode, stable, not fpln)
    for i, (spec, layer) in enumerate(zip(p["conv"], m.feature_extractor.conv_layers)):
        w = layer.conv.weight.detach().numpy()               # [c_out][c_in][k]
        assert np.array_equal(spec["weight"], w.transpose(2, 1, 0)[:, 0] if i == 0 else w.transpose(2, 1, 0))
        assert (spec["kernel"], spec["stride"]) == (layer.conv.kernel_size[0], layer.conv.stride[0])
        assert ("gamma" in spec) == (mode == "layer" or i == 0) and (spec["bias"] is None) == (mode != "layer")
    W, b, kw = p["pos"]
    conv = m.encoder.pos_conv_embed.conv                      # weight-normed: .weight is g * v / |v|, folded
    assert kw == dict(c_in=48, c_out=48, kernel=16, groups=4, padding=(8, 7)) and W.shape == (16, 12, 48)
    assert np.array_equal(W, conv.weight.detach().numpy().transpose(2, 1, 0))
    assert not np.array_equal(conv.weight.detach().numpy(), conv.parametrizations.weight.original1.detach().numpy())
    q, at = p["layers"][1], m.encoder.layers[1].attention
    assert q["w_in"].shape == (48, 144) and q["heads"] == 4
    for j, lin in enumerate((at.q_proj, at.k_proj, at.v_proj)):
        assert np.array_equal(q["w_in"][:, 48 * j:48 * (j + 1)], lin.weight.detach().numpy().T)
        assert np.array_equal(q["b_in"][48 * j:48 * (j + 1)], lin.bias.detach().numpy())
    assert np.array_equal(q["w1"], m.encoder.layers[1].feed_forward.intermediate_dense.weight.detach().numpy().T)
    assert np.array_equal(q["norm2"][0], m.encoder.layers[1].final_layer_norm.weight.detach().numpy())
    assert p["lm"][0].shape == (48, 20) and p["fp"][0].shape == (32, 48)


@pytest.mark.parametrize("field,value", [("feat_extract_activation", "relu"), ("hidden_act", "relu"),
                                         ("add_adapter", True), ("position_embeddings_type", "relative"),
                                         ("feat_extract_norm", "batch")], ids=str)
def test_pack_transformers_refuses(field, value):
    m = w2v.StandIn()
    setattr(m.config, field, value)
    with pytest.raises(ValueError):
        asr.Wav2Vec2Encoder.pack_transformers(m)


def test_pack_transformers_refuses_modules():
    m = w2v.StandIn()
    m.encoder.layers[0].attention.rel_attn_embed = torch.nn.Embedding(4, 4)        # WavLM's relative bias
    with pytest.raises(ValueError):
        asr.Wav2Vec2Encoder.pack_transformers(m)
    m = w2v.StandIn()
    m.encoder.pos_conv_embed.layers = torch.nn.ModuleList([m.encoder.pos_conv_embed.conv])   # data2vec's stack
    del m.encoder.pos_conv_embed.conv
    with pytest.raises(ValueError):
        asr.Wav2Vec2Encoder.pack_transformers(m)


# ---------------------------------------------------------------- refusals
def wave(null=None, B=4, S=400, ldw=None, ldo=None, **kw):
    d = asr.WaveConvDesc(**{**dict(channels=16, kernel=10, stride=5, norm=asr.WAVE_NORM_TIME, eps=1e-5), **kw})
    p = dict(wave=FAKE, W=FAKE, work=FAKE, out=FAKE2)
    p[null] = None
    return asr.lib().asr_wave_conv_fwd(None if null == "desc" else ctypes.byref(d), p["wave"], S if ldw is None else ldw,
                                       FAKE, p["W"], FAKE, FAKE, FAKE, p["work"], p["out"],
                                       d.channels if ldo is None else ldo, FAKE, B, S, None)


def gconv(null=None, T=8, B=4, ldx=None, ldo=None, ldr=None, out=FAKE2, **kw):
    d = asr.GroupedConv1dDesc(**{**dict(c_in=16, c_out=32, kernel=4, pad_left=2, pad_right=1, groups=4, act=1), **kw})
    p = dict(x=FAKE, W=FAKE, out=out)
    p[null] = None
    return asr.lib().asr_grouped_conv1d_fwd(None if null == "desc" else ctypes.byref(d), p["x"],
                                            d.c_in if ldx is None else ldx, FAKE, p["W"], FAKE, FAKE,
                                            d.c_out if ldr is None else ldr, p["out"], d.c_out if ldo is None else ldo,
                                            FAKE, T, B, None)


def lngelu(x=FAKE, out=FAKE, T=8, B=4, N=16, ldx=16, ldo=16, eps=1e-5, norm=1):
    return asr.lib().asr_layernorm_gelu_fwd(x, ldx, FAKE, FAKE, eps, norm, FAKE, out, ldo, T, B, N, None)


WAVE_CASES = [(ARG, dict(null=n)) for n in ("desc", "wave", "W", "out", "work")] + [
    (ARG, kw) for kw in (dict(channels=0), dict(kernel=0), dict(stride=-1), dict(norm=3), dict(eps=float("nan")),
                         dict(eps=-1.0), dict(B=0), dict(S=0), dict(ldw=399), dict(ldo=15), dict(S=9),
                         dict(kernel=33, eps=float("inf")), dict(channels=4097, ldo=16))] + [
    (UNS, kw) for kw in (dict(kernel=33), dict(stride=17), dict(channels=4097), dict(S=INT_MAX, ldw=INT_MAX, B=8))]
GCONV_CASES = [(ARG, dict(null=n)) for n in ("desc", "x", "W", "out")] + [
    (ARG, kw) for kw in (dict(c_in=0), dict(c_out=-4), dict(kernel=0), dict(groups=0), dict(pad_left=-1),
                         dict(pad_right=-1), dict(c_in=18), dict(c_out=30), dict(act=3), dict(T=0), dict(B=0),
                         dict(ldx=15), dict(ldo=31), dict(ldr=31), dict(out=FAKE), dict(T=2, pad_left=0, pad_right=0),
                         dict(groups=1, T=0), dict(kernel=200, ldx=3))] + [
    (UNS, kw) for kw in (dict(groups=1), dict(groups=16), dict(c_in=4 * 129, ldx=4 * 129), dict(c_out=4 * 129),
                         dict(kernel=129, pad_left=128), dict(c_in=2 ** 17, c_out=2 ** 17, groups=2 ** 16),
                         dict(T=INT_MAX - 4096), dict(T=1 << 20, B=1 << 12), dict(B=65536))]
LN_CASES = [(ARG, kw) for kw in (dict(x=None), dict(out=None), dict(T=0), dict(B=-1), dict(N=0), dict(ldx=15),
                                 dict(ldo=15), dict(norm=2), dict(eps=float("nan")), dict(eps=-1e-6),
                                 dict(N=5000, ldx=8))] + [
    (UNS, kw) for kw in (dict(N=4097, ldx=4097, ldo=4097), dict(T=1 << 20, B=1 << 12))]


@pytest.mark.parametrize("fn,want,kw", [(f, w, kw) for f, cases in ((wave, WAVE_CASES), (gconv, GCONV_CASES),
                                                                    (lngelu, LN_CASES)) for w, kw in cases],
                         ids=lambda v: v.__name__ if callable(v) else ids(v) if isinstance(v, dict) else str(v))
def test_refusals(fn, want, kw):
    assert fn(**kw) == want


def test_out_frames():
    d = asr.wave_conv_desc(512, 10, 5, "group")
    assert [asr.wave_conv_out_frames(d, n) for n in (-3, 0, 9, 10, 14, 15, 400, 160000)] == [0, 0, 0, 1, 1, 2, 79, 31999]
    assert asr.wave_conv_out_frames(asr.wave_conv_desc(512, 33, 5), 100) == -UNS
    assert asr.wave_conv_workspace_bytes(d, 400, 3) == 3 * 1 * 512 * 16 + 3 * 512 * 12
    assert asr.wave_conv_workspace_bytes(asr.wave_conv_desc(512, 10, 5, "layer"), 400, 3) == 0
    g = asr.grouped_conv1d_desc(768, 768, 128, 16, 64, 63, "gelu")
    assert [asr.grouped_conv1d_out_frames(g, n) for n in (0, 1, 5, 499)] == [0, 1, 5, 499]
    g = asr.grouped_conv1d_desc(16, 16, 5, 4, 1, 0)
    assert [asr.grouped_conv1d_out_frames(g, n) for n in (-1, 3, 4, 10)] == [0, 0, 1, 7]
    assert asr.grouped_conv1d_out_frames(asr.grouped_conv1d_desc(16, 16, 5, 16), 10) == -UNS
    assert asr.grouped_conv1d_out_frames(asr.grouped_conv1d_desc(16, 18, 5, 4), 10) == -ARG

