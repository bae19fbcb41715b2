"""Times of the wav2vec 2.0 / HuBERT additions at the Base shapes (C 512, E 768,
12 layers, positional conv k = 128 in 16 groups, "group" norm) and the Large
ones (E 1024, 24 layers, "layer" norm), 10 s utterances (160000 samples, 31999
frames after layer 0, 499 after the feature encoder), B = 16 and 64.
  (a) asr_wave_conv_fwd in time mode against torch fp32 conv1d -> GroupNorm ->
      GELU on the same GPU, with the bytes of one write of the output over the
      time (the store-bound floor's rate);
  (b) asr_grouped_conv1d_fwd (GELU, residual) against torch's grouped conv1d +
      GELU + add, and against what the library could already express: one
      asr_conv1d_fwd per group on column views, then asr_layernorm_gelu_fwd
      (norm = 0) and asr_matadd;
  (c) Wav2Vec2Encoder.forward against the stand-in of tests/wav2vec2_reference.py
      in torch fp32 eager, utterance by utterance (the stand-in takes one).
No torch figure is the code under test.  HIP events around back-to-back calls
after warm-up, interleaved rounds, median and min per call.  One JSON line per
variant.
    python tools/wav2vec2_bench.py [--rounds 11] [--warmup 2] [--batches 16,64] [--skip-encoder]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tests"))
from conftest import asr  # noqa: E402
import wav2vec2_reference as w2v  # noqa: E402
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--batches", default="16,64")
ap.add_argument("--skip-encoder", action="store_true")
a = ap.parse_args()
S, C, K0, S0 = 160000, 512, 10, 5
dev = torch.device("cuda")
torch.manual_seed(0)
f = torch.nn.functional


class Buf:
    """A torch tensor seen as a device matrix of the library."""

    def __init__(self, t):
        self.t, self.ptr, self.rows, self.cols = t, t.data_ptr(), t.shape[0], t.shape[1]


def uni(shape, s=1.0):
    return (torch.rand(shape, device=dev) * 2 - 1) * s


variants = {}   # name -> (call, extra record fields)
for B in (int(v) for v in a.batches.split(",")):
    # (a) layer 0 in time mode
    desc = asr.wave_conv_desc(C, K0, S0, "group")
    T1 = asr.wave_conv_out_frames(desc, S)
    wave, W0, g0, b0 = Buf(uni((B, S))), Buf(uni((K0, C), .3)), Buf(uni((C, 1)) + 1.5), Buf(uni((C, 1), .1))
    out0 = Buf(torch.empty((T1 * B, C), device=dev))
    work = asr.DeviceBytes(asr.wave_conv_workspace_bytes(desc, S, B))
    tw = W0.t.T[:, None, :].contiguous()
    variants[f"wave_conv_time_B{B}"] = (
        lambda wave=wave, W0=W0, g0=g0, b0=b0, out0=out0, work=work, desc=desc, B=B:
        asr.wave_conv_fwd(wave, W0, None, out0, B, S, desc, g0, b0, work),
        dict(out_bytes=4 * T1 * B * C))
    variants[f"torch_conv_groupnorm_gelu_B{B}"] = (
        lambda wave=wave, tw=tw, g0=g0, b0=b0:
        f.gelu(f.group_norm(f.conv1d(wave.t[:, None, :], tw, stride=S0), C, g0.t[:, 0], b0.t[:, 0])), {})
    # (b) the positional convolution
    for E in (768, 1024):
        T, G, K = 499, 16, 128
        cg = E // G
        gd = asr.grouped_conv1d_desc(E, E, K, G, K // 2, K // 2 - 1, "gelu")
        x, Wp, bp, y = Buf(uni((T * B, E))), Buf(uni((K * cg, E), (K * cg) ** -.5)), Buf(uni((E, 1), .1)), Buf(
            torch.empty((T * B, E), device=dev))
        variants[f"grouped_conv_E{E}_B{B}"] = (
            lambda x=x, Wp=Wp, bp=bp, y=y, gd=gd, B=B, T=T: asr.grouped_conv1d_fwd(x, Wp, bp, y, T, B, gd, res=x),
            dict(flop=2 * T * B * E * cg * K))
        tx = x.t.view(T, B, E).permute(1, 2, 0).contiguous()                 # torch's own [B][E][T] layout
        tpw = Wp.t.view(K, cg, E).permute(2, 1, 0).contiguous()
        variants[f"torch_grouped_conv_E{E}_B{B}"] = (
            lambda tx=tx, tpw=tpw, bp=bp, K=K, G=G:
            tx + f.gelu(f.conv1d(tx, tpw, bp.t[:, 0], padding=K // 2, groups=G)[:, :, :-1]), {})
        # one dense asr_conv1d_fwd per group: W of group g as a contiguous [k][cg][cg] block
        cd = asr.conv1d_desc(cg, cg, K, pad_left=K // 2, pad_right=K // 2 - 1)
        wgs = [Buf(Wp.t.view(K, cg, E)[:, :, g * cg:(g + 1) * cg].contiguous().view(K * cg, cg)) for g in range(G)]
        bgs = [Buf(bp.t[g * cg:(g + 1) * cg].contiguous()) for g in range(G)]

        def per_group(x=x, y=y, wgs=wgs, bgs=bgs, cd=cd, B=B, T=T, E=E, cg=cg, G=G):
            for g in range(G):
                asr.conv1d_fwd(asr.ColumnView(x, g * cg), wgs[g], bgs[g], y, T, B, cd, col=g * cg)
            asr.layernorm_gelu_fwd(y, y, T, B, E, norm=False)
            asr.check(asr.lib().asr_matadd(x.ptr, y.ptr, y.ptr, T * B, E, 1.0, None), "asr_matadd")
        variants[f"conv1d_x16_gelu_add_E{E}_B{B}"] = (per_group, {})
    # (c) the whole encoder
    if not a.skip_encoder:
        for name, kw in (("base", dict(mode="group", hidden=768, heads=12, layers=12, inter=3072)),
                         ("large", dict(mode="layer", stable=True, hidden=1024, heads=16, layers=24, inter=4096))):
            m = w2v.StandIn(conv_dim=(512,) * 7, conv_stride=(5, 2, 2, 2, 2, 2, 2), conv_kernel=(10, 3, 3, 3, 3, 2, 2),
                            pos_k=128, pos_groups=16, vocab=32, conv_bias=kw["mode"] == "layer", **kw)
            enc = asr.Wav2Vec2Encoder.from_transformers(m)
            m = m.to(dev)
            variants[f"encoder_{name}_B{B}"] = (lambda enc=enc, wave=wave: enc.forward(wave), {})
            variants[f"torch_eager_{name}_B{B}"] = (lambda m=m, wave=wave: [m(w) for w in wave.t], {})

times = {k: [] for k in variants}
for r in range(a.warmup + a.rounds):
    for name, (call, _) in variants.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if r >= a.warmup:
            times[name].append(e0.elapsed_time(e1))
for name, (_, extra) in variants.items():
    med = statistics.median(times[name])
    rec = dict(variant=name, median_ms=round(med, 4), min_ms=round(min(times[name]), 4), rounds=a.rounds, **extra)
    if "out_bytes" in extra:
        rec["store_GBps"] = round(extra["out_bytes"] / med / 1e6, 1)
    if "flop" in extra:
        rec["TFLOPs"] = round(extra["flop"] / med / 1e9, 2)
    print(json.dumps(rec), flush=True)
