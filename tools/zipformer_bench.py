"""Time of the Zipformer layer and of asr_attention_zip_fwd's two forms against
torch eager on the device, at (T, B, E, heads, dq, dp, dv, ff, kernel) =
(250, 32, 384, 8, 32, 4, 12, 1536, 31), lengths ragged between T/2 and T:
    layer      asr.ZipformerLayer.forward
    torch      the stand-in layer of tests/zipformer_reference.py on the device in fp32 (it materialises the
               [H][B][T][T] probabilities once and uses them three times)
    head       asr_attention_zip_fwd, per-head form (dv = 12), one call
    wide       asr_attention_zip_fwd, wide gated form (dv = 3E/4 = 288, score head 0), one call
    plain      asr_attention_fwd at head_dim 32 on the same q, k: what the scores alone cost
HIP events around --iters back-to-back calls, warm-up, then interleaved rounds;
median, min and max of the rounds' per-call times, one JSON line per variant.
    python tools/zipformer_bench.py [--rounds 11] [--warmup 2] [--iters 20]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tests"))

SHAPE = dict(T=250, B=32, E=384, H=8, dq=32, dp=4, dv=12, ff=1536, kernel=31, pos_dim=48)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20, help="calls per timed window")
    a = ap.parse_args()
    if a.rounds < 10:
        sys.exit("--rounds: at least 10 timed runs")
    import torch
    import zipformer_reference as zr
    from conftest import asr
    s = SHAPE
    T, B, E, H, dq, dp, dv = (s[k] for k in ("T", "B", "E", "H", "dq", "dp", "dv"))
    hid, dev, st = 3 * E // 4, torch.device("cuda"), torch.cuda.Stream()
    mod = zr.StandInLayer(E, H, dq, dp, dv, (s["ff"],) * 3, s["kernel"], s["pos_dim"])
    layer = asr.ZipformerLayer.from_torch(mod)
    lens = np.random.default_rng(T + E).integers(T // 2, T + 1, B)
    lens[0] = T
    dl = asr.device_lengths(lens)
    xh = np.random.default_rng(0).uniform(-1, 1, (T, B, E)).astype(np.float32)
    pos = asr.compact_rel_positional_encoding(T, s["pos_dim"])
    x, dpos = asr.DeviceMatrix.from_numpy(xh.reshape(T * B, E)), asr.DeviceMatrix.from_numpy(pos)
    tmod, tx, tpos = mod.to(dev), torch.from_numpy(xh).to(dev), torch.from_numpy(pos).to(dev)
    valid = np.arange(T)[None, :] < lens[:, None]
    allowed = torch.from_numpy(np.broadcast_to(valid[:, None, :], (B, T, T)).copy()).to(dev)
    keep = torch.from_numpy(valid.T[:, :, None].copy()).to(dev)
    rnd = lambda n: asr.DeviceMatrix.from_numpy(np.random.default_rng(n).uniform(-1, 1, (T * B, n)).astype(np.float32))   # noqa: E731
    q, k, pz, v12, u3 = rnd(H * dq), rnd(H * dq + 1), rnd(H * dp), rnd(H * dv), rnd(3 * hid)
    k = asr.ColumnView(k, 1)
    table = asr.DeviceMatrix.from_numpy(np.random.default_rng(3).uniform(-1, 1, (2 * T - 1, H * dp)).astype(np.float32))
    o12, ow, op = asr.DeviceMatrix(T * B, H * dv), asr.DeviceMatrix(T * B, hid), asr.DeviceMatrix(T * B, H * dq)
    dh = asr.zattn_desc(H, dq, dp, dv, scale=1.0)
    dw = asr.zattn_desc(H, dq, dp, hid, value_heads=1, scale=1.0, gate=True)
    res = {}

    def eager():
        with torch.cuda.stream(st), torch.no_grad():
            res["t"] = tmod(tx, tpos, allowed, keep)

    cs = st.cuda_stream
    variants = {
        "layer": lambda: res.__setitem__("l", layer.forward(x, T, B, dpos, T - 1, dl, stream=cs)),
        "torch": eager,
        "head": lambda: asr.attention_zip_fwd(q, k, v12, o12, T, T, B, dh, pz=pz, pos=table, pos_zero=T - 1, lengths=dl,
                                              stream=cs),
        "wide": lambda: asr.attention_zip_fwd(q, k, asr.ColumnView(u3, hid), ow, T, T, B, dw, pz=pz, pos=table,
                                              pos_zero=T - 1, sg=u3, y=asr.ColumnView(u3, 2 * hid), lengths=dl, stream=cs),
        "plain": lambda: asr.attention_fwd(q, k, q, op, T, T, B, asr.attn_desc(H, dq, 1.0), lengths=dl, stream=cs),
    }
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        for call in variants.values():
            call()
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, call in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.iters):
                call()
            e1.record(st)
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.iters)
    got = res["l"].toCpu().reshape(T, B, E)
    diff = np.abs(got - res["t"].cpu().numpy())[valid.T].max()
    print(json.dumps({"max_abs_diff_layer_to_torch_on_valid_rows": float(diff)}), flush=True)
    for name, vals in ms.items():
        print(json.dumps({**s, "variant": name, "rounds": a.rounds, "iters": a.iters,
                          "ms": round(statistics.median(vals), 4), "ms_min": round(min(vals), 4),
                          "ms_max": round(max(vals), 4)}), flush=True)


if __name__ == "__main__":
    main()
