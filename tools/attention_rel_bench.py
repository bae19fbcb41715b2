"""Time of asr_attention_rel_fwd at the shapes of tools/attention_bench.py
(T, B, E, heads; lengths ragged between T/2 and T):
    s144   250, 64, 144, 4     full mask
    s256   250, 64, 256, 4     full mask
    s512   500, 64, 512, 8     full mask
    chunk  500, 64, 256, 4     chunk 16, left 4, right 0
Three columns per shape (HIP events around --iters back-to-back calls, warm-up,
then interleaved rounds; median, min and max of the rounds' per-call times):
    rel      asr_attention_rel_fwd with both biases and a projected table
    plain    asr_attention_fwd on the same Q, K, V: the difference is the price of the position term
    torch    the toolkits' eager fp32 formulation on the device: matrix_ac, matrix_bd over the 2T - 1 table, the
             pad-and-view rel_shift, masked softmax, @ v (building the mask is not in its time)
and, with --layer, one ConformerLayer.forward at (T, B, E, heads, F, kernel) = (200, 64, 256, 4, 1024, 31)
with MultiheadAttention and with RelPositionMultiheadAttention.
The largest difference between rel and torch on valid rows is printed with each
shape (a check, not a benchmark).

No shape lives in a module-level name: bench_shape() and bench_layer() get
theirs as arguments, build every buffer and closure from them and assert each
input's rows before timing.  Without --child the tool runs one child process
per shape under its own time limit and stops at the first that fails.
    python tools/attention_rel_bench.py [--shapes s144 s256 s512 chunk] [--layer] [--rounds 11] [--warmup 2] [--iters 50]
"""
import argparse
import json
import statistics
import subprocess
import sys
import types
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tests"))

SHAPES = {   # T, B, E, heads, chunk, left, right
    "s144": (250, 64, 144, 4, 1, -1, -1),
    "s256": (250, 64, 256, 4, 1, -1, -1),
    "s512": (500, 64, 512, 8, 1, -1, -1),
    "chunk": (500, 64, 256, 4, 16, 4, 0),
}
LAYER = (200, 64, 256, 4, 1024, 31)


def view(t, rows, cols):
    assert t.is_contiguous() and t.numel() == rows * cols, (tuple(t.shape), rows, cols)
    return types.SimpleNamespace(ptr=t.data_ptr(), rows=rows, cols=cols, keep=t)


def timed(variants, st, rounds, warmup, iters):
    """{name: per-call ms of each round}: warm-up, then every variant once per round."""
    import torch
    torch.cuda.synchronize()
    for _ in range(warmup):
        for call in variants.values():
            call()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, call in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(iters):
                call()
            e1.record(st)
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / iters)
    return ms


def report(ms, rec, rounds, base=None):
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, v in ms.items():
        row = {**rec, "variant": k, "rounds": rounds, "ms": round(med[k], 4), "ms_min": round(min(v), 4),
               "ms_max": round(max(v), 4)}
        if base and k != base:
            row["ratio_to_" + base] = round(med[k] / med[base], 3)
        print(json.dumps(row), flush=True)


def bench_shape(name, T, B, E, heads, chunk, left, right, rounds, warmup, iters):
    from conftest import asr
    import torch
    dev, D = torch.device("cuda"), E // heads
    torch.manual_seed(0)
    st = torch.cuda.Stream()
    lens = np.random.default_rng(T + E).integers(T // 2, T + 1, B)
    lens[0] = T
    fr = np.arange(T)
    win = np.ones((T, T), bool)
    if left >= 0:
        win &= fr[None, :] // chunk >= fr[:, None] // chunk - left
    if right >= 0:
        win &= fr[None, :] // chunk <= fr[:, None] // chunk + right
    valid = fr[None, :] < lens[:, None]                                        # [B][T]
    allowed = win[None] & valid[:, None, :] & valid[:, :, None]                # [B][Tq][Tk]
    qkv = torch.rand((T * B, 3 * E), device=dev) * 2 - 1
    out, outp = torch.zeros((T * B, E), device=dev), torch.zeros((T * B, E), device=dev)
    dl = torch.from_numpy(lens.astype(np.int32)).to(dev)
    desc = asr.attn_desc(heads, D, 0.0, chunk, left, right)
    # the projected table of all 2T - 1 distances (what the toolkits pass), distance 0 at row T - 1
    table = torch.rand((2 * T - 1, E), device=dev) * 2 - 1
    bu, bv = (torch.rand(E, device=dev) - 0.5 for _ in range(2))
    mq, mo, mop, mt = view(qkv, T * B, 3 * E), view(out, T * B, E), view(outp, T * B, E), view(table, 2 * T - 1, E)
    assert mq.rows == T * B and mo.rows == T * B and mop.rows == T * B and mt.rows == 2 * T - 1
    cols = [asr.ColumnView(mq, i * E) for i in range(3)]
    lv, vu, vv = (types.SimpleNamespace(ptr=t.data_ptr()) for t in (dl, bu, bv))
    # torch: [B][h][T][d] views of the same values; padded queries keep themselves visible (no NaN rows)
    tq, tk, tv = (qkv[:, i * E:(i + 1) * E].reshape(T, B, heads, D).permute(1, 2, 0, 3).contiguous() for i in range(3))
    tp = table.view(2 * T - 1, heads, D).permute(1, 2, 0).contiguous()         # [h][d][2T - 1]
    tmask = ~torch.from_numpy(allowed | (~valid[:, :, None] & np.eye(T, dtype=bool)[None]))[:, None].to(dev)
    hu, hv = bu.view(1, heads, 1, D), bv.view(1, heads, 1, D)
    res = {}

    def eager():
        with torch.cuda.stream(st), torch.no_grad():
            ac = torch.matmul(tq + hu, tk.transpose(-2, -1))
            bd = torch.matmul(tq + hv, tp)                                     # [B][h][T][2T - 1]
            pad = torch.cat([bd.new_zeros((B, heads, T, 1)), bd], dim=-1).view(B, heads, 2 * T, T)
            bd = pad[:, :, 1:].view_as(bd)[:, :, :, :T]
            s = ((ac + bd) / D ** 0.5).masked_fill(tmask, -float("inf"))
            res["o"] = torch.matmul(torch.softmax(s, dim=-1), tv)

    variants = {
        "rel": lambda: asr.attention_rel_fwd(*cols, mo, T, T, B, desc, mt, T - 1, vu, vv, lengths=lv,
                                             stream=st.cuda_stream),
        "plain": lambda: asr.attention_fwd(*cols, mop, T, T, B, desc, lengths=lv, stream=st.cuda_stream),
        "torch": eager,
    }
    ms = timed(variants, st, rounds, warmup, iters)
    mine = out.reshape(T, B, heads, D).permute(1, 2, 0, 3)
    diff = ((mine - res["o"]).abs() * torch.from_numpy(valid).to(dev)[:, None, :, None]).max().item()
    print(json.dumps({"shape": name, "max_abs_diff_rel_to_torch_on_valid_rows": diff}), flush=True)
    rec = {"shape": name, "T": T, "B": B, "E": E, "heads": heads, "chunk": chunk, "left": left, "right": right,
           "visible_pairs": int(allowed.sum())}
    report(ms, rec, rounds, base="plain")


def bench_layer(T, B, E, heads, F, kernel, rounds, warmup, iters):
    from conftest import asr
    import attention_rel_reference as atr
    import conformer_reference as cf
    import torch
    st = torch.cuda.Stream()
    block = cf.make_block((T, B, E, heads, F, kernel))
    parts = block.explicit_parts()
    torch.manual_seed(1)
    rel_parts = dict(parts, attn=(parts["attn"][0], atr.RelPositionAttention(E, heads)))
    layers = {"layer/plain": asr.ConformerLayer.from_torch(**parts), "layer/rel": asr.ConformerLayer.from_torch(**rel_parts)}
    lens = np.random.default_rng(T + E).integers(T // 2, T + 1, B)
    lens[0] = T
    dl = asr.device_lengths(lens)
    x = asr.DeviceMatrix.from_numpy(cf.draw_x(T, B, E).reshape(T * B, E))
    assert (x.rows, x.cols) == (T * B, E)
    keep = {}

    def call(k):
        keep[k] = layers[k].forward(x, T, B, lengths=dl, stream=st.cuda_stream)

    ms = timed({k: (lambda k=k: call(k)) for k in layers}, st, rounds, warmup, iters)
    report(ms, {"T": T, "B": B, "E": E, "heads": heads, "F": F, "kernel": kernel}, rounds, base="layer/plain")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--layer", action="store_true", help="also time one ConformerLayer.forward with and without")
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=50, help="calls per timed window")
    ap.add_argument("--limit", type=int, default=240, help="seconds each child process may take")
    ap.add_argument("--child", help="run this one shape (or 'layer') in this process")
    a = ap.parse_args()
    if a.rounds < 10:
        sys.exit("--rounds: at least 10 timed runs")
    if a.child == "layer":
        return bench_layer(*LAYER, a.rounds, a.warmup, a.iters)
    if a.child:
        return bench_shape(a.child, *SHAPES[a.child], a.rounds, a.warmup, a.iters)
    for name in a.shapes + (["layer"] if a.layer else []):
        cmd = [sys.executable, __file__, "--child", name, "--rounds", str(a.rounds), "--warmup", str(a.warmup),
               "--iters", str(a.iters)]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"{name}: no result within {a.limit} s; nothing more is started")
        if rc != 0:
            sys.exit(f"{name}: the child ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
