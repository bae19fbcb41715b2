"""Time of the LM-fused CTC beam search (asr_ctc_lm_decode, csrc/ctc_lm.hip)
against the plain decoder asr_ctc_decode on the same emissions (the existing
kernels: the baseline) and against the one-thread host twin
asr_ctc_lm_decode_host.

Shapes: C2's decode (B=64, T=500, V=29, beam 50), a C4 shard (B=1024, T=500,
V=29, beam 50) and V=1000, beam 200, B=32, T=200 with top_n=40; emissions are
the oracle's synthetic ones.  Models: tools/lm_bench.py's synthetic trigram
tables (100000 and 4000000 n-grams: 2.7 MB and 108 MB), the labels mapped to the
tokens that occur most often in the trigrams.  Device: HIP events on an
otherwise idle stream around each call, warm-up calls, then the median of
--rounds calls with min and max.  Host: wall clock around the twin on the first
--host-utts utterances (it takes seconds per utterance), one warm-up, the median
of --host-rounds calls, scaled to the batch; only on shapes listed in
--host-shapes.  One JSON line per shape and model.  The kernel counts no LM
lookups, so none are printed.
    python tools/ctc_lm_bench.py [--ngrams 100000,4000000] [--rounds 11] [--warmup 2]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tests"))
from conftest import asr, oracle  # noqa: E402
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ngrams", default="100000,4000000")
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--host-rounds", type=int, default=3)
ap.add_argument("--host-utts", type=int, default=1)
ap.add_argument("--host-shapes", default="c2")
ap.add_argument("--shapes", default="c2,c4,wide")
ap.add_argument("--alpha", type=float, default=0.5)
ap.add_argument("--beta", type=float, default=1.0)
a = ap.parse_args()
if a.rounds < 10:
    sys.exit("--rounds: at least 10 timed runs")

SHAPES = {"c2": dict(B=64, T=500, V=29, beam=50, top_n=0),
          "c4": dict(B=1024, T=500, V=29, beam=50, top_n=0),
          "wide": dict(B=32, T=200, V=1000, beam=200, top_n=40)}
W = 7


def digits(x, w):
    out = np.empty((len(x), w), np.uint8)
    for j in range(w):
        out[:, w - 1 - j] = 48 + (x // 10 ** j) % 10
    return out


def char(n, c):
    return np.full((n, 1), ord(c), np.uint8)


def section(k, grams, rng, backoff):
    n = len(grams)
    p = rng.integers(1, 60000, n)
    cols = [char(n, "-"), digits(p // 10000, 1), char(n, "."), digits(p % 10000, 4)]
    for j in range(k):
        cols += [char(n, "\t" if j == 0 else " "), digits(grams[:, j], W)]
    if backoff:
        cols += [char(n, "\t"), char(n, "-"), char(n, "0"), char(n, "."), digits(rng.integers(0, 1000, n), 3)]
    cols.append(char(n, "\n"))
    return np.concatenate(cols, axis=1).tobytes()


def make_model(rng, n_grams):
    """tools/lm_bench.py's synthetic trigram model: n_grams / 3 bigrams and the
    rest trigrams over n_grams / 40 + 1000 words; ids 0 and 1 are <s>, </s>."""
    V = n_grams // 40 + 1000
    nb, nt = n_grams // 3, n_grams - n_grams // 3
    key = np.unique(rng.integers(2, V, nb) * V + rng.integers(2, V, nb))
    bi = np.stack([key // V, key % V], axis=1)
    key = np.unique(key[rng.integers(0, len(key), nt)] * V + rng.integers(2, V, nt))
    tri = np.stack([key // (V * V), key // V % V, key % V], axis=1)
    uni = np.arange(2, V)[:, None]
    text = b"".join([
        ("\\data\\\nngram 1=%d\nngram 2=%d\nngram 3=%d\n\n\\1-grams:\n-2.5\t<s>\t-0.5\n-2.5\t</s>\n"
         % (V, len(bi), len(tri))).encode(),
        section(1, uni, rng, True), b"\n\\2-grams:\n", section(2, bi, rng, True),
        b"\n\\3-grams:\n", section(3, tri, rng, False), b"\n\\end\\\n"])
    return text, V, tri


def timed(st, run, warmup, rounds):
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        run()
        e1.record(st)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


dev = torch.device("cuda")
st = torch.cuda.Stream()
rng = np.random.default_rng(0)
for n_grams in [int(x) for x in a.ngrams.split(",")]:
    text, LV, tri = make_model(rng, n_grams)
    lm = asr.NGramLM.from_string(text)
    del text
    lm.upload()
    info = lm.info()
    common = np.argsort(-np.bincount(tri.reshape(-1), minlength=LV), kind="stable")   # token ids, most frequent first
    for name in a.shapes.split(","):
        s = SHAPES[name]
        B, T, V, beam, top_n = s["B"], s["T"], s["V"], s["beam"], s["top_n"]
        emis = oracle.synthetic_emissions(T, B, V)
        d_emis = torch.from_numpy(emis).to(dev)
        tok = np.concatenate([[-1], common[:V - 1]]).astype(np.int32)
        fused = asr.CTCLMDecoder(V, beam, lm, tok, a.alpha, a.beta, top_n=top_n)
        plain = asr.CTCDecoder(V, beam, 0)
        f = timed(st, lambda: fused.decode_device(d_emis.data_ptr(), T, B, False, st.cuda_stream), a.warmup, a.rounds)
        fused.beams(1)   # an overflow would show here
        p = timed(st, lambda: plain.decode_device(d_emis.data_ptr(), T, B, False, st.cuda_stream), a.warmup, a.rounds)
        plain.best()
        row = {"shape": name, "B": B, "T": T, "V": V, "beam": beam, "top_n": top_n, "ngrams": info["ngrams"],
               "table_bytes": info["table_bytes"], "alpha": a.alpha, "beta": a.beta,
               "fused_ms": round(f[0], 3), "fused_ms_min": round(f[1], 3), "fused_ms_max": round(f[2], 3),
               "plain_ms": round(p[0], 3), "plain_ms_min": round(p[1], 3), "plain_ms_max": round(p[2], 3),
               "fused_over_plain": round(f[0] / p[0], 2)}
        if name in a.host_shapes.split(","):
            nu = min(a.host_utts, B)
            sub = np.ascontiguousarray(emis[:, :nu])
            host_ms = []
            for r in range(a.host_rounds + 1):
                h0 = time.perf_counter()
                fused.decode_host(sub, is_log=False)
                if r:
                    host_ms.append((time.perf_counter() - h0) * 1e3)
            hm = statistics.median(host_ms) * B / nu
            row.update({"host_utts_timed": nu, "host_ms_scaled_to_B": round(hm, 1),
                        "host_over_fused": round(hm / f[0], 1)})
        print(json.dumps(row), flush=True)
        fused.close()
        plain.close()
    lm.close()
