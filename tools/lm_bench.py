"""Time of asr_lm_score (back-off n-gram LM scoring, csrc/lm.hip) against the
one-thread host scorer asr_lm_score_host on the same tables.

Synthetic trigram models of three sizes — a table that sits in one XCD's L2
(4 MiB), one in the Infinity Cache (256 MiB) and one beyond it — and two
workloads: N = 2048 x 50 hypotheses (the final beam of a C4 batch) and
N = 64 x 50, lengths near 40.  Three quarters of the hypotheses are chains of
the model's own trigrams (deep matches and back-offs both occur), the rest
random ids.  Device: HIP events on an otherwise idle stream around each call,
warm-up calls, then the median of --rounds calls.  Host: wall clock around
asr_lm_score_host, one warm-up, the median of --host-rounds calls.  One JSON
line per model and workload; "speedup" is host ms over device ms.
    python tools/lm_bench.py [--ngrams 100000,4000000,12000000] [--rounds 11] [--warmup 2] [--host-rounds 3]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tests"))
from conftest import asr  # noqa: E402
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ngrams", default="100000,4000000,12000000", help="bigrams + trigrams of each model")
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--host-rounds", type=int, default=3)
ap.add_argument("--length", type=int, default=40)
a = ap.parse_args()
if a.rounds < 10:
    sys.exit("--rounds: at least 10 timed runs")
W = 7   # digits of a token's name (its id, zero-padded)


def digits(x, w):
    out = np.empty((len(x), w), np.uint8)
    for j in range(w):
        out[:, w - 1 - j] = 48 + (x // 10 ** j) % 10
    return out


def char(n, c):
    return np.full((n, 1), ord(c), np.uint8)


def section(k, grams, rng, backoff):
    """The lines of a \\k-grams: section as bytes: -d.dddd <tab> tokens [<tab> -0.ddd]."""
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
    """ARPA bytes of a trigram model with n_grams / 3 bigrams and 2 n_grams / 3
    trigrams (prefix-closed, not suffix-closed) over n_grams / 40 + 1000 words;
    ids 0 and 1 are <s> and </s>, token i >= 2 is named by its id."""
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


def make_hyps(rng, V, tri, N, length):
    lens = np.clip(rng.integers(length - 8, length + 9, N), 0, None).astype(np.int32)
    max_len = int(lens.max())
    chains = tri[rng.integers(0, len(tri), (N, max_len // 3 + 1))].reshape(N, -1)[:, :max_len]
    rand = rng.integers(2, V, (N, max_len))
    tok = np.where((np.arange(N) % 4 == 0)[:, None], rand, chains).astype(np.int32)
    return np.ascontiguousarray(tok), lens, max_len


dev = torch.device("cuda")
st = torch.cuda.Stream()
rng = np.random.default_rng(0)
flags = asr.ASR_LM_BOS | asr.ASR_LM_EOS
for n_grams in [int(x) for x in a.ngrams.split(",")]:
    t0 = time.perf_counter()
    text, V, tri = make_model(rng, n_grams)
    t1 = time.perf_counter()
    lm = asr.NGramLM.from_string(text)
    t2 = time.perf_counter()
    del text
    lm.upload()
    info = lm.info()
    for N in (2048 * 50, 64 * 50):
        tok, lens, max_len = make_hyps(rng, V, tri, N, a.length)
        d_tok, d_len = torch.from_numpy(tok).to(dev), torch.from_numpy(lens).to(dev)
        d_logp = torch.empty(N, dtype=torch.float64, device=dev)

        def run():
            asr.check(asr.lib().asr_lm_score(lm.h, d_tok.data_ptr(), max_len, d_len.data_ptr(), N, max_len, flags,
                                             d_logp.data_ptr(), None, None, None, 0, st.cuda_stream), "asr_lm_score")

        for _ in range(a.warmup):
            run()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            run()
            e1.record(st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        h_logp = np.zeros(N, np.float64)
        host_ms = []
        for r in range(a.host_rounds + 1):
            h0 = time.perf_counter()
            asr.check(asr.lib().asr_lm_score_host(lm.h, tok.ctypes.data, max_len, lens.ctypes.data, N, max_len, flags,
                                                  h_logp.ctypes.data, None, None, None, 0), "asr_lm_score_host")
            if r:
                host_ms.append((time.perf_counter() - h0) * 1e3)
        same = bool((d_logp.cpu().numpy().view(np.int64) == h_logp.view(np.int64)).all())
        med, hmed = statistics.median(ms), statistics.median(host_ms)
        tokens = int(lens.sum()) + N
        print(json.dumps({"ngrams": info["ngrams"], "nodes_inserted": info["nodes_inserted"],
                          "table_bytes": info["table_bytes"], "N": N, "tokens": tokens, "device_ms": round(med, 4),
                          "device_ms_min": round(min(ms), 4), "device_ms_max": round(max(ms), 4),
                          "host_ms": round(hmed, 2), "speedup": round(hmed / med, 1),
                          "device_tokens_per_s": round(tokens / med * 1e3), "bit_equal_to_host": same,
                          "generate_s": round(t1 - t0, 1), "load_s": round(t2 - t1, 1)}), flush=True)
        if not same:
            sys.exit("device and host totals differ")
    lm.close()
