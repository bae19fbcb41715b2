"""Time of the word mode of the LM-fused CTC beam search (asr_ctc_lm_create_word:
a word-level LM fused through a lexicon trie, csrc/ctc_lm.hip) in both lexicon
modes, against the token mode asr_ctc_lm_decode and the plain decoder
asr_ctc_decode on the same emissions in the same call.

Shapes: tools/ctc_lm_bench.py's three (C2's decode B=64, T=500, V=29, beam 50; a
C4 shard B=1024; V=1000, beam 200, B=32, T=200 with top_n=40), the oracle's
synthetic emissions.  Model: tools/lm_bench.py's synthetic trigram tables
(--ngrams n-grams over n / 40 + 1000 tokens).  Lexicon, synthetic: label 0 is the
blank, label V-1 the space, and the model's tokens, most frequent in the
trigrams first, are spelled over the first min(V - 2, 27) letters as the strings
of 1, 2, 3, .. letters in lexicographic order (the frequent words are the short
ones), --words of them (0: every token).  The token mode maps the labels to the
most frequent tokens, as tools/ctc_lm_bench.py does.  Device: HIP events on an
otherwise idle stream around each call, warm-up calls, then the median of
--rounds calls with min and max.  One JSON line per shape, with the mean number
of words (tokens in the token mode) of the best hypotheses.  --oov-log10 is the
model's value of a word outside the lexicon: at the default -100 the open mode
hardly ever ends a word, at -1 it ends about as many as the closed mode.
    python tools/ctc_wordlm_bench.py [--ngrams 100000] [--rounds 11] [--warmup 2] [--oov-log10 -1]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tests"))
from conftest import asr, oracle  # noqa: E402
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ngrams", type=int, default=100000)
ap.add_argument("--words", type=int, default=0)
ap.add_argument("--rounds", type=int, default=11)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--shapes", default="c2,c4,wide")
ap.add_argument("--alpha", type=float, default=0.5)
ap.add_argument("--beta", type=float, default=1.0)
ap.add_argument("--oov-log10", type=float, default=-100.0)
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


def spellings(n, letters):
    """The first n strings over `letters` letters by (length, lexicographic order), as label ids 1 .. letters."""
    out, length = [], 1
    while len(out) < n:
        for i in range(letters ** length):
            if len(out) == n:
                break
            out.append([1 + (i // letters ** (length - 1 - j)) % letters for j in range(length)])
        length += 1
    return out


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
    return [round(x, 3) for x in (statistics.median(ms), min(ms), max(ms))]


dev = torch.device("cuda")
st = torch.cuda.Stream()
rng = np.random.default_rng(0)
text, LV, tri = make_model(rng, a.ngrams)
lm = asr.NGramLM.from_string(text, a.oov_log10)
del text
lm.upload()
info = lm.info()
common = np.argsort(-np.bincount(tri.reshape(-1), minlength=LV), kind="stable")   # token ids, most frequent first
common = common[common >= 2]                                                        # never <s>, </s>
n_words = min(a.words or len(common), len(common))
for name in a.shapes.split(","):
    s = SHAPES[name]
    B, T, V, beam, top_n = s["B"], s["T"], s["V"], s["beam"], s["top_n"]
    emis = oracle.synthetic_emissions(T, B, V)
    d_emis = torch.from_numpy(emis).to(dev)
    lex = asr.Lexicon(spellings(n_words, min(V - 2, 27)), common[:n_words].tolist(), V, V - 1)
    lex.upload()
    tok = np.concatenate([[-1], common[:V - 1]]).astype(np.int32)
    decoders = {"open": asr.CTCLMDecoder.word(V, beam, lm, lex, a.alpha, a.beta, top_n=top_n),
                "closed": asr.CTCLMDecoder.word(V, beam, lm, lex, a.alpha, a.beta, top_n=top_n, closed=True),
                "token": asr.CTCLMDecoder(V, beam, lm, tok, a.alpha, a.beta, top_n=top_n)}
    row = {"shape": name, "B": B, "T": T, "V": V, "beam": beam, "top_n": top_n, "ngrams": info["ngrams"],
           "table_bytes": info["table_bytes"], "lexicon": lex.info(), "alpha": a.alpha, "beta": a.beta,
           "oov_log10": a.oov_log10}
    for mode, dec in decoders.items():
        row[mode + "_ms"] = timed(st, lambda: dec.decode_device(d_emis.data_ptr(), T, B, False, st.cuda_stream),
                                  a.warmup, a.rounds)   # [median, min, max]
        try:
            beams = dec.beams(1)
            row[mode + "_mean_units"] = round(float(np.mean([u[0][4] for u in beams])), 2)   # words or tokens, best
        except asr.AsrError as e:   # an overflow shows here
            row[mode + "_error"] = e.status
    plain = asr.CTCDecoder(V, beam, 0)
    row["plain_ms"] = timed(st, lambda: plain.decode_device(d_emis.data_ptr(), T, B, False, st.cuda_stream),
                            a.warmup, a.rounds)
    plain.best()
    for mode in ("open", "closed"):
        row[mode + "_over_token"] = round(row[mode + "_ms"][0] / row["token_ms"][0], 3)
    print(json.dumps(row), flush=True)
    for dec in decoders.values():
        dec.close()
    plain.close()
    lex.close()
lm.close()
