"""Pure-Python reference of the back-off n-gram LM contract of include/asr_amd.h
(asr_lm_*): an ARPA reader into dicts, the recursion written literally, and a
generator of random ARPA models (prefix-closed, deliberately not suffix-closed).

Values are np.float32 as read; a token's value is a Python float (fp64) built
from 0.0 by adding, left to right, the back-offs from the longest context
downward (0.0 for an absent context) and then P — the library's order."""
import numpy as np

BOS, EOS = 1, 2


class ArpaModel:
    def __init__(self, text):
        self.tokens = []                 # id -> string, in \1-grams: order
        self.ids = {}
        self.prob = {}                   # tuple of ids -> np.float32
        self.backoff = {}                # tuple of ids -> np.float32
        self.counts = {}
        self.order = 0
        section = None
        seen_data = False
        for raw in text.splitlines():
            line = raw.strip()
            if not line:
                continue
            if not seen_data:
                seen_data = line == "\\data\\"
                continue
            if line == "\\end\\":
                break
            if line.startswith("ngram "):
                k, n = line[6:].split("=")
                self.counts[int(k)] = int(n)
                continue
            if line.startswith("\\"):
                section = int(line[1:line.index("-")])
                continue
            f = line.split()
            assert len(f) in (section + 1, section + 2), line
            if section == 1:
                self.ids[f[1]] = len(self.tokens)
                self.tokens.append(f[1])
            key = tuple(self.ids[t] for t in f[1:1 + section])
            assert key not in self.prob, line
            self.prob[key] = np.float32(f[0])
            self.backoff[key] = np.float32(f[section + 1]) if len(f) == section + 2 else np.float32(0.0)
            self.order = max(self.order, section)
        self.vocab = len(self.tokens)
        self.bos = self.ids.get("<s>", -1)
        self.eos = self.ids.get("</s>", -1)
        self.unk = self.ids.get("<unk>", -1)

    # p(w | h) by the recursion: returns (terms, matched order); terms are the
    # back-offs met on the way down, then P.
    def _cond(self, h, w):
        terms = []
        while True:
            if h + (w,) in self.prob:
                terms.append(float(self.prob[h + (w,)]))
                return terms, len(h) + 1
            terms.append(float(self.backoff[h]) if h in self.prob else 0.0)
            h = h[1:]

    def score(self, tokens, flags, oov_log10=-100.0):
        """(total, [n scored, n oov], per-token values, per-token orders); the
        total is the library's: 64 partial sums (position i into partial i % 64)
        reduced in its fixed tree."""
        seq = []
        n_oov = 0
        if flags & BOS:
            assert self.bos >= 0
            seq.append(("ctx", self.bos))
        for t in tokens:
            t = int(t)
            if t < 0 or t >= self.vocab:
                n_oov += 1
                seq.append(("tok", self.unk) if self.unk >= 0 else ("oov", -1))
            else:
                seq.append(("tok", t))
        if flags & EOS:
            assert self.eos >= 0
            seq.append(("tok", self.eos))
        values, orders = [], []
        for i, (kind, w) in enumerate(seq):
            if kind == "ctx":
                continue
            if kind == "oov":
                values.append(float(np.float32(oov_log10)))
                orders.append(0)
                continue
            h = []
            for j in range(i - 1, -1, -1):
                if len(h) == self.order - 1 or seq[j][0] == "oov":
                    break
                h.insert(0, seq[j][1])
            terms, q = self._cond(tuple(h), w)
            v = 0.0
            for x in terms:
                v += x
            values.append(v)
            orders.append(q)
        part = [0.0] * 64
        for i, v in enumerate(values):
            part[i % 64] += v
        off = 32
        while off >= 1:
            for l in range(off):
                part[l] += part[l + off]
            off //= 2
        return part[0], [len(values), n_oov], values, orders


def _fmt(x):
    return "%.9g" % float(x)   # 9 significant digits: exactly the fp32 back


def random_arpa(rng, vocab, order, ngrams, bos=True, eos=True, unk=False, low=-4.0):
    """ARPA text of a random model: `vocab` ordinary tokens w0.. plus the chosen
    special ones, ngrams[k-2] n-grams of order k = 2 .. order.  Prefix-closed
    (an n-gram of order k extends an existing one of order k-1 by a word on the
    right) and NOT suffix-closed (nothing makes (w2..wk) exist)."""
    names = ["w%d" % i for i in range(vocab)]
    if bos:
        names.insert(int(rng.integers(0, len(names) + 1)), "<s>")
    if eos:
        names.insert(int(rng.integers(0, len(names) + 1)), "</s>")
    if unk:
        names.insert(int(rng.integers(0, len(names) + 1)), "<unk>")
    V = len(names)
    bos_id = names.index("<s>") if bos else -1
    eos_id = names.index("</s>") if eos else -1
    levels = [[(i,) for i in range(V)]]
    for k in range(2, order + 1):
        want = ngrams[k - 2]
        prev = [g for g in levels[-1] if g[-1] != eos_id]   # nothing follows </s>
        got = set()
        tries = 0
        while len(got) < want and prev and tries < 50 * want + 100:
            tries += 1
            g = prev[int(rng.integers(0, len(prev)))]
            w = int(rng.integers(0, V))
            if w == bos_id:
                continue
            got.add(g + (w,))
        levels.append(sorted(got, key=lambda g: rng.random()))
    while len(levels) > 1 and not levels[-1]:
        levels.pop()
    out = ["", "\\data\\"]
    for k, lv in enumerate(levels, 1):
        out.append("ngram %d=%d" % (k, len(lv)))
    for k, lv in enumerate(levels, 1):
        out.append("")
        out.append("\\%d-grams:" % k)
        for g in lv:
            p = np.float32(rng.uniform(low, 0.0))
            line = _fmt(p) + "\t" + " ".join(names[i] for i in g)
            if k < len(levels) and rng.random() < 0.8:
                line += "\t" + _fmt(np.float32(rng.uniform(-2.0, 0.5)))
            out.append(line)
    out += ["", "\\end\\", ""]
    return "\n".join(out)


def windowed_arpa(rng, vocab, order, seqs, extra, low=-4.0):
    """ARPA text of a model of the given order over w0.. with <s> and </s> that
    is hit at every order: its n-grams of order k = 2 .. order are every window
    of k tokens of <s> seq </s> for each seq of `seqs` (lists of indices into
    w0..), and beside them extra[k-2] random ones made as random_arpa makes
    them.  Well formed: the prefix of a window is a window, and a random n-gram
    extends an n-gram of the order below on the right."""
    names = ["w%d" % i for i in range(vocab)]
    names.insert(int(rng.integers(0, len(names) + 1)), "<s>")
    names.insert(int(rng.integers(0, len(names) + 1)), "</s>")
    V = len(names)
    bos_id, eos_id = names.index("<s>"), names.index("</s>")
    rows = [[bos_id] + [names.index("w%d" % int(t)) for t in s] + [eos_id] for s in seqs]
    levels = [[(i,) for i in range(V)]]
    for k in range(2, order + 1):
        got = {tuple(r[i:i + k]) for r in rows for i in range(len(r) - k + 1)}
        prev = [g for g in levels[-1] if g[-1] != eos_id]   # nothing follows </s>
        want = len(got) + extra[k - 2]
        tries = 0
        while len(got) < want and prev and tries < 50 * want + 100:
            tries += 1
            g = prev[int(rng.integers(0, len(prev)))]
            w = int(rng.integers(0, V))
            if w == bos_id:
                continue
            got.add(g + (w,))
        levels.append(sorted(sorted(got), key=lambda g: rng.random()))
    out = ["", "\\data\\"]
    for k, lv in enumerate(levels, 1):
        out.append("ngram %d=%d" % (k, len(lv)))
    for k, lv in enumerate(levels, 1):
        out.append("")
        out.append("\\%d-grams:" % k)
        for g in lv:
            line = _fmt(np.float32(rng.uniform(low, 0.0))) + "\t" + " ".join(names[i] for i in g)
            if k < len(levels) and rng.random() < 0.8:
                line += "\t" + _fmt(np.float32(rng.uniform(-2.0, 0.5)))
            out.append(line)
    out += ["", "\\end\\", ""]
    return "\n".join(out)


def random_hypotheses(rng, model_vocab, lengths, oov_rate=0.0):
    """Token lists of the given lengths over [0, vocab); with oov_rate > 0 some
    ids are -1, vocab or beyond."""
    hyps = []
    for L in lengths:
        t = rng.integers(0, model_vocab, size=L).astype(np.int64)
        if oov_rate > 0 and L:
            bad = rng.random(L) < oov_rate
            t[bad] = rng.choice([-1, model_vocab, model_vocab + 7, -5], size=int(bad.sum()))
        hyps.append(t.tolist())
    return hyps
