// Stand-alone check of the token-and-duration transducer's host code (make
// rnnttdtcheck, ASan + UBSan, CPU only, no HIP call): random small decodes of
// the fp64 twin asr_rnnt_greedy_tdt_host in heap buffers of the exact size
// against a restatement of the walk written here (column-wise dot products,
// long double sums, k descending: another summation order), the same decodes
// truncated (max_out below the count, max_out = 0) and cut into chunks with the
// state and the frame skip carried in place, and every refusal of the
// asr_rnnt_*tdt* entry points and of the entry points that take no TDT handle.
#define RNNT_CHECK_SEED 38038
#define RNNT_CHECK_BLANK_BIAS 2.0f
#include "rnnt_check_common.h"

#include <algorithm>
#include <cstring>

struct Tdt {
    Model m;
    std::vector<int32_t> dur;
    std::vector<float> wdur, bdur;
};

static int create(const Tdt& x, asr_rnnt_t** h) {
    const asr_rnnt_weights w = x.m.ptrs();
    return asr_rnnt_create_tdt(&x.m.d, &w, (int)x.dur.size(), x.dur.data(), x.wdur.data(), x.bdur.data(), h);
}

static Tdt make_tdt(int V, int blank, int E, int D, int Hp, int L, int J, int act, int ms, std::vector<int32_t> dur) {
    Tdt x;
    x.m = make_model(V, blank, E, D, Hp, L, J, act, ms);
    x.dur = std::move(dur);
    fill(x.wdur, (size_t)J * x.dur.size(), 4.0f * std::sqrt(3.0f / J));
    fill(x.bdur, x.dur.size(), 0.1f);
    return x;
}

// ---- a restatement of the walk: dot products column by column, long double sums
struct Walk {
    std::vector<int> tokens, timesteps, durations;
    std::vector<double> logps, h, c;
    double total = 0, gap = HUGE_VAL, dgap = HUGE_VAL;
    int count = 0, skip = 0;
};
static void head(const std::vector<double>& x, int& k, double& lp, double& gap) {
    k = 0;
    for (size_t v = 1; v < x.size(); v++)
        if (x[v] > x[k]) k = (int)v;
    double second = -HUGE_VAL, se = 0;
    for (size_t v = 0; v < x.size(); v++) {
        if ((int)v != k && x[v] > second) second = x[v];
        se += std::exp(x[v] - x[k]);
    }
    lp = -std::log(se);
    gap = x[k] - second;
}
static Walk ref_walk(const Tdt& x, const float* enc, int T, int B, int b, int len) {
    const Model& m = x.m;
    const asr_rnnt_desc& d = m.d;
    const int nd = (int)x.dur.size();
    Walk w;
    w.h.assign((size_t)d.L * d.Hp, 0.0);
    w.c.assign((size_t)d.L * d.Hp, 0.0);
    ref_step(m, d.blank, w.h, w.c);
    len = len < 0 ? 0 : (len > T ? T : len);
    int t = 0, n = 0;
    while (t < len) {
        std::vector<double> e(enc + ((size_t)t * B + b) * d.E, enc + ((size_t)t * B + b + 1) * d.E);
        std::vector<double> ht(w.h.begin() + (size_t)(d.L - 1) * d.Hp, w.h.end()), z(d.J), logit(d.V), dlogit(nd);
        for (int j = 0; j < d.J; j++) {
            const double v = (dotcol(e, m.wenc.data(), d.E, d.J, j) + (double)m.benc[j]) +
                             (dotcol(ht, m.wpred.data(), d.Hp, d.J, j) + (double)m.bpred[j]);
            z[j] = d.act == ASR_RNNT_ACT_TANH ? std::tanh(v) : (v > 0 ? v : 0);
        }
        for (int v = 0; v < d.V; v++) logit[v] = dotcol(z, m.wout.data(), d.J, d.V, v) + (double)m.bout[v];
        for (int v = 0; v < nd; v++) dlogit[v] = dotcol(z, x.wdur.data(), d.J, nd, v) + (double)x.bdur[v];
        int k, di;
        double lpk, lpd, gk, gd;
        head(logit, k, lpk, gk);
        head(dlogit, di, lpd, gd);
        w.gap = std::min(w.gap, gk);
        w.dgap = std::min(w.dgap, gd);
        w.total += lpk + lpd;
        const int dur = x.dur[di];
        if (k == d.blank) {
            t += dur > 1 ? dur : 1;
            n = 0;
            continue;
        }
        w.tokens.push_back(k);
        w.timesteps.push_back(t);
        w.durations.push_back(dur);
        w.logps.push_back(lpk + lpd);
        w.count++;
        ref_step(m, k, w.h, w.c);
        if (dur > 0 || ++n == d.max_symbols) {
            t += dur > 0 ? dur : 1;
            n = 0;
        }
    }
    w.skip = t - len;
    return w;
}

struct Out {
    std::vector<int32_t> tok, ts, du, cnt, skip;
    std::vector<double> lp, total, gap, dgap, state;
    Out(int B, int mo, size_t nstate)
        : tok((size_t)B * mo), ts((size_t)B * mo), du((size_t)B * mo), cnt(B), skip(B), lp((size_t)B * mo), total(B),
          gap(B), dgap(B), state(nstate) {}
};
static int run(const asr_rnnt_t* h, const float* enc, const int32_t* lens, int T, int B, int mo, const double* sin,
               const int32_t* kin, Out& o, bool gaps = true) {
    return asr_rnnt_greedy_tdt_host(h, enc, lens, T, B, mo, sin, o.state.data(), kin, o.skip.data(),
                                    mo ? o.tok.data() : nullptr, mo ? o.ts.data() : nullptr, mo ? o.du.data() : nullptr,
                                    mo ? o.lp.data() : nullptr, o.cnt.data(), o.total.data(),
                                    gaps ? o.gap.data() : nullptr, gaps ? o.dgap.data() : nullptr);
}

static void random_decodes() {
    std::uniform_int_distribution<int> pick(0, 1 << 20);
    int compared = 0, truncated = 0, jumps = 0;
    for (int iter = 0; iter < 200; iter++) {
        const int V = 2 + pick(rng) % 20, L = 1 + pick(rng) % 2, E = 1 + pick(rng) % 12;
        const int D = 16 * (1 + pick(rng) % 2), Hp = 16 * (1 + pick(rng) % 2), J = 16 * (1 + pick(rng) % 2);
        const int T = 2 + pick(rng) % 7, B = 1 + pick(rng) % 4, ms = 1 + pick(rng) % 3;
        const int blank = iter % 3 == 0 ? 0 : (iter % 3 == 1 ? V - 1 : pick(rng) % V);
        std::vector<int32_t> dur(1 + pick(rng) % 6);
        for (int32_t& v : dur) v = pick(rng) % 5;
        dur[pick(rng) % dur.size()] = 1 + pick(rng) % 4;   // one entry advances
        const Tdt x = make_tdt(V, blank, E, D, Hp, L, J, pick(rng) % 2, ms, dur);
        asr_rnnt_t* h = nullptr;
        EXPECT(create(x, &h), ASR_OK);
        if (!h) continue;
        std::vector<float> enc;
        fill(enc, (size_t)T * B * E, 1.0f);
        std::vector<int32_t> len(B);
        for (int b = 0; b < B; b++) len[b] = pick(rng) % (T + 3) - 1;   // -1 .. T + 1: clamped
        const int32_t* lens = iter % 4 == 0 ? nullptr : len.data();
        const int full = T * ms;
        const size_t nstate = 2 * (size_t)L * B * Hp, half = (size_t)L * B * Hp;
        Out o(B, full, nstate);
        EXPECT(run(h, enc.data(), lens, T, B, full, nullptr, nullptr, o), ASR_OK);
        for (int b = 0; b < B; b++) {
            const Walk w = ref_walk(x, enc.data(), T, B, b, lens ? lens[b] : T);
            if (!(w.gap > 1e-6 && w.dgap > 1e-6)) continue;   // a near-tie: the two summation orders may part
            compared++;
            EXPECT(o.cnt[b], w.count);
            EXPECT(o.skip[b], w.skip);
            EXPECT_TRUE(close(o.total[b], w.total));
            EXPECT_TRUE(close(o.gap[b], w.gap) || (o.gap[b] == HUGE_VAL && w.gap == HUGE_VAL));
            EXPECT_TRUE(close(o.dgap[b], w.dgap) || (o.dgap[b] == HUGE_VAL && w.dgap == HUGE_VAL));
            for (int i = 0; i < w.count && i < o.cnt[b]; i++) {
                EXPECT(o.tok[(size_t)b * full + i], w.tokens[i]);
                EXPECT(o.ts[(size_t)b * full + i], w.timesteps[i]);
                EXPECT(o.du[(size_t)b * full + i], w.durations[i]);
                EXPECT_TRUE(close(o.lp[(size_t)b * full + i], w.logps[i]));
            }
            for (size_t n = 0; n < (size_t)L * Hp; n++) {
                const size_t l = n / Hp, k = n % Hp;
                EXPECT_TRUE(close(o.state[(l * B + b) * Hp + k], w.h[n]));
                EXPECT_TRUE(close(o.state[half + (l * B + b) * Hp + k], w.c[n]));
            }
        }
        // truncation: the count goes on, the records stop, the state and the skip are the untruncated ones
        for (int mo : {0, 1}) {
            Out t(B, mo, nstate);
            EXPECT(run(h, enc.data(), lens, T, B, mo, nullptr, nullptr, t, false), ASR_OK);
            EXPECT_TRUE(t.cnt == o.cnt && t.skip == o.skip && t.state == o.state && t.total == o.total);
            for (int b = 0; b < B && mo; b++)
                if (o.cnt[b] > 0) {
                    truncated++;
                    EXPECT(t.tok[b], o.tok[(size_t)b * full]);
                    EXPECT(t.du[b], o.du[(size_t)b * full]);
                    EXPECT_TRUE(t.lp[b] == o.lp[(size_t)b * full]);
                }
        }
        // two chunks at every cut, the state and the skip carried (the skip in place): the whole decode's records
        for (int cut = 1; cut < T; cut++) {
            std::vector<int32_t> l1(B), l2(B);
            for (int b = 0; b < B; b++) {
                const int lb = lens ? std::min(std::max(lens[b], 0), T) : T;
                l1[b] = std::min(lb, cut);
                l2[b] = std::max(lb - cut, 0);
            }
            Out c1(B, full, nstate), c2(B, full, nstate);
            EXPECT(run(h, enc.data(), l1.data(), cut, B, full, nullptr, nullptr, c1), ASR_OK);
            for (int b = 0; b < B; b++) jumps += c1.skip[b] > 0;
            c2.skip = c1.skip;
            EXPECT(run(h, enc.data() + (size_t)cut * B * E, l2.data(), T - cut, B, full, c1.state.data(), c2.skip.data(),
                       c2), ASR_OK);
            EXPECT_TRUE(c2.state == o.state && c2.skip == o.skip);
            for (int b = 0; b < B; b++) {
                EXPECT(c1.cnt[b] + c2.cnt[b], o.cnt[b]);
                for (int i = 0; i < o.cnt[b] && i < c1.cnt[b] + c2.cnt[b]; i++) {
                    const bool first = i < c1.cnt[b];
                    const Out& c = first ? c1 : c2;
                    const size_t j = (size_t)b * full + (first ? i : i - c1.cnt[b]), k = (size_t)b * full + i;
                    EXPECT(c.tok[j], o.tok[k]);
                    EXPECT(c.ts[j] + (first ? 0 : cut), o.ts[k]);
                    EXPECT(c.du[j], o.du[k]);
                    EXPECT_TRUE(c.lp[j] == o.lp[k]);
                }
            }
        }
        asr_rnnt_destroy(h);
    }
    EXPECT_TRUE(compared > 100 && truncated > 50 && jumps > 20);
    std::printf("rnnt_tdt_check: %d walks compared, %d truncated, %d cuts inside a jump\n", compared, truncated, jumps);
}

static void refusals() {
    const int V = 9, E = 8, D = 16, Hp = 16, J = 16, T = 5, B = 2;
    const Tdt x = make_tdt(V, 0, E, D, Hp, 1, J, ASR_RNNT_ACT_RELU, 2, {0, 1, 2});
    const asr_rnnt_weights w = x.m.ptrs();
    asr_rnnt_t* h = nullptr;
    // asr_rnnt_create_tdt, in the documented order
    EXPECT(asr_rnnt_create_tdt(nullptr, &w, 3, x.dur.data(), x.wdur.data(), x.bdur.data(), &h), ASR_ERR_ARG);
    EXPECT(asr_rnnt_create_tdt(&x.m.d, nullptr, 3, x.dur.data(), x.wdur.data(), x.bdur.data(), &h), ASR_ERR_ARG);
    EXPECT(asr_rnnt_create_tdt(&x.m.d, &w, 3, nullptr, x.wdur.data(), x.bdur.data(), &h), ASR_ERR_ARG);
    EXPECT(asr_rnnt_create_tdt(&x.m.d, &w, 3, x.dur.data(), nullptr, x.bdur.data(), &h), ASR_ERR_ARG);
    EXPECT(asr_rnnt_create_tdt(&x.m.d, &w, 3, x.dur.data(), x.wdur.data(), nullptr, &h), ASR_ERR_ARG);
    EXPECT(asr_rnnt_create_tdt(&x.m.d, &w, 3, x.dur.data(), x.wdur.data(), x.bdur.data(), nullptr), ASR_ERR_ARG);
    EXPECT(asr_rnnt_create_tdt(&x.m.d, &w, 0, x.dur.data(), x.wdur.data(), x.bdur.data(), &h), ASR_ERR_ARG);
    EXPECT(asr_rnnt_create_tdt(&x.m.d, &w, ASR_RNNT_TDT_MAX_DURATIONS + 1, x.dur.data(), x.wdur.data(), x.bdur.data(),
                               &h), ASR_ERR_ARG);
    for (std::vector<int32_t> bad : {std::vector<int32_t>{0, 0, 0}, {0, -1, 2}, {0, 1, 32768}}) {
        EXPECT(asr_rnnt_create_tdt(&x.m.d, &w, 3, bad.data(), x.wdur.data(), x.bdur.data(), &h), ASR_ERR_ARG);
        EXPECT_TRUE(h == nullptr);
    }
    {
        Tdt y = x;   // asr_rnnt_create's checks follow: a range, a multiple of 16, the LDS limit, a NULL weight
        y.m.d.max_symbols = 0;
        EXPECT(create(y, &h), ASR_ERR_ARG);
        y = x;
        y.m.d.Hp = 24;
        EXPECT(create(y, &h), ASR_ERR_UNSUPPORTED);
        y = x;
        y.m.d.Hp = y.m.d.J = 832;   // beyond the LDS limit (816); refused before a weight is read
        EXPECT(create(y, &h), ASR_ERR_UNSUPPORTED);
        asr_rnnt_weights nw = w;
        nw.w_out = nullptr;
        EXPECT(asr_rnnt_create_tdt(&x.m.d, &nw, 3, x.dur.data(), x.wdur.data(), x.bdur.data(), &h), ASR_ERR_ARG);
        EXPECT_TRUE(h == nullptr);
    }
    EXPECT(create(x, &h), ASR_OK);
    asr_rnnt_t* hp = nullptr;
    EXPECT(asr_rnnt_create(&x.m.d, &w, &hp), ASR_OK);
    int32_t tab[ASR_RNNT_TDT_MAX_DURATIONS] = {};
    EXPECT(asr_rnnt_tdt_durations(h, tab), 3);
    EXPECT_TRUE(tab[0] == 0 && tab[1] == 1 && tab[2] == 2);
    EXPECT(asr_rnnt_tdt_durations(h, nullptr), 3);
    EXPECT(asr_rnnt_tdt_durations(hp, tab), 0);
    EXPECT(asr_rnnt_tdt_durations(nullptr, tab), 0);
    EXPECT_TRUE(asr_rnnt_workspace_bytes(h, T, B) == asr_rnnt_workspace_bytes(hp, T, B));
    asr_rnnt_info info{};
    EXPECT(asr_rnnt_get_info(h, &info), ASR_OK);
    EXPECT(info.desc.V, V);
    EXPECT_TRUE(info.weight_bytes > 0 && info.uploaded == 0);

    std::vector<float> enc;
    fill(enc, (size_t)T * B * E, 1.0f);
    const int mo = T * 2;
    std::vector<int32_t> tok(B * mo), ts(B * mo), du(B * mo), cnt(B), bl(B * 2), nh(B);
    std::vector<double> lp(B * mo), tot(B), sc(B * 2);
    int dummy_ = 0;
    void* dummy = &dummy_;
    // the entry points of the one-softmax lattice refuse the TDT handle
    EXPECT(asr_rnnt_greedy(h, enc.data(), nullptr, T, B, mo, nullptr, nullptr, tok.data(), ts.data(), lp.data(),
                           cnt.data(), tot.data(), dummy, nullptr), ASR_ERR_UNSUPPORTED);
    EXPECT(asr_rnnt_greedy_host(h, enc.data(), nullptr, T, B, mo, nullptr, nullptr, tok.data(), ts.data(), lp.data(),
                                cnt.data(), tot.data(), nullptr), ASR_ERR_UNSUPPORTED);
    EXPECT(asr_rnnt_greedy_stateless(h, enc.data(), nullptr, T, B, mo, nullptr, nullptr, tok.data(), ts.data(),
                                     lp.data(), cnt.data(), tot.data(), dummy, nullptr), ASR_ERR_UNSUPPORTED);
    EXPECT(asr_rnnt_greedy_stateless_host(h, enc.data(), nullptr, T, B, mo, nullptr, nullptr, tok.data(), ts.data(),
                                          lp.data(), cnt.data(), tot.data(), nullptr), ASR_ERR_UNSUPPORTED);
    EXPECT(asr_rnnt_beam(h, enc.data(), nullptr, T, B, 2, 2, T, tok.data(), ts.data(), bl.data(), sc.data(), nh.data(),
                         dummy, nullptr), ASR_ERR_UNSUPPORTED);
    EXPECT(asr_rnnt_beam_host(h, enc.data(), nullptr, T, B, 2, 2, T, tok.data(), ts.data(), bl.data(), sc.data(),
                              nh.data(), nullptr), ASR_ERR_UNSUPPORTED);
    std::vector<int32_t> tgt = {1, 2}, tl = {1, 1};
    EXPECT(asr_rnnt_align(h, enc.data(), nullptr, T, B, tgt.data(), 1, tl.data(), nullptr, B, 1,
                          ASR_RNNT_LATTICE_STANDARD, tot.data(), nullptr, nullptr, dummy, nullptr), ASR_ERR_UNSUPPORTED);
    EXPECT(asr_rnnt_align_host(h, enc.data(), nullptr, T, B, tgt.data(), 1, tl.data(), nullptr, B, 1,
                               ASR_RNNT_LATTICE_STANDARD, tot.data(), nullptr, nullptr), ASR_ERR_UNSUPPORTED);
    // the TDT pair: asr_rnnt_greedy's checks in its order, then the kind, then the work area and the upload
    auto dev = [&](const asr_rnnt_t* hh, const float* e, int t, int b, int m, int32_t* d, void* work) {
        return asr_rnnt_greedy_tdt(hh, e, nullptr, t, b, m, nullptr, nullptr, nullptr, nullptr, tok.data(), ts.data(), d,
                                   lp.data(), cnt.data(), tot.data(), work, nullptr);
    };
    EXPECT(dev(nullptr, enc.data(), T, B, mo, du.data(), dummy), ASR_ERR_ARG);
    EXPECT(dev(h, nullptr, T, B, mo, du.data(), dummy), ASR_ERR_ARG);
    EXPECT(dev(h, enc.data(), 0, B, mo, du.data(), dummy), ASR_ERR_ARG);
    EXPECT(dev(h, enc.data(), T, 0, mo, du.data(), dummy), ASR_ERR_ARG);
    EXPECT(dev(h, enc.data(), T, B, -1, du.data(), dummy), ASR_ERR_ARG);
    EXPECT(dev(h, enc.data(), T, B, mo, nullptr, dummy), ASR_ERR_ARG);       // max_out > 0 without a durations array
    EXPECT(dev(h, enc.data(), 1 << 30, 4, mo, du.data(), dummy), ASR_ERR_UNSUPPORTED);   // T * B > INT_MAX
    EXPECT(dev(hp, enc.data(), T, B, mo, du.data(), dummy), ASR_ERR_UNSUPPORTED);        // a plain handle
    EXPECT(dev(h, enc.data(), T, B, mo, du.data(), nullptr), ASR_ERR_ARG);
    EXPECT(dev(h, enc.data(), T, B, mo, du.data(), dummy), ASR_ERR_STATE);
    EXPECT(asr_rnnt_greedy_tdt_host(hp, enc.data(), nullptr, T, B, mo, nullptr, nullptr, nullptr, nullptr, tok.data(),
                                    ts.data(), du.data(), lp.data(), cnt.data(), tot.data(), nullptr, nullptr),
           ASR_ERR_UNSUPPORTED);
    EXPECT(asr_rnnt_greedy_tdt_host(h, enc.data(), nullptr, T, B, mo, nullptr, nullptr, nullptr, nullptr, tok.data(),
                                    ts.data(), nullptr, lp.data(), cnt.data(), tot.data(), nullptr, nullptr),
           ASR_ERR_ARG);
    // a skip at or beyond the length: the chunk is skipped whole, nothing is evaluated
    std::vector<int32_t> len = {3, 5}, skip = {3, 9};
    EXPECT(asr_rnnt_greedy_tdt_host(h, enc.data(), len.data(), T, B, 0, nullptr, nullptr, skip.data(), skip.data(),
                                    nullptr, nullptr, nullptr, nullptr, cnt.data(), tot.data(), nullptr, nullptr), ASR_OK);
    EXPECT_TRUE(skip[0] == 0 && skip[1] == 4 && cnt[0] == 0 && cnt[1] == 0 && tot[0] == 0.0 && tot[1] == 0.0);
    asr_rnnt_destroy(h);
    asr_rnnt_destroy(hp);
}

int main() {
    random_decodes();
    refusals();
    if (failures) {
        std::printf("rnnt_tdt_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("rnnt_tdt_check: ok\n");
    return 0;
}
