// What the stand-alone transducer check programs share (rnnt_check_main.cpp,
// rnnt_beam_check_main.cpp, rnnt_lm_check_main.cpp, rnnt_align_check_main.cpp):
// EXPECT, a random model and the restatement of the predictor step (column-wise
// dot products, long double sums, k descending: another summation order than
// the twins').  A program defines RNNT_CHECK_SEED (the seed of its generator)
// and RNNT_CHECK_BLANK_BIAS (b_out at the blank) before it includes this file.
#pragma once
#include "asr_amd.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

static int failures = 0;
#define EXPECT(expr, want)                                                              \
    do {                                                                                \
        const long got_ = (long)(expr);                                                 \
        if (got_ != (long)(want)) {                                                     \
            std::printf("FAIL %s:%d %s: got %ld, want %ld\n", __FILE__, __LINE__, #expr, got_, (long)(want)); \
            failures++;                                                                 \
        }                                                                               \
    } while (0)
#define EXPECT_TRUE(expr) EXPECT(!!(expr), 1)

struct Model {
    asr_rnnt_desc d;
    std::vector<float> emb, wih[2], whh[2], bih[2], bhh[2], wenc, benc, wpred, bpred, wout, bout;
    asr_rnnt_weights ptrs() const {
        asr_rnnt_weights w{};
        w.emb = emb.data();
        for (int l = 0; l < d.L && l < 2; l++) {
            w.w_ih[l] = wih[l].data();
            w.w_hh[l] = whh[l].data();
            w.b_ih[l] = bih[l].data();
            w.b_hh[l] = bhh[l].data();
        }
        w.w_enc = wenc.data(); w.b_enc = benc.data();
        w.w_pred = wpred.data(); w.b_pred = bpred.data();
        w.w_out = wout.data(); w.b_out = bout.data();
        return w;
    }
};

static std::mt19937 rng(RNNT_CHECK_SEED);
static void fill(std::vector<float>& v, size_t n, float bound) {
    std::uniform_real_distribution<float> u(-bound, bound);
    v.resize(n);
    for (float& x : v) x = u(rng);
}

static Model make_model(int V, int blank, int E, int D, int Hp, int L, int J, int act, int max_symbols = 1) {
    Model m;
    m.d = asr_rnnt_desc{V, blank, E, D, Hp, L, J, act, max_symbols};
    const float k = 1.0f / std::sqrt((float)Hp);
    fill(m.emb, (size_t)V * D, 1.0f);
    for (int l = 0; l < L && l < 2; l++) {
        fill(m.wih[l], (size_t)(l ? Hp : D) * 4 * Hp, k);
        fill(m.whh[l], (size_t)Hp * 4 * Hp, k);
        fill(m.bih[l], 4 * (size_t)Hp, k);
        fill(m.bhh[l], 4 * (size_t)Hp, k);
    }
    fill(m.wenc, (size_t)E * J, std::sqrt(3.0f / E));
    fill(m.benc, J, 0.1f);
    fill(m.wpred, (size_t)Hp * J, 4.0f * std::sqrt(3.0f / Hp));
    fill(m.bpred, J, 0.1f);
    fill(m.wout, (size_t)J * V, 4.0f * std::sqrt(3.0f / J));
    fill(m.bout, V, 0.1f);
    m.bout[blank] = RNNT_CHECK_BLANK_BIAS;
    return m;
}

static double dotcol(const std::vector<double>& x, const float* W, int K, int N, int n) {
    long double s = 0;
    for (int k = K - 1; k >= 0; k--) s += (long double)x[k] * (long double)W[(size_t)k * N + n];
    return (double)s;
}
static double sigm(double v) { return 1.0 / (1.0 + std::exp(-v)); }
static void ref_step(const Model& m, int tok, std::vector<double>& h, std::vector<double>& c) {
    const int Hp = m.d.Hp;
    std::vector<double> x(m.emb.begin() + (size_t)tok * m.d.D, m.emb.begin() + (size_t)(tok + 1) * m.d.D);
    for (int l = 0; l < m.d.L; l++) {
        std::vector<double> hl(h.begin() + (size_t)l * Hp, h.begin() + (size_t)(l + 1) * Hp), z(4 * Hp);
        for (int n = 0; n < 4 * Hp; n++)
            z[n] = (dotcol(x, m.wih[l].data(), (int)x.size(), 4 * Hp, n) + dotcol(hl, m.whh[l].data(), Hp, 4 * Hp, n)) +
                   ((double)m.bih[l][n] + (double)m.bhh[l][n]);
        x.resize(Hp);
        for (int n = 0; n < Hp; n++) {
            const double cn = sigm(z[Hp + n]) * c[(size_t)l * Hp + n] + sigm(z[n]) * std::tanh(z[2 * Hp + n]);
            c[(size_t)l * Hp + n] = cn;
            x[n] = h[(size_t)l * Hp + n] = sigm(z[3 * Hp + n]) * std::tanh(cn);
        }
    }
}

// The candidate order of the beam searches (the two beam programs use it): score descending, then the index;
// a NaN after every number.
[[maybe_unused]] static bool before(double sa, long ia, double sb, long ib) {
    if (sa > sb) return true;
    if (sa < sb) return false;
    const bool na = sa != sa, nb = sb != sb;
    if (na != nb) return nb;
    return ia < ib;
}

static bool close(double a, double b) { return std::fabs(a - b) <= 1e-9 * (1.0 + std::fabs(b)); }
