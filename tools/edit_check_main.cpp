// The host twins of csrc/edit.hip as a stand-alone program for a sanitizer build
// on the CPU (`make -C gpu-accelerated-speech-recognition_amd edcheck` compiles
// csrc/edit.hip and this file with -fsanitize=address,undefined and runs the
// result): the worked examples, lengths 0 and 1024, clamped lengths, bad indices
// and bad group bounds, and every refusal of the four entry points.  Every array
// is a heap buffer of the exact size, so a read or write past an end is an ASan
// report.  No HIP call is made; no GPU is needed or used.
#include "asr_amd.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
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

static std::vector<int32_t> chars(const std::string& s) { return std::vector<int32_t>(s.begin(), s.end()); }

// One pair, each sequence in a buffer of exactly its length.
static void pair(const std::string& a, const std::string& b, int dist, int h, int s, int d, int i) {
    const std::vector<int32_t> ra = chars(a), rb = chars(b);
    int32_t got = -9;
    std::vector<int32_t> ops(4, -9);
    EXPECT(asr_edit_distance_host(ra.data(), (long)ra.size(), nullptr, 1, (int)ra.size(), rb.data(), (long)rb.size(),
                                  nullptr, 1, (int)rb.size(), nullptr, nullptr, 1, &got, ops.data()), ASR_OK);
    EXPECT(got, dist);
    EXPECT(ops[0], h);
    EXPECT(ops[1], s);
    EXPECT(ops[2], d);
    EXPECT(ops[3], i);
}

static void edit_cases() {
    pair("kitten", "sitting", 3, 4, 2, 0, 1);
    pair("ab", "ba", 2, 0, 2, 0, 0);
    pair("abcd", "bcde", 2, 3, 0, 1, 1);
    // lengths 0 and 1024: a NULL-free table of one token still has to exist
    const int L = ASR_EDIT_MAX_LEN;
    std::vector<int32_t> a(L), b(L), one(1, 5);
    for (int i = 0; i < L; i++) {
        a[i] = i % 3;
        b[i] = i % 3;
    }
    int32_t dist = -9;
    std::vector<int32_t> ops(4, -9), len0(1, 0);
    EXPECT(asr_edit_distance_host(a.data(), L, nullptr, 1, L, b.data(), L, nullptr, 1, L, nullptr, nullptr, 1, &dist,
                                  ops.data()), ASR_OK);
    EXPECT(dist, 0);
    EXPECT(ops[0], L);
    EXPECT(asr_edit_distance_host(a.data(), L, nullptr, 1, L, one.data(), 1, len0.data(), 1, 1, nullptr, nullptr, 1,
                                  &dist, ops.data()), ASR_OK);
    EXPECT(dist, L);
    EXPECT(ops[2], L);
    EXPECT(asr_edit_distance_host(one.data(), 0, nullptr, 1, 0, b.data(), L, nullptr, 1, L, nullptr, nullptr, 1, &dist,
                                  ops.data()), ASR_OK);
    EXPECT(dist, L);
    EXPECT(ops[3], L);
    EXPECT(asr_edit_distance_host(one.data(), 0, nullptr, 1, 0, one.data(), 0, nullptr, 1, 0, nullptr, nullptr, 1,
                                  &dist, nullptr), ASR_OK);
    EXPECT(dist, 0);
    for (int i = 0; i < L; i++) b[i] = 7;
    EXPECT(asr_edit_distance_host(a.data(), L, nullptr, 1, L, b.data(), L, nullptr, 1, L, nullptr, nullptr, 1, &dist,
                                  ops.data()), ASR_OK);
    EXPECT(dist, L);
    EXPECT(ops[1], L);

    // clamped lengths, index arrays with duplicates, bad indices
    const int n_ref = 3, n_hyp = 4, ldr = 5, ldh = 6, P = 8;
    std::vector<int32_t> ref(n_ref * ldr), hyp(n_hyp * ldh);
    for (size_t i = 0; i < ref.size(); i++) ref[i] = (int32_t)(i * 7 % 3);
    for (size_t i = 0; i < hyp.size(); i++) hyp[i] = (int32_t)(i * 5 % 3);
    const std::vector<int32_t> rl = {-4, 1000, 3}, hl = {std::numeric_limits<int32_t>::max(), 0, 2,
                                                         std::numeric_limits<int32_t>::min()};
    const std::vector<int32_t> ri = {0, 1, 2, 2, 3, -1, 1, std::numeric_limits<int32_t>::max()};
    const std::vector<int32_t> hi = {0, 0, 3, 3, 0, 0, 4, std::numeric_limits<int32_t>::min()};
    std::vector<int32_t> d(P, -9), o(4 * P, -9);
    EXPECT(asr_edit_distance_host(ref.data(), ldr, rl.data(), n_ref, 5, hyp.data(), ldh, hl.data(), n_hyp, 6, ri.data(),
                                  hi.data(), P, d.data(), o.data()), ASR_OK);
    EXPECT(d[0], 6);   // length -4 -> 0 against the clamped 6
    EXPECT(o[3], 6);
    EXPECT(d[2], 3);   // 3 tokens against length INT_MIN -> 0
    EXPECT(d[3], d[2]);
    for (int p = 4; p < P; p++) {
        EXPECT(d[p], -1);
        for (int q = 0; q < 4; q++) EXPECT(o[4 * p + q], -1);
    }
    EXPECT(asr_edit_distance_host(ref.data(), ldr, nullptr, n_ref, 5, hyp.data(), ldh, nullptr, n_hyp, 6, nullptr,
                                  nullptr, 3, d.data(), nullptr), ASR_OK);
    EXPECT(asr_edit_distance_host(ref.data(), ldr, nullptr, n_ref, 5, hyp.data(), ldh, nullptr, n_hyp, 6, nullptr,
                                  nullptr, 3, nullptr, o.data()), ASR_OK);
}

static void mbr_cases() {
    const int N = 9, ldt = 4, max_len = 4, max_hyps = 3, ldm = 3;
    std::vector<int32_t> tok(N * ldt), len = {4, 0, 2, 9, -1, 3, 4, 1, 2};
    for (size_t i = 0; i < tok.size(); i++) tok[i] = (int32_t)(i * 11 % 4);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const std::vector<double> w = {0.0, -1.0, nan, -inf, -inf, nan, inf, 0.0, 5.0};
    // valid, empty, oversize (3 of 5 rows), one row
    const std::vector<int32_t> gs = {0, 3, 3, 8, 9};
    std::vector<int32_t> dist(N * ldm, -9), best(4, -9);
    std::vector<double> risk(N, -9.0);
    EXPECT(asr_nbest_mbr_host(tok.data(), ldt, len.data(), N, max_len, gs.data(), 4, max_hyps, w.data(), dist.data(),
                              ldm, risk.data(), best.data()), ASR_OK);
    EXPECT(dist[0], 0);
    EXPECT(dist[1], 4);   // 4 tokens against none
    EXPECT(dist[1 * ldm + 0], 4);
    EXPECT(best[1], -1);
    EXPECT(risk[3] == risk[3], 1);
    EXPECT(risk[6] == -9.0 && risk[7] == -9.0, 1);   // beyond the first max_hyps of their group
    EXPECT(dist[6 * ldm], -9);
    EXPECT(best[3], 0);
    EXPECT(risk[8] == 0.0, 1);
    EXPECT(dist[8 * ldm + 1], -9);   // columns >= n are not touched
    // group 2: rows 3, 4, 5 with weights -inf, -inf, NaN: uniform
    EXPECT(risk[3] == (double)(dist[3 * ldm + 1] + dist[3 * ldm + 2]) / 3.0, 1);
    // bad group bounds: each is an empty group, nothing is read or written
    const std::vector<std::vector<int32_t>> bad = {{-1, 2}, {7, 10}, {5, 2}, {std::numeric_limits<int32_t>::min(), 0},
                                                   {0, std::numeric_limits<int32_t>::max()}};
    for (const auto& g : bad) {
        std::vector<int32_t> d2(N * ldm, -9), b2(1, -9);
        std::vector<double> r2(N, -9.0);
        EXPECT(asr_nbest_mbr_host(tok.data(), ldt, len.data(), N, max_len, g.data(), 1, max_hyps, w.data(), d2.data(),
                                  ldm, r2.data(), b2.data()), ASR_OK);
        EXPECT(b2[0], -1);
        for (int32_t v : d2) EXPECT(v, -9);
        for (double v : r2) EXPECT(v == -9.0, 1);
    }
    // uniform weights, NULL lengths, each output alone; one +inf weight
    EXPECT(asr_nbest_mbr_host(tok.data(), ldt, nullptr, N, max_len, gs.data(), 4, max_hyps, nullptr, dist.data(), ldm,
                              risk.data(), nullptr), ASR_OK);
    EXPECT(asr_nbest_mbr_host(tok.data(), ldt, nullptr, N, max_len, gs.data(), 4, max_hyps, nullptr, dist.data(), ldm,
                              nullptr, best.data()), ASR_OK);
    const std::vector<int32_t> tail = {6, 9};
    EXPECT(asr_nbest_mbr_host(tok.data(), ldt, len.data(), N, max_len, tail.data(), 1, max_hyps, w.data(), dist.data(),
                              ldm, risk.data(), best.data()), ASR_OK);
    EXPECT(best[0], 0);   // row 6 carries the +inf
    EXPECT(risk[6] == 0.0 && risk[7] == (double)dist[7 * ldm + 0], 1);
    // the largest group at the longest length
    {
        const int n = ASR_MBR_MAX_HYPS, L = ASR_EDIT_MAX_LEN;
        std::vector<int32_t> t((size_t)n * L), g2 = {0, n}, d2((size_t)n * n), b2(1);
        for (size_t i = 0; i < t.size(); i++) t[i] = (int32_t)((i / L + i % L) % 5);
        std::vector<int32_t> l2(n, 0);
        for (int k = 0; k < n; k++) l2[k] = k < 4 ? L : k % 9;   // a few long rows keep this quick
        std::vector<double> r2(n);
        EXPECT(asr_nbest_mbr_host(t.data(), L, l2.data(), n, L, g2.data(), 1, n, nullptr, d2.data(), n, r2.data(),
                                  b2.data()), ASR_OK);
        EXPECT(d2[0 * n + 1], d2[1 * n + 0]);
        EXPECT(b2[0] >= 0 && b2[0] < n, 1);
    }
}

static void refusals() {
    std::vector<int32_t> t(16, 0), out(16, 0);
    std::vector<double> r(4, 0.0);
    int32_t* p = t.data();
    int32_t* o = out.data();
    // asr_edit_distance_host and asr_edit_distance share the checks; the device entry
    // point is refused before any HIP call
#define BOTH_ED(want, ...)                                                 \
    do {                                                                   \
        EXPECT(asr_edit_distance_host(__VA_ARGS__), want);                 \
        EXPECT(asr_edit_distance(__VA_ARGS__, nullptr), want);             \
    } while (0)
    BOTH_ED(ASR_ERR_ARG, nullptr, 4, p, 4, 4, p, 4, p, 4, 4, p, p, 4, o, o);
    BOTH_ED(ASR_ERR_ARG, p, 4, p, 4, 4, nullptr, 4, p, 4, 4, p, p, 4, o, o);
    BOTH_ED(ASR_ERR_ARG, p, 4, p, 4, 4, p, 4, p, 4, 4, p, p, 0, o, o);
    BOTH_ED(ASR_ERR_ARG, p, 4, p, 4, 4, p, 4, p, 4, 4, p, p, -1, o, o);
    BOTH_ED(ASR_ERR_ARG, p, 4, p, 0, 4, p, 4, p, 4, 4, p, p, 4, o, o);
    BOTH_ED(ASR_ERR_ARG, p, 4, p, 4, 4, p, 4, p, -3, 4, p, p, 4, o, o);
    BOTH_ED(ASR_ERR_ARG, p, 3, p, 4, 4, p, 4, p, 4, 4, p, p, 4, o, o);
    BOTH_ED(ASR_ERR_ARG, p, 4, p, 4, 4, p, 3, p, 4, 4, p, p, 4, o, o);
    BOTH_ED(ASR_ERR_ARG, p, 4, p, 4, 4, p, 4, p, 4, 4, p, p, 4, nullptr, nullptr);
    BOTH_ED(ASR_ERR_ARG, p, 4, p, 4, 4, p, 4, p, 4, 4, nullptr, p, 5, o, o);
    BOTH_ED(ASR_ERR_ARG, p, 4, p, 4, 4, p, 4, p, 4, 4, p, nullptr, 5, o, o);
    BOTH_ED(ASR_ERR_UNSUPPORTED, p, 1025, p, 4, 1025, p, 4, p, 4, 4, p, p, 4, o, o);
    BOTH_ED(ASR_ERR_UNSUPPORTED, p, 4, p, 4, 4, p, 1025, p, 4, 1025, p, p, 4, o, o);
    BOTH_ED(ASR_ERR_UNSUPPORTED, p, 4, p, 4, -1, p, 4, p, 4, 4, p, p, 4, o, o);
    BOTH_ED(ASR_ERR_UNSUPPORTED, p, 4, p, 4, 4, p, 4, p, 4, -1, p, p, 4, o, o);
    BOTH_ED(ASR_ERR_ARG, p, 4, p, 4, 4, p, 4, p, 4, 1025, p, p, 4, o, o);   // ARG (ldh) before UNSUPPORTED
#undef BOTH_ED
    double* rk = r.data();
#define BOTH_MBR(want, ...)                                            \
    do {                                                               \
        EXPECT(asr_nbest_mbr_host(__VA_ARGS__), want);                 \
        EXPECT(asr_nbest_mbr(__VA_ARGS__, nullptr), want);             \
    } while (0)
    BOTH_MBR(ASR_ERR_ARG, nullptr, 4, p, 4, 4, p, 1, 2, rk, o, 2, rk, o);
    BOTH_MBR(ASR_ERR_ARG, p, 4, p, 4, 4, nullptr, 1, 2, rk, o, 2, rk, o);
    BOTH_MBR(ASR_ERR_ARG, p, 4, p, 4, 4, p, 1, 2, rk, nullptr, 2, rk, o);
    BOTH_MBR(ASR_ERR_ARG, p, 4, p, 0, 4, p, 1, 2, rk, o, 2, rk, o);
    BOTH_MBR(ASR_ERR_ARG, p, 4, p, 4, 4, p, 0, 2, rk, o, 2, rk, o);
    BOTH_MBR(ASR_ERR_ARG, p, 4, p, 4, 4, p, -1, 2, rk, o, 2, rk, o);
    BOTH_MBR(ASR_ERR_ARG, p, 4, p, 4, 4, p, 1, 0, rk, o, 2, rk, o);
    BOTH_MBR(ASR_ERR_ARG, p, 3, p, 4, 4, p, 1, 2, rk, o, 2, rk, o);
    BOTH_MBR(ASR_ERR_ARG, p, 4, p, 4, 4, p, 1, 2, rk, o, 1, rk, o);
    BOTH_MBR(ASR_ERR_ARG, p, 4, p, 4, 4, p, 1, 2, rk, o, 2, nullptr, nullptr);
    BOTH_MBR(ASR_ERR_UNSUPPORTED, p, 1025, p, 4, 1025, p, 1, 2, rk, o, 2, rk, o);
    BOTH_MBR(ASR_ERR_UNSUPPORTED, p, 4, p, 4, -1, p, 1, 2, rk, o, 2, rk, o);
    BOTH_MBR(ASR_ERR_UNSUPPORTED, p, 4, p, 4, 4, p, 1, 257, rk, o, 257, rk, o);
    BOTH_MBR(ASR_ERR_ARG, p, 4, p, 4, 4, p, 1, 257, rk, o, 256, rk, o);   // ARG (ldm) before UNSUPPORTED
#undef BOTH_MBR
}

int main() {
    edit_cases();
    mbr_cases();
    refusals();
    if (failures) {
        std::printf("edit check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("edit check: ok\n");
    return 0;
}
