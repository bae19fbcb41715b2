// Host-side checks of csrc/ctc_prefix.hip as a stand-alone program for a
// sanitizer build on the CPU (`make -C gpu-accelerated-speech-recognition_amd
// ctcprefixcheck` compiles csrc/ctc_prefix.hip and this file with
// -fsanitize=address,undefined and runs the result): every refusal of
// asr_ctc_prefix_begin, asr_ctc_prefix_score and asr_ctc_prefix_advance in the
// documented order (fake device pointers that are never dereferenced; where a
// call has two faults the earlier check must answer).  No GPU is needed or used.
#include "asr_amd.h"

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>

static int failures = 0;
#define EXPECT(expr, want)                                                              \
    do {                                                                                \
        const long got_ = (long)(expr);                                                 \
        if (got_ != (long)(want)) {                                                     \
            std::printf("FAIL %s: got %ld, want %ld\n", #expr, got_, (long)(want));     \
            failures++;                                                                 \
        }                                                                               \
    } while (0)

static float* const F = reinterpret_cast<float*>(0x10000);       // never dereferenced
static float* const F2 = reinterpret_cast<float*>(0x20000);
static int32_t* const L = reinterpret_cast<int32_t*>(0x30000);
static int32_t* const L2 = reinterpret_cast<int32_t*>(0x40000);
static double* const D[6] = {reinterpret_cast<double*>(0x50000), reinterpret_cast<double*>(0x60000),
                             reinterpret_cast<double*>(0x70000), reinterpret_cast<double*>(0x80000),
                             reinterpret_cast<double*>(0x90000), reinterpret_cast<double*>(0xa0000)};

static asr_ctc_prefix_desc base() {
    asr_ctc_prefix_desc d{};
    d.B = 3; d.K = 4; d.V = 11; d.T = 8; d.blank = 0; d.eos = 10; d.ctc_weight = 0.3; d.length_bonus = 0.0;
    return d;
}

// The three entry points on one descriptor: 0 begin, 1 score (with d_att), 2 advance.
static int call(int which, const asr_ctc_prefix_desc& d, long ld = 11, long ld_att = 11, long ldo = 11) {
    if (which == 0) return asr_ctc_prefix_begin(&d, F, ld, L, D[0], D[1], D[2], L2, nullptr);
    if (which == 1)
        return asr_ctc_prefix_score(&d, F, ld, L, D[0], D[1], D[2], L, D[3], L, F2, ld_att, F2, ldo, nullptr);
    return asr_ctc_prefix_advance(&d, F, ld, L, L, L, D[0], D[1], D[2], L, D[3], D[4], D[5], L2, nullptr);
}

static void nulls() {
    const asr_ctc_prefix_desc d = base();
    // begin: every pointer in turn
    void* b[7] = {F, L, D[0], D[1], D[2], L2, nullptr};
    for (int i = 0; i < 6; i++) {
        void* a[7];
        for (int j = 0; j < 7; j++) a[j] = j == i ? nullptr : b[j];
        EXPECT(asr_ctc_prefix_begin(&d, (float*)a[0], 11, (int32_t*)a[1], (double*)a[2], (double*)a[3], (double*)a[4],
                                    (int32_t*)a[5], nullptr), ASR_ERR_ARG);
    }
    EXPECT(asr_ctc_prefix_begin(nullptr, F, 11, L, D[0], D[1], D[2], L2, nullptr), ASR_ERR_ARG);
    // score: every pointer but d_att
    void* s[9] = {F, L, D[0], D[1], D[2], L, D[3], L, F2};
    for (int i = 0; i < 9; i++) {
        void* a[9];
        for (int j = 0; j < 9; j++) a[j] = j == i ? nullptr : s[j];
        EXPECT(asr_ctc_prefix_score(&d, (float*)a[0], 11, (int32_t*)a[1], (double*)a[2], (double*)a[3], (double*)a[4],
                                    (int32_t*)a[5], (double*)a[6], (int32_t*)a[7], F2, 11, (float*)a[8], 11, nullptr),
               ASR_ERR_ARG);
    }
    EXPECT(asr_ctc_prefix_score(nullptr, F, 11, L, D[0], D[1], D[2], L, D[3], L, F2, 11, F2, 11, nullptr), ASR_ERR_ARG);
    // advance: every pointer in turn
    void* v[12] = {F, L, L, L, D[0], D[1], D[2], L, D[3], D[4], D[5], L2};
    for (int i = 0; i < 12; i++) {
        void* a[12];
        for (int j = 0; j < 12; j++) a[j] = j == i ? nullptr : v[j];
        EXPECT(asr_ctc_prefix_advance(&d, (float*)a[0], 11, (int32_t*)a[1], (int32_t*)a[2], (int32_t*)a[3],
                                      (double*)a[4], (double*)a[5], (double*)a[6], (int32_t*)a[7], (double*)a[8],
                                      (double*)a[9], (double*)a[10], (int32_t*)a[11], nullptr), ASR_ERR_ARG);
    }
    EXPECT(asr_ctc_prefix_advance(nullptr, F, 11, L, L, L, D[0], D[1], D[2], L, D[3], D[4], D[5], L2, nullptr),
           ASR_ERR_ARG);
}

static void descriptor(int which) {
    asr_ctc_prefix_desc d;
    d = base(); d.B = 0; EXPECT(call(which, d), ASR_ERR_ARG);
    d = base(); d.B = INT_MIN; EXPECT(call(which, d), ASR_ERR_ARG);
    d = base(); d.K = 0; EXPECT(call(which, d), ASR_ERR_ARG);
    d = base(); d.K = ASR_ATTN_BEAM_MAX_K + 1; EXPECT(call(which, d), ASR_ERR_ARG);
    d = base(); d.V = 0; EXPECT(call(which, d, 11), ASR_ERR_ARG);
    d = base(); d.T = 0; EXPECT(call(which, d), ASR_ERR_ARG);
    d = base(); d.T = -8; EXPECT(call(which, d), ASR_ERR_ARG);
    d = base(); d.blank = -1; EXPECT(call(which, d), ASR_ERR_ARG);
    d = base(); d.blank = 11; EXPECT(call(which, d), ASR_ERR_ARG);
    d = base(); d.eos = -1; EXPECT(call(which, d), ASR_ERR_ARG);
    d = base(); d.eos = 11; EXPECT(call(which, d), ASR_ERR_ARG);
    d = base(); d.blank = 10; EXPECT(call(which, d), ASR_ERR_ARG);                 // blank == eos
    d = base(); d.ctc_weight = -0.01; EXPECT(call(which, d), ASR_ERR_ARG);
    d = base(); d.ctc_weight = 1.01; EXPECT(call(which, d), ASR_ERR_ARG);
    d = base(); d.ctc_weight = NAN; EXPECT(call(which, d), ASR_ERR_ARG);
    d = base(); d.length_bonus = INFINITY; EXPECT(call(which, d), ASR_ERR_ARG);
    d = base(); d.length_bonus = NAN; EXPECT(call(which, d), ASR_ERR_ARG);
    d = base(); EXPECT(call(which, d, 10), ASR_ERR_ARG);                           // ld < V
    d = base(); EXPECT(call(which, d, -11), ASR_ERR_ARG);
    d = base(); EXPECT(call(which, d, LONG_MIN), ASR_ERR_ARG);
    // both a bad argument and unsupported: the argument answers
    d = base(); d.B = 65536; EXPECT(call(which, d, 10), ASR_ERR_ARG);
    d = base(); d.B = 1 << 15; d.T = 1 << 15; d.ctc_weight = 2.0; EXPECT(call(which, d), ASR_ERR_ARG);
    // unsupported
    d = base(); d.B = 65536; EXPECT(call(which, d), ASR_ERR_UNSUPPORTED);
    d = base(); d.B = 1 << 15; d.K = 16; d.T = 1 << 13; EXPECT(call(which, d), ASR_ERR_UNSUPPORTED);   // B*K*T = 2^32
    d = base(); d.B = 65535; d.K = 16; d.T = INT_MAX; EXPECT(call(which, d), ASR_ERR_UNSUPPORTED);
    d = base(); d.ctc_weight = 0.0; d.length_bonus = -3.5; d.B = 65536; EXPECT(call(which, d), ASR_ERR_UNSUPPORTED);
    d = base(); d.ctc_weight = 1.0; d.B = 65536; EXPECT(call(which, d), ASR_ERR_UNSUPPORTED);
}

static void own_checks() {
    asr_ctc_prefix_desc d = base();
    // score: the strides of the output and of d_att (ignored without d_att)
    EXPECT(call(1, d, 11, 11, 10), ASR_ERR_ARG);
    EXPECT(call(1, d, 11, 10, 11), ASR_ERR_ARG);
    EXPECT(call(1, d, 11, LONG_MIN, 11), ASR_ERR_ARG);
    d.B = 65536;
    EXPECT(call(1, d, 11, 11, 10), ASR_ERR_ARG);                                   // before unsupported
    EXPECT(asr_ctc_prefix_score(&d, F, 11, L, D[0], D[1], D[2], L, D[3], L, nullptr, 0, F2, 11, nullptr),
           ASR_ERR_UNSUPPORTED);                                                   // no d_att: ld_att is not looked at
    d = base();
    // begin: rn and rb must be two buffers
    EXPECT(asr_ctc_prefix_begin(&d, F, 11, L, D[0], D[0], D[2], L2, nullptr), ASR_ERR_ARG);
    // advance: an out buffer that is an in buffer, or the other out buffer
    EXPECT(asr_ctc_prefix_advance(&d, F, 11, L, L, L, D[0], D[1], D[2], L, D[0], D[4], D[5], L2, nullptr), ASR_ERR_ARG);
    EXPECT(asr_ctc_prefix_advance(&d, F, 11, L, L, L, D[0], D[1], D[2], L, D[1], D[4], D[5], L2, nullptr), ASR_ERR_ARG);
    EXPECT(asr_ctc_prefix_advance(&d, F, 11, L, L, L, D[0], D[1], D[2], L, D[3], D[0], D[5], L2, nullptr), ASR_ERR_ARG);
    EXPECT(asr_ctc_prefix_advance(&d, F, 11, L, L, L, D[0], D[1], D[2], L, D[3], D[1], D[5], L2, nullptr), ASR_ERR_ARG);
    EXPECT(asr_ctc_prefix_advance(&d, F, 11, L, L, L, D[0], D[1], D[2], L, D[3], D[3], D[5], L2, nullptr), ASR_ERR_ARG);
    EXPECT(asr_ctc_prefix_advance(&d, F, 11, L, L, L, D[0], D[1], D[2], L, D[3], D[4], D[2], L2, nullptr), ASR_ERR_ARG);
    EXPECT(asr_ctc_prefix_advance(&d, F, 11, L, L, L, D[0], D[1], D[2], L2, D[3], D[4], D[5], L2, nullptr), ASR_ERR_ARG);
    d.B = 65536;
    EXPECT(asr_ctc_prefix_advance(&d, F, 11, L, L, L, D[0], D[1], D[2], L, D[0], D[4], D[5], L2, nullptr), ASR_ERR_ARG);
    EXPECT(asr_ctc_prefix_begin(&d, F, 11, L, D[0], D[0], D[2], L2, nullptr), ASR_ERR_ARG);
}

int main() {
    nulls();
    for (int which = 0; which < 3; which++) descriptor(which);
    own_checks();
    if (failures) {
        std::printf("ctc prefix check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("ctc prefix check: ok\n");
    return 0;
}
