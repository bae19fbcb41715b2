// Host-side argument and shape checks of asr_csgu_fwd and asr_merge_dwconv_fwd,
// as a stand-alone program for a sanitizer build on the CPU
// (`make -C gpu-accelerated-speech-recognition_amd cgmlpcheck` compiles
// csrc/cgmlp.hip and this file with -fsanitize=address,undefined and runs the
// result).  Every call here is refused before any HIP call: invalid descriptors
// and sizes, NULL pointers and fake device pointers that are never
// dereferenced.  No GPU is needed or used.
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

static float* const U = reinterpret_cast<float*>(0x10000);       // never dereferenced
static float* const X2 = reinterpret_cast<float*>(0x18000);
static float* const O = reinterpret_cast<float*>(0x20000);
static float* const S = reinterpret_cast<float*>(0x28000);
static int32_t* const L = reinterpret_cast<int32_t*>(0x30000);

static asr_csgu_desc cbase() {
    asr_csgu_desc d{};
    d.channels = 16; d.kernel = 3; d.pad_left = 1; d.pad_right = 1; d.eps = 1e-5f;
    return d;
}
static asr_merge_dwconv_desc mbase() {
    asr_merge_dwconv_desc d{};
    d.channels = 16; d.kernel = 3; d.pad_left = 1; d.pad_right = 1;
    return d;
}

static int csgu(const asr_csgu_desc& d, int T = 8, int B = 4, long ldu = -1, long ldo = -1, float* out = O) {
    return asr_csgu_fwd(&d, U, ldu < 0 ? 2L * d.channels : ldu, L, U, U, U, U, S, out, ldo < 0 ? d.channels : ldo, T,
                        B, nullptr);
}
static int merge(const asr_merge_dwconv_desc& d, int T = 8, int B = 4, long ld1 = -1, long ld2 = -1, long ldo = -1,
                 float* out = O) {
    return asr_merge_dwconv_fwd(&d, U, ld1 < 0 ? d.channels : ld1, X2, ld2 < 0 ? d.channels : ld2, L, U, U, out,
                                ldo < 0 ? 2L * d.channels : ldo, T, B, nullptr);
}

int main() {
    // asr_csgu_fwd, ASR_ERR_ARG in the documented order
    {
        asr_csgu_desc d = cbase();
        EXPECT(asr_csgu_fwd(nullptr, U, 32, L, U, U, U, U, S, O, 16, 8, 4, nullptr), ASR_ERR_ARG);
        EXPECT(asr_csgu_fwd(&d, nullptr, 32, L, U, U, U, U, S, O, 16, 8, 4, nullptr), ASR_ERR_ARG);
        EXPECT(asr_csgu_fwd(&d, U, 32, L, U, U, nullptr, U, S, O, 16, 8, 4, nullptr), ASR_ERR_ARG);
        EXPECT(asr_csgu_fwd(&d, U, 32, L, U, U, U, U, nullptr, O, 16, 8, 4, nullptr), ASR_ERR_ARG);
        EXPECT(asr_csgu_fwd(&d, U, 32, L, U, U, U, U, S, nullptr, 16, 8, 4, nullptr), ASR_ERR_ARG);
        EXPECT(csgu(d, 0), ASR_ERR_ARG);
        EXPECT(csgu(d, 8, INT_MIN), ASR_ERR_ARG);
        d = cbase(); d.channels = 0; EXPECT(csgu(d, 8, 4, 32, 16), ASR_ERR_ARG);
        d = cbase(); d.channels = INT_MAX; EXPECT(csgu(d, 8, 4, INT_MAX, INT_MAX), ASR_ERR_ARG);   // 2C does not wrap
        d = cbase(); d.kernel = -3; EXPECT(csgu(d), ASR_ERR_ARG);
        d = cbase(); d.pad_left = -1; d.pad_right = 3; EXPECT(csgu(d), ASR_ERR_ARG);
        d = cbase(); d.pad_right = INT_MIN; EXPECT(csgu(d), ASR_ERR_ARG);
        d = cbase(); EXPECT(csgu(d, 8, 4, 31), ASR_ERR_ARG);
        EXPECT(csgu(d, 8, 4, 32, 15), ASR_ERR_ARG);
        EXPECT(asr_csgu_fwd(&d, U, LONG_MIN, L, U, U, U, U, S, O, 16, 8, 4, nullptr), ASR_ERR_ARG);
        d = cbase(); d.eps = NAN; EXPECT(csgu(d), ASR_ERR_ARG);
        d = cbase(); d.eps = INFINITY; EXPECT(csgu(d), ASR_ERR_ARG);
        d = cbase(); d.eps = -1e-6f; EXPECT(csgu(d), ASR_ERR_ARG);
        d = cbase(); EXPECT(csgu(d, 8, 4, -1, -1, U), ASR_ERR_ARG);                   // d_out == d_u
        // ASR_ERR_ARG comes before ASR_ERR_UNSUPPORTED
        d = cbase(); d.kernel = 200; d.eps = -1.f; EXPECT(csgu(d), ASR_ERR_ARG);
        d = cbase(); d.pad_left = 5; EXPECT(csgu(d, 8, 4, -1, -1, U), ASR_ERR_ARG);
        d = cbase(); EXPECT(csgu(d, INT_MAX, INT_MAX, 8), ASR_ERR_ARG);
    }
    // asr_csgu_fwd, ASR_ERR_UNSUPPORTED
    {
        asr_csgu_desc d;
        d = cbase(); d.pad_left = 2; EXPECT(csgu(d), ASR_ERR_UNSUPPORTED);
        d = cbase(); d.pad_left = INT_MAX; d.pad_right = INT_MAX; EXPECT(csgu(d), ASR_ERR_UNSUPPORTED);
        d = cbase(); d.kernel = ASR_CGMLP_MAX_KERNEL + 1; d.pad_left = ASR_CGMLP_MAX_KERNEL; d.pad_right = 0;
        EXPECT(csgu(d, 200), ASR_ERR_UNSUPPORTED);
        d = cbase(); d.kernel = INT_MAX; d.pad_left = INT_MAX - 1; d.pad_right = 0; EXPECT(csgu(d), ASR_ERR_UNSUPPORTED);
        d = cbase(); d.channels = 4097; EXPECT(csgu(d), ASR_ERR_UNSUPPORTED);
        d = cbase(); EXPECT(csgu(d, 1 << 20, 1 << 12), ASR_ERR_UNSUPPORTED);          // T*B > INT_MAX
        d = cbase(); EXPECT(csgu(d, INT_MAX - 4095, 1), ASR_ERR_UNSUPPORTED);         // a tile's frame index
        d = cbase(); d.channels = 4096; d.kernel = 1; d.pad_left = d.pad_right = 0;
        EXPECT(csgu(d, 65, 1 << 24), ASR_ERR_UNSUPPORTED);                            // the grid: 2^24 * 2 * 64
    }
    // asr_merge_dwconv_fwd
    {
        asr_merge_dwconv_desc d = mbase();
        EXPECT(asr_merge_dwconv_fwd(nullptr, U, 16, X2, 16, L, U, U, O, 32, 8, 4, nullptr), ASR_ERR_ARG);
        EXPECT(asr_merge_dwconv_fwd(&d, nullptr, 16, X2, 16, L, U, U, O, 32, 8, 4, nullptr), ASR_ERR_ARG);
        EXPECT(asr_merge_dwconv_fwd(&d, U, 16, nullptr, 16, L, U, U, O, 32, 8, 4, nullptr), ASR_ERR_ARG);
        EXPECT(asr_merge_dwconv_fwd(&d, U, 16, X2, 16, L, nullptr, U, O, 32, 8, 4, nullptr), ASR_ERR_ARG);
        EXPECT(asr_merge_dwconv_fwd(&d, U, 16, X2, 16, L, U, U, nullptr, 32, 8, 4, nullptr), ASR_ERR_ARG);
        EXPECT(merge(d, 0), ASR_ERR_ARG);
        EXPECT(merge(d, 8, -4), ASR_ERR_ARG);
        EXPECT(merge(d, 8, 4, 15), ASR_ERR_ARG);
        EXPECT(merge(d, 8, 4, 16, 15), ASR_ERR_ARG);
        EXPECT(merge(d, 8, 4, 16, 16, 31), ASR_ERR_ARG);
        EXPECT(merge(d, 8, 4, -1, -1, -1, U), ASR_ERR_ARG);                           // d_out == d_x1
        EXPECT(merge(d, 8, 4, -1, -1, -1, X2), ASR_ERR_ARG);                          // d_out == d_x2
        d = mbase(); d.channels = INT_MAX; EXPECT(merge(d, 8, 4, INT_MAX, INT_MAX, INT_MAX), ASR_ERR_ARG);
        d = mbase(); d.kernel = 0; EXPECT(merge(d), ASR_ERR_ARG);
        d = mbase(); d.pad_left = -2; EXPECT(merge(d), ASR_ERR_ARG);
        d = mbase(); d.pad_left = 5; EXPECT(merge(d, 8, 4, -1, -1, -1, X2), ASR_ERR_ARG);
        d = mbase(); d.pad_left = 2; EXPECT(merge(d), ASR_ERR_UNSUPPORTED);
        d = mbase(); d.kernel = ASR_CGMLP_MAX_KERNEL + 1; d.pad_left = ASR_CGMLP_MAX_KERNEL; d.pad_right = 0;
        EXPECT(merge(d, 200), ASR_ERR_UNSUPPORTED);
        d = mbase(); d.channels = 4097; EXPECT(merge(d), ASR_ERR_UNSUPPORTED);
        d = mbase(); EXPECT(merge(d, 1 << 20, 1 << 12), ASR_ERR_UNSUPPORTED);
        d = mbase(); EXPECT(merge(d, INT_MAX, 1), ASR_ERR_UNSUPPORTED);
        d = mbase(); d.channels = 4096; d.kernel = 1; d.pad_left = d.pad_right = 0;
        EXPECT(merge(d, 65, 1 << 23), ASR_ERR_UNSUPPORTED);                           // the grid: 2^23 * 2 * 128
    }

    if (failures) {
        std::printf("cgmlp argcheck: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("cgmlp argcheck: ok\n");
    return 0;
}
