// Host-side argument and shape checks of asr_attention_fwd, asr_layernorm_fwd and
// asr_mask_rows, as a stand-alone program for a sanitizer build on the CPU
// (`make -C gpu-accelerated-speech-recognition_amd attncheck` compiles
// csrc/attention.hip and this file with -fsanitize=address,undefined and runs
// the result).  Every call here is refused before any HIP call: invalid
// descriptors and sizes, NULL pointers and fake device pointers that are never
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

static asr_attn_desc base() {
    asr_attn_desc d{};
    d.heads = 4; d.head_dim = 16; d.scale = 0.f; d.chunk = 1; d.left = -1; d.right = -1;
    return d;
}

static float* const F = reinterpret_cast<float*>(0x10000);       // 16-byte aligned, never dereferenced
static int32_t* const L = reinterpret_cast<int32_t*>(0x10000);

static int att(const asr_attn_desc& d, int Tq = 8, int Tk = 8, int B = 2, int q0 = 0, int k0 = 0, long ld = -1) {
    const long l = ld < 0 ? (long)d.heads * d.head_dim : ld;
    return asr_attention_fwd(&d, F, l, F, l, F, l, L, F, l, Tq, q0, Tk, k0, B, nullptr);
}

static int ln(int T = 8, int B = 2, int N = 16, long ldx = -1, long ldr = -1, long ldo = -1, float eps = 1e-5f,
              const float* res = F) {
    return asr_layernorm_fwd(F, ldx < 0 ? N : ldx, res, ldr < 0 ? N : ldr, F, F, eps, L, F, ldo < 0 ? N : ldo, T, B,
                             N, nullptr);
}

int main() {
    // asr_attention_fwd: ASR_ERR_ARG
    {
        const asr_attn_desc d = base();
        EXPECT(asr_attention_fwd(nullptr, F, 64, F, 64, F, 64, L, F, 64, 8, 0, 8, 0, 2, nullptr), ASR_ERR_ARG);
        EXPECT(asr_attention_fwd(&d, nullptr, 64, F, 64, F, 64, L, F, 64, 8, 0, 8, 0, 2, nullptr), ASR_ERR_ARG);
        EXPECT(asr_attention_fwd(&d, F, 64, nullptr, 64, F, 64, L, F, 64, 8, 0, 8, 0, 2, nullptr), ASR_ERR_ARG);
        EXPECT(asr_attention_fwd(&d, F, 64, F, 64, nullptr, 64, L, F, 64, 8, 0, 8, 0, 2, nullptr), ASR_ERR_ARG);
        EXPECT(asr_attention_fwd(&d, F, 64, F, 64, F, 64, L, nullptr, 64, 8, 0, 8, 0, 2, nullptr), ASR_ERR_ARG);
        EXPECT(att(d, 0), ASR_ERR_ARG);
        EXPECT(att(d, -1), ASR_ERR_ARG);
        EXPECT(att(d, 8, 0), ASR_ERR_ARG);
        EXPECT(att(d, 8, INT_MIN), ASR_ERR_ARG);
        EXPECT(att(d, 8, 8, 0), ASR_ERR_ARG);
        EXPECT(att(d, 8, 8, -2), ASR_ERR_ARG);
        EXPECT(att(d, 8, 8, 2, -1), ASR_ERR_ARG);
        EXPECT(att(d, 8, 8, 2, 0, -1), ASR_ERR_ARG);
        EXPECT(att(d, 8, 8, 2, 0, 0, 63), ASR_ERR_ARG);
        EXPECT(asr_attention_fwd(&d, F, 64, F, 63, F, 64, L, F, 64, 8, 0, 8, 0, 2, nullptr), ASR_ERR_ARG);
        EXPECT(asr_attention_fwd(&d, F, 64, F, 64, F, 0, L, F, 64, 8, 0, 8, 0, 2, nullptr), ASR_ERR_ARG);
        EXPECT(asr_attention_fwd(&d, F, 64, F, 64, F, 64, L, F, -64, 8, 0, 8, 0, 2, nullptr), ASR_ERR_ARG);
    }
    {
        asr_attn_desc d;
        d = base(); d.heads = 0; EXPECT(att(d, 8, 8, 2, 0, 0, 64), ASR_ERR_ARG);
        d = base(); d.heads = -4; EXPECT(att(d, 8, 8, 2, 0, 0, 64), ASR_ERR_ARG);
        d = base(); d.head_dim = 0; EXPECT(att(d, 8, 8, 2, 0, 0, 64), ASR_ERR_ARG);
        d = base(); d.head_dim = INT_MIN; EXPECT(att(d, 8, 8, 2, 0, 0, 64), ASR_ERR_ARG);
        d = base(); d.chunk = 0; EXPECT(att(d), ASR_ERR_ARG);
        d = base(); d.left = -2; EXPECT(att(d), ASR_ERR_ARG);
        d = base(); d.right = INT_MIN; EXPECT(att(d), ASR_ERR_ARG);
        d = base(); d.scale = -1.f; EXPECT(att(d), ASR_ERR_ARG);
        d = base(); d.scale = INFINITY; EXPECT(att(d), ASR_ERR_ARG);
        d = base(); d.scale = NAN; EXPECT(att(d), ASR_ERR_ARG);
        // both a bad argument and unsupported: ARG
        d = base(); d.head_dim = 18; d.chunk = 0; EXPECT(att(d), ASR_ERR_ARG);
        d = base(); d.head_dim = 256; d.scale = NAN; EXPECT(att(d), ASR_ERR_ARG);
        d = base(); d.heads = INT_MAX; d.head_dim = INT_MAX; EXPECT(att(d, 8, 8, 2, 0, 0, 64), ASR_ERR_ARG);  // stride
        d = base(); EXPECT(att(d, INT_MAX, INT_MAX, 70000, -1), ASR_ERR_ARG);
    }
    // asr_attention_fwd: ASR_ERR_UNSUPPORTED
    {
        asr_attn_desc d;
        d = base(); d.head_dim = 18; EXPECT(att(d), ASR_ERR_UNSUPPORTED);
        d = base(); d.head_dim = 2; EXPECT(att(d), ASR_ERR_UNSUPPORTED);
        d = base(); d.head_dim = 132; EXPECT(att(d), ASR_ERR_UNSUPPORTED);
        d = base(); d.heads = 33; d.head_dim = 128; EXPECT(att(d), ASR_ERR_UNSUPPORTED);          // E = 4224
        d = base(); d.heads = INT_MAX; d.head_dim = 4; EXPECT(att(d, 8, 8, 2, 0, 0, LONG_MAX), ASR_ERR_UNSUPPORTED);
        d = base(); d.heads = 65536; d.head_dim = 4; EXPECT(att(d, 8, 8, 2, 0, 0, LONG_MAX), ASR_ERR_UNSUPPORTED);
        d = base(); EXPECT(att(d, 8, 8, 65536), ASR_ERR_UNSUPPORTED);
        d = base(); EXPECT(att(d, 8, 8, 1, INT_MAX - 70), ASR_ERR_UNSUPPORTED);
        d = base(); EXPECT(att(d, 8, 8, 1, 0, INT_MAX), ASR_ERR_UNSUPPORTED);
        d = base(); EXPECT(att(d, INT_MAX, 8, 1), ASR_ERR_UNSUPPORTED);
        d = base(); EXPECT(att(d, 1 << 20, 8, 1 << 12), ASR_ERR_UNSUPPORTED);                     // Tq*B > INT_MAX
        d = base(); EXPECT(att(d, 8, 1 << 20, 1 << 12), ASR_ERR_UNSUPPORTED);                     // Tk*B > INT_MAX
    }

    // asr_layernorm_fwd
    EXPECT(asr_layernorm_fwd(nullptr, 16, F, 16, F, F, 1e-5f, L, F, 16, 8, 2, 16, nullptr), ASR_ERR_ARG);
    EXPECT(asr_layernorm_fwd(F, 16, F, 16, F, F, 1e-5f, L, nullptr, 16, 8, 2, 16, nullptr), ASR_ERR_ARG);
    EXPECT(ln(0), ASR_ERR_ARG);
    EXPECT(ln(8, -1), ASR_ERR_ARG);
    EXPECT(ln(8, 2, 0), ASR_ERR_ARG);
    EXPECT(ln(8, 2, INT_MIN), ASR_ERR_ARG);
    EXPECT(ln(8, 2, 16, 15), ASR_ERR_ARG);
    EXPECT(ln(8, 2, 16, 16, 15), ASR_ERR_ARG);
    EXPECT(ln(8, 2, 16, 16, 16, 15), ASR_ERR_ARG);
    EXPECT(ln(8, 2, 16, 16, 16, 16, -1e-5f), ASR_ERR_ARG);
    EXPECT(ln(8, 2, 16, 16, 16, 16, INFINITY), ASR_ERR_ARG);
    EXPECT(ln(8, 2, 16, 16, 16, 16, NAN), ASR_ERR_ARG);
    EXPECT(ln(8, 2, 5000, 4999), ASR_ERR_ARG);                       // before unsupported
    EXPECT(ln(INT_MAX, INT_MAX, 16, 16, 16, 16, NAN), ASR_ERR_ARG);
    EXPECT(ln(8, 2, 4097), ASR_ERR_UNSUPPORTED);
    EXPECT(ln(8, 2, INT_MAX), ASR_ERR_UNSUPPORTED);
    EXPECT(ln(1 << 20, 1 << 12), ASR_ERR_UNSUPPORTED);
    EXPECT(ln(INT_MAX, INT_MAX), ASR_ERR_UNSUPPORTED);
    EXPECT(ln(1 << 20, 1 << 12, 16, 16, 0, 16, 1e-5f, nullptr), ASR_ERR_UNSUPPORTED);   // ldr unused without res

    // asr_mask_rows
    EXPECT(asr_mask_rows(nullptr, 16, L, 8, 2, 16, nullptr), ASR_ERR_ARG);
    EXPECT(asr_mask_rows(F, 16, L, 0, 2, 16, nullptr), ASR_ERR_ARG);
    EXPECT(asr_mask_rows(F, 16, L, 8, -2, 16, nullptr), ASR_ERR_ARG);
    EXPECT(asr_mask_rows(F, 16, L, 8, 2, 0, nullptr), ASR_ERR_ARG);
    EXPECT(asr_mask_rows(F, 15, L, 8, 2, 16, nullptr), ASR_ERR_ARG);
    EXPECT(asr_mask_rows(F, 16, L, INT_MAX, INT_MAX, 16, nullptr), ASR_ERR_UNSUPPORTED);
    EXPECT(asr_mask_rows(F, 16, nullptr, 8, 2, 16, nullptr), ASR_OK);                  // no lengths: no launch

    if (failures) {
        std::printf("attention argcheck: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("attention argcheck: ok\n");
    return 0;
}
