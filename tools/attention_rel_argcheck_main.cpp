// Host-side argument and shape checks of asr_attention_rel_fwd as a stand-alone
// program for a sanitizer build on the CPU (`make -C
// gpu-accelerated-speech-recognition_amd attnrelcheck` compiles
// csrc/attention_rel.hip and this file with -fsanitize=address,undefined and
// runs the result).  Every call here is refused before any HIP call, in the
// order include/asr_amd.h documents: NULL pointers, sizes, window, strides,
// scale, the table's range (all ASR_ERR_ARG), then ASR_ERR_UNSUPPORTED.  Fake
// device pointers are never dereferenced.  No GPU is needed or used.
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

struct Call {
    const float *q = F, *k = F, *v = F, *pos = F;
    float* out = F;
    long ld = -1, ldp = -1;
    int n_pos = 1 << 30, pos_zero = 1 << 29;          // a table that covers every distance of the small calls
    int Tq = 8, q0 = 0, Tk = 8, k0 = 0, B = 2;
};

static int rel(const asr_attn_desc* d, const Call& c) {
    const long E = d ? (long)d->heads * d->head_dim : 64;
    return asr_attention_rel_fwd(d, c.q, c.ld < 0 ? E : c.ld, c.k, c.ld < 0 ? E : c.ld, c.v, c.ld < 0 ? E : c.ld, c.pos,
                                 c.ldp < 0 ? E : c.ldp, c.n_pos, c.pos_zero, nullptr, F, L, c.out, c.ld < 0 ? E : c.ld,
                                 c.Tq, c.q0, c.Tk, c.k0, c.B, nullptr);
}

int main() {
    asr_attn_desc d = base();
    Call c;
    // 1. NULL pointers (a short table at the same time: the pointer is reported first, both are ARG)
    EXPECT(rel(nullptr, c), ASR_ERR_ARG);
    c = Call(); c.q = nullptr; EXPECT(rel(&d, c), ASR_ERR_ARG);
    c = Call(); c.k = nullptr; EXPECT(rel(&d, c), ASR_ERR_ARG);
    c = Call(); c.v = nullptr; EXPECT(rel(&d, c), ASR_ERR_ARG);
    c = Call(); c.out = nullptr; EXPECT(rel(&d, c), ASR_ERR_ARG);
    c = Call(); c.pos = nullptr; EXPECT(rel(&d, c), ASR_ERR_ARG);
    // 2. sizes
    c = Call(); c.Tq = 0; EXPECT(rel(&d, c), ASR_ERR_ARG);
    c = Call(); c.Tk = INT_MIN; EXPECT(rel(&d, c), ASR_ERR_ARG);
    c = Call(); c.B = -2; EXPECT(rel(&d, c), ASR_ERR_ARG);
    c = Call(); c.n_pos = 0; EXPECT(rel(&d, c), ASR_ERR_ARG);
    c = Call(); c.n_pos = INT_MIN; EXPECT(rel(&d, c), ASR_ERR_ARG);
    c = Call();
    d = base(); d.heads = 0; c.ld = c.ldp = 64; EXPECT(rel(&d, c), ASR_ERR_ARG);
    d = base(); d.head_dim = -16; EXPECT(rel(&d, c), ASR_ERR_ARG);
    d = base(); d.chunk = 0; EXPECT(rel(&d, c), ASR_ERR_ARG);
    // 3. window and positions
    d = base(); d.left = -2; EXPECT(rel(&d, Call()), ASR_ERR_ARG);
    d = base(); d.right = INT_MIN; EXPECT(rel(&d, Call()), ASR_ERR_ARG);
    d = base();
    c = Call(); c.q0 = -1; EXPECT(rel(&d, c), ASR_ERR_ARG);
    c = Call(); c.k0 = -1; EXPECT(rel(&d, c), ASR_ERR_ARG);
    // 4. strides
    c = Call(); c.ld = 63; c.ldp = 64; EXPECT(rel(&d, c), ASR_ERR_ARG);
    c = Call(); c.ldp = 63; EXPECT(rel(&d, c), ASR_ERR_ARG);
    c = Call(); c.ldp = 0; EXPECT(rel(&d, c), ASR_ERR_ARG);
    // 5. scale
    d = base(); d.scale = -1.f; EXPECT(rel(&d, Call()), ASR_ERR_ARG);
    d = base(); d.scale = NAN; EXPECT(rel(&d, Call()), ASR_ERR_ARG);
    d = base(); d.scale = INFINITY; EXPECT(rel(&d, Call()), ASR_ERR_ARG);
    // 6. the table's range: Tq = Tk = 8 full attention needs distances 7 .. -7
    d = base();
    c = Call(); c.n_pos = 15; c.pos_zero = 7; c.B = 70000; EXPECT(rel(&d, c), ASR_ERR_UNSUPPORTED);   // exactly enough
    c = Call(); c.n_pos = 15; c.pos_zero = 6; EXPECT(rel(&d, c), ASR_ERR_ARG);       // one row short at the top
    c = Call(); c.n_pos = 14; c.pos_zero = 7; EXPECT(rel(&d, c), ASR_ERR_ARG);       // one row short at the bottom
    c = Call(); c.n_pos = 15; c.pos_zero = 8; EXPECT(rel(&d, c), ASR_ERR_ARG);
    c = Call(); c.n_pos = 15; c.pos_zero = -1; EXPECT(rel(&d, c), ASR_ERR_ARG);
    c = Call(); c.n_pos = 15; c.pos_zero = INT_MIN; EXPECT(rel(&d, c), ASR_ERR_ARG);
    c = Call(); c.n_pos = INT_MAX; c.pos_zero = INT_MAX; EXPECT(rel(&d, c), ASR_ERR_ARG);
    // the window bounds the range: (chunk 4, left 1, right 0) needs 7 .. -3
    d = base(); d.chunk = 4; d.left = 1; d.right = 0;
    c = Call(); c.Tq = c.Tk = 100; c.n_pos = 11; c.pos_zero = 6; EXPECT(rel(&d, c), ASR_ERR_ARG);
    c = Call(); c.Tq = c.Tk = 100; c.n_pos = 11; c.pos_zero = 7; c.B = 70000; EXPECT(rel(&d, c), ASR_ERR_UNSUPPORTED);
    c = Call(); c.Tq = c.Tk = 100; c.n_pos = 11; c.pos_zero = 8; EXPECT(rel(&d, c), ASR_ERR_ARG);
    // positions shift it: queries 10 .. 13 over keys 2 .. 9 need 11 .. 1
    d = base();
    c = Call(); c.Tq = 4; c.q0 = 10; c.Tk = 8; c.k0 = 2; c.n_pos = 11; c.pos_zero = 10; EXPECT(rel(&d, c), ASR_ERR_ARG);
    c.pos_zero = 12; EXPECT(rel(&d, c), ASR_ERR_ARG);
    c.pos_zero = 11; c.B = 70000; EXPECT(rel(&d, c), ASR_ERR_UNSUPPORTED);
    // a short table and an unsupported shape: ARG comes first
    d = base(); d.head_dim = 18;
    c = Call(); c.n_pos = 14; c.pos_zero = 7; EXPECT(rel(&d, c), ASR_ERR_ARG);
    // 7. ASR_ERR_UNSUPPORTED, asr_attention_fwd's
    d = base(); d.head_dim = 18; EXPECT(rel(&d, Call()), ASR_ERR_UNSUPPORTED);
    d = base(); d.head_dim = 132; EXPECT(rel(&d, Call()), ASR_ERR_UNSUPPORTED);
    d = base(); d.heads = 33; d.head_dim = 128; EXPECT(rel(&d, Call()), ASR_ERR_UNSUPPORTED);      // E = 4224
    d = base(); d.heads = 65536; d.head_dim = 4; c = Call(); c.ld = c.ldp = LONG_MAX; EXPECT(rel(&d, c), ASR_ERR_UNSUPPORTED);
    d = base();
    c = Call(); c.B = 65536; EXPECT(rel(&d, c), ASR_ERR_UNSUPPORTED);
    c = Call(); c.B = 1; c.q0 = INT_MAX - 70; c.n_pos = INT_MAX; c.pos_zero = INT_MAX - 8; EXPECT(rel(&d, c), ASR_ERR_UNSUPPORTED);
    c = Call(); c.B = 1; c.k0 = INT_MAX - 70; c.n_pos = INT_MAX; c.pos_zero = 0; EXPECT(rel(&d, c), ASR_ERR_UNSUPPORTED);
    c = Call(); c.Tq = c.Tk = 1 << 20; c.B = 1 << 12; c.n_pos = 1 << 22; c.pos_zero = 1 << 21; EXPECT(rel(&d, c), ASR_ERR_UNSUPPORTED);

    if (failures) {
        std::printf("attention_rel argcheck: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("attention_rel argcheck: ok\n");
    return 0;
}
