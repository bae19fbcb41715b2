// Host-side argument and shape checks of asr_attention_zip_fwd, asr_biasnorm_fwd
// and asr_bypass_fwd as a stand-alone program for a sanitizer build on the CPU
// (`make -C gpu-accelerated-speech-recognition_amd zipcheck` compiles
// csrc/attention_zip.hip and this file with -fsanitize=address,undefined and
// runs the result).  Every call here is refused before any HIP call, in the
// order include/asr_amd.h documents; each ASR_ERR_ARG case also carries an
// unsupported width, so a refusal out of order shows.  Fake device pointers are
// never dereferenced.  No GPU is needed or used.
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

static float* const F = reinterpret_cast<float*>(0x10000);       // 16-byte aligned, never dereferenced
static int32_t* const L = reinterpret_cast<int32_t*>(0x10000);

static asr_zattn_desc base(bool bad = false) {
    asr_zattn_desc d{};
    d.heads = 2; d.query_dim = bad ? 6 : 8; d.pos_dim = 4; d.value_heads = 2; d.value_dim = 4; d.score_head = 0;
    d.scale = 0.f; d.chunk = 1; d.left = -1; d.right = -1; d.gate = 1;
    return d;
}

struct Call {
    const float *q = F, *k = F, *pz = F, *v = F, *sg = F, *y = F, *pos = F;
    float* out = F;
    long ldq = 16, ldk = 16, ldpz = 8, ldv = 8, ldsg = 8, ldy = 8, ldp = 8, ldo = 8;
    int n_pos = 15, pos_zero = 7, Tq = 8, q0 = 0, Tk = 8, k0 = 0, B = 2;
};

static int zip(const asr_zattn_desc* d, const Call& c) {
    return asr_attention_zip_fwd(d, c.q, c.ldq, c.k, c.ldk, c.pz, c.ldpz, c.v, c.ldv, c.sg, c.ldsg, c.y, c.ldy, c.pos,
                                 c.ldp, c.n_pos, c.pos_zero, L, c.out, c.ldo, c.Tq, c.q0, c.Tk, c.k0, c.B, nullptr);
}

#define ARG_CALL(stmt) do { Call c; asr_zattn_desc d = base(true); stmt; EXPECT(zip(&d, c), ASR_ERR_ARG); } while (0)
#define UNS_CALL(stmt) do { Call c; asr_zattn_desc d = base(); stmt; EXPECT(zip(&d, c), ASR_ERR_UNSUPPORTED); } while (0)

int main() {
    { Call c; EXPECT(zip(nullptr, c), ASR_ERR_ARG); }
    // NULL pointers, the conditional ones after the descriptor's own pos_dim / gate
    ARG_CALL(c.q = nullptr); ARG_CALL(c.k = nullptr); ARG_CALL(c.v = nullptr); ARG_CALL(c.out = nullptr);
    ARG_CALL(d.pos_dim = -4); ARG_CALL(d.gate = 2); ARG_CALL(d.gate = -1);
    ARG_CALL(c.pz = nullptr); ARG_CALL(c.pos = nullptr); ARG_CALL(c.sg = nullptr); ARG_CALL(c.y = nullptr);
    // sizes
    ARG_CALL(c.Tq = 0); ARG_CALL(c.Tk = INT_MIN); ARG_CALL(c.B = -2); ARG_CALL(d.heads = 0); ARG_CALL(d.query_dim = 0);
    ARG_CALL(d.value_dim = -4); ARG_CALL(d.chunk = 0); ARG_CALL(c.n_pos = 0);
    // head mapping
    ARG_CALL(d.value_heads = 3); ARG_CALL(d.value_heads = 0); ARG_CALL(d.score_head = 2); ARG_CALL(d.score_head = -1);
    // window and positions
    ARG_CALL(d.left = -2); ARG_CALL(d.right = INT_MIN); ARG_CALL(c.q0 = -1); ARG_CALL(c.k0 = -1);
    // strides (query_dim 6: heads * query_dim = 12)
    ARG_CALL(c.ldq = 11); ARG_CALL(c.ldk = 11); ARG_CALL(c.ldv = 7); ARG_CALL(c.ldo = 7); ARG_CALL(c.ldpz = 7);
    ARG_CALL(c.ldp = 0); ARG_CALL(c.ldsg = 7); ARG_CALL(c.ldy = LONG_MIN);
    // scale
    ARG_CALL(d.scale = -1.f); ARG_CALL(d.scale = NAN); ARG_CALL(d.scale = INFINITY);
    // the table's range: Tq = Tk = 8 full attention needs distances 7 .. -7
    ARG_CALL(c.pos_zero = 6); ARG_CALL(c.n_pos = 14); ARG_CALL(c.pos_zero = INT_MIN);
    ARG_CALL(c.n_pos = INT_MAX; c.pos_zero = INT_MAX);
    ARG_CALL(d.chunk = 4; d.left = 1; d.right = 0; c.Tq = c.Tk = 100; c.n_pos = 11; c.pos_zero = 6);
    UNS_CALL(d.chunk = 4; d.left = 1; d.right = 0; c.Tq = c.Tk = 100; c.n_pos = 11; c.pos_zero = 7; c.B = 70000);
    // what pos_dim = 0 and gate = 0 switch off is not checked
    UNS_CALL(d.pos_dim = 0; d.gate = 0; c.pz = c.pos = c.sg = c.y = nullptr; c.n_pos = 0; c.pos_zero = -5; c.ldp = 0;
             c.B = 70000);
    // ASR_ERR_UNSUPPORTED
    UNS_CALL(d.query_dim = 6; c.ldq = c.ldk = 12); UNS_CALL(d.query_dim = 132; c.ldq = c.ldk = 264);
    UNS_CALL(d.heads = d.value_heads = 64; d.query_dim = 128; c.ldq = c.ldk = c.ldpz = c.ldp = c.ldv = c.ldo = c.ldsg =
                 c.ldy = 8192);
    UNS_CALL(d.pos_dim = 6; c.ldpz = c.ldp = 12); UNS_CALL(d.pos_dim = 20; c.ldpz = c.ldp = 40);
    UNS_CALL(d.value_dim = 6; c.ldv = c.ldo = c.ldsg = c.ldy = 12);
    UNS_CALL(d.value_heads = 1; d.value_dim = 4100; c.ldv = c.ldo = c.ldsg = c.ldy = 4100);
    UNS_CALL(d.heads = 65536; d.value_heads = 1; d.query_dim = 4; d.pos_dim = 0; c.ldq = c.ldk = LONG_MAX);
    UNS_CALL(c.B = 65536);
    UNS_CALL(c.B = 1; c.q0 = INT_MAX - 70; c.n_pos = INT_MAX; c.pos_zero = INT_MAX - 8);
    UNS_CALL(c.B = 1; c.k0 = INT_MAX - 70; c.n_pos = INT_MAX; c.pos_zero = 0);
    UNS_CALL(c.Tq = c.Tk = 1 << 20; c.B = 1 << 12; c.n_pos = 1 << 22; c.pos_zero = 1 << 21);

    // asr_biasnorm_fwd (N = 5000 rides along as the later violation)
    const long W = 5000;
    EXPECT(asr_biasnorm_fwd(nullptr, W, F, 0.f, nullptr, 0, nullptr, L, F, W, 4, 2, 5000, nullptr), ASR_ERR_ARG);
    EXPECT(asr_biasnorm_fwd(F, W, nullptr, 0.f, nullptr, 0, nullptr, L, F, W, 4, 2, 5000, nullptr), ASR_ERR_ARG);
    EXPECT(asr_biasnorm_fwd(F, W, F, 0.f, nullptr, 0, nullptr, L, nullptr, W, 4, 2, 5000, nullptr), ASR_ERR_ARG);
    EXPECT(asr_biasnorm_fwd(F, W, F, 0.f, F, W, nullptr, L, F, W, 4, 2, 5000, nullptr), ASR_ERR_ARG);
    EXPECT(asr_biasnorm_fwd(F, W, F, 0.f, nullptr, W, F, L, F, W, 4, 2, 5000, nullptr), ASR_ERR_ARG);
    EXPECT(asr_biasnorm_fwd(F, W, F, 0.f, nullptr, 0, nullptr, L, F, W, 0, 2, 5000, nullptr), ASR_ERR_ARG);
    EXPECT(asr_biasnorm_fwd(F, W, F, 0.f, nullptr, 0, nullptr, L, F, W, 4, INT_MIN, 5000, nullptr), ASR_ERR_ARG);
    EXPECT(asr_biasnorm_fwd(F, W, F, 0.f, nullptr, 0, nullptr, L, F, W, 4, 2, 0, nullptr), ASR_ERR_ARG);
    EXPECT(asr_biasnorm_fwd(F, W - 1, F, 0.f, nullptr, 0, nullptr, L, F, W, 4, 2, 5000, nullptr), ASR_ERR_ARG);
    EXPECT(asr_biasnorm_fwd(F, W, F, 0.f, nullptr, 0, nullptr, L, F, LONG_MIN, 4, 2, 5000, nullptr), ASR_ERR_ARG);
    EXPECT(asr_biasnorm_fwd(F, W, F, 0.f, F, W - 1, F, L, F, W, 4, 2, 5000, nullptr), ASR_ERR_ARG);
    EXPECT(asr_biasnorm_fwd(F, W, F, NAN, nullptr, 0, nullptr, L, F, W, 4, 2, 5000, nullptr), ASR_ERR_ARG);
    EXPECT(asr_biasnorm_fwd(F, W, F, INFINITY, nullptr, 0, nullptr, L, F, W, 4, 2, 5000, nullptr), ASR_ERR_ARG);
    EXPECT(asr_biasnorm_fwd(F, W, F, 0.f, nullptr, 0, nullptr, nullptr, F, W, 4, 2, 5000, nullptr), ASR_ERR_UNSUPPORTED);
    EXPECT(asr_biasnorm_fwd(F, 8, F, 0.f, F, 8, F, L, F, 8, INT_MAX, INT_MAX, 8, nullptr), ASR_ERR_UNSUPPORTED);

    // asr_bypass_fwd
    EXPECT(asr_bypass_fwd(nullptr, W, F, W, F, L, F, W, 4, 2, 5000, nullptr), ASR_ERR_ARG);
    EXPECT(asr_bypass_fwd(F, W, nullptr, W, F, L, F, W, 4, 2, 5000, nullptr), ASR_ERR_ARG);
    EXPECT(asr_bypass_fwd(F, W, F, W, nullptr, L, F, W, 4, 2, 5000, nullptr), ASR_ERR_ARG);
    EXPECT(asr_bypass_fwd(F, W, F, W, F, L, nullptr, W, 4, 2, 5000, nullptr), ASR_ERR_ARG);
    EXPECT(asr_bypass_fwd(F, W, F, W, F, L, F, W, -1, 2, 5000, nullptr), ASR_ERR_ARG);
    EXPECT(asr_bypass_fwd(F, W, F, W, F, L, F, W, 4, 0, 5000, nullptr), ASR_ERR_ARG);
    EXPECT(asr_bypass_fwd(F, W, F, W, F, L, F, W, 4, 2, INT_MIN, nullptr), ASR_ERR_ARG);
    EXPECT(asr_bypass_fwd(F, W - 1, F, W, F, L, F, W, 4, 2, 5000, nullptr), ASR_ERR_ARG);
    EXPECT(asr_bypass_fwd(F, W, F, 0, F, L, F, W, 4, 2, 5000, nullptr), ASR_ERR_ARG);
    EXPECT(asr_bypass_fwd(F, W, F, W, F, L, F, W - 1, 4, 2, 5000, nullptr), ASR_ERR_ARG);
    EXPECT(asr_bypass_fwd(F, W, F, W, F, nullptr, F, W, 4, 2, 5000, nullptr), ASR_ERR_UNSUPPORTED);
    EXPECT(asr_bypass_fwd(F, 8, F, 8, F, L, F, 8, INT_MAX, 2, 8, nullptr), ASR_ERR_UNSUPPORTED);

    if (failures) {
        std::printf("zipformer argcheck: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("zipformer argcheck: ok\n");
    return 0;
}
