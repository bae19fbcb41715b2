// Host-side checks of csrc/attn_decode.hip as a stand-alone program for a
// sanitizer build on the CPU (`make -C gpu-accelerated-speech-recognition_amd
// attndeccheck` compiles csrc/attn_decode.hip and this file with
// -fsanitize=address,undefined and runs the result): every refusal of
// asr_decode_attention_fwd, asr_embed_fwd, asr_attn_beam_step and
// asr_attn_beam_step_host in the documented order (fake device pointers that
// are never dereferenced), and random small prunes of the host twin against a
// restatement of the rule (a full stable sort of every candidate).  No GPU is
// needed or used.
#include "asr_amd.h"

#include <algorithm>
#include <climits>
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
            std::printf("FAIL %s: got %ld, want %ld\n", #expr, got_, (long)(want));     \
            failures++;                                                                 \
        }                                                                               \
    } while (0)

static asr_xattn_desc base() {
    asr_xattn_desc d{};
    d.heads = 4; d.head_dim = 16; d.scale = 0.f;
    return d;
}

static float* const F = reinterpret_cast<float*>(0x10000);       // 16-byte aligned, never dereferenced
static int32_t* const L = reinterpret_cast<int32_t*>(0x10000);
static int32_t* const L2 = reinterpret_cast<int32_t*>(0x20000);
static double* const D = reinterpret_cast<double*>(0x10000);

static int da(const asr_xattn_desc& d, int N = 6, int Tk = 8, int S = 6, long ldc = 6, long ld = -1) {
    const long l = ld < 0 ? (long)d.heads * d.head_dim : ld;
    return asr_decode_attention_fwd(&d, F, l, F, l, F, l, L, ldc, L, F, l, N, Tk, S, nullptr);
}

static int em(int R = 6, int E = 32, int V = 11, int P = 8, long ld = -1, double scale = 2.0) {
    const long l = ld < 0 ? E : ld;
    return asr_embed_fwd(F, l, D, l, L, L, scale, F, l, R, E, V, P, nullptr);
}

static asr_attn_beam_desc bbase() {
    asr_attn_beam_desc d{};
    d.B = 3; d.K = 4; d.V = 11; d.max_len = 8; d.step = 2; d.eos = 10;
    return d;
}

static int bs(const asr_attn_beam_desc& d, long ld = -1, bool host = false) {
    const long l = ld < 0 ? d.V : ld;
    if (host) return asr_attn_beam_step_host(&d, F, l, D, L, L, L, D, L, L, L, L2, L2, L);
    return asr_attn_beam_step(&d, F, l, D, L, L, L, D, L, L, L, L2, L2, L, nullptr);
}

static void refusals() {
    // asr_decode_attention_fwd: ASR_ERR_ARG
    {
        const asr_xattn_desc d = base();
        EXPECT(asr_decode_attention_fwd(nullptr, F, 64, F, 64, F, 64, L, 6, L, F, 64, 6, 8, 6, nullptr), ASR_ERR_ARG);
        EXPECT(asr_decode_attention_fwd(&d, nullptr, 64, F, 64, F, 64, L, 6, L, F, 64, 6, 8, 6, nullptr), ASR_ERR_ARG);
        EXPECT(asr_decode_attention_fwd(&d, F, 64, nullptr, 64, F, 64, L, 6, L, F, 64, 6, 8, 6, nullptr), ASR_ERR_ARG);
        EXPECT(asr_decode_attention_fwd(&d, F, 64, F, 64, nullptr, 64, L, 6, L, F, 64, 6, 8, 6, nullptr), ASR_ERR_ARG);
        EXPECT(asr_decode_attention_fwd(&d, F, 64, F, 64, F, 64, L, 6, L, nullptr, 64, 6, 8, 6, nullptr), ASR_ERR_ARG);
        EXPECT(asr_decode_attention_fwd(&d, F, 64, F, 64, F, 64, nullptr, 6, L, F, 64, 6, 8, 6, nullptr), ASR_ERR_ARG);
        EXPECT(asr_decode_attention_fwd(&d, F, 64, F, 64, F, 64, nullptr, 0, L, F, 64, 6, 8, 6, nullptr), ASR_ERR_ARG);
        EXPECT(da(d, 0), ASR_ERR_ARG);
        EXPECT(da(d, INT_MIN), ASR_ERR_ARG);
        EXPECT(da(d, 6, 0), ASR_ERR_ARG);
        EXPECT(da(d, 6, -8), ASR_ERR_ARG);
        EXPECT(da(d, 6, 8, 0), ASR_ERR_ARG);
        EXPECT(da(d, 6, 8, -1), ASR_ERR_ARG);
        EXPECT(da(d, 6, 8, 6, 5), ASR_ERR_ARG);                          // 0 < ldc < N
        EXPECT(da(d, 6, 8, 6, 1), ASR_ERR_ARG);
        EXPECT(da(d, 6, 8, 6, -6), ASR_ERR_ARG);
        EXPECT(da(d, 6, 8, 6, LONG_MIN), ASR_ERR_ARG);
        EXPECT(da(d, 6, 8, 6, 6, 63), ASR_ERR_ARG);
        EXPECT(asr_decode_attention_fwd(&d, F, 64, F, 63, F, 64, L, 6, L, F, 64, 6, 8, 6, nullptr), ASR_ERR_ARG);
        EXPECT(asr_decode_attention_fwd(&d, F, 64, F, 64, F, 0, L, 6, L, F, 64, 6, 8, 6, nullptr), ASR_ERR_ARG);
        EXPECT(asr_decode_attention_fwd(&d, F, 64, F, 64, F, 64, L, 6, L, F, -64, 6, 8, 6, nullptr), ASR_ERR_ARG);
    }
    {
        asr_xattn_desc d;
        d = base(); d.heads = 0; EXPECT(da(d, 6, 8, 6, 6, 64), ASR_ERR_ARG);
        d = base(); d.head_dim = -16; EXPECT(da(d, 6, 8, 6, 6, 64), ASR_ERR_ARG);
        d = base(); d.scale = -1.f; EXPECT(da(d), ASR_ERR_ARG);
        d = base(); d.scale = INFINITY; EXPECT(da(d), ASR_ERR_ARG);
        d = base(); d.scale = NAN; EXPECT(da(d), ASR_ERR_ARG);
        // both a bad argument and unsupported: ARG
        d = base(); d.head_dim = 18; EXPECT(da(d, 6, 8, 6, 3), ASR_ERR_ARG);
        d = base(); d.head_dim = 256; d.scale = NAN; EXPECT(da(d), ASR_ERR_ARG);
        d = base(); EXPECT(da(d, 6, 1 << 20, 1 << 12, 2), ASR_ERR_ARG);
    }
    // asr_decode_attention_fwd: ASR_ERR_UNSUPPORTED; ldc = 0 and ldc = N are both taken up to here
    {
        asr_xattn_desc d;
        d = base(); d.head_dim = 18; EXPECT(da(d), ASR_ERR_UNSUPPORTED);
        d = base(); d.head_dim = 2; EXPECT(da(d, 6, 8, 6, 0), ASR_ERR_UNSUPPORTED);
        d = base(); d.head_dim = 132; EXPECT(da(d), ASR_ERR_UNSUPPORTED);
        d = base(); d.heads = 33; d.head_dim = 128; EXPECT(da(d), ASR_ERR_UNSUPPORTED);           // E = 4224
        d = base(); d.heads = 65536; d.head_dim = 4; EXPECT(da(d, 6, 8, 6, 6, LONG_MAX), ASR_ERR_UNSUPPORTED);
        d = base(); EXPECT(da(d, 6, 1 << 20, 1 << 12), ASR_ERR_UNSUPPORTED);                      // Tk*S > INT_MAX
        d = base(); EXPECT(da(d, 6, INT_MAX, INT_MAX, 0), ASR_ERR_UNSUPPORTED);
    }

    // asr_embed_fwd
    EXPECT(asr_embed_fwd(nullptr, 32, D, 32, L, L, 1.0, F, 32, 6, 32, 11, 8, nullptr), ASR_ERR_ARG);
    EXPECT(asr_embed_fwd(F, 32, D, 32, nullptr, L, 1.0, F, 32, 6, 32, 11, 8, nullptr), ASR_ERR_ARG);
    EXPECT(asr_embed_fwd(F, 32, D, 32, L, L, 1.0, nullptr, 32, 6, 32, 11, 8, nullptr), ASR_ERR_ARG);
    EXPECT(asr_embed_fwd(F, 32, D, 32, L, nullptr, 1.0, F, 32, 6, 32, 11, 8, nullptr), ASR_ERR_ARG);   // pe without pos
    EXPECT(em(0), ASR_ERR_ARG);
    EXPECT(em(-6), ASR_ERR_ARG);
    EXPECT(em(6, 0), ASR_ERR_ARG);
    EXPECT(em(6, 32, 0), ASR_ERR_ARG);
    EXPECT(em(6, 32, 11, 0), ASR_ERR_ARG);
    EXPECT(em(6, 32, 11, -1), ASR_ERR_ARG);
    EXPECT(em(6, 32, 11, 8, 31), ASR_ERR_ARG);
    EXPECT(asr_embed_fwd(F, 32, D, 31, L, L, 1.0, F, 32, 6, 32, 11, 8, nullptr), ASR_ERR_ARG);
    EXPECT(asr_embed_fwd(F, 32, D, 32, L, L, 1.0, F, 8, 6, 32, 11, 8, nullptr), ASR_ERR_ARG);
    EXPECT(em(6, 32, 11, 8, -1, NAN), ASR_ERR_ARG);
    EXPECT(em(6, 32, 11, 8, -1, INFINITY), ASR_ERR_ARG);
    EXPECT(em(1 << 20, 1 << 12, 11, 8, 31), ASR_ERR_ARG);               // before unsupported
    EXPECT(em(1 << 20, 1 << 12), ASR_ERR_UNSUPPORTED);
    EXPECT(asr_embed_fwd(F, 1 << 12, nullptr, 0, L, nullptr, 1.0, F, 1 << 12, 1 << 20, 1 << 12, 11, 0, nullptr),
           ASR_ERR_UNSUPPORTED);                                         // no pe: pos, ldp and P are ignored

    // asr_attn_beam_step and its host twin: the same checks
    for (int host = 0; host < 2; host++) {
        const bool h = host != 0;
        asr_attn_beam_desc d = bbase();
        EXPECT(h ? asr_attn_beam_step_host(nullptr, F, 11, D, L, L, L, D, L, L, L, L2, L2, L)
                 : asr_attn_beam_step(nullptr, F, 11, D, L, L, L, D, L, L, L, L2, L2, L, nullptr), ASR_ERR_ARG);
        EXPECT(h ? asr_attn_beam_step_host(&d, nullptr, 11, D, L, L, L, D, L, L, L, L2, L2, L)
                 : asr_attn_beam_step(&d, nullptr, 11, D, L, L, L, D, L, L, L, L2, L2, L, nullptr), ASR_ERR_ARG);
        EXPECT(h ? asr_attn_beam_step_host(&d, F, 11, nullptr, L, L, L, D, L, L, L, L2, L2, L)
                 : asr_attn_beam_step(&d, F, 11, nullptr, L, L, L, D, L, L, L, L2, L2, L, nullptr), ASR_ERR_ARG);
        EXPECT(h ? asr_attn_beam_step_host(&d, F, 11, D, nullptr, L, L, D, L, L, L, L2, L2, L)
                 : asr_attn_beam_step(&d, F, 11, D, nullptr, L, L, D, L, L, L, L2, L2, L, nullptr), ASR_ERR_ARG);
        EXPECT(h ? asr_attn_beam_step_host(&d, F, 11, D, L, nullptr, L, D, L, L, L, L2, L2, L)
                 : asr_attn_beam_step(&d, F, 11, D, L, nullptr, L, D, L, L, L, L2, L2, L, nullptr), ASR_ERR_ARG);
        EXPECT(h ? asr_attn_beam_step_host(&d, F, 11, D, L, L, nullptr, D, L, L, L, L2, L2, L)
                 : asr_attn_beam_step(&d, F, 11, D, L, L, nullptr, D, L, L, L, L2, L2, L, nullptr), ASR_ERR_ARG);
        EXPECT(h ? asr_attn_beam_step_host(&d, F, 11, D, L, L, L, nullptr, L, L, L, L2, L2, L)
                 : asr_attn_beam_step(&d, F, 11, D, L, L, L, nullptr, L, L, L, L2, L2, L, nullptr), ASR_ERR_ARG);
        EXPECT(h ? asr_attn_beam_step_host(&d, F, 11, D, L, L, L, D, nullptr, L, L, L2, L2, L)
                 : asr_attn_beam_step(&d, F, 11, D, L, L, L, D, nullptr, L, L, L2, L2, L, nullptr), ASR_ERR_ARG);
        EXPECT(h ? asr_attn_beam_step_host(&d, F, 11, D, L, L, L, D, L, nullptr, L, L2, L2, L)
                 : asr_attn_beam_step(&d, F, 11, D, L, L, L, D, L, nullptr, L, L2, L2, L, nullptr), ASR_ERR_ARG);
        EXPECT(h ? asr_attn_beam_step_host(&d, F, 11, D, L, L, L, D, L, L, nullptr, L2, L2, L)
                 : asr_attn_beam_step(&d, F, 11, D, L, L, L, D, L, L, nullptr, L2, L2, L, nullptr), ASR_ERR_ARG);
        EXPECT(h ? asr_attn_beam_step_host(&d, F, 11, D, L, L, L, D, L, L, L, nullptr, L2, L)
                 : asr_attn_beam_step(&d, F, 11, D, L, L, L, D, L, L, L, nullptr, L2, L, nullptr), ASR_ERR_ARG);
        EXPECT(h ? asr_attn_beam_step_host(&d, F, 11, D, L, L, L, D, L, L, L, L2, nullptr, L)
                 : asr_attn_beam_step(&d, F, 11, D, L, L, L, D, L, L, L, L2, nullptr, L, nullptr), ASR_ERR_ARG);
        EXPECT(h ? asr_attn_beam_step_host(&d, F, 11, D, L, L, L, D, L, L, L, L2, L2, nullptr)
                 : asr_attn_beam_step(&d, F, 11, D, L, L, L, D, L, L, L, L2, L2, nullptr, nullptr), ASR_ERR_ARG);
        d = bbase(); d.B = 0; EXPECT(bs(d, -1, h), ASR_ERR_ARG);
        d = bbase(); d.K = 0; EXPECT(bs(d, -1, h), ASR_ERR_ARG);
        d = bbase(); d.K = 17; EXPECT(bs(d, -1, h), ASR_ERR_ARG);
        d = bbase(); d.V = 0; EXPECT(bs(d, 11, h), ASR_ERR_ARG);
        d = bbase(); d.max_len = 0; EXPECT(bs(d, -1, h), ASR_ERR_ARG);
        d = bbase(); d.step = -1; EXPECT(bs(d, -1, h), ASR_ERR_ARG);
        d = bbase(); d.step = 8; EXPECT(bs(d, -1, h), ASR_ERR_ARG);
        d = bbase(); d.eos = -1; EXPECT(bs(d, -1, h), ASR_ERR_ARG);
        d = bbase(); d.eos = 11; EXPECT(bs(d, -1, h), ASR_ERR_ARG);
        d = bbase(); EXPECT(bs(d, 10, h), ASR_ERR_ARG);
        // an out table that is its in table
        d = bbase();
        EXPECT(h ? asr_attn_beam_step_host(&d, F, 11, D, L, L, L, D, L, L, L, L, L2, L)
                 : asr_attn_beam_step(&d, F, 11, D, L, L, L, D, L, L, L, L, L2, L, nullptr), ASR_ERR_ARG);
        EXPECT(h ? asr_attn_beam_step_host(&d, F, 11, D, L, L, L, D, L, L, L, L2, L, L)
                 : asr_attn_beam_step(&d, F, 11, D, L, L, L, D, L, L, L, L2, L, L, nullptr), ASR_ERR_ARG);
        d = bbase(); d.B = 1 << 28; d.K = 16; EXPECT(bs(d, 10, h), ASR_ERR_ARG);    // before unsupported
        d = bbase(); d.B = 1 << 28; d.K = 16; EXPECT(bs(d, -1, h), ASR_ERR_UNSUPPORTED);
        d = bbase(); d.B = 1 << 20; d.max_len = 1 << 12; EXPECT(bs(d, -1, h), ASR_ERR_UNSUPPORTED);
    }
}

struct Cand {
    double s;
    int k, v;
};

// Random prunes of the twin against a restatement: every candidate listed, one stable sort by the documented order.
static void twin(unsigned seed, int B, int K, int V, int max_len, int step) {
    std::mt19937 rng(seed);
    std::uniform_int_distribution<int> coarse(-6, 0), pick(0, 9), tokd(0, V - 1);
    const int N = B * K, eos = V - 1;
    std::vector<float> logp((size_t)N * (V + 1));
    std::vector<double> sc(N), so(N);
    std::vector<int32_t> fin(N), fo(N), par(N), tok(N), tin((size_t)max_len * N), ain((size_t)max_len * N),
        tout((size_t)max_len * N, -7), aout((size_t)max_len * N, -7);
    for (auto& x : logp) x = 0.5f * (float)coarse(rng);              // a coarse grid: many exact ties
    for (int n = 0; n < N; n++) {
        const int r = pick(rng);
        sc[n] = r < 2 ? -(double)INFINITY : 0.25 * coarse(rng);
        fin[n] = r >= 7;
        if (r == 9) logp[(size_t)n * (V + 1) + tokd(rng)] = -INFINITY;
    }
    for (auto& x : tin) x = tokd(rng);
    for (int j = 0; j < max_len; j++)
        for (int n = 0; n < N; n++) ain[(size_t)j * N + n] = (n / K) * K + (int)(rng() % K);
    int32_t live = -1;
    asr_attn_beam_desc d{B, K, V, max_len, step, eos};
    EXPECT(asr_attn_beam_step_host(&d, logp.data(), V + 1, sc.data(), fin.data(), tin.data(), ain.data(), so.data(),
                                   fo.data(), par.data(), tok.data(), tout.data(), aout.data(), &live), ASR_OK);
    int want_live = 0, bad = 0;
    for (int b = 0; b < B; b++) {
        std::vector<Cand> c;
        for (int k = 0; k < K; k++) {
            const int n = b * K + k;
            if (sc[n] == -(double)INFINITY) continue;
            if (fin[n]) { c.push_back({sc[n], k, eos}); continue; }
            for (int v = 0; v < V; v++) {
                const double x = sc[n] + (double)logp[(size_t)n * (V + 1) + v];
                if (x != -(double)INFINITY) c.push_back({x, k, v});
            }
        }
        std::stable_sort(c.begin(), c.end(), [](const Cand& a, const Cand& e) { return a.s > e.s; });   // (k, v) order kept
        for (int k = 0; k < K; k++) {
            const int n = b * K + k;
            const bool has = k < (int)c.size();
            const int pk = has ? c[k].k : k, tv = has ? c[k].v : eos;
            const double s = has ? c[k].s : -(double)INFINITY;
            const int f = has && (fin[b * K + pk] || tv == eos);
            want_live += has && !f;
            bad += so[n] != s || fo[n] != f || par[n] != b * K + pk || tok[n] != tv;
            for (int j = 0; j < max_len; j++) {
                const int32_t wt = j < step ? tin[(size_t)j * N + b * K + pk] : j == step ? tv : -7;
                const int32_t wa = j <= step ? ain[(size_t)j * N + b * K + pk] : j == step + 1 ? n : -7;
                bad += tout[(size_t)j * N + n] != wt || aout[(size_t)j * N + n] != wa;
            }
        }
    }
    bad += live != want_live;
    if (bad) {
        std::printf("FAIL twin seed %u B %d K %d V %d step %d: %d differences\n", seed, B, K, V, step, bad);
        failures++;
    }
}

int main() {
    refusals();
    unsigned seed = 1;
    for (int K : {1, 2, 4, 16})
        for (int V : {1, 2, 5, 70})
            for (int rep = 0; rep < 12; rep++) {
                const int max_len = 1 + rep % 5;
                twin(seed++, 3, K, V, max_len, rep % max_len);
            }
    if (failures) {
        std::printf("attention-decode check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("attention-decode check: ok\n");
    return 0;
}
