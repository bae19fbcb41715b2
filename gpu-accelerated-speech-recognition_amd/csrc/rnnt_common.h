// What the transducer decoders share (rnnt.hip: greedy, rnnt_beam.hip: beam
// search): the handle, the MFMA column-tile product with its register ring, the
// running (max, argmax, sum-exp) of a row and the fp64 host model.
#pragma once
#include "dense.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <vector>

struct asr_rnnt {
    asr_rnnt_desc d{};
    std::vector<float> emb, wih[ASR_RNNT_MAX_LAYERS], whh[ASR_RNNT_MAX_LAYERS], bih[ASR_RNNT_MAX_LAYERS],
        bhh[ASR_RNNT_MAX_LAYERS], wenc, benc, wpred, bpred, wout, bout;
    int lds_bytes = 0;
    int64_t weight_bytes = 0;
    // device copy (asr_rnnt_upload): one allocation
    float* d_blob = nullptr;
    const float *d_embw = nullptr, *d_wih1 = nullptr, *d_whh[ASR_RNNT_MAX_LAYERS] = {}, *d_bih[ASR_RNNT_MAX_LAYERS] = {},
                *d_bhh[ASR_RNNT_MAX_LAYERS] = {}, *d_wenc = nullptr, *d_benc = nullptr, *d_wpred = nullptr,
                *d_bpred = nullptr, *d_wout = nullptr, *d_bout = nullptr;
};

namespace asr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RT_ROWS = 16;     // rows per workgroup (one MFMA row tile)
constexpr int RT_WAVES = 8;     // waves per workgroup; column tile j belongs to wave j % 8
constexpr int RT_DEPTH = 3;     // 16-k chunks of fragments in flight per wave
constexpr int RT_NONE = INT_MAX;    // argmax of an empty set
constexpr int RT_LDS_SMALL = 4096;  // bytes kept for the per-row walk state and the wave partials
constexpr int RT_LDS_MAX = 160 * 1024;

// LDS bytes of the decode kernel: h [2][L][16][Hp + 4], z [16][J + 4], the small area.
static long rnnt_lds_bytes(int L, int Hp, int J) {
    return ((long)2 * L * (Hp + 4) + (J + 4)) * RT_ROWS * 4 + RT_LDS_SMALL;
}

__device__ __forceinline__ float rt_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

// acc[q] += A(16 x 16*nch) . W[:, col[q]] for the lane's column of NQ tiles.
// a: this lane's row of A in LDS at k = 4g (row c of the tile); W: the matrix.
// MFMA (i, e) of lane group g contracts k = 16i + 4g + e, as in gated_rnn.hip; the
// fragments of chunk i + RT_DEPTH load while chunk i's MFMAs issue (loads past
// the last chunk re-read it and are not used).
template <int NQ>
__device__ __forceinline__ void rt_mma(const float* a, int nch, const float* __restrict__ W, unsigned ldw, int g,
                                       const int (&col)[NQ], f32x4 (&acc)[NQ]) {
    // one uniform base per k row and a 32-bit lane offset per tile
    unsigned off[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) off[q] = 4u * g * ldw + (unsigned)col[q];
    float4 av[RT_DEPTH];
    float bv[RT_DEPTH][4][NQ];
    auto fetch = [&](int u, int i) {
        const int ii = min(i, nch - 1);
        av[u] = *reinterpret_cast<const float4*>(a + 16 * ii);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float* be = W + (size_t)(16 * ii + e) * ldw;
#pragma unroll
            for (int q = 0; q < NQ; q++) bv[u][e][q] = be[off[q]];
        }
    };
#pragma unroll
    for (int u = 0; u < RT_DEPTH; u++) fetch(u, u);
    for (int i0 = 0; i0 < nch; i0 += RT_DEPTH) {
#pragma unroll
        for (int u = 0; u < RT_DEPTH; u++) {
            if (i0 + u < nch) {
                const float4 x = av[u];
#pragma unroll
                for (int q = 0; q < NQ; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, bv[u][0][q], acc[q], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < NQ; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, bv[u][1][q], acc[q], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < NQ; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, bv[u][2][q], acc[q], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < NQ; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, bv[u][3][q], acc[q], 0, 0, 0);
            }
            fetch(u, i0 + u + RT_DEPTH);
        }
    }
}

// Running (max, lowest argmax, sum of exp(x - max)) of a row.
struct RtTop {
    float m, s;
    int i;
};
__device__ __forceinline__ void rt_push(RtTop& a, float x, int n) {
    if (x > a.m) {
        a.s = (a.s == 0.f ? 0.f : a.s * expf(a.m - x)) + 1.f;
        a.m = x;
        a.i = n;
    } else {
        a.s += x == a.m ? 1.f : expf(x - a.m);
        if (x == a.m && n < a.i) a.i = n;
    }
}
// Symmetric in its arguments, bit for bit (both partners of a shuffle get the same result).
__device__ __forceinline__ RtTop rt_join(const RtTop& a, const RtTop& b) {
    RtTop r;
    r.m = b.m > a.m ? b.m : a.m;
    r.i = b.m > a.m ? b.i : (b.m == a.m ? min(a.i, b.i) : a.i);
    const float sa = a.s == 0.f ? 0.f : (a.m == r.m ? a.s : a.s * expf(a.m - r.m));
    const float sb = b.s == 0.f ? 0.f : (b.m == r.m ? b.s : b.s * expf(b.m - r.m));
    r.s = sa + sb;
    return r;
}

// ---------------------------------------------------------------------------
// Host model: one thread, fp64 accumulation from the fp32 weights.
// ---------------------------------------------------------------------------
struct RnntHost {
    const asr_rnnt& m;
    std::vector<double> gates, gx, x, g, f, z;
    explicit RnntHost(const asr_rnnt& mm) : m(mm) {
        const int in = std::max(m.d.D, m.d.Hp);
        gates.resize(4 * (size_t)m.d.Hp);
        gx.resize(4 * (size_t)m.d.Hp);
        x.resize(in);
        g.resize(m.d.J);
        f.resize(m.d.J);
        z.resize(m.d.J);
    }
    // y[n] = sum_k x[k] * W[k][n], k ascending
    static void matvec(const double* x, const float* W, int K, int N, double* y) {
        for (int n = 0; n < N; n++) y[n] = 0.0;
        for (int k = 0; k < K; k++) {
            const double xv = x[k];
            const float* row = W + (size_t)k * N;
            for (int n = 0; n < N; n++) y[n] += xv * (double)row[n];
        }
    }
    static double sigmoid(double v) { return 1.0 / (1.0 + std::exp(-v)); }
    // one predictor step on Emb[tok]; h, c: [L][Hp]
    void step(int tok, double* h, double* c) {
        const int Hp = m.d.Hp;
        int in = m.d.D;
        for (int k = 0; k < in; k++) x[k] = (double)m.emb[(size_t)tok * in + k];
        for (int l = 0; l < m.d.L; l++) {
            matvec(x.data(), m.wih[l].data(), in, 4 * Hp, gx.data());
            matvec(h + (size_t)l * Hp, m.whh[l].data(), Hp, 4 * Hp, gates.data());
            for (int n = 0; n < 4 * Hp; n++)
                gates[n] = (gx[n] + gates[n]) + ((double)m.bih[l][n] + (double)m.bhh[l][n]);
            for (int n = 0; n < Hp; n++) {
                const double ig = sigmoid(gates[n]), fg = sigmoid(gates[Hp + n]), gg = std::tanh(gates[2 * Hp + n]),
                             og = sigmoid(gates[3 * Hp + n]);
                const double cn = fg * c[(size_t)l * Hp + n] + ig * gg;
                c[(size_t)l * Hp + n] = cn;
                h[(size_t)l * Hp + n] = og * std::tanh(cn);
            }
            in = Hp;
            for (int k = 0; k < in; k++) x[k] = h[(size_t)l * Hp + k];
        }
    }
    void pred_proj(const double* h) {
        matvec(h + (size_t)(m.d.L - 1) * m.d.Hp, m.wpred.data(), m.d.Hp, m.d.J, g.data());
        for (int n = 0; n < m.d.J; n++) g[n] += (double)m.bpred[n];
    }
    void enc_proj(const float* e) {
        std::vector<double> ev(e, e + m.d.E);
        matvec(ev.data(), m.wenc.data(), m.d.E, m.d.J, f.data());
        for (int n = 0; n < m.d.J; n++) f[n] += (double)m.benc[n];
    }
};

}  // namespace asr
