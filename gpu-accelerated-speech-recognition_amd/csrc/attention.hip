// Self-attention over time and LayerNorm in the library's time-major layout:
// asr_attention_fwd / asr_layernorm_fwd.
//
// Attention.  Row i*B + b of q holds heads*head_dim floats (head h at columns
// [h*D, (h+1)*D)), k / v have Tk frames, out has Tq frames.  Query row i stands
// at absolute frame p = q_pos0 + i, key row j at r = k_pos0 + j.  Key r exists
// for utterance b iff 0 <= j < Tk and r < len_b; query p sees it iff it exists
// and p/chunk - left <= r/chunk <= p/chunk + right (a -1 drops that side).
//   out(p, b, h, :) = sum_r softmax_r(scale * q(p).k(r)) v(r)   over the keys p sees,
// exactly 0 for p >= len_b and for a query that sees no key.
//
// One workgroup (4 waves) owns (utterance b, head h, 64 query rows), a wave 16
// of them; grid (ceil(Tq / 64), heads, B).  Keys are walked in ascending blocks
// of 64 aligned on ABSOLUTE positions (block n = frames [64n, 64n + 64)); only
// the blocks that intersect the union of the tile's windows are visited.  The
// K and V blocks (64 keys x D, zero-filled to a multiple of 16 columns) are
// fetched global -> registers before the MFMAs of the block before them and
// written to LDS after them (one LDS copy of each, two barriers per block);
// rows of keys that do not exist are not loaded, their zeros are selected.
//
// Both products run on v_mfma_f32_16x16x4_f32 (A[l & 15][k = l >> 4],
// B[k = l >> 4][l & 15], C rows 4g + i, column l & 15; g = l >> 4, c = l & 15):
//  - S^T = K Q^T: A = K[key 16 kt + c][dim], B = Q[query c][dim]; the MFMA
//    (sub, mm) contracts dims 16 sub + 4 g + mm over g (so a lane's operands of
//    four MFMAs are one 16-byte read of natural-layout K and Q), sub ascending,
//    mm ascending.  Register i of tile kt then holds the score of key
//    16 kt + 4 g + i for query c: the lane's column is its query.
//  - O^T = V^T P^T: B = P^T[k = g][query c] is that same register i, A =
//    V[key 16 kt + 4 g + i][dim 16 dt + c]; P never leaves its registers.  The
//    result has dims 16 dt + 4 g + i of query c in a lane, so the running
//    maximum m, the sum l and the rescale factor are lane-local, and the
//    epilogue stores 16 bytes per (lane, dt).
// Softmax: fp32, online, exp on v_exp_f32.  Per block: masked scores are -inf by selection; the
// block maximum and the block sum are a fixed tree over the lane's 16 registers
// and then lanes l ^ 16, l ^ 32.  A block in which a query sees nothing leaves
// m, l and O bit-unchanged (factor exactly 1, P exactly 0; no -inf - -inf), and
// a wave none of whose queries sees anything in a block skips it.
//
// So an output row's bits depend only on its query, the keys and values it
// sees at their absolute positions, and the descriptor; 16-byte loads / stores
// of aligned rows move the same values as the scalar ones.
//
// LayerNorm.  One wave per row, the row in registers (lane l: columns l,
// l + 64, ...); two-pass mean / biased variance, the mean refined once by the
// mean of the centred values; sums are a lane's columns ascending, then the
// butterfly l ^ 32, ^ 16, ... ^ 1 (the tree of asr_lm_score).
#include "asr_internal.h"

#include <climits>
#include <cmath>
#include <cstddef>

namespace asr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct AttnArgs {
    const float *q, *k, *v;
    float* out;
    long ldq, ldk, ldv, ldo;
    const int32_t* lengths;
    int Tq, q_pos0, Tk, k_pos0, B;
    int D;                         // head_dim
    float scale;
    int chunk, left, right;
    int vq, vk, vv, vo;            // rows may be moved 16 bytes at a time
};

constexpr int AT_QT = 64;                        // query rows per workgroup
constexpr int AT_KB = ASR_ATTN_KEY_BLOCK;        // keys per block
static_assert(AT_KB == 64, "the kernel's tiling is written for 64-key blocks");

// Keys [lo, hi) that a live query at position pos sees, of the keys [k_pos0, kend) that exist.
__device__ __forceinline__ void attn_window(const AttnArgs& p, int pos, int kend, int& lo, int& hi) {
    const int qc = pos / p.chunk;
    lo = p.k_pos0;
    hi = kend;
    if (p.left >= 0) {
        const long v = ((long)qc - p.left) * p.chunk;        // <= pos
        if (v > lo) lo = (int)v;
    }
    if (p.right >= 0) {
        const long v = ((long)qc + p.right + 1) * p.chunk;
        if (v < hi) hi = (int)v;
    }
}

__device__ __forceinline__ f32x4 attn_load4(const float* src, bool vec) {
    if (vec) return *reinterpret_cast<const f32x4*>(src);
    return f32x4{src[0], src[1], src[2], src[3]};
}

// exp(x) for x <= 0 on v_exp_f32: the argument's rounding error is relative to |x| and exp(x) falls faster,
// so the result is within 1e-7 of expf's, at a sixth of its instructions.  exp(-inf) = 0.
__device__ __forceinline__ float attn_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }

// NDT = ceil(D / 16): 16-column tiles of a head.
// Two waves per SIMD at least: at most 256 registers, which makes the compiler keep the MFMA accumulators in
// VGPRs.  With the 512 of one wave per SIMD it put them in AGPRs and moved O and S between the two files around
// every rescale and every MFMA (540 v_accvgpr moves per key block at D = 64).
template <int NDT>
__global__ __launch_bounds__(256, 2) void attention_kernel(const AttnArgs p) {
    constexpr int LD = 16 * NDT + 4;             // LDS row stride: 16-byte reads of 16 rows and 4-byte reads of
                                                 // rows 4 apart both spread over the 64 banks
    __shared__ __attribute__((aligned(16))) float Ks[AT_KB * LD];
    __shared__ __attribute__((aligned(16))) float Vs[AT_KB * LD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int b = blockIdx.z, h = blockIdx.y, i0 = blockIdx.x * AT_QT;
    const int D = p.D;
    const float NEG = -INFINITY;

    const int len = p.lengths ? max(p.lengths[b], 0) : INT_MAX;
    const int kend = min(p.k_pos0 + p.Tk, len);              // keys [k_pos0, kend) exist

    // The blocks the tile visits: from its first query's lower bound to its last live query's upper bound.
    int nb0 = 0, nb1 = -1;
    {
        const int P0 = p.q_pos0 + i0;
        const int P1 = min(p.q_pos0 + min(p.Tq, i0 + AT_QT), len) - 1;
        if (P1 >= P0) {
            int lo, hi, t;
            attn_window(p, P0, kend, lo, t);
            attn_window(p, P1, kend, t, hi);
            if (hi > lo) {
                nb0 = lo / AT_KB;
                nb1 = (hi - 1) / AT_KB;
            }
        }
    }

    // This lane's query.
    const int iq = i0 + 16 * w + c;
    const int pos = p.q_pos0 + iq;
    const bool live = iq < p.Tq && pos < len;
    int rlo = 0, rhi = 0;
    if (live) attn_window(p, pos, kend, rlo, rhi);
    f32x4 qf[NDT];                                           // qf[sub][mm] = Q[query c][16 sub + 4 g + mm]
    {
        const float* qr = p.q + ((long)(live ? iq : 0) * p.B + b) * p.ldq + (long)h * D;
#pragma unroll
        for (int sub = 0; sub < NDT; sub++) {
            const int d0 = 16 * sub + 4 * g;
            qf[sub] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (live && d0 < D) qf[sub] = attn_load4(qr + d0, p.vq);
        }
    }

    // Thread tid fetches 4-float pieces e = tid + 256 u of a block: key e / (4 NDT), dims 4 (e % (4 NDT)) ...
    f32x4 kr[NDT], vr[NDT];
    auto fetch = [&](int n) {
#pragma unroll
        for (int u = 0; u < NDT; u++) {
            const int e = tid + 256 * u;
            const int key = e / (4 * NDT), d0 = 4 * (e % (4 * NDT));
            const int r = n * AT_KB + key;
            kr[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            vr[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (r >= p.k_pos0 && r < kend && d0 < D) {
                const long row = (long)(r - p.k_pos0) * p.B + b;
                kr[u] = attn_load4(p.k + row * p.ldk + (long)h * D + d0, p.vk);
                vr[u] = attn_load4(p.v + row * p.ldv + (long)h * D + d0, p.vv);
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int u = 0; u < NDT; u++) {
            const int e = tid + 256 * u;
            const int key = e / (4 * NDT), d0 = 4 * (e % (4 * NDT));
            *reinterpret_cast<f32x4*>(&Ks[key * LD + d0]) = kr[u];
            *reinterpret_cast<f32x4*>(&Vs[key * LD + d0]) = vr[u];
        }
    };

    f32x4 o[NDT];                                            // o[dt][i] = O[query c][16 dt + 4 g + i]
#pragma unroll
    for (int dt = 0; dt < NDT; dt++) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = NEG, l = 0.f;

    if (nb0 <= nb1) fetch(nb0);
    for (int n = nb0; n <= nb1; n++) {
        __syncthreads();                                     // the block before this one has been read
        stage();
        __syncthreads();
        if (n < nb1) fetch(n + 1);
        const int r0 = n * AT_KB;
        const bool any = rlo < rhi && rlo < r0 + AT_KB && rhi > r0;
        if (__builtin_amdgcn_ballot_w64(any) == 0) continue; // uniform in the wave; the barriers are above

        f32x4 s[4];
#pragma unroll
        for (int kt = 0; kt < 4; kt++) s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int sub = 0; sub < NDT; sub++) {
            f32x4 a[4];
#pragma unroll
            for (int kt = 0; kt < 4; kt++)
                a[kt] = *reinterpret_cast<const f32x4*>(&Ks[(16 * kt + c) * LD + 16 * sub + 4 * g]);
#pragma unroll
            for (int mm = 0; mm < 4; mm++) {
                if (16 * sub + mm < D) {
#pragma unroll
                    for (int kt = 0; kt < 4; kt++)
                        s[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kt][mm], qf[sub][mm], s[kt], 0, 0, 0);
                }
            }
        }
        // mask by selection, block maximum
        float bm = NEG;
#pragma unroll
        for (int kt = 0; kt < 4; kt++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int r = r0 + 16 * kt + 4 * g + i;
                const float sv = (r >= rlo && r < rhi) ? s[kt][i] * p.scale : NEG;
                s[kt][i] = sv;
                bm = fmaxf(bm, sv);
            }
        bm = fmaxf(bm, __shfl_xor(bm, 16));
        bm = fmaxf(bm, __shfl_xor(bm, 32));
        const float mn = fmaxf(m, bm);
        const float alpha = (m == mn) ? 1.f : attn_exp(m - mn);     // O and l are 0 while m is -inf
        float ps[4];
#pragma unroll
        for (int kt = 0; kt < 4; kt++) {
#pragma unroll
            for (int i = 0; i < 4; i++) s[kt][i] = (s[kt][i] == NEG) ? 0.f : attn_exp(s[kt][i] - mn);
            ps[kt] = (s[kt][0] + s[kt][1]) + (s[kt][2] + s[kt][3]);
        }
        float bs = (ps[0] + ps[1]) + (ps[2] + ps[3]);
        bs += __shfl_xor(bs, 16);
        bs += __shfl_xor(bs, 32);
        l = l * alpha + bs;
        m = mn;
#pragma unroll
        for (int dt = 0; dt < NDT; dt++) o[dt] *= alpha;
#pragma unroll
        for (int kt = 0; kt < 4; kt++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float* vrow = &Vs[(16 * kt + 4 * g + i) * LD + c];
#pragma unroll
                for (int dt = 0; dt < NDT; dt++)
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vrow[16 * dt], s[kt][i], o[dt], 0, 0, 0);
            }
    }

    if (iq >= p.Tq) return;
    const bool nz = live && l > 0.f;
    float* orow = p.out + ((long)iq * p.B + b) * p.ldo + (long)h * D;
#pragma unroll
    for (int dt = 0; dt < NDT; dt++) {
        const int d0 = 16 * dt + 4 * g;
        if (d0 >= D) continue;
        f32x4 r;
#pragma unroll
        for (int i = 0; i < 4; i++) r[i] = nz ? o[dt][i] / l : 0.f;
        if (p.vo) {
            *reinterpret_cast<f32x4*>(orow + d0) = r;
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) orow[d0 + i] = r[i];
        }
    }
}

// ---------------------------------------------------------------------------
// LayerNorm.  Grid ceil(M / 4) workgroups of 4 waves, one row per wave.
// NU = columns per lane (a power of two >= ceil(N / 64)).
// ---------------------------------------------------------------------------
struct LnArgs {
    const float *x, *res, *gamma, *beta;
    float* out;
    long ldx, ldr, ldo;
    const int32_t* lengths;
    float eps;
    int T, B, N, M;
};

__device__ __forceinline__ float ln_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

template <int NU>
__global__ __launch_bounds__(256) void layernorm_kernel(const LnArgs p) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + w;
    if (row >= p.M) return;
    const int t = row / p.B, b = row - t * p.B;
    const int len = p.lengths ? min(max(p.lengths[b], 0), p.T) : p.T;
    float* orow = p.out + (long)row * p.ldo;
    if (t >= len) {
#pragma unroll
        for (int u = 0; u < NU; u++)
            if (lane + 64 * u < p.N) orow[lane + 64 * u] = 0.f;
        return;
    }
    const float* xr = p.x + (long)row * p.ldx;
    const float* rr = p.res ? p.res + (long)row * p.ldr : nullptr;
    float v[NU];
    float sum = 0.f;
#pragma unroll
    for (int u = 0; u < NU; u++) {
        const int col = lane + 64 * u;
        v[u] = 0.f;
        if (col < p.N) v[u] = rr ? xr[col] + rr[col] : xr[col];
        sum += v[u];
    }
    // mean = mean0 + corr: the residual mean of v - mean0 takes out mean0's own rounding error, which is
    // relative to |v| (a row at 1000 +- 1 would otherwise be centred 5e-5 off)
    const float mean0 = ln_wave_sum(sum) / (float)p.N;
    float rs = 0.f;
#pragma unroll
    for (int u = 0; u < NU; u++) {
        v[u] = (lane + 64 * u < p.N) ? v[u] - mean0 : 0.f;
        rs += v[u];
    }
    const float corr = ln_wave_sum(rs) / (float)p.N;
    float sq = 0.f;
#pragma unroll
    for (int u = 0; u < NU; u++) {
        v[u] = (lane + 64 * u < p.N) ? v[u] - corr : 0.f;
        sq += v[u] * v[u];
    }
    const float var = ln_wave_sum(sq) / (float)p.N;
    const float rstd = 1.f / sqrtf(var + p.eps);
#pragma unroll
    for (int u = 0; u < NU; u++) {
        const int col = lane + 64 * u;
        if (col < p.N) {
            const float gm = p.gamma ? p.gamma[col] : 1.f;
            const float bt = p.beta ? p.beta[col] : 0.f;
            orow[col] = (v[u] * rstd) * gm + bt;
        }
    }
}

// Zero columns [0, N) of the rows past their utterance's length; one wave per row.
__global__ __launch_bounds__(256) void mask_rows_kernel(float* x, long ldx, const int32_t* lengths, int T, int B,
                                                        int N, int M) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int t = row / B, b = row - t * B;
    if (t < min(max(lengths[b], 0), T)) return;
    float* xr = x + (long)row * ldx;
    for (int col = lane; col < N; col += 64) xr[col] = 0.f;
}

static bool aligned16(const void* ptr, long ld) { return ((uintptr_t)ptr & 15) == 0 && ld % 4 == 0; }

}  // namespace asr

extern "C" {

int asr_attention_fwd(const asr_attn_desc* d, const float* d_q, long ldq, const float* d_k, long ldk,
                      const float* d_v, long ldv, const int32_t* d_lengths, float* d_out, long ldo, int Tq,
                      int q_pos0, int Tk, int k_pos0, int B, asr_stream_t s) {
    if (!d || !d_q || !d_k || !d_v || !d_out) return ASR_ERR_ARG;
    if (Tq <= 0 || Tk <= 0 || B <= 0 || d->heads <= 0 || d->head_dim <= 0 || d->chunk <= 0) return ASR_ERR_ARG;
    if (d->left < -1 || d->right < -1 || q_pos0 < 0 || k_pos0 < 0) return ASR_ERR_ARG;
    const long E = (long)d->heads * d->head_dim;
    if (ldq < E || ldk < E || ldv < E || ldo < E) return ASR_ERR_ARG;
    if (!std::isfinite(d->scale) || d->scale < 0.f) return ASR_ERR_ARG;
    if (d->head_dim % 4 != 0 || d->head_dim > 128 || E > 4096) return ASR_ERR_UNSUPPORTED;
    if (d->heads > 65535 || B > 65535) return ASR_ERR_UNSUPPORTED;                  // grid dimensions
    // key and query positions, and a block's end past them, stay inside an int
    if ((long)q_pos0 + Tq > (long)INT_MAX - 64 || (long)k_pos0 + Tk > (long)INT_MAX - 64) return ASR_ERR_UNSUPPORTED;
    if ((long)Tq * B > INT_MAX || (long)Tk * B > INT_MAX) return ASR_ERR_UNSUPPORTED;

    asr::AttnArgs p{};
    p.q = d_q; p.k = d_k; p.v = d_v; p.out = d_out;
    p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo;
    p.lengths = d_lengths;
    p.Tq = Tq; p.q_pos0 = q_pos0; p.Tk = Tk; p.k_pos0 = k_pos0; p.B = B;
    p.D = d->head_dim;
    p.scale = d->scale == 0.f ? 1.f / std::sqrt((float)d->head_dim) : d->scale;
    p.chunk = d->chunk; p.left = d->left; p.right = d->right;
    p.vq = asr::aligned16(d_q, ldq); p.vk = asr::aligned16(d_k, ldk);
    p.vv = asr::aligned16(d_v, ldv); p.vo = asr::aligned16(d_out, ldo);

    const dim3 grid((unsigned)((Tq + asr::AT_QT - 1) / asr::AT_QT), (unsigned)d->heads, (unsigned)B);
    hipStream_t st = asr_stream(s);
    switch ((d->head_dim + 15) / 16) {
        case 1: hipLaunchKernelGGL(asr::attention_kernel<1>, grid, dim3(256), 0, st, p); break;
        case 2: hipLaunchKernelGGL(asr::attention_kernel<2>, grid, dim3(256), 0, st, p); break;
        case 3: hipLaunchKernelGGL(asr::attention_kernel<3>, grid, dim3(256), 0, st, p); break;
        case 4: hipLaunchKernelGGL(asr::attention_kernel<4>, grid, dim3(256), 0, st, p); break;
        case 5: hipLaunchKernelGGL(asr::attention_kernel<5>, grid, dim3(256), 0, st, p); break;
        case 6: hipLaunchKernelGGL(asr::attention_kernel<6>, grid, dim3(256), 0, st, p); break;
        case 7: hipLaunchKernelGGL(asr::attention_kernel<7>, grid, dim3(256), 0, st, p); break;
        default: hipLaunchKernelGGL(asr::attention_kernel<8>, grid, dim3(256), 0, st, p); break;
    }
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

int asr_layernorm_fwd(const float* d_x, long ldx, const float* d_res, long ldr, const float* d_gamma,
                      const float* d_beta, float eps, const int32_t* d_lengths, float* d_out, long ldo, int T,
                      int B, int N, asr_stream_t s) {
    if (!d_x || !d_out) return ASR_ERR_ARG;
    if (T <= 0 || B <= 0 || N <= 0) return ASR_ERR_ARG;
    if (ldx < N || ldo < N || (d_res && ldr < N)) return ASR_ERR_ARG;
    if (!std::isfinite(eps) || eps < 0.f) return ASR_ERR_ARG;
    if (N > 4096) return ASR_ERR_UNSUPPORTED;
    if ((long)T * B > INT_MAX) return ASR_ERR_UNSUPPORTED;

    asr::LnArgs p{};
    p.x = d_x; p.res = d_res; p.gamma = d_gamma; p.beta = d_beta; p.out = d_out;
    p.ldx = ldx; p.ldr = ldr; p.ldo = ldo; p.lengths = d_lengths; p.eps = eps;
    p.T = T; p.B = B; p.N = N; p.M = T * B;
    const dim3 grid((unsigned)((p.M + 3) / 4));
    hipStream_t st = asr_stream(s);
    const int nu = (N + 63) / 64;
    if (nu <= 1) hipLaunchKernelGGL(asr::layernorm_kernel<1>, grid, dim3(256), 0, st, p);
    else if (nu <= 2) hipLaunchKernelGGL(asr::layernorm_kernel<2>, grid, dim3(256), 0, st, p);
    else if (nu <= 4) hipLaunchKernelGGL(asr::layernorm_kernel<4>, grid, dim3(256), 0, st, p);
    else if (nu <= 8) hipLaunchKernelGGL(asr::layernorm_kernel<8>, grid, dim3(256), 0, st, p);
    else if (nu <= 16) hipLaunchKernelGGL(asr::layernorm_kernel<16>, grid, dim3(256), 0, st, p);
    else if (nu <= 32) hipLaunchKernelGGL(asr::layernorm_kernel<32>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(asr::layernorm_kernel<64>, grid, dim3(256), 0, st, p);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

int asr_mask_rows(float* d_x, long ldx, const int32_t* d_lengths, int T, int B, int N, asr_stream_t s) {
    if (!d_x) return ASR_ERR_ARG;
    if (T <= 0 || B <= 0 || N <= 0 || ldx < N) return ASR_ERR_ARG;
    if ((long)T * B > INT_MAX) return ASR_ERR_UNSUPPORTED;
    if (!d_lengths) return ASR_OK;                           // every row is inside its utterance
    const int M = T * B;
    hipLaunchKernelGGL(asr::mask_rows_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, asr_stream(s), d_x, ldx,
                       d_lengths, T, B, N, M);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

}  // extern "C"
