// The two depthwise-convolution pieces of an E-Branchformer block, time-major:
//
// asr_csgu_fwd: the convolutional spatial gating unit of a cgMLP branch.
// u row t*B + b holds >= 2C floats: columns [0, C) the values x_r, [C, 2C) the
// gates x_g (torch's chunk(2, dim=-1)).  w is [k][C].
//   n(t, b, c)   = (((x_g - mean0) - corr) * rstd) * gamma[c] + beta[c]   for 0 <= t < len_b, exactly 0 outside
//   out(t, b, c) = x_r(t, b, c) * ((sum_{j<k} n(t - pl + j, b, c) * w[j][c]) + bias[c])
// mean0 + corr is the refined mean of the C gates of the row and rstd =
// 1 / sqrt(var + eps), all three by asr_layernorm_fwd's expressions and tree.
//
// asr_merge_dwconv_fwd: the depthwise convolution over the concatenation of the
// two branches plus its own input.  x1, x2 rows hold >= C floats each, w is
// [k][2C], out rows >= 2C floats:
//   s(t, b, c')   = c' < C ? x1(t, b, c') : x2(t, b, c' - C)                for 0 <= t < len_b, exactly 0 outside
//   out(t, b, c') = s(t, b, c') + ((sum_{j<k} s(t - pl + j, b, c') * w[j][c']) + bias[c'])
// A depthwise convolution never mixes channels, so a lane picks its source
// once and the concatenation is never written.
//
// Both: stride 1, dilation 1, pl + pr = k - 1, rows t >= len_b of out are zeros,
// the zero of n / s SELECTED where the element is fetched (the load is not
// issued): padding rows may hold NaN.
//
// One staging core, the frame of glu_conv.hip: a workgroup owns one utterance,
// 64 channels (a lane each: 256-byte runs) and 64 output frames (16 per wave).
// The 64 + k - 1 input frames and the k taps are staged in LDS once, the CSGU's
// normalisation evaluated there (once per staged element, not once per tap),
// then one fmaf chain per output element from 0 over the taps ascending, then
// the bias, then the product / the residual.  The merge's residual term is
// read back from the staged tile, so each source is read once.  LDS is
// (63 + 2k) rows of 256 bytes: 31 KiB at k = 31, 56 KiB at the limit k = 80.
//
// The CSGU's row statistics need the whole gate row, which a 64-channel tile
// does not see: a pre-pass (one wave per row, the rows past the lengths not
// read) leaves (mean0, corr, rstd) per row in the caller's d_stats, and the
// conv kernel reads three wave-uniform floats per staged row.  The mean is
// kept in its two parts because one fp32 cannot hold it: a gate row at
// 1000 +- 1 would be centred up to 3e-5 off.
//
// An output row's bits depend on the values in its receptive field, the
// weights and the descriptor only: every element goes through the same
// expressions wherever its row sits in a tile, whatever T, B, the strides and
// the alignment are (all loads are 4-byte ones).  Compiled without FMA
// contraction: the operations are the written ones.
#include "asr_internal.h"

#include <climits>
#include <cmath>
#include <cstddef>

namespace asr {

struct CgArgs {
    const float* x1;         // CSGU: u (values at +0, gates at +C); merge: the first source
    const float* x2;         // merge: the second source
    long ld1, ld2;
    const int32_t* lengths;
    const float *gamma, *beta;
    const float* stats;      // CSGU: [T*B][3] (mean0, corr, rstd)
    const float* w;          // [k][nch]
    const float* bias;       // [nch] or NULL
    float* out;
    long ldo;
    int T, B, C, k, pl;
};

constexpr int CG_CH = 64;                // channels per workgroup (one per lane)
constexpr int CG_PER = 16;               // output frames per wave
constexpr int CG_TT = 4 * CG_PER;        // output frames per workgroup
constexpr int CG_BATCH = 8;              // staging rows in flight per thread
constexpr int CG_ROWS = CG_TT - 1 + 2 * ASR_CGMLP_MAX_KERNEL;   // LDS rows of 64 floats at most
static_assert(CG_ROWS * CG_CH * sizeof(float) <= 64 * 1024, "the staged tile fits a workgroup's default LDS");

// The fixed tree of asr_layernorm_fwd: butterfly l ^ 32, ^ 16, ... ^ 1.
__device__ __forceinline__ float cg_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Row statistics of the gate half, one wave per row; NU = columns per lane (a
// power of two >= ceil(C / 64)), a lane's columns l, l + 64, ... ascending.
template <int NU>
__global__ __launch_bounds__(256) void csgu_stats_kernel(const float* u, long ldu, const int32_t* lengths,
                                                         float* stats, float eps, int T, int B, int C, int M) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const int t = row / B, b = row - t * B;
    const int len = lengths ? min(max(lengths[b], 0), T) : T;
    if (t >= len) return;                                    // never read, and never read back
    const float* g = u + (long)row * ldu + C;
    float v[NU];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NU; i++) {
        const int col = lane + 64 * i;
        v[i] = col < C ? g[col] : 0.f;
        sum += v[i];
    }
    const float mean0 = cg_wave_sum(sum) / (float)C;
    float rs = 0.f;
#pragma unroll
    for (int i = 0; i < NU; i++) {
        v[i] = (lane + 64 * i < C) ? v[i] - mean0 : 0.f;
        rs += v[i];
    }
    const float corr = cg_wave_sum(rs) / (float)C;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < NU; i++) {
        v[i] = (lane + 64 * i < C) ? v[i] - corr : 0.f;
        sq += v[i] * v[i];
    }
    const float var = cg_wave_sum(sq) / (float)C;
    const float rstd = 1.f / sqrtf(var + eps);
    if (lane < 3) stats[3L * row + lane] = lane == 0 ? mean0 : lane == 1 ? corr : rstd;
}

// blockIdx.x = (b * ntt + tt) * nct + ct.  Dynamic LDS: xs[halo][64] staged
// input frames, then ws[k][64] taps, halo = CG_TT + k - 1.  nch: the channels
// of w, bias and out (C for the CSGU, 2C for the merge).
template <bool CSGU>
__global__ __launch_bounds__(256) void cg_dwconv_kernel(const CgArgs p, int nch, int nct, int ntt) {
    extern __shared__ float cg_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int id = blockIdx.x;
    const int ct = id % nct;
    id /= nct;
    const int tt = id % ntt, b = id / ntt;
    const int ch = ct * CG_CH + lane;
    const bool cok = ch < nch;
    const int len = p.lengths ? min(max(p.lengths[b], 0), p.T) : p.T;
    const int t0 = tt * CG_TT;                       // first output frame of the workgroup
    const int tbase = t0 - p.pl;                     // input frame of halo row 0
    const int halo = CG_TT + p.k - 1;
    const float* const xs = cg_lds;
    const float* const ws = cg_lds + halo * CG_CH;
    float acc[CG_PER];
#pragma unroll
    for (int i = 0; i < CG_PER; i++) acc[i] = 0.f;
    if (t0 < len) {                                  // else the whole tile is zeros (uniform in the workgroup)
        // the lane's column of frame 0 of utterance b, and the distance between its frames
        const float* src = nullptr;
        long fstride = 0;
        float gm = 1.f, bt = 0.f;
        if (cok) {
            if (CSGU) {
                src = p.x1 + (long)b * p.ld1 + p.C + ch;
                fstride = (long)p.B * p.ld1;
                if (p.gamma) gm = p.gamma[ch];
                if (p.beta) bt = p.beta[ch];
            } else if (ch < p.C) {
                src = p.x1 + (long)b * p.ld1 + ch;
                fstride = (long)p.B * p.ld1;
            } else {
                src = p.x2 + (long)b * p.ld2 + (ch - p.C);
                fstride = (long)p.B * p.ld2;
            }
        }
        const int rows = halo + p.k;
        for (int h0 = w; h0 < rows; h0 += 4 * CG_BATCH) {
            float v[CG_BATCH], m0[CG_BATCH], cr[CG_BATCH], rs[CG_BATCH];
            bool in[CG_BATCH];
#pragma unroll
            for (int i = 0; i < CG_BATCH; i++) {
                const int h = h0 + 4 * i;
                const int tin = tbase + h;
                v[i] = 0.f;
                m0[i] = cr[i] = rs[i] = 0.f;
                in[i] = cok && h < halo && tin >= 0 && tin < len;
                if (in[i]) {
                    v[i] = src[(long)tin * fstride];
                    if (CSGU) {
                        const float* st = p.stats + 3L * ((long)tin * p.B + b);
                        m0[i] = st[0];
                        cr[i] = st[1];
                        rs[i] = st[2];
                    }
                } else if (cok && h >= halo && h < rows) {
                    v[i] = p.w[(long)(h - halo) * nch + ch];
                }
            }
#pragma unroll
            for (int i = 0; i < CG_BATCH; i++) {
                const int h = h0 + 4 * i;
                float y = v[i];
                if (CSGU && in[i]) y = (((v[i] - m0[i]) - cr[i]) * rs[i]) * gm + bt;
                if (h < rows) cg_lds[h * CG_CH + lane] = y;
            }
        }
        __syncthreads();
#pragma unroll 2
        for (int j = 0; j < p.k; j++) {
            const float wj = ws[j * CG_CH + lane];
#pragma unroll
            for (int i = 0; i < CG_PER; i++) acc[i] = fmaf(xs[(CG_PER * w + i + j) * CG_CH + lane], wj, acc[i]);
        }
    }
    if (!cok) return;
    const float bv = p.bias ? p.bias[ch] : 0.f;
#pragma unroll
    for (int i = 0; i < CG_PER; i++) {
        const int tq = t0 + CG_PER * w + i;
        if (tq >= p.T) break;
        float y = 0.f;
        if (tq < len) {                              // t0 < len here: the tile was staged
            const float c = acc[i] + bv;
            if (CSGU) y = p.x1[((long)tq * p.B + b) * p.ld1 + ch] * c;
            else y = xs[(CG_PER * w + i + p.pl) * CG_CH + lane] + c;
        }
        p.out[((long)tq * p.B + b) * p.ldo + ch] = y;
    }
}

// The checks the two entry points share once their pointers are known good.
static int cg_check(int C, int k, int pl, int pr, long ld1, long ld2, long ldmin, long ldo, long nch, int T, int B,
                    float eps) {
    if (T <= 0 || B <= 0 || C <= 0 || k <= 0) return ASR_ERR_ARG;
    if (pl < 0 || pr < 0) return ASR_ERR_ARG;
    if (ld1 < ldmin || ld2 < ldmin || ldo < nch) return ASR_ERR_ARG;
    if (!std::isfinite(eps) || eps < 0.f) return ASR_ERR_ARG;
    return ASR_OK;
}

static int cg_limits(int C, int k, int pl, int pr, long nch, int T, int B, long* blocks, int* nct, int* ntt) {
    if ((long)pl + pr != (long)k - 1) return ASR_ERR_UNSUPPORTED;
    if (k > ASR_CGMLP_MAX_KERNEL) return ASR_ERR_UNSUPPORTED;
    if (C > 4096) return ASR_ERR_UNSUPPORTED;
    // frame indices t0 - pl + h of a tile's halo stay inside an int
    if ((long)T * B > INT_MAX || T > INT_MAX - 4096) return ASR_ERR_UNSUPPORTED;
    *nct = (int)((nch + CG_CH - 1) / CG_CH);
    *ntt = (T + CG_TT - 1) / CG_TT;
    *blocks = (long)B * *ntt * *nct;
    if (*blocks > INT_MAX) return ASR_ERR_UNSUPPORTED;         // one grid dimension
    return ASR_OK;
}

}  // namespace asr

extern "C" {

int asr_csgu_fwd(const asr_csgu_desc* d, const float* d_u, long ldu, const int32_t* d_lengths, const float* d_gamma,
                 const float* d_beta, const float* d_w, const float* d_b, float* d_stats, float* d_out, long ldo,
                 int T, int B, asr_stream_t s) {
    if (!d || !d_u || !d_w || !d_stats || !d_out) return ASR_ERR_ARG;
    const int C = d->channels;
    int rc = asr::cg_check(C, d->kernel, d->pad_left, d->pad_right, ldu, ldu, 2L * C, ldo, C, T, B, d->eps);
    if (rc) return rc;
    if (d_out == d_u) return ASR_ERR_ARG;
    long blocks;
    int nct, ntt;
    rc = asr::cg_limits(C, d->kernel, d->pad_left, d->pad_right, C, T, B, &blocks, &nct, &ntt);
    if (rc) return rc;

    hipStream_t st = asr_stream(s);
    const int M = T * B;
    const dim3 sgrid((unsigned)((M + 3) / 4));
    const int nu = (C + 63) / 64;
#define CG_STATS(NU) \
    hipLaunchKernelGGL(asr::csgu_stats_kernel<NU>, sgrid, dim3(256), 0, st, d_u, ldu, d_lengths, d_stats, d->eps, T, \
                       B, C, M)
    if (nu <= 1) CG_STATS(1);
    else if (nu <= 2) CG_STATS(2);
    else if (nu <= 4) CG_STATS(4);
    else if (nu <= 8) CG_STATS(8);
    else if (nu <= 16) CG_STATS(16);
    else if (nu <= 32) CG_STATS(32);
    else CG_STATS(64);
#undef CG_STATS
    ASR_LAUNCH_TRY();

    asr::CgArgs p{};
    p.x1 = d_u; p.ld1 = ldu; p.lengths = d_lengths; p.gamma = d_gamma; p.beta = d_beta; p.stats = d_stats;
    p.w = d_w; p.bias = d_b; p.out = d_out; p.ldo = ldo;
    p.T = T; p.B = B; p.C = C; p.k = d->kernel; p.pl = d->pad_left;
    const size_t lds = (size_t)(asr::CG_TT - 1 + 2 * d->kernel) * asr::CG_CH * sizeof(float);
    hipLaunchKernelGGL(asr::cg_dwconv_kernel<true>, dim3((unsigned)blocks), dim3(256), lds, st, p, C, nct, ntt);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

int asr_merge_dwconv_fwd(const asr_merge_dwconv_desc* d, const float* d_x1, long ldx1, const float* d_x2, long ldx2,
                         const int32_t* d_lengths, const float* d_w, const float* d_b, float* d_out, long ldo, int T,
                         int B, asr_stream_t s) {
    if (!d || !d_x1 || !d_x2 || !d_w || !d_out) return ASR_ERR_ARG;
    const int C = d->channels;
    int rc = asr::cg_check(C, d->kernel, d->pad_left, d->pad_right, ldx1, ldx2, C, ldo, 2L * C, T, B, 0.f);
    if (rc) return rc;
    if (d_out == d_x1 || d_out == d_x2) return ASR_ERR_ARG;
    long blocks;
    int nct, ntt;
    rc = asr::cg_limits(C, d->kernel, d->pad_left, d->pad_right, 2L * C, T, B, &blocks, &nct, &ntt);
    if (rc) return rc;

    asr::CgArgs p{};
    p.x1 = d_x1; p.ld1 = ldx1; p.x2 = d_x2; p.ld2 = ldx2; p.lengths = d_lengths;
    p.w = d_w; p.bias = d_b; p.out = d_out; p.ldo = ldo;
    p.T = T; p.B = B; p.C = C; p.k = d->kernel; p.pl = d->pad_left;
    const size_t lds = (size_t)(asr::CG_TT - 1 + 2 * d->kernel) * asr::CG_CH * sizeof(float);
    hipLaunchKernelGGL(asr::cg_dwconv_kernel<false>, dim3((unsigned)blocks), dim3(256), lds, asr_stream(s), p, 2 * C,
                       nct, ntt);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

}  // extern "C"
