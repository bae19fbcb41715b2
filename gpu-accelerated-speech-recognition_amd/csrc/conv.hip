// Conv1d over time (torch.nn.Conv1d semantics) in the library's time-major
// layout: asr_conv1d_out_frames / asr_conv1d_fwd.
//
// x row t*B + b holds c_in floats, out row t'*B + b holds c_out floats,
// W is [k][c_in / groups][c_out] (the library's [in][out] layout per tap).
//   out(t', b, co) = act((sum_{j<k} sum_{ci} xh(t'*s - pl + j*d, b, ci) * W[j][ci][co]) + bias[co])
// with xh = x inside the utterance ([0, len_b)) and exactly 0 outside it.  The
// zero is SELECTED where x is fetched (the load is not issued), never made by
// multiplying with a mask: padding rows of x may hold NaN.
//
// Dense (groups == 1): an implicit GEMM, M = T_out*B, N = c_out, K = k*c_in,
// on v_mfma_f32_16x16x4_f32 (exact fp32) whatever asr_set_dense_arith says.
// No im2col: tap j of output row (t', b) is input row (t'*s - pl + j*d)*B + b,
// so the k-loop walks k shifted row blocks of the same x.  A workgroup
// (4 waves) owns 128 output rows x 64 output columns; a stage is (tap j, 32
// channels).  A stage's A block (128 rows x 32 channels of x, shifted by the
// tap) and its slice of W[j] (32 x 64) go global -> registers -> LDS, double
// buffered, one barrier per stage, the next stage's loads in flight under the
// MFMAs of this one.  A is read straight from global memory once per tap (L2
// catches the k-fold reuse: the k taps of a row tile and its neighbours in
// time touch the same frames within a short window); no halo is staged.
// Row metadata (t', b, len_b) is computed once per row, by the thread that
// fetches the row, before the stage loop.
//
// Operand layouts are those of gated_rnn.hip: A[l & 15][k = l >> 4],
// B[k = l >> 4][l & 15], C rows 4g + i, column l & 15.  MFMA number m of a
// 16-channel group contracts channels 4m .. 4m+3 (lane group g supplies
// channel 4m + g), so every output element is accumulated from a zero
// accumulator over taps ascending and, within a tap, channels ascending in
// groups of 4 with a zero-filled tail; groups wholly past c_in are not
// issued.  LDS holds both operands permuted so that one ds_read_b128 yields a
// lane's operands of the four MFMAs of a 16-channel group.
//
// Depthwise (groups == c_in == c_out): a VALU kernel, lanes across channels
// (coalesced loads and stores), one fmaf chain per output element over the
// taps ascending from 0, then bias, then activation.  A workgroup owns one
// utterance, 64 channels and 64 output frames; the (64-1)*s + (k-1)*d + 1
// input frames they read and the k taps are staged in LDS once when they fit
// (224 rows of 64 floats together), else read from global memory per tap
// (same chain, same bits).
//
// An output row's bits depend on the values in its receptive field, the
// weights, the bias and the descriptor only: the kernel and its tiling depend
// on the descriptor alone, every element sees the same sequence of MFMAs /
// fmafs wherever its row sits, and the 16-byte-load path for aligned x rows
// loads the same values as the scalar path.
#include "asr_internal.h"

#include <climits>
#include <cmath>
#include <cstddef>

namespace asr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct ConvArgs {
    const float* x;
    long ldx;
    const int32_t* lengths;
    const float* W;
    const float* bias;
    float* out;
    long ldo;
    int32_t* out_lengths;
    int T, B, T_out, M;            // M = T_out * B
    int c_in, c_out, k, s, d, pl, pr, act;
    float clip;
    int vec;                       // rows of x may be read with 16-byte loads
};

// Frames out for n frames in (n <= 0: none); the caller has checked the fields.
__host__ __device__ static inline long conv_frames(long n, int k, int s, int d, int pl, int pr) {
    if (n <= 0) return 0;
    const long span = n + pl + pr - (long)d * (k - 1) - 1;
    return span < 0 ? 0 : span / s + 1;
}

__device__ __forceinline__ float conv_act(float v, int act, float clip) {
    if (act == ASR_CONV_ACT_RELU) return fmaxf(v, 0.f);
    if (act == ASR_CONV_ACT_CLIP) return fminf(fmaxf(v, 0.f), clip);
    return v;
}

__device__ __forceinline__ int conv_len(const int32_t* lengths, int b, int T) {
    return lengths ? min(max(lengths[b], 0), T) : T;
}

// d_out_lengths[b] = out_frames(len_b), by the first workgroup of the launch.
__device__ __forceinline__ void conv_write_lengths(const ConvArgs& p) {
    if (!p.out_lengths) return;
    for (int b = threadIdx.x; b < p.B; b += blockDim.x)
        p.out_lengths[b] = (int32_t)conv_frames(conv_len(p.lengths, b, p.T), p.k, p.s, p.d, p.pl, p.pr);
}

// ---------------------------------------------------------------------------
// Dense kernel.  Grid (ceil(M / 128), ceil(c_out / 64)), 256 threads.
// Wave w computes rows [64 (w >> 1), +64) x columns [32 (w & 1), +32) of the
// tile: 4 x 2 MFMA tiles, 8 accumulator chains.
// ---------------------------------------------------------------------------
constexpr int CV_TM = 128;               // output rows per workgroup
constexpr int CV_TN = 64;                // output columns per workgroup
constexpr int CV_KC = 32;                // channels per stage
constexpr int CV_LDA = CV_KC + 4;        // LDS row stride of A (floats): b128 reads of 16 rows hit 64 banks once
constexpr int CV_THREADS = 256;

__global__ __launch_bounds__(CV_THREADS) void conv1d_dense_kernel(const ConvArgs p) {
    // As[buf][row][16 sub + 4 g + m] = x-hat(row, channel 16 sub + 4 m + g of the stage)
    __shared__ __attribute__((aligned(16))) float As[2][CV_TM * CV_LDA];
    // Ws[buf][((4 sub + g) * 64 + col) * 4 + m] = W[j][channel 16 sub + 4 m + g of the stage][n0 + col]
    __shared__ __attribute__((aligned(16))) float Ws[2][CV_KC * CV_TN];
    __shared__ int live[CV_TM];          // 1: the row computes; 0: zeros (past its utterance's count); -1: no such row
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int m0 = blockIdx.x * CV_TM, n0 = blockIdx.y * CV_TN;
    if (blockIdx.x == 0 && blockIdx.y == 0) conv_write_lengths(p);

    // This thread fetches channels [16 asub, +16) of every stage for row ar.
    const int ar = tid >> 1, asub = tid & 1;
    int alen = 0, atin0 = 0;
    const float* xb = p.x;
    {
        const int m = m0 + ar;
        const bool ok = m < p.M;
        int lv = -1;
        if (ok) {
            const int tq = m / p.B, b = m - tq * p.B;
            alen = conv_len(p.lengths, b, p.T);
            atin0 = tq * p.s - p.pl;
            xb = p.x + (long)b * p.ldx;
            lv = tq < conv_frames(alen, p.k, p.s, p.d, p.pl, p.pr) ? 1 : 0;
        }
        if (asub == 0) live[ar] = lv;
    }
    const long fstride = (long)p.B * p.ldx;          // floats of x per frame
    // This thread fetches W rows (channels) 16 e + 4 m + w (e = 0, 1; m = 0 .. 3), column n0 + lane.
    const int wcol = n0 + lane;
    const bool wcok = wcol < p.c_out;

    const int nq = (p.c_in + CV_KC - 1) / CV_KC;
    const int S = p.k * nq;
    f32x4 pa[4];                                     // pa[m][e]: channel 16 asub + 4 m + e of the stage
    float pw[2][4];
    auto fetch = [&](int j, int q) {
        const int tin = atin0 + j * p.d;
        const bool rv = tin >= 0 && tin < alen;      // alen == 0 for a row past M
        const int ch0 = q * CV_KC + 16 * asub;
        const float* xr = xb + (long)(rv ? tin : 0) * fstride + ch0;
#pragma unroll
        for (int m = 0; m < 4; m++) {
            pa[m] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (rv) {
                if (p.vec) {
                    if (ch0 + 4 * m < p.c_in) pa[m] = *reinterpret_cast<const f32x4*>(xr + 4 * m);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        if (ch0 + 4 * m + e < p.c_in) pa[m][e] = xr[4 * m + e];
                }
            }
        }
        const float* wj = p.W + ((long)j * p.c_in + q * CV_KC) * p.c_out + wcol;
#pragma unroll
        for (int e = 0; e < 2; e++)
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const int ch = 16 * e + 4 * m + w;
                pw[e][m] = (wcok && q * CV_KC + ch < p.c_in) ? wj[(long)ch * p.c_out] : 0.f;
            }
    };
    auto stage = [&](int buf) {
        float* a = &As[buf][ar * CV_LDA + 16 * asub];
#pragma unroll
        for (int e = 0; e < 4; e++)
            *reinterpret_cast<f32x4*>(a + 4 * e) = f32x4{pa[0][e], pa[1][e], pa[2][e], pa[3][e]};
#pragma unroll
        for (int e = 0; e < 2; e++)
            *reinterpret_cast<f32x4*>(&Ws[buf][((4 * e + w) * CV_TN + lane) * 4]) =
                f32x4{pw[e][0], pw[e][1], pw[e][2], pw[e][3]};
    };

    f32x4 acc[4][2];
#pragma unroll
    for (int rt = 0; rt < 4; rt++)
#pragma unroll
        for (int ct = 0; ct < 2; ct++) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int wr = w >> 1, wc = w & 1;

    fetch(0, 0);
    stage(0);
    __syncthreads();
    int j = 0, q = 0;
    for (int st = 0; st < S; st++) {
        const int buf = st & 1;
        int jn = j, qn = q + 1;
        if (qn == nq) { qn = 0; jn = j + 1; }
        const bool more = st + 1 < S;
        if (more) fetch(jn, qn);
        const int cc = min(CV_KC, p.c_in - q * CV_KC);       // channels of this stage, >= 1
#pragma unroll
        for (int sub = 0; sub < 2; sub++) {
            const int rem = cc - 16 * sub;
            if (rem > 0) {
                f32x4 af[4], bf[2];
#pragma unroll
                for (int rt = 0; rt < 4; rt++)
                    af[rt] = *reinterpret_cast<const f32x4*>(
                        &As[buf][(64 * wr + 16 * rt + c) * CV_LDA + 16 * sub + 4 * g]);
#pragma unroll
                for (int ct = 0; ct < 2; ct++)
                    bf[ct] = *reinterpret_cast<const f32x4*>(
                        &Ws[buf][((4 * sub + g) * CV_TN + 32 * wc + 16 * ct + c) * 4]);
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    if (4 * m < rem) {
#pragma unroll
                        for (int rt = 0; rt < 4; rt++)
#pragma unroll
                            for (int ct = 0; ct < 2; ct++)
                                acc[rt][ct] =
                                    __builtin_amdgcn_mfma_f32_16x16x4f32(af[rt][m], bf[ct][m], acc[rt][ct], 0, 0, 0);
                    }
                }
            }
        }
        if (more) stage(buf ^ 1);
        __syncthreads();
        j = jn;
        q = qn;
    }

#pragma unroll
    for (int ct = 0; ct < 2; ct++) {
        const int col = n0 + 32 * wc + 16 * ct + c;
        if (col >= p.c_out) continue;
        const float bv = p.bias ? p.bias[col] : 0.f;
#pragma unroll
        for (int rt = 0; rt < 4; rt++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int r = 64 * wr + 16 * rt + 4 * g + i;
                const int lv = live[r];
                if (lv < 0) continue;
                const float v = conv_act(acc[rt][ct][i] + bv, p.act, p.clip);
                p.out[(long)(m0 + r) * p.ldo + col] = lv ? v : 0.f;
            }
    }
}

// ---------------------------------------------------------------------------
// Depthwise kernel.  One workgroup: utterance b, channels [64 ct, +64), output
// frames [64 tt, +64); wave w owns frames 16 w .. 16 w + 15 of those, a lane
// one channel.  blockIdx.x = (b * ntt + tt) * nct + ct.
// ---------------------------------------------------------------------------
constexpr int DW_CH = 64;                // channels per workgroup (one per lane)
constexpr int DW_PER = 16;               // output frames per wave
constexpr int DW_TT = 4 * DW_PER;        // output frames per workgroup
constexpr int DW_ROWS = 224;             // LDS rows of 64 floats at most (56 KiB): input frames + taps
constexpr int DW_BATCH = 16;             // staging loads in flight per thread

// LDS = true: dynamic LDS of (halo + k) rows: xs[halo][64] input frames, then ws[k][64] weights.
template <bool LDS>
__global__ __launch_bounds__(256) void conv1d_dw_kernel(const ConvArgs p, int nct, int ntt) {
    extern __shared__ float dw_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (blockIdx.x == 0) conv_write_lengths(p);
    int id = blockIdx.x;
    const int ct = id % nct;
    id /= nct;
    const int tt = id % ntt, b = id / ntt;
    const int ch = ct * DW_CH + lane;
    const bool cok = ch < p.c_out;
    const int len = conv_len(p.lengths, b, p.T);
    const int nout = (int)conv_frames(len, p.k, p.s, p.d, p.pl, p.pr);
    const int t0 = tt * DW_TT;                       // first output frame of the workgroup
    const int tbase = t0 * p.s - p.pl;               // input frame of halo row 0
    const float* xb = p.x + (long)b * p.ldx + ch;
    const long fstride = (long)p.B * p.ldx;
    const int halo = (DW_TT - 1) * p.s + (p.k - 1) * p.d + 1;
    float* const xs = dw_lds;
    float* const ws = dw_lds + halo * DW_CH;
    float acc[DW_PER];
#pragma unroll
    for (int u = 0; u < DW_PER; u++) acc[u] = 0.f;
    if (t0 < nout) {                                 // else the whole tile is zeros (uniform in the workgroup)
        if (LDS) {
            // rows [0, halo): input frames; rows [halo, halo + k): taps.  DW_BATCH loads, then their stores.
            const int rows = halo + p.k;
            for (int h0 = w; h0 < rows; h0 += 4 * DW_BATCH) {
                float v[DW_BATCH];
#pragma unroll
                for (int i = 0; i < DW_BATCH; i++) {
                    const int h = h0 + 4 * i;
                    const int tin = tbase + h;
                    v[i] = 0.f;
                    if (cok && h < halo) {
                        if (tin >= 0 && tin < len) v[i] = xb[(long)tin * fstride];
                    } else if (cok && h < rows) {
                        v[i] = p.W[(long)(h - halo) * p.c_out + ch];
                    }
                }
#pragma unroll
                for (int i = 0; i < DW_BATCH; i++) {
                    const int h = h0 + 4 * i;
                    if (h < rows) dw_lds[h * DW_CH + lane] = v[i];
                }
            }
            __syncthreads();
        }
#pragma unroll 2
        for (int j = 0; j < p.k; j++) {
            const float wj = LDS ? ws[j * DW_CH + lane] : cok ? p.W[(long)j * p.c_out + ch] : 0.f;
#pragma unroll
            for (int u = 0; u < DW_PER; u++) {
                const int h = (DW_PER * w + u) * p.s + j * p.d;
                float v;
                if (LDS) {
                    v = xs[h * DW_CH + lane];
                } else {
                    const int tin = tbase + h;
                    v = 0.f;
                    if (cok && tin >= 0 && tin < len) v = xb[(long)tin * fstride];
                }
                acc[u] = fmaf(v, wj, acc[u]);
            }
        }
    }
    if (!cok) return;
    const float bv = p.bias ? p.bias[ch] : 0.f;
#pragma unroll
    for (int u = 0; u < DW_PER; u++) {
        const int tq = t0 + DW_PER * w + u;
        if (tq >= p.T_out) break;
        const float v = conv_act(acc[u] + bv, p.act, p.clip);
        p.out[((long)tq * p.B + b) * p.ldo + ch] = tq < nout ? v : 0.f;
    }
}

// The descriptor's own checks: ASR_ERR_ARG first, then ASR_ERR_UNSUPPORTED.
static int conv_desc_arg(const asr_conv1d_desc* d) {
    if (!d) return ASR_ERR_ARG;
    if (d->c_in <= 0 || d->c_out <= 0 || d->kernel <= 0 || d->stride <= 0 || d->dilation <= 0) return ASR_ERR_ARG;
    if (d->pad_left < 0 || d->pad_right < 0) return ASR_ERR_ARG;
    if (d->act != ASR_CONV_ACT_NONE && d->act != ASR_CONV_ACT_RELU && d->act != ASR_CONV_ACT_CLIP) return ASR_ERR_ARG;
    if (d->act == ASR_CONV_ACT_CLIP && !(std::isfinite(d->clip) && d->clip > 0.f)) return ASR_ERR_ARG;
    return ASR_OK;
}
static bool conv_depthwise(const asr_conv1d_desc* d) {
    return d->groups != 1 && d->groups == d->c_in && d->groups == d->c_out;
}
static int conv_desc_unsupported(const asr_conv1d_desc* d) {
    if (d->groups != 1 && !conv_depthwise(d)) return ASR_ERR_UNSUPPORTED;
    if (d->kernel > 128 || d->stride > 16 || d->dilation > 16) return ASR_ERR_UNSUPPORTED;
    if (d->c_in > 4096 || d->c_out > 4096) return ASR_ERR_UNSUPPORTED;
    return ASR_OK;
}

}  // namespace asr

extern "C" {

int asr_conv1d_out_frames(const asr_conv1d_desc* d, int n_frames) {
    if (int rc = asr::conv_desc_arg(d)) return -rc;
    if (int rc = asr::conv_desc_unsupported(d)) return -rc;
    const long n = asr::conv_frames(n_frames, d->kernel, d->stride, d->dilation, d->pad_left, d->pad_right);
    return n > INT_MAX ? -ASR_ERR_UNSUPPORTED : (int)n;
}

int asr_conv1d_fwd(const asr_conv1d_desc* d, const float* d_x, long ldx, const int32_t* d_lengths, const float* d_W,
                   const float* d_b, float* d_out, long ldo, int32_t* d_out_lengths, int T, int B, asr_stream_t s) {
    if (!d || !d_x || !d_W || !d_out) return ASR_ERR_ARG;
    if (int rc = asr::conv_desc_arg(d)) return rc;
    if (T <= 0 || B <= 0 || ldx < d->c_in || ldo < d->c_out) return ASR_ERR_ARG;
    const long T_out = asr::conv_frames(T, d->kernel, d->stride, d->dilation, d->pad_left, d->pad_right);
    if (T_out == 0) return ASR_ERR_ARG;
    if (int rc = asr::conv_desc_unsupported(d)) return rc;
    // frame indices t'*s - pl + j*d (and a depthwise tile's halo past them) stay inside an int
    if ((long)T + d->pad_left + d->pad_right > (long)INT_MAX - 4096) return ASR_ERR_UNSUPPORTED;
    if ((long)T * B > INT_MAX || T_out * B > INT_MAX) return ASR_ERR_UNSUPPORTED;

    asr::ConvArgs p{};
    p.x = d_x; p.ldx = ldx; p.lengths = d_lengths; p.W = d_W; p.bias = d_b;
    p.out = d_out; p.ldo = ldo; p.out_lengths = d_out_lengths;
    p.T = T; p.B = B; p.T_out = (int)T_out; p.M = (int)(T_out * B);
    p.c_in = d->c_in; p.c_out = d->c_out; p.k = d->kernel; p.s = d->stride; p.d = d->dilation;
    p.pl = d->pad_left; p.pr = d->pad_right; p.act = d->act; p.clip = d->clip;
    p.vec = (d->c_in % 4 == 0 && ldx % 4 == 0 && ((uintptr_t)d_x & 15) == 0) ? 1 : 0;

    if (asr::conv_depthwise(d)) {
        const int nct = (d->c_out + asr::DW_CH - 1) / asr::DW_CH;
        const int ntt = (int)((T_out + asr::DW_TT - 1) / asr::DW_TT);
        const long blocks = (long)B * ntt * nct;
        if (blocks > INT_MAX) return ASR_ERR_UNSUPPORTED;     // one grid dimension
        const int halo = (asr::DW_TT - 1) * d->stride + (d->kernel - 1) * d->dilation + 1;
        if (halo + d->kernel <= asr::DW_ROWS)
            hipLaunchKernelGGL(asr::conv1d_dw_kernel<true>, dim3((unsigned)blocks), dim3(256),
                               (size_t)(halo + d->kernel) * asr::DW_CH * sizeof(float), asr_stream(s), p, nct, ntt);
        else
            hipLaunchKernelGGL(asr::conv1d_dw_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, asr_stream(s), p,
                               nct, ntt);
        ASR_LAUNCH_TRY();
        return ASR_OK;
    }
    const unsigned gx = (unsigned)((p.M + asr::CV_TM - 1) / asr::CV_TM);
    const unsigned gy = (unsigned)((d->c_out + asr::CV_TN - 1) / asr::CV_TN);
    hipLaunchKernelGGL(asr::conv1d_dense_kernel, dim3(gx, gy), dim3(asr::CV_THREADS), 0, asr_stream(s), p);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

}  // extern "C"
