// Conv2d over (time, frequency) (torch.nn.Conv2d semantics on [B][C][T][F]) in
// the library's time-major layout: asr_conv2d_out_frames / asr_conv2d_out_feats /
// asr_conv2d_fwd.  The first module of ESPnet / WeNet / NeMo / icefall
// encoders (Conv2dSubsampling) is two or three of these and a Linear.
//
// x row t*B + b holds F*c_in floats, element (f, ci) at f*c_in + ci; out row
// t'*B + b holds F_out*c_out floats, element (f', co) at f'*c_out + co; W is
// [kernel_t][kernel_f][c_in / groups][c_out].
//   out(t', b, f', co) = act(sum_jt sum_jf sum_ci xh(t' s_t - pt + jt, b, f' s_f - pf + jf, ci)
//                                               * W[jt][jf][ci][co] + bias[co])
// with xh = x inside the utterance's [0, len_b) x [0, F) and exactly 0 outside.
// The zero is SELECTED where x is fetched (the load is not issued), never made
// by multiplying with a mask: padding rows of x may hold NaN.
//
// Dense (groups == 1): the implicit GEMM of conv.hip's conv1d_dense_kernel with
// one generalisation.  M = T_out*B*F_out with flat row m = (t'*B + b)*F_out + f',
// N = c_out.  A tap is jt; a tap's "channels" are the RUN of kernel_f*c_in
// consecutive floats of input row (t' s_t - pt + jt)*B + b that starts at
// column (f' s_f - pf)*c_in (jf-major, ci-minor: contiguous in memory, and W's
// rows (jt, jf, ci) are in the same order), masked element-wise to
// [0, F*c_in).  Everything else is that kernel: a workgroup (4 waves) owns 128
// output rows x 64 output columns, a stage is (tap, 32 run elements), A and W
// go global -> registers -> LDS double buffered with one barrier per stage,
// v_mfma_f32_16x16x4_f32 whatever asr_set_dense_arith says.  Row metadata (t',
// b, f', len_b, run offset, live flag, output offset) is computed once per row
// before the stage loop.  Every output element is accumulated from a zero
// accumulator over jt ascending and, within jt, the run ascending in groups of
// 4 counted from the run's start with a zero-filled tail; groups wholly past
// the run are not issued.  c_in = 1 (a log-mel matrix as it stands) needs no
// special contract; when all taps fit one stage (kernel_t * roundup4(run) <= 32)
// the PACKED instantiation stages them together (below): the same MFMAs.
//
// The 16-byte path (c_in % 4 == 0, ldx % 4 == 0, d_x 16-byte aligned) loads the
// same values as the scalar path: the run's start and both mask edges are
// multiples of c_in, so a group of 4 is inside the row or outside it as a whole.
//
// Depthwise (groups == c_in == c_out): a VALU kernel, lanes across channels
// (coalesced loads and stores), one fmaf chain per output element over jt
// ascending, jf ascending from 0, then bias, then activation; the same zero
// selection.  x is read from global memory per tap (each element kernel_t *
// kernel_f / (s_t s_f) times, from L1 / L2); no LDS.
//
// An output element's bits depend on the values in its receptive field, the
// weights, the bias and the descriptor only.
#include "asr_internal.h"

#include <climits>
#include <cmath>
#include <cstddef>

namespace asr {

typedef float c2_f32x4 __attribute__((ext_vector_type(4)));

struct Conv2dArgs {
    const float* x;
    long ldx;
    const int32_t* lengths;
    const float* W;
    const float* bias;
    float* out;
    long ldo;
    int32_t* out_lengths;
    int T, B, T_out, F_out, M;     // M = T_out * B * F_out
    int c_in, c_out, F, FC;        // FC = F * c_in: floats of content in a row of x
    int kt, kf, R;                 // R = kf * c_in: the run of one tap
    int Rp;                        // R rounded up to a multiple of 4: the slots of a tap in the packed stage
    int st, sf, ptl, pth, pfl, act;
    float clip;
    int vec;                       // runs of x may be read with 16-byte loads
};

// Positions out for n positions in (n <= 0: none), dilation 1; the caller has checked the fields.
__host__ __device__ static inline long conv2d_count(long n, int k, int s, int lo, int hi) {
    if (n <= 0) return 0;
    const long span = n + lo + hi - k;
    return span < 0 ? 0 : span / s + 1;
}

__device__ __forceinline__ float conv2d_act(float v, int act, float clip) {
    if (act == ASR_CONV_ACT_RELU) return fmaxf(v, 0.f);
    if (act == ASR_CONV_ACT_CLIP) return fminf(fmaxf(v, 0.f), clip);
    return v;
}

__device__ __forceinline__ int conv2d_len(const int32_t* lengths, int b, int T) {
    return lengths ? min(max(lengths[b], 0), T) : T;
}

// d_out_lengths[b] = out_frames(len_b), by the first workgroup of the launch.
__device__ __forceinline__ void conv2d_write_lengths(const Conv2dArgs& p) {
    if (!p.out_lengths) return;
    for (int b = threadIdx.x; b < p.B; b += blockDim.x)
        p.out_lengths[b] = (int32_t)conv2d_count(conv2d_len(p.lengths, b, p.T), p.kt, p.st, p.ptl, p.pth);
}

// ---------------------------------------------------------------------------
// Dense kernel.  Grid (ceil(M / 128), ceil(c_out / 64)), 256 threads.
// Wave w computes rows [64 (w >> 1), +64) x columns [32 (w & 1), +32) of the
// tile: 4 x 2 MFMA tiles, 8 accumulator chains.
// ---------------------------------------------------------------------------
constexpr int C2_TM = 128;               // output rows per workgroup
constexpr int C2_TN = 64;                // output columns per workgroup
constexpr int C2_KC = 32;                // run elements per stage
constexpr int C2_LDA = C2_KC + 4;        // LDS row stride of A (floats): b128 reads of 16 rows hit 64 banks once
constexpr int C2_THREADS = 256;

// PACKED (kernel_t * Rp <= 32, e.g. the first layer's c_in = 1, 3 x 3): all of
// K in ONE stage.  Tap jt's run sits at stage slots [jt Rp, jt Rp + R), the
// slots up to the next multiple of 4 are zeros, so the MFMA groups are exactly
// those the general route issues tap by tap (jt ascending, the run in groups
// of 4 from its start with a zero-filled tail): the same bits, with one load
// round trip and one barrier instead of kernel_t.
template <bool PACKED>
__global__ __launch_bounds__(C2_THREADS) void conv2d_dense_kernel(const Conv2dArgs p) {
    // As[buf][row][16 sub + 4 g + m] = x-hat(row, run element 16 sub + 4 m + g of the stage)
    __shared__ __attribute__((aligned(16))) float As[PACKED ? 1 : 2][C2_TM * C2_LDA];   // PACKED: one stage, one buffer
    // Ws[buf][((4 sub + g) * 64 + col) * 4 + m] = W[jt][run element 16 sub + 4 m + g of the stage][n0 + col]
    __shared__ __attribute__((aligned(16))) float Ws[PACKED ? 1 : 2][C2_KC * C2_TN];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int m0 = blockIdx.x * C2_TM, n0 = blockIdx.y * C2_TN;
    if (blockIdx.x == 0 && blockIdx.y == 0) conv2d_write_lengths(p);

    // This thread fetches run elements [16 asub, +16) of every stage for row ar.
    const int ar = tid >> 1, asub = tid & 1;
    int alen = 0, atin0 = 0, aoff = 0;
    int alv = -1;                        // 1: the row computes; 0: zeros (past its utterance's count); -1: no such row
    long aoo = 0;                        // the row's first float in out: (t' B + b) ldo + f' c_out
    const float* xb = p.x;
    {
        const int m = m0 + ar;
        if (m < p.M) {
            const int tb = m / p.F_out, fq = m - tb * p.F_out;
            const int tq = tb / p.B, b = tb - tq * p.B;
            alen = conv2d_len(p.lengths, b, p.T);
            atin0 = tq * p.st - p.ptl;
            aoff = (fq * p.sf - p.pfl) * p.c_in;
            xb = p.x + (long)b * p.ldx;
            alv = tq < conv2d_count(alen, p.kt, p.st, p.ptl, p.pth) ? 1 : 0;
            aoo = (long)tb * p.ldo + (long)fq * p.c_out;
        }
    }
    const long fstride = (long)p.B * p.ldx;          // floats of x per frame
    // This thread fetches W rows (run elements) 16 e + 4 m + w (e = 0, 1; m = 0 .. 3), column n0 + lane.
    const int wcol = n0 + lane;
    const bool wcok = wcol < p.c_out;

    const int nq = (p.R + C2_KC - 1) / C2_KC;
    const int S = PACKED ? 1 : p.kt * nq;
    c2_f32x4 pa[4];                                  // pa[m][e]: run element 16 asub + 4 m + e of the stage
    float pw[2][4];
    auto fetch = [&](int j, int q) {
        const int s0 = (PACKED ? 0 : q * C2_KC) + 16 * asub;   // first run element (PACKED: stage slot) of this thread
#pragma unroll
        for (int m = 0; m < 4; m++) {
            int jt = j, r0 = s0 + 4 * m;             // tap and first run element of this group of 4
            if (PACKED) {
                jt = r0 / p.Rp;
                r0 -= jt * p.Rp;
            }
            const int tin = atin0 + jt;
            const bool rv = jt < p.kt && tin >= 0 && tin < alen;   // alen == 0 for a row past M
            const int pos0 = aoff + r0;              // the group's column in the row of x (may be < 0 or >= FC)
            const float* xr = xb + (long)(rv ? tin : 0) * fstride + pos0;
            pa[m] = c2_f32x4{0.f, 0.f, 0.f, 0.f};
            if (rv) {
                if (p.vec) {
                    if (r0 < p.R && pos0 >= 0 && pos0 < p.FC) pa[m] = *reinterpret_cast<const c2_f32x4*>(xr);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const int pos = pos0 + e;
                        if (r0 + e < p.R && pos >= 0 && pos < p.FC) pa[m][e] = xr[e];
                    }
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 2; e++)
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const int ch = 16 * e + 4 * m + w;
                int jt = j, r = q * C2_KC + ch;
                if (PACKED) {
                    jt = ch / p.Rp;
                    r = ch - jt * p.Rp;
                }
                pw[e][m] = (wcok && jt < p.kt && r < p.R) ? p.W[((long)jt * p.R + r) * p.c_out + wcol] : 0.f;
            }
    };
    auto stage = [&](int buf) {
        float* a = &As[buf][ar * C2_LDA + 16 * asub];
#pragma unroll
        for (int e = 0; e < 4; e++)
            *reinterpret_cast<c2_f32x4*>(a + 4 * e) = c2_f32x4{pa[0][e], pa[1][e], pa[2][e], pa[3][e]};
#pragma unroll
        for (int e = 0; e < 2; e++)
            *reinterpret_cast<c2_f32x4*>(&Ws[buf][((4 * e + w) * C2_TN + lane) * 4]) =
                c2_f32x4{pw[e][0], pw[e][1], pw[e][2], pw[e][3]};
    };

    c2_f32x4 acc[4][2];
#pragma unroll
    for (int rt = 0; rt < 4; rt++)
#pragma unroll
        for (int ct = 0; ct < 2; ct++) acc[rt][ct] = c2_f32x4{0.f, 0.f, 0.f, 0.f};
    const int wr = w >> 1, wc = w & 1;

    fetch(0, 0);
    stage(0);
    __syncthreads();
    int j = 0, q = 0;
    for (int sg = 0; sg < S; sg++) {
        const int buf = PACKED ? 0 : sg & 1;
        int jn = j, qn = q + 1;
        if (qn == nq) { qn = 0; jn = j + 1; }
        const bool more = sg + 1 < S;
        if (!PACKED && more) fetch(jn, qn);
        const int cc = PACKED ? p.kt * p.Rp : min(C2_KC, p.R - q * C2_KC);   // elements (slots) of this stage, >= 1
#pragma unroll
        for (int sub = 0; sub < 2; sub++) {
            const int rem = cc - 16 * sub;
            if (rem > 0) {
                c2_f32x4 af[4], bf[2];
#pragma unroll
                for (int rt = 0; rt < 4; rt++)
                    af[rt] = *reinterpret_cast<const c2_f32x4*>(
                        &As[buf][(64 * wr + 16 * rt + c) * C2_LDA + 16 * sub + 4 * g]);
#pragma unroll
                for (int ct = 0; ct < 2; ct++)
                    bf[ct] = *reinterpret_cast<const c2_f32x4*>(
                        &Ws[buf][((4 * sub + g) * C2_TN + 32 * wc + 16 * ct + c) * 4]);
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
        if (!PACKED && more) stage(buf ^ 1);
        __syncthreads();
        j = jn;
        q = qn;
    }

    // The stage buffers are free now (the loop's last barrier is behind every read of them): they carry
    // the rows' flags and output offsets to the epilogue, so the metadata costs no LDS of its own (with
    // it the general instantiation would not fit three workgroups per CU).
    int* const live = reinterpret_cast<int*>(&Ws[0][0]);       // [C2_TM]
    long* const ooff = reinterpret_cast<long*>(&As[0][0]);     // [C2_TM]
    if (asub == 0) {
        live[ar] = alv;
        ooff[ar] = aoo;
    }
    __syncthreads();
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
                const float v = conv2d_act(acc[rt][ct][i] + bv, p.act, p.clip);
                p.out[ooff[r] + col] = lv ? v : 0.f;
            }
    }
}

// ---------------------------------------------------------------------------
// Depthwise kernel.  Grid (ceil(M / 32), ceil(C / 64)), 256 threads: a lane is
// one channel of the workgroup's 64, wave w owns the 8 flat output positions
// m = 32 blockIdx.x + 8 w + u (m = (t' B + b) F_out + f' as in the dense kernel).
// ---------------------------------------------------------------------------
constexpr int D2_CH = 64;                // channels per workgroup (one per lane)
constexpr int D2_PER = 8;                // output positions per wave
constexpr int D2_TM = 4 * D2_PER;        // output positions per workgroup

__global__ __launch_bounds__(256) void conv2d_dw_kernel(const Conv2dArgs p) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (blockIdx.x == 0 && blockIdx.y == 0) conv2d_write_lengths(p);
    const int ch = blockIdx.y * D2_CH + lane;
    const bool cok = ch < p.c_out;
    const long fstride = (long)p.B * p.ldx;
    int tin0[D2_PER], fin0[D2_PER], len[D2_PER], lv[D2_PER];
    long xo[D2_PER], oo[D2_PER];
    float acc[D2_PER];
#pragma unroll
    for (int u = 0; u < D2_PER; u++) {
        const int m = blockIdx.x * D2_TM + D2_PER * w + u;   // uniform in the wave
        acc[u] = 0.f;
        tin0[u] = fin0[u] = len[u] = 0;
        xo[u] = oo[u] = 0;
        lv[u] = -1;
        if (m < p.M) {
            const int tb = m / p.F_out, fq = m - tb * p.F_out;
            const int tq = tb / p.B, b = tb - tq * p.B;
            len[u] = conv2d_len(p.lengths, b, p.T);
            tin0[u] = tq * p.st - p.ptl;
            fin0[u] = fq * p.sf - p.pfl;
            xo[u] = (long)b * p.ldx + ch;
            oo[u] = (long)tb * p.ldo + (long)fq * p.c_out + ch;
            lv[u] = tq < conv2d_count(len[u], p.kt, p.st, p.ptl, p.pth) ? 1 : 0;
            if (!lv[u]) len[u] = 0;                          // a zero row fetches nothing
        }
    }
    for (int jt = 0; jt < p.kt; jt++)
        for (int jf = 0; jf < p.kf; jf++) {
            const float wv = cok ? p.W[(long)(jt * p.kf + jf) * p.c_out + ch] : 0.f;
#pragma unroll
            for (int u = 0; u < D2_PER; u++) {
                const int tin = tin0[u] + jt, fin = fin0[u] + jf;
                float v = 0.f;
                if (cok && tin >= 0 && tin < len[u] && fin >= 0 && fin < p.F)   // len == 0 for a position past M
                    v = p.x[xo[u] + (long)tin * fstride + (long)fin * p.c_in];
                acc[u] = fmaf(v, wv, acc[u]);
            }
        }
    if (!cok) return;
    const float bv = p.bias ? p.bias[ch] : 0.f;
#pragma unroll
    for (int u = 0; u < D2_PER; u++) {
        if (lv[u] < 0) continue;
        const float v = conv2d_act(acc[u] + bv, p.act, p.clip);
        p.out[oo[u]] = lv[u] ? v : 0.f;
    }
}

// The limits of ASR_ERR_UNSUPPORTED (include/asr_amd.h states them).
constexpr int C2_MAX_KERNEL = 16, C2_MAX_STRIDE = 16, C2_MAX_CH = 4096, C2_MAX_FEAT = 4096, C2_MAX_FPAD = 4096;

// The descriptor's own checks: ASR_ERR_ARG first, then ASR_ERR_UNSUPPORTED.
static int conv2d_desc_arg(const asr_conv2d_desc* d) {
    if (!d) return ASR_ERR_ARG;
    if (d->c_in <= 0 || d->c_out <= 0 || d->feat_in <= 0) return ASR_ERR_ARG;
    if (d->kernel_t <= 0 || d->kernel_f <= 0 || d->stride_t <= 0 || d->stride_f <= 0) return ASR_ERR_ARG;
    if (d->pad_t_lo < 0 || d->pad_t_hi < 0 || d->pad_f_lo < 0 || d->pad_f_hi < 0) return ASR_ERR_ARG;
    if (d->act != ASR_CONV_ACT_NONE && d->act != ASR_CONV_ACT_RELU && d->act != ASR_CONV_ACT_CLIP) return ASR_ERR_ARG;
    if (d->act == ASR_CONV_ACT_CLIP && !(std::isfinite(d->clip) && d->clip > 0.f)) return ASR_ERR_ARG;
    // no output bin at all: the kernel does not fit feat_in and its padding
    if (conv2d_count(d->feat_in, d->kernel_f, d->stride_f, d->pad_f_lo, d->pad_f_hi) == 0) return ASR_ERR_ARG;
    return ASR_OK;
}
static bool conv2d_depthwise(const asr_conv2d_desc* d) {
    return d->groups != 1 && d->groups == d->c_in && d->groups == d->c_out;
}
static int conv2d_desc_unsupported(const asr_conv2d_desc* d) {
    if (d->groups != 1 && !conv2d_depthwise(d)) return ASR_ERR_UNSUPPORTED;
    if (d->kernel_t > C2_MAX_KERNEL || d->kernel_f > C2_MAX_KERNEL) return ASR_ERR_UNSUPPORTED;
    if (d->stride_t > C2_MAX_STRIDE || d->stride_f > C2_MAX_STRIDE) return ASR_ERR_UNSUPPORTED;
    if (d->c_in > C2_MAX_CH || d->c_out > C2_MAX_CH || d->feat_in > C2_MAX_FEAT) return ASR_ERR_UNSUPPORTED;
    if (d->pad_f_lo > C2_MAX_FPAD || d->pad_f_hi > C2_MAX_FPAD) return ASR_ERR_UNSUPPORTED;
    return ASR_OK;
}

}  // namespace asr

extern "C" {

int asr_conv2d_out_frames(const asr_conv2d_desc* d, int n_frames) {
    if (int rc = asr::conv2d_desc_arg(d)) return -rc;
    if (int rc = asr::conv2d_desc_unsupported(d)) return -rc;
    const long n = asr::conv2d_count(n_frames, d->kernel_t, d->stride_t, d->pad_t_lo, d->pad_t_hi);
    return n > INT_MAX ? -ASR_ERR_UNSUPPORTED : (int)n;
}

int asr_conv2d_out_feats(const asr_conv2d_desc* d) {
    if (int rc = asr::conv2d_desc_arg(d)) return -rc;
    if (int rc = asr::conv2d_desc_unsupported(d)) return -rc;
    // <= (4096 + 2 * 4096 - 1) / 1 + 1 after the checks above
    return (int)asr::conv2d_count(d->feat_in, d->kernel_f, d->stride_f, d->pad_f_lo, d->pad_f_hi);
}

int asr_conv2d_fwd(const asr_conv2d_desc* d, const float* d_x, long ldx, const int32_t* d_lengths, const float* d_W,
                   const float* d_b, float* d_out, long ldo, int32_t* d_out_lengths, int T, int B, asr_stream_t s) {
    if (!d || !d_x || !d_W || !d_out) return ASR_ERR_ARG;
    if (int rc = asr::conv2d_desc_arg(d)) return rc;
    const long F_out = asr::conv2d_count(d->feat_in, d->kernel_f, d->stride_f, d->pad_f_lo, d->pad_f_hi);   // >= 1
    if (T <= 0 || B <= 0) return ASR_ERR_ARG;
    // ldx < feat_in * c_in, ldo < F_out * c_out (by division: F_out * c_out may not fit a long before the limits)
    if (ldx < (long)d->feat_in * d->c_in || ldo / d->c_out < F_out) return ASR_ERR_ARG;
    const long T_out = asr::conv2d_count(T, d->kernel_t, d->stride_t, d->pad_t_lo, d->pad_t_hi);
    if (T_out == 0) return ASR_ERR_ARG;
    if (int rc = asr::conv2d_desc_unsupported(d)) return rc;
    // frame indices t' s_t - pad_t_lo + jt stay inside an int
    if ((long)T + d->pad_t_lo + d->pad_t_hi > (long)INT_MAX - 4096) return ASR_ERR_UNSUPPORTED;
    if ((long)T * B > INT_MAX || T_out * B > INT_MAX) return ASR_ERR_UNSUPPORTED;
    // flat output rows, and a workgroup's first row + 127, inside an int (F_out <= 12288 here)
    if (T_out * B * F_out > (long)INT_MAX - 128) return ASR_ERR_UNSUPPORTED;
    const long M = T_out * B * F_out;

    asr::Conv2dArgs p{};
    p.x = d_x; p.ldx = ldx; p.lengths = d_lengths; p.W = d_W; p.bias = d_b;
    p.out = d_out; p.ldo = ldo; p.out_lengths = d_out_lengths;
    p.T = T; p.B = B; p.T_out = (int)T_out; p.F_out = (int)F_out; p.M = (int)M;
    p.c_in = d->c_in; p.c_out = d->c_out; p.F = d->feat_in; p.FC = d->feat_in * d->c_in;
    p.kt = d->kernel_t; p.kf = d->kernel_f; p.R = d->kernel_f * d->c_in; p.Rp = (p.R + 3) & ~3;
    p.st = d->stride_t; p.sf = d->stride_f; p.ptl = d->pad_t_lo; p.pth = d->pad_t_hi; p.pfl = d->pad_f_lo;
    p.act = d->act; p.clip = d->clip;
    p.vec = (d->c_in % 4 == 0 && ldx % 4 == 0 && ((uintptr_t)d_x & 15) == 0) ? 1 : 0;

    // grid dimensions: x <= ceil(INT_MAX / 32) < 2^31, y <= 4096 / 64 = 64
    if (asr::conv2d_depthwise(d)) {
        const unsigned gx = (unsigned)((M + asr::D2_TM - 1) / asr::D2_TM);
        const unsigned gy = (unsigned)((d->c_out + asr::D2_CH - 1) / asr::D2_CH);
        hipLaunchKernelGGL(asr::conv2d_dw_kernel, dim3(gx, gy), dim3(256), 0, asr_stream(s), p);
        ASR_LAUNCH_TRY();
        return ASR_OK;
    }
    const unsigned gx = (unsigned)((M + asr::C2_TM - 1) / asr::C2_TM);
    const unsigned gy = (unsigned)((d->c_out + asr::C2_TN - 1) / asr::C2_TN);
    if ((long)p.kt * p.Rp <= asr::C2_KC)              // chosen by the descriptor alone; the bits are the same
        hipLaunchKernelGGL(asr::conv2d_dense_kernel<true>, dim3(gx, gy), dim3(asr::C2_THREADS), 0, asr_stream(s), p);
    else
        hipLaunchKernelGGL(asr::conv2d_dense_kernel<false>, dim3(gx, gy), dim3(asr::C2_THREADS), 0, asr_stream(s), p);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

}  // extern "C"
