// The middle of a Conformer convolution module in one launch:
// GLU -> depthwise Conv1d over time -> bias (a folded BatchNorm) -> activation
// (asr_glu_dwconv_fwd), in the library's time-major layout.
//
// u row t*B + b holds >= 2C floats: columns [0, C) the values, [C, 2C) the
// gates (torch's GLU over the channel dimension of the first pointwise
// convolution's output).  w is [k][C], out row t*B + b receives C floats.
//   g(t, b, c)   = u[t, b, c] / (1 + exp(-u[t, b, C + c]))   for 0 <= t < len_b, exactly 0 outside
//   out(t, b, c) = act((sum_{j<k} g(t - pl + j, b, c) * w[j][c]) + bias[c])
// Stride 1, dilation 1, pl + pr = k - 1, so T_out = T; rows t >= len_b are zeros.
// The zero of g is SELECTED where u is fetched (the loads are not issued),
// never made by multiplying with a mask: padding rows of u may hold NaN.
//
// A VALU kernel shaped like conv.hip's depthwise one: a workgroup owns one
// utterance, 64 channels (a lane each: both halves of u are read and out is
// written in 256-byte runs) and 64 output frames (16 per wave).  The
// 64 + k - 1 gated input frames and the k taps are staged in LDS once, the
// sigmoid evaluated there: once per staged element, not once per tap.  Then
// one fmaf chain per output element from 0 over the taps ascending, then the
// bias, then the activation.  LDS is (63 + 2k) rows of 256 bytes: 31 KiB at
// k = 31 (five workgroups, 20 waves, per CU of 160 KiB), 56 KiB at the limit
// k = 80, under the 64 KiB a workgroup gets without an attribute.  There is no
// second path: every supported k is staged.
//
// An output row's bits depend on the values in its receptive field, the
// weights, the bias and the descriptor only: every element is gated by the same
// expression and summed by the same chain wherever its row sits in a tile,
// whatever B, ldu, ldo and the alignment of u are (all loads are 4-byte ones).
#include "asr_internal.h"
#include "dense.h"

#include <climits>
#include <cstddef>

namespace asr {

struct GluConvArgs {
    const float* u;
    long ldu;
    const int32_t* lengths;
    const float* w;
    const float* bias;
    float* out;
    long ldo;
    int T, B, C, k, pl, act;
};

constexpr int GD_CH = 64;                // channels per workgroup (one per lane)
constexpr int GD_PER = 16;               // output frames per wave
constexpr int GD_TT = 4 * GD_PER;        // output frames per workgroup
constexpr int GD_BATCH = 8;              // staging rows in flight per thread (two loads each)
constexpr int GD_ROWS = GD_TT - 1 + 2 * ASR_GLU_DWCONV_MAX_KERNEL;   // LDS rows of 64 floats at most
static_assert(GD_ROWS * GD_CH * sizeof(float) <= 64 * 1024, "the staged tile fits a workgroup's default LDS");

__device__ __forceinline__ float glu_act(float v, int act) {
    if (act == ASR_GLU_ACT_RELU) return fmaxf(v, 0.f);
    if (act == ASR_GLU_ACT_SILU) return silu_f32(v);
    return v;
}

// blockIdx.x = (b * ntt + tt) * nct + ct.  Dynamic LDS: gs[halo][64] gated input
// frames, then ws[k][64] taps, halo = GD_TT + k - 1.
__global__ __launch_bounds__(256) void glu_dwconv_kernel(const GluConvArgs p, int nct, int ntt) {
    extern __shared__ float gd_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int id = blockIdx.x;
    const int ct = id % nct;
    id /= nct;
    const int tt = id % ntt, b = id / ntt;
    const int ch = ct * GD_CH + lane;
    const bool cok = ch < p.C;
    const int len = p.lengths ? min(max(p.lengths[b], 0), p.T) : p.T;
    const int t0 = tt * GD_TT;                       // first output frame of the workgroup
    const int tbase = t0 - p.pl;                     // input frame of halo row 0
    const int halo = GD_TT + p.k - 1;
    const float* const gs = gd_lds;
    const float* const ws = gd_lds + halo * GD_CH;
    float acc[GD_PER];
#pragma unroll
    for (int i = 0; i < GD_PER; i++) acc[i] = 0.f;
    if (t0 < len) {                                  // else the whole tile is zeros (uniform in the workgroup)
        const float* ub = p.u + (long)b * p.ldu + ch;
        const long fstride = (long)p.B * p.ldu;
        const int rows = halo + p.k;
        for (int h0 = w; h0 < rows; h0 += 4 * GD_BATCH) {
            float v[GD_BATCH], gt[GD_BATCH];
            bool in[GD_BATCH];
#pragma unroll
            for (int i = 0; i < GD_BATCH; i++) {
                const int h = h0 + 4 * i;
                const int tin = tbase + h;
                v[i] = 0.f;
                gt[i] = 0.f;
                in[i] = cok && h < halo && tin >= 0 && tin < len;
                if (in[i]) {
                    const float* r = ub + (long)tin * fstride;
                    v[i] = r[0];
                    gt[i] = r[p.C];
                } else if (cok && h >= halo && h < rows) {
                    v[i] = p.w[(long)(h - halo) * p.C + ch];
                }
            }
#pragma unroll
            for (int i = 0; i < GD_BATCH; i++) {
                const int h = h0 + 4 * i;
                // value * sigmoid(gate) in one division; a gate of -100 gives value / inf = 0
                if (h < rows) gd_lds[h * GD_CH + lane] = in[i] ? v[i] / (1.f + __expf(-gt[i])) : v[i];
            }
        }
        __syncthreads();
#pragma unroll 2
        for (int j = 0; j < p.k; j++) {
            const float wj = ws[j * GD_CH + lane];
#pragma unroll
            for (int i = 0; i < GD_PER; i++) acc[i] = fmaf(gs[(GD_PER * w + i + j) * GD_CH + lane], wj, acc[i]);
        }
    }
    if (!cok) return;
    const float bv = p.bias ? p.bias[ch] : 0.f;
#pragma unroll
    for (int i = 0; i < GD_PER; i++) {
        const int tq = t0 + GD_PER * w + i;
        if (tq >= p.T) break;
        const float v = glu_act(acc[i] + bv, p.act);
        p.out[((long)tq * p.B + b) * p.ldo + ch] = tq < len ? v : 0.f;
    }
}

}  // namespace asr

extern "C" {

int asr_glu_dwconv_fwd(const asr_glu_dwconv_desc* d, const float* d_u, long ldu, const int32_t* d_lengths,
                       const float* d_w, const float* d_b, float* d_out, long ldo, int T, int B, asr_stream_t s) {
    if (!d || !d_u || !d_w || !d_out) return ASR_ERR_ARG;
    if (T <= 0 || B <= 0 || d->channels <= 0 || d->kernel <= 0) return ASR_ERR_ARG;
    if (d->pad_left < 0 || d->pad_right < 0) return ASR_ERR_ARG;
    if (ldu < 2L * d->channels || ldo < d->channels) return ASR_ERR_ARG;
    if (d->act != ASR_GLU_ACT_NONE && d->act != ASR_GLU_ACT_RELU && d->act != ASR_GLU_ACT_SILU) return ASR_ERR_ARG;
    if (d_out == d_u) return ASR_ERR_ARG;
    if ((long)d->pad_left + d->pad_right != (long)d->kernel - 1) return ASR_ERR_UNSUPPORTED;
    if (d->kernel > ASR_GLU_DWCONV_MAX_KERNEL) return ASR_ERR_UNSUPPORTED;
    // frame indices t0 - pl + h of a tile's halo stay inside an int
    if ((long)T * B > INT_MAX || T > INT_MAX - 4096) return ASR_ERR_UNSUPPORTED;
    const long nct = ((long)d->channels + asr::GD_CH - 1) / asr::GD_CH;
    const int ntt = (T + asr::GD_TT - 1) / asr::GD_TT;
    const long blocks = (long)B * ntt * nct;
    if (blocks > INT_MAX) return ASR_ERR_UNSUPPORTED;         // one grid dimension

    asr::GluConvArgs p{};
    p.u = d_u; p.ldu = ldu; p.lengths = d_lengths; p.w = d_w; p.bias = d_b;
    p.out = d_out; p.ldo = ldo;
    p.T = T; p.B = B; p.C = d->channels; p.k = d->kernel; p.pl = d->pad_left; p.act = d->act;
    const size_t lds = (size_t)(asr::GD_TT - 1 + 2 * d->kernel) * asr::GD_CH * sizeof(float);
    hipLaunchKernelGGL(asr::glu_dwconv_kernel, dim3((unsigned)blocks), dim3(256), lds, asr_stream(s), p, (int)nct,
                       ntt);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

}  // extern "C"
