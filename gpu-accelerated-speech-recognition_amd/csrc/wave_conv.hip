// The first layer of a wav2vec 2.0 / HuBERT feature encoder: asr_wave_conv_out_frames /
// asr_wave_conv_workspace_bytes / asr_wave_conv_fwd.
//
// A Conv1d with c_in = 1 over raw samples (batch-major [B][ldw], asr_fbank_fwd's
// convention) into time-major rows of C channels, then one of three tails:
//   NONE     gelu(v)                                   v = conv + bias
//   CHANNEL  gelu(LayerNorm_C(v) * gamma + beta)       over the C channels of a frame
//   TIME     gelu(((v - mean) * rstd) * gamma + beta)  mean / biased variance of channel c over
//                                                      the utterance's own frames: GroupNorm(C, C)
// k fmaf per output against 4 bytes stored: the kernels are store-bound and use no MFMA.
// A workgroup stages its span of samples in LDS once ((frames - 1) s + k floats; a sample at
// or past the utterance's count is SELECTED as zero, the load is not issued), lanes run
// across channels (coalesced stores, broadcast LDS reads) and every output is one fmaf
// chain over the taps ascending from a zero accumulator, then the bias is added.
//
// wave_conv_kernel (NONE and both passes of TIME): one workgroup = (utterance, 256 frames);
// wave w owns frames 64 w .. 64 w + 63 in four groups of 16 accumulators, and walks the
// channels in blocks of 64, one per lane.
// TIME never writes the un-normalised activations.  Pass 1 recomputes the convolution and
// keeps, per (utterance, 256-frame chunk, channel), the chunk's mean and centred sum of
// squares in fp64: a group's 16 values are centred on their own mean (so 1000 +- 1 is as
// accurate as +- 1), groups, waves and chunks are merged by Chan's update in a fixed order
// (groups ascending in a wave, waves ascending in a chunk, chunks ascending in wave_stats_kernel).
// The chunk grid depends on the frame index alone, so the statistics never depend on B, S
// or the strides.  wave_stats_kernel leaves (mean_hi, mean_lo, rstd) per (utterance, channel):
// the mean in two floats, since one fp32 mean centres a channel at 1000 +- 1 up to 3e-5 off.
// Pass 2 recomputes the convolution, normalises, applies GELU and stores.
//
// wave_conv_ln_kernel (CHANNEL): one workgroup = (utterance, 64 frames); a wave owns whole
// rows (16 frames, R at a time, lane l holding channels l, l + 64, ...), so the LayerNorm is
// done on registers with asr_layernorm_fwd's statistics (layernorm_row.h) before the store.
#include "asr_internal.h"
#include "gelu.h"
#include "layernorm_row.h"

#include <climits>
#include <cmath>
#include <cstddef>

namespace asr {

struct WaveArgs {
    const float* wave;
    long ldw;
    const int32_t* nsamples;
    const float *W, *bias, *gamma, *beta;
    double* part;                  // TIME: [B][nchunk][C][2] (mean, M2) of each chunk
    float* stats;                  // TIME: [B][C][3] (mean_hi, mean_lo, rstd)
    float* out;
    long ldo;
    int32_t* out_lengths;
    int B, S, T1, C, k, s, ntile;  // ntile: workgroups per utterance
    float eps;
};

constexpr int WV_TT = 256;                           // frames per workgroup = the statistics chunk
constexpr int WV_PER = 16;                           // accumulators per lane
constexpr int WV_HALO = (WV_TT - 1) * 16 + 32;       // staged samples at most (s <= 16, k <= 32)
constexpr int WL_TT = 64;                            // CHANNEL mode: frames per workgroup
constexpr int WL_HALO = (WL_TT - 1) * 16 + 32;

__host__ __device__ static inline long wave_frames(long n, int k, int s) { return n < k ? 0 : (n - k) / s + 1; }

__device__ __forceinline__ int wave_len(const WaveArgs& p, int b) {
    return p.nsamples ? min(max(p.nsamples[b], 0), p.S) : p.S;
}

__device__ __forceinline__ void wave_write_lengths(const WaveArgs& p) {
    if (!p.out_lengths) return;
    for (int b = threadIdx.x; b < p.B; b += blockDim.x)
        p.out_lengths[b] = (int32_t)wave_frames(wave_len(p, b), p.k, p.s);
}

// xs[i] = sample t0 * s + i of utterance b for i < (tt - 1) s + k, zero at or past its count n.
__device__ __forceinline__ void wave_stage(float* xs, const WaveArgs& p, int b, int t0, int tt, int n) {
    const int halo = (tt - 1) * p.s + p.k;
    const long i0 = (long)t0 * p.s;
    const float* wv = p.wave + (long)b * p.ldw;
    for (int i = threadIdx.x; i < halo; i += blockDim.x) xs[i] = (i0 + i < n) ? wv[i0 + i] : 0.f;
}

// Rows [r0, r1) of utterance b become zeros (the whole workgroup).
__device__ __forceinline__ void wave_zero_rows(const WaveArgs& p, int b, int r0, int r1) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int tq = r0 + w; tq < r1; tq += 4) {
        float* orow = p.out + ((long)tq * p.B + b) * p.ldo;
        for (int c = lane; c < p.C; c += 64) orow[c] = 0.f;
    }
}

// Chan's update: (n, mean, M2) absorbs a block of nb values with mean mb and centred sum of squares M2b.
__host__ __device__ static inline void chan_merge(double& n, double& mean, double& M2, double nb, double mb,
                                                  double M2b) {
    if (nb == 0.0) return;
    const double nt = n + nb, d = mb - mean;
    mean += d * (nb / nt);
    M2 += M2b + d * d * (n * nb / nt);
    n = nt;
}

// PASS 0: NONE.  PASS 1: TIME statistics (no store to out).  PASS 2: TIME apply.
template <int PASS>
__global__ __launch_bounds__(256) void wave_conv_kernel(const WaveArgs p) {
    __shared__ float xs[WV_HALO];
    __shared__ double red[2][4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (PASS != 1 && blockIdx.x == 0) wave_write_lengths(p);
    const int b = blockIdx.x / p.ntile, tile = blockIdx.x - b * p.ntile;
    const int n = wave_len(p, b);
    const int nout = (int)wave_frames(n, p.k, p.s);
    const int t0 = tile * WV_TT;
    const int tend = min(t0 + WV_TT, p.T1);
    if (t0 >= nout) {                                // uniform in the workgroup
        if (PASS != 1) wave_zero_rows(p, b, t0, tend);
        return;
    }
    wave_stage(xs, p, b, t0, WV_TT, n);
    __syncthreads();
    const int ncb = (p.C + 63) / 64;
    for (int cb = 0; cb < ncb; cb++) {
        const int c = cb * 64 + lane;
        const bool cok = c < p.C;
        const float bv = (cok && p.bias) ? p.bias[c] : 0.f;
        float hi = 0.f, lo = 0.f, rstd = 0.f, gm = 1.f, bt = 0.f;
        if (PASS == 2 && cok) {
            const float* st = p.stats + ((long)b * p.C + c) * 3;
            hi = st[0]; lo = st[1]; rstd = st[2];
            if (p.gamma) gm = p.gamma[c];
            if (p.beta) bt = p.beta[c];
        }
        double rn = 0.0, rmean = 0.0, rM2 = 0.0;
        for (int g = 0; g < 4; g++) {
            const int f0 = 64 * w + WV_PER * g;      // first frame of the group inside the tile
            if (t0 + f0 >= (PASS == 1 ? nout : tend)) break;
            float acc[WV_PER];
#pragma unroll
            for (int u = 0; u < WV_PER; u++) acc[u] = 0.f;
            for (int j = 0; j < p.k; j++) {
                const float wj = cok ? p.W[(long)j * p.C + c] : 0.f;
#pragma unroll
                for (int u = 0; u < WV_PER; u++) acc[u] = fmaf(xs[(f0 + u) * p.s + j], wj, acc[u]);
            }
            if (PASS == 1) {
                const int cnt = min(WV_PER, nout - (t0 + f0));
                double sum = 0.0;
#pragma unroll
                for (int u = 0; u < WV_PER; u++)
                    if (u < cnt) sum += (double)(acc[u] + bv);
                const double gmean = sum / (double)cnt;
                double gM2 = 0.0;
#pragma unroll
                for (int u = 0; u < WV_PER; u++)
                    if (u < cnt) {
                        const double dv = (double)(acc[u] + bv) - gmean;
                        gM2 += dv * dv;
                    }
                chan_merge(rn, rmean, rM2, (double)cnt, gmean, gM2);
            } else if (cok) {
#pragma unroll
                for (int u = 0; u < WV_PER; u++) {
                    const int tq = t0 + f0 + u;
                    if (tq < tend) {
                        float v = acc[u] + bv;
                        if (PASS == 2) v = (((v - hi) - lo) * rstd) * gm + bt;
                        p.out[((long)tq * p.B + b) * p.ldo + c] = tq < nout ? gelu_f32(v) : 0.f;
                    }
                }
            }
        }
        if (PASS == 1) {
            red[0][w][lane] = rmean;
            red[1][w][lane] = rM2;
            __syncthreads();
            if (w == 0 && cok) {
                double cn = 0.0, cmean = 0.0, cM2 = 0.0;
                for (int ww = 0; ww < 4; ww++) {
                    const int cnt = min(max(nout - (t0 + 64 * ww), 0), 64);
                    chan_merge(cn, cmean, cM2, (double)cnt, red[0][ww][lane], red[1][ww][lane]);
                }
                double* pt = p.part + (((long)b * p.ntile + tile) * p.C + c) * 2;
                pt[0] = cmean;
                pt[1] = cM2;
            }
            __syncthreads();
        }
    }
}

// One thread per (utterance, channel): the chunks' moments merged in ascending order.
__global__ __launch_bounds__(256) void wave_stats_kernel(const WaveArgs p) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)p.B * p.C) return;
    const int b = (int)(idx / p.C), c = (int)(idx - (long)b * p.C);
    const int nout = (int)wave_frames(wave_len(p, b), p.k, p.s);
    double n = 0.0, mean = 0.0, M2 = 0.0;
    for (int ch = 0; ch * WV_TT < nout; ch++) {
        const double* pt = p.part + (((long)b * p.ntile + ch) * p.C + c) * 2;
        chan_merge(n, mean, M2, (double)min(WV_TT, nout - ch * WV_TT), pt[0], pt[1]);
    }
    float* st = p.stats + idx * 3;
    const float hi = (float)mean;
    st[0] = hi;
    st[1] = (float)(mean - (double)hi);
    st[2] = nout > 0 ? (float)(1.0 / sqrt(M2 / n + (double)p.eps)) : 0.f;
}

// CHANNEL mode.  NU = channels per lane (a power of two >= ceil(C / 64)), R rows at a time.
template <int NU, int R>
__global__ __launch_bounds__(256) void wave_conv_ln_kernel(const WaveArgs p) {
    __shared__ float xs[WL_HALO];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (blockIdx.x == 0) wave_write_lengths(p);
    const int b = blockIdx.x / p.ntile, tile = blockIdx.x - b * p.ntile;
    const int n = wave_len(p, b);
    const int nout = (int)wave_frames(n, p.k, p.s);
    const int t0 = tile * WL_TT;
    const int tend = min(t0 + WL_TT, p.T1);
    if (t0 >= nout) {                                // uniform in the workgroup
        wave_zero_rows(p, b, t0, tend);
        return;
    }
    wave_stage(xs, p, b, t0, WL_TT, n);
    __syncthreads();
    for (int f = 16 * w; f < 16 * w + 16; f += R) {
        if (t0 + f >= tend) break;
        float acc[R][NU];
#pragma unroll
        for (int u = 0; u < NU; u++) {
            const int c = lane + 64 * u;
            const bool cok = c < p.C;
#pragma unroll
            for (int r = 0; r < R; r++) acc[r][u] = 0.f;
            if (64 * u < p.C) {                      // uniform in the wave
                for (int j = 0; j < p.k; j++) {
                    const float wj = cok ? p.W[(long)j * p.C + c] : 0.f;
#pragma unroll
                    for (int r = 0; r < R; r++) acc[r][u] = fmaf(xs[(f + r) * p.s + j], wj, acc[r][u]);
                }
                const float bv = (cok && p.bias) ? p.bias[c] : 0.f;
#pragma unroll
                for (int r = 0; r < R; r++) acc[r][u] = cok ? acc[r][u] + bv : 0.f;
            }
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int tq = t0 + f + r;
            if (tq >= tend) break;                   // uniform in the wave
            float* orow = p.out + ((long)tq * p.B + b) * p.ldo;
            if (tq >= nout) {
                for (int c = lane; c < p.C; c += 64) orow[c] = 0.f;
                continue;
            }
            const float rstd = ln_row_centre<NU>(acc[r], lane, p.C, p.eps);
#pragma unroll
            for (int u = 0; u < NU; u++) {
                const int c = lane + 64 * u;
                if (c < p.C) {
                    const float gm = p.gamma ? p.gamma[c] : 1.f;
                    const float bt = p.beta ? p.beta[c] : 0.f;
                    orow[c] = gelu_f32((acc[r][u] * rstd) * gm + bt);
                }
            }
        }
    }
}

// The descriptor's own checks: ASR_ERR_ARG first, then ASR_ERR_UNSUPPORTED.
static int wave_desc_check(const asr_wave_conv_desc* d) {
    if (!d) return ASR_ERR_ARG;
    if (d->channels <= 0 || d->kernel <= 0 || d->stride <= 0) return ASR_ERR_ARG;
    if (d->norm != ASR_WAVE_NORM_NONE && d->norm != ASR_WAVE_NORM_CHANNEL && d->norm != ASR_WAVE_NORM_TIME)
        return ASR_ERR_ARG;
    if (d->norm != ASR_WAVE_NORM_NONE && !(std::isfinite(d->eps) && d->eps >= 0.f)) return ASR_ERR_ARG;
    if (d->kernel > 32 || d->stride > 16 || d->channels > 4096) return ASR_ERR_UNSUPPORTED;
    return ASR_OK;
}

static size_t wave_part_bytes(long T1, int B, int C) {
    const long nchunk = (T1 + WV_TT - 1) / WV_TT;
    return (size_t)B * (size_t)nchunk * (size_t)C * 2 * sizeof(double);
}

}  // namespace asr

extern "C" {

int asr_wave_conv_out_frames(const asr_wave_conv_desc* d, int n_samples) {
    if (int rc = asr::wave_desc_check(d)) return -rc;
    return (int)asr::wave_frames(n_samples, d->kernel, d->stride);
}

size_t asr_wave_conv_workspace_bytes(const asr_wave_conv_desc* d, int S, int B) {
    if (asr::wave_desc_check(d) != ASR_OK || d->norm != ASR_WAVE_NORM_TIME || S <= 0 || B <= 0) return 0;
    const long T1 = asr::wave_frames(S, d->kernel, d->stride);
    if (T1 <= 0) return 0;
    return asr::wave_part_bytes(T1, B, d->channels) + (size_t)B * d->channels * 3 * sizeof(float);
}

int asr_wave_conv_fwd(const asr_wave_conv_desc* d, const float* d_wave, long ldw, const int32_t* d_nsamples,
                      const float* d_W, const float* d_b, const float* d_gamma, const float* d_beta, void* d_work,
                      float* d_out, long ldo, int32_t* d_out_lengths, int B, int S, asr_stream_t s) {
    if (!d || !d_wave || !d_W || !d_out) return ASR_ERR_ARG;
    const int rc = asr::wave_desc_check(d);
    if (rc == ASR_ERR_ARG) return rc;
    if (B <= 0 || S <= 0 || ldw < S || ldo < d->channels) return ASR_ERR_ARG;
    if (d->norm == ASR_WAVE_NORM_TIME && !d_work) return ASR_ERR_ARG;
    const long T1 = asr::wave_frames(S, d->kernel, d->stride);
    if (T1 == 0) return ASR_ERR_ARG;
    if (rc) return rc;
    if (T1 * B > INT_MAX) return ASR_ERR_UNSUPPORTED;
    const bool rows = d->norm == ASR_WAVE_NORM_CHANNEL;
    const int tt = rows ? asr::WL_TT : asr::WV_TT;
    const long ntile = (T1 + tt - 1) / tt;
    if (ntile * B > INT_MAX) return ASR_ERR_UNSUPPORTED;          // one grid dimension

    asr::WaveArgs p{};
    p.wave = d_wave; p.ldw = ldw; p.nsamples = d_nsamples; p.W = d_W; p.bias = d_b;
    p.gamma = d_gamma; p.beta = d_beta; p.out = d_out; p.ldo = ldo; p.out_lengths = d_out_lengths;
    p.B = B; p.S = S; p.T1 = (int)T1; p.C = d->channels; p.k = d->kernel; p.s = d->stride;
    p.ntile = (int)ntile; p.eps = d->eps;
    const dim3 grid((unsigned)(ntile * B));
    hipStream_t st = asr_stream(s);
    if (d->norm == ASR_WAVE_NORM_NONE) {
        hipLaunchKernelGGL(asr::wave_conv_kernel<0>, grid, dim3(256), 0, st, p);
    } else if (d->norm == ASR_WAVE_NORM_TIME) {
        p.part = static_cast<double*>(d_work);
        p.stats = reinterpret_cast<float*>(static_cast<char*>(d_work) + asr::wave_part_bytes(T1, B, d->channels));
        hipLaunchKernelGGL(asr::wave_conv_kernel<1>, grid, dim3(256), 0, st, p);
        hipLaunchKernelGGL(asr::wave_stats_kernel, dim3((unsigned)(((long)B * d->channels + 255) / 256)), dim3(256), 0,
                           st, p);
        hipLaunchKernelGGL(asr::wave_conv_kernel<2>, grid, dim3(256), 0, st, p);
    } else {
        const int nu = (d->channels + 63) / 64;
        if (nu <= 1) hipLaunchKernelGGL((asr::wave_conv_ln_kernel<1, 4>), grid, dim3(256), 0, st, p);
        else if (nu <= 2) hipLaunchKernelGGL((asr::wave_conv_ln_kernel<2, 4>), grid, dim3(256), 0, st, p);
        else if (nu <= 4) hipLaunchKernelGGL((asr::wave_conv_ln_kernel<4, 4>), grid, dim3(256), 0, st, p);
        else if (nu <= 8) hipLaunchKernelGGL((asr::wave_conv_ln_kernel<8, 4>), grid, dim3(256), 0, st, p);
        else if (nu <= 16) hipLaunchKernelGGL((asr::wave_conv_ln_kernel<16, 2>), grid, dim3(256), 0, st, p);
        else if (nu <= 32) hipLaunchKernelGGL((asr::wave_conv_ln_kernel<32, 1>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((asr::wave_conv_ln_kernel<64, 1>), grid, dim3(256), 0, st, p);
    }
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

}  // extern "C"
