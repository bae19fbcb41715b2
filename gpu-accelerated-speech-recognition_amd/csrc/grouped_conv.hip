// Grouped Conv1d over time with 1 < groups < c_in (stride 1, dilation 1), bias,
// optional GELU and an optional fused residual: asr_grouped_conv1d_out_frames /
// asr_grouped_conv1d_fwd.  The positional convolution of wav2vec 2.0 / HuBERT
// (Conv1d(E, E, 128, padding = 64, groups = 16) + SamePad + GELU, added to its input).
//
//   out(t', b, co) = res(t', b, co) + act((sum_{j<k} sum_{ci<cg_in} xh(t' - pl + j, b, g cg_in + ci)
//                                          W[j][ci][co]) + bias[co]),      g = co / cg_out
// xh = x inside the utterance and a SELECTED zero outside it (padding may hold NaN).
//
// The dense kernel of conv.hip re-reads its A block from L2 once per tap; with 128 taps at
// stride 1 every frame would be fetched 128 times.  Here a workgroup (4 waves) owns
// (utterance b, group g, GC_TT = 128 output frames) and stages the (GC_TT + k - 1) x cg_in
// window of x's group slice in LDS ONCE; tap j's A operand is that window read at row
// offset j.  Only W moves in the loop: a stage is (tap j, 16 input channels), its
// 16 x cg_out slice of W[j] goes global -> registers -> LDS, double buffered, one barrier
// per stage, the next stage's loads in flight under this stage's MFMAs.
//
// v_mfma_f32_16x16x4_f32 with the operand layouts of conv.hip: A[l & 15][l >> 4],
// B[l >> 4][l & 15], C rows 4 (l >> 4) + i, column l & 15.  Wave w computes rows
// [32 w, +32) x all NCT column tiles of the group: 2 x NCT accumulators.  MFMA m of a
// 16-channel block contracts channels 4m .. 4m + 3, so an output is accumulated from a
// zero accumulator over taps ascending and, in a tap, channels ascending in groups of 4
// with a zero-filled tail; groups wholly past cg_in are not issued.  Both operands sit in
// LDS permuted so that one ds_read_b128 yields a lane's operands of the four MFMAs of a
// block: window row r holds channel 16 q + 4 m + g4 at float 16 q + 4 g4 + m, row stride
// cin16 + 4 floats (cin16 = cg_in rounded up to 16; the 4 spreads the 16 rows of a read
// over the banks).
//
// A row's bits depend on its window, the weights and the descriptor only: the tiling
// follows the descriptor, every element sees the same MFMA sequence wherever its row
// sits, and x is read with scalar loads whatever ldx and the alignment are.
#include "asr_internal.h"
#include "gelu.h"

#include <climits>
#include <cstddef>

namespace asr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct GConvArgs {
    const float* x;
    long ldx;
    const int32_t* lengths;
    const float *W, *bias, *res;
    long ldr;
    float* out;
    long ldo;
    int32_t* out_lengths;
    int T, B, T_out;
    int cg_in, cg_out, c_out, k, pl, pr, act;
    int cin16, lda, rows;          // rows = GC_TT + k - 1 window rows of lda floats
};

constexpr int GC_TT = 128;         // output frames per workgroup
constexpr int GC_KC = 16;          // input channels per stage

__host__ __device__ static inline long gconv_frames(long n, int k, int pl, int pr) {
    if (n <= 0) return 0;
    const long f = n + pl + pr - k + 1;
    return f < 0 ? 0 : f;
}
__device__ __forceinline__ int gconv_len(const GConvArgs& p, int b) {
    return p.lengths ? min(max(p.lengths[b], 0), p.T) : p.T;
}

// Grid (ceil(T_out / GC_TT), groups, B), 256 threads, dynamic LDS: the window, then Ws[2][16][16 NCT].
template <int NCT>
__global__ __launch_bounds__(256) void grouped_conv1d_kernel(const GConvArgs p) {
    extern __shared__ __attribute__((aligned(16))) float gc_lds[];
    constexpr int NCOL = 16 * NCT;
    float* const win = gc_lds;
    float* const Ws = gc_lds + p.rows * p.lda;       // Ws[buf][(g4 * NCOL + col) * 4 + m] = W[j][16 q + 4 m + g4][col]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g4 = lane >> 4, c = lane & 15;
    const int t0 = blockIdx.x * GC_TT, grp = blockIdx.y, b = blockIdx.z;
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && p.out_lengths)
        for (int bb = tid; bb < p.B; bb += 256)
            p.out_lengths[bb] = (int32_t)gconv_frames(gconv_len(p, bb), p.k, p.pl, p.pr);
    const int len = gconv_len(p, b);
    const int nout = (int)gconv_frames(len, p.k, p.pl, p.pr);
    const int tend = min(t0 + GC_TT, p.T_out);
    float* const ob = p.out + (long)b * p.ldo + (long)grp * p.cg_out;
    const long ostride = (long)p.B * p.ldo;
    if (t0 >= nout) {                                // the whole tile is zeros (uniform in the workgroup)
        for (int e = tid; e < (tend - t0) * p.cg_out; e += 256) {
            const int r = e / p.cg_out, col = e - r * p.cg_out;
            ob[(long)(t0 + r) * ostride + col] = 0.f;
        }
        return;
    }

    // the window, once: row i = input frame t0 - pl + i, channels permuted per block of 16
    {
        const float* xb = p.x + (long)b * p.ldx + (long)grp * p.cg_in;
        const long fstride = (long)p.B * p.ldx;
        const int total = p.rows * p.cin16;
        for (int e = tid; e < total; e += 256) {
            const int i = e / p.cin16, pos = e - i * p.cin16;
            const int ch = (pos & ~15) + 4 * (pos & 3) + ((pos >> 2) & 3);
            const int tin = t0 - p.pl + i;
            float v = 0.f;
            if (ch < p.cg_in && tin >= 0 && tin < len) v = xb[(long)tin * fstride + ch];
            win[i * p.lda + pos] = v;
        }
    }

    const int nq = p.cin16 / GC_KC;
    const int S = p.k * nq;
    const float* const wg = p.W + (long)grp * p.cg_out;
    float pw[NCT];
    auto fetch = [&](int j, int q) {
#pragma unroll
        for (int i = 0; i < NCT; i++) {
            const int e = tid + 256 * i;
            const int chn = e / NCOL, col = e - chn * NCOL;
            const int ch = q * GC_KC + chn;
            pw[i] = (ch < p.cg_in && col < p.cg_out) ? wg[((long)j * p.cg_in + ch) * p.c_out + col] : 0.f;
        }
    };
    auto stage = [&](int buf) {
        float* ws = Ws + buf * (GC_KC * NCOL);
#pragma unroll
        for (int i = 0; i < NCT; i++) {
            const int e = tid + 256 * i;
            const int chn = e / NCOL, col = e - chn * NCOL;
            ws[((chn & 3) * NCOL + col) * 4 + (chn >> 2)] = pw[i];
        }
    };

    f32x4 acc[2][NCT];
#pragma unroll
    for (int rt = 0; rt < 2; rt++)
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

    fetch(0, 0);
    stage(0);
    __syncthreads();                                 // the window and the first W slice
    int j = 0, q = 0;
    for (int st = 0; st < S; st++) {
        const int buf = st & 1;
        int jn = j, qn = q + 1;
        if (qn == nq) { qn = 0; jn = j + 1; }
        const bool more = st + 1 < S;
        if (more) fetch(jn, qn);
        const int rem = p.cg_in - q * GC_KC;         // channels left in this block, >= 1
        const float* ws = Ws + buf * (GC_KC * NCOL);
        f32x4 af[2], bf[NCT];
#pragma unroll
        for (int rt = 0; rt < 2; rt++)
            af[rt] = *reinterpret_cast<const f32x4*>(&win[(32 * w + 16 * rt + c + j) * p.lda + GC_KC * q + 4 * g4]);
#pragma unroll
        for (int ct = 0; ct < NCT; ct++)
            bf[ct] = *reinterpret_cast<const f32x4*>(&ws[(g4 * NCOL + 16 * ct + c) * 4]);
#pragma unroll
        for (int m = 0; m < 4; m++) {
            if (4 * m < rem) {
#pragma unroll
                for (int rt = 0; rt < 2; rt++)
#pragma unroll
                    for (int ct = 0; ct < NCT; ct++)
                        acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[rt][m], bf[ct][m], acc[rt][ct], 0, 0, 0);
            }
        }
        if (more) stage(buf ^ 1);
        __syncthreads();
        j = jn;
        q = qn;
    }

    const float* const rb = p.res ? p.res + (long)b * p.ldr + (long)grp * p.cg_out : nullptr;
    const long rstride = (long)p.B * p.ldr;
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) {
        const int col = 16 * ct + c;
        if (col >= p.cg_out) continue;
        const float bv = p.bias ? p.bias[grp * p.cg_out + col] : 0.f;
#pragma unroll
        for (int rt = 0; rt < 2; rt++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int tq = t0 + 32 * w + 16 * rt + 4 * g4 + i;
                if (tq >= tend) continue;
                float v = acc[rt][ct][i] + bv;
                if (p.act == ASR_GCONV_ACT_GELU) v = gelu_f32(v);
                if (tq < nout) {
                    if (rb) v = rb[(long)tq * rstride + col] + v;
                } else {
                    v = 0.f;
                }
                ob[(long)tq * ostride + col] = v;
            }
    }
}

static int gconv_desc_arg(const asr_grouped_conv1d_desc* d) {
    if (!d) return ASR_ERR_ARG;
    if (d->c_in <= 0 || d->c_out <= 0 || d->kernel <= 0 || d->groups <= 0) return ASR_ERR_ARG;
    if (d->pad_left < 0 || d->pad_right < 0) return ASR_ERR_ARG;
    if (d->c_in % d->groups != 0 || d->c_out % d->groups != 0) return ASR_ERR_ARG;
    if (d->act != ASR_GCONV_ACT_NONE && d->act != ASR_GCONV_ACT_GELU) return ASR_ERR_ARG;
    return ASR_OK;
}
static int gconv_desc_unsupported(const asr_grouped_conv1d_desc* d) {
    if (d->groups == 1 || d->groups >= d->c_in) return ASR_ERR_UNSUPPORTED;      // asr_conv1d_fwd's cases
    if (d->c_in / d->groups > 128 || d->c_out / d->groups > 128) return ASR_ERR_UNSUPPORTED;
    if (d->kernel > 128 || d->groups > 65535) return ASR_ERR_UNSUPPORTED;
    return ASR_OK;
}

template <int NCT>
static int gconv_launch(const GConvArgs& p, dim3 grid, size_t lds, hipStream_t st) {
    static AsrAttrOnce once;
    if (int rc = once.set(reinterpret_cast<const void*>(&grouped_conv1d_kernel<NCT>), 160 * 1024)) return rc;
    hipLaunchKernelGGL(grouped_conv1d_kernel<NCT>, grid, dim3(256), lds, st, p);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

}  // namespace asr

extern "C" {

int asr_grouped_conv1d_out_frames(const asr_grouped_conv1d_desc* d, int n_frames) {
    if (int rc = asr::gconv_desc_arg(d)) return -rc;
    if (int rc = asr::gconv_desc_unsupported(d)) return -rc;
    const long n = asr::gconv_frames(n_frames, d->kernel, d->pad_left, d->pad_right);
    return n > INT_MAX ? -ASR_ERR_UNSUPPORTED : (int)n;
}

int asr_grouped_conv1d_fwd(const asr_grouped_conv1d_desc* d, const float* d_x, long ldx, const int32_t* d_lengths,
                           const float* d_W, const float* d_b, const float* d_res, long ldr, float* d_out, long ldo,
                           int32_t* d_out_lengths, int T, int B, asr_stream_t s) {
    if (!d || !d_x || !d_W || !d_out) return ASR_ERR_ARG;
    if (int rc = asr::gconv_desc_arg(d)) return rc;
    if (T <= 0 || B <= 0 || ldx < d->c_in || ldo < d->c_out || (d_res && ldr < d->c_out)) return ASR_ERR_ARG;
    if (d_out == d_x) return ASR_ERR_ARG;
    const long T_out = asr::gconv_frames(T, d->kernel, d->pad_left, d->pad_right);
    if (T_out == 0) return ASR_ERR_ARG;
    if (int rc = asr::gconv_desc_unsupported(d)) return rc;
    if ((long)T + d->pad_left + d->pad_right > (long)INT_MAX - 4096) return ASR_ERR_UNSUPPORTED;
    if ((long)T * B > INT_MAX || T_out * B > INT_MAX || B > 65535) return ASR_ERR_UNSUPPORTED;

    asr::GConvArgs p{};
    p.x = d_x; p.ldx = ldx; p.lengths = d_lengths; p.W = d_W; p.bias = d_b; p.res = d_res; p.ldr = ldr;
    p.out = d_out; p.ldo = ldo; p.out_lengths = d_out_lengths;
    p.T = T; p.B = B; p.T_out = (int)T_out;
    p.cg_in = d->c_in / d->groups; p.cg_out = d->c_out / d->groups; p.c_out = d->c_out;
    p.k = d->kernel; p.pl = d->pad_left; p.pr = d->pad_right; p.act = d->act;
    p.cin16 = (p.cg_in + 15) / 16 * 16; p.lda = p.cin16 + 4; p.rows = asr::GC_TT + d->kernel - 1;
    const int nct = (p.cg_out + 15) / 16;
    const size_t lds = ((size_t)p.rows * p.lda + 2 * (size_t)asr::GC_KC * 16 * nct) * sizeof(float);
    const dim3 grid((unsigned)((T_out + asr::GC_TT - 1) / asr::GC_TT), (unsigned)d->groups, (unsigned)B);
    hipStream_t st = asr_stream(s);
    switch (nct) {
        case 1: return asr::gconv_launch<1>(p, grid, lds, st);
        case 2: return asr::gconv_launch<2>(p, grid, lds, st);
        case 3: return asr::gconv_launch<3>(p, grid, lds, st);
        case 4: return asr::gconv_launch<4>(p, grid, lds, st);
        case 5: return asr::gconv_launch<5>(p, grid, lds, st);
        case 6: return asr::gconv_launch<6>(p, grid, lds, st);
        case 7: return asr::gconv_launch<7>(p, grid, lds, st);
        default: return asr::gconv_launch<8>(p, grid, lds, st);
    }
}

}  // extern "C"
