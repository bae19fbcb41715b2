// Grouped cross-attention for attention-decoder rescoring and the token-score
// gather that ends it: asr_cross_attention_fwd / asr_token_score.
//
// Cross-attention.  N hypotheses attend to the memories of B utterances, each
// hypothesis to its own utterance's only: hypotheses off[b] .. off[b+1] - 1
// belong to utterance b.  Row u*N + n of q / out is token u of hypothesis n,
// row j*B + b of k / v frame j of utterance b; heads*head_dim floats, head h at
// columns [h*D, (h+1)*D).
//   out(u, n, h, :) = sum_j softmax_j(scale * q(u,n,h).k(j,b,h)) v(j,b,h)   over j < klen[b],
// exactly 0 for u >= qlen[n] and for klen[b] = 0.  No window: every live query
// sees every key of its utterance.
//
// Grid (ceil(U * max_hyps / 64), heads, B).  The queries of utterance b are
// numbered TOKEN-MAJOR: flat query f = u * cnt_b + j is token u of the
// utterance's j-th hypothesis (n = first_b + j), so consecutive f are
// consecutive rows of q and out.  Workgroup x of utterance b owns f in
// [64 x, 64 x + 64), a wave 16 of them, a lane one (its MFMA column), as in
// attention_kernel; a workgroup with 64 x >= U * cnt_b exits before the first
// barrier.  So the hypotheses of one utterance share query tiles and with them
// every K / V block the tile stages.  A lane past qlen[n] stays in its tile as
// a dead lane (its row is written as zeros); a wave none of whose lanes is
// live skips the MFMAs of every block.  Dead lanes are not compacted away.
//
// The map is clamped where it is read: cnt_b = off[b+1] - off[b] into
// [0, max_hyps], first_b = off[b] into [0, N - cnt_b]; qlen into [0, U], klen
// into [0, T].  A wrong map therefore gives wrong numbers (two utterances may
// even write the same row) and never an access outside the buffers.  Rows of
// hypotheses that no utterance's clamped range covers are NOT written.
//
// The arithmetic is attention_kernel's (attention.hip), repeated here: 64-key
// blocks from frame 0 ascending, both products on v_mfma_f32_16x16x4_f32 in the
// same (sub, mm) order, the same block-maximum and block-sum trees, the same
// attn_exp, the same epilogue, the same K / V staging global -> registers ->
// LDS with two barriers per block, one instantiation per ceil(head_dim / 16).
// So a row's bits depend only on its query, its utterance's keys and values and
// the descriptor: never on which hypotheses share its tile, on N, B, U, T,
// max_hyps, strides or alignment, and they are asr_attention_fwd's bits for that
// hypothesis alone (B = 1, Tq = qlen, Tk = klen, no window).
//
// Token score.  score[n] = sum over u < len[n], ascending, of
// logp[u*N + n][tok[u*N + n]] in fp64; one thread per hypothesis.  A token
// outside [0, V) adds -inf and reads nothing.
#include "asr_internal.h"

#include <climits>
#include <cmath>
#include <cstddef>

namespace asr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct XAttnArgs {
    const float *q, *k, *v;
    float* out;
    long ldq, ldk, ldv, ldo;
    const int32_t *qlen, *klen, *off;
    int U, N, T, B, max_hyps;
    int D;                         // head_dim
    float scale;
    int vq, vk, vv, vo;            // rows may be moved 16 bytes at a time
};

constexpr int XA_QT = 64;                        // flat queries per workgroup
constexpr int XA_KB = ASR_ATTN_KEY_BLOCK;        // keys per block
static_assert(XA_KB == 64, "the kernel's tiling is written for 64-key blocks");

__device__ __forceinline__ f32x4 xattn_load4(const float* src, bool vec) {
    if (vec) return *reinterpret_cast<const f32x4*>(src);
    return f32x4{src[0], src[1], src[2], src[3]};
}

// attention.hip's attn_exp: exp(x) for x <= 0 on v_exp_f32; exp(-inf) = 0.
__device__ __forceinline__ float xattn_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }

// NDT = ceil(D / 16): 16-column tiles of a head.  Two waves per SIMD at least, as attention_kernel: at most 256
// registers keeps the MFMA accumulators in VGPRs.
template <int NDT>
__global__ __launch_bounds__(256, 2) void cross_attention_kernel(const XAttnArgs p) {
    constexpr int LD = 16 * NDT + 4;             // LDS row stride, as attention_kernel
    __shared__ __attribute__((aligned(16))) float Ks[XA_KB * LD];
    __shared__ __attribute__((aligned(16))) float Vs[XA_KB * LD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int b = blockIdx.z, h = blockIdx.y, f0 = blockIdx.x * XA_QT;
    const int D = p.D;
    const float NEG = -INFINITY;

    // The utterance's hypotheses, clamped: cnt in [0, max_hyps] (<= N), first in [0, N - cnt].
    const long o0 = p.off[b], o1 = p.off[b + 1];
    const int cnt = (int)min(max(o1 - o0, 0L), (long)p.max_hyps);
    const int first = (int)min(max(o0, 0L), (long)(p.N - cnt));
    const int nq = p.U * cnt;                                // U * max_hyps <= INT_MAX - 64
    if (f0 >= nq) return;                                    // before the first barrier; uniform in the workgroup

    const int kend = p.klen ? min(max(p.klen[b], 0), p.T) : p.T;       // keys [0, kend) exist
    const int nb0 = 0, nb1 = kend > 0 ? (kend - 1) / XA_KB : -1;

    // This lane's query: token u of hypothesis n.
    const int f = f0 + 16 * w + c;
    const bool inside = f < nq;
    const int u = inside ? f / cnt : 0;
    const int n = first + (inside ? f - u * cnt : 0);        // < N
    const int qlen = p.qlen ? min(max(p.qlen[n], 0), p.U) : p.U;
    const bool live = inside && u < qlen;
    const int rlo = 0, rhi = live ? kend : 0;
    f32x4 qf[NDT];                                           // qf[sub][mm] = Q[query c][16 sub + 4 g + mm]
    {
        const float* qr = p.q + ((long)(live ? u : 0) * p.N + n) * p.ldq + (long)h * D;
#pragma unroll
        for (int sub = 0; sub < NDT; sub++) {
            const int d0 = 16 * sub + 4 * g;
            qf[sub] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (live && d0 < D) qf[sub] = xattn_load4(qr + d0, p.vq);
        }
    }

    // Thread tid fetches 4-float pieces e = tid + 256 u of a block: key e / (4 NDT), dims 4 (e % (4 NDT)) ...
    f32x4 kr[NDT], vr[NDT];
    auto fetch = [&](int nblk) {
#pragma unroll
        for (int t = 0; t < NDT; t++) {
            const int e = tid + 256 * t;
            const int key = e / (4 * NDT), d0 = 4 * (e % (4 * NDT));
            const int r = nblk * XA_KB + key;
            kr[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            vr[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (r < kend && d0 < D) {
                const long row = (long)r * p.B + b;
                kr[t] = xattn_load4(p.k + row * p.ldk + (long)h * D + d0, p.vk);
                vr[t] = xattn_load4(p.v + row * p.ldv + (long)h * D + d0, p.vv);
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int t = 0; t < NDT; t++) {
            const int e = tid + 256 * t;
            const int key = e / (4 * NDT), d0 = 4 * (e % (4 * NDT));
            *reinterpret_cast<f32x4*>(&Ks[key * LD + d0]) = kr[t];
            *reinterpret_cast<f32x4*>(&Vs[key * LD + d0]) = vr[t];
        }
    };

    f32x4 o[NDT];                                            // o[dt][i] = O[query c][16 dt + 4 g + i]
#pragma unroll
    for (int dt = 0; dt < NDT; dt++) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = NEG, l = 0.f;

    if (nb0 <= nb1) fetch(nb0);
    for (int nblk = nb0; nblk <= nb1; nblk++) {
        __syncthreads();                                     // the block before this one has been read
        stage();
        __syncthreads();
        if (nblk < nb1) fetch(nblk + 1);
        const int r0 = nblk * XA_KB;
        const bool any = rlo < rhi && rlo < r0 + XA_KB && rhi > r0;
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
        const float alpha = (m == mn) ? 1.f : xattn_exp(m - mn);    // O and l are 0 while m is -inf
        float ps[4];
#pragma unroll
        for (int kt = 0; kt < 4; kt++) {
#pragma unroll
            for (int i = 0; i < 4; i++) s[kt][i] = (s[kt][i] == NEG) ? 0.f : xattn_exp(s[kt][i] - mn);
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

    if (!inside) return;
    const bool nz = live && l > 0.f;
    float* orow = p.out + ((long)u * p.N + n) * p.ldo + (long)h * D;
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

// One thread per hypothesis; the tokens of a hypothesis in ascending order.
__global__ __launch_bounds__(64) void token_score_kernel(const float* logp, long ld, const int32_t* tokens,
                                                         const int32_t* lengths, double* scores, int U, int N,
                                                         int V) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const int len = lengths ? min(max(lengths[n], 0), U) : U;
    double sum = 0.0;
    for (int u = 0; u < len; u++) {
        const long row = (long)u * N + n;
        const int tok = tokens[row];
        sum += (tok >= 0 && tok < V) ? (double)logp[row * ld + tok] : -(double)INFINITY;
    }
    scores[n] = sum;
}

static bool xattn_aligned16(const void* ptr, long ld) { return ((uintptr_t)ptr & 15) == 0 && ld % 4 == 0; }

}  // namespace asr

extern "C" {

int asr_cross_attention_fwd(const asr_xattn_desc* d, const float* d_q, long ldq, const float* d_k, long ldk,
                            const float* d_v, long ldv, const int32_t* d_q_lengths, const int32_t* d_k_lengths,
                            const int32_t* d_hyp_offsets, int max_hyps, float* d_out, long ldo, int U, int N, int T,
                            int B, asr_stream_t s) {
    if (!d || !d_q || !d_k || !d_v || !d_out || !d_hyp_offsets) return ASR_ERR_ARG;
    if (U <= 0 || N <= 0 || T <= 0 || B <= 0 || d->heads <= 0 || d->head_dim <= 0) return ASR_ERR_ARG;
    if (max_hyps < 1 || max_hyps > N) return ASR_ERR_ARG;
    const long E = (long)d->heads * d->head_dim;
    if (ldq < E || ldk < E || ldv < E || ldo < E) return ASR_ERR_ARG;
    if (!std::isfinite(d->scale) || d->scale < 0.f) return ASR_ERR_ARG;
    if (d->head_dim % 4 != 0 || d->head_dim > 128 || E > 4096) return ASR_ERR_UNSUPPORTED;
    if (d->heads > 65535 || B > 65535) return ASR_ERR_UNSUPPORTED;                  // grid dimensions
    if ((long)U * N > INT_MAX || (long)T * B > INT_MAX) return ASR_ERR_UNSUPPORTED;
    // a tile's last flat query, 64 x + 63, stays inside an int
    if ((long)U * max_hyps > (long)INT_MAX - 64) return ASR_ERR_UNSUPPORTED;

    asr::XAttnArgs p{};
    p.q = d_q; p.k = d_k; p.v = d_v; p.out = d_out;
    p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo;
    p.qlen = d_q_lengths; p.klen = d_k_lengths; p.off = d_hyp_offsets;
    p.U = U; p.N = N; p.T = T; p.B = B; p.max_hyps = max_hyps;
    p.D = d->head_dim;
    p.scale = d->scale == 0.f ? 1.f / std::sqrt((float)d->head_dim) : d->scale;
    p.vq = asr::xattn_aligned16(d_q, ldq); p.vk = asr::xattn_aligned16(d_k, ldk);
    p.vv = asr::xattn_aligned16(d_v, ldv); p.vo = asr::xattn_aligned16(d_out, ldo);

    const dim3 grid((unsigned)(((long)U * max_hyps + asr::XA_QT - 1) / asr::XA_QT), (unsigned)d->heads, (unsigned)B);
    hipStream_t st = asr_stream(s);
    switch ((d->head_dim + 15) / 16) {
        case 1: hipLaunchKernelGGL(asr::cross_attention_kernel<1>, grid, dim3(256), 0, st, p); break;
        case 2: hipLaunchKernelGGL(asr::cross_attention_kernel<2>, grid, dim3(256), 0, st, p); break;
        case 3: hipLaunchKernelGGL(asr::cross_attention_kernel<3>, grid, dim3(256), 0, st, p); break;
        case 4: hipLaunchKernelGGL(asr::cross_attention_kernel<4>, grid, dim3(256), 0, st, p); break;
        case 5: hipLaunchKernelGGL(asr::cross_attention_kernel<5>, grid, dim3(256), 0, st, p); break;
        case 6: hipLaunchKernelGGL(asr::cross_attention_kernel<6>, grid, dim3(256), 0, st, p); break;
        case 7: hipLaunchKernelGGL(asr::cross_attention_kernel<7>, grid, dim3(256), 0, st, p); break;
        default: hipLaunchKernelGGL(asr::cross_attention_kernel<8>, grid, dim3(256), 0, st, p); break;
    }
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

int asr_token_score(const float* d_logp, long ld, const int32_t* d_tokens, const int32_t* d_lengths,
                    double* d_scores, int U, int N, int V, asr_stream_t s) {
    if (!d_logp || !d_tokens || !d_scores) return ASR_ERR_ARG;
    if (U <= 0 || N <= 0 || V <= 0) return ASR_ERR_ARG;
    if (ld < V) return ASR_ERR_ARG;
    if ((long)U * N > INT_MAX) return ASR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(asr::token_score_kernel, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, asr_stream(s), d_logp,
                       ld, d_tokens, d_lengths, d_scores, U, N, V);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

}  // extern "C"
