// The step of an attention-decoder beam search: asr_decode_attention_fwd,
// asr_embed_fwd, asr_attn_beam_step and its host twin asr_attn_beam_step_host.
//
// Decode attention.  Each of N hypotheses has ONE query row; hypothesis n
// attends to keys j < len[n], key j being row j*S + col(j, n) of k / v:
//   out(n, h, :) = sum_j softmax_j(scale * q(n,h).k(j, col(j,n), h)) v(j, col(j,n), h)
// col(j, n) = cols[j*ldc + n], clamped into [0, S - 1] where it is read.
// ldc = 0: one column for every j (cross-attention over the utterance of the
// hypothesis, S = B, Tk = T).  ldc >= N: the ancestry table of a beam search,
// which slot wrote this hypothesis's key at step j; a beam reorder permutes
// the table and never moves K / V.
//
// Grid (N, heads), one wave per (hypothesis, head); a workgroup IS one wave,
// so waves of different lengths never wait for each other and the barriers
// below are wave-local.  Per 64-key block, from key 0 ascending:
//   1. lane i owns key r0 + i: it reads its K row 16 bytes at a time and
//      chains one fmaf per dimension, d ascending, against q (LDS, broadcast);
//   2. s = dot * scale, masked by selection; block maximum and block sum by
//      xor butterflies (every lane ends with the same bits);
//   3. p and the row number go to LDS; lane (g = lane / 32, c = lane % 32)
//      owns dimensions [4c, 4c + 4) and the keys r0 + 32 g + t, t ascending:
//      o = fmaf(p, v, o) with V read 16 bytes at a time, a half wave reading
//      one row side by side.
// The two halves are added once, after the last block (g = 0 + g = 1), then
// divided by l.  Every choice above is a function of head_dim alone, so a
// row's bits depend only on its query, the keys and values it sees in order
// and the descriptor: never on N, S, the slot, other hypotheses, ldc, the
// column numbers, strides or alignment (an unaligned row is read float by
// float into the same registers).  The product order differs from
// attention_kernel's MFMA order: the bits are NOT asr_attention_fwd's.
//
// Rows j >= len[n] and rows the table does not name are never read; a row
// with len 0 is exact zeros.
//
// Embedding.  out[r] = fp32((double)emb[tok[r]] * scale + pe[pos[r]]): one
// rounded fp64 product and one rounded fp64 sum (this file is compiled with
// -ffp-contract=off; the attention kernel spells its fmaf out), one thread per
// element.  A token outside [0, V) or a position outside [0, P) gives a zero
// row and reads nothing.
//
// Beam step.  One workgroup per utterance.  The candidates of utterance b
// are, per slot k: nothing (score -inf), itself with token eos (finished), or
// V tokens (score + (double)logp[v]; a candidate that comes out -inf or NaN
// is dropped).  The total order is score descending, then parent slot
// ascending, then token ascending; K rounds each take the best candidate
// strictly after the one before, so the result is exact and its order fixed.
// The workgroup then gathers the two history tables through parent.  The host
// twin states the same rule with a sort.
#include "asr_internal.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <vector>

namespace asr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int DA_KB = ASR_ATTN_KEY_BLOCK;        // keys per block, one per lane
static_assert(DA_KB == 64, "one key per lane of a 64-lane wave");
constexpr int DA_MAX_D = 128;

struct DecAttnArgs {
    const float *q, *k, *v;
    float* out;
    long ldq, ldk, ldv, ldo, ldc;
    const int32_t *cols, *lengths;
    int N, Tk, S, D;
    float scale;
    int vq, vk, vv, vo;            // rows may be moved 16 bytes at a time
};

__device__ __forceinline__ f32x4 da_load4(const float* src, bool vec) {
    if (vec) return *reinterpret_cast<const f32x4*>(src);
    return f32x4{src[0], src[1], src[2], src[3]};
}

// attention.hip's attn_exp: exp(x) for x <= 0 on v_exp_f32; exp(-inf) = 0.
__device__ __forceinline__ float da_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }

__global__ __launch_bounds__(64) void decode_attention_kernel(const DecAttnArgs p) {
    __shared__ __attribute__((aligned(16))) float qs[DA_MAX_D];
    __shared__ float ps[DA_KB];
    __shared__ int rows[DA_KB];                  // Tk * S <= INT_MAX
    const int lane = threadIdx.x, n = blockIdx.x, h = blockIdx.y;
    const int D = p.D;
    const float NEG = -INFINITY;
    const int len = p.lengths ? min(max(p.lengths[n], 0), p.Tk) : p.Tk;
    const int g = lane >> 5, c = lane & 31;
    const bool owns = 4 * c < D;                 // this lane owns output dimensions [4c, 4c + 4)

    if (owns && g == 0 && len > 0)
        *reinterpret_cast<f32x4*>(&qs[4 * c]) = da_load4(p.q + (long)n * p.ldq + (long)h * D + 4 * c, p.vq);
    __syncthreads();

    f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = NEG, l = 0.f;
    for (int r0 = 0; r0 < len; r0 += DA_KB) {
        const int r = r0 + lane;
        const bool live = r < len;
        long row = 0;
        float s = NEG;
        if (live) {
            const int col = p.cols[(long)r * p.ldc + n];         // ldc = 0: cols[n] for every key
            row = (long)r * p.S + min(max(col, 0), p.S - 1);
            const float* kr = p.k + row * p.ldk + (long)h * D;
            float acc = 0.f;
#pragma unroll 4
            for (int d0 = 0; d0 < D; d0 += 4) {
                const f32x4 kk = da_load4(kr + d0, p.vk);
                const f32x4 qq = *reinterpret_cast<const f32x4*>(&qs[d0]);
                acc = __builtin_fmaf(kk[0], qq[0], acc);
                acc = __builtin_fmaf(kk[1], qq[1], acc);
                acc = __builtin_fmaf(kk[2], qq[2], acc);
                acc = __builtin_fmaf(kk[3], qq[3], acc);
            }
            s = acc * p.scale;
        }
        float bm = s;
#pragma unroll
        for (int x = 1; x < 64; x <<= 1) bm = fmaxf(bm, __shfl_xor(bm, x));
        const float mn = fmaxf(m, bm);           // finite: key r0 is live
        const float alpha = (m == mn) ? 1.f : da_exp(m - mn);       // o and l are 0 while m is -inf
        const float pr = live ? da_exp(s - mn) : 0.f;
        float bs = pr;
#pragma unroll
        for (int x = 1; x < 64; x <<= 1) bs += __shfl_xor(bs, x);
        l = l * alpha + bs;
        m = mn;
        __syncthreads();                         // the block before this one has been read
        ps[lane] = pr;
        rows[lane] = (int)row;
        __syncthreads();
        o *= alpha;
        if (owns) {
            const int nk = min(len - r0 - 32 * g, 32);              // this half's keys in the block
#pragma unroll 4
            for (int t = 0; t < nk; t++) {
                const int i = 32 * g + t;
                const f32x4 vv = da_load4(p.v + (long)rows[i] * p.ldv + (long)h * D + 4 * c, p.vv);
                const float pw = ps[i];
                o[0] = __builtin_fmaf(pw, vv[0], o[0]);
                o[1] = __builtin_fmaf(pw, vv[1], o[1]);
                o[2] = __builtin_fmaf(pw, vv[2], o[2]);
                o[3] = __builtin_fmaf(pw, vv[3], o[3]);
            }
        }
    }
    f32x4 r;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float both = o[i] + __shfl_xor(o[i], 32);             // g = 0 + g = 1, the same bits in both halves
        r[i] = l > 0.f ? both / l : 0.f;
    }
    if (!owns || g != 0) return;
    float* orow = p.out + (long)n * p.ldo + (long)h * D + 4 * c;
    if (p.vo) {
        *reinterpret_cast<f32x4*>(orow) = r;
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) orow[i] = r[i];
    }
}

__global__ __launch_bounds__(256) void embed_kernel(const float* emb, long lde, const double* pe, long ldp,
                                                    const int32_t* tokens, const int32_t* pos, double scale,
                                                    float* out, long ldo, int R, int E, int V, int P) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)R * E) return;
    const int r = (int)(idx / E), e = (int)(idx - (long)r * E);
    const int tok = tokens[r];
    const int ps = pe ? pos[r] : 0;
    float res = 0.f;
    if (tok >= 0 && tok < V && (!pe || (ps >= 0 && ps < P))) {
        double x = (double)emb[(long)tok * lde + e] * scale;
        if (pe) x = x + pe[(long)ps * ldp + e];
        res = (float)x;
    }
    out[(long)r * ldo + e] = res;
}

struct BeamArgs {
    const float* logp;
    long ld;
    const double* scores;
    const int32_t *finished, *tokens_in, *anc_in;
    double* scores_out;
    int32_t *finished_out, *parent, *token, *tokens_out, *anc_out, *all_finished;
    int B, K, V, max_len, step, eos;
};

constexpr int BS_THREADS = 256;
constexpr int BS_MAX_K = ASR_ATTN_BEAM_MAX_K;

// (key, idx) is better than (bk, bi): a larger key, or the same key and a smaller idx.  key 0 = absent.
__device__ __forceinline__ bool bs_better(uint64_t key, uint64_t idx, uint64_t bk, uint64_t bi) {
    return key > bk || (key == bk && key != 0 && idx < bi);
}

__global__ __launch_bounds__(BS_THREADS) void attn_beam_step_kernel(const BeamArgs p) {
    __shared__ double sc[BS_MAX_K];
    __shared__ int fin[BS_MAX_K];
    __shared__ uint64_t wkey[BS_THREADS / 64], widx[BS_THREADS / 64];
    __shared__ uint64_t skey[BS_MAX_K], sidx[BS_MAX_K];
    __shared__ int par[BS_MAX_K];
    const int tid = threadIdx.x, b = blockIdx.x, K = p.K, V = p.V;
    const long N = (long)p.B * K, n0 = (long)b * K;
    if (tid < K) {
        sc[tid] = p.scores[n0 + tid];
        fin[tid] = p.finished[n0 + tid] != 0;
    }
    __syncthreads();

    uint64_t tk = 0, ti = 0;                     // the candidate taken last
    for (int round = 0; round < K; round++) {
        uint64_t bk = 0, bi = 0;
        for (int k = 0; k < K; k++) {
            const double base = sc[k];
            if (!(base > -(double)INFINITY)) continue;              // an empty slot (or NaN): no candidate
            if (fin[k]) {
                if (tid == 0) {
                    const uint64_t key = asr_d2key(base), idx = (uint64_t)k * V + p.eos;
                    const bool after = round == 0 || key < tk || (key == tk && idx > ti);
                    if (after && bs_better(key, idx, bk, bi)) { bk = key; bi = idx; }
                }
                continue;
            }
            const float* lp = p.logp + (n0 + k) * p.ld;
            for (int v = tid; v < V; v += BS_THREADS) {
                const double x = base + (double)lp[v];
                if (!(x > -(double)INFINITY)) continue;             // -inf or NaN: dropped
                const uint64_t key = asr_d2key(x), idx = (uint64_t)k * V + v;
                const bool after = round == 0 || key < tk || (key == tk && idx > ti);
                if (after && bs_better(key, idx, bk, bi)) { bk = key; bi = idx; }
            }
        }
#pragma unroll
        for (int x = 1; x < 64; x <<= 1) {
            const uint64_t ok = __shfl_xor(bk, x), oi = __shfl_xor(bi, x);
            if (bs_better(ok, oi, bk, bi)) { bk = ok; bi = oi; }
        }
        if ((tid & 63) == 0) { wkey[tid >> 6] = bk; widx[tid >> 6] = bi; }
        __syncthreads();
        bk = wkey[0]; bi = widx[0];
#pragma unroll
        for (int w = 1; w < BS_THREADS / 64; w++)
            if (bs_better(wkey[w], widx[w], bk, bi)) { bk = wkey[w]; bi = widx[w]; }
        if (tid == 0) { skey[round] = bk; sidx[round] = bi; }
        tk = bk; ti = bi;
        __syncthreads();                         // wkey / widx are rewritten by the next round
        if (bk == 0) {                           // no candidate is left: uniform in the workgroup
            if (tid == 0)
                for (int r = round + 1; r < K; r++) { skey[r] = 0; sidx[r] = 0; }
            break;
        }
    }
    __syncthreads();

    if (tid < K) {
        const long n = n0 + tid;
        int pk = tid, tok = p.eos, f = 0;
        double s = -(double)INFINITY;
        if (skey[tid] != 0) {
            pk = (int)(sidx[tid] / (uint64_t)V);
            tok = (int)(sidx[tid] - (uint64_t)pk * V);
            if (fin[pk]) {
                s = sc[pk];
                f = 1;
            } else {
                s = sc[pk] + (double)p.logp[(n0 + pk) * p.ld + tok];
                f = tok == p.eos;
            }
        }
        par[tid] = pk;
        p.scores_out[n] = s;
        p.finished_out[n] = f;
        p.parent[n] = (int32_t)(n0 + pk);
        p.token[n] = tok;
        p.tokens_out[(long)p.step * N + n] = tok;
        if (p.step + 1 < p.max_len) p.anc_out[(long)(p.step + 1) * N + n] = (int32_t)n;
    }
    __syncthreads();
    if (tid == 0) {
        int live = 0;
        for (int k = 0; k < K; k++) live += skey[k] != 0 && !(fin[par[k]] || (int)(sidx[k] % (uint64_t)V) == p.eos);
        if (live) atomicAdd(p.all_finished, live);
    }
    // the histories, through parent: tokens rows j < step, ancestry rows j <= step
    for (long e = tid; e < (long)(p.step + 1) * K; e += BS_THREADS) {
        const long j = e / K;
        const int k = (int)(e - j * K);
        const long src = j * N + n0 + par[k], dst = j * N + n0 + k;
        if (j < p.step) p.tokens_out[dst] = p.tokens_in[src];
        p.anc_out[dst] = p.anc_in[src];
    }
}

static bool da_aligned16(const void* ptr, long ld) { return ((uintptr_t)ptr & 15) == 0 && ld % 4 == 0; }

static int beam_step_check(const asr_attn_beam_desc* d, const void* logp, long ld, const void* scores,
                           const void* finished, const void* tokens_in, const void* anc_in, const void* scores_out,
                           const void* finished_out, const void* parent, const void* token, const void* tokens_out,
                           const void* anc_out, const void* all_finished) {
    if (!d || !logp || !scores || !finished || !tokens_in || !anc_in || !scores_out || !finished_out || !parent ||
        !token || !tokens_out || !anc_out || !all_finished)
        return ASR_ERR_ARG;
    if (d->B <= 0 || d->K < 1 || d->K > ASR_ATTN_BEAM_MAX_K || d->V <= 0 || d->max_len <= 0) return ASR_ERR_ARG;
    if (d->step < 0 || d->step >= d->max_len || d->eos < 0 || d->eos >= d->V) return ASR_ERR_ARG;
    if (ld < d->V) return ASR_ERR_ARG;
    if (tokens_out == tokens_in || anc_out == anc_in) return ASR_ERR_ARG;          // a gather: never in place
    if ((long)d->B * d->K > INT_MAX || (long)d->B * d->K * d->max_len > INT_MAX) return ASR_ERR_UNSUPPORTED;
    return ASR_OK;
}

}  // namespace asr

extern "C" {

int asr_decode_attention_fwd(const asr_xattn_desc* d, const float* d_q, long ldq, const float* d_k, long ldk,
                             const float* d_v, long ldv, const int32_t* d_cols, long ldc, const int32_t* d_lengths,
                             float* d_out, long ldo, int N, int Tk, int S, asr_stream_t s) {
    if (!d || !d_q || !d_k || !d_v || !d_out || !d_cols) return ASR_ERR_ARG;
    if (N <= 0 || Tk <= 0 || S <= 0 || d->heads <= 0 || d->head_dim <= 0) return ASR_ERR_ARG;
    if (ldc != 0 && ldc < N) return ASR_ERR_ARG;
    const long E = (long)d->heads * d->head_dim;
    if (ldq < E || ldk < E || ldv < E || ldo < E) return ASR_ERR_ARG;
    if (!std::isfinite(d->scale) || d->scale < 0.f) return ASR_ERR_ARG;
    if (d->head_dim % 4 != 0 || d->head_dim > asr::DA_MAX_D || E > 4096) return ASR_ERR_UNSUPPORTED;
    if (d->heads > 65535) return ASR_ERR_UNSUPPORTED;                                // grid dimension
    if ((long)Tk * S > INT_MAX) return ASR_ERR_UNSUPPORTED;

    asr::DecAttnArgs p{};
    p.q = d_q; p.k = d_k; p.v = d_v; p.out = d_out;
    p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo; p.ldc = ldc;
    p.cols = d_cols; p.lengths = d_lengths;
    p.N = N; p.Tk = Tk; p.S = S; p.D = d->head_dim;
    p.scale = d->scale == 0.f ? 1.f / std::sqrt((float)d->head_dim) : d->scale;
    p.vq = asr::da_aligned16(d_q, ldq) && d->head_dim % 4 == 0;
    p.vk = asr::da_aligned16(d_k, ldk); p.vv = asr::da_aligned16(d_v, ldv); p.vo = asr::da_aligned16(d_out, ldo);
    hipLaunchKernelGGL(asr::decode_attention_kernel, dim3((unsigned)N, (unsigned)d->heads), dim3(64), 0,
                       asr_stream(s), p);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

int asr_embed_fwd(const float* d_emb, long lde, const double* d_pe, long ldp, const int32_t* d_tokens,
                  const int32_t* d_pos, double scale, float* d_out, long ldo, int R, int E, int V, int P,
                  asr_stream_t s) {
    if (!d_emb || !d_tokens || !d_out || (d_pe && !d_pos)) return ASR_ERR_ARG;
    if (R <= 0 || E <= 0 || V <= 0 || (d_pe && P <= 0)) return ASR_ERR_ARG;
    if (lde < E || ldo < E || (d_pe && ldp < E)) return ASR_ERR_ARG;
    if (!std::isfinite(scale)) return ASR_ERR_ARG;
    if ((long)R * E > INT_MAX) return ASR_ERR_UNSUPPORTED;
    const unsigned grid = (unsigned)(((long)R * E + 255) / 256);
    hipLaunchKernelGGL(asr::embed_kernel, dim3(grid), dim3(256), 0, asr_stream(s), d_emb, lde, d_pe, ldp, d_tokens,
                       d_pos, scale, d_out, ldo, R, E, V, P);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

int asr_attn_beam_step(const asr_attn_beam_desc* d, const float* d_logp, long ld, const double* d_scores,
                       const int32_t* d_finished, const int32_t* d_tokens_in, const int32_t* d_anc_in,
                       double* d_scores_out, int32_t* d_finished_out, int32_t* d_parent, int32_t* d_token,
                       int32_t* d_tokens_out, int32_t* d_anc_out, int32_t* d_all_finished, asr_stream_t s) {
    const int rc = asr::beam_step_check(d, d_logp, ld, d_scores, d_finished, d_tokens_in, d_anc_in, d_scores_out,
                                        d_finished_out, d_parent, d_token, d_tokens_out, d_anc_out, d_all_finished);
    if (rc != ASR_OK) return rc;
    asr::BeamArgs p{};
    p.logp = d_logp; p.ld = ld; p.scores = d_scores; p.finished = d_finished;
    p.tokens_in = d_tokens_in; p.anc_in = d_anc_in;
    p.scores_out = d_scores_out; p.finished_out = d_finished_out; p.parent = d_parent; p.token = d_token;
    p.tokens_out = d_tokens_out; p.anc_out = d_anc_out; p.all_finished = d_all_finished;
    p.B = d->B; p.K = d->K; p.V = d->V; p.max_len = d->max_len; p.step = d->step; p.eos = d->eos;
    hipStream_t st = asr_stream(s);
    ASR_HIP_TRY(hipMemsetAsync(d_all_finished, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(asr::attn_beam_step_kernel, dim3((unsigned)d->B), dim3(asr::BS_THREADS), 0, st, p);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

int asr_attn_beam_step_host(const asr_attn_beam_desc* d, const float* logp, long ld, const double* scores,
                            const int32_t* finished, const int32_t* tokens_in, const int32_t* anc_in,
                            double* scores_out, int32_t* finished_out, int32_t* parent, int32_t* token,
                            int32_t* tokens_out, int32_t* anc_out, int32_t* all_finished) {
    const int rc = asr::beam_step_check(d, logp, ld, scores, finished, tokens_in, anc_in, scores_out, finished_out,
                                        parent, token, tokens_out, anc_out, all_finished);
    if (rc != ASR_OK) return rc;
    struct Cand {
        double score;
        int k, v;
    };
    const int B = d->B, K = d->K, V = d->V, step = d->step, eos = d->eos;
    const long N = (long)B * K;
    int live = 0;
    std::vector<Cand> cand;
    for (int b = 0; b < B; b++) {
        const long n0 = (long)b * K;
        cand.clear();
        for (int k = 0; k < K; k++) {
            const double base = scores[n0 + k];
            if (!(base > -(double)INFINITY)) continue;
            if (finished[n0 + k]) {
                cand.push_back(Cand{base, k, eos});
                continue;
            }
            for (int v = 0; v < V; v++) {
                const double x = base + (double)logp[(n0 + k) * ld + v];
                if (x > -(double)INFINITY) cand.push_back(Cand{x, k, v});
            }
        }
        const size_t keep = std::min(cand.size(), (size_t)K);
        std::partial_sort(cand.begin(), cand.begin() + keep, cand.end(), [](const Cand& a, const Cand& c) {
            if (a.score != c.score) return a.score > c.score;
            if (a.k != c.k) return a.k < c.k;
            return a.v < c.v;
        });
        for (int k = 0; k < K; k++) {
            const long n = n0 + k;
            int pk = k, tok = eos, f = 0;
            double s = -(double)INFINITY;
            if ((size_t)k < keep) {
                pk = cand[k].k;
                tok = cand[k].v;
                s = cand[k].score;
                f = finished[n0 + pk] != 0 || tok == eos;
                live += !f;
            }
            scores_out[n] = s;
            finished_out[n] = f;
            parent[n] = (int32_t)(n0 + pk);
            token[n] = tok;
            for (long j = 0; j <= step; j++) {
                if (j < step) tokens_out[j * N + n] = tokens_in[j * N + n0 + pk];
                anc_out[j * N + n] = anc_in[j * N + n0 + pk];
            }
            tokens_out[(long)step * N + n] = tok;
            if (step + 1 < d->max_len) anc_out[(long)(step + 1) * N + n] = (int32_t)n;
        }
    }
    *all_finished = live;
    return ASR_OK;
}

}  // extern "C"
