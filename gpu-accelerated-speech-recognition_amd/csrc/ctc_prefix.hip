// The CTC prefix scorer of joint CTC / attention decoding: asr_ctc_prefix_begin,
// asr_ctc_prefix_score and asr_ctc_prefix_advance (the formulas are in
// include/asr_amd.h).
//
// Score.  d(g, c) = psi(g.c) - psi(g) is, per utterance, a log-domain matrix
// product of the K hypotheses' phi [K][T_b] against the emission columns
// [T_b][V], without a recurrence.  The emissions are the traffic (T*B*V floats
// per decoding step) and the K hypotheses of an utterance read the same ones, so
//   - grid (ceil(V / 256), B): a workgroup serves ONE utterance and 256 tokens;
//   - a lane owns one token c and keeps one (m, s) accumulator pair per live
//     hypothesis of the utterance (K <= 16, 32 registers): the running maximum
//     and the sum of exp2(term - m), both in the base-2 domain;
//   - it reads x[t, b, c] once (a wave reads 256 contiguous bytes of a frame's
//     row), eight frames at a time and one chunk ahead of the arithmetic, and
//     uses each value for every hypothesis;
//   - phi, shifted by psi(g) in fp64 and scaled by log2(e) before it is rounded
//     to fp32, is staged in LDS 64 frames at a time in both forms side by side
//     (rn + rb | rb alone): a lane reads the pair as a broadcast and takes the
//     second when its token is the hypothesis's last.
// Per chunk of eight frames (t = 1 + 8q .. 8 + 8q, whatever the shape) and
// hypothesis: the eight terms, their maximum with m, one rescale of s and eight
// exp2 (nine v_exp_f32 for eight terms).  The term at the maximum contributes
// exactly 1, so a finite result never underflows, and a sum whose terms are all
// -inf stays -inf.  Frames ascend, the chunk edges depend on t alone, and every
// value is moved four bytes at a time, so a (slot, token) result depends only on
// the slot's state and last token, the utterance's emissions and length and the
// descriptor's scalars: never on B, K, N, the slot, other slots, strides or
// alignment.  No MFMA: the terms of one sum span hundreds of nats, which neither
// the matrix units' fixed-point-like accumulation of exp'd values (the
// probability domain underflows) nor a log-domain operand fits.
//
// Advance and begin are N x T cells against the scorer's N x V x T terms: a lane
// per slot walks its frames in fp64 with lse2 (csrc/ctc_lse.h), the state
// [T][N] read and written with the slots of a wave side by side, the inputs of
// frame t + 1 loaded before the three dependent lse2 chains of frame t.
#include "asr_internal.h"
#include "ctc_lse.h"

#include <climits>
#include <cmath>

namespace asr {

constexpr int PS_THREADS = 256;                  // tokens per workgroup, one per lane
constexpr int PS_MAX_K = ASR_ATTN_BEAM_MAX_K;
constexpr int PS_STAGE = 64;                     // frames of phi per LDS stage
constexpr int PS_CHUNK = 8;                      // frames per maximum
constexpr int ADV_THREADS = 64;
constexpr float PS_LOG2E = 1.44269504088896340736f;
constexpr float PS_LN2 = 0.69314718055994530942f;
constexpr double PS_LOG2E_D = 1.44269504088896340736;
static_assert(PS_STAGE % PS_CHUNK == 0 && PS_MAX_K == 16, "the unrolled hypothesis loop below is written for 16");

struct PrefixArgs {
    const float* x;
    long ld;
    const int32_t* enc;
    const double *rn, *rb, *psi;
    const int32_t* last;
    const double* scores;
    const int32_t* fin;
    const float* att;
    long lda;
    float* out;
    long ldo;
    int B, K, V, T, blank, eos;
    double w, bonus;
};

__device__ __forceinline__ float ps_exp2(float x) { return __builtin_amdgcn_exp2f(x); }   // x <= 0; exp2(-inf) = 0

// Four waves per SIMD: left alone the compiler interleaves the sixteen hypothesis bodies over 249 VGPRs (two waves).
__global__ __launch_bounds__(PS_THREADS) __attribute__((amdgpu_waves_per_eu(4))) void ctc_prefix_score_kernel(
    const PrefixArgs p) {
    __shared__ float2 ph[PS_MAX_K][PS_STAGE];    // (rn + rb | rb) - psi, times log2(e); frame tp = s0 + column
    __shared__ double psij[PS_MAX_K];
    __shared__ float eosd[PS_MAX_K];
    __shared__ int slot[PS_MAX_K], lastj[PS_MAX_K], dead[PS_MAX_K];
    __shared__ int counts[2];
    const int tid = threadIdx.x, b = blockIdx.y, K = p.K, V = p.V, B = p.B;
    const int c = blockIdx.x * PS_THREADS + tid;
    const bool own = c < V;
    const long N = (long)B * K, n0 = (long)b * K;
    const int Tb = min(max(p.enc[b], 0), p.T);
    const float NEG = -INFINITY;
    if (Tb == 0) return;                         // an utterance without frames: nothing is read or written

    // the live slots, compacted in slot order; a live slot that cannot be emitted (psi -inf) gets a row of -inf
    if (tid == 0) {
        int nl = 0, nd = 0;
        for (int k = 0; k < K; k++) {
            const long n = n0 + k;
            if (!(p.scores[n] > -(double)INFINITY) || p.fin[n] != 0) continue;
            const double ps = p.psi[n];
            if (!(ps > -(double)INFINITY)) {
                dead[nd++] = k;
            } else {
                slot[nl] = k; lastj[nl] = p.last[n]; psij[nl] = ps;
                nl++;
            }
        }
        counts[0] = nl; counts[1] = nd;
    }
    __syncthreads();
    const int nl = __builtin_amdgcn_readfirstlane(counts[0]), nd = __builtin_amdgcn_readfirstlane(counts[1]);
    if (own)
        for (int i = 0; i < nd; i++) p.out[(n0 + dead[i]) * p.ldo + c] = NEG;
    if (nl == 0) return;
    // psi(g.eos) - psi(g) = (rn + rb)[T_b - 1] - psi, by the workgroup that owns eos
    if (p.eos / PS_THREADS == (int)blockIdx.x && tid < nl) {
        const long at = (long)(Tb - 1) * N + n0 + slot[tid];
        eosd[tid] = (float)(lse2(p.rn[at], p.rb[at]) - psij[tid]);
    }

    const float* xb = p.x + (long)b * p.ld + (own ? c : 0);
    const long xstep = (long)B * p.ld;
    float m[PS_MAX_K], s[PS_MAX_K];
    unsigned same = 0;                           // bit j: this lane's token is hypothesis j's last
    {
        const float x0 = own ? xb[0] * PS_LOG2E : NEG;
#pragma unroll
        for (int j = 0; j < PS_MAX_K; j++) {
            m[j] = NEG; s[j] = 0.f;
            if (j < nl) {
                const int lj = lastj[j];
                if (lj == c) same |= 1u << j;
                if (lj < 0) { m[j] = x0; s[j] = x0 > NEG ? 1.f : 0.f; }       // the empty prefix: x[0, b, c]
            }
        }
    }

    // terms t = 1 .. T_b - 1 in chunks of eight; xs holds the chunk's emissions, xn the next chunk's
    const int nchunk = (Tb - 1 + PS_CHUNK - 1) / PS_CHUNK;
    float xs[PS_CHUNK], xn[PS_CHUNK];
#pragma unroll
    for (int i = 0; i < PS_CHUNK; i++) xs[i] = (own && 1 + i < Tb) ? xb[(long)(1 + i) * xstep] * PS_LOG2E : NEG;
    for (int ch = 0; ch < nchunk; ch++) {
        const int q = ch % (PS_STAGE / PS_CHUNK);
        if (q == 0) {
            const int s0 = ch * PS_CHUNK;        // phi of frames tp = s0 .. s0 + 63, tp <= T_b - 2
            __syncthreads();                     // the stage before this one has been read
            for (int e = tid; e < nl * PS_STAGE; e += PS_THREADS) {
                const int tl = e / nl, j = e - tl * nl, tp = s0 + tl;
                float2 f = float2{NEG, NEG};
                if (tp < Tb - 1) {
                    const long at = (long)tp * N + n0 + slot[j];
                    const double vb = p.rb[at], ps = psij[j];
                    f.x = (float)((lse2(p.rn[at], vb) - ps) * PS_LOG2E_D);
                    f.y = (float)((vb - ps) * PS_LOG2E_D);
                }
                ph[j][tl] = f;
            }
            __syncthreads();
        }
        const int t1 = 1 + (ch + 1) * PS_CHUNK;
#pragma unroll
        for (int i = 0; i < PS_CHUNK; i++) xn[i] = (own && t1 + i < Tb) ? xb[(long)(t1 + i) * xstep] * PS_LOG2E : NEG;
#pragma unroll
        for (int j = 0; j < PS_MAX_K; j++) {
            if (j < nl) {                        // uniform: nl is a scalar
                const bool sm = (same >> j) & 1u;
                float v[PS_CHUNK], mx = m[j];
#pragma unroll
                for (int i = 0; i < PS_CHUNK; i++) {
                    const float2 f = ph[j][q * PS_CHUNK + i];
                    v[i] = (sm ? f.y : f.x) + xs[i];
                    mx = fmaxf(mx, v[i]);
                }
                const float ms = mx == NEG ? 0.f : mx;              // nothing finite yet: every exp2 below is 0
                float acc = s[j] * ps_exp2(m[j] - ms);
#pragma unroll
                for (int i = 0; i < PS_CHUNK; i++) acc += ps_exp2(v[i] - ms);
                s[j] = acc; m[j] = mx;
            }
        }
#pragma unroll
        for (int i = 0; i < PS_CHUNK; i++) xs[i] = xn[i];
    }
    __syncthreads();                             // eosd
    if (!own) return;
#pragma unroll
    for (int j = 0; j < PS_MAX_K; j++) {
        if (j < nl) {
            float d = s[j] > 0.f ? (m[j] + __log2f(s[j])) * PS_LN2 : NEG;
            if (c == p.eos) d = eosd[j];
            if (c == p.blank) d = NEG;
            const long n = n0 + slot[j];
            if (p.att && d > NEG) {              // a candidate CTC cannot emit stays -inf at every weight
                const double a = p.w < 1.0 ? (1.0 - p.w) * (double)p.att[n * p.lda + c] : 0.0;
                d = (float)(a + p.w * (double)d + p.bonus);
            }
            p.out[n * p.ldo + c] = d;
        }
    }
}

struct StateArgs {
    const float* x;
    long ld;
    const int32_t *enc, *parent, *token;
    const double *rn_in, *rb_in, *psi_in;
    const int32_t* last_in;
    double *rn, *rb, *psi;
    int32_t* last;
    int B, K, V, T, blank, eos;
};

__global__ __launch_bounds__(ADV_THREADS) void ctc_prefix_begin_kernel(const StateArgs p) {
    const long N = (long)p.B * p.K, n = (long)blockIdx.x * ADV_THREADS + threadIdx.x;
    if (n >= N) return;
    const int b = (int)(n / p.K), Tb = min(max(p.enc[b], 0), p.T);
    const float* xb = p.x + (long)b * p.ld + p.blank;
    const long xstep = (long)p.B * p.ld;
    double cum = 0.0;
    for (int t = 0; t < Tb; t++) {
        cum = cum + (double)xb[(long)t * xstep];
        p.rn[(long)t * N + n] = -(double)INFINITY;
        p.rb[(long)t * N + n] = cum;
    }
    p.psi[n] = 0.0;
    p.last[n] = -1;
}

__global__ __launch_bounds__(ADV_THREADS) void ctc_prefix_advance_kernel(const StateArgs p) {
    const long N = (long)p.B * p.K, n = (long)blockIdx.x * ADV_THREADS + threadIdx.x;
    if (n >= N) return;
    const int b = (int)(n / p.K), Tb = min(max(p.enc[b], 0), p.T);
    const long lo = (long)b * p.K;
    const long par = min(max((long)p.parent[n], lo), lo + p.K - 1);  // a slot of the same utterance, whatever the table holds
    const int c = p.token[n], lastp = p.last_in[par];
    const double NEG = -(double)INFINITY;
    if (c == p.eos || c < 0 || c >= p.V) {       // an ended (or empty) hypothesis: the parent's state as it is
        for (int t = 0; t < Tb; t++) {
            p.rn[(long)t * N + n] = p.rn_in[(long)t * N + par];
            p.rb[(long)t * N + n] = p.rb_in[(long)t * N + par];
        }
        p.psi[n] = p.psi_in[par];
        p.last[n] = lastp;
        return;
    }
    p.last[n] = c;
    if (Tb == 0) {
        p.psi[n] = NEG;
        return;
    }
    const float* xc = p.x + (long)b * p.ld + c;
    const float* xk = p.x + (long)b * p.ld + p.blank;
    const long xstep = (long)p.B * p.ld;
    const bool same = c == lastp;
    double rn = lastp < 0 ? (double)xc[0] : NEG, rb = NEG, psi = rn;
    p.rn[n] = rn;
    p.rb[n] = rb;
    double pa = p.rn_in[par], pb = p.rb_in[par];                     // the parent's frame t - 1
    double xct = Tb > 1 ? (double)xc[xstep] : 0.0, xbt = Tb > 1 ? (double)xk[xstep] : 0.0;
    for (int t = 1; t < Tb; t++) {
        const double ca = pa, cb = pb, cx = xct, cy = xbt;
        pa = p.rn_in[(long)t * N + par];
        pb = p.rb_in[(long)t * N + par];
        if (t + 1 < Tb) {
            xct = (double)xc[(long)(t + 1) * xstep];
            xbt = (double)xk[(long)(t + 1) * xstep];
        }
        const double phi = same ? cb : lse2(ca, cb);
        const double nrn = lse2(rn, phi) + cx;
        const double nrb = lse2(rn, rb) + cy;
        psi = lse2(psi, phi + cx);
        rn = nrn;
        rb = nrb;
        p.rn[(long)t * N + n] = rn;
        p.rb[(long)t * N + n] = rb;
    }
    p.psi[n] = psi;
}

// The descriptor's checks, shared by the three entry points (after their NULL checks).
static int prefix_desc_check(const asr_ctc_prefix_desc* d, long ld) {
    if (d->B <= 0 || d->K < 1 || d->K > ASR_ATTN_BEAM_MAX_K || d->V <= 0 || d->T <= 0) return ASR_ERR_ARG;
    if (d->blank < 0 || d->blank >= d->V || d->eos < 0 || d->eos >= d->V || d->blank == d->eos) return ASR_ERR_ARG;
    if (!(d->ctc_weight >= 0.0 && d->ctc_weight <= 1.0) || !std::isfinite(d->length_bonus)) return ASR_ERR_ARG;
    if (ld < d->V) return ASR_ERR_ARG;
    return ASR_OK;
}

static int prefix_size_check(const asr_ctc_prefix_desc* d) {
    if (d->B > 65535 || (long)d->B * d->K * d->T > INT_MAX) return ASR_ERR_UNSUPPORTED;
    return ASR_OK;
}

static StateArgs state_args(const asr_ctc_prefix_desc* d, const float* x, long ld, const int32_t* enc) {
    StateArgs p{};
    p.x = x; p.ld = ld; p.enc = enc;
    p.B = d->B; p.K = d->K; p.V = d->V; p.T = d->T; p.blank = d->blank; p.eos = d->eos;
    return p;
}

}  // namespace asr

extern "C" {

int asr_ctc_prefix_begin(const asr_ctc_prefix_desc* d, const float* d_emis, long ld, const int32_t* d_enc_lengths,
                         double* d_rn, double* d_rb, double* d_psi, int32_t* d_last, asr_stream_t s) {
    if (!d || !d_emis || !d_enc_lengths || !d_rn || !d_rb || !d_psi || !d_last) return ASR_ERR_ARG;
    int rc = asr::prefix_desc_check(d, ld);
    if (rc != ASR_OK) return rc;
    if (d_rn == d_rb) return ASR_ERR_ARG;
    if ((rc = asr::prefix_size_check(d)) != ASR_OK) return rc;
    asr::StateArgs p = asr::state_args(d, d_emis, ld, d_enc_lengths);
    p.rn = d_rn; p.rb = d_rb; p.psi = d_psi; p.last = d_last;
    const unsigned grid = (unsigned)(((long)d->B * d->K + asr::ADV_THREADS - 1) / asr::ADV_THREADS);
    hipLaunchKernelGGL(asr::ctc_prefix_begin_kernel, dim3(grid), dim3(asr::ADV_THREADS), 0, asr_stream(s), p);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

int asr_ctc_prefix_score(const asr_ctc_prefix_desc* d, const float* d_emis, long ld, const int32_t* d_enc_lengths,
                         const double* d_rn, const double* d_rb, const double* d_psi, const int32_t* d_last,
                         const double* d_scores, const int32_t* d_finished, const float* d_att, long ld_att,
                         float* d_out, long ldo, asr_stream_t s) {
    if (!d || !d_emis || !d_enc_lengths || !d_rn || !d_rb || !d_psi || !d_last || !d_scores || !d_finished || !d_out)
        return ASR_ERR_ARG;
    int rc = asr::prefix_desc_check(d, ld);
    if (rc != ASR_OK) return rc;
    if (ldo < d->V || (d_att && ld_att < d->V)) return ASR_ERR_ARG;
    if ((rc = asr::prefix_size_check(d)) != ASR_OK) return rc;
    asr::PrefixArgs p{};
    p.x = d_emis; p.ld = ld; p.enc = d_enc_lengths;
    p.rn = d_rn; p.rb = d_rb; p.psi = d_psi; p.last = d_last; p.scores = d_scores; p.fin = d_finished;
    p.att = d_att; p.lda = ld_att; p.out = d_out; p.ldo = ldo;
    p.B = d->B; p.K = d->K; p.V = d->V; p.T = d->T; p.blank = d->blank; p.eos = d->eos;
    p.w = d->ctc_weight; p.bonus = d->length_bonus;
    const unsigned gx = (unsigned)((d->V + asr::PS_THREADS - 1) / asr::PS_THREADS);
    hipLaunchKernelGGL(asr::ctc_prefix_score_kernel, dim3(gx, (unsigned)d->B), dim3(asr::PS_THREADS), 0,
                       asr_stream(s), p);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

int asr_ctc_prefix_advance(const asr_ctc_prefix_desc* d, const float* d_emis, long ld, const int32_t* d_enc_lengths,
                           const int32_t* d_parent, const int32_t* d_token, const double* d_rn_in,
                           const double* d_rb_in, const double* d_psi_in, const int32_t* d_last_in, double* d_rn_out,
                           double* d_rb_out, double* d_psi_out, int32_t* d_last_out, asr_stream_t s) {
    if (!d || !d_emis || !d_enc_lengths || !d_parent || !d_token || !d_rn_in || !d_rb_in || !d_psi_in || !d_last_in ||
        !d_rn_out || !d_rb_out || !d_psi_out || !d_last_out)
        return ASR_ERR_ARG;
    int rc = asr::prefix_desc_check(d, ld);
    if (rc != ASR_OK) return rc;
    if (d_rn_out == d_rn_in || d_rn_out == d_rb_in || d_rb_out == d_rn_in || d_rb_out == d_rb_in ||
        d_rn_out == d_rb_out || d_psi_out == d_psi_in || d_last_out == d_last_in)
        return ASR_ERR_ARG;                      // a gather through parent: never in place
    if ((rc = asr::prefix_size_check(d)) != ASR_OK) return rc;
    asr::StateArgs p = asr::state_args(d, d_emis, ld, d_enc_lengths);
    p.parent = d_parent; p.token = d_token;
    p.rn_in = d_rn_in; p.rb_in = d_rb_in; p.psi_in = d_psi_in; p.last_in = d_last_in;
    p.rn = d_rn_out; p.rb = d_rb_out; p.psi = d_psi_out; p.last = d_last_out;
    const unsigned grid = (unsigned)(((long)d->B * d->K + asr::ADV_THREADS - 1) / asr::ADV_THREADS);
    hipLaunchKernelGGL(asr::ctc_prefix_advance_kernel, dim3(grid), dim3(asr::ADV_THREADS), 0, asr_stream(s), p);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

}  // extern "C"
