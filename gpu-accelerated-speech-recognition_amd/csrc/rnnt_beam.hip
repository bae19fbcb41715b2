// RNN-T (transducer) beam search, one symbol per frame (the "modified beam
// search" of k2 / icefall): asr_rnnt_beam_workspace_bytes / asr_rnnt_beam /
// asr_rnnt_beam_host.  The model, the weight layouts and the start are
// rnnt.hip's (h = c = 0, then one predictor step on Emb[blank]).
//
// Search of utterance b, beam width K (the definition; include/asr_amd.h has the
// same text).  A hypothesis is (ys, one timestep per token, a score in double,
// the predictor state after ys); the beam A is ordered by rank and starts as
// the empty hypothesis with score 0.  Each frame t < len_b: every hypothesis i
// gets lp_i = log_softmax(joint(f_t, h_top_i)); candidate (i, v) scores
// s_i + lp_i[v]; the best min(K, |A| V) candidates are kept, ordered by score
// descending, then i, then v ascending (a NaN after every number).  (i, blank)
// is hypothesis i with the new score; (i, v) is ys_i + [v] at timestep t, its
// state hypothesis i's stepped on Emb[v].  Kept candidates with equal token
// sequences merge: score logaddexp, timesteps of the higher score (the earlier
// candidate on equal scores).  AT MOST TWO candidates can share a sequence,
// A + blank and B + v: two blanks are two different hypotheses of A, and
// (i, v), (j, w) with ys_i + [v] = ys_j + [w] have v = w and ys_i = ys_j, so
// i = j.  There is no n-way merge here.  The new A is the merged set by score
// descending, ties by the position of the earlier constituent.
//
// Device form.  f for all T frames is one gemm_launch; the search is ONE launch.
// A workgroup of 8 waves owns the 16 rows of a v_mfma_f32_16x16x4_f32 tile; an
// utterance takes R rows (R the smallest power of two >= K), so a workgroup
// holds 16 / R utterances and row u R + i is rank i of its utterance u.  Rows
// without a live hypothesis are computed and ignored.  Per frame:
//   1. z = act(f_t + g), logits tile by tile as in rnnt.hip with the running
//      (max, sum-exp) per row; the logits go to the workgroup's slice [16][V].
//   2. every live row's best min(K, V) candidates (no more of a row can reach the
//      utterance's top K): a wave per row, K rounds of "the best candidate
//      after the last one taken" over the row's slice;
//   3. the utterance's top K of those R K: every candidate counts the ones
//      before it in the order above (a total order, so ranks are unique);
//   4. one thread per utterance merges (length and a 64-bit prefix hash as the
//      filter, then the two back-pointer chains are walked until they meet or
//      differ), orders, appends the node records (parent, token, t, length)
//      and writes each new row's parent row and step token;
//   5. the predictor step reads h and c of the PARENT row (h: the lane's A row
//      in LDS; c: the slice, two buffers, written by another lane of the same
//      wave one barrier earlier) and rows kept by blank copy both; skipped by a
//      workgroup-uniform branch when no row changed.  g is recomputed for
//      every row after a step.
// A merged hypothesis takes the state of its blank constituent (a copy): equal
// ys give equal states bit for bit, since a row's bits do not depend on where
// the row sits.  The outputs are traced back at the end of the launch.  No
// workgroup reads what another writes; the loop runs the longest length of the
// workgroup's utterances, at most T, a bound set by the host.
//
// LM fusion (asr_rnnt_lm_* / asr_rnnt_beam_lm*; the definition is
// in include/asr_amd.h): the kernel is a template <bool LM>.  With LM a
// hypothesis carries, beside its acoustic score, W (the LM weight of ys), L (the
// log10 sum) and a slot: the index of its LM row [V] in the workgroup's pool of
// 16, the lm_position values of ys + [v] for every label v.  Candidates compare
// (s + lp[v]) + (W + ((aln10 * row[v]) + beta)), W alone at the blank.  A row is
// filled when a hypothesis takes a token, in the phase of the predictor step:
// one thread per changed row walks the node table back for the context (at most
// 7 tokens, into LDS), then all 512 threads share the changed rows' V lookups.
// A row kept by blank, at whatever rank, keeps its slot; rows that took a token
// get the slots nobody kept.  Nothing of this exists in the LM = false
// instantiation.
#include "lm_tables.h"
#include "rnnt_common.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

namespace asr {

constexpr int RB_LDS_SMALL = 8192;   // the beam state, the candidates and the wave partials
constexpr int RB_MAX_K = 16;

struct BeamArgs {
    const float* f;          // [T*B][J]
    RtNet net;
    const int32_t* lengths;
    int32_t* tokens;         // [B][nbest][max_out]
    int32_t* timesteps;
    int32_t* len;            // [B][nbest]
    double* score;
    int32_t* nhyp;           // [B]
    float* slices;           // per workgroup: c [2][L][16][Hp], g [16][J], logits [16][V]
    int4* nodes;             // [B][T*K + 1]: (parent, token, t, length); node 0 is the empty sequence
    int T, B, K, lgR, nbest, max_out, max_iters;
};

// What the LM = true instantiation takes beside BeamArgs (p.score is then am).
struct BeamLmArgs {
    LmTables lm;             // device pointers
    const int32_t* tok;      // [V]: label -> LM token
    double* rows;            // per workgroup [16][V]: the pool of LM rows
    double* total;           // [B][nbest]
    double* lm_log10;        // [B][nbest] or NULL
    int32_t* ntok;           // [B][nbest] or NULL
    double aln10, beta;
    int flags;
};

// W(ys + [y]) = W(ys) + ((aln10 * v) + beta): three rounded fp64 operations.  The pragma keeps the product
// and the sum apart on the host and on the device (__dmul_rn / __dadd_rn are plain operators, which contract).
__host__ __device__ __forceinline__ double rb_weight(double W, double aln10, double v, double beta) {
#pragma clang fp contract(off)
    const double x = aln10 * v;
    const double y = x + beta;
    return W + y;
}

// total + (aln10 * v_eos), the same way.
__host__ __device__ __forceinline__ double rb_eos_total(double total, double aln10, double v) {
#pragma clang fp contract(off)
    const double x = aln10 * v;
    return total + x;
}

// The candidate order: score descending, then the index ascending; a NaN after every number.
__host__ __device__ __forceinline__ bool rb_before(double sa, long ia, double sb, long ib) {
    if (sa > sb) return true;
    if (sa < sb) return false;
    const bool na = sa != sa, nb = sb != sb;
    if (na != nb) return nb;
    return ia < ib;
}

__device__ __forceinline__ unsigned long long rb_hash(unsigned long long h, int v) {
    h = (h ^ ((unsigned long long)(unsigned)v + 0x9e3779b97f4a7c15ull)) * 0xff51afd7ed558ccdull;
    return h ^ (h >> 32);
}

// The thread index as a value the compiler cannot trace to threadIdx: the short
// one-thread-per-item phases compute their addresses where they run, instead of
// in the prologue, where they would be held (in scratch) across the frame loop.
__device__ __forceinline__ int rb_here(int x) {
    asm volatile("" : "+v"(x));
    return x;
}

// logaddexp in fp64 for the merge: ctc_lse.h's two chains (the same operations in
// the same order), with the coefficients read from a constant table by rolled
// Horner loops.  Inlined as they stand, the chains' ~25 fp64 constants are
// hoisted into VGPRs for the whole frame loop, which then spills; a merge is one
// thread's work a few times per utterance, so the rolled form costs nothing.
__constant__ double RB_EXP_C[14] = {1.0 / 6227020800.0, 1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0,
                                    1.0 / 362880.0,     1.0 / 40320.0,     1.0 / 5040.0,     1.0 / 720.0,
                                    1.0 / 120.0,        1.0 / 24.0,        1.0 / 6.0,        0.5,
                                    1.0,                1.0};
__constant__ double RB_LOG_C[10] = {2.0 / 21.0, 2.0 / 19.0, 2.0 / 17.0, 2.0 / 15.0, 2.0 / 13.0,
                                    2.0 / 11.0, 2.0 / 9.0,  2.0 / 7.0,  2.0 / 5.0,  2.0 / 3.0};
__device__ __forceinline__ double rb_lse2(double a, double b) {
    if (a == -INFINITY) return b;
    if (b == -INFINITY) return a;
    const double x = -fabs(a - b);
    // exp(x), x in [-746, 0] (lse_exp_neg)
    const double k = __builtin_rint(x * 1.4426950408889634074);
    double r = __builtin_fma(-k, 6.93147180369123816490e-01, x);
    r = __builtin_fma(-k, 1.90821492927058770002e-10, r);
    double pe = RB_EXP_C[0];
#pragma unroll 1
    for (int i = 1; i < 14; i++) pe = __builtin_fma(pe, r, RB_EXP_C[i]);
    const double e = __builtin_ldexp(pe, (int)k);
    // log1p(e), e in [0, 1] (lse_log1p01)
    const double u = 1.0 + e;
    const double cc = e - (u - 1.0);
    const bool hi = u > 1.4142135623730951;
    const double f = hi ? 0.5 * u : u;
    const double kk = hi ? 1.0 : 0.0;
    const double num = f - 1.0, den = f + 1.0;
    double y = __builtin_amdgcn_rcp(den);
    y = __builtin_fma(y, __builtin_fma(-den, y, 1.0), y);
    y = __builtin_fma(y, __builtin_fma(-den, y, 1.0), y);
    double q = num * y;
    q = __builtin_fma(__builtin_fma(-den, q, num), y, q);
    const double s2 = q * q;
    double P = RB_LOG_C[0];
#pragma unroll 1
    for (int i = 1; i < 10; i++) P = __builtin_fma(P, s2, RB_LOG_C[i]);
    const double lf = __builtin_fma(q * s2, P, 2.0 * q);
    const double cu = cc * __builtin_amdgcn_rcp(u);
    return fmax(a, b) +
           __builtin_fma(kk, 6.93147180369123816490e-01, lf + __builtin_fma(kk, 1.90821492927058770002e-10, cu));
}

// ys(na) == ys(nb) + [v]?  Equal lengths on both sides are the caller's filter.
__device__ __forceinline__ bool rb_same_seq(const int4* nodes, int na, int nb, int v) {
    if (na == 0) return false;
    const int4 ra = nodes[na];
    if (ra.y != v) return false;
    int p = ra.x, q = nb;
    while (p != q) {
        if (p == 0 || q == 0) return false;
        const int4 rp = nodes[p], rq = nodes[q];
        if (rp.y != rq.y) return false;
        p = rp.x;
        q = rq.x;
    }
    return true;
}

template <bool LM>
__global__ __launch_bounds__(64 * RT_WAVES) void rnnt_beam_kernel(const BeamArgs p, const BeamLmArgs q) {
    extern __shared__ __attribute__((aligned(16))) float rb_lds[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    const RtNet& net = p.net;
    const int Hp = net.Hp, J = net.J, V = net.V, L = net.L, B = p.B, K = p.K;
    const int LDH = Hp + 4, LDJ = J + 4;
    const int lgR = p.lgR, R = 1 << lgR, U = RT_ROWS >> lgR;
    const int b0 = blockIdx.x * U;
    // LDS: h [2][L][16][LDH], z [16][LDJ], then the small area
    float* const hbuf = rb_lds;
    float* const zbuf = hbuf + (size_t)2 * L * RT_ROWS * LDH;
    float* const small = zbuf + (size_t)RT_ROWS * LDJ;
    // 8-byte items first: [16] each but the candidates' [16][16]
    double* const row_score = reinterpret_cast<double*>(small);
    double* const ent_score = row_score + RT_ROWS;
    double* const kept_sc = ent_score + RT_ROWS;
    double* const cand_sc = kept_sc + RT_ROWS;
    unsigned long long* const row_hash = reinterpret_cast<unsigned long long*>(cand_sc + RT_ROWS * RB_MAX_K);
    unsigned long long* const ent_hash = row_hash + RT_ROWS;
    float* const red_m = reinterpret_cast<float*>(ent_hash + RT_ROWS);          // [8][16]
    float* const red_s = red_m + RT_WAVES * RT_ROWS;
    float* const row_m = red_s + RT_WAVES * RT_ROWS;                            // the row's max logit
    float* const row_ls = row_m + RT_ROWS;                                      // log of its sum-exp
    int* const cand_v = reinterpret_cast<int*>(row_ls + RT_ROWS);               // [16][16]
    int* const cand_n = cand_v + RT_ROWS * RB_MAX_K;
    int* const row_node = cand_n + RT_ROWS;
    int* const row_len = row_node + RT_ROWS;
    int* const row_prow = row_len + RT_ROWS;     // the row whose state this row takes at the next step
    int* const row_tok = row_prow + RT_ROWS;     // the token it then steps on, -1: a copy
    int* const kept_row = row_tok + RT_ROWS;
    int* const kept_v = kept_row + RT_ROWS;
    int* const ent_node = kept_v + RT_ROWS;      // the entry's node, or the parent of the node it creates
    int* const ent_ntok = ent_node + RT_ROWS;    // the token of the node it creates, -1: none
    int* const ent_len = ent_ntok + RT_ROWS;
    int* const ent_prow = ent_len + RT_ROWS;
    int* const ent_step = ent_prow + RT_ROWS;
    int* const ent_dead = ent_step + RT_ROWS;
    int* const utt_len = ent_dead + RT_ROWS;
    int* const utt_live = utt_len + RT_ROWS;
    int* const utt_nodes = utt_live + RT_ROWS;
    // LM only: [16] each but the contexts' [16][LM_CTX]
    double* const row_W = reinterpret_cast<double*>(utt_nodes + RT_ROWS);
    double* const row_L = row_W + RT_ROWS;
    double* const kept_ac = row_L + RT_ROWS;      // the kept candidate's acoustic score (kept_sc: fused)
    double* const kept_W = kept_ac + RT_ROWS;
    double* const kept_L = kept_W + RT_ROWS;
    double* const ent_W = kept_L + RT_ROWS;
    double* const ent_L = ent_W + RT_ROWS;
    int* const row_slot = reinterpret_cast<int*>(ent_L + RT_ROWS);   // the row's LM row in the pool
    int* const ent_slot = row_slot + RT_ROWS;
    int* const lm_m = ent_slot + RT_ROWS;         // tokens of context in lm_ctx
    int* const fill_list = lm_m + RT_ROWS;        // the rows to fill, then their number at [16]
    int* const lm_ctx = fill_list + 2 * RT_ROWS;  // [16][LM_CTX]: the row's last LM tokens, oldest first
    auto hb = [&](int buf, int l) { return hbuf + ((size_t)buf * L + l) * RT_ROWS * LDH; };
    // this workgroup's slice: c [2][L][16][Hp], g [16][J], logits [16][V]
    const size_t csz = (size_t)L * RT_ROWS * Hp;
    float* const cw = p.slices + (size_t)blockIdx.x * (2 * csz + (size_t)RT_ROWS * J + (size_t)RT_ROWS * V);
    float* const gw = cw + 2 * csz;
    float* const lg = gw + (size_t)RT_ROWS * J;
    const size_t npu = (size_t)p.T * K + 1;      // nodes per utterance
    double* const lmw = LM ? q.rows + (size_t)blockIdx.x * RT_ROWS * V : nullptr;

    if (tid < RT_ROWS) {
        row_score[tid] = 0.0;
        row_hash[tid] = 0x243f6a8885a308d3ull;
        row_node[tid] = 0;
        row_len[tid] = 0;
        row_prow[tid] = tid;
        row_tok[tid] = net.blank;    // the start step on Emb[blank], every row
        const int b = b0 + tid;
        utt_len[tid] = (tid < U && b < B) ? (p.lengths ? min(max(p.lengths[b], 0), p.T) : p.T) : 0;
        utt_live[tid] = 1;
        utt_nodes[tid] = 1;
        if constexpr (LM) {
            row_W[tid] = 0.0;
            row_L[tid] = 0.0;
            row_slot[tid] = tid;
        }
    }
    for (int x = tid; x < L * RT_ROWS * Hp; x += 64 * RT_WAVES) {
        const int l = x / (RT_ROWS * Hp), row = (x / Hp) % RT_ROWS, n = x % Hp;
        hb(0, l)[row * LDH + n] = 0.f;
    }
    for (int l = 0; l < L; l++)
        for (int jt = w; jt < (Hp >> 4); jt += RT_WAVES)
#pragma unroll
            for (int j = 0; j < 4; j++) cw[(unsigned)((l * RT_ROWS + 4 * g + j) * Hp + 16 * jt + c)] = 0.f;
    __syncthreads();

    int cur = 0;
    for (int it = 0;; it++) {
        int any_change = 0, any_live = 0;
#pragma unroll
        for (int x = 0; x < RT_ROWS; x++) {
            any_change |= (row_tok[x] >= 0) | (row_prow[x] != x);
            any_live |= it < utt_len[x];
        }
        if (any_change) {
            if constexpr (LM) {
                // The LM rows of the hypotheses that took a token (at the start: the empty one of every utterance).
                if (tid < RT_ROWS) {
                    const int row = rb_here(tid), u = row >> lgR;
                    const bool need = row_tok[row] >= 0 && (it > 0 || ((row & (R - 1)) == 0 && b0 + u < B));
                    const unsigned long long mask = __ballot(need);
                    if (need) {
                        fill_list[__popcll(mask & ((1ull << row) - 1))] = row;
                        const int4* const nodes = p.nodes + (size_t)(b0 + u) * npu;
                        const int m = min(row_len[row], LM_CTX);
                        int n = row_node[row];
                        for (int x = m - 1; x >= 0; x--) {
                            const int4 rec = nodes[n];
                            lm_ctx[row * LM_CTX + x] = q.tok[rec.y];
                            n = rec.x;
                        }
                        lm_m[row] = m;
                    }
                    if (row == 0) fill_list[RT_ROWS] = __popcll(mask);
                }
                __syncthreads();
                const int nf = fill_list[RT_ROWS] * V;   // <= 16 V
                for (int x = tid; x < nf; x += 64 * RT_WAVES) {
                    const int k = x / V, v = x - k * V, row = fill_list[k];
                    int32_t ctx[LM_CTX];
#pragma unroll
                    for (int j = 0; j < LM_CTX; j++) ctx[j] = lm_ctx[row * LM_CTX + j];
                    double val = 0.0;
                    if (v != net.blank) val = lm_value_after(q.lm, ctx, lm_m[row], q.tok[v], false, q.flags);
                    lmw[(unsigned)(row_slot[row] * V + v)] = val;
                }
            }
            // Predictor step by parent row; rows without a token copy their parent's h and c.
            rt_lstm_step(net, hb, cur, cw + (size_t)cur * csz, cw + (size_t)(cur ^ 1) * csz,
                         [&](int row) { return row_prow[row]; }, [&](int row) { return row_tok[row]; }, w, g, c);
            cur ^= 1;
            // g = h_top.W_pred + b_pred of every row
            rt_sweep<1, false>(hb(cur, L - 1) + c * LDH + 4 * g, 0, Hp >> 4, net.wpred, net.bpred, J, w, g, c,
                               [&](int, int n, f32x4 x) {
#pragma unroll
                                   for (int j = 0; j < 4; j++) gw[(unsigned)((4 * g + j) * J + n)] = x[j];
                               });
        }
        if (!any_live || it >= p.max_iters) break;

        // z = act(f_t + g): the lane that owns g's element; every row of an utterance at frame it
        {
            const float* ft = p.f + ((size_t)min(it, p.T - 1) * B + b0) * J;   // uniform; a row adds less than 16 J
            for (int jt = w; jt < (J >> 4); jt += RT_WAVES) {
                const int n = 16 * jt + c;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int row = 4 * g + j;
                    const int du = min(row >> lgR, B - 1 - b0);
                    const float x = ft[(unsigned)(du * J + n)] + gw[(unsigned)(row * J + n)];
                    zbuf[row * LDJ + n] = rt_act(x, net.act);
                }
            }
        }
        __syncthreads();

        // logit = z.W_out + b_out over the V column tiles, kept in the slice; columns >= V do not exist
        RtTop top[4];
#pragma unroll
        for (int j = 0; j < 4; j++) top[j] = RtTop{-INFINITY, 0.f, 0};   // no argmax here: every index is 0
        rt_sweep<1, true>(zbuf + c * LDJ + 4 * g, 0, J >> 4, net.wout, net.bout, V, w, g, c, [&](int, int n, f32x4 x) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                rt_push(top[j], x[j], 0);
                lg[(unsigned)(4 * g + j) * (unsigned)V + (unsigned)n] = x[j];
            }
        });
        // the 16 lanes of a row, then the waves in the order 0..7
#pragma unroll
        for (int j = 0; j < 4; j++) rt_row_partial<false>(top[j], c, w * RT_ROWS + 4 * g + j, red_m, red_s, nullptr);
        __syncthreads();
        if (tid < RT_ROWS) {
            const RtTop a = rt_row_total<false>(tid, RT_ROWS, red_m, red_s, nullptr);
            row_m[tid] = a.m;
            row_ls[tid] = logf(a.s);   // lp[v] = (logit[v] - max) - log(sum-exp): -logf(s) at the maximum, as in rnnt.hip
        }
        __syncthreads();   // and the slice's logits, written by other waves

        // every live row's best min(K, V) candidates: wave w takes rows 2w and 2w + 1
        for (int rr = 0; rr < 2; rr++) {
            const int row = 2 * w + rr, u = row >> lgR, i = row & (R - 1);
            const int kc = (i < utt_live[u] && it < utt_len[u]) ? min(K, V) : 0;
            if (lane == 0) cand_n[row] = kc;
            const double s = row_score[row];
            const float m = row_m[row], ls = row_ls[row];
            const float* lr = lg + (unsigned)row * (unsigned)V;   // 16 V < 2^32: V * J <= INT_MAX
            const double Wr = LM ? row_W[row] : 0.0;
            const double* const wr = LM ? lmw + (unsigned)(row_slot[row] * V) : nullptr;
            double lsc = 0.0;
            int lv = -1;
            for (int r = 0; r < kc; r++) {
                double bs = 0.0;
                int bv = RT_NONE;
                for (int v = lane; v < V; v += 64) {
                    double sc = s + (double)((lr[v] - m) - ls);
                    if constexpr (LM) sc = __dadd_rn(sc, v == net.blank ? Wr : rb_weight(Wr, q.aln10, wr[v], q.beta));
                    if ((r == 0 || rb_before(lsc, lv, sc, v)) && (bv == RT_NONE || rb_before(sc, v, bs, bv))) {
                        bs = sc;
                        bv = v;
                    }
                }
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const double os = __shfl_xor(bs, d);
                    const int ov = __shfl_xor(bv, d);
                    if (ov != RT_NONE && (bv == RT_NONE || rb_before(os, ov, bs, bv))) {
                        bs = os;
                        bv = ov;
                    }
                }
                lsc = bs;
                lv = bv;
                if (lane == 0) {
                    cand_sc[row * RB_MAX_K + r] = bs;
                    cand_v[row * RB_MAX_K + r] = bv;
                }
            }
        }
        __syncthreads();

        // the utterance's top K of its rows' candidates, by counting the candidates before each
        if (tid < RT_ROWS * RB_MAX_K) {
            const int td = rb_here(tid);
            const int row = td >> 4, r = td & 15;
            if (r < cand_n[row]) {
                const int base = (row >> lgR) << lgR;
                const double sc = cand_sc[td];
                const int v = cand_v[td];
                const long idx = (long)(row - base) * V + v;
                int rank = 0;
                for (int i2 = 0; i2 < R; i2++) {
                    const int row2 = base + i2, n2 = cand_n[row2];
                    for (int r2 = 0; r2 < n2; r2++)
                        rank += rb_before(cand_sc[row2 * RB_MAX_K + r2], (long)i2 * V + cand_v[row2 * RB_MAX_K + r2], sc,
                                          idx);
                }
                if (rank < K) {
                    kept_row[base + rank] = row;
                    kept_v[base + rank] = v;
                    kept_sc[base + rank] = sc;
                    if constexpr (LM) {   // the parts of sc, by step 2's operations
                        const bool bl = v == net.blank;
                        const double val = bl ? 0.0 : lmw[(unsigned)(row_slot[row] * V + v)];
                        kept_ac[base + rank] =
                            row_score[row] + (double)((lg[(unsigned)row * (unsigned)V + (unsigned)v] - row_m[row]) - row_ls[row]);
                        kept_W[base + rank] = bl ? row_W[row] : rb_weight(row_W[row], q.aln10, val, q.beta);
                        kept_L[base + rank] = bl ? row_L[row] : __dadd_rn(row_L[row], val);
                    }
                }
            }
        }
        __syncthreads();

        // one thread per utterance: merge, order, append the nodes, set the next step
        if (tid < U) {
            const int u = rb_here(tid), base = u << lgR;
            if (it < utt_len[u]) {
                int4* const nodes = p.nodes + (size_t)(b0 + u) * npu;
                int total = 0;
                for (int i = 0; i < R; i++) total += cand_n[base + i];
                const int nk = min(K, total);
                for (int j = 0; j < nk; j++) {
                    const int e = base + j, row = kept_row[e], v = kept_v[e];
                    const bool bl = v == net.blank;
                    ent_score[e] = LM ? kept_ac[e] : kept_sc[e];
                    if constexpr (LM) {
                        ent_W[e] = kept_W[e];
                        ent_L[e] = kept_L[e];
                        ent_slot[e] = row_slot[row];
                    }
                    ent_prow[e] = row;
                    ent_step[e] = bl ? -1 : v;
                    ent_ntok[e] = bl ? -1 : v;
                    ent_node[e] = row_node[row];
                    ent_len[e] = row_len[row] + (bl ? 0 : 1);
                    ent_hash[e] = bl ? row_hash[row] : rb_hash(row_hash[row], v);
                    ent_dead[e] = 0;
                }
                // A + blank against B + v: at most one partner each (see the top of the file)
                for (int j = 0; j < nk; j++) {
                    const int ej = base + j;
                    if (ent_ntok[ej] >= 0 || ent_dead[ej]) continue;
                    for (int m = 0; m < nk; m++) {
                        const int em = base + m;
                        if (m == j || ent_ntok[em] < 0 || ent_dead[em] || ent_len[em] != ent_len[ej] ||
                            ent_hash[em] != ent_hash[ej] || !rb_same_seq(nodes, ent_node[ej], ent_node[em], ent_ntok[em]))
                            continue;
                        const double sj = ent_score[ej], sm = ent_score[em];
                        // with LM the fused scores decide; W is the same on both sides
                        const double fj = LM ? __dadd_rn(sj, ent_W[ej]) : sj, fm = LM ? __dadd_rn(sm, ent_W[em]) : sm;
                        const bool blank_wins = fj > fm || (fj == fm && j < m);
                        const int keep = min(ej, em), drop = max(ej, em);
                        const int node = blank_wins ? ent_node[ej] : ent_node[em];
                        const int ntok = blank_wins ? -1 : ent_ntok[em];
                        const int prow = ent_prow[ej];
                        ent_score[keep] = rb_lse2(sj, sm);
                        ent_node[keep] = node;
                        ent_ntok[keep] = ntok;
                        ent_prow[keep] = prow;     // the state of the blank constituent, a copy
                        ent_step[keep] = -1;
                        ent_dead[drop] = 1;
                        if constexpr (LM) {
                            ent_W[keep] = ent_W[ej];
                            ent_L[keep] = ent_L[ej];
                            ent_slot[keep] = ent_slot[ej];   // the blank constituent's row: the same sequence
                        }
                        break;
                    }
                }
                unsigned used = 0;   // LM: the slots of the rows that keep theirs
                if constexpr (LM) {
                    for (int j = 0; j < nk; j++) {
                        const int e = base + j;
                        if (!ent_dead[e] && ent_step[e] < 0) used |= 1u << (ent_slot[e] - base);
                        kept_sc[e] = __dadd_rn(ent_score[e], ent_W[e]);   // the entry's fused score
                    }
                }
                const double* const ord = LM ? kept_sc : ent_score;
                int nl = 0;
                for (int j = 0; j < nk; j++) {
                    const int e = base + j;
                    if (ent_dead[e]) continue;
                    int rank = 0;
                    for (int m = 0; m < nk; m++) rank += !ent_dead[base + m] && rb_before(ord[base + m], m, ord[e], j);
                    int node = ent_node[e];
                    if (ent_ntok[e] >= 0) {
                        const int id = utt_nodes[u]++;
                        nodes[id] = make_int4(node, ent_ntok[e], it, ent_len[e]);
                        node = id;
                    }
                    const int nr = base + rank;
                    row_score[nr] = ent_score[e];
                    row_node[nr] = node;
                    row_len[nr] = ent_len[e];
                    row_hash[nr] = ent_hash[e];
                    row_prow[nr] = ent_prow[e];
                    row_tok[nr] = ent_step[e];
                    if constexpr (LM) {
                        row_W[nr] = ent_W[e];
                        row_L[nr] = ent_L[e];
                        int sl = ent_slot[e] - base;
                        if (ent_step[e] >= 0) {   // a new sequence: the lowest slot nobody keeps
                            sl = __ffs(~used) - 1;
                            used |= 1u << sl;
                        }
                        row_slot[nr] = base + sl;
                    }
                    nl++;
                }
                for (int i = nl; i < R; i++) {
                    row_prow[base + i] = base + i;
                    row_tok[base + i] = -1;
                    if constexpr (LM) {   // the slots stay a permutation
                        const int sl = __ffs(~used) - 1;
                        used |= 1u << sl;
                        row_slot[base + i] = base + sl;
                    }
                }
                utt_live[u] = nl;
            } else {
                for (int i = 0; i < R; i++) {
                    row_prow[base + i] = base + i;
                    row_tok[base + i] = -1;
                }
            }
        }
        __syncthreads();
    }

    // trace back: one thread per final hypothesis
    int out_rank = -1;   // LM: the rank by total
    if constexpr (LM) {
        double total = 0.0;
        bool live = false;
        if (tid < RT_ROWS) {
            const int td = rb_here(tid);
            const int u = td >> lgR, j = td & (R - 1), b = b0 + u;
            live = b < B && j < utt_live[u];
            if (live) {
                total = __dadd_rn(row_score[td], row_W[td]);
                if (q.flags & ASR_LM_EOS) {
                    const int4* const nodes = p.nodes + (size_t)b * npu;
                    const int m = min(row_len[td], LM_CTX);
                    int n = row_node[td];
                    for (int x = m - 1; x >= 0; x--) {
                        const int4 rec = nodes[n];
                        lm_ctx[td * LM_CTX + x] = q.tok[rec.y];
                        n = rec.x;
                    }
                    int32_t ctx[LM_CTX];
#pragma unroll
                    for (int x = 0; x < LM_CTX; x++) ctx[x] = x < m ? lm_ctx[td * LM_CTX + x] : 0;
                    const double ve = lm_value_after(q.lm, ctx, m, 0, true, q.flags);
                    total = rb_eos_total(total, q.aln10, ve);
                    row_L[td] = __dadd_rn(row_L[td], ve);
                }
                ent_score[td] = total;
            }
        }
        __syncthreads();
        if (live) {
            const int td = rb_here(tid);
            const int u = td >> lgR, j = td & (R - 1), base = u << lgR;
            out_rank = 0;
            for (int m = 0; m < utt_live[u]; m++) out_rank += rb_before(ent_score[base + m], m, total, j);
        }
    }
    if (tid < RT_ROWS) {
        const int td = rb_here(tid);
        const int u = td >> lgR, j = LM ? out_rank : td & (R - 1), b = b0 + u;
        if (b < B) {
            const int nh = min(utt_live[u], p.nbest);
            if ((td & (R - 1)) == 0) p.nhyp[b] = nh;
            if (j >= 0 && j < nh) {
                const int4* const nodes = p.nodes + (size_t)b * npu;
                const size_t o = (size_t)b * p.nbest + j;
                p.len[o] = row_len[td];
                if (!LM || p.score) p.score[o] = row_score[td];
                if constexpr (LM) {
                    q.total[o] = ent_score[td];
                    if (q.lm_log10) q.lm_log10[o] = row_L[td];
                    if (q.ntok) q.ntok[o] = row_len[td];
                }
                for (int n = row_node[td]; n != 0;) {
                    const int4 rec = nodes[n];
                    if (rec.w - 1 < p.max_out) {
                        p.tokens[o * p.max_out + rec.w - 1] = rec.y;
                        p.timesteps[o * p.max_out + rec.w - 1] = rec.z;
                    }
                    n = rec.x;
                }
            }
        }
    }
}

// The checks the device and the host search share, before any HIP call.
static int rnnt_beam_check(const asr_rnnt* h, const void* enc, int T, int B, int K, int nbest, int max_out,
                           const void* tokens, const void* timesteps, const void* len, const void* score,
                           const void* nhyp) {
    if (!h || !enc || !len || !score || !nhyp || T <= 0 || B <= 0) return ASR_ERR_ARG;
    if (K < 1 || K > RB_MAX_K) return ASR_ERR_ARG;
    if (nbest < 1 || nbest > K) return ASR_ERR_ARG;
    if (max_out < 0) return ASR_ERR_ARG;
    if (max_out > 0 && (!tokens || !timesteps)) return ASR_ERR_ARG;
    if ((long)T * B > INT_MAX || (long)T * K + 1 > INT_MAX) return ASR_ERR_UNSUPPORTED;
    return ASR_OK;
}

static int rb_log2_rows(int K) {
    int lg = 0;
    while ((1 << lg) < K) lg++;
    return lg;
}

// A hypothesis of the host twin.
struct BeamHyp {
    std::vector<int32_t> ys, ts;
    double score = 0.0;           // acoustic
    double W = 0.0, Lg = 0.0;     // LM weight and log10 sum of ys
    std::vector<double> h, c, g;
    std::vector<double> lmv;      // LM: lm_position's value of ys + [v], every label v
};
struct BeamCand {
    double score;   // acoustic
    double w;       // the LM weight of the candidate's sequence, 0 without an LM
    double fused;   // score + w
    int i, v;
    long pos;     // position in candidate order (of the earlier constituent after a merge)
    int ts_parent;  // merged and the token constituent won: the hypothesis whose timesteps it extends; else -1
    bool dead;
};

}  // namespace asr

// The fusion handle: a model, an LM and how they combine.  Both must outlive it.
struct asr_rnnt_lm {
    const asr_rnnt* model = nullptr;
    const asr_lm* lm = nullptr;
    std::vector<int32_t> tok;     // [V]: label -> LM token
    int32_t* d_tok = nullptr;     // its device copy, made by the first asr_rnnt_beam_lm
    double aln10 = 0.0, beta = 0.0;
    int flags = 0;
};

namespace asr {
static int rnnt_beam_host_run(const asr_rnnt* h, const asr_rnnt_lm* z, const float* h_enc, const int32_t* h_lengths,
                              int T, int B, int K, int nbest, int max_out, int32_t* h_tokens, int32_t* h_timesteps,
                              int32_t* h_len, double* h_total, double* h_am, double* h_lm_log10, int32_t* h_ntok,
                              int32_t* h_nhyp, double* h_margin);
}

namespace asr {

// f [T*B][J]; per workgroup c [2][L][16][Hp], g [16][J], logits [16][V]; per utterance T*K + 1 nodes of 16 bytes;
// with an LM, per workgroup the pool of LM rows [16][V] of doubles behind the nodes.
static size_t rnnt_beam_work_bytes(const asr_rnnt* h, int T, int B, int K, bool lm) {
    if (!h || T <= 0 || B <= 0 || K < 1 || K > RB_MAX_K || (long)T * B > INT_MAX || (long)T * K + 1 > INT_MAX) return 0;
    const size_t U = (size_t)RT_ROWS >> rb_log2_rows(K);
    const size_t tiles = ((size_t)B + U - 1) / U;
    return ((size_t)T * B * h->d.J + tiles * RT_ROWS * ((size_t)2 * h->d.L * h->d.Hp + h->d.J + h->d.V)) * sizeof(float) +
           (size_t)B * ((size_t)T * K + 1) * sizeof(int4) + (lm ? tiles * RT_ROWS * (size_t)h->d.V * sizeof(double) : 0);
}

// The GEMM for f and the search's one launch; z = NULL: without an LM.  The arguments were checked.
static int rnnt_beam_launch(const asr_rnnt* h, const asr_rnnt_lm* z, const LmTables* lmdev, const float* d_enc,
                            const int32_t* d_lengths, int T, int B, int K, int nbest, int max_out, int32_t* d_tokens,
                            int32_t* d_timesteps, int32_t* d_len, double* d_score, double* d_total, double* d_lm_log10,
                            int32_t* d_ntok, int32_t* d_nhyp, void* d_work, asr_stream_t s) {
    const asr_rnnt_desc& d = h->d;
    const long lds = rnnt_lds_bytes(d.L, d.Hp, d.J, RB_LDS_SMALL);
    float* f = (float*)d_work;
    if (int rc = rnnt_enc_launch(h, d_enc, T, B, f, asr_stream(s))) return rc;
    const int lgR = asr::rb_log2_rows(K), U = asr::RT_ROWS >> lgR;
    const size_t tiles = ((size_t)B + U - 1) / U;
    asr::BeamArgs a{};
    a.f = f;
    a.net = rnnt_net(h);
    a.lengths = d_lengths;
    a.tokens = d_tokens; a.timesteps = d_timesteps; a.len = d_len; a.score = d_score; a.nhyp = d_nhyp;
    a.slices = f + (size_t)T * B * d.J;
    a.nodes = reinterpret_cast<int4*>(a.slices + tiles * asr::RT_ROWS * ((size_t)2 * d.L * d.Hp + d.J + d.V));
    a.T = T; a.B = B; a.K = K; a.lgR = lgR; a.nbest = nbest; a.max_out = max_out;
    a.max_iters = T;   // one joint evaluation per hypothesis and frame
    asr::BeamLmArgs q{};
    if (z) {
        q.lm = *lmdev;
        q.tok = z->d_tok;
        q.rows = reinterpret_cast<double*>(a.nodes + (size_t)B * ((size_t)T * K + 1));
        q.total = d_total;
        q.lm_log10 = d_lm_log10;
        q.ntok = d_ntok;
        q.aln10 = z->aln10;
        q.beta = z->beta;
        q.flags = z->flags;
        static AsrAttrOnce attr;
        if (int rc = attr.set((const void*)rnnt_beam_kernel<true>, RT_LDS_MAX)) return rc;
        hipLaunchKernelGGL(rnnt_beam_kernel<true>, dim3((unsigned)tiles), dim3(64 * RT_WAVES), (size_t)lds, asr_stream(s),
                           a, q);
    } else {
        static AsrAttrOnce attr;
        if (int rc = attr.set((const void*)rnnt_beam_kernel<false>, RT_LDS_MAX)) return rc;
        hipLaunchKernelGGL(rnnt_beam_kernel<false>, dim3((unsigned)tiles), dim3(64 * RT_WAVES), (size_t)lds, asr_stream(s),
                           a, q);
    }
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

}  // namespace asr

extern "C" {

size_t asr_rnnt_beam_workspace_bytes(const asr_rnnt_t* h, int T, int B, int K) {
    return asr::rnnt_beam_work_bytes(h, T, B, K, false);
}

int asr_rnnt_beam(const asr_rnnt_t* h, const float* d_enc, const int32_t* d_lengths, int T, int B, int K, int nbest,
                  int max_out, int32_t* d_tokens, int32_t* d_timesteps, int32_t* d_len, double* d_score,
                  int32_t* d_nhyp, void* d_work, asr_stream_t s) {
    if (int rc = asr::rnnt_beam_check(h, d_enc, T, B, K, nbest, max_out, d_tokens, d_timesteps, d_len, d_score, d_nhyp))
        return rc;
    if (!d_work) return ASR_ERR_ARG;
    if (asr::rnnt_lds_bytes(h->d.L, h->d.Hp, h->d.J, asr::RB_LDS_SMALL) > asr::RT_LDS_MAX) return ASR_ERR_UNSUPPORTED;
    if (!h->d_blob) return ASR_ERR_STATE;
    return asr::rnnt_beam_launch(h, nullptr, nullptr, d_enc, d_lengths, T, B, K, nbest, max_out, d_tokens, d_timesteps,
                                 d_len, d_score, nullptr, nullptr, nullptr, d_nhyp, d_work, s);
}

int asr_rnnt_beam_host(const asr_rnnt_t* h, const float* h_enc, const int32_t* h_lengths, int T, int B, int K,
                       int nbest, int max_out, int32_t* h_tokens, int32_t* h_timesteps, int32_t* h_len,
                       double* h_score, int32_t* h_nhyp, double* h_margin) {
    if (int rc = asr::rnnt_beam_check(h, h_enc, T, B, K, nbest, max_out, h_tokens, h_timesteps, h_len, h_score, h_nhyp))
        return rc;
    return asr::rnnt_beam_host_run(h, nullptr, h_enc, h_lengths, T, B, K, nbest, max_out, h_tokens, h_timesteps, h_len,
                                   h_score, nullptr, nullptr, nullptr, h_nhyp, h_margin);
}

}  // extern "C"

namespace asr {

// lm_position's values of ys + [v] for every label v (0 at the blank): the host twin's LM row.
static void rnnt_lm_row(const asr_rnnt_lm& z, const LmTables& t, const std::vector<int32_t>& ys, int V, int blank,
                        std::vector<double>& out) {
    std::vector<int32_t> row(ys.size() + 1);
    for (size_t x = 0; x < ys.size(); x++) row[x] = z.tok[(size_t)ys[x]];
    out.assign((size_t)V, 0.0);
    for (int v = 0; v < V; v++) {
        if (v == blank) continue;
        row[ys.size()] = z.tok[(size_t)v];
        out[(size_t)v] = lm_position(t, row.data(), (int)row.size(), (int)ys.size(), z.flags & ASR_LM_BOS).v;
    }
}

// The search on host memory, one thread, fp64.  z = NULL: asr_rnnt_beam_host (h_total is its score array and
// every W is absent); else asr_rnnt_beam_lm_host.  The arguments were checked.
static int rnnt_beam_host_run(const asr_rnnt* h, const asr_rnnt_lm* z, const float* h_enc, const int32_t* h_lengths,
                              int T, int B, int K, int nbest, int max_out, int32_t* h_tokens, int32_t* h_timesteps,
                              int32_t* h_len, double* h_total, double* h_am, double* h_lm_log10, int32_t* h_ntok,
                              int32_t* h_nhyp, double* h_margin) {
    const asr_rnnt_desc& d = h->d;
    const size_t LH = (size_t)d.L * d.Hp;
    const LmTables* lt = nullptr;
    if (z) {
        const LmTables* dev;
        (void)asr_internal_lm_tables(z->lm, &lt, &dev);
    }
    try {
        asr::RnntHost m(*h);
        std::vector<double> logit(d.V);
        std::vector<BeamCand> cands, kept;
        for (int b = 0; b < B; b++) {
            std::vector<BeamHyp> A(1);
            A[0].h.assign(LH, 0.0);
            A[0].c.assign(LH, 0.0);
            m.step(d.blank, A[0].h.data(), A[0].c.data());
            m.pred_proj(A[0].h.data());
            A[0].g = m.g;
            if (z) rnnt_lm_row(*z, *lt, A[0].ys, d.V, d.blank, A[0].lmv);
            const int len = h_lengths ? std::min(std::max(h_lengths[b], 0), T) : T;
            double margin = HUGE_VAL;
            for (int t = 0; t < len; t++) {
                m.enc_proj(h_enc + ((size_t)t * B + b) * d.E);
                cands.clear();
                for (int i = 0; i < (int)A.size(); i++) {
                    m.logits(A[i].g.data(), logit.data());
                    double best = -HUGE_VAL;
                    for (int v = 0; v < d.V; v++)
                        if (logit[v] > best) best = logit[v];
                    double se = 0.0;
                    for (int v = 0; v < d.V; v++) se += std::exp(logit[v] - best);
                    const double lse = best + std::log(se);
                    for (int v = 0; v < d.V; v++) {
                        const double ac = A[i].score + (logit[v] - lse);
                        if (!z) {
                            cands.push_back(BeamCand{ac, 0.0, ac, i, v, 0, -1, false});
                        } else {
                            const double w =
                                v == d.blank ? A[i].W : rb_weight(A[i].W, z->aln10, A[i].lmv[(size_t)v], z->beta);
                            cands.push_back(BeamCand{ac, w, ac + w, i, v, 0, -1, false});
                        }
                    }
                }
                const size_t nk = std::min((size_t)K, cands.size());
                const size_t ns = std::min(nk + 1, cands.size());   // one more, for the margin
                const long V = d.V;
                std::partial_sort(cands.begin(), cands.begin() + ns, cands.end(),
                                  [V](const BeamCand& x, const BeamCand& y) {
                                      return asr::rb_before(x.fused, x.i * V + x.v, y.fused, y.i * V + y.v);
                                  });
                if (ns > nk) margin = std::min(margin, cands[nk - 1].fused - cands[nk].fused);
                kept.assign(cands.begin(), cands.begin() + nk);
                for (size_t j = 0; j < nk; j++) kept[j].pos = (long)j;
                // A + blank against B + v: at most one partner each (see the top of the file)
                for (size_t j = 0; j < nk; j++) {
                    if (kept[j].v != d.blank || kept[j].dead) continue;
                    const std::vector<int32_t>& ya = A[kept[j].i].ys;
                    for (size_t x = 0; x < nk; x++) {
                        if (x == j || kept[x].v == d.blank || kept[x].dead) continue;
                        const std::vector<int32_t>& yb = A[kept[x].i].ys;
                        if (ya.size() != yb.size() + 1 || ya.back() != kept[x].v ||
                            !std::equal(yb.begin(), yb.end(), ya.begin()))
                            continue;
                        const double sj = kept[j].score, sx = kept[x].score;
                        const double fj = kept[j].fused, fx = kept[x].fused;   // the same W on both sides
                        margin = std::min(margin, std::fabs(fj - fx));
                        const bool blank_wins = fj > fx || (fj == fx && j < x);
                        const size_t keep = std::min(j, x), drop = std::max(j, x);
                        BeamCand e = kept[j];   // the blank constituent: its state, a copy
                        e.score = std::max(sj, sx) + std::log1p(std::exp(-std::fabs(sj - sx)));
                        e.fused = z ? e.score + e.w : e.score;
                        e.pos = (long)keep;
                        e.ts_parent = blank_wins ? -1 : kept[x].i;
                        kept[keep] = e;
                        kept[drop].dead = true;
                        break;
                    }
                }
                std::vector<BeamCand> live;
                for (size_t j = 0; j < nk; j++)
                    if (!kept[j].dead) live.push_back(kept[j]);
                std::stable_sort(live.begin(), live.end(), [](const BeamCand& x, const BeamCand& y) {
                    return asr::rb_before(x.fused, x.pos, y.fused, y.pos);
                });
                std::vector<BeamHyp> N(live.size());
                for (size_t j = 0; j < live.size(); j++) {
                    const BeamCand& e = live[j];
                    N[j] = A[e.i];
                    N[j].score = e.score;
                    if (e.ts_parent >= 0) {          // merged, the token constituent's timesteps
                        N[j].ts = A[e.ts_parent].ts;
                        N[j].ts.push_back(t);
                    } else if (e.v != d.blank) {
                        N[j].ys.push_back(e.v);
                        N[j].ts.push_back(t);
                        m.step(e.v, N[j].h.data(), N[j].c.data());
                        m.pred_proj(N[j].h.data());
                        N[j].g = m.g;
                        if (z) {
                            N[j].W = e.w;
                            N[j].Lg = A[e.i].Lg + A[e.i].lmv[(size_t)e.v];
                            rnnt_lm_row(*z, *lt, N[j].ys, d.V, d.blank, N[j].lmv);
                        }
                    }
                }
                A.swap(N);
            }
            // the totals; with an LM the final A is ranked again by them (</s> can change the order)
            std::vector<double> total(A.size());
            std::vector<size_t> ord(A.size());
            for (size_t j = 0; j < A.size(); j++) {
                ord[j] = j;
                total[j] = z ? A[j].score + A[j].W : A[j].score;
                if (z && (z->flags & ASR_LM_EOS)) {
                    std::vector<int32_t> row(A[j].ys.size());
                    for (size_t x = 0; x < row.size(); x++) row[x] = z->tok[(size_t)A[j].ys[x]];
                    const double ve =
                        lm_position(*lt, row.data(), (int)row.size(), (int)row.size(), z->flags & ASR_LM_BOS).v;
                    total[j] = rb_eos_total(total[j], z->aln10, ve);
                    A[j].Lg = A[j].Lg + ve;
                }
            }
            if (z)
                std::stable_sort(ord.begin(), ord.end(),
                                 [&](size_t x, size_t y) { return rb_before(total[x], (long)x, total[y], (long)y); });
            for (size_t j = 0; j + 1 < A.size(); j++) margin = std::min(margin, total[ord[j]] - total[ord[j + 1]]);
            const int nh = (int)std::min(A.size(), (size_t)nbest);
            h_nhyp[b] = nh;
            for (int j = 0; j < nh; j++) {
                const size_t o = (size_t)b * nbest + j;
                const BeamHyp& a = A[ord[(size_t)j]];
                h_len[o] = (int32_t)a.ys.size();
                h_total[o] = total[ord[(size_t)j]];
                if (h_am) h_am[o] = a.score;
                if (h_lm_log10) h_lm_log10[o] = a.Lg;
                if (h_ntok) h_ntok[o] = (int32_t)a.ys.size();
                for (int x = 0; x < (int)a.ys.size() && x < max_out; x++) {
                    h_tokens[o * max_out + x] = a.ys[x];
                    h_timesteps[o * max_out + x] = a.ts[x];
                }
            }
            if (h_margin) h_margin[b] = margin;
        }
    } catch (const std::bad_alloc&) {
        return ASR_ERR_OOM;
    }
    return ASR_OK;
}

}  // namespace asr

extern "C" {

int asr_rnnt_lm_create(const asr_rnnt_t* model, const asr_lm_t* lm, const int32_t* tok_of_label, float alpha,
                       float beta, int lm_flags, asr_rnnt_lm_t** out) {
    if (!out) return ASR_ERR_ARG;
    *out = nullptr;
    if (!model || !lm || !tok_of_label) return ASR_ERR_ARG;
    if (!std::isfinite(alpha) || alpha < 0.0f || !std::isfinite(beta)) return ASR_ERR_ARG;
    if (lm_flags & ~(ASR_LM_BOS | ASR_LM_EOS)) return ASR_ERR_ARG;
    const asr::LmTables *host, *dev;
    (void)asr_internal_lm_tables(lm, &host, &dev);
    if (((lm_flags & ASR_LM_BOS) && host->bos < 0) || ((lm_flags & ASR_LM_EOS) && host->eos < 0)) return ASR_ERR_ARG;
    asr_rnnt_lm* z = nullptr;
    try {
        z = new asr_rnnt_lm();
        z->tok.assign(tok_of_label, tok_of_label + model->d.V);
    } catch (const std::bad_alloc&) {
        delete z;
        return ASR_ERR_OOM;
    }
    z->model = model;
    z->lm = lm;
    z->aln10 = (double)alpha * 2.302585092994046;
    z->beta = (double)beta;
    z->flags = lm_flags;
    *out = z;
    return ASR_OK;
}

int asr_rnnt_lm_destroy(asr_rnnt_lm_t* z) {
    if (!z) return ASR_ERR_ARG;
    if (z->d_tok) {
        (void)hipDeviceSynchronize();
        (void)hipFree(z->d_tok);
    }
    delete z;
    return ASR_OK;
}

size_t asr_rnnt_beam_lm_workspace_bytes(const asr_rnnt_lm_t* z, int T, int B, int K) {
    return z ? asr::rnnt_beam_work_bytes(z->model, T, B, K, true) : 0;
}

int asr_rnnt_beam_lm(asr_rnnt_lm_t* z, const float* d_enc, const int32_t* d_lengths, int T, int B, int K, int nbest,
                     int max_out, int32_t* d_tokens, int32_t* d_timesteps, int32_t* d_len, double* d_total,
                     double* d_am, double* d_lm_log10, int32_t* d_ntok, int32_t* d_nhyp, void* d_work, asr_stream_t s) {
    if (!z) return ASR_ERR_ARG;
    const asr_rnnt* h = z->model;
    if (int rc = asr::rnnt_beam_check(h, d_enc, T, B, K, nbest, max_out, d_tokens, d_timesteps, d_len, d_total, d_nhyp))
        return rc;
    if (!d_work) return ASR_ERR_ARG;
    if (asr::rnnt_lds_bytes(h->d.L, h->d.Hp, h->d.J, asr::RB_LDS_SMALL) > asr::RT_LDS_MAX) return ASR_ERR_UNSUPPORTED;
    const asr::LmTables *host, *dev;
    if (!h->d_blob || !asr_internal_lm_tables(z->lm, &host, &dev)) return ASR_ERR_STATE;
    if (!z->d_tok) {   // once per handle
        void* d = nullptr;
        ASR_HIP_TRY(hipMalloc(&d, z->tok.size() * sizeof(int32_t)));
        const hipError_t e = hipMemcpy(d, z->tok.data(), z->tok.size() * sizeof(int32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            asr_internal_set_error("hipMemcpy (tok_of_label)", hipGetErrorString(e), __FILE__, __LINE__);
            (void)hipFree(d);
            return ASR_ERR_HIP;
        }
        z->d_tok = (int32_t*)d;
    }
    return asr::rnnt_beam_launch(h, z, dev, d_enc, d_lengths, T, B, K, nbest, max_out, d_tokens, d_timesteps, d_len, d_am,
                                 d_total, d_lm_log10, d_ntok, d_nhyp, d_work, s);
}

int asr_rnnt_beam_lm_host(const asr_rnnt_lm_t* z, const float* h_enc, const int32_t* h_lengths, int T, int B, int K,
                          int nbest, int max_out, int32_t* h_tokens, int32_t* h_timesteps, int32_t* h_len,
                          double* h_total, double* h_am, double* h_lm_log10, int32_t* h_ntok, int32_t* h_nhyp,
                          double* h_margin) {
    if (!z) return ASR_ERR_ARG;
    if (int rc = asr::rnnt_beam_check(z->model, h_enc, T, B, K, nbest, max_out, h_tokens, h_timesteps, h_len, h_total,
                                      h_nhyp))
        return rc;
    return asr::rnnt_beam_host_run(z->model, z, h_enc, h_lengths, T, B, K, nbest, max_out, h_tokens, h_timesteps, h_len,
                                   h_total, h_am, h_lm_log10, h_ntok, h_nhyp, h_margin);
}

}  // extern "C"
