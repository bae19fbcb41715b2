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
#include "rnnt_common.h"

#include <cstdint>
#include <new>

namespace asr {

constexpr int RB_LDS_SMALL = 8192;   // the beam state, the candidates and the wave partials
constexpr int RB_MAX_K = 16;

static long rnnt_beam_lds_bytes(int L, int Hp, int J) {
    return ((long)2 * L * (Hp + 4) + (J + 4)) * RT_ROWS * 4 + RB_LDS_SMALL;
}

struct BeamArgs {
    const float* f;          // [T*B][J]
    const float* embw;       // [V][4Hp] = Emb.W_ih of layer 0
    const float* wih1;       // [Hp][4Hp], layer 1 (L = 2)
    const float* whh[2];
    const float* bih[2];
    const float* bhh[2];
    const float* wpred;
    const float* bpred;
    const float* wout;
    const float* bout;
    const int32_t* lengths;
    int32_t* tokens;         // [B][nbest][max_out]
    int32_t* timesteps;
    int32_t* len;            // [B][nbest]
    double* score;
    int32_t* nhyp;           // [B]
    float* slices;           // per workgroup: c [2][L][16][Hp], g [16][J], logits [16][V]
    int4* nodes;             // [B][T*K + 1]: (parent, token, t, length); node 0 is the empty sequence
    int T, B, Hp, J, V, L, blank, act, K, lgR, nbest, max_out, max_iters;
};

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

__global__ __launch_bounds__(64 * RT_WAVES) void rnnt_beam_kernel(const BeamArgs p) {
    extern __shared__ __attribute__((aligned(16))) float rb_lds[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int Hp = p.Hp, J = p.J, V = p.V, L = p.L, B = p.B, K = p.K;
    const int H4 = 4 * Hp, LDH = Hp + 4, LDJ = J + 4;
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
    auto hb = [&](int buf, int l) { return hbuf + ((size_t)buf * L + l) * RT_ROWS * LDH; };
    // this workgroup's slice: c [2][L][16][Hp], g [16][J], logits [16][V]
    const size_t csz = (size_t)L * RT_ROWS * Hp;
    float* const cw = p.slices + (size_t)blockIdx.x * (2 * csz + (size_t)RT_ROWS * J + (size_t)RT_ROWS * V);
    float* const gw = cw + 2 * csz;
    float* const lg = gw + (size_t)RT_ROWS * J;
    const size_t npu = (size_t)p.T * K + 1;      // nodes per utterance

    if (tid < RT_ROWS) {
        row_score[tid] = 0.0;
        row_hash[tid] = 0x243f6a8885a308d3ull;
        row_node[tid] = 0;
        row_len[tid] = 0;
        row_prow[tid] = tid;
        row_tok[tid] = p.blank;    // the start step on Emb[blank], every row
        const int b = b0 + tid;
        utt_len[tid] = (tid < U && b < B) ? (p.lengths ? min(max(p.lengths[b], 0), p.T) : p.T) : 0;
        utt_live[tid] = 1;
        utt_nodes[tid] = 1;
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
            // Predictor step by parent row; rows without a token copy their parent's h and c.
            const float* cold_b = cw + (size_t)cur * csz;
            float* cnew_b = cw + (size_t)(cur ^ 1) * csz;
            const int prc = row_prow[c];
            for (int l = 0; l < L; l++) {
                const float* hold = hb(cur, l);
                float* hnew = hb(cur ^ 1, l);
                const float* Whh = p.whh[l];
                for (int jt = w; jt < (Hp >> 4); jt += RT_WAVES) {
                    const int n = 16 * jt + c;
                    const int col[4] = {n, Hp + n, 2 * Hp + n, 3 * Hp + n};
                    f32x4 acc[4], accx[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) acc[q] = accx[q] = f32x4{0.f, 0.f, 0.f, 0.f};
                    rt_mma<4>(hold + prc * LDH + 4 * g, Hp >> 4, Whh, H4, g, col, acc);
                    if (l > 0)   // x = the layer below's new h, already in the new rows' order
                        rt_mma<4>(hb(cur ^ 1, l - 1) + c * LDH + 4 * g, Hp >> 4, p.wih1, H4, g, col, accx);
                    float bias[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) bias[q] = p.bih[l][col[q]] + p.bhh[l][col[q]];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int row = 4 * g + j, pr = row_prow[row], tk = row_tok[row];
                        const bool em = tk >= 0;
                        float px[4];
                        if (l == 0) {
                            const float* e = p.embw + (unsigned)(max(tk, 0) * H4);   // V * 4Hp <= INT_MAX
#pragma unroll
                            for (int q = 0; q < 4; q++) px[q] = e[col[q]];
                        } else {
#pragma unroll
                            for (int q = 0; q < 4; q++) px[q] = accx[q][j];
                        }
                        const float cold = cold_b[(unsigned)((l * RT_ROWS + pr) * Hp + n)];
                        const float zi = (px[0] + acc[0][j]) + bias[0], zf = (px[1] + acc[1][j]) + bias[1];
                        const float zg = (px[2] + acc[2][j]) + bias[2], zo = (px[3] + acc[3][j]) + bias[3];
                        const float ig = rt_sigmoid(zi), fg = rt_sigmoid(zf), gg = tanhf(zg), og = rt_sigmoid(zo);
                        const float cn = fg * cold + ig * gg;
                        const float hn = og * tanhf(cn);
                        cnew_b[(unsigned)((l * RT_ROWS + row) * Hp + n)] = em ? cn : cold;
                        hnew[row * LDH + n] = em ? hn : hold[pr * LDH + n];
                    }
                }
                __syncthreads();   // layer l's new h, before layer l + 1 and g read it
            }
            cur ^= 1;
            // g = h_top.W_pred + b_pred of every row
            const float* ht = hb(cur, L - 1) + c * LDH + 4 * g;
            const int nt = J >> 4;
            for (int base = 0; base < nt; base += 4 * RT_WAVES) {
                const int t0 = base + w;
                const int nv = t0 < nt ? min(4, (nt - 1 - t0) / RT_WAVES + 1) : 0;
                if (nv == 4) {
                    const int col[4] = {16 * t0 + c, 16 * (t0 + RT_WAVES) + c, 16 * (t0 + 2 * RT_WAVES) + c,
                                        16 * (t0 + 3 * RT_WAVES) + c};
                    f32x4 acc[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
                    rt_mma<4>(ht, Hp >> 4, p.wpred, J, g, col, acc);
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const float b = p.bpred[col[q]];
#pragma unroll
                        for (int j = 0; j < 4; j++) gw[(unsigned)((4 * g + j) * J + col[q])] = acc[q][j] + b;
                    }
                } else {
                    for (int q = 0; q < nv; q++) {
                        const int col[1] = {16 * (t0 + q * RT_WAVES) + c};
                        f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
                        rt_mma<1>(ht, Hp >> 4, p.wpred, J, g, col, acc);
                        const float b = p.bpred[col[0]];
#pragma unroll
                        for (int j = 0; j < 4; j++) gw[(unsigned)((4 * g + j) * J + col[0])] = acc[0][j] + b;
                    }
                }
            }
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
                    zbuf[row * LDJ + n] = p.act ? tanhf(x) : fmaxf(x, 0.f);
                }
            }
        }
        __syncthreads();

        // logit = z.W_out + b_out over the V column tiles, kept in the slice; columns >= V do not exist
        RtTop top[4];
#pragma unroll
        for (int j = 0; j < 4; j++) top[j] = RtTop{-INFINITY, 0.f, 0};   // no argmax here: every index is 0
        {
            const float* za = zbuf + c * LDJ + 4 * g;
            const int nt = (V + 15) >> 4;
            for (int base = 0; base < nt; base += 4 * RT_WAVES) {
                const int t0 = base + w;
                const int nv = t0 < nt ? min(4, (nt - 1 - t0) / RT_WAVES + 1) : 0;
                if (nv == 4) {
                    int n[4], col[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        n[q] = 16 * (t0 + q * RT_WAVES) + c;
                        col[q] = min(n[q], V - 1);
                    }
                    f32x4 acc[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
                    rt_mma<4>(za, J >> 4, p.wout, V, g, col, acc);
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        if (n[q] >= V) continue;
                        const float b = p.bout[n[q]];
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const float x = acc[q][j] + b;
                            rt_push(top[j], x, 0);
                            lg[(unsigned)(4 * g + j) * (unsigned)V + (unsigned)n[q]] = x;
                        }
                    }
                } else {
                    for (int q = 0; q < nv; q++) {
                        const int n = 16 * (t0 + q * RT_WAVES) + c;
                        const int col[1] = {min(n, V - 1)};
                        f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
                        rt_mma<1>(za, J >> 4, p.wout, V, g, col, acc);
                        if (n >= V) continue;
                        const float b = p.bout[n];
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const float x = acc[0][j] + b;
                            rt_push(top[j], x, 0);
                            lg[(unsigned)(4 * g + j) * (unsigned)V + (unsigned)n] = x;
                        }
                    }
                }
            }
        }
        // the 16 lanes of a row, then the waves in the order 0..7 (rnnt.hip's order)
#pragma unroll
        for (int j = 0; j < 4; j++) {
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) {
                RtTop o;
                o.m = __shfl_xor(top[j].m, d);
                o.s = __shfl_xor(top[j].s, d);
                o.i = 0;
                top[j] = rt_join(top[j], o);
            }
            if (c == 0) {
                red_m[w * RT_ROWS + 4 * g + j] = top[j].m;
                red_s[w * RT_ROWS + 4 * g + j] = top[j].s;
            }
        }
        __syncthreads();
        if (tid < RT_ROWS) {
            RtTop a{red_m[tid], red_s[tid], 0};
            for (int x = 1; x < RT_WAVES; x++) a = rt_join(a, RtTop{red_m[x * RT_ROWS + tid], red_s[x * RT_ROWS + tid], 0});
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
            double lsc = 0.0;
            int lv = -1;
            for (int r = 0; r < kc; r++) {
                double bs = 0.0;
                int bv = RT_NONE;
                for (int v = lane; v < V; v += 64) {
                    const double sc = s + (double)((lr[v] - m) - ls);
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
                    const bool bl = v == p.blank;
                    ent_score[e] = kept_sc[e];
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
                        const bool blank_wins = sj > sm || (sj == sm && j < m);
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
                        break;
                    }
                }
                int nl = 0;
                for (int j = 0; j < nk; j++) {
                    const int e = base + j;
                    if (ent_dead[e]) continue;
                    int rank = 0;
                    for (int m = 0; m < nk; m++)
                        rank += !ent_dead[base + m] && rb_before(ent_score[base + m], m, ent_score[e], j);
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
                    nl++;
                }
                for (int i = nl; i < R; i++) {
                    row_prow[base + i] = base + i;
                    row_tok[base + i] = -1;
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
    if (tid < RT_ROWS) {
        const int td = rb_here(tid);
        const int u = td >> lgR, j = td & (R - 1), b = b0 + u;
        if (b < B) {
            const int nh = min(utt_live[u], p.nbest);
            if (j == 0) p.nhyp[b] = nh;
            if (j < nh) {
                const int4* const nodes = p.nodes + (size_t)b * npu;
                const size_t o = (size_t)b * p.nbest + j;
                p.len[o] = row_len[td];
                p.score[o] = row_score[td];
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
    double score = 0.0;
    std::vector<double> h, c, g;
};
struct BeamCand {
    double score;
    int i, v;
    long pos;     // position in candidate order (of the earlier constituent after a merge)
    int ts_parent;  // merged and the token constituent won: the hypothesis whose timesteps it extends; else -1
    bool dead;
};

}  // namespace asr

extern "C" {

size_t asr_rnnt_beam_workspace_bytes(const asr_rnnt_t* h, int T, int B, int K) {
    if (!h || T <= 0 || B <= 0 || K < 1 || K > asr::RB_MAX_K || (long)T * B > INT_MAX || (long)T * K + 1 > INT_MAX)
        return 0;
    const size_t U = (size_t)asr::RT_ROWS >> asr::rb_log2_rows(K);
    const size_t tiles = ((size_t)B + U - 1) / U;
    // f [T*B][J]; per workgroup c [2][L][16][Hp], g [16][J], logits [16][V]; per utterance T*K + 1 nodes of 16 bytes
    return ((size_t)T * B * h->d.J + tiles * asr::RT_ROWS * ((size_t)2 * h->d.L * h->d.Hp + h->d.J + h->d.V)) *
               sizeof(float) +
           (size_t)B * ((size_t)T * K + 1) * sizeof(int4);
}

int asr_rnnt_beam(const asr_rnnt_t* h, const float* d_enc, const int32_t* d_lengths, int T, int B, int K, int nbest,
                  int max_out, int32_t* d_tokens, int32_t* d_timesteps, int32_t* d_len, double* d_score,
                  int32_t* d_nhyp, void* d_work, asr_stream_t s) {
    if (int rc = asr::rnnt_beam_check(h, d_enc, T, B, K, nbest, max_out, d_tokens, d_timesteps, d_len, d_score, d_nhyp))
        return rc;
    if (!d_work) return ASR_ERR_ARG;
    const asr_rnnt_desc& d = h->d;
    const long lds = asr::rnnt_beam_lds_bytes(d.L, d.Hp, d.J);
    if (lds > asr::RT_LDS_MAX) return ASR_ERR_UNSUPPORTED;
    if (!h->d_blob) return ASR_ERR_STATE;
    float* f = (float*)d_work;
    asr::GemmArgs g{};
    g.A = d_enc; g.B = h->d_wenc; g.b1 = h->d_benc; g.C = f;
    g.M = T * B; g.N = d.J; g.K = d.E;
    g.sam = d.E; g.sak = 1; g.sbk = d.J; g.sbn = 1; g.ldc = d.J;
    if (int rc = asr::gemm_launch(g, asr::EPI_BIAS, asr_stream(s))) return rc;
    const int lgR = asr::rb_log2_rows(K), U = asr::RT_ROWS >> lgR;
    const size_t tiles = ((size_t)B + U - 1) / U;
    asr::BeamArgs a{};
    a.f = f;
    a.embw = h->d_embw;
    a.wih1 = h->d_wih1;
    for (int l = 0; l < d.L; l++) {
        a.whh[l] = h->d_whh[l];
        a.bih[l] = h->d_bih[l];
        a.bhh[l] = h->d_bhh[l];
    }
    a.wpred = h->d_wpred; a.bpred = h->d_bpred; a.wout = h->d_wout; a.bout = h->d_bout;
    a.lengths = d_lengths;
    a.tokens = d_tokens; a.timesteps = d_timesteps; a.len = d_len; a.score = d_score; a.nhyp = d_nhyp;
    a.slices = f + (size_t)T * B * d.J;
    a.nodes = reinterpret_cast<int4*>(a.slices + tiles * asr::RT_ROWS * ((size_t)2 * d.L * d.Hp + d.J + d.V));
    a.T = T; a.B = B; a.Hp = d.Hp; a.J = d.J; a.V = d.V; a.L = d.L; a.blank = d.blank; a.act = d.act;
    a.K = K; a.lgR = lgR; a.nbest = nbest; a.max_out = max_out;
    a.max_iters = T;   // one joint evaluation per hypothesis and frame
    static AsrAttrOnce attr;
    if (int rc = attr.set((const void*)asr::rnnt_beam_kernel, asr::RT_LDS_MAX)) return rc;
    hipLaunchKernelGGL(asr::rnnt_beam_kernel, dim3((unsigned)tiles), dim3(64 * asr::RT_WAVES), (size_t)lds,
                       asr_stream(s), a);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

int asr_rnnt_beam_host(const asr_rnnt_t* h, const float* h_enc, const int32_t* h_lengths, int T, int B, int K,
                       int nbest, int max_out, int32_t* h_tokens, int32_t* h_timesteps, int32_t* h_len,
                       double* h_score, int32_t* h_nhyp, double* h_margin) {
    if (int rc = asr::rnnt_beam_check(h, h_enc, T, B, K, nbest, max_out, h_tokens, h_timesteps, h_len, h_score, h_nhyp))
        return rc;
    using asr::BeamCand;
    using asr::BeamHyp;
    const asr_rnnt_desc& d = h->d;
    const size_t LH = (size_t)d.L * d.Hp;
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
            const int len = h_lengths ? std::min(std::max(h_lengths[b], 0), T) : T;
            double margin = HUGE_VAL;
            for (int t = 0; t < len; t++) {
                m.enc_proj(h_enc + ((size_t)t * B + b) * d.E);
                cands.clear();
                for (int i = 0; i < (int)A.size(); i++) {
                    for (int j = 0; j < d.J; j++) {
                        const double v = m.f[j] + A[i].g[j];
                        m.z[j] = d.act == ASR_RNNT_ACT_TANH ? std::tanh(v) : (v > 0.0 ? v : 0.0);
                    }
                    asr::RnntHost::matvec(m.z.data(), h->wout.data(), d.J, d.V, logit.data());
                    double best = -HUGE_VAL;
                    for (int v = 0; v < d.V; v++) {
                        logit[v] += (double)h->bout[v];
                        if (logit[v] > best) best = logit[v];
                    }
                    double se = 0.0;
                    for (int v = 0; v < d.V; v++) se += std::exp(logit[v] - best);
                    const double lse = best + std::log(se);
                    for (int v = 0; v < d.V; v++)
                        cands.push_back(BeamCand{A[i].score + (logit[v] - lse), i, v, 0, -1, false});
                }
                const size_t nk = std::min((size_t)K, cands.size());
                const size_t ns = std::min(nk + 1, cands.size());   // one more, for the margin
                const long V = d.V;
                std::partial_sort(cands.begin(), cands.begin() + ns, cands.end(),
                                  [V](const BeamCand& x, const BeamCand& y) {
                                      return asr::rb_before(x.score, x.i * V + x.v, y.score, y.i * V + y.v);
                                  });
                if (ns > nk) margin = std::min(margin, cands[nk - 1].score - cands[nk].score);
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
                        margin = std::min(margin, std::fabs(sj - sx));
                        const bool blank_wins = sj > sx || (sj == sx && j < x);
                        const size_t keep = std::min(j, x), drop = std::max(j, x);
                        BeamCand e = kept[j];   // the blank constituent: its state, a copy
                        e.score = std::max(sj, sx) + std::log1p(std::exp(-std::fabs(sj - sx)));
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
                    return asr::rb_before(x.score, x.pos, y.score, y.pos);
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
                    }
                }
                A.swap(N);
            }
            for (size_t j = 0; j + 1 < A.size(); j++) margin = std::min(margin, A[j].score - A[j + 1].score);
            const int nh = (int)std::min(A.size(), (size_t)nbest);
            h_nhyp[b] = nh;
            for (int j = 0; j < nh; j++) {
                const size_t o = (size_t)b * nbest + j;
                h_len[o] = (int32_t)A[j].ys.size();
                h_score[o] = A[j].score;
                for (int x = 0; x < (int)A[j].ys.size() && x < max_out; x++) {
                    h_tokens[o * max_out + x] = A[j].ys[x];
                    h_timesteps[o * max_out + x] = A[j].ts[x];
                }
            }
            if (h_margin) h_margin[b] = margin;
        }
    } catch (const std::bad_alloc&) {
        return ASR_ERR_OOM;
    }
    return ASR_OK;
}

}  // extern "C"
