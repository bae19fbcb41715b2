// ============================================================================
// Edit distance, WER counts and n-best minimum-Bayes-risk rescoring on gfx950
// (the contract is in include/asr_amd.h).
//
// Cell.  One DP cell is one 32-bit word: the distance in the high half, the hits
// of the chosen alignment in the low half.  The other three counts follow from
// the cell's position: every path to (i, j) has H + S + D = i, H + S + I = j and
// S + D + I = distance, so I = distance - (i - H), D = I + i - j, S = i - H - D.
// Carrying the hits forward with the chosen predecessor (diagonal, then up, then
// left among equal minima) therefore carries all four counts.
//
// Kernel.  One wave per pair, the DP in registers: lane l owns the K contiguous
// hypothesis columns l*K+1 .. l*K+K (K = 1 .. 16 from the call's maximum
// hypothesis length) and the wave sweeps the reference as a skewed wavefront —
// at step s lane l works on reference row s - l + 1.  A step takes lane l-1's
// last cell of the same row (one shuffle), keeps the one received a step earlier
// as its diagonal, and passes the reference token up the lanes the same way; the
// tokens enter at lane 0 from a 64-token chunk read in one coalesced load.  No
// LDS, no workspace, no dependent load per row.
//
// ed_cell(), ed_counts(), mbr_weight() and mbr_lane_partial() are __host__
// __device__: the kernels and the host twins run the same code, so integers
// agree exactly and risks differ only through exp().
// ============================================================================
#include "asr_internal.h"

#include <algorithm>
#include <cmath>

namespace asr {

constexpr int ED_WAVES = 4;    // pairs per workgroup (waves are independent: no LDS, no barrier)
constexpr int MBR_WAVES = 4;   // waves of a risk workgroup (one group per workgroup)
constexpr unsigned ED_MAX_GRID_Y = 65535;

// D[i][j] from its three neighbours; `ne`: a_i != b_j.  Strict comparisons keep
// the preference diagonal, up, left among equal minima.
__host__ __device__ static inline uint32_t ed_cell(uint32_t diag, uint32_t up, uint32_t left, bool ne) {
    uint32_t best = diag + (ne ? 0x10000u : 1u);   // a substitution costs 1, a hit counts 1
    const uint32_t u = up + 0x10000u, l = left + 0x10000u;
    if ((u >> 16) < (best >> 16)) best = u;
    if ((l >> 16) < (best >> 16)) best = l;
    return best;
}

// (H, S, D, I) of the final cell of a pair of lengths la, lb.
__host__ __device__ static inline void ed_counts(uint32_t cell, int la, int lb, int32_t* ops) {
    const int dist = (int)(cell >> 16), h = (int)(cell & 0xFFFFu);
    const int ins = dist - (la - h);
    const int del = ins + la - lb;
    ops[0] = h;
    ops[1] = la - h - del;
    ops[2] = del;
    ops[3] = ins;
}

__host__ __device__ static inline int ed_clamp(const int32_t* len, long row, int max_len) {
    if (!len) return max_len;
    const int v = len[row];
    return v < 0 ? 0 : (v > max_len ? max_len : v);
}

// exp(w - m) with the edge cases of the contract; m is the group's maximum of
// the weights with NaN read as -inf.
__host__ __device__ static inline double mbr_clean(double w) { return w != w ? -__builtin_inf() : w; }
__host__ __device__ static inline double mbr_weight(double w, double m) {
    w = mbr_clean(w);
    if (m == -__builtin_inf()) return 1.0;
    if (m == __builtin_inf()) return w == m ? 1.0 : 0.0;
    return exp(w - m);
}

// Partial `lane` of the two sums of one row: j = lane, lane + 64, .. in
// increasing order from 0.0.  w == NULL: uniform weights.
__host__ __device__ static inline void mbr_lane_partial(const double* __restrict__ w, double m,
                                                        const int32_t* __restrict__ drow, int n, int lane,
                                                        double* z, double* num) {
    double zz = 0.0, nn = 0.0;
    for (int j = lane; j < n; j += 64) {
        const double e = w ? mbr_weight(w[j], m) : 1.0;
        const double prod = e * (double)drow[j];
        zz += e;
        nn += prod;
    }
    *z = zz;
    *num = nn;
}

// Members of group g: rows [*start, *start + n); n = 0 for an empty or invalid group.
__host__ __device__ static inline int mbr_group(const int32_t* __restrict__ gs, long g, int N, int max_hyps,
                                                long* start) {
    const int lo = gs[g], hi = gs[g + 1];
    *start = lo;
    if (lo < 0 || hi > N || hi < lo) return 0;
    const int n = hi - lo;
    return n < max_hyps ? n : max_hyps;
}

// The final cell D[la][lb] of one pair, in every lane.  a, la, lb are wave-uniform.
template <int K>
__device__ static inline uint32_t ed_pair(const int32_t* __restrict__ a, int la, const int32_t* __restrict__ b,
                                          int lb, int lane) {
    if (la == 0 || lb == 0) return (uint32_t)(la + lb) << 16;   // all deletions or all insertions
    const int col0 = lane * K;
    int32_t bt[K];
    uint32_t row[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        bt[k] = col0 + k < lb ? b[col0 + k] : 0;
        row[k] = (uint32_t)(col0 + k + 1) << 16;   // D[0][j] = j
    }
    uint32_t dprev = (uint32_t)col0 << 16;         // D[i-1][col0], the diagonal of this lane's first column
    uint32_t last = 0;
    int32_t tok = 0, chunk = 0;
    const int nl = (lb + K - 1) / K;               // lanes that own a column
    const int nsteps = la + nl - 1;
    for (int s = 0; s < nsteps; s++) {
        if ((s & 63) == 0) chunk = s + lane < la ? a[s + lane] : 0;
        const uint32_t recv = (uint32_t)__shfl_up((int)last, 1);
        const int32_t tprev = __shfl_up(tok, 1);
        const int32_t t0 = __builtin_amdgcn_readlane(chunk, s & 63);
        tok = lane == 0 ? t0 : tprev;
        const int i = s - lane + 1;
        if (i >= 1 && i <= la) {
            uint32_t left = lane == 0 ? (uint32_t)i << 16 : recv;   // D[i][col0]
            uint32_t diag = dprev;
            dprev = left;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const uint32_t c = ed_cell(diag, row[k], left, tok != bt[k]);
                diag = row[k];
                row[k] = c;
                left = c;
            }
            last = left;
        }
    }
    const int fl = (lb - 1) / K, fk = (lb - 1) % K;
    uint32_t v = row[0];
#pragma unroll
    for (int k = 1; k < K; k++)
        if (fk == k) v = row[k];
    return (uint32_t)__shfl((int)v, fl);
}

struct EditArgs {
    const int32_t* ref;
    const int32_t* ref_len;
    const int32_t* hyp;
    const int32_t* hyp_len;
    const int32_t* ref_idx;
    const int32_t* hyp_idx;
    int32_t* dist;
    int32_t* ops;
    long ldr, ldh;
    int n_ref, max_ref_len, n_hyp, max_hyp_len, P;
};

template <int K>
__global__ __launch_bounds__(64 * ED_WAVES) void edit_distance_kernel(const EditArgs p) {
    const int lane = threadIdx.x & 63;
    const long n = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) + (long)blockIdx.x * ED_WAVES;
    if (n >= p.P) return;   // wave-uniform
    const long r = p.ref_idx ? (long)p.ref_idx[n] : n;
    const long h = p.hyp_idx ? (long)p.hyp_idx[n] : n;
    if (r < 0 || r >= p.n_ref || h < 0 || h >= p.n_hyp) {
        if (lane == 0 && p.dist) p.dist[n] = -1;
        if (lane < 4 && p.ops) p.ops[4 * n + lane] = -1;
        return;
    }
    const int la = __builtin_amdgcn_readfirstlane(ed_clamp(p.ref_len, r, p.max_ref_len));
    const int lb = __builtin_amdgcn_readfirstlane(ed_clamp(p.hyp_len, h, p.max_hyp_len));
    const uint32_t c = ed_pair<K>(p.ref + r * p.ldr, la, p.hyp + h * p.ldh, lb, lane);
    if (lane == 0) {
        if (p.dist) p.dist[n] = (int32_t)(c >> 16);
        if (p.ops) {
            int32_t o[4];
            ed_counts(c, la, lb, o);
            p.ops[4 * n + 0] = o[0];
            p.ops[4 * n + 1] = o[1];
            p.ops[4 * n + 2] = o[2];
            p.ops[4 * n + 3] = o[3];
        }
    }
}

struct MbrArgs {
    const int32_t* tokens;
    const int32_t* lengths;
    const int32_t* group_start;
    const double* weight;
    int32_t* dist;
    double* risk;
    int32_t* best;
    long ldt, ldm;
    int N, max_len, G, max_hyps;
};

// Unordered pairs (k <= j) of one group, one wave each: t = j (j + 1) / 2 + k.
// The distance is symmetric, so d(k, j) is stored at both places.
template <int K>
__global__ __launch_bounds__(64 * ED_WAVES) void mbr_pairs_kernel(const MbrArgs p) {
    const int lane = threadIdx.x & 63;
    const int t = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) + (int)blockIdx.x * ED_WAVES;
    int j = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    if (j * (j + 1) / 2 > t) j--;   // 8 t + 1 < 2^24 is exact, so the root is off by less than one
    else if ((j + 1) * (j + 2) / 2 <= t) j++;
    const int k = t - j * (j + 1) / 2;
    for (long g = blockIdx.y; g < p.G; g += gridDim.y) {
        long start;
        const int n = mbr_group(p.group_start, g, p.N, p.max_hyps, &start);
        if (j >= n || k < 0 || k > j) continue;   // wave-uniform
        int32_t* out_kj = p.dist + (start + k) * p.ldm + j;
        if (k == j) {
            if (lane == 0) *out_kj = 0;
            continue;
        }
        const int la = __builtin_amdgcn_readfirstlane(ed_clamp(p.lengths, start + k, p.max_len));
        const int lb = __builtin_amdgcn_readfirstlane(ed_clamp(p.lengths, start + j, p.max_len));
        const uint32_t c = ed_pair<K>(p.tokens + (start + k) * p.ldt, la, p.tokens + (start + j) * p.ldt, lb, lane);
        if (lane == 0) {
            *out_kj = (int32_t)(c >> 16);
            p.dist[(start + j) * p.ldm + k] = (int32_t)(c >> 16);
        }
    }
}

// One workgroup per group, one wave per row (rows w, w + MBR_WAVES, ..), lanes
// over j; the risks of the group meet in LDS for the argmin.
__global__ __launch_bounds__(64 * MBR_WAVES) void mbr_risk_kernel(const MbrArgs p) {
    __shared__ double risk_s[ASR_MBR_MAX_HYPS];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    {
        const long g = blockIdx.x;
        long start;
        const int n = mbr_group(p.group_start, g, p.N, p.max_hyps, &start);
        if (n == 0) {   // workgroup-uniform
            if (threadIdx.x == 0 && p.best) p.best[g] = -1;
            return;
        }
        const double* w = p.weight ? p.weight + start : nullptr;
        double m = -__builtin_inf();
        if (w) {
            for (int j = lane; j < n; j += 64) m = fmax(m, mbr_clean(w[j]));
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) m = fmax(m, __shfl_xor(m, off));
        }
        for (int k = wave; k < n; k += MBR_WAVES) {
            double z, num;
            mbr_lane_partial(w, m, p.dist + (start + k) * p.ldm, n, lane, &z, &num);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                z += __shfl_down(z, off);
                num += __shfl_down(num, off);
            }
            if (lane == 0) {
                const double r = num / z;
                risk_s[k] = r;
                if (p.risk) p.risk[start + k] = r;
            }
        }
        __syncthreads();
        if (wave == 0 && p.best) {
            double br = __builtin_inf();
            int bk = ASR_MBR_MAX_HYPS;
            for (int k = lane; k < n; k += 64) {
                const double r = risk_s[k];
                if (r < br) {   // k increases: the lowest row wins a tie
                    br = r;
                    bk = k;
                }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const double orr = __shfl_xor(br, off);
                const int ok = __shfl_xor(bk, off);
                if (orr < br || (orr == br && ok < bk)) {
                    br = orr;
                    bk = ok;
                }
            }
            if (lane == 0) p.best[g] = bk;
        }
    }
}

// ------------------------------------------------------------------ host twins
// Two rows of the same cells, one thread.
static uint32_t ed_pair_host(const int32_t* a, int la, const int32_t* b, int lb) {
    uint32_t row[ASR_EDIT_MAX_LEN + 1];
    for (int j = 0; j <= lb; j++) row[j] = (uint32_t)j << 16;
    for (int i = 1; i <= la; i++) {
        uint32_t diag = row[0];
        row[0] = (uint32_t)i << 16;
        const int32_t ai = a[i - 1];
        for (int j = 1; j <= lb; j++) {
            const uint32_t c = ed_cell(diag, row[j], row[j - 1], ai != b[j - 1]);
            diag = row[j];
            row[j] = c;
        }
    }
    return row[lb];
}

static int ed_check(const int32_t* ref, long ldr, int n_ref, int max_ref_len, const int32_t* hyp, long ldh, int n_hyp,
                    int max_hyp_len, const int32_t* ref_idx, const int32_t* hyp_idx, int P, const int32_t* dist,
                    const int32_t* ops) {
    if (!ref || !hyp) return ASR_ERR_ARG;
    if (P <= 0 || n_ref <= 0 || n_hyp <= 0) return ASR_ERR_ARG;
    if (ldr < (long)max_ref_len || ldh < (long)max_hyp_len) return ASR_ERR_ARG;
    if (!dist && !ops) return ASR_ERR_ARG;
    if ((!ref_idx && P > n_ref) || (!hyp_idx && P > n_hyp)) return ASR_ERR_ARG;
    if (max_ref_len < 0 || max_ref_len > ASR_EDIT_MAX_LEN || max_hyp_len < 0 || max_hyp_len > ASR_EDIT_MAX_LEN)
        return ASR_ERR_UNSUPPORTED;
    return ASR_OK;
}

static int mbr_check(const int32_t* tokens, long ldt, int N, int max_len, const int32_t* group_start, int G,
                     int max_hyps, const int32_t* dist, long ldm, const double* risk, const int32_t* best) {
    if (!tokens || !group_start || !dist) return ASR_ERR_ARG;
    if (N <= 0 || G <= 0 || max_hyps <= 0) return ASR_ERR_ARG;
    if (ldt < (long)max_len || ldm < (long)max_hyps) return ASR_ERR_ARG;
    if (!risk && !best) return ASR_ERR_ARG;
    if (max_len < 0 || max_len > ASR_EDIT_MAX_LEN || max_hyps > ASR_MBR_MAX_HYPS) return ASR_ERR_UNSUPPORTED;
    return ASR_OK;
}

// K = columns per lane: the smallest of 1, 2, .., 16 with 64 K >= max_hyp_len.
static int ed_k(int max_hyp_len) {
    int k = 1;
    while (64 * k < max_hyp_len) k *= 2;
    return k;
}

}  // namespace asr

extern "C" {

int asr_edit_distance_host(const int32_t* h_ref, long ldr, const int32_t* h_ref_len, int n_ref, int max_ref_len,
                           const int32_t* h_hyp, long ldh, const int32_t* h_hyp_len, int n_hyp, int max_hyp_len,
                           const int32_t* h_ref_idx, const int32_t* h_hyp_idx, int P, int32_t* h_dist,
                           int32_t* h_ops) {
    const int rc = asr::ed_check(h_ref, ldr, n_ref, max_ref_len, h_hyp, ldh, n_hyp, max_hyp_len, h_ref_idx, h_hyp_idx,
                                 P, h_dist, h_ops);
    if (rc != ASR_OK) return rc;
    for (long n = 0; n < P; n++) {
        const long r = h_ref_idx ? (long)h_ref_idx[n] : n;
        const long h = h_hyp_idx ? (long)h_hyp_idx[n] : n;
        if (r < 0 || r >= n_ref || h < 0 || h >= n_hyp) {
            if (h_dist) h_dist[n] = -1;
            if (h_ops)
                for (int q = 0; q < 4; q++) h_ops[4 * n + q] = -1;
            continue;
        }
        const int la = asr::ed_clamp(h_ref_len, r, max_ref_len);
        const int lb = asr::ed_clamp(h_hyp_len, h, max_hyp_len);
        const uint32_t c = asr::ed_pair_host(h_ref + r * ldr, la, h_hyp + h * ldh, lb);
        if (h_dist) h_dist[n] = (int32_t)(c >> 16);
        if (h_ops) asr::ed_counts(c, la, lb, h_ops + 4 * n);
    }
    return ASR_OK;
}

int asr_edit_distance(const int32_t* d_ref, long ldr, const int32_t* d_ref_len, int n_ref, int max_ref_len,
                      const int32_t* d_hyp, long ldh, const int32_t* d_hyp_len, int n_hyp, int max_hyp_len,
                      const int32_t* d_ref_idx, const int32_t* d_hyp_idx, int P, int32_t* d_dist, int32_t* d_ops,
                      asr_stream_t s) {
    const int rc = asr::ed_check(d_ref, ldr, n_ref, max_ref_len, d_hyp, ldh, n_hyp, max_hyp_len, d_ref_idx, d_hyp_idx,
                                 P, d_dist, d_ops);
    if (rc != ASR_OK) return rc;
    asr::EditArgs a;
    a.ref = d_ref;
    a.ref_len = d_ref_len;
    a.hyp = d_hyp;
    a.hyp_len = d_hyp_len;
    a.ref_idx = d_ref_idx;
    a.hyp_idx = d_hyp_idx;
    a.dist = d_dist;
    a.ops = d_ops;
    a.ldr = ldr;
    a.ldh = ldh;
    a.n_ref = n_ref;
    a.max_ref_len = max_ref_len;
    a.n_hyp = n_hyp;
    a.max_hyp_len = max_hyp_len;
    a.P = P;
    const dim3 grid((unsigned)(((long)P + asr::ED_WAVES - 1) / asr::ED_WAVES)), block(64 * asr::ED_WAVES);
    hipStream_t st = asr_stream(s);
    switch (asr::ed_k(max_hyp_len)) {
        case 1: asr::edit_distance_kernel<1><<<grid, block, 0, st>>>(a); break;
        case 2: asr::edit_distance_kernel<2><<<grid, block, 0, st>>>(a); break;
        case 4: asr::edit_distance_kernel<4><<<grid, block, 0, st>>>(a); break;
        case 8: asr::edit_distance_kernel<8><<<grid, block, 0, st>>>(a); break;
        default: asr::edit_distance_kernel<16><<<grid, block, 0, st>>>(a); break;
    }
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

int asr_nbest_mbr_host(const int32_t* h_tokens, long ldt, const int32_t* h_lengths, int N, int max_len,
                       const int32_t* h_group_start, int G, int max_hyps, const double* h_weight, int32_t* h_dist,
                       long ldm, double* h_risk, int32_t* h_best) {
    const int rc = asr::mbr_check(h_tokens, ldt, N, max_len, h_group_start, G, max_hyps, h_dist, ldm, h_risk, h_best);
    if (rc != ASR_OK) return rc;
    for (long g = 0; g < G; g++) {
        long start;
        const int n = asr::mbr_group(h_group_start, g, N, max_hyps, &start);
        if (n == 0) {
            if (h_best) h_best[g] = -1;
            continue;
        }
        for (int j = 0; j < n; j++) {
            const int lb = asr::ed_clamp(h_lengths, start + j, max_len);
            h_dist[(start + j) * ldm + j] = 0;
            for (int k = 0; k < j; k++) {
                const int la = asr::ed_clamp(h_lengths, start + k, max_len);
                const uint32_t c = asr::ed_pair_host(h_tokens + (start + k) * ldt, la, h_tokens + (start + j) * ldt, lb);
                h_dist[(start + k) * ldm + j] = (int32_t)(c >> 16);
                h_dist[(start + j) * ldm + k] = (int32_t)(c >> 16);
            }
        }
        const double* w = h_weight ? h_weight + start : nullptr;
        double m = -__builtin_inf();
        if (w)
            for (int j = 0; j < n; j++) m = std::fmax(m, asr::mbr_clean(w[j]));
        double br = __builtin_inf();
        int bk = -1;
        for (int k = 0; k < n; k++) {
            double z[64], num[64];
            for (int l = 0; l < 64; l++) asr::mbr_lane_partial(w, m, h_dist + (start + k) * ldm, n, l, &z[l], &num[l]);
            for (int off = 32; off >= 1; off >>= 1)   // the kernel's reduction tree
                for (int l = 0; l < off; l++) {
                    z[l] += z[l + off];
                    num[l] += num[l + off];
                }
            const double r = num[0] / z[0];
            if (h_risk) h_risk[start + k] = r;
            if (r < br) {
                br = r;
                bk = k;
            }
        }
        if (h_best) h_best[g] = bk;
    }
    return ASR_OK;
}

int asr_nbest_mbr(const int32_t* d_tokens, long ldt, const int32_t* d_lengths, int N, int max_len,
                  const int32_t* d_group_start, int G, int max_hyps, const double* d_weight, int32_t* d_dist, long ldm,
                  double* d_risk, int32_t* d_best, asr_stream_t s) {
    const int rc = asr::mbr_check(d_tokens, ldt, N, max_len, d_group_start, G, max_hyps, d_dist, ldm, d_risk, d_best);
    if (rc != ASR_OK) return rc;
    asr::MbrArgs a;
    a.tokens = d_tokens;
    a.lengths = d_lengths;
    a.group_start = d_group_start;
    a.weight = d_weight;
    a.dist = d_dist;
    a.risk = d_risk;
    a.best = d_best;
    a.ldt = ldt;
    a.ldm = ldm;
    a.N = N;
    a.max_len = max_len;
    a.G = G;
    a.max_hyps = max_hyps;
    const unsigned gy = (unsigned)std::min<long>(G, asr::ED_MAX_GRID_Y);
    const int pairs = max_hyps * (max_hyps + 1) / 2;
    const dim3 grid((unsigned)((pairs + asr::ED_WAVES - 1) / asr::ED_WAVES), gy), block(64 * asr::ED_WAVES);
    hipStream_t st = asr_stream(s);
    switch (asr::ed_k(max_len)) {
        case 1: asr::mbr_pairs_kernel<1><<<grid, block, 0, st>>>(a); break;
        case 2: asr::mbr_pairs_kernel<2><<<grid, block, 0, st>>>(a); break;
        case 4: asr::mbr_pairs_kernel<4><<<grid, block, 0, st>>>(a); break;
        case 8: asr::mbr_pairs_kernel<8><<<grid, block, 0, st>>>(a); break;
        default: asr::mbr_pairs_kernel<16><<<grid, block, 0, st>>>(a); break;
    }
    ASR_LAUNCH_TRY();
    asr::mbr_risk_kernel<<<dim3((unsigned)G), dim3(64 * asr::MBR_WAVES), 0, st>>>(a);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

}  // extern "C"
