// RNN-T lattice scoring and forced alignment of GIVEN transcripts:
// asr_rnnt_align_workspace_bytes / asr_rnnt_align / asr_rnnt_align_host
// (the definition is in include/asr_amd.h).
//
// Device form, four stages on one stream:
//   1. f = enc.W_enc + b_enc for all frames: one gemm_launch, as the decoders.
//   2. The predictor, teacher-forced over the N targets: rnnt_align_prep_kernel
//      gathers the layer-0 input projections [U+1][N][4Hp] from the Emb.W_ih
//      table of asr_rnnt_upload (the start row, then one row per label) and
//      writes the lengths U_n + 1; the library's gated recurrence
//      (asr_lstm_recur_fwd, asr_lstm_fwd for a second layer) runs them with
//      h0 = c0 = 0; one gemm_launch makes g [(U+1)*N][J].
//   3. rnnt_joint_kernel, the hot path.  The rows of a workgroup are 16 * NRT
//      consecutive lattice nodes r = t * (U_n + 1) + u of ONE target (NRT <= 3
//      row tiles, the most whose z fits in LDS: 3 up to J = 816).
//      z = act(f_t + g_u) is formed into LDS from one f row and one g row; the
//      8 waves split the 16-column tiles of W_out (tile j belongs to wave j % 8)
//      and stream them from L2 through rt_mma's register ring, each fragment
//      feeding NRT MFMAs.  Every row keeps a running (max, sum-exp) (rt_push,
//      rt_join; columns >= V never enter), the lanes that own the blank column
//      and the row's label column keep those two logits, and two floats per
//      node leave the kernel.  Workgroups past a target's len * (U + 1) nodes
//      and those of infeasible targets leave at once (workgroup-uniform).  The
//      tile-to-wave map and the k order are fixed and MFMA rows are
//      independent, so a node's bits depend on the model's shape only.
//   4. rnnt_lattice_kernel: one wave per target, alpha and the Viterbi values in
//      fp64, lane l owns the KU = 1, 2 or 4 contiguous u in [l*KU, l*KU + KU).
//      Step d takes alpha_{d-1} to alpha_d: a frame under ONE_PER_FRAME, an
//      anti-diagonal t + u = d under STANDARD (state u then sits at frame
//      d - u).  Both have the same shape: every state forms its blank and its
//      label candidate, the label candidate moves one state up (one shuffle
//      across lanes per recurrence and step), lse or max joins the two.  The
//      node values of step d + 1 are requested before step d is computed.
//      Back-pointers are one bit per node, one byte per lane and step; the
//      traceback is the tail of the same kernel, 64 steps per memory round trip
//      as in ctc_align.hip.
// No workgroup waits on another; every loop is bounded by T, U or V.
#include "ctc_lse.h"
#include "rnnt_common.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <new>
#include <vector>

namespace asr {

constexpr int RA_MAX_U = 255;        // max_target_len: U + 1 <= 256 states, 4 per lane
constexpr int RA_WAVES = RT_WAVES;   // waves of the joint kernel
constexpr int RA_MAX_RT = 3;         // row tiles of 16 nodes per workgroup, at most (4 spill: 256 VGPRs)
constexpr long RA_LSTM_OOB = 0x7ff00000L;   // asr_lstm_recur_fwd: one frame of P per buffer resource

// LDS bytes of the joint kernel with nrt row tiles: z [16 nrt][J + 4], then per
// row the blank logit, the label logit, the label and the 8 waves' (max, sum).
static long ra_lds_bytes(int nrt, int J) { return (long)16 * nrt * ((J + 4) + 3 + 2 * RA_WAVES) * 4; }
static int ra_row_tiles(int J) {
    for (int nrt = RA_MAX_RT; nrt > 1; nrt--)
        if (ra_lds_bytes(nrt, J) <= RT_LDS_MAX) return nrt;
    return 1;
}
static size_t ra_up4(size_t n) { return (n + 3) & ~(size_t)3; }

// The workspace, in this order (every part a multiple of 16 bytes).
struct RaLayout {
    size_t f, p, hid, g, lpb, lpy, meta, bp, total;   // byte offsets
};
static RaLayout ra_layout(const asr_rnnt_desc& d, int T, int B, int N, int mtl) {
    const size_t U1 = (size_t)mtl + 1, NU = (size_t)N * U1;
    RaLayout o{};
    size_t at = 0;
    o.f = at;    at += (size_t)T * B * d.J * 4;
    o.p = at;    at += (NU * 4 * d.Hp + (size_t)N * d.Hp) * 4;   // asr_lstm_workspace_bytes(U1, N, Hp)
    o.hid = at;  at += (size_t)d.L * NU * d.Hp * 4;
    o.g = at;    at += NU * d.J * 4;
    o.lpb = at;  at += ra_up4((size_t)N * T * U1) * 4;
    o.lpy = at;  at += ra_up4((size_t)N * T * U1) * 4;
    o.meta = at; at += ra_up4((size_t)2 * N) * 4;                // U_n + 1 [N], feasible [N]
    o.bp = at;   at += (size_t)N * ((size_t)T + U1) * 64;
    o.total = at;
    return o;
}

struct RaArgs {
    const float* f;      // [T*B][J]
    const float* g;      // [(mtl+1)*N][J], row u * N + n
    const float* embw;   // [V][4Hp]
    float* P;            // [(mtl+1)*N][4Hp]
    const float* wout;
    const float* bout;
    const int32_t* lengths;
    const int32_t* targets;
    long ldt;
    const int32_t* target_lengths;
    const int32_t* utt;
    int32_t* lens1;      // [N]: U_n + 1
    int32_t* ok;         // [N]: the target is feasible
    float* lpb;          // [N][T*(mtl+1)], node t * (U_n + 1) + u
    float* lpy;
    unsigned char* bp;   // [N][T + mtl + 1][64]
    double* score;
    double* vscore;
    int32_t* frames;
    int T, B, N, mtl, Hp, J, V, blank, act, topology, tiles;
};

// Target n: its clamped length U, its utterance b (-1: outside [0, B)) and that utterance's clamped length.
__device__ __forceinline__ void ra_target(const RaArgs& p, int n, int& U, int& b, int& len) {
    U = min(max(p.target_lengths[n], 0), p.mtl);
    b = p.utt ? p.utt[n] : n;
    if (b < 0 || b >= p.B) b = -1;
    len = 0;
    if (b >= 0) len = p.lengths ? min(max(p.lengths[b], 0), p.T) : p.T;
}

// One workgroup per target: the feasibility flag, the length U + 1 and the
// layer-0 input projections (Emb.W_ih rows: the start row, then one per label;
// rows past U repeat the start row and are never used).
__global__ __launch_bounds__(256) void rnnt_align_prep_kernel(const RaArgs p) {
    const int n = blockIdx.x, tid = threadIdx.x;
    int U, b, len;
    ra_target(p, n, U, b, len);
    const int32_t* tgt = p.targets + (long)n * p.ldt;
    int bad = 0;
    for (int i = tid; i < U; i += 256) {
        const int y = tgt[i];
        bad |= (y < 0 || y >= p.V || y == p.blank);
    }
    bad = __syncthreads_or(bad);
    if (tid == 0) {
        p.lens1[n] = U + 1;
        p.ok[n] = !(bad || b < 0 || (len == 0 && U > 0) || (p.topology == ASR_RNNT_LATTICE_ONE_PER_FRAME && U > len));
    }
    const int q4 = p.Hp;   // float4s of a row of 4Hp floats
    for (int x = tid; x < (p.mtl + 1) * q4; x += 256) {
        const int u = x / q4, k = x - u * q4;
        int tok = p.blank;
        if (u >= 1 && u <= U && !bad) tok = tgt[u - 1];
        reinterpret_cast<float4*>(p.P + ((size_t)u * p.N + n) * 4 * p.Hp)[k] =
            reinterpret_cast<const float4*>(p.embw + (size_t)tok * 4 * p.Hp)[k];
    }
}

template <int NRT>
__global__ __launch_bounds__(64 * RA_WAVES) void rnnt_joint_kernel(const RaArgs p) {
    extern __shared__ __attribute__((aligned(16))) float ra_lds[];
    constexpr int R = 16 * NRT;
    const int n = blockIdx.x / p.tiles, tile = blockIdx.x - n * p.tiles;
    if (!p.ok[n]) return;
    int U, b, len;
    ra_target(p, n, U, b, len);
    const int U1 = U + 1, cnt = len * U1, r0 = tile * R;
    if (r0 >= cnt) return;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int J = p.J, V = p.V, LDJ = J + 4;
    float* const zbuf = ra_lds;                                // [R][LDJ]
    float* const sb = zbuf + (size_t)R * LDJ;                  // [R] the blank logit
    float* const sy = sb + R;                                  // [R] the label logit
    int* const rlab = reinterpret_cast<int*>(sy + R);          // [R] the row's label, -1: none
    float* const red_m = reinterpret_cast<float*>(rlab + R);   // [8][R]
    float* const red_s = red_m + RA_WAVES * R;
    const int32_t* tgt = p.targets + (long)n * p.ldt;

    // z = act(f_t + g_u); rows past the target's last node repeat it and are not stored
    {
        const int j4n = J >> 2;
        for (int x = tid; x < R * j4n; x += 64 * RA_WAVES) {
            const int row = x / j4n, j4 = x - row * j4n;
            const int r = min(r0 + row, cnt - 1), t = r / U1, u = r - t * U1;
            const float4 fv = reinterpret_cast<const float4*>(p.f + ((size_t)t * p.B + b) * J)[j4];
            const float4 gv = reinterpret_cast<const float4*>(p.g + ((size_t)u * p.N + n) * J)[j4];
            float4 z{fv.x + gv.x, fv.y + gv.y, fv.z + gv.z, fv.w + gv.w};
            if (p.act) z = float4{tanhf(z.x), tanhf(z.y), tanhf(z.z), tanhf(z.w)};
            else z = float4{fmaxf(z.x, 0.f), fmaxf(z.y, 0.f), fmaxf(z.z, 0.f), fmaxf(z.w, 0.f)};
            *reinterpret_cast<float4*>(zbuf + (size_t)row * LDJ + 4 * j4) = z;
        }
        if (tid < R) {
            const int r = min(r0 + tid, cnt - 1), u = r % U1;
            rlab[tid] = u < U ? tgt[u] : -1;
        }
    }
    __syncthreads();

    int lab[NRT][4];
    RtTop top[NRT][4];
#pragma unroll
    for (int rt = 0; rt < NRT; rt++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            lab[rt][j] = rlab[16 * rt + 4 * g + j];
            top[rt][j] = RtTop{-INFINITY, 0.f, RT_NONE};
        }
    // logit = z.W_out + b_out over the V column tiles; columns >= V do not exist.  The schedule is rt_sweep's and
    // the reduction below rt_row_partial / rt_row_total's, written out: through the shared functions this kernel
    // measured 0.3 to 0.9 % slower in three jobs.  The tile-to-wave map and both orders must stay
    // theirs.
    {
        const float* za = zbuf + (size_t)c * LDJ + 4 * g;
        const int nt = (V + 15) >> 4;
        auto take = [&](int rt, int nn, const f32x4& a, float bias) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float x = a[j] + bias;
                rt_push(top[rt][j], x, nn);
                if (nn == p.blank) sb[16 * rt + 4 * g + j] = x;
                if (nn == lab[rt][j]) sy[16 * rt + 4 * g + j] = x;
            }
        };
        for (int base = 0; base < nt; base += 4 * RA_WAVES) {
            const int t0 = base + w;
            const int nv = t0 < nt ? min(4, (nt - 1 - t0) / RA_WAVES + 1) : 0;
            if (nv == 4) {
                int nn[4], col[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    nn[q] = 16 * (t0 + q * RA_WAVES) + c;
                    col[q] = min(nn[q], V - 1);
                }
                f32x4 acc[NRT][4];
#pragma unroll
                for (int rt = 0; rt < NRT; rt++)
#pragma unroll
                    for (int q = 0; q < 4; q++) acc[rt][q] = f32x4{0.f, 0.f, 0.f, 0.f};
                rt_mma<NRT, 4>(za, 16 * LDJ, J >> 4, p.wout, V, g, col, acc);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (nn[q] >= V) continue;
                    const float bias = p.bout[nn[q]];
#pragma unroll
                    for (int rt = 0; rt < NRT; rt++) take(rt, nn[q], acc[rt][q], bias);
                }
            } else {
                for (int q = 0; q < nv; q++) {
                    const int nn = 16 * (t0 + q * RA_WAVES) + c;
                    const int col[1] = {min(nn, V - 1)};
                    f32x4 acc[NRT][1];
#pragma unroll
                    for (int rt = 0; rt < NRT; rt++) acc[rt][0] = f32x4{0.f, 0.f, 0.f, 0.f};
                    rt_mma<NRT, 1>(za, 16 * LDJ, J >> 4, p.wout, V, g, col, acc);
                    if (nn >= V) continue;
                    const float bias = p.bout[nn];
#pragma unroll
                    for (int rt = 0; rt < NRT; rt++) take(rt, nn, acc[rt][0], bias);
                }
            }
        }
    }
    // the 16 lanes of a row, then the waves in the order 0..7
#pragma unroll
    for (int rt = 0; rt < NRT; rt++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) {
                RtTop o;
                o.m = __shfl_xor(top[rt][j].m, d);
                o.s = __shfl_xor(top[rt][j].s, d);
                o.i = __shfl_xor(top[rt][j].i, d);
                top[rt][j] = rt_join(top[rt][j], o);
            }
            if (c == 0) {
                red_m[w * R + 16 * rt + 4 * g + j] = top[rt][j].m;
                red_s[w * R + 16 * rt + 4 * g + j] = top[rt][j].s;
            }
        }
    __syncthreads();
    if (tid < R && r0 + tid < cnt) {
        const int row = tid, r = r0 + row, u = r % U1;
        RtTop a{red_m[row], red_s[row], 0};
        for (int x = 1; x < RA_WAVES; x++) a = rt_join(a, RtTop{red_m[x * R + row], red_s[x * R + row], 0});
        const float lse = a.m + logf(a.s);
        const size_t o = (size_t)n * p.T * (p.mtl + 1) + r;
        p.lpb[o] = sb[row] - lse;
        if (u < U) p.lpy[o] = sy[row] - lse;
    }
}

// Value of state u (wave-uniform) from the lane that owns it.
template <int KU>
__device__ __forceinline__ double ra_fetch(const double (&x)[KU], int u) {
    const int j = u % KU;
    double m = x[0];
#pragma unroll
    for (int i = 1; i < KU; i++) m = (j == i) ? x[i] : m;
    return __shfl(m, u / KU);
}

template <int KU>
__global__ __launch_bounds__(64) void rnnt_lattice_kernel(const RaArgs p) {
    constexpr int TBC = 64;   // steps of back-pointer rows per traceback round trip
    const int n = blockIdx.x, lane = threadIdx.x;
    const double NINF = -INFINITY;
    const bool fwd = p.score != nullptr, vit = p.vscore != nullptr || p.frames != nullptr;
    const bool topo1 = p.topology == ASR_RNNT_LATTICE_ONE_PER_FRAME;
    int U, b, len;
    ra_target(p, n, U, b, len);
    const bool feasible = p.ok[n] != 0;
    const int U1 = U + 1;
    const int D = !feasible || len == 0 ? 0 : (topo1 ? len : len - 1 + U);   // steps
    int32_t* frames = p.frames ? p.frames + (long)n * p.ldt : nullptr;
    unsigned char* const bprow = p.bp + (size_t)n * ((size_t)p.T + p.mtl + 1) * 64 + lane;

    double score = NINF, vscore = NINF;
    if (feasible && len == 0) {
        score = vscore = 0.0;   // U == 0: the empty alignment
    } else if (feasible) {
        const float* lpb = p.lpb + (size_t)n * p.T * (p.mtl + 1);
        const float* lpy = p.lpy + (size_t)n * p.T * (p.mtl + 1);
        double a[KU], v[KU];
#pragma unroll
        for (int j = 0; j < KU; j++) a[j] = v[j] = (lane == 0 && j == 0) ? 0.0 : NINF;
        // step d: state u stands at frame tj = d - 1 (one per frame) or d - 1 - u (anti-diagonal)
        float nb[KU], ny[KU];
        auto request = [&](int d) {
#pragma unroll
            for (int j = 0; j < KU; j++) {
                const int u = lane * KU + j, tj = topo1 ? d - 1 : d - 1 - u;
                const bool in = tj >= 0 && tj < len && u <= U && d <= D;
                const int x = in ? tj * U1 + u : 0;
                nb[j] = lpb[x];
                ny[j] = (in && u < U) ? lpy[x] : 0.f;
            }
        };
        request(1);
        for (int d = 1; d <= D; d++) {
            double cb[KU], cy[KU], vb[KU], vy[KU];
#pragma unroll
            for (int j = 0; j < KU; j++) {
                const int u = lane * KU + j, tj = topo1 ? d - 1 : d - 1 - u;
                const bool in = tj >= 0 && tj < len && u <= U;
                const bool okb = in && (topo1 || tj + 1 < len), oky = in && u < U;
                const double lb = (double)nb[j], ly = (double)ny[j];
                cb[j] = okb ? a[j] + lb : NINF;
                cy[j] = oky ? a[j] + ly : NINF;
                vb[j] = okb ? v[j] + lb : NINF;
                vy[j] = oky ? v[j] + ly : NINF;
            }
            request(d + 1);
            double pa = NINF, pv = NINF;
            if (fwd) {
                pa = __shfl_up(cy[KU - 1], 1);
                if (lane == 0) pa = NINF;
            }
            if (vit) {
                pv = __shfl_up(vy[KU - 1], 1);
                if (lane == 0) pv = NINF;
            }
            uint32_t bits = 0;
#pragma unroll
            for (int j = 0; j < KU; j++) {
                if (fwd) a[j] = lse2(cb[j], j ? cy[j - 1] : pa);
                if (vit) {
                    const double y = j ? vy[j - 1] : pv;
                    const bool label = y > vb[j];   // equal: the blank predecessor
                    v[j] = label ? y : vb[j];
                    bits |= (label ? 1u : 0u) << j;
                }
            }
            if (frames) bprow[(size_t)d * 64] = (unsigned char)bits;
        }
        if (fwd) score = ra_fetch<KU>(a, U);
        if (vit) vscore = ra_fetch<KU>(v, U);
        if (!topo1) {
            const double last = (double)lpb[(len - 1) * U1 + U];
            score += last;
            vscore += last;
        }
    }
    if (lane == 0) {
        if (fwd) p.score[n] = score;
        if (p.vscore) p.vscore[n] = vscore;
    }
    if (!frames) return;

    // ---- traceback (the rows were written by the lanes of this wave)
    __threadfence();
    const bool found = __builtin_amdgcn_readfirstlane((int)(vscore > NINF)) != 0;
    if (found) {
        int u = U;
        for (int tb = D / TBC * TBC; tb >= 0; tb -= TBC) {
            uint32_t w[TBC];
#pragma unroll
            for (int x = 0; x < TBC; x++) {
                const int d = tb + x;
                w[x] = (d >= 1 && d <= D) ? (uint32_t)bprow[(size_t)d * 64] : 0u;
            }
#pragma unroll
            for (int x = TBC - 1; x >= 0; x--) {
                const int d = tb + x;
                if (d >= 1 && d <= D && u >= 1) {
                    const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)w[x], u / KU);
                    if ((word >> (u % KU)) & 1u) {   // the label arc that emits label u - 1
                        if (lane == 0) frames[u - 1] = topo1 ? d - 1 : d - u;
                        u = __builtin_amdgcn_readfirstlane(u - 1);
                    }
                }
            }
        }
    }
    for (int i = (found ? U : 0) + lane; i < p.mtl; i += 64) frames[i] = -1;
}

// The checks the device and the host call share, before any HIP call.
static int ra_check(const asr_rnnt* h, const void* enc, int T, int B, const void* targets, long ldt,
                    const void* target_lengths, const void* utt, int N, int mtl, int topology, const void* score,
                    const void* vscore, const void* frames) {
    if (!h || !enc || !targets || !target_lengths || T <= 0 || B <= 0 || N <= 0 || mtl < 0) return ASR_ERR_ARG;
    if (ldt < mtl || (!score && !vscore && !frames)) return ASR_ERR_ARG;
    if (topology != ASR_RNNT_LATTICE_STANDARD && topology != ASR_RNNT_LATTICE_ONE_PER_FRAME) return ASR_ERR_ARG;
    if (!utt && N > B) return ASR_ERR_ARG;
    if (mtl > RA_MAX_U) return ASR_ERR_UNSUPPORTED;
    const long U1 = mtl + 1, tiles = ((long)T * U1 + 15) / 16;
    if ((long)T * B > INT_MAX || (long)N * U1 > INT_MAX || (long)T * U1 > INT_MAX || (long)N * tiles > INT_MAX ||
        (long)N * 16 * h->d.Hp > RA_LSTM_OOB)
        return ASR_ERR_UNSUPPORTED;
    return ASR_OK;
}

template <int NRT>
static int ra_joint_launch(const RaArgs& a, hipStream_t st) {
    static AsrAttrOnce attr;
    if (int rc = attr.set((const void*)rnnt_joint_kernel<NRT>, RT_LDS_MAX)) return rc;
    const int tiles = (int)(((long)a.T * (a.mtl + 1) + 16 * NRT - 1) / (16 * NRT));
    RaArgs b = a;
    b.tiles = tiles;
    hipLaunchKernelGGL(rnnt_joint_kernel<NRT>, dim3((unsigned)a.N * (unsigned)tiles), dim3(64 * RA_WAVES),
                       (size_t)ra_lds_bytes(NRT, a.J), st, b);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

static double ra_host_lse(double a, double b) {
    if (a == -HUGE_VAL) return b;
    if (b == -HUGE_VAL) return a;
    return std::max(a, b) + std::log1p(std::exp(-std::fabs(a - b)));
}

}  // namespace asr

extern "C" {

size_t asr_rnnt_align_workspace_bytes(const asr_rnnt_t* h, int T, int B, int N, int max_target_len) {
    static const int32_t one = 0;
    if (asr::ra_check(h, &one, T, B, &one, max_target_len, &one, &one, N, max_target_len, 0, &one, nullptr, nullptr))
        return 0;
    return asr::ra_layout(h->d, T, B, N, max_target_len).total;
}

int asr_rnnt_align(const asr_rnnt_t* h, const float* d_enc, const int32_t* d_lengths, int T, int B,
                   const int32_t* d_targets, long ldt, const int32_t* d_target_lengths, const int32_t* d_utt, int N,
                   int max_target_len, int topology, double* d_score, double* d_vscore, int32_t* d_frames,
                   void* d_work, asr_stream_t s) {
    if (int rc = asr::ra_check(h, d_enc, T, B, d_targets, ldt, d_target_lengths, d_utt, N, max_target_len, topology,
                               d_score, d_vscore, d_frames))
        return rc;
    if (!d_work) return ASR_ERR_ARG;
    if (!h->d_blob) return ASR_ERR_STATE;
    const asr_rnnt_desc& d = h->d;
    const asr::RaLayout lay = asr::ra_layout(d, T, B, N, max_target_len);
    char* const wk = (char*)d_work;
    float* const f = (float*)(wk + lay.f);
    float* const P = (float*)(wk + lay.p);
    float* const hid = (float*)(wk + lay.hid);
    float* const gbuf = (float*)(wk + lay.g);
    const int U1 = max_target_len + 1;
    hipStream_t st = asr_stream(s);

    asr::RaArgs a{};
    // the model's part from the one place that knows the handle; the kernels' argument layout stays their own
    const asr::RtNet net = asr::rnnt_net(h);
    a.f = f; a.g = gbuf; a.embw = net.embw; a.P = P; a.wout = net.wout; a.bout = net.bout;
    a.lengths = d_lengths; a.targets = d_targets; a.ldt = ldt; a.target_lengths = d_target_lengths; a.utt = d_utt;
    a.lens1 = (int32_t*)(wk + lay.meta);
    a.ok = a.lens1 + N;
    a.lpb = (float*)(wk + lay.lpb); a.lpy = (float*)(wk + lay.lpy); a.bp = (unsigned char*)(wk + lay.bp);
    a.score = d_score; a.vscore = d_vscore; a.frames = d_frames;
    a.T = T; a.B = B; a.N = N; a.mtl = max_target_len; a.Hp = net.Hp; a.J = net.J; a.V = net.V; a.blank = net.blank;
    a.act = net.act; a.topology = topology;

    // 1. f = enc.W_enc + b_enc
    if (int rc = asr::rnnt_enc_launch(h, d_enc, T, B, f, st)) return rc;
    // 2. the predictor over the N targets, then g = h_top.W_pred + b_pred
    hipLaunchKernelGGL(asr::rnnt_align_prep_kernel, dim3((unsigned)N), dim3(256), 0, st, a);
    ASR_LAUNCH_TRY();
    if (int rc = asr_lstm_recur_fwd(P, nullptr, nullptr, h->d_whh[0], h->d_bih[0], h->d_bhh[0], hid, d.Hp, nullptr,
                                    nullptr, a.lens1, P, U1, N, d.Hp, 0, s))
        return rc;
    const float* htop = hid;
    if (d.L == 2) {
        float* const hid1 = hid + (size_t)U1 * N * d.Hp;
        if (int rc = asr_lstm_fwd(hid, nullptr, nullptr, h->d_wih1, h->d_whh[1], h->d_bih[1], h->d_bhh[1], hid1, d.Hp,
                                  nullptr, nullptr, a.lens1, P, U1, N, d.Hp, d.Hp, 0, s))
            return rc;
        htop = hid1;
    }
    {
        asr::GemmArgs g{};
        g.A = htop; g.B = h->d_wpred; g.b1 = h->d_bpred; g.C = gbuf;
        g.M = U1 * N; g.N = d.J; g.K = d.Hp;
        g.sam = d.Hp; g.sak = 1; g.sbk = d.J; g.sbn = 1; g.ldc = d.J;
        if (int rc = asr::gemm_launch(g, asr::EPI_BIAS, st)) return rc;
    }
    // 3. the fused joint: lpb, lpy of every lattice node
    int rc;
    switch (asr::ra_row_tiles(d.J)) {
        case 3: rc = asr::ra_joint_launch<3>(a, st); break;
        case 2: rc = asr::ra_joint_launch<2>(a, st); break;
        default: rc = asr::ra_joint_launch<1>(a, st); break;
    }
    if (rc) return rc;
    // 4. the lattice
    if (max_target_len < 64) hipLaunchKernelGGL(asr::rnnt_lattice_kernel<1>, dim3((unsigned)N), dim3(64), 0, st, a);
    else if (max_target_len < 128) hipLaunchKernelGGL(asr::rnnt_lattice_kernel<2>, dim3((unsigned)N), dim3(64), 0, st, a);
    else hipLaunchKernelGGL(asr::rnnt_lattice_kernel<4>, dim3((unsigned)N), dim3(64), 0, st, a);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

int asr_rnnt_align_host(const asr_rnnt_t* h, const float* h_enc, const int32_t* h_lengths, int T, int B,
                        const int32_t* h_targets, long ldt, const int32_t* h_target_lengths, const int32_t* h_utt,
                        int N, int max_target_len, int topology, double* h_score, double* h_vscore,
                        int32_t* h_frames) {
    if (int rc = asr::ra_check(h, h_enc, T, B, h_targets, ldt, h_target_lengths, h_utt, N, max_target_len, topology,
                               h_score, h_vscore, h_frames))
        return rc;
    const asr_rnnt_desc& d = h->d;
    const double NINF = -HUGE_VAL;
    const bool topo1 = topology == ASR_RNNT_LATTICE_ONE_PER_FRAME;
    try {
        asr::RnntHost m(*h);
        const size_t LH = (size_t)d.L * d.Hp;
        std::vector<double> hs(LH), cs(LH), gs, logit(d.V), lpb, lpy, a, v, cb, cy, vb, vy;
        std::vector<unsigned char> bits;
        for (int n = 0; n < N; n++) {
            const int U = std::min(std::max(h_target_lengths[n], 0), max_target_len), U1 = U + 1;
            const int32_t* tgt = h_targets + (long)n * ldt;
            int32_t* frames = h_frames ? h_frames + (long)n * ldt : nullptr;
            const int b = h_utt ? h_utt[n] : n;
            const bool utt_ok = b >= 0 && b < B;
            const int len = !utt_ok ? 0 : h_lengths ? std::min(std::max(h_lengths[b], 0), T) : T;
            bool bad = false;
            for (int i = 0; i < U; i++) bad = bad || tgt[i] < 0 || tgt[i] >= d.V || tgt[i] == d.blank;
            const bool feasible = !(bad || !utt_ok || (len == 0 && U > 0) || (topo1 && U > len));
            double score = NINF, vscore = NINF;
            if (frames)
                for (int i = 0; i < max_target_len; i++) frames[i] = -1;
            if (feasible && len == 0) {
                score = vscore = 0.0;
            } else if (feasible) {
                // the predictor, teacher-forced: g_u for u = 0 .. U
                gs.assign((size_t)U1 * d.J, 0.0);
                std::fill(hs.begin(), hs.end(), 0.0);
                std::fill(cs.begin(), cs.end(), 0.0);
                for (int u = 0; u <= U; u++) {
                    m.step(u ? tgt[u - 1] : d.blank, hs.data(), cs.data());
                    m.pred_proj(hs.data());
                    std::copy(m.g.begin(), m.g.end(), gs.begin() + (size_t)u * d.J);
                }
                // the joint over the grid
                lpb.assign((size_t)len * U1, 0.0);
                lpy.assign((size_t)len * U1, NINF);
                for (int t = 0; t < len; t++) {
                    m.enc_proj(h_enc + ((size_t)t * B + b) * d.E);
                    for (int u = 0; u <= U; u++) {
                        m.logits(gs.data() + (size_t)u * d.J, logit.data());
                        double best = NINF;
                        for (int k = 0; k < d.V; k++)
                            if (logit[k] > best) best = logit[k];
                        double se = 0.0;
                        for (int k = 0; k < d.V; k++) se += std::exp(logit[k] - best);
                        const double lse = best + std::log(se);
                        lpb[(size_t)t * U1 + u] = logit[d.blank] - lse;
                        if (u < U) lpy[(size_t)t * U1 + u] = logit[tgt[u]] - lse;
                    }
                }
                // the lattice: step d, state u at frame d - 1 (one per frame) or d - 1 - u (anti-diagonal)
                const int D = topo1 ? len : len - 1 + U;
                a.assign(U1, NINF);
                v.assign(U1, NINF);
                a[0] = v[0] = 0.0;
                cb.assign(U1, NINF); cy.assign(U1, NINF); vb.assign(U1, NINF); vy.assign(U1, NINF);
                bits.assign((size_t)(D + 1) * U1, 0);
                for (int dd = 1; dd <= D; dd++) {
                    for (int u = 0; u <= U; u++) {
                        const int tj = topo1 ? dd - 1 : dd - 1 - u;
                        const bool in = tj >= 0 && tj < len;
                        const bool okb = in && (topo1 || tj + 1 < len), oky = in && u < U;
                        const size_t x = in ? (size_t)tj * U1 + u : 0;
                        cb[u] = okb ? a[u] + lpb[x] : NINF;
                        cy[u] = oky ? a[u] + lpy[x] : NINF;
                        vb[u] = okb ? v[u] + lpb[x] : NINF;
                        vy[u] = oky ? v[u] + lpy[x] : NINF;
                    }
                    for (int u = 0; u <= U; u++) {
                        a[u] = asr::ra_host_lse(cb[u], u ? cy[u - 1] : NINF);
                        const double y = u ? vy[u - 1] : NINF;
                        const bool label = y > vb[u];   // equal: the blank predecessor
                        v[u] = label ? y : vb[u];
                        bits[(size_t)dd * U1 + u] = label;
                    }
                }
                score = a[U];
                vscore = v[U];
                if (!topo1) {
                    score += lpb[(size_t)(len - 1) * U1 + U];
                    vscore += lpb[(size_t)(len - 1) * U1 + U];
                }
                if (frames && vscore > NINF) {
                    int u = U;
                    for (int dd = D; dd >= 1 && u >= 1; dd--)
                        if (bits[(size_t)dd * U1 + u]) {
                            frames[u - 1] = topo1 ? dd - 1 : dd - u;
                            u--;
                        }
                }
            }
            if (h_score) h_score[n] = score;
            if (h_vscore) h_vscore[n] = vscore;
        }
    } catch (const std::bad_alloc&) {
        return ASR_ERR_OOM;
    }
    return ASR_OK;
}

}  // extern "C"
