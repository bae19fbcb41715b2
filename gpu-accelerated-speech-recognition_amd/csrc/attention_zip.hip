// The Zipformer's attention and row kernels in the library's time-major layout:
// asr_attention_zip_fwd, asr_biasnorm_fwd, asr_bypass_fwd.
//
// Shared-score attention.
//   score(p, r, h) = scale * (q(p,b,h,:) . k(r,b,h,:) + pz(p,b,h,:) . pi(h, p - r))
//   out(p, b, g, :) = sum_r softmax_r(score(p, r, s(g))) v(r, b, g, :)   over the keys p sees,
// q / k heads of width dq, pz heads of width dp (0 .. 16), value heads of width
// dv; s(g) = g when there are as many value heads as score heads, and the one
// wide value head (G = 1) uses score head `score_head`.  With the gate on the
// value is x(r) * tanh(sg(r)), formed once per element where the V block is
// written to LDS, and the output row is multiplied by y(p) where it is stored.
// The probabilities are never written anywhere: each use of a layer's scores
// recomputes them from q, k and pz.
//
// Layout, positions, lengths, the chunk / left / right window, the zeros of
// dead queries, the grid over (64 query rows, ., utterance), the four waves of
// 16 queries, the 64-key blocks aligned on absolute positions, the K / V
// prefetch, the online softmax and the P V product are asr_attention_fwd's
// (csrc/attention.hip), and the content product S^T = K Q^T keeps that kernel's
// chain (sub ascending, mm ascending, the same operands).  attn_window,
// attn_load4 and attn_exp are restated here: attention.hip stays as it is.
//
// What differs:
//  - Two widths.  NQT = 16-column tiles of a query head (1, 2, 4 or 8: a power
//    of two >= ceil(dq / 16), whole tiles past dq are skipped at run time), NVT
//    = 16-column tiles of the value slab a workgroup owns.  grid.y = G * nslab:
//    a value head wider than 128 columns is cut into slabs of 16 NVT = 128
//    columns and every slab's workgroup recomputes the head's scores (about
//    9 + 5 score MFMAs per 16 keys against 4 NVT = 32 of P V at dq = 32); slabs
//    share nothing, the last partial slab's columns are masked by selection.
//    A column's bits do not depend on dv or on the slab count.
//  - The position term.  dp <= 16 floats per head, so the MFMA contracts the
//    dims the other way round from the content product: step j contracts dims
//    4 j + g over the lane groups g, and dp = 4 is ONE v_mfma_f32_16x16x4_f32
//    per 16 distances (five per wave and key block for 64 keys; the relative-
//    position kernel of attention_rel.hip spends 4 ceil(D / 16) x 5).  The
//    table rows live in that kernel's ring (128 rows, two halves, 64 new rows
//    per key block, fetched with K and V and written between the same two
//    barriers) at a row stride of 20 floats: 10,240 B whatever dq and dv are;
//    a lane's operand is one 4-byte read at row * 20 + 4 j + g, 64 different
//    banks.  The skew (register i of tile t holds R[16 t + 4 g + i][c], key j
//    of query c needs R[j + 15 - c][c]) is that kernel's rolling window of 32
//    rows x 20 floats per wave; a tile of 16 distances that no live, unmasked
//    pair of the wave uses is skipped.  dp = 0 drops all of it.
//
// So an output row's bits depend only on its query, the keys, values and table
// rows it sees at their absolute positions and distances, and the descriptor.
//
// BiasNorm and the per-channel bypass: one wave per row, the row in registers
// (lane l: columns l, l + 64, ...), sums in layernorm_row.h's order (a lane's
// columns ascending, then the butterfly l ^ 32 ... l ^ 1).
#include "asr_internal.h"
#include "layernorm_row.h"

#include <climits>
#include <cmath>
#include <cstddef>

namespace asr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct ZipArgs {
    const float *q, *k, *pz, *v, *sg, *y, *pos;
    float* out;
    long ldq, ldk, ldpz, ldv, ldsg, ldy, ldp, ldo;
    const int32_t* lengths;
    int Tq, q_pos0, Tk, k_pos0, B;
    int H, G, Dq, Dp, Dv;          // score heads, value heads, the three widths
    int score_head, nslab, gate;
    float scale;
    int chunk, left, right;
    int pos_zero, row_lo, row_hi;  // table rows [row_lo, row_hi] may be loaded
    int vq, vk, vv, vsg, vy, vp, vo;    // rows may be moved 16 bytes at a time
};

constexpr int AZ_QT = 64;                        // query rows per workgroup
constexpr int AZ_KB = ASR_ATTN_KEY_BLOCK;        // keys per block
static_assert(AZ_KB == 64, "the kernel's tiling is written for 64-key blocks");
constexpr int AZ_RING = 2 * AZ_KB;               // table rows in LDS
constexpr int AZ_PLD = 20;                       // their row stride: 16 floats + 4
constexpr int AZ_SKR = 32, AZ_SKLD = 20;         // the skew window: rows, row stride

// Keys [lo, hi) that a live query at position pos sees, of the keys [k_pos0, kend) that exist.
__device__ __forceinline__ void attn_window(const ZipArgs& p, int pos, int kend, int& lo, int& hi) {
    const int qc = pos / p.chunk;
    lo = p.k_pos0;
    hi = kend;
    if (p.left >= 0) {
        const long v = ((long)qc - p.left) * p.chunk;        // <= pos
        if (v > lo) lo = (int)v;
    }
    if (p.right >= 0) {
        const long v = ((long)qc + p.right + 1) * p.chunk;
        if (v < hi) hi = (int)v;
    }
}

__device__ __forceinline__ f32x4 attn_load4(const float* src, bool vec) {
    if (vec) return *reinterpret_cast<const f32x4*>(src);
    return f32x4{src[0], src[1], src[2], src[3]};
}

// exp(x) for x <= 0 on v_exp_f32 (attention.hip); exp(-inf) = 0.
__device__ __forceinline__ float attn_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }

// Orders this wave's LDS writes before its LDS reads after it (and the other way round).
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

// Two waves per SIMD (at most 256 registers, the accumulators in VGPRs, see attention.hip) up to dq = 64; the
// widest query heads prefetch 8 + 2 x 8 pieces per thread beside Q and O and take one.
template <int NQT, int NVT>
__global__ __launch_bounds__(256, NQT <= 4 ? 2 : 1) void attention_zip_kernel(const ZipArgs p) {
    constexpr int LDK = 16 * NQT + 4;            // LDS row strides of K and V (attention.hip)
    constexpr int LDV = 16 * NVT + 4;
    __shared__ __attribute__((aligned(16))) float Ks[AZ_KB * LDK];
    __shared__ __attribute__((aligned(16))) float Vs[AZ_KB * LDV];
    __shared__ __attribute__((aligned(16))) float Ps[AZ_RING * AZ_PLD];
    __shared__ float Sk[4 * AZ_SKR * AZ_SKLD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int b = blockIdx.z, i0 = blockIdx.x * AZ_QT;
    const int vh = blockIdx.y / p.nslab, c0 = (blockIdx.y % p.nslab) * (16 * NVT);   // value head, slab's first column
    const int h = p.G == p.H ? vh : p.score_head;
    const int Dq = p.Dq, Dp = p.Dp;
    const int nv = p.Dv - c0;                                // the slab's columns [0, min(nv, 16 NVT)) exist
    const float NEG = -INFINITY;

    const int len = p.lengths ? max(p.lengths[b], 0) : INT_MAX;
    const int kend = min(p.k_pos0 + p.Tk, len);              // keys [k_pos0, kend) exist

    // The blocks the tile visits: from its first query's lower bound to its last live query's upper bound.
    int nb0 = 0, nb1 = -1;
    {
        const int P0 = p.q_pos0 + i0;
        const int P1 = min(p.q_pos0 + min(p.Tq, i0 + AZ_QT), len) - 1;
        if (P1 >= P0) {
            int lo, hi, t;
            attn_window(p, P0, kend, lo, t);
            attn_window(p, P1, kend, t, hi);
            if (hi > lo) {
                nb0 = lo / AZ_KB;
                nb1 = (hi - 1) / AZ_KB;
            }
        }
    }

    // This lane's query.
    const int iq = i0 + 16 * w + c;
    const int pos = p.q_pos0 + iq;
    const bool live = iq < p.Tq && pos < len;
    int rlo = 0, rhi = 0;
    if (live) attn_window(p, pos, kend, rlo, rhi);
    const long qrow = (long)(live ? iq : 0) * p.B + b;
    f32x4 qf[NQT];                                           // qf[sub][mm] = Q[query c][16 sub + 4 g + mm]
    {
        const float* qr = p.q + qrow * p.ldq + (long)h * Dq;
#pragma unroll
        for (int sub = 0; sub < NQT; sub++) {
            const int d0 = 16 * sub + 4 * g;
            qf[sub] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (live && d0 < Dq) qf[sub] = attn_load4(qr + d0, p.vq);
        }
    }
    f32x4 pzr = f32x4{0.f, 0.f, 0.f, 0.f};                   // pzr[j] = pz[query c][4 j + g]
    if (live && Dp > 0) {
        const float* pr = p.pz + qrow * p.ldpz + (long)h * Dp;
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (4 * j < Dp) pzr[j] = pr[4 * j + g];
    }

    // Table row of relative row 0 of block n: pos_zero - (P0 + 63 - 64 n); rows outside [row_lo, row_hi] read as zeros.
    const long base0 = (long)p.pos_zero - ((long)p.q_pos0 + i0 + (AZ_QT - 1));
    const int pkey = tid >> 2, pd0 = 4 * (tid & 3);          // the thread's piece of a ring half: row, dims
    auto table4 = [&](long t) {
        f32x4 r = f32x4{0.f, 0.f, 0.f, 0.f};
        if (t >= p.row_lo && t <= p.row_hi && pd0 < Dp) r = attn_load4(p.pos + t * p.ldp + (long)h * Dp + pd0, p.vp);
        return r;
    };

    // Thread tid fetches 4-float pieces e = tid + 256 u of a K block (key e / (4 NQT), dims 4 (e % (4 NQT)) ...)
    // and of the V slab (key e / (4 NVT), columns c0 + 4 (e % (4 NVT)) ...; with the gate, of x and of sg); of
    // the table, relative row 64 + pkey of the block (its rows 0 .. 63 are in the ring already).
    f32x4 kr[NQT], vr[NVT], sr[NVT], pr = f32x4{0.f, 0.f, 0.f, 0.f};
    auto fetch = [&](int n) {
#pragma unroll
        for (int u = 0; u < NQT; u++) {
            const int e = tid + 256 * u;
            const int key = e / (4 * NQT), d0 = 4 * (e % (4 * NQT));
            const int r = n * AZ_KB + key;
            kr[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (r >= p.k_pos0 && r < kend && d0 < Dq)
                kr[u] = attn_load4(p.k + ((long)(r - p.k_pos0) * p.B + b) * p.ldk + (long)h * Dq + d0, p.vk);
        }
#pragma unroll
        for (int u = 0; u < NVT; u++) {
            const int e = tid + 256 * u;
            const int key = e / (4 * NVT), d0 = 4 * (e % (4 * NVT));
            const int r = n * AZ_KB + key;
            vr[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            sr[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (r >= p.k_pos0 && r < kend && d0 < nv) {
                const long row = (long)(r - p.k_pos0) * p.B + b;
                const long col = (long)vh * p.Dv + c0 + d0;
                vr[u] = attn_load4(p.v + row * p.ldv + col, p.vv);
                if (p.gate) sr[u] = attn_load4(p.sg + row * p.ldsg + col, p.vsg);
            }
        }
        if (Dp > 0) pr = table4(base0 + (long)AZ_KB * n + AZ_KB + pkey);
    };
    auto stage = [&](int n) {
#pragma unroll
        for (int u = 0; u < NQT; u++) {
            const int e = tid + 256 * u;
            const int key = e / (4 * NQT), d0 = 4 * (e % (4 * NQT));
            *reinterpret_cast<f32x4*>(&Ks[key * LDK + d0]) = kr[u];
        }
#pragma unroll
        for (int u = 0; u < NVT; u++) {
            const int e = tid + 256 * u;
            const int key = e / (4 * NVT), d0 = 4 * (e % (4 * NVT));
            f32x4 val = vr[u];
            if (p.gate) {                                    // x * tanh(sg), once per element; tanh(+-100) is +-1
#pragma unroll
                for (int i = 0; i < 4; i++) val[i] = vr[u][i] * tanhf(sr[u][i]);
            }
            *reinterpret_cast<f32x4*>(&Vs[key * LDV + d0]) = val;
        }
        if (Dp > 0) {
            const int half = ((n - nb0 + 1) & 1) * AZ_KB;    // ring rows of the block's relative rows 64 .. 127
            *reinterpret_cast<f32x4*>(&Ps[(half + pkey) * AZ_PLD + pd0]) = pr;
        }
    };

    f32x4 o[NVT];                                            // o[dt][i] = O[query c][c0 + 16 dt + 4 g + i]
#pragma unroll
    for (int dt = 0; dt < NVT; dt++) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = NEG, l = 0.f;
    float* sk = &Sk[w * (AZ_SKR * AZ_SKLD)];
    const int ws = 48 - 16 * w;                              // the wave's first relative row

    if (nb0 <= nb1) {
        // relative rows 0 .. 63 of the first block into ring half 0; the loop's barriers order them
        if (Dp > 0)
            *reinterpret_cast<f32x4*>(&Ps[pkey * AZ_PLD + pd0]) = table4(base0 + (long)AZ_KB * nb0 + pkey);
        fetch(nb0);
    }
    for (int n = nb0; n <= nb1; n++) {
        __syncthreads();                                     // the block before this one has been read
        stage(n);
        __syncthreads();
        if (n < nb1) fetch(n + 1);
        const int r0 = n * AZ_KB;
        const bool any = rlo < rhi && rlo < r0 + AZ_KB && rhi > r0;
        if (__builtin_amdgcn_ballot_w64(any) == 0) continue; // uniform in the wave; the barriers are above

        f32x4 s[4];
#pragma unroll
        for (int kt = 0; kt < 4; kt++) s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int sub = 0; sub < NQT; sub++) {
            if (16 * sub < Dq) {
                f32x4 a[4];
#pragma unroll
                for (int kt = 0; kt < 4; kt++)
                    a[kt] = *reinterpret_cast<const f32x4*>(&Ks[(16 * kt + c) * LDK + 16 * sub + 4 * g]);
#pragma unroll
                for (int mm = 0; mm < 4; mm++)
#pragma unroll
                    for (int kt = 0; kt < 4; kt++)
                        s[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kt][mm], qf[sub][mm], s[kt], 0, 0, 0);
            }
        }

        if (Dp > 0) {
            // The position product: tile t = relative rows ws + 16 t ... of the ring; the lane's query uses the
            // distances rho = j + 15 - c of its visible keys j.
            const int rl = any ? max(rlo, r0) - r0 + 15 - c : 128;
            const int rh = any ? min(rhi, r0 + AZ_KB) - 1 - r0 + 15 - c : -1;
            const int rbase = ws + ((n - nb0) & 1) * AZ_KB + c;   // ring row of the lane's row of tile 0, before the wrap
            bool use[5];
#pragma unroll
            for (int t = 0; t < 5; t++) use[t] = __builtin_amdgcn_ballot_w64(rl <= 16 * t + 15 && rh >= 16 * t) != 0;
            // Tile t: its MFMA chain (step j contracts dims 4 j + g), then its rows into the skew window (row rho
            // at (rho & 31) * 20 + c).
            auto tile = [&](int t) {
                if (!use[t]) return;
                const float* prow = &Ps[((rbase + 16 * t) & (AZ_RING - 1)) * AZ_PLD + g];
                f32x4 rt = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (4 * j < Dp) rt = __builtin_amdgcn_mfma_f32_16x16x4f32(prow[4 * j], pzr[j], rt, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; i++) sk[(((16 * t) & (AZ_SKR - 1)) + 4 * g + i) * AZ_SKLD + c] = rt[i];
            };
            // The skew, key tile by key tile: rows 16 kt .. 16 kt + 30 are tiles kt and kt + 1, so tile kt + 1 goes
            // over tile kt - 1 once key tile kt - 1 has been read.  A skipped tile's rows hold anything: only
            // masked pairs read them.
            tile(0);
#pragma unroll
            for (int kt = 0; kt < 4; kt++) {
                tile(kt + 1);
                wave_lds_sync();
#pragma unroll
                for (int i = 0; i < 4; i++)
                    s[kt][i] += sk[((16 * kt + 4 * g + i + 15 - c) & (AZ_SKR - 1)) * AZ_SKLD + c];
                wave_lds_sync();
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
        const float alpha = (m == mn) ? 1.f : attn_exp(m - mn);     // O and l are 0 while m is -inf
        float ps[4];
#pragma unroll
        for (int kt = 0; kt < 4; kt++) {
#pragma unroll
            for (int i = 0; i < 4; i++) s[kt][i] = (s[kt][i] == NEG) ? 0.f : attn_exp(s[kt][i] - mn);
            ps[kt] = (s[kt][0] + s[kt][1]) + (s[kt][2] + s[kt][3]);
        }
        float bs = (ps[0] + ps[1]) + (ps[2] + ps[3]);
        bs += __shfl_xor(bs, 16);
        bs += __shfl_xor(bs, 32);
        l = l * alpha + bs;
        m = mn;
#pragma unroll
        for (int dt = 0; dt < NVT; dt++) o[dt] *= alpha;
#pragma unroll
        for (int kt = 0; kt < 4; kt++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float* vrow = &Vs[(16 * kt + 4 * g + i) * LDV + c];
#pragma unroll
                for (int dt = 0; dt < NVT; dt++)
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vrow[16 * dt], s[kt][i], o[dt], 0, 0, 0);
            }
    }

    if (iq >= p.Tq) return;
    const bool nz = live && l > 0.f;
    const long ocol = (long)vh * p.Dv + c0;
    float* orow = p.out + ((long)iq * p.B + b) * p.ldo + ocol;
    const float* yrow = p.gate ? p.y + ((long)iq * p.B + b) * p.ldy + ocol : nullptr;
#pragma unroll
    for (int dt = 0; dt < NVT; dt++) {
        const int d0 = 16 * dt + 4 * g;
        if (d0 >= nv) continue;
        f32x4 r = f32x4{0.f, 0.f, 0.f, 0.f};
        if (nz) {                                            // a dead row's y is not read: it may hold NaN
#pragma unroll
            for (int i = 0; i < 4; i++) r[i] = o[dt][i] / l;
            if (p.gate) r *= attn_load4(yrow + d0, p.vy);
        }
        if (p.vo) {
            *reinterpret_cast<f32x4*>(orow + d0) = r;
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) orow[d0 + i] = r[i];
        }
    }
}

template <int NQT>
static void attention_zip_launch(const ZipArgs& p, int nvt, dim3 grid, hipStream_t st) {
    if (nvt <= 1) hipLaunchKernelGGL((attention_zip_kernel<NQT, 1>), grid, dim3(256), 0, st, p);
    else if (nvt <= 2) hipLaunchKernelGGL((attention_zip_kernel<NQT, 2>), grid, dim3(256), 0, st, p);
    else if (nvt <= 4) hipLaunchKernelGGL((attention_zip_kernel<NQT, 4>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((attention_zip_kernel<NQT, 8>), grid, dim3(256), 0, st, p);
}

// ---------------------------------------------------------------------------
// BiasNorm (MODE 0, with the layer's last bypass fused when x0 is given) and the
// per-channel bypass alone (MODE 1).  Grid ceil(M / 4) workgroups of 4 waves,
// one row per wave.  NU = columns per lane (a power of two >= ceil(N / 64)).
// ---------------------------------------------------------------------------
struct ZipRowArgs {
    const float *x, *bias, *x0, *bypass;
    float* out;
    long ldx, ldx0, ldo;
    const int32_t* lengths;
    float scale;                   // exp(log_scale)
    int T, B, N, M;
};

template <int NU, int MODE>
__global__ __launch_bounds__(256) void zip_row_kernel(const ZipRowArgs p) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + w;
    if (row >= p.M) return;
    const int t = row / p.B, b = row - t * p.B;
    const int len = p.lengths ? min(max(p.lengths[b], 0), p.T) : p.T;
    float* orow = p.out + (long)row * p.ldo;
    if (t >= len) {
#pragma unroll
        for (int u = 0; u < NU; u++)
            if (lane + 64 * u < p.N) orow[lane + 64 * u] = 0.f;
        return;
    }
    const float* xr = p.x + (long)row * p.ldx;
    const float* x0r = p.x0 ? p.x0 + (long)row * p.ldx0 : nullptr;
    float v[NU];
    float sq = 0.f;
#pragma unroll
    for (int u = 0; u < NU; u++) {
        const int col = lane + 64 * u;
        v[u] = 0.f;
        if (col < p.N) {
            v[u] = xr[col];
            if (MODE == 0) {
                const float dl = v[u] - p.bias[col];
                sq += dl * dl;
            }
        }
    }
    float f = 1.f;
    if (MODE == 0) f = p.scale / sqrtf(ln_wave_sum(sq) / (float)p.N);   // a row equal to its bias: +inf
#pragma unroll
    for (int u = 0; u < NU; u++) {
        const int col = lane + 64 * u;
        if (col < p.N) {
            float y = MODE == 0 ? v[u] * f : v[u];
            if (x0r) {
                const float a = x0r[col];
                y = a + (y - a) * p.bypass[col];
            }
            orow[col] = y;
        }
    }
}

template <int MODE>
static int zip_row_launch(const ZipRowArgs& p, asr_stream_t s) {
    const dim3 grid((unsigned)((p.M + 3) / 4));
    hipStream_t st = asr_stream(s);
    const int nu = (p.N + 63) / 64;
    if (nu <= 1) hipLaunchKernelGGL((zip_row_kernel<1, MODE>), grid, dim3(256), 0, st, p);
    else if (nu <= 2) hipLaunchKernelGGL((zip_row_kernel<2, MODE>), grid, dim3(256), 0, st, p);
    else if (nu <= 4) hipLaunchKernelGGL((zip_row_kernel<4, MODE>), grid, dim3(256), 0, st, p);
    else if (nu <= 8) hipLaunchKernelGGL((zip_row_kernel<8, MODE>), grid, dim3(256), 0, st, p);
    else if (nu <= 16) hipLaunchKernelGGL((zip_row_kernel<16, MODE>), grid, dim3(256), 0, st, p);
    else if (nu <= 32) hipLaunchKernelGGL((zip_row_kernel<32, MODE>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((zip_row_kernel<64, MODE>), grid, dim3(256), 0, st, p);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

static bool aligned16(const void* ptr, long ld) { return ((uintptr_t)ptr & 15) == 0 && ld % 4 == 0; }

}  // namespace asr

extern "C" {

int asr_attention_zip_fwd(const asr_zattn_desc* d, const float* d_q, long ldq, const float* d_k, long ldk,
                          const float* d_pz, long ldpz, const float* d_v, long ldv, const float* d_sg, long ldsg,
                          const float* d_y, long ldy, const float* d_pos, long ldp, int n_pos, int pos_zero,
                          const int32_t* d_lengths, float* d_out, long ldo, int Tq, int q_pos0, int Tk, int k_pos0,
                          int B, asr_stream_t s) {
    if (!d || !d_q || !d_k || !d_v || !d_out) return ASR_ERR_ARG;
    if (d->pos_dim < 0 || (d->gate != 0 && d->gate != 1)) return ASR_ERR_ARG;
    if (d->pos_dim > 0 && (!d_pz || !d_pos)) return ASR_ERR_ARG;
    if (d->gate && (!d_sg || !d_y)) return ASR_ERR_ARG;
    if (Tq <= 0 || Tk <= 0 || B <= 0 || d->heads <= 0 || d->query_dim <= 0 || d->value_dim <= 0 || d->chunk <= 0 ||
        (d->pos_dim > 0 && n_pos <= 0))
        return ASR_ERR_ARG;
    if (d->value_heads != d->heads && d->value_heads != 1) return ASR_ERR_ARG;
    if (d->score_head < 0 || d->score_head >= d->heads) return ASR_ERR_ARG;
    if (d->left < -1 || d->right < -1 || q_pos0 < 0 || k_pos0 < 0) return ASR_ERR_ARG;
    const long Eq = (long)d->heads * d->query_dim, Ep = (long)d->heads * d->pos_dim;
    const long Ev = (long)d->value_heads * d->value_dim;
    if (ldq < Eq || ldk < Eq || ldv < Ev || ldo < Ev) return ASR_ERR_ARG;
    if (d->pos_dim > 0 && (ldpz < Ep || ldp < Ep)) return ASR_ERR_ARG;
    if (d->gate && (ldsg < Ev || ldy < Ev)) return ASR_ERR_ARG;
    if (!std::isfinite(d->scale) || d->scale < 0.f) return ASR_ERR_ARG;
    // the distances query frame - key frame the call can ask for, lengths aside
    long dmax = (long)q_pos0 + Tq - 1 - k_pos0, dmin = (long)q_pos0 - ((long)k_pos0 + Tk - 1);
    if (d->left >= 0) dmax = std::min(dmax, ((long)d->left + 1) * d->chunk - 1);
    if (d->right >= 0) dmin = std::max(dmin, -(((long)d->right + 1) * d->chunk - 1));
    if (d->pos_dim > 0 && dmax >= dmin && ((long)pos_zero - dmax < 0 || (long)pos_zero - dmin > (long)n_pos - 1))
        return ASR_ERR_ARG;
    if (d->query_dim % 4 != 0 || d->query_dim > 128 || Eq > 4096) return ASR_ERR_UNSUPPORTED;
    if (d->pos_dim % 4 != 0 || d->pos_dim > 16) return ASR_ERR_UNSUPPORTED;
    if (d->value_dim % 4 != 0 || Ev > 4096) return ASR_ERR_UNSUPPORTED;
    if (d->heads > 65535 || B > 65535) return ASR_ERR_UNSUPPORTED;                  // grid dimensions
    // key and query positions, and a block's end past them, stay inside an int
    if ((long)q_pos0 + Tq > (long)INT_MAX - 64 || (long)k_pos0 + Tk > (long)INT_MAX - 64) return ASR_ERR_UNSUPPORTED;
    if ((long)Tq * B > INT_MAX || (long)Tk * B > INT_MAX) return ASR_ERR_UNSUPPORTED;

    const int tv = (d->value_dim + 15) / 16;                 // 16-column tiles of a value head
    const int nvt = tv <= 1 ? 1 : tv <= 2 ? 2 : tv <= 4 ? 4 : 8;

    asr::ZipArgs p{};
    p.q = d_q; p.k = d_k; p.pz = d_pz; p.v = d_v; p.sg = d_sg; p.y = d_y; p.pos = d_pos; p.out = d_out;
    p.ldq = ldq; p.ldk = ldk; p.ldpz = ldpz; p.ldv = ldv; p.ldsg = ldsg; p.ldy = ldy; p.ldp = ldp; p.ldo = ldo;
    p.lengths = d_lengths;
    p.Tq = Tq; p.q_pos0 = q_pos0; p.Tk = Tk; p.k_pos0 = k_pos0; p.B = B;
    p.H = d->heads; p.G = d->value_heads; p.Dq = d->query_dim; p.Dp = d->pos_dim; p.Dv = d->value_dim;
    p.score_head = d->score_head; p.gate = d->gate;
    p.nslab = (tv + nvt - 1) / nvt;                          // <= 4096 / 128 slabs a head, <= 1024 slabs in all
    p.scale = d->scale == 0.f ? 1.f / std::sqrt((float)d->query_dim) : d->scale;
    p.chunk = d->chunk; p.left = d->left; p.right = d->right;
    p.pos_zero = pos_zero;
    p.row_lo = dmax >= dmin ? (int)(pos_zero - dmax) : 0;    // no distance at all: no row is loaded
    p.row_hi = dmax >= dmin ? (int)(pos_zero - dmin) : -1;
    p.vq = asr::aligned16(d_q, ldq); p.vk = asr::aligned16(d_k, ldk);
    p.vv = asr::aligned16(d_v, ldv); p.vo = asr::aligned16(d_out, ldo);
    p.vsg = asr::aligned16(d_sg, ldsg); p.vy = asr::aligned16(d_y, ldy);
    p.vp = asr::aligned16(d_pos, ldp);

    const dim3 grid((unsigned)((Tq + asr::AZ_QT - 1) / asr::AZ_QT), (unsigned)(d->value_heads * p.nslab), (unsigned)B);
    hipStream_t st = asr_stream(s);
    const int nq = (d->query_dim + 15) / 16;
    if (nq <= 1) asr::attention_zip_launch<1>(p, nvt, grid, st);
    else if (nq <= 2) asr::attention_zip_launch<2>(p, nvt, grid, st);
    else if (nq <= 4) asr::attention_zip_launch<4>(p, nvt, grid, st);
    else asr::attention_zip_launch<8>(p, nvt, grid, st);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

int asr_biasnorm_fwd(const float* d_x, long ldx, const float* d_bias, float log_scale, const float* d_x0, long ldx0,
                     const float* d_bypass, const int32_t* d_lengths, float* d_out, long ldo, int T, int B, int N,
                     asr_stream_t s) {
    if (!d_x || !d_bias || !d_out) return ASR_ERR_ARG;
    if ((d_x0 == nullptr) != (d_bypass == nullptr)) return ASR_ERR_ARG;
    if (T <= 0 || B <= 0 || N <= 0) return ASR_ERR_ARG;
    if (ldx < N || ldo < N || (d_x0 && ldx0 < N)) return ASR_ERR_ARG;
    if (!std::isfinite(log_scale)) return ASR_ERR_ARG;
    if (N > 4096) return ASR_ERR_UNSUPPORTED;
    if ((long)T * B > INT_MAX) return ASR_ERR_UNSUPPORTED;

    asr::ZipRowArgs p{};
    p.x = d_x; p.bias = d_bias; p.x0 = d_x0; p.bypass = d_bypass; p.out = d_out;
    p.ldx = ldx; p.ldx0 = ldx0; p.ldo = ldo; p.lengths = d_lengths;
    p.scale = (float)std::exp((double)log_scale);
    p.T = T; p.B = B; p.N = N; p.M = T * B;
    return asr::zip_row_launch<0>(p, s);
}

int asr_bypass_fwd(const float* d_x, long ldx, const float* d_x0, long ldx0, const float* d_scale,
                   const int32_t* d_lengths, float* d_out, long ldo, int T, int B, int N, asr_stream_t s) {
    if (!d_x || !d_x0 || !d_scale || !d_out) return ASR_ERR_ARG;
    if (T <= 0 || B <= 0 || N <= 0) return ASR_ERR_ARG;
    if (ldx < N || ldx0 < N || ldo < N) return ASR_ERR_ARG;
    if (N > 4096) return ASR_ERR_UNSUPPORTED;
    if ((long)T * B > INT_MAX) return ASR_ERR_UNSUPPORTED;

    asr::ZipRowArgs p{};
    p.x = d_x; p.x0 = d_x0; p.bypass = d_scale; p.out = d_out;
    p.ldx = ldx; p.ldx0 = ldx0; p.ldo = ldo; p.lengths = d_lengths;
    p.scale = 1.f;
    p.T = T; p.B = B; p.N = N; p.M = T * B;
    return asr::zip_row_launch<1>(p, s);
}

}  // extern "C"
