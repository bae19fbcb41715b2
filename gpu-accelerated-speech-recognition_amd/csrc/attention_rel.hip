// Relative-position (Transformer-XL) self-attention in the library's time-major
// layout: asr_attention_rel_fwd.
//
//   score(p, r) = scale * ((q_p + u_h) . k_r + (q_p + v_h) . pi_h(p - r))
//   out(p, b, h, :) = sum_r softmax_r(score(p, r)) v(r)      over the keys p sees,
// pi_h(delta) = columns [h*D, (h+1)*D) of row pos_zero - delta of the projected
// table d_pos.  Layout, positions, lengths, the chunk / left / right window and
// the zeros of dead queries are asr_attention_fwd's (csrc/attention.hip), and so
// are the grid (ceil(Tq / 64), heads, B), the four waves of 16 queries, the
// 64-key blocks aligned on absolute positions, the K / V prefetch, the online
// softmax and the P V product; the content product S^T = K (Q + u)^T keeps that
// kernel's chain (sub ascending, mm ascending, the same operands), so a zero
// table and NULL biases give asr_attention_fwd's bits.  attn_window, attn_load4
// and attn_exp are restated here: attention.hip stays as it is.
//
// The position term.  The workgroup's queries stand at frames P0 .. P0 + 63, the
// block's keys at r0 .. r0 + 63.  Relative row x = 63 - qi + j (query qi, key j,
// both 0 .. 63) is table row base + x, base = pos_zero - (P0 + 63 - r0): 127
// rows, and when the block advances by 64 keys base advances by 64 rows.
//  - Ring.  Ps holds 128 table rows in the table's own layout at the K block's
//    row stride, as two halves of 64.  Block n reads relative rows 0 .. 63 from
//    half (n - nb0) & 1 and rows 64 .. 127 from the other; rows 64 .. 127 of
//    block n are rows 0 .. 63 of block n + 1, so each block loads 64 new rows,
//    the traffic of one more K block, instead of the 4 x 80 rows four waves would
//    load for themselves.  The new half travels global -> registers -> LDS with
//    K and V: fetched before the MFMAs of the block before, written between the
//    two barriers over the half whose rows the block before has finished with.
//    No third barrier.  Rows outside [row_lo, row_hi] (the distances the call
//    can ask for, checked on the host against the table's size) are never
//    loaded: zeros are selected.
//  - Product.  Wave w needs relative rows 48 - 16 w + rho, rho = 0 .. 78: five
//    16-row tiles.  R^T[rho][query c] = pi(rho) . (q_c + v) on
//    v_mfma_f32_16x16x4_f32, A = the ring rows read as K is read (16 bytes per
//    lane, the same banks), B = Q + v in registers, dims chained in the content
//    product's order.  A tile none of whose 16 distances a live, unmasked pair
//    of the wave uses is skipped (a wave-uniform ballot per tile).
//  - Skew.  Register i of tile t holds R[16 t + 4 g + i][c]; key j of query c
//    needs R[j + 15 - c][c].  Per wave through LDS, a rolling window of 32 rows
//    x stride 20 floats: key tile kt reads rows 16 kt .. 16 kt + 30, which tiles
//    kt and kt + 1 hold, so tile kt + 1 is written over tile kt - 1 before key
//    tile kt is read.  Row rho lives at (rho & 31) * 20 + c; 32 * 20 is a
//    multiple of the 64 banks, so the wrap keeps the banks of the unwrapped
//    layout: the writes (banks c, 16 + c within a half-wave) and the skewed
//    reads (13 c, 16 + 13 c mod 32) are conflict-free.  Wave-level fences, no
//    workgroup barrier.  2,560 B per wave: at D <= 64 the kernel's LDS is
//    K + V + ring + skew = 3 x 17,408 + 10,240 = 62,464 ... 79,872 B, two
//    workgroups per CU.
//  - score = (ac + bd) * scale, masked by selection.
//
// So an output row's bits depend only on its query, the keys, values and table
// rows it sees at their absolute positions and distances, the biases and the
// descriptor: a tile's R[rho][c] is one MFMA chain over the dims of one table
// row and one query, whatever else the tile holds.
#include "asr_internal.h"

#include <climits>
#include <cmath>
#include <cstddef>

namespace asr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct AttnRelArgs {
    const float *q, *k, *v, *pos, *bias_u, *bias_v;
    float* out;
    long ldq, ldk, ldv, ldo, ldp;
    const int32_t* lengths;
    int Tq, q_pos0, Tk, k_pos0, B;
    int D;                         // head_dim
    float scale;
    int chunk, left, right;
    int pos_zero, row_lo, row_hi;  // table rows [row_lo, row_hi] may be loaded
    int vq, vk, vv, vo, vp, vbu, vbv;   // rows may be moved 16 bytes at a time
};

constexpr int AR_QT = 64;                        // query rows per workgroup
constexpr int AR_KB = ASR_ATTN_KEY_BLOCK;        // keys per block
static_assert(AR_KB == 64, "the kernel's tiling is written for 64-key blocks");
constexpr int AR_RING = 2 * AR_KB;               // table rows in LDS
constexpr int AR_SKR = 32, AR_SKLD = 20;         // the skew window: rows, row stride

// Keys [lo, hi) that a live query at position pos sees, of the keys [k_pos0, kend) that exist.
__device__ __forceinline__ void attn_window(const AttnRelArgs& p, int pos, int kend, int& lo, int& hi) {
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

// NDT = ceil(D / 16): 16-column tiles of a head.  Two waves per SIMD (at most 256 registers, the accumulators in
// VGPRs, see attention.hip) up to D = 64, where the LDS lets two workgroups share a CU; past it K + V + ring leave
// room for one workgroup per CU, and Q + u, Q + v and three prefetched blocks take more than 256 registers.
template <int NDT>
__global__ __launch_bounds__(256, NDT <= 4 ? 2 : 1) void attention_rel_kernel(const AttnRelArgs p) {
    constexpr int LD = 16 * NDT + 4;             // LDS row stride of K, V and the ring (attention.hip)
    __shared__ __attribute__((aligned(16))) float Ks[AR_KB * LD];
    __shared__ __attribute__((aligned(16))) float Vs[AR_KB * LD];
    __shared__ __attribute__((aligned(16))) float Ps[AR_RING * LD];
    __shared__ float Sk[4 * AR_SKR * AR_SKLD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int b = blockIdx.z, h = blockIdx.y, i0 = blockIdx.x * AR_QT;
    const int D = p.D;
    const float NEG = -INFINITY;

    const int len = p.lengths ? max(p.lengths[b], 0) : INT_MAX;
    const int kend = min(p.k_pos0 + p.Tk, len);              // keys [k_pos0, kend) exist

    // The blocks the tile visits: from its first query's lower bound to its last live query's upper bound.
    int nb0 = 0, nb1 = -1;
    {
        const int P0 = p.q_pos0 + i0;
        const int P1 = min(p.q_pos0 + min(p.Tq, i0 + AR_QT), len) - 1;
        if (P1 >= P0) {
            int lo, hi, t;
            attn_window(p, P0, kend, lo, t);
            attn_window(p, P1, kend, t, hi);
            if (hi > lo) {
                nb0 = lo / AR_KB;
                nb1 = (hi - 1) / AR_KB;
            }
        }
    }

    // This lane's query.
    const int iq = i0 + 16 * w + c;
    const int pos = p.q_pos0 + iq;
    const bool live = iq < p.Tq && pos < len;
    int rlo = 0, rhi = 0;
    if (live) attn_window(p, pos, kend, rlo, rhi);
    f32x4 qf[NDT], qv[NDT];                                  // [sub][mm] = (Q + u | Q + v)[query c][16 sub + 4 g + mm]
    {
        const float* qr = p.q + ((long)(live ? iq : 0) * p.B + b) * p.ldq + (long)h * D;
#pragma unroll
        for (int sub = 0; sub < NDT; sub++) {
            const int d0 = 16 * sub + 4 * g;
            qf[sub] = f32x4{0.f, 0.f, 0.f, 0.f};
            qv[sub] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (live && d0 < D) {
                const f32x4 qq = attn_load4(qr + d0, p.vq);
                qf[sub] = qv[sub] = qq;
                if (p.bias_u) qf[sub] = qq + attn_load4(p.bias_u + (long)h * D + d0, p.vbu);
                if (p.bias_v) qv[sub] = qq + attn_load4(p.bias_v + (long)h * D + d0, p.vbv);
            }
        }
    }

    // Table row of relative row 0 of block n: pos_zero - (P0 + 63 - 64 n); rows outside [row_lo, row_hi] read as zeros.
    const long base0 = (long)p.pos_zero - ((long)p.q_pos0 + i0 + (AR_QT - 1));
    auto table4 = [&](long t, int d0) {
        f32x4 r = f32x4{0.f, 0.f, 0.f, 0.f};
        if (t >= p.row_lo && t <= p.row_hi && d0 < D) r = attn_load4(p.pos + t * p.ldp + (long)h * D + d0, p.vp);
        return r;
    };

    // Thread tid fetches 4-float pieces e = tid + 256 u of a block: key e / (4 NDT), dims 4 (e % (4 NDT)) ...;
    // of the table, relative row 64 + key of the block (its rows 0 .. 63 are in the ring already).
    f32x4 kr[NDT], vr[NDT], pr[NDT];
    auto fetch = [&](int n) {
#pragma unroll
        for (int u = 0; u < NDT; u++) {
            const int e = tid + 256 * u;
            const int key = e / (4 * NDT), d0 = 4 * (e % (4 * NDT));
            const int r = n * AR_KB + key;
            kr[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            vr[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (r >= p.k_pos0 && r < kend && d0 < D) {
                const long row = (long)(r - p.k_pos0) * p.B + b;
                kr[u] = attn_load4(p.k + row * p.ldk + (long)h * D + d0, p.vk);
                vr[u] = attn_load4(p.v + row * p.ldv + (long)h * D + d0, p.vv);
            }
            pr[u] = table4(base0 + (long)AR_KB * n + AR_KB + key, d0);
        }
    };
    auto stage = [&](int n) {
        const int half = ((n - nb0 + 1) & 1) * AR_KB;        // ring rows of the block's relative rows 64 .. 127
#pragma unroll
        for (int u = 0; u < NDT; u++) {
            const int e = tid + 256 * u;
            const int key = e / (4 * NDT), d0 = 4 * (e % (4 * NDT));
            *reinterpret_cast<f32x4*>(&Ks[key * LD + d0]) = kr[u];
            *reinterpret_cast<f32x4*>(&Vs[key * LD + d0]) = vr[u];
            *reinterpret_cast<f32x4*>(&Ps[(half + key) * LD + d0]) = pr[u];
        }
    };

    f32x4 o[NDT];                                            // o[dt][i] = O[query c][16 dt + 4 g + i]
#pragma unroll
    for (int dt = 0; dt < NDT; dt++) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = NEG, l = 0.f;
    float* sk = &Sk[w * (AR_SKR * AR_SKLD)];
    const int ws = 48 - 16 * w;                              // the wave's first relative row

    if (nb0 <= nb1) {
        // relative rows 0 .. 63 of the first block into ring half 0; the loop's barriers order them
#pragma unroll
        for (int u = 0; u < NDT; u++) {
            const int e = tid + 256 * u;
            const int key = e / (4 * NDT), d0 = 4 * (e % (4 * NDT));
            *reinterpret_cast<f32x4*>(&Ps[key * LD + d0]) = table4(base0 + (long)AR_KB * nb0 + key, d0);
        }
        fetch(nb0);
    }
    for (int n = nb0; n <= nb1; n++) {
        __syncthreads();                                     // the block before this one has been read
        stage(n);
        __syncthreads();
        if (n < nb1) fetch(n + 1);
        const int r0 = n * AR_KB;
        const bool any = rlo < rhi && rlo < r0 + AR_KB && rhi > r0;
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

        // The position product: tile t = relative rows ws + 16 t ... of the ring; the lane's query uses the
        // distances rho = j + 15 - c of its visible keys j.
        const int rl = any ? max(rlo, r0) - r0 + 15 - c : 128, rh = any ? min(rhi, r0 + AR_KB) - 1 - r0 + 15 - c : -1;
        const int rbase = ws + ((n - nb0) & 1) * AR_KB + c;  // ring row of the lane's row of tile 0, before the wrap
        bool use[5];
#pragma unroll
        for (int t = 0; t < 5; t++) use[t] = __builtin_amdgcn_ballot_w64(rl <= 16 * t + 15 && rh >= 16 * t) != 0;
        // Tile t: its MFMA chain, then its rows into the skew window (row rho at (rho & 31) * 20 + c).
        auto tile = [&](int t) {
            if (!use[t]) return;
            const float* prow = &Ps[((rbase + 16 * t) & (AR_RING - 1)) * LD + 4 * g];
            f32x4 rt = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int sub = 0; sub < NDT; sub++) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(prow + 16 * sub);
#pragma unroll
                for (int mm = 0; mm < 4; mm++)
                    if (16 * sub + mm < D) rt = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mm], qv[sub][mm], rt, 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < 4; i++) sk[(((16 * t) & (AR_SKR - 1)) + 4 * g + i) * AR_SKLD + c] = rt[i];
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
                s[kt][i] += sk[((16 * kt + 4 * g + i + 15 - c) & (AR_SKR - 1)) * AR_SKLD + c];
            wave_lds_sync();
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

    if (iq >= p.Tq) return;
    const bool nz = live && l > 0.f;
    float* orow = p.out + ((long)iq * p.B + b) * p.ldo + (long)h * D;
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

static bool aligned16(const void* ptr, long ld) { return ((uintptr_t)ptr & 15) == 0 && ld % 4 == 0; }

}  // namespace asr

extern "C" {

int asr_attention_rel_fwd(const asr_attn_desc* d, const float* d_q, long ldq, const float* d_k, long ldk,
                          const float* d_v, long ldv, const float* d_pos, long ldp, int n_pos, int pos_zero,
                          const float* d_bias_u, const float* d_bias_v, const int32_t* d_lengths, float* d_out,
                          long ldo, int Tq, int q_pos0, int Tk, int k_pos0, int B, asr_stream_t s) {
    if (!d || !d_q || !d_k || !d_v || !d_out || !d_pos) return ASR_ERR_ARG;
    if (Tq <= 0 || Tk <= 0 || B <= 0 || d->heads <= 0 || d->head_dim <= 0 || d->chunk <= 0 || n_pos <= 0)
        return ASR_ERR_ARG;
    if (d->left < -1 || d->right < -1 || q_pos0 < 0 || k_pos0 < 0) return ASR_ERR_ARG;
    const long E = (long)d->heads * d->head_dim;
    if (ldq < E || ldk < E || ldv < E || ldo < E || ldp < E) return ASR_ERR_ARG;
    if (!std::isfinite(d->scale) || d->scale < 0.f) return ASR_ERR_ARG;
    // the distances query frame - key frame the call can ask for, lengths aside
    long dmax = (long)q_pos0 + Tq - 1 - k_pos0, dmin = (long)q_pos0 - ((long)k_pos0 + Tk - 1);
    if (d->left >= 0) dmax = std::min(dmax, ((long)d->left + 1) * d->chunk - 1);
    if (d->right >= 0) dmin = std::max(dmin, -(((long)d->right + 1) * d->chunk - 1));
    if (dmax >= dmin && ((long)pos_zero - dmax < 0 || (long)pos_zero - dmin > (long)n_pos - 1)) return ASR_ERR_ARG;
    if (d->head_dim % 4 != 0 || d->head_dim > 128 || E > 4096) return ASR_ERR_UNSUPPORTED;
    if (d->heads > 65535 || B > 65535) return ASR_ERR_UNSUPPORTED;                  // grid dimensions
    // key and query positions, and a block's end past them, stay inside an int
    if ((long)q_pos0 + Tq > (long)INT_MAX - 64 || (long)k_pos0 + Tk > (long)INT_MAX - 64) return ASR_ERR_UNSUPPORTED;
    if ((long)Tq * B > INT_MAX || (long)Tk * B > INT_MAX) return ASR_ERR_UNSUPPORTED;

    asr::AttnRelArgs p{};
    p.q = d_q; p.k = d_k; p.v = d_v; p.out = d_out; p.pos = d_pos; p.bias_u = d_bias_u; p.bias_v = d_bias_v;
    p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo; p.ldp = ldp;
    p.lengths = d_lengths;
    p.Tq = Tq; p.q_pos0 = q_pos0; p.Tk = Tk; p.k_pos0 = k_pos0; p.B = B;
    p.D = d->head_dim;
    p.scale = d->scale == 0.f ? 1.f / std::sqrt((float)d->head_dim) : d->scale;
    p.chunk = d->chunk; p.left = d->left; p.right = d->right;
    p.pos_zero = pos_zero;
    p.row_lo = dmax >= dmin ? (int)(pos_zero - dmax) : 0;    // no distance at all: no row is loaded
    p.row_hi = dmax >= dmin ? (int)(pos_zero - dmin) : -1;
    p.vq = asr::aligned16(d_q, ldq); p.vk = asr::aligned16(d_k, ldk);
    p.vv = asr::aligned16(d_v, ldv); p.vo = asr::aligned16(d_out, ldo);
    p.vp = asr::aligned16(d_pos, ldp);
    p.vbu = asr::aligned16(d_bias_u, 4); p.vbv = asr::aligned16(d_bias_v, 4);

    const dim3 grid((unsigned)((Tq + asr::AR_QT - 1) / asr::AR_QT), (unsigned)d->heads, (unsigned)B);
    hipStream_t st = asr_stream(s);
    switch ((d->head_dim + 15) / 16) {
        case 1: hipLaunchKernelGGL(asr::attention_rel_kernel<1>, grid, dim3(256), 0, st, p); break;
        case 2: hipLaunchKernelGGL(asr::attention_rel_kernel<2>, grid, dim3(256), 0, st, p); break;
        case 3: hipLaunchKernelGGL(asr::attention_rel_kernel<3>, grid, dim3(256), 0, st, p); break;
        case 4: hipLaunchKernelGGL(asr::attention_rel_kernel<4>, grid, dim3(256), 0, st, p); break;
        case 5: hipLaunchKernelGGL(asr::attention_rel_kernel<5>, grid, dim3(256), 0, st, p); break;
        case 6: hipLaunchKernelGGL(asr::attention_rel_kernel<6>, grid, dim3(256), 0, st, p); break;
        case 7: hipLaunchKernelGGL(asr::attention_rel_kernel<7>, grid, dim3(256), 0, st, p); break;
        default: hipLaunchKernelGGL(asr::attention_rel_kernel<8>, grid, dim3(256), 0, st, p); break;
    }
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

}  // extern "C"
