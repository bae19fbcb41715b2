// ============================================================================
// CTC prefix beam search, one WAVE per utterance (V + 1 <= 64 columns), built
// for throughput: many utterances per CU.
//
// Same semantics, state model, arithmetic and HBM node format as the
// workgroup kernel (ctc_beam_kernel.inc: CTCBeamSearch.cpp:50-187 with F1-F3,
// fp64 log domain, prefix scores L0 = lse(SNB, SB) kept per slot, orphan
// Bloom filters; DESIGN.md §2-3), so every survivor's score is the same bits
// and only the slot order (which no result depends on) differs.  What changes
// is the schedule (DESIGN.md §3c):
//   * one wave64 owns the utterance: lane r holds row r (slot r of the beam,
//     + 64k for the k-th row group).  No workgroup barrier and no cross-wave
//     exchange exist, and every uniform decision (floor, selection bins,
//     offsets) is made once, in scalar registers, instead of once per wave;
//   * candidates are generated only for LIVE labels: an extension by c scores
//     at most (best state) + ln 2 + e_c, so only the labels whose bound
//     reaches the floor G (guessed from the last frame's cutoff) are visited
//     — a handful of the V per frame on realistic emissions.  Up to NL of
//     them keep their keys in registers; further ones are regenerated in each
//     selection pass;
//   * the exact (beam+1)-th largest key comes from the 64-bin histogram
//     selection of the workgroup kernel (kth_select_all with one wave: its
//     barriers compile away), from the floor G; when fewer than K keys reach
//     G every label is visited and every column-1 fold done (exact, rare).
// The kernel is small (no per-wave column groups, no staging arrays for other
// waves): 128 VGPRs and 9.9 KB of LDS at beam <= 56, so a CU holds 16
// utterances and keeps its SIMDs busy where the workgroup kernel leaves them
// waiting on barriers and LDS round trips.
//
// The selection (wave_kth_select) and the argument why its passes on the
// keys' high words are exact are in ctc_wave_select.h.
// ============================================================================
#pragma once
#include "ctc_beam_kernel.inc"
#include "ctc_wave_select.h"

namespace asr {

// The selection histogram in two copies (even / odd lanes; the second in the
// next frame's orphan filter, zero during the selection): C4 at 16 per CU
// 9.46 -> 9.22 us per frame-step on the bench's emissions (6.07 -> 6.19 on
// sigma = 3 synthetic ones), C4 +1.1-1.6 % paired (run sr).  0: one copy (A/B).
#ifndef ASR_CTC_HIST2
#define ASR_CTC_HIST2 1
#endif
constexpr int WOFW = 64;   // orphan-filter words (2048 bits, three hashes) of the wave kernel
// live labels whose extension keys are kept in registers (measured, DESIGN.md
// §3c: 4 beats 8 and 3 — the per-label state spilled SGPRs at 8)
constexpr int WNL = 4;

// Emission frames staged per chunk: the staging is one LDS array of fp64
// logs, kept small (the LDS bounds how many utterances share a CU).
__host__ __device__ constexpr int wave_ch(int V) { return V <= 16 ? 8 : 4; }

// Child masks (bit c: the child prefix q+c is live) are 32-bit words when
// every label fits (V <= 32: C2/C4's 29), else 64-bit.
template <bool C64>
using WChild = typename std::conditional<C64, uint64_t, uint32_t>::type;

template <int KC, bool C64>
struct WLds {
    static constexpr uint32_t CB = C64 ? 8u : 4u;           // bytes per child mask
    // ---- one frame-parity buffer (the rows of a frame)
    static constexpr uint32_t H = 0;                        // u64[KC]  prefix hash
    static constexpr uint32_t HP = H + 8u * KC;             // u64[KC]  parent prefix hash
    static constexpr uint32_t SNB = HP + 8u * KC;           // f64[KC]  score of (q, not-blank)
    static constexpr uint32_t SB = SNB + 8u * KC;           // f64[KC]  score of (q, blank)
    static constexpr uint32_t SL0 = SB + 8u * KC;           // f64[KC]  prefix score lse(SNB, SB)
    static constexpr uint32_t TAIL = SL0 + 8u * KC;         // u64[KC]  packed label tail, count << 56
    static constexpr uint32_t NODE = TAIL + 8u * KC;        // i32[KC]  last flushed block (-1 = none)
    static constexpr uint32_t META = NODE + 4u * KC;        // u32[KC]  last label | flags
    static constexpr uint32_t PLINK = META + 4u * KC;       // i32[KC]  parent slot or -1
    static constexpr uint32_t OFILT = PLINK + 4u * KC;      // u32[WOFW] orphan filter (parent-prefix hashes)
    static constexpr uint32_t CHILD = OFILT + 4u * WOFW;    // u32/u64[KC] bit c: live child prefix q+c
    static constexpr uint32_t BUF = align16(CHILD + CB * KC);
    // ---- shared
    static constexpr uint32_t HIST = 2u * BUF;              // u32[64]  selection histogram (kept zeroed)
    static constexpr uint32_t EMAX = HIST + 64u * 4u;       // u64[8]   key of each staged frame's largest log emission
    static constexpr uint32_t LE = EMAX + 8u * 8u;          // f64[ch*V] log emissions of the staged chunk
    static __host__ __device__ constexpr uint32_t total(int V) { return align16(LE + 8u * wave_ch(V) * V); }
    static_assert(KC % 64 == 0 && (LE % 16) == 0, "LDS alignment");
    // Saved beam of one utterance between the segments of a segmented decode:
    // 32 bytes of scalars (P, overflow, err, best state key, gap), then the
    // image of one frame-parity buffer (slots, links, child masks, orphan filter)
    static constexpr uint32_t SEG_SCALARS = 32u;
    static constexpr uint32_t SEG = SEG_SCALARS + BUF;
    static_assert((BUF % 16) == 0, "buffer image copied as 16-byte words");
};

// Orphan filter of the wave kernel: WOFW*32 bits, three hashes (the
// workgroup kernel's ofilt_* with a smaller table: ~50 orphans per frame).
__device__ __forceinline__ void wofilt_insert(uint32_t* f, uint64_t key) {
    constexpr uint32_t M = WOFW * 32 - 1;
    const uint32_t i1 = (uint32_t)(key >> 13) & M, i2 = (uint32_t)(key >> 26) & M, i3 = (uint32_t)(key >> 39) & M;
    atomicOr(&f[i1 >> 5], 1u << (i1 & 31u));
    atomicOr(&f[i2 >> 5], 1u << (i2 & 31u));
    atomicOr(&f[i3 >> 5], 1u << (i3 & 31u));
}

__device__ __forceinline__ bool wofilt_maybe(const uint32_t* f, uint64_t key) {
    constexpr uint32_t M = WOFW * 32 - 1;
    const uint32_t i1 = (uint32_t)(key >> 13) & M, i2 = (uint32_t)(key >> 26) & M, i3 = (uint32_t)(key >> 39) & M;
    return ((f[i1 >> 5] >> (i1 & 31u)) & (f[i2 >> 5] >> (i2 & 31u)) & (f[i3 >> 5] >> (i3 & 31u)) & 1u) != 0u;
}

__device__ __forceinline__ uint32_t mbcnt64(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ double readlane_f64(double x, int l) {
    const uint64_t u = __builtin_bit_cast(uint64_t, x);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), l);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// A row's candidate state for one frame (lane r + 64k of the wave).
template <int RPT>
struct WRows {
    uint32_t meta[RPT];
    double sb[RPT], l0[RPT];
    uint64_t child[RPT];             // live child labels (zero-extended 32-bit masks)
    uint64_t kb[RPT], k1[RPT];       // keys of (q, blank) and (q, not) (k1 a lower bound while pending)
    uint64_t kx[RPT][WNL];           // extension keys of the first nl live labels
};

// The frame's candidate keys, visited by the selection helpers: the rows' own
// columns, the registered extension keys, and the extensions by the live
// labels past the first WNL, regenerated on every visit.
template <int RPT>
struct WKeys {
    const WRows<RPT>& R;
    int nl;                // registered live labels (<= WNL)
    uint64_t rest;         // live labels without registered keys
    double ev;             // lane c: log emission of label c
    template <class F>
    __device__ __forceinline__ void each(F&& f) const {
#pragma unroll
        for (int k = 0; k < RPT; k++) {
            f(R.kb[k]);
            f(R.k1[k]);
#pragma unroll
            for (int j = 0; j < WNL; j++)
                f(R.kx[k][j]);   // j >= nl: key 0, in no range
        }
        for (uint64_t m = rest; m; m &= m - 1ull) {   // uniform loop
            const int c = __builtin_ctzll(m);
            const double ec = readlane_f64(ev, c);
#pragma unroll
            for (int k = 0; k < RPT; k++) f(ext_key(k, c, ec));
        }
    }
    // (q+c, not) of row k: L0 + e_c, or SB + e_c when c repeats last(q); 0
    // when the child prefix is live (merged into its column 1) or no source
    __device__ __forceinline__ uint64_t ext_key(int k, int c, double ec) const {
        const bool taken = (R.child[k] >> c) & 1ull;
        const double base = c == (int)(R.meta[k] & META_LAST) ? R.sb[k] : R.l0[k];
        return (!taken && base > -INFINITY) ? asr_d2key(base + ec) : 0ull;
    }
};

// Child-mask bit of label `lab` set in a mask shared with other lanes (the
// bits set into one mask are distinct: 32-bit adds, see set_label_bit).
__device__ __forceinline__ void set_child_bit(uint32_t* m, uint32_t lab) { atomicAdd(m, 1u << (lab & 31u)); }
__device__ __forceinline__ void set_child_bit(uint64_t* m, uint32_t lab) { set_label_bit(m, lab); }

template <int RPT, bool C64>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(RPT == 1 ? 4 : 2)))
void ctc_wave_kernel(CtcArgs a) {
    constexpr int KC = 64 * RPT;
    using L = WLds<KC, C64>;
    using CM = WChild<C64>;
    const CtcGeom g = a.g;
    const int lane = threadIdx.x;
    const int b = blockIdx.x;
    const int V = g.V, blank = g.blank, kcap = g.kcap, K = g.K;
    const int ch = wave_ch(V);
    int4* nodes = a.nodes + (size_t)b * a.T * kcap;
    const float* ecol = a.emis + (size_t)b * a.ustride;   // frame a.t0 (segment-local)
    const size_t tstride = (size_t)a.tstride;
    const int Tb = a.lengths ? min(max(a.lengths[b], 0), a.T) : a.T;
    // this launch's frames: [t0, tend) (a whole decode: [0, Tb)); an
    // utterance that ended in an earlier segment was finalised there
    const int t0 = a.t0;
    const int tend = min(a.t1, Tb);
    if (t0 > 0 && Tb <= t0) return;
    unsigned char* const seg = a.seg_state ? a.seg_state + (size_t)b * a.seg_bytes : nullptr;

    double* lech = lds<double>(L::LE);
    uint32_t* hist = lds<uint32_t>(L::HIST);
    hist[lane] = 0u;
    for (int i = lane; i < WOFW; i += 64) {
        lds<uint32_t>(L::OFILT)[i] = 0u;
        lds<uint32_t>(L::BUF + L::OFILT)[i] = 0u;
    }
    if (t0 == 0 && lane == 0) {   // root: empty prefix in the blank state, log-score 0 (cpp:87-95)
        lds<uint64_t>(L::H)[0] = ROOT_HASH;
        lds<uint64_t>(L::HP)[0] = 0ull;
        lds<double>(L::SNB)[0] = -INFINITY;
        lds<double>(L::SB)[0] = 0.0;
        lds<double>(L::SL0)[0] = 0.0;
        lds<int>(L::NODE)[0] = -1;
        lds<uint64_t>(L::TAIL)[0] = 0ull;
        lds<uint32_t>(L::META)[0] = META_LAST | META_HAS_B;
        lds<int>(L::PLINK)[0] = -1;
        lds<CM>(L::CHILD)[0] = 0;
    }
    int P = 1;
    int overflow = 0;
    int err = 0;   // a selection ran out of passes (never expected)
    uint64_t best_state = asr_d2key(0.0);   // bounds every state's score key
    double gap = 8.0;                       // last frame's (best - cutoff) distance
    if (t0 > 0) {   // resume: the beam saved at the end of the last segment, into frame t0's buffer
        const uint4* src = reinterpret_cast<const uint4*>(seg + L::SEG_SCALARS);
        const uint32_t dst = (t0 & 1) ? L::BUF : 0u;
        for (uint32_t i = lane; i < L::BUF / 16u; i += 64u) lds<uint4>(dst)[i] = src[i];
        const int4 s0 = reinterpret_cast<const int4*>(seg)[0];
        const int4 s1 = reinterpret_cast<const int4*>(seg)[1];
        P = __builtin_amdgcn_readfirstlane(s0.x);
        overflow = __builtin_amdgcn_readfirstlane(s0.y);
        err = __builtin_amdgcn_readfirstlane(s0.z);
        best_state = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(s1.y) << 32) |
                     (uint32_t)__builtin_amdgcn_readfirstlane(s1.x);
        gap = __builtin_bit_cast(double, ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(s1.w) << 32) |
                                             (uint32_t)__builtin_amdgcn_readfirstlane(s1.z));
    }

    // emission prefetch: element e = lane + 64j of a chunk is (frame s, label v)
    float pf[4];   // ch*V <= 16*16, 8*32, 4*63: at most 256 floats, 4 per lane
    const int chunk_elems = ch * V;
    // per element: its byte offset (s * tstride + v) * 4 from the chunk's
    // first frame (the launcher checks (ch - 1) * tstride + V < 2^31 / 4), or
    // past any buffer for no element.  A chunk is read through a buffer
    // resource over its frames below tend: out-of-range elements read 0
    // (never used), and no 64-bit per-lane address is kept.
    uint32_t eoff[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int e_ = lane + 64 * j;
        const int s_ = e_ / V, v_ = e_ - s_ * V;
        eoff[j] = e_ < chunk_elems ? 4u * (uint32_t)(s_ * (int)tstride + v_) : 0x7fffffffu;
    }
#define ASR_WLOAD_CHUNK(tc)                                                                   \
    {                                                                                         \
        const float* pc_ = ecol + (size_t)((tc) - t0) * tstride;                              \
        const int nf_ = min(tend - (tc), ch);                                                 \
        const auto rs_ = __builtin_amdgcn_make_buffer_rsrc(                                   \
            const_cast<float*>(pc_), (short)0, nf_ > 0 ? ((nf_ - 1) * (int)tstride + V) * 4 : 0, \
            0x00020000);                                                                      \
        _Pragma("unroll") for (int j = 0; j < 4; j++) pf[j] = __builtin_bit_cast(             \
            float, __builtin_amdgcn_raw_buffer_load_b32(rs_, (int)eoff[j], 0, 0));             \
    }
    ASR_WLOAD_CHUNK(t0)
    // Diagnostic build only (-DASR_CTC_STAMPS): shader clock per phase,
    // summed over frames, and event counts (tools/ctc_profile.py --stamps).
#ifdef ASR_CTC_STAMPS
    uint64_t wst[16] = {};
    uint64_t wt0 = __builtin_amdgcn_s_memtime();
#define ASR_WPH(i)                                              \
    {                                                           \
        const uint64_t wt1_ = __builtin_amdgcn_s_memtime();     \
        wst[i] += wt1_ - wt0;                                   \
        wt0 = wt1_;                                             \
    }
#define ASR_WCNT(i, n) wst[i] += (uint64_t)(n)
#else
#define ASR_WPH(i) {}
#define ASR_WCNT(i, n) {}
#endif

    for (int t = t0; t < tend; t++) {
        const int si = (t - t0) % ch;
        if (si == 0) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int e = lane + 64 * j;
                if (e < chunk_elems) lech[e] = a.is_log ? (double)pf[j] : log((double)pf[j]);
            }
            if (t + ch < tend) ASR_WLOAD_CHUNK(t + ch)
            // each staged frame's largest log emission (the bound every
            // candidate of that frame shares), once per chunk: lane
            // (s, j) = (lane / gs, lane % gs) takes labels j, j + gs, ... of
            // frame s, then a max over its group of gs lanes (DPP row shifts;
            // the group's last lane holds it)
            {
                const int gs = 64 / ch;   // 16 (4 frames) or 8 (8 frames)
                const int s = lane / gs, j = lane - s * gs;
                uint64_t m = 0ull;
                for (int v = j; v < V; v += gs) {
                    const uint64_t k = asr_d2key(lech[s * V + v]);
                    m = k > m ? k : m;
                }
#define ASR_DPP_GMAX(ctrl)                                                                            \
                {                                                                                     \
                    const uint32_t lo_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)m, ctrl, \
                                                                               0xF, 0xF, true);        \
                    const uint32_t hi_ = (uint32_t)__builtin_amdgcn_update_dpp(                       \
                        0, (int)(uint32_t)(m >> 32), ctrl, 0xF, 0xF, true);                           \
                    const uint64_t y_ = ((uint64_t)hi_ << 32) | lo_;                                  \
                    m = y_ > m ? y_ : m;                                                              \
                }
                ASR_DPP_GMAX(0x111)   // row_shr:1
                ASR_DPP_GMAX(0x112)   // row_shr:2
                ASR_DPP_GMAX(0x114)   // row_shr:4
                if (gs == 16) ASR_DPP_GMAX(0x118)   // row_shr:8
#undef ASR_DPP_GMAX
                if (j == gs - 1) lds<uint64_t>(L::EMAX)[s] = m;
            }
        }
        ASR_WPH(0)   // emission staging
        const double* le = lech + si * V;
        const int cur = t & 1;
        const uint32_t bufC = cur ? L::BUF : 0u, bufN = L::BUF - bufC;
        const uint64_t* c_h = lds<uint64_t>(bufC + L::H);
        const uint64_t* c_hp = lds<uint64_t>(bufC + L::HP);
        const double* c_snb = lds<double>(bufC + L::SNB);
        const double* c_sb = lds<double>(bufC + L::SB);
        const double* c_l0 = lds<double>(bufC + L::SL0);
        const int* c_node = lds<int>(bufC + L::NODE);
        const uint64_t* c_tail = lds<uint64_t>(bufC + L::TAIL);
        const uint32_t* c_meta = lds<uint32_t>(bufC + L::META);
        const int* plC = lds<int>(bufC + L::PLINK);
        const CM* chC = lds<CM>(bufC + L::CHILD);
        const uint32_t* ofC = lds<uint32_t>(bufC + L::OFILT);
        uint64_t* n_h = lds<uint64_t>(bufN + L::H);
        uint64_t* n_hp = lds<uint64_t>(bufN + L::HP);
        double* n_snb = lds<double>(bufN + L::SNB);
        double* n_sb = lds<double>(bufN + L::SB);
        double* n_l0 = lds<double>(bufN + L::SL0);
        int* n_node = lds<int>(bufN + L::NODE);
        uint64_t* n_tail = lds<uint64_t>(bufN + L::TAIL);
        uint32_t* n_meta = lds<uint32_t>(bufN + L::META);
        int* plN = lds<int>(bufN + L::PLINK);
        CM* chN = lds<CM>(bufN + L::CHILD);
        uint32_t* ofN = lds<uint32_t>(bufN + L::OFILT);

        // ---- rows and the frame's emissions (lane c: label c)
        const double ev = lane < V ? le[lane] : -INFINITY;
        const double eb = readlane_f64(ev, blank);
        const double smaxS = asr_key2d(best_state);
        // the frame's largest log emission: a wave max over the label lanes
        const double smaxU = smaxS + asr_key2d(lds<uint64_t>(L::EMAX)[si]);
        // (a bound rounded up to an all-ones low word: ctc_wave_select.h)
        const uint64_t kmaxU = asr_d2key(smaxU + 1.1) | 0xFFFFFFFFull;
        constexpr uint64_t FLOOR1 = 1ull << 32;   // floor "1": below every present key, zero low word
        // the selection floor guessed from the last frame's cutoff distance:
        // a pure speed knob (a guess above the cutoff falls back to the exact
        // floor-1 path; 1.1 / 0.35 measured best, profiles/r03)
        const double Gd = smaxU - (1.1 * gap + 0.35);
        // (rounded down to a zero low word: ctc_wave_select.h)
        const uint64_t G = smaxU > -INFINITY ? asr_d2key(Gd) & ~0xFFFFFFFFull : FLOOR1;
        WRows<RPT> R;
        double rx[RPT], rsnb[RPT], rel[RPT];
        uint32_t pend = 0u;   // bit k: column 1 of row k has two sources (needs the exact fold)
#pragma unroll
        for (int k = 0; k < RPT; k++) {
            const int r = lane + 64 * k;
            const bool live = r < P;
            const uint32_t m_ = c_meta[r];
            const double snb_ = c_snb[r], sb_ = c_sb[r], l0_ = c_l0[r];
            const uint64_t ch_ = (uint64_t)chC[r];
            const int p = live ? plC[r] : -1;
            R.meta[k] = live ? m_ : 0u;
            rsnb[k] = live ? snb_ : -INFINITY;
            R.sb[k] = live ? sb_ : -INFINITY;
            R.l0[k] = live ? l0_ : -INFINITY;
            R.child[k] = live ? ch_ : 0ull;
            const bool hp = p >= 0;
            const uint32_t pm_ = hp ? c_meta[p] : 0u;
            const double pl0_ = hp ? c_l0[p] : -INFINITY, psb_ = hp ? c_sb[p] : -INFINITY;
            double y_;
            col1_sources(R.meta[k], rsnb[k], p, pm_, pl0_, psb_, rx[k], y_);
            rel[k] = le[min((int)(R.meta[k] & META_LAST), V - 1)];
            // (q, blank) <- L0 + e_blank: exact
            R.kb[k] = (live && R.l0[k] > -INFINITY) ? asr_d2key(R.l0[k] + eb) : 0ull;
            // (q, not) <- lse(x, y) + e_last: lower bound max(x, y) + e_last until folded
            R.k1[k] = 0ull;
            if (live && (rx[k] > -INFINITY || y_ > -INFINITY)) {
                R.k1[k] = asr_d2key(fmax(rx[k], y_) + rel[k]);
                if (rx[k] > -INFINITY && y_ > -INFINITY) pend |= 1u << k;
            }
            // the next frame's child masks (last read in frame t-1); its parent
            // links are written by each slot's builder
            chN[r] = 0;
        }
        for (int i = lane; i < WOFW; i += 64) ofN[i] = 0u;
        // an extension by c scores base + e_c with base = L0 or SB <= L0 of
        // its row: with the largest L0, an exact bound per label (rounding is
        // monotone), tighter than the selection's (best state) + ln 2
        uint64_t l0k = 0ull;
#pragma unroll
        for (int k = 0; k < RPT; k++) {
            const uint64_t x = R.l0[k] > -INFINITY ? asr_d2key(R.l0[k]) : 0ull;
            l0k = x > l0k ? x : l0k;
        }
        // the largest HIGH word with an all-ones low word: still an upper bound
        // (2^-20 relative looser), from a 32-bit DPP maximum and one readlane
        const uint32_t l0h = (uint32_t)__builtin_amdgcn_readlane((int)wave_max_u32_last((uint32_t)(l0k >> 32)), 63);
        l0k = l0h ? ((uint64_t)l0h << 32) | 0xFFFFFFFFull : 0ull;
        const double maxL0 = l0k ? asr_key2d(l0k) : -INFINITY;

        // exact folds of column 1 where the upper bound max + ln 2 reaches FILT
#define ASR_WFOLDS(FILT, LSE)                                                                     \
        _Pragma("unroll") for (int k = 0; k < RPT; k++) {                                        \
            const bool job_ = ((pend >> k) & 1u) && asr_d2key(asr_key2d(R.k1[k]) + 0.7) >= (FILT); \
            if (!__ballot(job_)) continue;                                                        \
            if (job_) {                                                                           \
                pend &= ~(1u << k);                                                               \
                R.k1[k] = asr_d2key(LSE(rx[k], rsnb[k]) + rel[k]);                                \
            }                                                                                     \
        }
        ASR_WPH(1)   // rows, own keys
        ASR_WFOLDS(G, lse2)
        ASR_WPH(2)   // folds above the floor

        // ---- live labels: an extension by c scores <= best state + ln 2 + e_c
        uint64_t tau = 1ull, ktop = 0ull;
        bool prune = false;
        int nl = 0;
        uint64_t rest = 0ull;
        int labs[WNL];
        for (int attempt = 0; attempt < 2; attempt++) {
            const uint64_t floorG = attempt ? FLOOR1 : G;
            uint64_t lm = __ballot(lane < V && lane != blank &&
                                   (attempt || asr_d2key(maxL0 + ev) >= G));
            nl = 0;
#pragma unroll
            for (int j = 0; j < WNL; j++) {
                const bool have = lm != 0ull;
                const int c = have ? __builtin_ctzll(lm) : 0;
                lm &= lm - 1ull;
                labs[j] = c;
                nl += have ? 1 : 0;
                if (have) {
                    const double ec = readlane_f64(ev, c);
#pragma unroll
                    for (int k = 0; k < RPT; k++) {
                        const bool taken = (R.child[k] >> c) & 1ull;
                        const double base = c == (int)(R.meta[k] & META_LAST) ? R.sb[k] : R.l0[k];
                        R.kx[k][j] = (!taken && base > -INFINITY) ? asr_d2key(base + ec) : 0ull;
                    }
                } else {   // absent: key 0, counted by no pass and kept by no stage
#pragma unroll
                    for (int k = 0; k < RPT; k++) R.kx[k][j] = 0ull;
                }
            }
            rest = lm;
            ASR_WCNT(8, nl);
            ASR_WCNT(9, __popcll(rest));
            ASR_WCNT(10, attempt);
            ASR_WPH(3)   // live labels, extension keys
            const WKeys<RPT> keys{R, nl, rest, ev};
            // the exact K-th largest key from the floor: exact when >= K keys reach it
            // (every pending fold below the floor has its upper bound < floor <= tau)
#if ASR_CTC_HIST2
            uint32_t* const hist2 = ofN;   // this frame's next orphan filter: zero until the builds below
#else
            uint32_t* const hist2 = nullptr;
#endif
#ifdef ASR_CTC_STAMPS
            prune = wave_kth_select(keys, K, floorG, kmaxU, hist, tau, ktop, err, hist2, wst + 12);
#else
            prune = wave_kth_select(keys, K, floorG, kmaxU, hist, tau, ktop, err, hist2);
#endif
            ASR_WPH(4)   // selection
            if (prune || attempt) break;
            // the guess was above the cutoff (or fewer than K candidates: F2):
            // every label, every fold, from floor 1
            ASR_WFOLDS(1ull, lse2_call)
        }
#undef ASR_WFOLDS
        if (!prune) tau = 1ull;   // fewer than K candidates: all survive (F2)
        if (prune) {
            const double dg = smaxU - asr_key2d(tau);
            gap = (dg >= 0.0 && dg < 1e30) ? dg : 8.0;
        }

        // ---- survivors: own prefixes first (row order), then extensions
        uint64_t smask[RPT];
        int spre[RPT];
        int nself = 0;
#pragma unroll
        for (int k = 0; k < RPT; k++) {
            const bool sb_ = R.kb[k] >= tau, snb_ = R.k1[k] >= tau;
            smask[k] = __ballot(sb_ || snb_);
            spre[k] = nself;
            nself += __popcll(smask[k]);
        }
        // the next slot of row r's own prefix (or -1)
        const auto newslot = [&](int r) -> int {
            const int kk = r >> 6, l = r & 63;
            uint64_t m = 0ull;
            int pre = 0;
#pragma unroll
            for (int k = 0; k < RPT; k++) {
                if (k == kk) { m = smask[k]; pre = spre[k]; }
            }
            if (!((m >> l) & 1ull)) return -1;
            const int idx = pre + __popcll(m & ((1ull << l) - 1ull));
            return idx < kcap ? idx : -1;
        };
        // extensions, in enumeration order, staged straight into their slots
        // of the next buffer: the score (final) into SNB, row | label << 16
        // into NODE (overwritten by the slot's builder below)
        int xtot = 0;
        {
            const auto stage = [&](uint64_t key, int r, int c) {
                const bool s = key >= tau;   // tau >= 1: an absent key (0) fails it
                const uint64_t bal = __ballot(s);
                if (s) {
                    const int i = nself + xtot + (int)mbcnt64(bal);
                    if (i < kcap) {
                        n_snb[i] = asr_key2d(key);
                        n_node[i] = r | (c << 16);
                    }
                }
                xtot += __popcll(bal);
            };
#pragma unroll
            for (int j = 0; j < WNL; j++) {   // j >= nl: key 0, nothing staged
#pragma unroll
                for (int k = 0; k < RPT; k++) stage(R.kx[k][j], lane + 64 * k, labs[j]);
            }
            const WKeys<RPT> keys{R, nl, rest, ev};
            for (uint64_t m = rest; m; m &= m - 1ull) {
                const int c = __builtin_ctzll(m);
                const double ec = readlane_f64(ev, c);
#pragma unroll
                for (int k = 0; k < RPT; k++) stage(keys.ext_key(k, c, ec), lane + 64 * k, c);
            }
        }
        const int total = nself + xtot;
        if (total > kcap) overflow = 1;
        // best state (bounds every survivor): the top of the selection's
        // highest bin, or (nothing pruned: tau = 1, every present key survives;
        // uniform and rare) the maximum key
        if (prune) {
            best_state = ktop;
        } else {
            uint64_t kbest = 0ull;
            const WKeys<RPT> keys{R, nl, rest, ev};
            keys.each([&](uint64_t x) { kbest = x > kbest ? x : kbest; });
            best_state = wave_max_u64(kbest);
        }

        ASR_WCNT(11, xtot);
        ASR_WPH(5)   // survivors staged
        // ---- own prefixes: row r's slot, built by lane r
#pragma unroll
        for (int k = 0; k < RPT; k++) {
            const int r = lane + 64 * k;
            if (!((smask[k] >> lane) & 1ull)) continue;
            const int i = spre[k] + (int)mbcnt64(smask[k]);
            if (i >= kcap) continue;
            const uint32_t m0 = R.meta[k];
            const uint32_t lab = m0 & META_LAST;
            const uint64_t kb = R.kb[k], knb = R.k1[k];
            uint32_t m = m0 & (META_LAST | META_HAS_PAR);
            m |= kb >= tau ? META_HAS_B : 0u;
            m |= knb >= tau ? META_HAS_NB : 0u;
            const double vb = kb >= tau ? asr_key2d(kb) : -INFINITY;
            const double vnb = knb >= tau ? asr_key2d(knb) : -INFINITY;
            n_sb[i] = vb;
            n_snb[i] = vnb;
            n_l0[i] = (vb > -INFINITY && vnb > -INFINITY) ? lse2(vnb, vb) : fmax(vnb, vb);
            n_node[i] = c_node[r];
            n_tail[i] = c_tail[r];
            n_meta[i] = m;
            n_h[i] = c_h[r];
            const uint64_t hp = c_hp[r];
            n_hp[i] = hp;
            const int pr = plC[r];
            const int y = pr >= 0 && pr < kcap ? newslot(pr) : -1;
            plN[i] = y;   // (or -1) before any adoption below rewrites it
            if (y >= 0) {
                set_child_bit(&chN[y], lab);
            } else if (m0 & META_HAS_PAR) {
                // an orphan next frame, unless an extension built now
                // recreates its parent (then the entry is never matched)
                wofilt_insert(ofN, hp);
            }
        }
        ASR_WPH(6)   // own prefixes built
        // ---- extensions: one per lane, slots [nself, total)
        const int xend = min(xtot, kcap - nself);
        for (int j = lane; j < xend; j += 64) {
            const int i = nself + j;
            const double vy = n_snb[i];
            const uint32_t d = (uint32_t)n_node[i];
            const int r = (int)(d & 0xFFFFu);
            const uint32_t lab = d >> 16;
            const uint64_t hr = c_h[r];
            const uint64_t tl = c_tail[r];
            const int nd = c_node[r];
            const uint64_t h = mix_hash(hr, lab);
            n_sb[i] = -INFINITY;
            n_l0[i] = vy;
            {   // append lab to the tail; the 8th label flushes a block
                const uint32_t n = (uint32_t)(tl >> 56);
                const uint64_t pk = (tl & TAIL_LABELS) | ((uint64_t)(lab & 0xFFu) << (8u * n));
                if (n == 7u) {
                    nodes[t * kcap + i] = make_int4(nd, 0, (int)(uint32_t)pk, (int)(uint32_t)(pk >> 32));
                    n_node[i] = t * kcap + i;
                    n_tail[i] = 0ull;
                } else {
                    n_node[i] = nd;
                    n_tail[i] = pk | ((uint64_t)(n + 1u) << 56);
                }
            }
            n_meta[i] = lab | META_HAS_NB | META_HAS_PAR;
            n_h[i] = h;
            n_hp[i] = hr;
            const int y = newslot(r);
            plN[i] = y;
            if (y >= 0) {
                set_child_bit(&chN[y], lab);
            } else {
                wofilt_insert(ofN, hr);
            }
            // a new prefix may recreate the parent of this frame's orphans
            if (wofilt_maybe(ofC, h)) {
                const uint64_t cm = orphan_adopt_scan(c_hp, plC, c_meta, P, h, newslot, plN, i);
                if (cm) chN[i] = (CM)cm;
            }
        }
        P = total < kcap ? total : kcap;
        ASR_WPH(7)   // extensions built
    }
#undef ASR_WLOAD_CHUNK
#undef ASR_WPH
#undef ASR_WCNT

    if (tend < Tb) {   // segmented decode, utterance not done: save the beam for the next segment
        const uint32_t src = (tend & 1) ? L::BUF : 0u;
        uint4* dst = reinterpret_cast<uint4*>(seg + L::SEG_SCALARS);
        for (uint32_t i = lane; i < L::BUF / 16u; i += 64u) dst[i] = lds<uint4>(src)[i];
        if (lane == 0) {
            reinterpret_cast<int4*>(seg)[0] = make_int4(P, overflow, err, 0);
            const uint64_t gb = __builtin_bit_cast(uint64_t, gap);
            reinterpret_cast<int4*>(seg)[1] = make_int4((int)(uint32_t)best_state, (int)(uint32_t)(best_state >> 32),
                                                        (int)(uint32_t)gb, (int)(uint32_t)(gb >> 32));
        }
        return;
    }
    // Final merge (cpp:169-187 with F3): strip the trailing blank, "q" + "q$":
    // each slot's score of "q" merged with "q$" is its L0 = lse(SNB, SB).
    const uint32_t bufC = (Tb & 1) ? L::BUF : 0u;
    for (int i = lane; i < P; i += 64) {
        a.fin_score[(size_t)b * kcap + i] = lds<double>(bufC + L::SL0)[i];
        a.fin_node[(size_t)b * kcap + i] = lds<int>(bufC + L::NODE)[i];
        a.fin_tail[(size_t)b * kcap + i] = lds<uint64_t>(bufC + L::TAIL)[i];
    }
    if (lane == 0) {
        a.fin_n[b] = P;
        a.status[b] = overflow | (err << 1);
#ifdef ASR_CTC_STAMPS
        for (int i = 0; i < NSTAMP; i++) a.stamps[(size_t)b * NSTAMP + i] = wst[i];
#endif
    }
}

}  // namespace asr
