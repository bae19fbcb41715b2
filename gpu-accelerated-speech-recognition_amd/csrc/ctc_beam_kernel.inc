// ============================================================================
// CTC prefix beam search on gfx950 — one workgroup per utterance, the whole
// beam resident on chip (LDS + registers) for all T frames.
//
// Semantics: the reference CPU decoder CTCBeamSearch.cpp:50-187 with fixes
// F1-F3 in fp64 log domain (DESIGN.md §2, SURVEY.md Appendix A):
//   * a state is (prefix q, flag ends-in-blank) — the reference's state
//     string "q" or "q$";
//   * every frame: extend all states by all labels (cpp:120-167), merge equal
//     states by log-sum-exp in the reference's std::set iteration order
//     (cpp:159-164), prune to the states scoring >= the (beam+1)-th largest
//     score (cpp:97-118 with F1/F2);
//   * finally strip the trailing blank and merge "q" with "q$" (cpp:169-187).
//
// Design (DESIGN.md §3):
//   * The beam is kept per PREFIX ("slot") in LDS: 64-bit prefix hash,
//     parent-prefix hash, last label, node id and the scores of the two
//     states (not-blank, blank).
//   * Merging is structural instead of the reference's string sort
//     (CTCBeamSearch.cu:150-172, 460-489): a target (q+c, not) can only
//     receive from (q, not), (q, blank) and (q+c, not).  Every slot keeps
//     a link to its parent prefix's slot and a mask of its live children,
//     built during compaction (structurally, plus a small hash table for
//     slots whose parent prefix is recreated), so all candidates are
//     generated with no search.  The fold order of those
//     contributions is the reference's set order ("q" < "q$" ? "qc"),
//     decided by comparing the blank's code with c's code.
//   * Candidates live in REGISTERS: thread (wave w, lane l) owns rows
//     l + 64k and the column group [w*CW, w*CW + CW).  Column 0 is the row's
//     (q, blank) state, column 1 its (q, not) state, columns 2.. its
//     extensions by the non-blank labels in label order.
//   * Prune threshold in two exact stages: the (beam+1)-th largest LOWER
//     bound (max of a candidate's contributions, no transcendentals), then
//     the exact log-sum-exp only for the multi-source candidates whose upper
//     bound (max + ln n) reaches it, then the (beam+1)-th largest exact key.
//     Selection = count the keys above a lower bound, compact the few and
//     rank them exactly; a radix pass narrows the range when too many.
//   * Survivors are compacted by one block scan; a new prefix appends one
//     label to its slot's packed tail of up to 7 labels; every 8th label
//     flushes one (parent node, 8 labels) record to a per-utterance node
//     table in HBM (node id = t*max_states + slot).  Strings are rebuilt
//     once at the end by chasing node ids (T/8 dependent loads).
//   * Emission rows are prefetched one 32-frame chunk ahead into registers
//     and staged in LDS as fp64 logs once per chunk.
// ============================================================================
#pragma once
#include "ctc_beam.h"
#include "ctc_lse.h"

namespace asr {

constexpr uint32_t META_LAST = 0xFFFFu;
constexpr uint32_t META_HAS_NB = 1u << 16;
constexpr uint32_t META_HAS_B = 1u << 17;
constexpr uint32_t META_HAS_PAR = 1u << 18;
constexpr uint64_t ROOT_HASH = 0x243F6A8885A308D3ull;
constexpr uint64_t TAIL_LABELS = (1ull << 56) - 1ull;   // packed-tail label bits
constexpr int LISTMAX = 256;   // keys ranked exactly by the selection

// Hash of prefix q+c from the hash of q.  splitmix64 finaliser (a bijection)
// of h + phi*(c+1): distinct labels under one parent never collide; distinct
// parents collide with probability ~2^-63.  Bit 0 forced to 1 so that 0 marks
// an empty hash-table cell.
__device__ __forceinline__ uint64_t mix_hash(uint64_t h, uint32_t c) {
    uint64_t x = h + 0x9E3779B97F4A7C15ull * (uint64_t)(c + 1u);
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x | 1ull;
}

// Out of line: only candidates near the cutoff need it, and inlining the fp64
// exp/log1p at every unrolled call site bloats the kernel past 256 VGPRs.
__device__ __noinline__ double lse2_call(double a, double b) { return lse2(a, b); }

// Diagnostic build only (-DASR_CTC_STAMPS, libasr_amd_stamps.so): shader
// clock per decode phase, summed over frames, per utterance.
#ifdef ASR_CTC_STAMPS
#define ASR_STAMP(i)                                          \
    do {                                                      \
        __syncthreads();                                      \
        const uint64_t now_ = __builtin_amdgcn_s_memtime();   \
        st_acc[i] += now_ - st_last;                          \
        st_last = now_;                                       \
    } while (0)
// Wave-local split (no barrier): time since the last stamp of this wave.
#define ASR_WSTAMP(i)                                         \
    do {                                                      \
        const uint64_t now_ = __builtin_amdgcn_s_memtime();   \
        st_acc[i] += now_ - st_last;                          \
        st_last = now_;                                       \
    } while (0)
#elif defined(ASR_CTC_WSTAMPS)
// Per-wave arrival times (no barrier): wt[i] = clock at point i of this
// frame; accumulated as (wt[i] - wt[0]) per wave at the end of the frame.
#define ASR_STAMP(i) do { wt[i] = __builtin_amdgcn_s_memtime(); } while (0)
#define ASR_WSTAMP(i) ASR_STAMP(i)
#else
#define ASR_STAMP(i) do {} while (0)
#define ASR_WSTAMP(i) do {} while (0)
#endif
#ifdef ASR_CTC_WSTAMPS
#define ASR_WT(i) ASR_STAMP(i)
#else
#define ASR_WT(i) do {} while (0)
#endif
// Diagnostic event counters of the stamps build (per frame, in MISC).
#ifdef ASR_CTC_STAMPS
#define ASR_COUNT(i, n) atomicAdd(lds<uint32_t>(L::MISC) + (i), (uint32_t)(n))
#else
#define ASR_COUNT(i, n) do {} while (0)
#endif

// Orphans.  A slot whose parent prefix is not live is an "orphan"; it is
// entered in its frame's orphan table under the parent-prefix hash.  When a
// new extension recreates that prefix, its builder finds the orphans there
// and links their continuations to itself (DESIGN.md §3).

// ---------------------------------------------------------------- LDS plan
// Every LDS array is addressed as smem + a 32-bit byte offset so that the
// compiler emits ds_* instructions (generic pointers lower to flat_*).
extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

// Compile-time layout for a row capacity KC = 64 x rows per thread (the
// runtime max_states is <= KC).  Offsets are constants, so every access is a
// ds_* instruction with an immediate offset from one of two uniform bases:
// the two frame-parity buffers are identical blocks BUF bytes apart.
__host__ __device__ constexpr uint32_t align16(uint32_t x) { return (x + 15u) & ~15u; }
constexpr uint32_t CHMAX = 32;   // emission frames staged per chunk, at most
constexpr int OFW = 256;         // orphan-filter words of the workgroup kernel (8192 bits)

template <int KC>
struct Lds {
    static constexpr uint32_t HT = 4u * KC;                 // orphan-table cells
    // ---- one frame-parity buffer
    static constexpr uint32_t H = 0;                        // u64[KC]  prefix hash
    static constexpr uint32_t HP = H + 8u * KC;             // u64[KC]  parent prefix hash (META_HAS_PAR)
    static constexpr uint32_t SNB = HP + 8u * KC;           // f64[KC]  score of (q, not-blank)
    static constexpr uint32_t SB = SNB + 8u * KC;           // f64[KC]  score of (q, blank)
    static constexpr uint32_t SL0 = SB + 8u * KC;           // f64[KC]  score of prefix q: lse(SNB, SB)
    static constexpr uint32_t TAIL = SL0 + 8u * KC;         // u64[KC]  labels after the last block, count << 56
    static constexpr uint32_t CHILD = TAIL + 8u * KC;       // u64[KC]  bit c: live child prefix q+c
    static constexpr uint32_t NODE = CHILD + 8u * KC;       // i32[KC]  last flushed block of q (-1 = none)
    static constexpr uint32_t META = NODE + 4u * KC;        // u32[KC]  last label | flags
    static constexpr uint32_t PLINK = META + 4u * KC;       // i32[KC]  parent slot or -1
    static constexpr uint32_t OFILT = PLINK + 4u * KC;      // u32[OFW]  orphan filter: parent-prefix hashes
    static constexpr uint32_t BUF = align16(OFILT + 4u * OFW);
    // ---- shared
    static constexpr uint32_t NEWIDX = 2u * BUF;            // i32[KC]  next-frame slot of each row's own prefix
    static constexpr uint32_t HIST = NEWIDX + 4u * KC;      // u32[3][256] radix histograms (rotating)
    static constexpr uint32_t LIST = HIST + 3u * 256u * 4u; // u64[LISTMAX] rank list
    static constexpr uint32_t RED = LIST + LISTMAX * 8u;    // u64[64]  cross-wave scratch
    static constexpr uint32_t MISC = RED + 64u * 8u;        // u64[8]   diagnostics
    static constexpr uint32_t LCOUNT = MISC + 64u;          // u32      rank-list length
    static constexpr uint32_t LMAX = LCOUNT + 16u;          // u64[CHMAX] key of each staged frame's max log emission
    static constexpr uint32_t HW = LMAX + 8u * CHMAX;       // u32[256] histogram of the one-decider selection (kept zeroed)
    static constexpr uint32_t DEC = HW + 1024u;             // u64[8]   its decision record (+ own-prefix row masks)
    static constexpr uint32_t CTR = DEC + 64u;              // u32[2]   extension slots taken, by frame parity
    static constexpr uint32_t OWNK = CTR + 16u;             // u64[KC][2] exact keys of (q, blank), (q, not) by row
    static constexpr uint32_t KCAP = KC;
    static constexpr uint32_t STG_W = 16u * KC;             // per wave: u64 key [KC]; u32 row | label << 16 [KC]
    static constexpr uint32_t STG = OWNK + 16u * KC;        // STG_W x 8 waves
    static constexpr uint32_t LE = STG + 8u * STG_W;        // f64[ch*V] log emissions of the staged chunk
    // then f32[ch*V] raw emissions of the staged chunk (offset depends on V)
    static __host__ __device__ constexpr uint32_t ebuf(int ch, int V) { return align16(LE + 8u * ch * V); }
    static __host__ __device__ constexpr uint32_t total(int ch, int V) { return align16(ebuf(ch, V) + 4u * ch * V); }
    // Timesteps mode only (asr_ctc_set_timesteps), allocated past total():
    // per frame parity TS0 u64[KC] (append frames of tail labels 0-3, 16 bits
    // each) and TS1 u64[KC] (labels 4-6); decodes without timesteps neither
    // allocate nor touch them (ADVICE r2 #4).
    static constexpr uint32_t TSPAR = 16u * KC;            // bytes per parity
    static __host__ __device__ constexpr uint32_t ts_base(int ch, int V) { return total(ch, V); }
    static __host__ __device__ constexpr uint32_t total_ts(int ch, int V) { return total(ch, V) + 2u * TSPAR; }
    static_assert(KC % 64 == 0 && (LIST % 16) == 0, "LDS alignment");
};

template <typename T>
__device__ __forceinline__ T* lds(uint32_t off) { return reinterpret_cast<T*>(smem + off); }

// ------------------------------------------------------ block-level helpers
// Cross-wave scratch (red, 64 u64): the scan uses red[32 + ph*16 .. +2*NW),
// double-buffered by a parity bit so that consecutive scans need one barrier
// each.  NW <= 8.
template <int NW>
struct Block {
    static_assert(NW >= 1 && NW <= 8, "scratch layout holds at most 8 waves");
    uint64_t* red;
    int ph;
    // Offset of this wave's run given each wave's (uniform) count n, the block
    // total, and the block max of mx — one exchange (one barrier).
    template <bool MAX = true>
    __device__ __forceinline__ int wave_offsets(int n, int& total, uint64_t& mx);
};

// Inclusive prefix sum over the 64 lanes, all in DPP (no readlane, no SALU):
// row shifts 1/2/4/8 within each 16-lane row, then the GFX9 row broadcasts —
// lane 15 of each row into the next row (rows 1 and 3), lane 31 into rows 2
// and 3.  Rows a broadcast does not write keep `old` = 0, so the add is a no-op.
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, true);   // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, true);   // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, true);   // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, true);   // row_shr:8
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);  // row_bcast:15
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);  // row_bcast:31
    return x;
}

// Max over the 64 lanes (every lane gets it): DPP row shifts on both halves,
// then the four row maxima via readlane.
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t x) {
#define ASR_DPP_MAX_STEP(ctrl)                                                                \
    {                                                                                         \
        const uint32_t lo_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)x, ctrl, \
                                                                   0xF, 0xF, true);           \
        const uint32_t hi_ = (uint32_t)__builtin_amdgcn_update_dpp(                           \
            0, (int)(uint32_t)(x >> 32), ctrl, 0xF, 0xF, true);                               \
        const uint64_t y_ = ((uint64_t)hi_ << 32) | lo_;                                      \
        x = y_ > x ? y_ : x;                                                                  \
    }
    ASR_DPP_MAX_STEP(0x111)
    ASR_DPP_MAX_STEP(0x112)
    ASR_DPP_MAX_STEP(0x114)
    ASR_DPP_MAX_STEP(0x118)
#undef ASR_DPP_MAX_STEP
    uint64_t m = 0ull;
#pragma unroll
    for (int r = 15; r < 64; r += 16) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, r);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), r);
        const uint64_t y = ((uint64_t)hi << 32) | lo;
        m = y > m ? y : m;
    }
    return m;
}

template <int NW>
template <bool MAX>
__device__ __forceinline__ int Block<NW>::wave_offsets(int n, int& total, uint64_t& mx) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t wm = MAX ? wave_max_u64(mx) : 0ull;
    if (NW == 1) {
        total = n;
        if (MAX) mx = wm;
        return 0;
    }
    uint64_t* s = red + 32 + ph * 16;
    ph ^= 1;
    if (lane == 0) { s[w] = (uint64_t)(uint32_t)n; if (MAX) s[NW + w] = wm; }
    __syncthreads();
    int off = 0, tot = 0;
    uint64_t m = 0ull;
#pragma unroll
    for (int i = 0; i < NW; i++) {
        const int c = (int)s[i];
        if (i < w) off += c;
        tot += c;
        if (MAX) {
            const uint64_t y = s[NW + i];
            m = y > m ? y : m;
        }
    }
    total = tot;
    if (MAX) mx = m;
    return off;
}

// Selection over the candidate keys held in registers (key 0 = none).
// Three 256-bin histograms rotate: pass n fills hist[n%3] and zeroes
// hist[(n+1)%3], whose last readers (pass n-2) finished before the barrier of
// pass n-1.  Every wave scans the histogram itself, so a pass costs one
// barrier and no broadcast.
struct SelScratch {
    uint32_t* hist3;   // [3][256]
    uint32_t* lcount;  // rank-list length (zeroed once per frame)
    uint64_t* list;    // [64] rank list
    int hph;
    int err;           // set if a bounded search loop ran out (never expected)
#ifdef ASR_CTC_STAMPS
    uint32_t n_pass1 = 0, n_pass2 = 0, n_rank = 0, sum_cd = 0;   // diagnostic counters
    uint64_t t_entry = 0, t_pre = 0, t_bar = 0, t_post = 0;
#endif
};

// The candidate keys a thread holds, visited by the selection helpers: a
// register array here; the wide-vocabulary kernel adds a pool key.
template <int RPT, int CW>
struct RegKeys {
    const uint64_t (&k)[RPT][CW];
    template <class F>
    __device__ __forceinline__ void each(F&& f) const {
#pragma unroll
        for (int r = 0; r < RPT; r++)
#pragma unroll
            for (int j = 0; j < CW; j++) f(k[r][j]);
    }
};

// One 8-bit radix pass over the keys in [lb, ub) (all keys <= kmax): finds
// the bucket [b0, b1) holding the need-th largest of them, its count cd, and
// how many keys lie above it.  Returns false when fewer than `need` keys are
// in range (a guessed lb was too high).  Uniform across the block.
template <int NW, class KS>
__device__ __forceinline__ bool radix_pass(const KS& keys, int need, uint64_t lb,
                                           uint64_t ub, uint64_t kmax, SelScratch& sc, uint64_t& b0,
                                           uint64_t& b1, int& cd, int& above) {
    constexpr int NT = 64 * NW;
    const int tid = threadIdx.x, lane = tid & 63;
    const uint64_t hiK = (ub - 1ull) < kmax ? (ub - 1ull) : kmax;
    const int top = 63 - __clzll((long long)(hiK ^ lb));   // caller ensures hiK > lb
    const int lo = top - 7 > 0 ? top - 7 : 0;
    const uint64_t dmask = (1ull << (top - lo + 1)) - 1ull;
#ifdef ASR_CTC_STAMPS
    sc.t_entry = __builtin_amdgcn_s_memtime();
#endif
    uint32_t* hist = sc.hist3 + 256 * sc.hph;
    uint32_t* hzero = sc.hist3 + 256 * (sc.hph == 2 ? 0 : sc.hph + 1);
    sc.hph = sc.hph == 2 ? 0 : sc.hph + 1;
    keys.each([&](uint64_t x) {
        if (x >= lb && x < ub) atomicAdd(&hist[(uint32_t)((x >> lo) & dmask)], 1u);
    });
    for (int i = tid; i < 256; i += NT) hzero[i] = 0u;
#ifdef ASR_CTC_STAMPS
    const uint64_t rt0_ = __builtin_amdgcn_s_memtime();
#endif
    __syncthreads();
#ifdef ASR_CTC_STAMPS
    const uint64_t rt1_ = __builtin_amdgcn_s_memtime();
#endif
    // lane l owns bins 4(63-l) .. 4(63-l)+3, so the lane prefix sum is a
    // suffix sum over the bins (largest keys first).
    const uint4 c4 = reinterpret_cast<const uint4*>(hist)[63 - lane];
    const uint32_t s = c4.x + c4.y + c4.z + c4.w;
    const uint32_t S = wave_incl_scan(s);
#ifdef ASR_CTC_STAMPS
    sc.t_bar += rt1_ - rt0_;
    sc.t_pre += rt0_ - sc.t_entry;
#endif
    if ((uint32_t)__builtin_amdgcn_readlane((int)S, 63) < (uint32_t)need) return false;
    const uint64_t hit = __ballot(S >= (uint32_t)need);
    const int L = __builtin_ctzll(hit);   // first lane whose suffix reaches need
    const uint32_t SL = (uint32_t)__builtin_amdgcn_readlane((int)S, L);
    const uint32_t sL = (uint32_t)__builtin_amdgcn_readlane((int)s, L);
    uint4 cL;   // lane L's four bins, from registers (no second LDS round trip)
    cL.x = (uint32_t)__builtin_amdgcn_readlane((int)c4.x, L);
    cL.y = (uint32_t)__builtin_amdgcn_readlane((int)c4.y, L);
    cL.z = (uint32_t)__builtin_amdgcn_readlane((int)c4.z, L);
    cL.w = (uint32_t)__builtin_amdgcn_readlane((int)c4.w, L);
    uint32_t ab = SL - sL, c;
    int d;
    if (ab + cL.w >= (uint32_t)need) { d = 3; c = cL.w; }
    else if (ab + cL.w + cL.z >= (uint32_t)need) { d = 2; c = cL.z; ab += cL.w; }
    else if (ab + cL.w + cL.z + cL.y >= (uint32_t)need) { d = 1; c = cL.y; ab += cL.w + cL.z; }
    else { d = 0; c = cL.x; ab += cL.w + cL.z + cL.y; }
    cd = (int)c;
    above = (int)ab;
    const uint64_t base = top + 1 >= 64 ? 0ull : (lb >> (top + 1)) << (top + 1);   // common prefix
    b0 = base | ((uint64_t)(4 * (63 - L) + d) << lo);
    b1 = b0 + (1ull << lo);
    b0 = b0 > lb ? b0 : lb;
    if (!(b1 > b0 && b1 < ub)) b1 = ub;   // b1 <= b0: carried past 2^64
#ifdef ASR_CTC_STAMPS
    sc.t_post += __builtin_amdgcn_s_memtime() - rt1_;
#endif
    return true;
}

// A lower bound of the need-th largest key: the floor of its radix bucket
// (one pass).  lb: a guess below kmax (retried from 1 when too high); kmax:
// an upper bound of every key.  Returns false when there are fewer than
// `need` keys in all (then nothing is pruned).
template <int NW, bool RETRY = true, class KS>
__device__ __forceinline__ bool kth_lower_bound(const KS& keys, int need,
                                                uint64_t lb, uint64_t kmax, SelScratch& sc,
                                                uint64_t& tauL) {
    uint64_t b0, b1;
    int cd, above;
    tauL = 1ull;
    if (kmax <= 1ull) return false;   // no key can exist (all are 0)
    if (lb >= kmax) lb = 1ull;
#ifdef ASR_CTC_STAMPS
    sc.n_pass1++;
#endif
    if (radix_pass<NW>(keys, need, lb, ~0ull, kmax, sc, b0, b1, cd, above)) {
        tauL = b0;
        return true;
    }
    if (!RETRY || lb == 1ull) return false;
#ifdef ASR_CTC_STAMPS
    sc.n_pass1++;
#endif
    if (radix_pass<NW>(keys, need, 1ull, ~0ull, kmax, sc, b0, b1, cd, above)) {
        tauL = b0;
        return true;
    }
    return false;
}

// The exact need-th largest key, as a threshold tau: the survivors are
// exactly the keys >= tau.  lb must be a proven lower bound of the answer.
// Radix passes shrink [lb, ub) to the answer's bucket; once that holds <= 64
// keys they are appended to a list and every wave ranks them with shuffles.
// kth_exact_from: the same from a floor lb that is only a guess: returns
// false (no error) when fewer than `need` keys are >= lb, else true and tau.
template <int NW, class KS>
__device__ __forceinline__ bool kth_exact_from(const KS& keys, int need, uint64_t lb, uint64_t kmax,
                                               SelScratch& sc, uint64_t& tau) {
    const int lane = threadIdx.x & 63;
    uint64_t ub = ~0ull;
    tau = lb;
    for (int it = 0;; it++) {   // each pass fixes 8 more key bits: <= 8 passes
        if (it == 9) { sc.err = 1; return true; }
        const uint64_t hiK = (ub - 1ull) < kmax ? (ub - 1ull) : kmax;
        if (hiK <= lb) {   // a single key value remains (after a pass: the answer)
            tau = lb;
            return it > 0;   // on entry nothing was counted: let the caller fall back
        }
        uint64_t b0, b1;
        int cd, above;
#ifdef ASR_CTC_STAMPS
        sc.n_pass2++;
#endif
        if (!radix_pass<NW>(keys, need, lb, ub, kmax, sc, b0, b1, cd, above)) {
            if (it == 0) return false;   // the floor was above the answer
            sc.err = 1;
            return true;
        }
        need -= above;
        lb = b0;
        ub = b1;
        if (cd == need) { tau = lb; return true; }   // the whole bucket survives
        if (cd > 64) continue;
#ifdef ASR_CTC_STAMPS
        sc.n_rank++;
        sc.sum_cd += (uint32_t)cd;
#endif
        keys.each([&](uint64_t x) {
            if (x >= lb && x < ub) sc.list[atomicAdd(sc.lcount, 1u)] = x;
        });
        // zero-pad the list to a multiple of 8 (a 0 key never outranks one)
        const int cd8 = (cd + 7) & ~7;
        if ((int)threadIdx.x >= cd && (int)threadIdx.x < cd8) sc.list[threadIdx.x] = 0ull;
        __syncthreads();
        // rank: every lane reads the whole list (LDS broadcast, two keys per
        // 16-byte load, 8 keys per step so the loads pipeline)
        const uint64_t e = lane < cd ? sc.list[lane] : 0ull;
        int gt = 0, ge = 0;
        const uint4* l4 = reinterpret_cast<const uint4*>(sc.list);
        for (int x = 0; x < cd8 / 2; x += 4) {
            uint4 q[4];
#pragma unroll
            for (int u = 0; u < 4; u++) q[u] = l4[x + u];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint64_t v0 = ((uint64_t)q[u].y << 32) | q[u].x;
                const uint64_t v1 = ((uint64_t)q[u].w << 32) | q[u].z;
                gt += (v0 > e) + (v1 > e);
                ge += (v0 >= e) + (v1 >= e);
            }
        }
        const uint64_t hit = __ballot(lane < cd && gt < need && need <= ge);
        if (hit == 0ull) { sc.err = 1; tau = lb; return true; }
        const int L = __builtin_ctzll(hit);
        const uint32_t lo32 = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)e, L);
        const uint32_t hi32 = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(e >> 32), L);
        tau = ((uint64_t)hi32 << 32) | lo32;
        return true;
    }
}

// The exact need-th largest key as a threshold tau (survivors: keys >= tau),
// with ONE wave making every decision: all waves add their keys in [lo, hi]
// to a 256-bin histogram (largest keys first), then wave 0 alone scans it,
// picks the bin holding the need-th key and publishes its decision (done /
// rank the bin / narrow to the bin) in dec[]; the other waves wait at the
// barrier.  Uniform work is done once instead of once per wave (8 waves on
// the CU's one scalar unit and 2 waves per SIMD made it the costliest phase).
// lb: a floor (a guess); returns false when fewer than need keys are >= lb.
// ktop: top of the first pass's highest non-empty bin, a bound of the best key.
// own(tau, dec + 4): wave 0 publishes whatever the other waves need from the
// final cutoff with the decision (the own-prefix survivor masks).
struct NoOwn {
    __device__ void operator()(uint64_t, uint64_t*) const {}
};

template <int NW, class KS, class OWN = NoOwn>
__device__ bool kth_select_w0(const KS& keys, int need, uint64_t lb, uint64_t kmax, SelScratch& sc,
                              uint32_t* hist, uint64_t* dec, uint64_t& tau, uint64_t& ktop,
                              const OWN& own = OWN{}) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (kmax < lb) return false;
    uint64_t lo = lb, hi = kmax;   // inclusive range that holds the answer
    for (int pass = 0; pass < 9; pass++) {
#ifdef ASR_CTC_STAMPS
        sc.n_pass2++;
#endif
        const uint64_t span = hi - lo;
        const int top = span ? 63 - __clzll((long long)span) : 0;
        const int sh = top > 7 ? top - 7 : 0;
        keys.each([&](uint64_t x) {
            if (x >= lo && x <= hi) atomicAdd(&hist[255u - (uint32_t)((x - lo) >> sh)], 1u);
        });
        __syncthreads();
        if (w == 0) {
            uint4* h4 = reinterpret_cast<uint4*>(hist);
            const uint4 c4 = h4[lane];                 // bins 4l..4l+3 from the largest keys
            h4[lane] = make_uint4(0u, 0u, 0u, 0u);    // zeroed for the next pass
            const uint32_t s = c4.x + c4.y + c4.z + c4.w;
            const uint32_t S = wave_incl_scan(s);
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)S, 63);
            uint64_t code, b0 = lo, b1 = hi, kt = 0ull;
            int nneed = need;
            if (pass == 0) {   // highest non-empty bin
                const uint64_t nz = __ballot(s != 0u);
                if (nz) {
                    const int Lz = __builtin_ctzll(nz);
                    const uint32_t dz = c4.x ? 0u : (c4.y ? 1u : (c4.z ? 2u : 3u));
                    const uint32_t bz = 255u - (uint32_t)__builtin_amdgcn_readlane((int)(4u * lane + dz), Lz);
                    const uint64_t t0 = lo + ((uint64_t)bz << sh) + ((1ull << sh) - 1ull);
                    kt = (t0 > hi || t0 < lo) ? hi : t0;
                }
            }
            if (total < (uint32_t)need) {
                code = 0;   // fewer than need keys in range
            } else {
                const int L = __builtin_ctzll(__ballot(S >= (uint32_t)need));
                const uint32_t ex = S - s;
                const uint32_t c0 = ex + c4.x, c1 = c0 + c4.y, c2 = c1 + c4.z;
                const uint32_t nd = (uint32_t)need;
                const uint32_t d = c0 >= nd ? 0u : (c1 >= nd ? 1u : (c2 >= nd ? 2u : 3u));
                const uint32_t above = d == 0u ? ex : (d == 1u ? c0 : (d == 2u ? c1 : c2));
                const uint32_t cnt = d == 0u ? c4.x : (d == 1u ? c4.y : (d == 2u ? c4.z : c4.w));
                const uint32_t binTop = (uint32_t)__builtin_amdgcn_readlane((int)(4u * lane + d), L);
                const int ab = __builtin_amdgcn_readlane((int)above, L);
                const int cd = __builtin_amdgcn_readlane((int)cnt, L);
                b0 = lo + ((uint64_t)(255u - binTop) << sh);
                b1 = b0 + ((1ull << sh) - 1ull);
                if (b1 > hi || b1 < b0) b1 = hi;
                nneed = need - ab;
                code = (cd == nneed || sh == 0) ? 1 : (cd <= 64 ? 3 : 2);
                if (code == 1) own(b0, dec + 4);
            }
            if (lane == 0) {
                dec[0] = code | ((uint64_t)(uint32_t)nneed << 8);
                dec[1] = b0;
                dec[2] = b1;
                dec[3] = kt;
            }
        }
        __syncthreads();
        const uint64_t d0 = dec[0];
        const int code = (int)(d0 & 0xFF);
        const uint64_t b0 = dec[1], b1 = dec[2];
        if (pass == 0) ktop = dec[3];
        if (code == 0) {
            if (pass == 0) return false;
            sc.err = 1;
            tau = lo;
            return true;
        }
        need = (int)(uint32_t)(d0 >> 8);
        if (code == 1) { tau = b0; return true; }   // the whole bin survives / one key value
        lo = b0;
        hi = b1;
        if (code == 2) continue;
        // rank the bin's keys (<= 64): every wave lists its keys, wave 0 ranks
#ifdef ASR_CTC_STAMPS
        sc.n_rank++;
#endif
        keys.each([&](uint64_t x) {
            if (x >= lo && x <= hi) sc.list[atomicAdd(sc.lcount, 1u)] = x;
        });
        __syncthreads();
        if (w == 0) {
            const int nr = (int)*sc.lcount;
            const int n8 = (nr + 7) & ~7;
            if (lane >= nr && lane < n8) sc.list[lane] = 0ull;   // a 0 key never outranks one
            const uint64_t e = lane < nr ? sc.list[lane] : 0ull;
            int gt = 0, ge = 0;
            const uint4* l4 = reinterpret_cast<const uint4*>(sc.list);
            for (int x = 0; x < n8 / 2; x += 4) {
                uint4 q[4];
#pragma unroll
                for (int u = 0; u < 4; u++) q[u] = l4[x + u];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const uint64_t v0 = ((uint64_t)q[u].y << 32) | q[u].x;
                    const uint64_t v1 = ((uint64_t)q[u].w << 32) | q[u].z;
                    gt += (v0 > e) + (v1 > e);
                    ge += (v0 >= e) + (v1 >= e);
                }
            }
            const uint64_t hit = __ballot(lane < nr && gt < need && need <= ge);
            uint64_t tv = lo;
            if (hit) {
                const int H = __builtin_ctzll(hit);
                tv = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(e >> 32), H) << 32) |
                     (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)e, H);
            }
            own(tv, dec + 4);
            if (lane == 0) {
                dec[1] = tv;
                dec[0] = hit ? 0ull : 1ull;
            }
        }
        __syncthreads();
        tau = dec[1];
        if (dec[0]) { sc.err = 1; tau = lo; }
        return true;
    }
    sc.err = 1;
    tau = lo;
    return true;
}

// The need-th largest key as a threshold tau (survivors: keys >= tau) with
// EVERY wave deciding: a pass adds the keys in [lo, hi] to a 64-bin LDS
// histogram (one bin per lane, largest keys in lane 0), and after its one
// barrier every wave reads the 64 counts, scans them with DPP and finds the
// bin holding the need-th key itself — the same decision in all waves, so
// there is no decider, no published decision and no second barrier.  A bin
// that holds exactly the keys still needed (or a single key value) ends the
// search; otherwise the next pass splits that bin 64 ways (usually two passes
// in all).  Three histograms rotate (pass n fills h[n%3] and zeroes
// h[(n+1)%3], whose readers finished before pass n-1's barrier; the rotation
// continues across frames through hph).  lb: a floor (a guess): returns false
// when fewer than need keys are >= lb.  ktop: top of the first pass's highest
// non-empty bin, a bound of the best key.
template <int NW, class KS>
__device__ __forceinline__ bool kth_select_all(const KS& keys, int need, uint64_t lb, uint64_t kmax,
                                               uint32_t* hist3, int& hph, uint64_t& tau, uint64_t& ktop,
                                               SelScratch& sc, uint64_t* wts = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63;
    if (kmax < lb) return false;
    uint64_t lo = lb, hi = kmax;   // inclusive range that holds the answer
    for (int pass = 0; pass < 12; pass++) {
#ifdef ASR_CTC_STAMPS
        sc.n_pass2++;
#endif
        const uint64_t span = hi - lo;
        const int top = span ? 63 - __clzll((long long)span) : 0;
        const int sh = top > 5 ? top - 5 : 0;   // span >> sh < 64
        uint32_t* h = hist3 + 64 * hph;
        uint32_t* hz = hist3 + 64 * (hph == 2 ? 0 : hph + 1);
        hph = hph == 2 ? 0 : hph + 1;
#ifdef ASR_CTC_WSTAMPS
        if (pass == 0) wts[11] = __builtin_amdgcn_s_memtime();
#endif
        keys.each([&](uint64_t x) {
            const uint64_t d = x - lo;   // x in [lo, hi] <=> x - lo <= span (unsigned)
            if (d <= span) atomicAdd(&h[63u - (uint32_t)(d >> sh)], 1u);
        });
        if (tid < 64) hz[tid] = 0u;
#ifdef ASR_CTC_WSTAMPS
        if (pass == 0) wts[12] = __builtin_amdgcn_s_memtime();
#endif
        __syncthreads();
#ifdef ASR_CTC_WSTAMPS
        if (pass == 0) wts[13] = __builtin_amdgcn_s_memtime();
#endif
        const uint32_t c = h[lane];
        const uint32_t S = wave_incl_scan(c);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)S, 63);
        if (pass == 0) {   // highest non-empty bin
            const uint64_t nz = __ballot(c != 0u);
            if (nz) {
                const int Lz = __builtin_ctzll(nz);
                const uint64_t t0 = lo + ((uint64_t)(64 - Lz) << sh) - 1ull;
                ktop = (t0 > hi || t0 < lo) ? hi : t0;
            }
        }
        if (total < (uint32_t)need) {
            if (pass == 0) return false;   // fewer than need keys >= the floor
            sc.err = 1;
            tau = lo;
            return true;
        }
        const int L = __builtin_ctzll(__ballot(S >= (uint32_t)need));
        const uint32_t cd = (uint32_t)__builtin_amdgcn_readlane((int)c, L);
        const uint32_t SL = (uint32_t)__builtin_amdgcn_readlane((int)S, L);
        const uint64_t b0 = lo + ((uint64_t)(63 - L) << sh);
        uint64_t b1 = b0 + ((1ull << sh) - 1ull);
        if (b1 > hi || b1 < b0) b1 = hi;
        need -= (int)(SL - cd);
#ifdef ASR_CTC_WSTAMPS
        if (pass == 0) wts[14] = __builtin_amdgcn_s_memtime();
#endif
        if ((int)cd == need || sh == 0 || b1 == b0) {   // the whole bin survives / one key value
            tau = b0;
            return true;
        }
        lo = b0;
        hi = b1;
    }
    sc.err = 1;
    tau = lo;
    return true;
}

// The exact need-th largest key; lb must be a proven lower bound of it.
template <int NW, class KS>
__device__ __forceinline__ uint64_t kth_exact(const KS& keys, int need, uint64_t lb, uint64_t kmax,
                                              SelScratch& sc) {
    if (kmax <= lb) return lb;   // every key >= lb equals lb: that is the answer
    uint64_t tau;
    if (!kth_exact_from<NW>(keys, need, lb, kmax, sc, tau)) { sc.err = 1; return lb; }
    return tau;
}

// Contributions to column 1 of a row, (q, not): the parent's extension by
// last(q) (when the parent prefix is live) and the collapse q+last(q) -> q, in
// the reference's set order: "p" < {"p$", "pc"} with "p$" < "pc" iff
// code(blank) < code(c) (cpp:125-164).  Returns how many exist.  Used by
// the list and wide-vocabulary kernels, which fold per contribution.
__device__ __forceinline__ int col1_contribs(uint32_t meta, double snb, int p, uint32_t pmeta,
                                             double psnb, double psb, double e,
                                             bool bl, double& v0, double& v1, double& v2) {
    // Branch-free: a lambda writing through references with a dynamic count
    // makes a stack object (scratch), whose reload waits on vmcnt(0) and so
    // drains the emission prefetch.
    const bool hasnb = meta & META_HAS_NB;
    const int last = (int)(meta & META_LAST);
    if (p < 0 && !hasnb) return 0;
    const bool hA = p >= 0 && (pmeta & META_HAS_NB) && (int)(pmeta & META_LAST) != last;
    const bool hB = p >= 0 && (pmeta & META_HAS_B);
    // bl: code(blank) < code(last), i.e. "p$" < "pc"
    const double A = psnb + e, Bv = psb + e, C = snb + e;
    // ordered slots: A, then B before C iff "p$" < "pc"
    const double x1 = bl ? Bv : C, x2 = bl ? C : Bv;
    const bool f1 = bl ? hB : hasnb, f2 = bl ? hasnb : hB;
    v0 = hA ? A : (f1 ? x1 : x2);
    v1 = hA ? (f1 ? x1 : x2) : x2;
    v2 = x2;
    return (int)hA + (int)f1 + (int)f2;
}

// The two sources of column 1 of a row, (q, not) with l = last(q), before
// the emission e_l they all take: x from the parent prefix p (its prefix
// score L0_p = lse(SNB_p, SB_p) when last(p) != l, else only (p, blank): the
// (p, not) + l path collapses into p itself), y = (q, not) repeating l
// (cpp:125-164).  The exact candidate is lse(x, y) + e_l — the reference's
// fold of the three contributions in set order up to rounding.
__device__ __forceinline__ void col1_sources(uint32_t meta, double snb, int p, uint32_t pmeta,
                                             double pl0, double psb, double& x, double& y) {
    const int last = (int)(meta & META_LAST);
    x = p >= 0 ? ((int)(pmeta & META_LAST) != last ? pl0 : psb) : -INFINITY;
    y = (meta & META_HAS_NB) ? snb : -INFINITY;
}

// Set bit `lab` of a 64-bit label mask shared with other lanes.  The bits
// set into one mask are always distinct (one per child prefix), so a 32-bit
// add is an OR; LDS coalesces same-address 32-bit adds, whereas same-address
// OR/MAX and 64-bit atomics serialise lane by lane (~70 cycles each).
__device__ __forceinline__ void set_label_bit(uint64_t* mask, uint32_t lab) {
    atomicAdd(reinterpret_cast<uint32_t*>(mask) + ((lab >> 5) & 1u), 1u << (lab & 31u));
}

// Orphan tables are bucketed: 8 cells (64 bytes of keys) per bucket, read at
// once, so a lookup is one round of loads and compares instead of a
// dependent probe chain (a divergent probe loop runs as long as its longest
// lane).  A cell is claimed with a 32-bit add on the bucket's counter (LDS
// coalesces those; no CAS retries); a full bucket spills into the next one.
// Home bucket from the high bits (bit 0 of every hash is forced to 1).
constexpr int OBK = 8;

__device__ __forceinline__ uint32_t home_bucket(uint64_t key, uint32_t bmask) {
    return (uint32_t)(key >> 40) & bmask;
}

// Enter orphan slot `slot` (last label `last`) under parent-prefix hash key.
// Never fills: <= kcap entries in 4*kcap cells.
__device__ __forceinline__ void orphan_insert(uint64_t* okey, uint32_t* opay, uint32_t* ocnt,
                                              uint32_t bmask, uint64_t key, int slot,
                                              uint32_t last) {
    uint32_t bkt = home_bucket(key, bmask);
    for (uint32_t n = 0; n <= bmask; n++) {
        const uint32_t c = atomicAdd(&ocnt[bkt], 1u);
        if (c < (uint32_t)OBK) {
            okey[bkt * OBK + c] = key;
            opay[bkt * OBK + c] = (uint32_t)slot | (last << 16);
            return;
        }
        bkt = (bkt + 1u) & bmask;
    }
}

// The builder of new prefix h (slot idx) adopts this frame's orphans whose
// parent prefix it recreates: links each orphan's continuation (newidx) to
// idx and returns idx's child-label mask.
template <class NI>
__device__ __forceinline__ uint64_t orphan_adopt_f(const uint64_t* okey, const uint32_t* opay,
                                                   const uint32_t* ocnt, uint32_t bmask, uint64_t h,
                                                   NI&& newslot, int kcap, int* plN, int idx) {
    uint64_t mask = 0ull;
    uint32_t bkt = home_bucket(h, bmask);
    for (uint32_t n = 0; n <= bmask; n++) {
        const uint32_t cnt = ocnt[bkt];
        const uint4* kp = reinterpret_cast<const uint4*>(okey + bkt * OBK);
        uint32_t hits = 0u;
#pragma unroll
        for (int i = 0; i < OBK / 2; i++) {
            const uint4 v = kp[i];
            hits |= (((uint64_t)v.y << 32) | v.x) == h && (uint32_t)(2 * i) < cnt ? 1u << (2 * i) : 0u;
            hits |= (((uint64_t)v.w << 32) | v.z) == h && (uint32_t)(2 * i + 1) < cnt ? 2u << (2 * i) : 0u;
        }
        while (hits) {   // usually none; siblings share a bucket
            const int c = __builtin_ctz(hits);
            hits &= hits - 1u;
            const uint32_t pay = opay[bkt * OBK + c];
            const int o = (int)(pay & 0xFFFFu);
            const int ni = o < kcap ? newslot(o) : -1;
            if (ni >= 0) {
                plN[ni] = idx;
                mask |= 1ull << ((pay >> 16) & 63u);
            }
        }
        if (cnt < (uint32_t)OBK) break;
        bkt = (bkt + 1u) & bmask;
    }
    return mask;
}

__device__ __forceinline__ uint64_t orphan_adopt(const uint64_t* okey, const uint32_t* opay,
                                                 const uint32_t* ocnt, uint32_t bmask, uint64_t h,
                                                 const int* newidx, int kcap, int* plN, int idx) {
    return orphan_adopt_f(okey, opay, ocnt, bmask, h, [&](int o) { return newidx[o]; }, kcap, plN, idx);
}

// Orphans of the workgroup kernel, round 2.  Counted on the bench's emissions
// (stamps build): ~50 orphans per C2 frame (the beam turns over almost
// entirely, so nearly every survivor's parent prefix dies) and ~0 adoptions.
// So an orphan is only MARKED, in an 8192-bit Bloom filter of parent-prefix
// hashes (three bits, non-returning ds_or: no returning atomics, no entries),
// and the builder of a new prefix tests its own hash against last frame's
// filter; only on a hit (an adoption, or a false positive: ~5e-5 per lookup
// at 100 orphans) does it scan the current rows for orphans (HAS_PAR, no
// parent link) whose parent hash is its own.  The orphans' data is in their
// slots already.
__device__ __forceinline__ void ofilt_insert(uint32_t* f, uint64_t key) {
    const uint32_t i1 = (uint32_t)(key >> 13) & 8191u, i2 = (uint32_t)(key >> 26) & 8191u,
                   i3 = (uint32_t)(key >> 39) & 8191u;
    atomicOr(&f[i1 >> 5], 1u << (i1 & 31u));
    atomicOr(&f[i2 >> 5], 1u << (i2 & 31u));
    atomicOr(&f[i3 >> 5], 1u << (i3 & 31u));
}

__device__ __forceinline__ bool ofilt_maybe(const uint32_t* f, uint64_t key) {
    const uint32_t i1 = (uint32_t)(key >> 13) & 8191u, i2 = (uint32_t)(key >> 26) & 8191u,
                   i3 = (uint32_t)(key >> 39) & 8191u;
    return ((f[i1 >> 5] >> (i1 & 31u)) & (f[i2 >> 5] >> (i2 & 31u)) & (f[i3 >> 5] >> (i3 & 31u)) & 1u) != 0u;
}

// The builder of new prefix h (slot idx) adopts the current rows that are
// orphans of h: links each one's continuation (newslot) to idx and returns
// idx's child-label mask.
template <class NI>
__device__ __forceinline__ uint64_t orphan_adopt_scan(const uint64_t* c_hp, const int* plC, const uint32_t* c_meta,
                                                   int P, uint64_t h, NI newslot, int* plN, int idx) {
    // rare (a hit of the filter): a plain loop, so that it costs no registers
    uint64_t mask = 0ull;
#pragma nounroll
    for (int r = 0; r < P; r++) {
        if (c_hp[r] != h || plC[r] >= 0) continue;
        const uint32_t m = c_meta[r];
        if (!(m & META_HAS_PAR)) continue;
        const int ni = newslot(r);
        if (ni >= 0) {
            plN[ni] = idx;
            mask |= 1ull << (m & 63u);
        }
    }
    return mask;
}

// ------------------------------------------------------------ main kernel
// The 4-wave kernels that fit a 168-VGPR budget with (almost)
// no spills — CW <= 8 columns at one row per thread, or CW <= 2 at up to two
// — are compiled for three waves per SIMD, so that THREE 4-wave workgroups
// share a CU (measured at C4's batch, bench emissions, T = 300: 0.66
// utterance-frames per us per CU at three per CU vs 0.51 at two, 188 ->
// 167 VGPRs with 4 spilled; alone on a CU unchanged, 3.51 vs 3.56 us per
// frame).  runtime.hip auto_waves reads the resulting fit from the
// occupancy query.
template <int NW, int CW, int RPT, bool CU>
constexpr int ctc_waves_per_eu() {
    return (NW == 4 && !CU && ((CW <= 8 && RPT == 1) || (CW <= 2 && RPT <= 2))) ? 3 : 1;
}
template <int NW, int CW, int RPT, bool CU>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(ctc_waves_per_eu<NW, CW, RPT, CU>())))
void ctc_beam_kernel(CtcArgs a) {
    constexpr int NT = 64 * NW;
    constexpr int PF = 16 / NW;   // prefetch registers per thread: a chunk is <= 1024 floats
    const CtcGeom g = a.g;
    using L = Lds<64 * RPT>;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.x;
    const int V = g.V, blank = g.blank, kcap = g.kcap, ch = g.ch, K = g.K;
    const int R = V + 1;
    int4* nodes = a.nodes + (size_t)b * a.T * kcap;
    const float* ecol = a.emis + (size_t)b * a.ustride;  // utterance b's row at t=0
    const size_t tstride = (size_t)a.tstride;            // floats between frames
    const int Tb = a.lengths ? min(max(a.lengths[b], 0), a.T) : a.T;   // this utterance's frames

    double* lech = lds<double>(L::LE);
    int* newidx = lds<int>(L::NEWIDX);
    uint32_t* hist = lds<uint32_t>(L::HIST);
    Block<NW> blk{lds<uint64_t>(L::RED), 0};
    SelScratch sc{hist, lds<uint32_t>(L::LCOUNT), lds<uint64_t>(L::LIST), 0, 0};
    for (int i = tid; i < 768; i += NT) hist[i] = 0u;
    for (int i = tid; i < 256; i += NT) lds<uint32_t>(L::HW)[i] = 0u;
    if (tid < 2) lds<uint32_t>(L::CTR)[tid] = 0u;

    // Root slot: empty prefix in the blank state with log-score 0.  One
    // extend+prune from it is exactly initialPath + prune (cpp:87-95).
    for (int i = tid; i < OFW; i += NT) lds<uint32_t>(L::OFILT)[i] = 0u;
    __syncthreads();
    if (tid == 0) {
        lds<uint64_t>(L::H)[0] = ROOT_HASH;
        lds<uint64_t>(L::HP)[0] = 0ull;
        lds<double>(L::SNB)[0] = -INFINITY;
        lds<double>(L::SB)[0] = 0.0;
        lds<double>(L::SL0)[0] = 0.0;
        lds<int>(L::NODE)[0] = -1;
        lds<uint64_t>(L::TAIL)[0] = 0ull;
        if (a.nodes_ts) {
            lds<uint64_t>(L::ts_base(ch, V))[0] = 0ull;
            lds<uint64_t>(L::ts_base(ch, V) + 8u * (64 * RPT))[0] = 0ull;
        }
        lds<uint32_t>(L::META)[0] = META_LAST | META_HAS_B;
        lds<int>(L::PLINK)[0] = -1;
        lds<uint64_t>(L::CHILD)[0] = 0ull;
        for (int k_ = 0; k_ < 6; k_++) lds<uint32_t>(L::MISC)[k_] = 0u;
    }
    int P = 1;
    int overflow = 0;
    int hph_all = 0;   // histogram rotation of kth_select_all (uniform)
    uint64_t best_state = asr_d2key(0.0);   // key of the best state's score
    double gap = 8.0;   // last frame's (best - cutoff) lower-bound distance
#ifdef ASR_CTC_STAMPS
    uint64_t st_acc[NSTAMP] = {};
    uint64_t st_last = __builtin_amdgcn_s_memtime();
#endif
#ifdef ASR_CTC_WSTAMPS
    // lane i (< 16) of every wave accumulates point i of its own wave; lane i
    // of wave 0 also the LAST wave's arrival at point i relative to the FIRST
    // wave's frame start (the critical path).  Lane-parallel, so that the
    // bookkeeping adds ~100 instructions per frame, not a serial loop.
    uint64_t st_lane = 0ull, crit_lane = 0ull, frames_ = 0ull;
    uint64_t wt[16];
#endif

    // Emission prefetch: a chunk of ch frames = ch*V floats, PF per thread;
    // element e = tid + j*NT is (frame s, label v), advanced incrementally.
    float pf[PF];
    float* ebuf = lds<float>(L::ebuf(ch, V));
    const int chunk_elems = ch * V;
    const int s_first = tid / V, v_first = tid - s_first * V;
    const int s_step = NT / V, v_step = NT - s_step * V;
#define ASR_LOAD_CHUNK(t0)                                                         \
    {                                                                              \
        int s_ = s_first, v_ = v_first;                                            \
        _Pragma("unroll") for (int j = 0; j < PF; j++) {                           \
            pf[j] = 1.f;                                                           \
            if (tid + j * NT < chunk_elems && (t0) + s_ < Tb)                      \
                pf[j] = ecol[(size_t)((t0) + s_) * tstride + v_];                  \
            s_ += s_step;                                                          \
            v_ += v_step;                                                          \
            if (v_ >= V) { v_ -= V; s_++; }                                        \
        }                                                                          \
    }
    ASR_LOAD_CHUNK(0)

    for (int t = 0; t < Tb; t++) {
        const int si = t % ch;
        if (si == 0) {
            uint64_t* lmax = lds<uint64_t>(L::LMAX);
#pragma unroll
            for (int j = 0; j < PF; j++) {
                const int e = tid + j * NT;
                if (e < chunk_elems) ebuf[e] = pf[j];
            }
            __syncthreads();
            if (t + ch < Tb) ASR_LOAD_CHUNK(t + ch)
            for (int e = tid; e < chunk_elems; e += NT)
                lech[e] = a.is_log ? (double)ebuf[e] : log((double)ebuf[e]);
            // largest log emission per frame: log is monotone, so the log of
            // the largest raw value (the same log call as above)
            for (int sf = tid; sf < ch; sf += NT) {
                float mx = ebuf[sf * V];
                for (int v = 1; v < V; v++) mx = fmaxf(mx, ebuf[sf * V + v]);
                lmax[sf] = asr_d2key(a.is_log ? (double)mx : log((double)mx));
            }
            __syncthreads();
        }
        const double* le = lech + si * V;
        const int cur = t & 1;
        const uint32_t bufC = cur ? L::BUF : 0u, bufN = L::BUF - bufC;   // frame-parity buffers
        const uint64_t* c_h = lds<uint64_t>(bufC + L::H);
        const uint64_t* c_hp = lds<uint64_t>(bufC + L::HP);
        const double* c_snb = lds<double>(bufC + L::SNB);
        const double* c_sb = lds<double>(bufC + L::SB);
        const double* c_l0 = lds<double>(bufC + L::SL0);
        const int* c_node = lds<int>(bufC + L::NODE);
        const uint64_t* c_tail = lds<uint64_t>(bufC + L::TAIL);
        // timesteps mode: TS0/TS1 of this parity past the layout's total (ts_base)
        const uint32_t tsC = L::ts_base(ch, V) + (cur ? L::TSPAR : 0u), tsN = L::ts_base(ch, V) + (cur ? 0u : L::TSPAR);
        const uint64_t* c_ts0 = lds<uint64_t>(tsC);
        const uint64_t* c_ts1 = lds<uint64_t>(tsC + 8u * (64 * RPT));
        const uint32_t* c_meta = lds<uint32_t>(bufC + L::META);
        uint64_t* n_h = lds<uint64_t>(bufN + L::H);
        uint64_t* n_hp = lds<uint64_t>(bufN + L::HP);
        double* n_snb = lds<double>(bufN + L::SNB);
        double* n_sb = lds<double>(bufN + L::SB);
        double* n_l0 = lds<double>(bufN + L::SL0);
        int* n_node = lds<int>(bufN + L::NODE);
        uint64_t* n_tail = lds<uint64_t>(bufN + L::TAIL);
        uint64_t* n_ts0 = lds<uint64_t>(tsN);
        uint64_t* n_ts1 = lds<uint64_t>(tsN + 8u * (64 * RPT));
        uint32_t* n_meta = lds<uint32_t>(bufN + L::META);
        const int* plC = lds<int>(bufC + L::PLINK);
        const uint64_t* chC = lds<uint64_t>(bufC + L::CHILD);
        int* plN = lds<int>(bufN + L::PLINK);
        uint64_t* chN = lds<uint64_t>(bufN + L::CHILD);
        const uint32_t* ofC = lds<uint32_t>(bufC + L::OFILT);
        uint32_t* ofN = lds<uint32_t>(bufN + L::OFILT);
#ifdef ASR_CTC_WSTAMPS
#pragma unroll
        for (int i_ = 0; i_ < 16; i_++) wt[i_] = 0ull;
#endif
        ASR_STAMP(0);   // chunk staging

        // P1. candidate lower bounds into registers; clear the next frame's
        //     links and orphan table (their last readers ran in frame t-1).
        //     Columns q != 1 are exact at once: their sources (q_r, not) and
        //     (q_r, blank) take the same emission, so the candidate is the
        //     prefix score L0 = lse(SNB, SB) (kept per slot, computed when the
        //     slot was built) plus the emission — (q_r, blank) alone when the
        //     label repeats the row's last one.  Only column 1 (three sources
        //     with the parent's extension) keeps a lower bound and a fold.
        for (int i = tid; i < OFW; i += NT) ofN[i] = 0u;
        for (int i = tid; i < kcap; i += NT) {
            plN[i] = -1;
            chN[i] = 0ull;
            if (CU) newidx[i] = -1;
        }
        if (tid == 0) {
            *sc.lcount = 0u;
            lds<uint32_t>(L::CTR)[t & 1] = 0u;   // extension slots of this frame
        }
        uint64_t keys[RPT][CW];
        uint32_t pend[RPT];   // bit 1: column 1 has two or more sources (needs the exact fold)
        uint32_t rmeta[RPT];
        double rsnb[RPT], rsb[RPT], rl0[RPT];
        int rp[RPT];                     // wave 0 only: parent slot
        double rx[RPT], rel[RPT];   // column 1's parent source (col1_sources); log emission of the row's last label
        // Every load of this phase is issued up front, so that it costs two
        // LDS round trips (rows, then parents) instead of one per column:
        // this wave's column labels are uniform, so their log emissions are
        // broadcast loads independent of the rows.
        // Selection floor of the fast path (P2), known before the candidates:
        // every contribution is a state score plus a log emission, so smaxU =
        // (best state) + (largest log emission) bounds every lower bound.
        const double smaxU = asr_key2d(best_state) + asr_key2d(lds<uint64_t>(L::LMAX)[si]);
        const uint64_t kmaxU = asr_d2key(smaxU + 1.1);
        const double Gd = smaxU - (1.1 * gap + 0.35);
        const uint64_t G = smaxU > -INFINITY ? asr_d2key(Gd) : 1ull;
        // extension column j's label this frame (by id, the blank skipped)
        auto col_label = [&](int q) -> int {
            if (q == 0) return blank;
            if (q == 1 || q >= R) return 0;
            return q - 2 + (q - 2 >= blank ? 1 : 0);
        };
        double ecol[CW];
        int labj[CW];
#pragma unroll
        for (int j = 0; j < CW; j++) {
            const int q = w * CW + j;
            labj[j] = col_label(q);
            ecol[j] = le[(q < R && q != 1) ? labj[j] : 0];
        }
        uint64_t rchild[RPT];
#pragma unroll
        for (int k = 0; k < RPT; k++) {
            const int r = lane + 64 * k;
            const bool live = r < P;
            // loaded unconditionally (r < KC): they need not wait for P
            const uint32_t m_ = c_meta[r];
            const double snb_ = c_snb[r], sb_ = c_sb[r], l0_ = c_l0[r];
            const uint64_t ch_ = chC[r];
            const int pl_ = plC[r];
            rmeta[k] = live ? m_ : 0u;
            rsnb[k] = live ? snb_ : -INFINITY;
            rsb[k] = live ? sb_ : -INFINITY;
            rl0[k] = live ? l0_ : -INFINITY;
            rchild[k] = live ? ch_ : 0ull;
            rp[k] = (w == 0 && live) ? pl_ : -1;
        }
        if (w == 0) {   // parents and the row's own label emission (second round trip)
#pragma unroll
            for (int k = 0; k < RPT; k++) {
                const bool hp = rp[k] >= 0;
                const uint32_t pm_ = hp ? c_meta[rp[k]] : 0u;
                const double pl0_ = hp ? c_l0[rp[k]] : -INFINITY, psb_ = hp ? c_sb[rp[k]] : -INFINITY;
                double y_;
                col1_sources(rmeta[k], rsnb[k], rp[k], pm_, pl0_, psb_, rx[k], y_);
                rel[k] = le[min((int)(rmeta[k] & META_LAST), V - 1)];
            }
        }
#pragma unroll
        for (int k = 0; k < RPT; k++) {
            const int r = lane + 64 * k;
            const bool live = r < P;
            pend[k] = 0u;
            const int last = (int)(rmeta[k] & META_LAST);
#pragma unroll
            for (int j = 0; j < CW; j++) {
                const int q = w * CW + j;
                const int lab = labj[j];
                const bool col = live && q < R && q != 1;
                const bool taken = q != 0 && ((rchild[k] >> lab) & 1ull);   // merged into column 1 of the child
                // (q, blank) <- L0 + e_blank; (q+c, not) <- L0 + e_c, or SB + e_c when c = last(q)
                const double base = (q != 0 && lab == last) ? rsb[k] : rl0[k];
                keys[k][j] = (col && !taken && base > -INFINITY) ? asr_d2key(base + ecol[j]) : 0ull;
            }
            if (w == 0 && live) {   // column 1: (q_r, not) <- lse(x, y) + e_last
                const double x = rx[k], y = (rmeta[k] & META_HAS_NB) ? rsnb[k] : -INFINITY;
                if (x > -INFINITY || y > -INFINITY) {
                    keys[k][1] = asr_d2key(fmax(x, y) + rel[k]);   // lower bound; exact with one source
                    if (x > -INFINITY && y > -INFINITY) pend[k] |= 2u;
                }
            }
        }
        if (CU && t == Tb - 1 && w == 0) {
            // .cu semantics, last step (CTCBeamSearch.cu:452-456): the
            // trailing blank is stripped before merging, so (q, blank) and
            // (q, not) become one state "q" before the prune.
#pragma unroll
            for (int k = 0; k < RPT; k++) {
                if (!keys[k][0] && !keys[k][1]) continue;
                double c0 = -INFINITY, c1 = -INFINITY;
                if (keys[k][0]) c0 = asr_key2d(keys[k][0]);
                if (keys[k][1]) {
                    if (pend[k] & 2u) {
                        c1 = lse2_call(rx[k], rsnb[k]) + rel[k];
                    } else {
                        c1 = asr_key2d(keys[k][1]);
                    }
                }
                const double m = keys[k][0] && keys[k][1] ? lse2_call(c0, c1) : (keys[k][0] ? c0 : c1);
                keys[k][0] = asr_d2key(m);
                keys[k][1] = 0ull;
                pend[k] &= ~3u;
            }
        }
        ASR_STAMP(1);   // candidates (lower bounds)

        // P2. prune threshold (cpp:97-118 with F1/F2): keep keys >= tau.
        //     Every contribution is a state score plus a log emission, so
        //     smaxU = (best state) + (largest log emission) bounds every lower
        //     bound, and smaxU + ln 3 every exact score: no block reduction.
        //     Exact folds are needed only where max + ln(n) can reach tau.
        //     Fast path: a filter G guessed from the last frame's cutoff;
        //     fold where upper >= G, then select from the floor G.  If at
        //     least K keys are >= G the answer tau >= G is exact: every
        //     unfolded candidate is < its upper bound < G <= tau (mixed keys
        //     are never above exact ones, and all keys >= tau are exact).
        //     Otherwise (guess too high, or fewer than K candidates: F2)
        //     fall back to stage 1 (the K-th largest lower bound tauL),
        //     folds where upper >= tauL, and stage 2.
// Exact fold of column 1 (the rows' (q, not), wave 0) where its upper bound
// max + ln 2 reaches FILT: lse(x, y) + e_last (col1_sources).  Every other
// column is exact from P1.
#define ASR_EXACT_FOLDS(FILT)                                                                     \
    if (w == 0) {                                                                                 \
        _Pragma("unroll") for (int k = 0; k < RPT; k++) {                                        \
            const bool job_ = (pend[k] & 2u) && asr_d2key(asr_key2d(keys[k][1]) + 0.7) >= (FILT); \
            if (!__ballot(job_)) continue;                                                        \
            if (job_) {                                                                           \
                pend[k] &= ~2u;                                                                   \
                const double y_ = (RPT <= 2) ? lse2(rx[k], rsnb[k])             \
                                                               : lse2_call(rx[k], rsnb[k]);       \
                keys[k][1] = asr_d2key(y_ + rel[k]);                                              \
            }                                                                                     \
        }                                                                                         \
    }
        ASR_EXACT_FOLDS(G)
        // the rows' own-state keys (final unless the fallback folds again),
        // for the wave that builds the own prefixes (the last one)
#define ASR_PUBLISH_OWN()                                                                         \
        if (!CU && NW > 1 && w == 0) {                                                            \
            _Pragma("unroll") for (int k = 0; k < RPT; k++)                                       \
                reinterpret_cast<uint4*>(lds<uint64_t>(L::OWNK))[lane + 64 * k] =                 \
                    make_uint4((uint32_t)keys[k][0], (uint32_t)(keys[k][0] >> 32),                \
                               (uint32_t)keys[k][1], (uint32_t)(keys[k][1] >> 32));               \
        }
        ASR_PUBLISH_OWN()
        ASR_STAMP(2);   // folds above the guess
        uint64_t tau = 1ull, ktop = 0ull;
        bool prune;
        if (CU)
            prune = kth_select_w0<NW>(RegKeys<RPT, CW>{keys}, K, G, kmaxU, sc, lds<uint32_t>(L::HW),
                                      lds<uint64_t>(L::DEC), tau, ktop);
        else   // every wave decides; own-prefix masks are read from OWNK below
            prune = kth_select_all<NW>(RegKeys<RPT, CW>{keys}, K, G, kmaxU, lds<uint32_t>(L::HW), hph_all,
                                       tau, ktop, sc
#ifdef ASR_CTC_WSTAMPS
                                       , wt
#endif
            );
        const bool fast = prune;   // ktop bounds every survivor's key
        ASR_STAMP(3);   // selection from the guess
        if (!prune) {
#ifdef ASR_CTC_STAMPS
            sc.n_pass1++;   // fallbacks
#endif
            uint64_t tauL;
            prune = kth_lower_bound<NW>(RegKeys<RPT, CW>{keys}, K,
                                        smaxU > -INFINITY ? asr_d2key(smaxU - (2.5 * gap + 1.0)) : 1ull,
                                        kmaxU, sc, tauL);
            ASR_EXACT_FOLDS(tauL)
            ASR_PUBLISH_OWN()
            tau = prune ? kth_exact<NW>(RegKeys<RPT, CW>{keys}, K, tauL, kmaxU, sc) : 1ull;
        }
#undef ASR_EXACT_FOLDS
#undef ASR_PUBLISH_OWN
        if (prune) {
            const double dg = smaxU - asr_key2d(tau);
            gap = (dg >= 0.0 && dg < 1e30) ? dg : 8.0;
            if (CU) {
                // .cu semantics keep exactly K states (stable sort + cut,
                // cu:174-196): of the keys tied at tau only the first
                // K - #(keys > tau) survive, in thread order (a deterministic
                // stand-in for the .cu's string order among equal scores).
                int ngt = 0, neq = 0;
#pragma unroll
                for (int k = 0; k < RPT; k++)
#pragma unroll
                    for (int j = 0; j < CW; j++) {
                        ngt += keys[k][j] > tau;
                        neq += keys[k][j] == tau;
                    }
                int gt_total, eq_total;
                uint64_t unused = 0ull;
                (void)blk.wave_offsets(__builtin_amdgcn_readlane((int)wave_incl_scan((uint32_t)ngt), 63),
                                       gt_total, unused);
                const int eincl = (int)wave_incl_scan((uint32_t)neq);
                int erank = blk.wave_offsets(__builtin_amdgcn_readlane(eincl, 63), eq_total, unused) +
                            eincl - neq;
                const int room = K - gt_total;
#pragma unroll
                for (int k = 0; k < RPT; k++)
#pragma unroll
                    for (int j = 0; j < CW; j++)
                        if (keys[k][j] == tau) {
                            if (erank >= room) keys[k][j] = 0ull;
                            erank++;
                        }
            }
        }
        ASR_STAMP(4);   // stage 2

        // P3. compaction of survivors into the next slot buffer.  Slot order
        //     is free (ranking and ties never depend on it): wave w owns
        //     slots [off_w, off_w + n_w); wave 0 puts the rows' own prefixes
        //     first.  A row's own prefix is built by the thread holding the
        //     row; extensions are listed in a wave-private descriptor run
        //     (in slot order) and built one per lane, by every wave at once.
        //     Parent links of the next frame are built here (DESIGN.md §3):
        //     * extension (r, c) -> the slot of row r's own prefix;
        //     * row r's own prefix -> its parent row's new slot (the parent
        //       prefix, if live, cannot reappear as an extension: merged);
        //     * a continuing orphan -> the extension that recreates its
        //       parent prefix, through its group (completed next frame).
        int next = 0;                 // extensions emitted by this thread
        uint64_t kbest = 0ull;        // every survivor key is exact: the best state
        uint32_t selfbits = 0u;       // bit k: row lane+64k keeps its own prefix
#pragma unroll
        for (int k = 0; k < RPT; k++)
#pragma unroll
            for (int j = 0; j < CW; j++) {
                const int q = w * CW + j;
                if (q == 0) selfbits |= (keys[k][0] >= tau || keys[k][1] >= tau) ? 1u << k : 0u;
                else if (q >= 2) next += keys[k][j] >= tau;
                kbest = keys[k][j] >= tau && keys[k][j] > kbest ? keys[k][j] : kbest;
            }
        // own-prefix slots of wave 0: ballot order, k-major
        int selfidx[RPT];
        int nself = 0;
#pragma unroll
        for (int k = 0; k < RPT; k++) {
            const uint64_t bal = __ballot((selfbits >> k) & 1u);
            selfidx[k] = nself + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32),
                                      __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
            nself += __popcll(bal);
        }
        if (w != 0) nself = 0;
        const int xincl = (int)wave_incl_scan((uint32_t)next);
        const int xtot = __builtin_amdgcn_readlane(xincl, 63);
        int total = 0, xbase;   // xbase: this wave's first extension slot
        uint64_t smask[RPT];    // bit l of word k: row l + 64k keeps its own prefix
        int spre[RPT];          // own prefixes in earlier words
        uint32_t* ctr = lds<uint32_t>(L::CTR) + (t & 1);
        ASR_WT(7);   // arrival at the offsets exchange
        if (CU) {
            // .cu mode: slot order must follow thread order (its tie cut
            // runs on it next frame), so offsets come from one exchange
            if (w == 0) {   // wave 0 comes first: its slot numbers are final now
#pragma unroll
                for (int k = 0; k < RPT; k++) {
                    const int r = lane + 64 * k;
                    if (((selfbits >> k) & 1u) && selfidx[k] < kcap) newidx[r] = selfidx[k];
                }
            }
            const int woff = blk.template wave_offsets<true>(nself + xtot, total, kbest);
            best_state = kbest;
            xbase = woff + nself;
        } else {
            // Own prefixes take slots [0, nself) in row order; every wave
            // reads the rows' masks (published by wave 0 with the cutoff) and
            // takes its extension slots with one returning add: no exchange.
            if (!fast) {   // fallback selection: the block max by one exchange
                int unused_;
                (void)blk.template wave_offsets<true>(0, unused_, kbest);
            }
            best_state = fast ? ktop : kbest;
            int pre = 0;
#pragma unroll
            for (int k = 0; k < RPT; k++) {   // every wave reads the rows' own keys and the cutoff
                const uint4 o = reinterpret_cast<const uint4*>(lds<uint64_t>(L::OWNK))[lane + 64 * k];
                const uint64_t kb_ = ((uint64_t)o.y << 32) | o.x, knb_ = ((uint64_t)o.w << 32) | o.z;
                smask[k] = __ballot(kb_ >= tau || knb_ >= tau);
                spre[k] = pre;
                pre += __popcll(smask[k]);
            }
            nself = pre;
            int got = 0;
            if (xtot > 0 && lane == 0) got = (int)atomicAdd(ctr, (uint32_t)xtot);
            xbase = nself + __builtin_amdgcn_readlane(got, 0);
        }
        // the next slot of row r's own prefix (or -1)
        const auto newslot = [&](int r) -> int {
            if (CU) return newidx[r];
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
        if (CU && total > kcap) { overflow = 1; total = kcap; }
        ASR_STAMP(5);   // scan
        // own prefixes: row r's slot is built by lane r of the last wave
        // (the lightest: fewest valid columns), from the keys wave 0
        // published; in .cu mode (keys cut after the selection) by wave 0.
        constexpr int WB = NW - 1;
        if ((CU || NW == 1) ? w == 0 : w == WB) {
#pragma unroll
            for (int k = 0; k < RPT; k++) {
                const int r = lane + 64 * k;
                int i;
                uint64_t kb, knb;
                uint32_t m0;
                int pr;
                if (CU || NW == 1) {
                    i = selfidx[k];
                    if (!((selfbits >> k) & 1u) || i >= kcap) continue;
                    kb = keys[k][0];
                    knb = keys[k][1];
                    m0 = rmeta[k];
                    pr = rp[k];                              // complete (P1)
                } else {
                    if (!((smask[k] >> lane) & 1ull)) continue;
                    i = spre[k] + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(smask[k] >> 32),
                                          __builtin_amdgcn_mbcnt_lo((uint32_t)smask[k], 0u));
                    if (i >= kcap) continue;
                    const uint4 o = reinterpret_cast<const uint4*>(lds<uint64_t>(L::OWNK))[r];
                    kb = ((uint64_t)o.y << 32) | o.x;
                    knb = ((uint64_t)o.w << 32) | o.z;
                    m0 = rmeta[k];
                    pr = plC[r];
                }
                const uint32_t lab = m0 & META_LAST;
                const uint64_t hp = c_hp[r];
                uint32_t m = m0 & (META_LAST | META_HAS_PAR);
                m |= kb >= tau ? META_HAS_B : 0u;
                m |= knb >= tau ? META_HAS_NB : 0u;
                const double vb = kb >= tau ? asr_key2d(kb) : -INFINITY;
                const double vnb = knb >= tau ? asr_key2d(knb) : -INFINITY;
                n_sb[i] = vb;
                n_snb[i] = vnb;
                n_l0[i] = (vb > -INFINITY && vnb > -INFINITY)
                              ? ((RPT <= 2) ? lse2(vnb, vb) : lse2_call(vnb, vb))
                              : fmax(vnb, vb);
                n_node[i] = c_node[r];
                n_tail[i] = c_tail[r];
                if (a.nodes_ts) {   // a continuing prefix keeps its labels' append frames
                    n_ts0[i] = c_ts0[r];
                    n_ts1[i] = c_ts1[r];
                }
                n_meta[i] = m;
                n_h[i] = c_h[r];
                n_hp[i] = hp;
                const int y = pr >= 0 && pr < kcap ? newslot(pr) : -1;
                if (y >= 0) {
                    plN[i] = y;
                    set_label_bit(&chN[y], lab);
                } else if (m0 & META_HAS_PAR) {
                    // an orphan next frame, unless an extension built now
                    // recreates its parent (then the entry is never matched:
                    // that prefix stays live, so it is not extended again)
                    ASR_COUNT(0, 1);
                    ofilt_insert(ofN, hp);
                }
            }
        }
        ASR_WT(8);   // own prefixes built
        // extensions: each wave stages its own in a private run of records
        // (key, row | label; indices independent of the slot base the
        // returning add hands out), then builds them one per lane, reading
        // the row's hash, tail and node from the current buffer (P1 loads
        // only what the candidates need).
        {
            constexpr uint32_t SW = L::STG_W;   // bytes per wave
            const uint32_t sb = L::STG + (uint32_t)w * SW;
            uint64_t* s_key = lds<uint64_t>(sb);
            uint32_t* s_rl = lds<uint32_t>(sb + 8u * L::KCAP);
            const int base = xbase;
            int pos = xincl - next;   // this thread's first record in the wave's run
#pragma unroll
            for (int k = 0; k < RPT; k++)
#pragma unroll
                for (int j = 0; j < CW; j++) {
                    const int q = w * CW + j;
                    if (q < 2 || keys[k][j] < tau) continue;
                    if (pos < (int)L::KCAP) {
                        const uint32_t lab = (uint32_t)col_label(q);
                        s_key[pos] = keys[k][j];
                        s_rl[pos] = (uint32_t)(lane + 64 * k) | (lab << 16);
                    }
                    pos++;
                }
            ASR_WT(9);   // descriptors written
            const int xend = base + xtot < kcap ? base + xtot : kcap;
            for (int i = base + lane; i < xend; i += 64) {
                const int li = i - base;   // < kcap <= KCAP
                const uint64_t ky = s_key[li];
                const uint32_t rl = s_rl[li];
                const int r = (int)(rl & 0xFFFFu);
                const uint32_t lab = rl >> 16;
                const uint64_t hr = c_h[r];
                const uint64_t tl = c_tail[r];
                const int nd = c_node[r];
                const uint64_t h = mix_hash(hr, lab);
                const double vy = asr_key2d(ky);
                n_snb[i] = vy;
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
                    if (a.nodes_ts) {   // timesteps: label n was appended at frame t
                        uint64_t f0 = c_ts0[r], f1 = c_ts1[r];
                        if (n < 4u) f0 |= (uint64_t)(t & 0xFFFF) << (16u * n);
                        else f1 |= (uint64_t)(t & 0xFFFF) << (16u * (n - 4u));
                        if (n == 7u) {
                            a.nodes_ts[(size_t)b * a.T * kcap + t * kcap + i] =
                                make_int4((int)(uint32_t)f0, (int)(uint32_t)(f0 >> 32), (int)(uint32_t)f1,
                                          (int)(uint32_t)(f1 >> 32));
                            f0 = f1 = 0ull;
                        }
                        n_ts0[i] = f0;
                        n_ts1[i] = f1;
                    }
                }
                n_meta[i] = lab | META_HAS_NB | META_HAS_PAR;
                n_h[i] = h;
                n_hp[i] = hr;
                const int y = newslot(r);
                if (y >= 0) {
                    plN[i] = y;
                    set_label_bit(&chN[y], lab);
                } else {
                    ASR_COUNT(0, 1);
                    ofilt_insert(ofN, hr);
                }
                // a new prefix may recreate the parent of this frame's orphans
                if (ofilt_maybe(ofC, h)) {
                    const uint64_t cm = orphan_adopt_scan(c_hp, plC, c_meta, P, h, newslot, plN, i);
                    if (cm) chN[i] = cm;
                    ASR_COUNT(1, 1);   // filter hits (adoption scans)
                }
                ASR_COUNT(2, 1);
            }
        }
        ASR_WT(10);   // extensions built
#ifdef ASR_CTC_WSTAMPS
        // this frame's arrival clocks, one per lane (the staging records are
        // not touched again before the next frame's P3b)
        uint64_t wv_ = 0ull;
#pragma unroll
        for (int i_ = 0; i_ < 16; i_++) wv_ = lane == i_ ? wt[i_] : wv_;
        if (lane < 16) lds<uint64_t>(L::STG + (uint32_t)w * L::STG_W)[lane] = wv_;
#endif
        __syncthreads();
        if (CU) {
            P = total;
        } else {   // every wave's extensions are counted now
            const int tot = nself + (int)*ctr;
            if (tot > kcap) overflow = 1;
            P = tot < kcap ? tot : kcap;
        }
        ASR_STAMP(6);   // slot build + links
#ifdef ASR_CTC_WSTAMPS
        {
            if (lane == 6) wv_ = wt[6];
            if (lane < 16 && wv_) st_lane += wv_ - wt[0];
            frames_ += 1;
            if (w == 0) {
                uint64_t m_ = 0ull, s0_ = ~0ull;
#pragma unroll
                for (int v_ = 0; v_ < NW; v_++) {
                    const uint64_t x_ = lds<uint64_t>(L::STG + (uint32_t)v_ * L::STG_W)[lane & 15];
                    const uint64_t y_ = lds<uint64_t>(L::STG + (uint32_t)v_ * L::STG_W)[0];
                    m_ = x_ > m_ ? x_ : m_;
                    s0_ = y_ < s0_ ? y_ : s0_;
                }
                if (lane == 6) m_ = wt[6];
                if (lane < 16 && m_ && lane != 0) crit_lane += m_ - s0_;
            }
        }
#endif
#ifdef ASR_CTC_STAMPS
        st_acc[7] += lds<uint32_t>(L::MISC)[0];   // orphan entries inserted this frame
        st_acc[8] += lds<uint32_t>(L::MISC)[1];   // orphan continuations linked (adopted)
        st_acc[9] += lds<uint32_t>(L::MISC)[2];   // extensions built
        __syncthreads();
        if (tid < 6) lds<uint32_t>(L::MISC)[tid] = 0u;
#endif
    }
#undef ASR_LOAD_CHUNK

    // Final merge (cpp:169-187 with F3): strip the trailing blank, "q" + "q$".
    const int cur = Tb & 1;
    const uint32_t bufC = cur ? L::BUF : 0u;
    // Each slot's score of "q" merged with "q$" is its L0 = lse(SNB, SB).
    const int* c_node = lds<int>(bufC + L::NODE);
    const double* c_l0 = lds<double>(bufC + L::SL0);
    for (int i = tid; i < P; i += NT) {
        a.fin_score[(size_t)b * kcap + i] = c_l0[i];   // lse(SNB, SB), computed when the slot was built
        a.fin_node[(size_t)b * kcap + i] = c_node[i];
        a.fin_tail[(size_t)b * kcap + i] = lds<uint64_t>(bufC + L::TAIL)[i];
        if (a.nodes_ts) {
            const uint32_t tsF = L::ts_base(ch, V) + (cur ? L::TSPAR : 0u);
            a.fin_ts[((size_t)b * kcap + i) * 2] = lds<uint64_t>(tsF)[i];
            a.fin_ts[((size_t)b * kcap + i) * 2 + 1] = lds<uint64_t>(tsF + 8u * (64 * RPT))[i];
        }
    }
#ifdef ASR_CTC_WSTAMPS
    if (lane < 16) a.stamps[(size_t)b * NSTAMP + w * 16 + lane] = lane == 0 ? frames_ : st_lane;
    if (w == 0 && lane < 16) a.stamps[(size_t)b * NSTAMP + 8 * 16 + lane] = lane == 0 ? frames_ : crit_lane;
#endif
    if (tid == 0) {
        a.fin_n[b] = P;
        a.status[b] = overflow | (sc.err << 1);
#ifdef ASR_CTC_STAMPS
        st_acc[10] = sc.t_pre;
        st_acc[11] = sc.t_bar;
        st_acc[12] = sc.t_post;
        st_acc[13] = sc.n_pass1;
        st_acc[14] = sc.n_pass2;
        st_acc[15] = sc.n_rank | ((uint64_t)sc.sum_cd << 32);
        for (int i = 0; i < NSTAMP; i++) a.stamps[(size_t)b * NSTAMP + i] = st_acc[i];
#endif
    }
}

}  // namespace asr
