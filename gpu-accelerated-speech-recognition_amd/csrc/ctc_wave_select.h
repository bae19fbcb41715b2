// ============================================================================
// One-wave CTC decoder (ctc_wave_kernel.inc): the exact K-th-largest-key
// selection of a frame and the 32-bit wave maximum of the frame loop's
// live-label bound.
// Included after ctc_beam_kernel.inc (wave_incl_scan, wave_max_u64).
//
// Selection on high words.  A pass of
// wave_kth_select bins a key x by (x - lo) >> sh and counts it when
// x - lo <= hi - lo.  When lo's low 32-bit word is 0, hi's is all ones and
// sh >= 32, both depend on x's high word xh alone:
//   * x - lo borrows nothing from the (zero) low word, so its high word is
//     xh - loh and (x - lo) >> sh == (xh - loh) >> (sh - 32);
//   * lo <= x <= hi  <=>  loh <= xh <= hih (every low word lies between 0 and
//     all ones)  <=>  xh - loh <= hih - loh in wrapping 32-bit arithmetic.
// So the pass counts the same keys into the same bins with 32-bit subtract,
// compare and shift.  The first pass has the property because the floor G is
// rounded DOWN to a zero low word where it is made (a speed knob used
// consistently by the live-label filter, the folds and the selection: a lower
// floor counts more keys and finds the same K-th one) and the bound kmaxU,
// which carries 1.1 of slack, is rounded UP to an all-ones low word; floor 1
// becomes 2^32, below every key asr_d2key makes (-inf is 0x000FFFFFFFFFFFFF)
// and above the absent key 0.  A split keeps it while sh >= 32:
// b0 = lo + (n << sh) has lo's low word and b1 = b0 + 2^sh - 1 (or hi) all
// ones.  Each pass tests the property on the scalar unit and falls back to the
// 64-bit form (always the case below sh = 32).  The survivors are the keys >=
// the K-th largest in either form; tau and ktop, a separator and a bound, may
// differ from the unrounded run's within those roles.
// ============================================================================
#pragma once

namespace asr {

// Max over the 64 lanes, in lane 63: wave_incl_scan's DPP steps with max for
// add (a lane a step does not reach reads 0, the identity).
__device__ __forceinline__ uint32_t wave_max_u32_last(uint32_t x) {
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, true));    // row_shr:1
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, true));    // row_shr:2
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, true));    // row_shr:4
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, true));    // row_shr:8
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false));   // row_bcast:15
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false));   // row_bcast:31
    return x;
}

// The need-th largest key as a threshold tau (survivors: keys >= tau), one
// wave: kth_select_all's 64-bin passes (keys in [lo, hi] counted per bin,
// largest keys in lane 0; the bin holding the need-th key is split next)
// over ONE histogram — the wave reads its 64 counts and zeroes them in
// program order, so no rotation and no barrier.  Returns false when fewer
// than need keys are >= lb.  ktop: top of the first pass's highest
// non-empty bin (a bound of the best key).
// h2 (ASR_CTC_HIST2): a second copy of the histogram for the odd lanes
// (same-bin atomics of one instruction split over two words), bin b at word
// (b + 16) & 63 so that the copies' words of one bin sit in different banks.
template <class KS>
__device__ __forceinline__ bool wave_kth_select(const KS& keys, int need, uint64_t lb, uint64_t kmax,
                                                uint32_t* h, uint64_t& tau, uint64_t& ktop, int& err,
                                                uint32_t* h2 = nullptr, uint64_t* npass = nullptr) {
    const int lane = threadIdx.x & 63;
    if (kmax < lb) return false;
    uint64_t lo = lb, hi = kmax;   // inclusive range that holds the answer
    uint32_t* const hs = (h2 && (lane & 1)) ? h2 : h;
    const uint32_t rot = (h2 && (lane & 1)) ? 16u : 0u;
    for (int pass = 0; pass < 12; pass++) {
        const uint64_t span = hi - lo;
        const int top = span ? 63 - __clzll((long long)span) : 0;
        const int sh = top > 5 ? top - 5 : 0;   // span >> sh < 64
        if (sh >= 32 && (uint32_t)lo == 0u && (uint32_t)hi == 0xFFFFFFFFu) {
            // high words only (header): the same keys into the same bins
            const uint32_t loh = (uint32_t)(lo >> 32), spanh = (uint32_t)(span >> 32);
            const int shh = sh - 32;
            keys.each([&](uint64_t x) {
                const uint32_t d = (uint32_t)(x >> 32) - loh;
                if (d <= spanh) atomicAdd(&hs[(63u - (d >> shh) + rot) & 63u], 1u);
            });
        } else {
            keys.each([&](uint64_t x) {
                const uint64_t d = x - lo;   // x in [lo, hi] <=> x - lo <= span (unsigned)
                if (d <= span) atomicAdd(&hs[(63u - (uint32_t)(d >> sh) + rot) & 63u], 1u);
            });
        }
        uint32_t c = h[lane];
        h[lane] = 0u;
        if (h2) {
            c += h2[(lane + 16) & 63];
            h2[(lane + 16) & 63] = 0u;
        }
        const uint32_t S = wave_incl_scan(c);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)S, 63);
        if (npass) {   // diagnostic counters: passes, keys counted in the first pass
            npass[0]++;
            if (pass == 0) npass[1] += total;
        }
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
            err = 1;
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
        if ((int)cd == need || sh == 0 || b1 == b0) {   // the whole bin survives / one key value
            tau = b0;
            return true;
        }
        lo = b0;
        hi = b1;
    }
    err = 1;
    tau = lo;
    return true;
}

}  // namespace asr
