// ============================================================================
// CTC forced alignment and exact transcript scoring on gfx950 — one wave per
// (target, utterance) pair, the whole lattice column resident in registers for
// all T frames, one launch per call.
//
// The extended target ext has S = 2L+1 states (ext[2i] = blank, ext[2i+1] =
// target[i]).  Two recurrences over the same lattice run side by side, each
// compiled out when its outputs are not wanted:
//   forward  a_t[s] = lse(lse(a[s], a[s-1]), a[s-2] if skip(s)) + lp(t, ext[s])
//   Viterbi  v_t[s] = max(v[s], v[s-1], v[s-2] if skip(s))      + lp(t, ext[s])
// with skip(s) = ext[s] != blank && ext[s] != ext[s-2].  Viterbi ties take the
// smallest jump (stay, then s-1, then s-2); the final state is S-1 unless
// v[S-2] > v[S-1] strictly.
//
// Layout: lane l owns the K contiguous states [l*K, l*K+K), K in {1,2,4,8,16}
// chosen on the host from max_target_len (S <= 64 K).  States s-1 and s-2 are
// in-lane except for a lane's first two states, which take the previous
// lane's last two (K = 1: lanes l-1 and l-2): two fp64 values per recurrence
// cross lanes per frame, whatever K is.  The operations of one state are the
// same for every K, so a target's bits do not depend on K, N or T.
//
// Emission rows are gathered PF frames ahead into a register ring (a lane
// loads the blank column and its K/2 label columns; addresses do not depend
// on the recurrence).  The Viterbi choices of a frame are 2 bits per state:
// one store of 1, 2 or 4 bytes per lane into a coalesced row of d_work per
// frame.  The traceback is the tail of the same kernel: the wave loads the
// rows of ASR_ALIGN_TB_CHUNK frames at once (every lane its own word of each
// row, all loads independent), then walks the chunk with register reads
// (v_readlane of the lane that owns the current state), so the dependent
// chain has one memory round trip per chunk instead of one per frame.
// ============================================================================
#include "asr_internal.h"
#include "ctc_lse.h"

#include <cmath>

// Frames of back-pointer rows the traceback loads per memory round trip
// (1 .. 64; 1 = the plain dependent chain of one load per frame).  A/B timing:
//   make cvariant CV=tb1 CVFLAGS=-DASR_ALIGN_TB_CHUNK=1     (ASR_LIB selects the library)
//   make cvariant CV=notb CVFLAGS=-DASR_ALIGN_NO_TRACEBACK
#ifndef ASR_ALIGN_TB_CHUNK
#define ASR_ALIGN_TB_CHUNK 64
#endif

namespace asr {

struct AlignArgs {
    const float* emis;
    long frame_stride, utt_stride;
    const int32_t* lengths;          // [B] or NULL
    const int32_t* targets;          // [N][ldt]
    long ldt;
    const int32_t* target_lengths;   // [N]
    const int32_t* utt;              // [N] or NULL
    double* score;                   // [N] or NULL
    double* vscore;                  // [N] or NULL
    int32_t* path;                   // [N][ldp] or NULL
    long ldp;
    int32_t* spans;                  // [N][ldt][2] or NULL
    void* work;
    int T, B, V, N, max_target_len, is_log, blank;
};

constexpr int align_k(int max_target_len) {
    const int S = 2 * max_target_len + 1;
    return S <= 64 ? 1 : S <= 128 ? 2 : S <= 256 ? 4 : S <= 512 ? 8 : 16;
}
// bytes of one lane's 2K back-pointer bits
constexpr int align_word_bytes(int K) { return K <= 4 ? 1 : K == 8 ? 2 : 4; }

// Value of state s (wave-uniform, 0 <= s < 64 K) from the lane that owns it.
template <int K>
__device__ __forceinline__ double align_fetch(const double (&x)[K], int s, int lane) {
    const int j = s % K;
    double m = x[0];
#pragma unroll
    for (int i = 1; i < K; i++) m = (j == i) ? x[i] : m;
    return __shfl(m, s / K);
}

// VIT: 0 = no Viterbi, 1 = its score only, 2 = back-pointers and traceback.
template <int K, bool FWD, int VIT>
__global__ __launch_bounds__(64) void ctc_align_kernel(const AlignArgs p) {
    constexpr int NL = K >= 2 ? K / 2 : 1;    // label states of a lane
    constexpr int NC = K >= 2 ? NL + 1 : 1;   // emission columns a lane loads per frame (K >= 2: blank first)
    constexpr int PF = K >= 8 ? 4 : 8;        // frames of emissions in flight
    constexpr int WB = align_word_bytes(K);
    constexpr int TBC = ASR_ALIGN_TB_CHUNK;
    static_assert(TBC >= 1 && TBC <= 64, "traceback chunk");
    const int n = blockIdx.x, lane = threadIdx.x;
    const int T = p.T, V = p.V, blank = p.blank, mtl = p.max_target_len;
    const double NINF = -INFINITY;

    int L = p.target_lengths[n];
    L = L < 0 ? 0 : (L > mtl ? mtl : L);
    const int S = 2 * L + 1;
    const int b = p.utt ? p.utt[n] : n;
    const bool utt_ok = b >= 0 && b < p.B;
    int len = 0;
    if (utt_ok) {
        len = p.lengths ? p.lengths[b] : T;
        len = len < 0 ? 0 : (len > T ? T : len);
    }
    const int32_t* tgt = p.targets + (long)n * p.ldt;
    int32_t* path = (VIT == 2 && p.path) ? p.path + (long)n * p.ldp : nullptr;
    int32_t* spans = (VIT == 2 && p.spans) ? p.spans + (long)n * p.ldt * 2 : nullptr;

    // ---- this lane's states: labels, emission columns, skip and validity masks
    const int s0 = lane * K;
    int col[NC];
    uint32_t skipmask = 0, okmask = 0;
    bool bad = false;
    if (K == 1) {
        const int i = (lane - 1) >> 1;   // label index of an odd state
        int lab = blank;
        if ((lane & 1) && i < L) {
            lab = tgt[i];
            if (lab < 0 || lab >= V || lab == blank) {
                bad = true;
                lab = blank;
            } else if (i >= 1 && tgt[i - 1] != lab) {
                skipmask = 1;
            }
        }
        col[0] = lab;
        okmask = s0 < S ? 1u : 0u;
    } else {
        col[0] = blank;
#pragma unroll
        for (int q = 0; q < NL; q++) {
            const int i = lane * NL + q;   // label index of state s0 + 2q + 1
            int lab = blank;
            if (i < L) {
                lab = tgt[i];
                if (lab < 0 || lab >= V || lab == blank) {
                    bad = true;
                    lab = blank;
                } else if (i >= 1 && tgt[i - 1] != lab) {
                    skipmask |= 1u << (2 * q + 1);
                }
            }
            col[q + 1] = lab;
        }
#pragma unroll
        for (int j = 0; j < K; j++) okmask |= (s0 + j < S) ? (1u << j) : 0u;
    }
    const bool infeasible_input = __any(bad) || !utt_ok || (len == 0 && L > 0);

    double a[K], v[K];
#pragma unroll
    for (int j = 0; j < K; j++) a[j] = v[j] = NINF;

    double score = NINF, vscore = NINF;
    int sfin = -1;   // final Viterbi state, -1: infeasible

    if (!infeasible_input && len == 0) {
        score = vscore = 0.0;   // L == 0: the empty alignment
    } else if (!infeasible_input) {
        const float* ebase = p.emis + (long)b * p.utt_stride;
        const long fs = p.frame_stride;
        const bool is_log = p.is_log != 0;
        auto to_lp = [&](float x) -> double { return is_log ? (double)x : log((double)x); };

        // ---- frame 0
        {
            double lp0[NC];
#pragma unroll
            for (int c = 0; c < NC; c++) lp0[c] = to_lp(ebase[col[c]]);
#pragma unroll
            for (int j = 0; j < K; j++) {
                const double e = K == 1 ? lp0[0] : ((j & 1) ? lp0[1 + j / 2] : lp0[0]);
                const double x = (s0 + j < 2 && ((okmask >> j) & 1u)) ? e : NINF;
                a[j] = v[j] = x;
            }
        }
        // ---- frames 1 .. len-1, emission rows PF frames ahead in registers
        float raw[PF][NC];
#pragma unroll
        for (int u = 0; u < PF; u++) {
            const int row = 1 + u < len ? 1 + u : len - 1;
            const float* r = ebase + (long)row * fs;
#pragma unroll
            for (int c = 0; c < NC; c++) raw[u][c] = r[col[c]];
        }
        char* const wrow = VIT == 2 ? (char*)p.work + (long)n * T * (64 * WB) + lane * WB : nullptr;
        for (int t0 = 1; t0 < len; t0 += PF) {
#pragma unroll
            for (int u = 0; u < PF; u++) {
                const int t = t0 + u;
                if (t < len) {
                    double lp[NC];
#pragma unroll
                    for (int c = 0; c < NC; c++) lp[c] = to_lp(raw[u][c]);
                    {
                        const int row = t + PF < len ? t + PF : len - 1;
                        const float* r = ebase + (long)row * fs;
#pragma unroll
                        for (int c = 0; c < NC; c++) raw[u][c] = r[col[c]];
                    }
                    // the previous lane's last two states (K = 1: the two previous lanes)
                    double pa1 = NINF, pa2 = NINF, pv1 = NINF, pv2 = NINF;
                    if (FWD) {
                        pa1 = __shfl_up(a[K - 1], 1);
                        pa2 = K == 1 ? __shfl_up(a[0], 2) : __shfl_up(a[K >= 2 ? K - 2 : 0], 1);
                        if (lane < 1) pa1 = NINF;
                        if (lane < (K == 1 ? 2 : 1)) pa2 = NINF;
                    }
                    if (VIT) {
                        pv1 = __shfl_up(v[K - 1], 1);
                        pv2 = K == 1 ? __shfl_up(v[0], 2) : __shfl_up(v[K >= 2 ? K - 2 : 0], 1);
                        if (lane < 1) pv1 = NINF;
                        if (lane < (K == 1 ? 2 : 1)) pv2 = NINF;
                    }
                    uint32_t bits = 0;
#pragma unroll
                    for (int j = K - 1; j >= 0; j--) {   // descending: a[j-1], a[j-2] still hold frame t-1
                        const bool label_state = K == 1 || (j & 1);   // K >= 2: even states are blanks (never skip)
                        const bool sk = (skipmask >> j) & 1u;
                        const bool ok = (okmask >> j) & 1u;
                        const double e = K == 1 ? lp[0] : ((j & 1) ? lp[1 + j / 2] : lp[0]);
                        if (FWD) {
                            const double x1 = j >= 1 ? a[j - 1] : pa1;
                            const double x2 = j >= 2 ? a[j - 2] : (j == 1 ? pa1 : pa2);
                            double r = lse2(a[j], x1);
                            if (label_state) r = lse2(r, sk ? x2 : NINF);
                            a[j] = ok ? r + e : NINF;
                        }
                        if (VIT) {
                            const double x1 = j >= 1 ? v[j - 1] : pv1;
                            const double x2 = j >= 2 ? v[j - 2] : (j == 1 ? pv1 : pv2);
                            double best = v[j];
                            uint32_t c = 0;
                            if (x1 > best) {
                                best = x1;
                                c = 1;
                            }
                            if (label_state && sk && x2 > best) {
                                best = x2;
                                c = 2;
                            }
                            v[j] = ok ? best + e : NINF;
                            bits |= c << (2 * j);
                        }
                    }
                    if (VIT == 2) {
                        char* w = wrow + (long)t * (64 * WB);
                        if (WB == 1) *(uint8_t*)w = (uint8_t)bits;
                        else if (WB == 2) *(uint16_t*)w = (uint16_t)bits;
                        else *(uint32_t*)w = bits;
                    }
                }
            }
        }
        // ---- final scores
        if (FWD) {
            const double a1 = align_fetch<K>(a, S - 1, lane);
            score = L >= 1 ? lse2(a1, align_fetch<K>(a, S - 2, lane)) : a1;
        }
        if (VIT) {
            const double v1 = align_fetch<K>(v, S - 1, lane);
            const double v2 = L >= 1 ? align_fetch<K>(v, S - 2, lane) : NINF;
            const bool second = v2 > v1;
            vscore = second ? v2 : v1;
            if (vscore > NINF) sfin = second ? S - 2 : S - 1;
        }
    }

    if (lane == 0) {
        if (FWD) p.score[n] = score;
        if (VIT && p.vscore) p.vscore[n] = vscore;
    }
    if (VIT != 2) return;
#ifdef ASR_ALIGN_NO_TRACEBACK   // A/B timing build only: the recurrence and its stores alone
    return;
#endif

    // ---- traceback (the rows were written by all lanes of this wave)
    __threadfence();
    sfin = __builtin_amdgcn_readfirstlane(sfin);
    if (sfin >= 0) {
        const char* const rrow = (const char*)p.work + (long)n * T * (64 * WB) + lane * WB;
        int s = sfin, s_above = -1;
        for (int tb = (len - 1) / TBC * TBC; tb >= 0; tb -= TBC) {
            uint32_t w[TBC];
#pragma unroll
            for (int u = 0; u < TBC; u++) {
                const int t = tb + u;
                w[u] = 0;
                if (t >= 1 && t < len) {
                    const char* r = rrow + (long)t * (64 * WB);
                    w[u] = WB == 1 ? (uint32_t) * (const uint8_t*)r
                                   : WB == 2 ? (uint32_t) * (const uint16_t*)r : *(const uint32_t*)r;
                }
            }
            int my_s = -1;   // lane u: the state at frame tb + u
#pragma unroll
            for (int u = TBC - 1; u >= 0; u--) {
                const int t = tb + u;
                if (t < len) {
                    if (lane == u) my_s = s;
                    if (t >= 1) {
                        const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)w[u], s / K);
                        s = __builtin_amdgcn_readfirstlane(s - (int)((word >> (2 * (s % K))) & 3u));
                    }
                }
            }
            // here s is the state at frame tb - 1
            const int t = tb + lane;
            int s_lo = __shfl_up(my_s, 1);
            if (lane == 0) s_lo = tb >= 1 ? s : -1;
            int s_hi = __shfl_down(my_s, 1);
            if (t + 1 >= len) s_hi = -1;
            else if (lane == TBC - 1) s_hi = s_above;
            if (lane < TBC && t < len) {
                const int i = (my_s - 1) >> 1;
                const bool label_state = my_s & 1;
                if (path) path[t] = label_state ? tgt[i] : blank;
                if (spans && label_state) {
                    if (s_lo != my_s) spans[2 * i] = t;
                    if (s_hi != my_s) spans[2 * i + 1] = t + 1;
                }
            }
            s_above = __builtin_amdgcn_readlane(my_s, 0);
        }
    } else if (path) {
        for (int t = lane; t < len; t += 64) path[t] = -1;
    }
    if (path)
        for (int t = len + lane; t < T; t += 64) path[t] = -1;
    if (spans)
        for (int i = (sfin >= 0 ? L : 0) + lane; i < mtl; i += 64) spans[2 * i] = spans[2 * i + 1] = -1;
}

template <int K, bool FWD, int VIT>
static void align_launch(const AlignArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((ctc_align_kernel<K, FWD, VIT>), dim3((unsigned)a.N), dim3(64), 0, st, a);
}

template <int K>
static void align_dispatch(const AlignArgs& a, bool fwd, int vit, hipStream_t st) {
    if (fwd) {
        if (vit == 0) align_launch<K, true, 0>(a, st);
        else if (vit == 1) align_launch<K, true, 1>(a, st);
        else align_launch<K, true, 2>(a, st);
    } else {
        if (vit == 1) align_launch<K, false, 1>(a, st);
        else align_launch<K, false, 2>(a, st);
    }
}

}  // namespace asr

extern "C" {

size_t asr_ctc_align_workspace_bytes(int T, int N, int max_target_len) {
    if (T <= 0 || N <= 0 || max_target_len < 0 || max_target_len > 511) return 0;
    const size_t row = 64u * (size_t)asr::align_word_bytes(asr::align_k(max_target_len));
    return ((size_t)N * (size_t)T * row + 15u) & ~(size_t)15u;
}

int asr_ctc_align(const float* d_emis, int T, int B, int V, long frame_stride, long utt_stride,
                  const int32_t* d_lengths, int is_log, int blank, const int32_t* d_targets, long ldt,
                  const int32_t* d_target_lengths, const int32_t* d_utt, int N, int max_target_len,
                  double* d_score, double* d_vscore, int32_t* d_path, long ldp, int32_t* d_spans, void* d_work,
                  asr_stream_t s) {
    if (!d_emis || !d_targets || !d_target_lengths || T <= 0 || B <= 0 || V <= 0 || N <= 0) return ASR_ERR_ARG;
    if (max_target_len < 0 || max_target_len > 511 || V > 4096) return ASR_ERR_UNSUPPORTED;
    if (blank < 0 || blank >= V || ldt < max_target_len) return ASR_ERR_ARG;
    if (!d_score && !d_vscore && !d_path && !d_spans) return ASR_ERR_ARG;
    if (d_path && ldp < T) return ASR_ERR_ARG;
    if ((d_path || d_spans) && !d_work) return ASR_ERR_ARG;
    if (!d_utt && N > B) return ASR_ERR_ARG;

    asr::AlignArgs a;
    a.emis = d_emis;
    a.frame_stride = frame_stride;
    a.utt_stride = utt_stride;
    a.lengths = d_lengths;
    a.targets = d_targets;
    a.ldt = ldt;
    a.target_lengths = d_target_lengths;
    a.utt = d_utt;
    a.score = d_score;
    a.vscore = d_vscore;
    a.path = d_path;
    a.ldp = ldp;
    a.spans = d_spans;
    a.work = d_work;
    a.T = T;
    a.B = B;
    a.V = V;
    a.N = N;
    a.max_target_len = max_target_len;
    a.is_log = is_log;
    a.blank = blank;
    const bool fwd = d_score != nullptr;
    const int vit = (d_path || d_spans) ? 2 : d_vscore ? 1 : 0;
    hipStream_t st = asr_stream(s);
    switch (asr::align_k(max_target_len)) {
        case 1: asr::align_dispatch<1>(a, fwd, vit, st); break;
        case 2: asr::align_dispatch<2>(a, fwd, vit, st); break;
        case 4: asr::align_dispatch<4>(a, fwd, vit, st); break;
        case 8: asr::align_dispatch<8>(a, fwd, vit, st); break;
        default: asr::align_dispatch<16>(a, fwd, vit, st); break;
    }
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

}  // extern "C"
