// The back-off n-gram model's tables and the per-token lookup, shared by the
// scorer (lm.hip) and the LM-fused beam searches (ctc_lm.hip, rnnt_beam.hip).
// The layout and the two walks are described at the head of lm.hip.
#pragma once
#include "asr_internal.h"

namespace asr {

constexpr int LM_CTX = ASR_LM_MAX_ORDER - 1;   // longest context

struct LmNode {
    float p;          // log10 probability; +inf: inserted node, no probability
    float bo;         // log10 back-off weight
    uint32_t child;   // first child at the next level
};

// Host or device pointers, by where it is used.  Index k = order, 1-based.
struct LmTables {
    const int32_t* words[ASR_LM_MAX_ORDER + 1];   // [k][n_k], k >= 2
    const LmNode* nodes[ASR_LM_MAX_ORDER + 1];    // [k][n_k + 1]
    int order, vocab, bos, eos, unk;
    float oov;
};

struct LmTok {
    double v;
    int order, oov;
};

// Index of `key` in the sorted words[lo, hi), or -1.
__host__ __device__ static inline long lm_find(const int32_t* __restrict__ words, uint32_t lo, uint32_t hi,
                                               int32_t key) {
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;   // lo + hi < 2^32: a level has < 2^31 nodes
        const int32_t v = words[mid];
        if (v == key) return (long)mid;
        if (v < key) lo = mid + 1;
        else hi = mid;
    }
    return -1;
}

// Position i of a hypothesis of L tokens (i == L: </s>).
__host__ __device__ static inline LmTok lm_position(const LmTables& t, const int32_t* __restrict__ tok, int L,
                                                    int i, int flags) {
    LmTok r;
    r.oov = 0;
    int32_t w = i < L ? tok[i] : t.eos;
    if (w < 0 || w >= t.vocab) {
        r.oov = 1;
        if (t.unk < 0) {
            r.v = (double)t.oov;
            r.order = 0;
            return r;
        }
        w = t.unk;
    }
    // context, most recent first: ctx[j-1] = token i-j
    int32_t ctx[LM_CTX];
    int m = 0;
    bool open = true;
#pragma unroll
    for (int j = 1; j <= LM_CTX; j++) {
        ctx[j - 1] = 0;
        if (open && j < t.order) {
            const int p = i - j;
            if (p >= 0) {
                int32_t c = tok[p];
                if (c < 0 || c >= t.vocab) c = t.unk;
                if (c < 0) open = false;   // an OOV without <unk> cuts the context
                else {
                    ctx[j - 1] = c;
                    m = j;
                }
            } else {
                if (p == -1 && (flags & ASR_LM_BOS)) {
                    ctx[j - 1] = t.bos;
                    m = j;
                }
                open = false;
            }
        }
    }
    // match walk: w, ctx[0], ctx[1], ..
    float P = t.nodes[1][w].p;
    int q = 1;
    {
        uint32_t lo = t.nodes[1][w].child, hi = t.nodes[1][w + 1].child;
        bool alive = true;
#pragma unroll
        for (int j = 1; j <= LM_CTX; j++) {
            if (alive && j <= m) {
                const long idx = lm_find(t.words[j + 1], lo, hi, ctx[j - 1]);
                if (idx < 0) alive = false;
                else {
                    const LmNode nd = t.nodes[j + 1][idx];
                    if (nd.p <= 0.0f) {
                        P = nd.p;
                        q = j + 1;
                    }
                    if (j < m) {
                        lo = nd.child;
                        hi = t.nodes[j + 1][idx + 1].child;
                    }
                }
            }
        }
    }
    // back-off walk: ctx[0], ctx[1], ..; bo[j-1] = back-off of the context of length j
    float bo[LM_CTX];
#pragma unroll
    for (int j = 0; j < LM_CTX; j++) bo[j] = 0.0f;
    if (q <= m) {
        const int32_t c0 = ctx[0];
        bo[0] = t.nodes[1][c0].bo;
        uint32_t lo = t.nodes[1][c0].child, hi = t.nodes[1][c0 + 1].child;
        bool alive = true;
#pragma unroll
        for (int j = 2; j <= LM_CTX; j++) {
            if (alive && j <= m) {
                const long idx = lm_find(t.words[j], lo, hi, ctx[j - 1]);
                if (idx < 0) alive = false;
                else {
                    const LmNode nd = t.nodes[j][idx];
                    bo[j - 1] = nd.bo;
                    if (j < m) {
                        lo = nd.child;
                        hi = t.nodes[j][idx + 1].child;
                    }
                }
            }
        }
    }
    double v = 0.0;
#pragma unroll
    for (int j = LM_CTX; j >= 1; j--)
        if (j <= m && j >= q) v += (double)bo[j - 1];
    v += (double)P;
    r.v = v;
    r.order = q;
    return r;
}

// The LM value of token `w` after a prefix whose last m = min(n, 7) tokens are
// ctx[0..m): exactly lm_position() at position n of the prefix's token row (a
// context never reaches further back than 7 tokens; <s> is in reach iff n < 7).
__host__ __device__ static inline double lm_value_after(const LmTables& t, const int32_t* ctx, int m, int32_t w,
                                                        bool eos, int flags) {
    int32_t tk[LM_CTX + 1];
#pragma unroll
    for (int j = 0; j < LM_CTX; j++) tk[j] = j < m ? ctx[j] : 0;
    tk[LM_CTX] = 0;
    if (!eos) tk[m] = w;
    return lm_position(t, tk, eos ? m : m + 1, m, flags & ASR_LM_BOS).v;
}

}  // namespace asr

// A handle's tables (lm.hip): *host always; *dev and the return value 1 once
// asr_lm_upload has run, else 0.  The pointers live as long as the handle.
struct asr_lm;
int asr_internal_lm_tables(const asr_lm* h, const asr::LmTables** host, const asr::LmTables** dev);
