// ============================================================================
// CTC prefix beam search with n-gram LM shallow fusion on gfx950 (DESIGN.md §21;
// the contract is in include/asr_amd.h): the reference search of DESIGN §2 in
// which the prune and the final ranking compare pathScore + W(prefix), W the
// per-prefix LM weight.  A new kernel with its own handle: the existing decoder
// kernels rest on filters proven for "prefix score + one emission" and are not
// touched.
//
// Device: one workgroup of 256 threads per utterance, the beam on chip in LDS
// for all frames, two buffers.  A slot is a prefix q: the fp64 scores of "q" and
// "q$", W, L, n, the last 7 token ids, a 64-bit hash of the string, its node
// record and its parent's.  Per frame:
//   pairs   every (slot, candidate label) over all lanes: the child "qc" is
//           looked up in an LDS hash table of the live prefixes (hash, length,
//           last label, then the parents' node chains compared).  A live child
//           gets its whole new score here (the reference's fold order: "q",
//           then "q$" / "qc" by code order); a new one gets its score, its LM
//           value (lm_position, a chain of dependent global loads) and its key;
//   slots   "q$" of every slot, the repeat of a slot whose parent is not live;
//   select  the (beam+1)-th largest order-preserving u64 key, exact, by an
//           8-pass byte radix select over the LDS keys and the pair keys;
//   write   survivors into the other buffer, node records (parent node, label)
//           of the new prefixes to HBM, the hash table rebuilt.
// The host twin (asr_ctc_lm_decode_host) is the same rule set written over
// std::map / std::set, one thread, no HIP call.
//
// Word mode (asr_ctc_lm_create_word): character labels and a
// word-level LM.  A slot also carries its node in a lexicon trie (asr_lexicon_*:
// three flat arrays in HBM, breadth-first) and its word count; W moves only when a
// space ends a word, and the closed mode drops pairs the trie does not have.  The
// frame loop is one template, instantiated once per mode.
// ============================================================================
#include "ctc_lse.h"
#include "lm_tables.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <new>
#include <set>
#include <vector>

namespace asr {

constexpr int CLM_NT = 256;       // threads per utterance
constexpr int CLM_HT = 512;       // hash-table cells (>= 2 x the slot capacity)
constexpr int CLM_MAXC = 255;     // candidate non-blank labels per frame
constexpr int CLM_VMAX = 4096;
constexpr uint64_t CLM_HASH0 = 0x243F6A8885A308D3ull;

struct ClmArgs {
    LmTables lm;
    const float* emis;      // element (t, b, v) at emis[t*tstride + b*ustride + v]
    long tstride, ustride;
    const int32_t* lengths; // [B] frames per utterance (device)
    int T, B, is_log;
    int V, blank, beam, kcap, nc, flags;
    double aln10, beta;
    const int32_t* codes;   // [V]
    const int32_t* tok;     // [V] LM token of a label
    const int32_t* cand;    // [B][T][nc] candidate labels per frame (top_n), or NULL: every label
    int2* nodes;            // [B][T*kcap] (parent node, label)
    uint64_t* ckey;         // [B][kcap*nc] fused key of a new prefix (0: none)
    double* cscore;         // [B][kcap*nc] its score
    double* cv;             // [B][kcap*nc] its last token's LM value
    int32_t* fin_n;         // [B] final hypotheses
    int32_t* status;        // [B] 1 = beam overflow
    int32_t* fin_node;      // [B][kcap]
    int32_t* fin_len;       // [B][kcap]
    double* fin_total;      // [B][kcap]
    double* fin_ctc;        // [B][kcap]
    double* fin_lm;         // [B][kcap]
};

// The lexicon trie of the word mode, breadth-first: node 0 is the
// root and the children of node i are the nodes first[i] .. first[i+1], their
// labels ascending, so a child is found as lm_find finds a word.
struct LexTables {
    const uint32_t* first;   // [nodes + 1]
    const int32_t* label;    // [nodes] the label on the edge into the node (root: -1)
    const int32_t* tok;      // [nodes] LM token of the word that ends at the node, -1: none
    int nodes, space, closed;
};
constexpr int LEX_OFF = -1;   // the partial word is no prefix of a lexicon word; never an index

struct ClmWordArgs {
    LexTables lex;
    int32_t* fin_nw;   // [B][kcap] words scored
};

// Child of node z by label c, or LEX_OFF; the arrays are read for z >= 0 only.
__host__ __device__ static inline int lex_child(const LexTables& t, int z, int c) {
    if (z < 0) return LEX_OFF;
    return (int)lm_find(t.label, t.first[z], t.first[z + 1], c);
}

// The token of the word that ends at z (z is not the root): -1, an OOV, unless z is terminal.
__host__ __device__ static inline int32_t lex_word(const LexTables& t, int z) { return z > 0 ? t.tok[z] : -1; }

__host__ __device__ static inline uint64_t clm_hash(uint64_t h, int c) {
    uint64_t x = (h ^ (uint64_t)(uint32_t)(c + 1)) * 0x9E3779B97F4A7C15ull;
    return x ^ (x >> 29);
}

__device__ __forceinline__ void clm_fold(double& acc, bool& have, double x, bool px) {
    if (!px) return;
    if (!have) {
        acc = x;
        have = true;
    } else {
        acc = lse2(acc, x);
    }
}

// Word mode: two more ints per slot and buffer (the trie node and the word count).
__host__ __device__ static inline size_t clm_lds_bytes(int kc, bool word = false) {
    return (size_t)kc * (word ? 228 : 212) + 256 * 8 + 256 * 4 + CLM_HT * 4 + 256 * 4 + 16 * 4;
}

enum { M_NSTATE = 0, M_NNEW, M_NODES, M_BUCKET, M_KREM, M_ALL };

// WORD: the word mode.  s_n stays the label count (the hash match
// and the trace need it), s_nw counts the words scored, s_z is the trie node of the
// partial word and s_ctx holds word tokens; W moves only when a space ends a word.
template <bool WORD>
__device__ __forceinline__ void clm_search(const ClmArgs& a, const ClmWordArgs& wa, unsigned char* smem) {
    const int KC = a.kcap, NC = a.nc;
    const int tid = threadIdx.x;
    const long ub = blockIdx.x;
    // LDS carve-up: 8-byte arrays first
    double* s_nb = (double*)smem;              // [2][KC] score of "q"
    double* s_b = s_nb + 2 * KC;               // [2][KC] score of "q$"
    double* s_W = s_b + 2 * KC;                // [2][KC]
    double* s_L = s_W + 2 * KC;                // [2][KC]
    uint64_t* s_hash = (uint64_t*)(s_L + 2 * KC);   // [2][KC]
    double* t_nb = (double*)(s_hash + 2 * KC); // [KC] new score of "q"
    double* t_b = t_nb + KC;                   // [KC] new score of "q$"
    uint64_t* k_nb = (uint64_t*)(t_b + KC);    // [KC] fused keys (0: absent)
    uint64_t* k_b = k_nb + KC;                 // [KC]
    double* s_ce = (double*)(k_b + KC);        // [256] log emission of candidate j
    int* s_n = (int*)(s_ce + 256);             // [2][KC] tokens of the prefix
    int* s_node = s_n + 2 * KC;                // [2][KC] node record (-1: empty prefix)
    int* s_pnode = s_node + 2 * KC;            // [2][KC] the parent's node record
    int* s_last = s_pnode + 2 * KC;            // [2][KC] last label (-1: empty prefix)
    int* s_fl = s_last + 2 * KC;               // [2][KC] bit 0: "q" present, bit 1: "q$" present
    int* s_ctx = s_fl + 2 * KC;                // [2][KC][7] last tokens, oldest first
    int* s_hnd = s_ctx + 2 * KC * LM_CTX;      // [KC] bit 0: new "q" score set by its parent's pair, bit 1: present
    int* s_clab = s_hnd + KC;                  // [256] candidate labels of the frame
    int* s_ht = s_clab + 256;                  // [CLM_HT] slot of a live prefix, -1: free
    unsigned* s_hist = (unsigned*)(s_ht + CLM_HT);   // [256]
    int* s_misc = (int*)(s_hist + 256);        // [16]
    int* s_z = s_misc + 16;                    // [2][KC] word mode: trie node (0: root, LEX_OFF)
    int* s_nw = s_z + 2 * KC;                  // [2][KC] word mode: words scored

    int len = a.lengths ? a.lengths[ub] : a.T;
    len = min(max(len, 1), a.T);
    int2* const nodes = a.nodes + ub * ((long)a.T * KC);
    uint64_t* const ckey = a.ckey + ub * ((long)KC * NC);
    double* const cscore = a.cscore + ub * ((long)KC * NC);
    double* const cv = a.cv + ub * ((long)KC * NC);
    const int code_blank = a.codes[a.blank];

    // the state before frame 0: "$" with score log 1, so that frame 0 is a frame like any other
    if (tid == 0) {
        s_nb[0] = 0.0;
        s_b[0] = 0.0;
        s_W[0] = 0.0;
        s_L[0] = 0.0;
        s_hash[0] = CLM_HASH0;
        s_n[0] = 0;
        s_node[0] = -1;
        s_pnode[0] = -2;
        s_last[0] = -1;
        s_fl[0] = 2;
        s_misc[M_NODES] = 0;
        if constexpr (WORD) {
            s_z[0] = 0;
            s_nw[0] = 0;
        }
    }
    for (int i = tid; i < CLM_HT; i += CLM_NT) s_ht[i] = -1;
    __syncthreads();
    if (tid == 0) s_ht[(int)(CLM_HASH0 & (CLM_HT - 1))] = 0;
    __syncthreads();

    int cur = 0, ns = 1;
    bool overflow = false;
    for (int t = 0; t < len; t++) {
        const float* const e = a.emis + (long)t * a.tstride + ub * a.ustride;
        for (int j = tid; j < NC; j += CLM_NT) {
            int c = a.cand ? a.cand[(ub * a.T + t) * NC + j] : j + (j >= a.blank ? 1 : 0);
            c = min(max(c, 0), a.V - 1);
            s_clab[j] = c;
            const double x = (double)e[c];
            s_ce[j] = a.is_log ? x : log(x);
        }
        double e_bl = (double)e[a.blank];
        if (!a.is_log) e_bl = log(e_bl);
        for (int s = tid; s < ns; s += CLM_NT) s_hnd[s] = 0;
        if (tid == 0) {
            s_misc[M_NSTATE] = 0;
            s_misc[M_NNEW] = 0;
        }
        __syncthreads();

        const int o = cur * KC;
        const int npairs = ns * NC;
        // ---- pairs
        for (int p = tid; p < npairs; p += CLM_NT) {
            const int s = p / NC, j = p - s * NC;
            const int c = s_clab[j];
            const double ec = s_ce[j];
            const int fl = s_fl[o + s];
            double acc = 0.0;
            bool have = false;
            clm_fold(acc, have, s_nb[o + s] + ec, (fl & 1) && s_last[o + s] != c);   // "q" + c
            const double viaBlank = s_b[o + s] + ec;                                  // "q$" + c
            const bool pBlank = (fl & 2) != 0;
            // is "qc" live?
            const uint64_t hc = clm_hash(s_hash[o + s], c);
            const int nq = s_n[o + s];
            int r = -1;
            for (int cell = (int)(hc & (CLM_HT - 1));; cell = (cell + 1) & (CLM_HT - 1)) {
                const int x = s_ht[cell];
                if (x < 0) break;
                if (s_hash[o + x] == hc && s_n[o + x] == nq + 1 && s_last[o + x] == c) {
                    int pa = s_pnode[o + x], pb = s_node[o + s];
                    bool same = true;
                    while (pa != pb) {   // equal lengths: both chains end at -1 together
                        if (pa < 0 || pb < 0) {
                            same = false;
                            break;
                        }
                        const int2 ra = nodes[pa], rb = nodes[pb];
                        if (ra.y != rb.y) {
                            same = false;
                            break;
                        }
                        pa = ra.x;
                        pb = rb.x;
                    }
                    if (same) {
                        r = x;
                        break;
                    }
                }
            }
            if (r >= 0) {
                const bool pRep = (s_fl[o + r] & 1) != 0;
                const double rep = s_nb[o + r] + ec;   // "qc" + c
                if (code_blank < a.codes[c]) {
                    clm_fold(acc, have, viaBlank, pBlank);
                    clm_fold(acc, have, rep, pRep);
                } else {
                    clm_fold(acc, have, rep, pRep);
                    clm_fold(acc, have, viaBlank, pBlank);
                }
                t_nb[r] = acc;
                s_hnd[r] = 1 | (have ? 2 : 0);
                ckey[p] = 0;
            } else {
                clm_fold(acc, have, viaBlank, pBlank);
                if (!have) {
                    ckey[p] = 0;
                } else if constexpr (WORD) {
                    const int z = s_z[o + s];
                    const bool sp = c == wa.lex.space;
                    // closed: a letter needs a child in the trie, a space a finished word
                    const bool ok =
                        !wa.lex.closed || (sp ? (z > 0 && wa.lex.tok[z] >= 0) : lex_child(wa.lex, z, c) >= 0);
                    if (!ok) {
                        ckey[p] = 0;
                    } else {
                        double v = 0.0, Wn = s_W[o + s];
                        if (sp && z != 0) {   // the space ends a word: the one LM lookup
                            v = lm_value_after(a.lm, s_ctx + (o + s) * LM_CTX, min(s_nw[o + s], LM_CTX), lex_word(wa.lex, z),
                                          false, a.flags);
                            Wn = Wn + ((a.aln10 * v) + a.beta);
                        }
                        ckey[p] = asr_d2key(acc + Wn);
                        cscore[p] = acc;
                        cv[p] = v;
                    }
                } else {
                    const double v = lm_value_after(a.lm, s_ctx + (o + s) * LM_CTX, min(nq, LM_CTX), a.tok[c], false, a.flags);
                    const double Wn = s_W[o + s] + ((a.aln10 * v) + a.beta);
                    ckey[p] = asr_d2key(acc + Wn);
                    cscore[p] = acc;
                    cv[p] = v;
                }
            }
        }
        // ---- slots: "q$"
        for (int s = tid; s < ns; s += CLM_NT) {
            const int fl = s_fl[o + s];
            double acc = 0.0;
            bool have = false;
            clm_fold(acc, have, s_nb[o + s] + e_bl, (fl & 1) != 0);
            clm_fold(acc, have, s_b[o + s] + e_bl, (fl & 2) != 0);
            t_b[s] = acc;   // a live slot has at least one state
        }
        __syncthreads();
        // ---- slots: the repeat of a prefix whose parent is not live, and the keys
        for (int s = tid; s < ns; s += CLM_NT) {
            int hd = s_hnd[s];
            if (!(hd & 1)) {
                const int c = s_last[o + s];
                int j = -1;
                if ((s_fl[o + s] & 1) && c >= 0)
                    for (int i = 0; i < NC; i++)
                        if (s_clab[i] == c) {
                            j = i;
                            break;
                        }
                if (j >= 0) {
                    t_nb[s] = s_nb[o + s] + s_ce[j];
                    hd = 3;
                } else {
                    hd = 1;
                }
                s_hnd[s] = hd;
            }
            const double W = s_W[o + s];
            k_nb[s] = (hd & 2) ? asr_d2key(t_nb[s] + W) : 0ull;
            k_b[s] = asr_d2key(t_b[s] + W);
        }
        __syncthreads();
        // ---- the (beam+1)-th largest key: byte radix select, most significant byte first
        uint64_t prefix = 0;
        int krem = a.beam + 1;
        bool all = false;
        for (int byte = 7; byte >= 0; byte--) {
            s_hist[tid] = 0;
            __syncthreads();
            const int sh = 8 * byte;
            for (int i = tid; i < 2 * ns; i += CLM_NT) {
                const uint64_t k = i < ns ? k_nb[i] : k_b[i - ns];
                if (k && (byte == 7 || (k >> (sh + 8)) == (prefix >> (sh + 8)))) atomicAdd(&s_hist[(k >> sh) & 255], 1u);
            }
            for (int p = tid; p < npairs; p += CLM_NT) {
                const uint64_t k = ckey[p];
                if (k && (byte == 7 || (k >> (sh + 8)) == (prefix >> (sh + 8)))) atomicAdd(&s_hist[(k >> sh) & 255], 1u);
            }
            __syncthreads();
            if (tid < 64) {
                // lane l owns bins 255-4l .. 252-4l: an exclusive prefix over the lanes, from the top bin down
                const unsigned h0 = s_hist[255 - 4 * tid], h1 = s_hist[254 - 4 * tid], h2 = s_hist[253 - 4 * tid],
                               h3 = s_hist[252 - 4 * tid];
                const unsigned mine = h0 + h1 + h2 + h3;
                unsigned incl = mine;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const unsigned y = __shfl_up(incl, off);
                    if (tid >= off) incl += y;
                }
                const unsigned total = __shfl(incl, 63);
                unsigned above = incl - mine;
                if (byte == 7 && total <= (unsigned)a.beam) {
                    if (tid == 0) s_misc[M_ALL] = 1;
                } else {
                    if (tid == 0) s_misc[M_ALL] = 0;
                    if (above < (unsigned)krem && incl >= (unsigned)krem) {   // exactly one lane
                        int bucket = 255 - 4 * tid;
                        if (above + h0 < (unsigned)krem) {
                            above += h0;
                            bucket--;
                            if (above + h1 < (unsigned)krem) {
                                above += h1;
                                bucket--;
                                if (above + h2 < (unsigned)krem) {
                                    above += h2;
                                    bucket--;
                                }
                            }
                        }
                        s_misc[M_BUCKET] = bucket;
                        s_misc[M_KREM] = krem - (int)above;
                    }
                }
            }
            __syncthreads();
            if (s_misc[M_ALL]) {
                all = true;
                break;
            }
            prefix |= (uint64_t)(unsigned)s_misc[M_BUCKET] << sh;
            krem = s_misc[M_KREM];
        }
        const uint64_t cut = all ? 1ull : prefix;
        // ---- survivors: count the states, refuse an overflow before anything is written
        {
            int cnt = 0;
            for (int s = tid; s < ns; s += CLM_NT) cnt += (k_nb[s] >= cut ? 1 : 0) + (k_b[s] >= cut ? 1 : 0);
            for (int p = tid; p < npairs; p += CLM_NT) cnt += ckey[p] >= cut ? 1 : 0;
            if (cnt) atomicAdd(&s_misc[M_NSTATE], cnt);
        }
        __syncthreads();
        if (s_misc[M_NSTATE] > KC) {
            overflow = true;
            break;
        }
        const int o2 = (cur ^ 1) * KC;
        for (int s = tid; s < ns; s += CLM_NT) {
            const bool sn = k_nb[s] >= cut, sb = k_b[s] >= cut;
            if (sn || sb) {
                const int d = o2 + atomicAdd(&s_misc[M_NNEW], 1);
                s_nb[d] = t_nb[s];
                s_b[d] = t_b[s];
                s_W[d] = s_W[o + s];
                s_L[d] = s_L[o + s];
                s_hash[d] = s_hash[o + s];
                s_n[d] = s_n[o + s];
                s_node[d] = s_node[o + s];
                s_pnode[d] = s_pnode[o + s];
                s_last[d] = s_last[o + s];
                s_fl[d] = (sn ? 1 : 0) | (sb ? 2 : 0);
#pragma unroll
                for (int i = 0; i < LM_CTX; i++) s_ctx[d * LM_CTX + i] = s_ctx[(o + s) * LM_CTX + i];
                if constexpr (WORD) {
                    s_z[d] = s_z[o + s];
                    s_nw[d] = s_nw[o + s];
                }
            }
        }
        for (int p = tid; p < npairs; p += CLM_NT) {
            if (ckey[p] >= cut) {
                const int s = p / NC, j = p - s * NC;
                const int c = s_clab[j];
                const double v = cv[p];
                const int d = o2 + atomicAdd(&s_misc[M_NNEW], 1);
                const int nid = atomicAdd(&s_misc[M_NODES], 1);   // < T*KC: at most KC new prefixes per frame
                nodes[nid] = make_int2(s_node[o + s], c);
                if constexpr (WORD) {
                    const int z = s_z[o + s];
                    const bool sp = c == wa.lex.space;
                    const bool scored = sp && z != 0;   // the space ended a word: v is its value
                    const int nw = s_nw[o + s];
                    const int m = min(nw, LM_CTX);
                    const int32_t tk = scored ? lex_word(wa.lex, z) : 0;
                    s_nb[d] = cscore[p];
                    s_b[d] = 0.0;
                    s_W[d] = scored ? s_W[o + s] + ((a.aln10 * v) + a.beta) : s_W[o + s];
                    s_L[d] = scored ? s_L[o + s] + v : s_L[o + s];
                    s_hash[d] = clm_hash(s_hash[o + s], c);
                    s_n[d] = s_n[o + s] + 1;
                    s_node[d] = nid;
                    s_pnode[d] = s_node[o + s];
                    s_last[d] = c;
                    s_fl[d] = 1;
                    s_z[d] = sp ? 0 : lex_child(wa.lex, z, c);
                    s_nw[d] = nw + (scored ? 1 : 0);
#pragma unroll
                    for (int i = 0; i < LM_CTX; i++) {
                        int y;
                        if (!scored) y = s_ctx[(o + s) * LM_CTX + i];
                        else if (m < LM_CTX) y = i < m ? s_ctx[(o + s) * LM_CTX + i] : (i == m ? tk : 0);
                        else y = i < LM_CTX - 1 ? s_ctx[(o + s) * LM_CTX + i + 1] : tk;
                        s_ctx[d * LM_CTX + i] = y;
                    }
                } else {
                    s_nb[d] = cscore[p];
                    s_b[d] = 0.0;
                    s_W[d] = s_W[o + s] + ((a.aln10 * v) + a.beta);
                    s_L[d] = s_L[o + s] + v;
                    s_hash[d] = clm_hash(s_hash[o + s], c);
                    const int nq = s_n[o + s];
                    s_n[d] = nq + 1;
                    s_node[d] = nid;
                    s_pnode[d] = s_node[o + s];
                    s_last[d] = c;
                    s_fl[d] = 1;
                    const int m = min(nq, LM_CTX);
                    const int32_t tk = a.tok[c];
#pragma unroll
                    for (int i = 0; i < LM_CTX; i++) {
                        int x;
                        if (m < LM_CTX) x = i < m ? s_ctx[(o + s) * LM_CTX + i] : (i == m ? tk : 0);
                        else x = i < LM_CTX - 1 ? s_ctx[(o + s) * LM_CTX + i + 1] : tk;
                        s_ctx[d * LM_CTX + i] = x;
                    }
                }
            }
        }
        for (int i = tid; i < CLM_HT; i += CLM_NT) s_ht[i] = -1;
        __syncthreads();
        ns = s_misc[M_NNEW];
        cur ^= 1;
        for (int s = tid; s < ns; s += CLM_NT) {
            for (int cell = (int)(s_hash[cur * KC + s] & (CLM_HT - 1));; cell = (cell + 1) & (CLM_HT - 1))
                if (atomicCAS(&s_ht[cell], -1, s) == -1) break;
        }
        __syncthreads();
    }

    if (overflow) {
        if (tid == 0) {
            a.fin_n[ub] = 0;
            a.status[ub] = 1;
        }
    } else {
        // the final "q" / "q$" merge and the totals
        const int o = cur * KC;
        for (int s = tid; s < ns; s += CLM_NT) {
            const int fl = s_fl[o + s];
            double acc = 0.0;
            bool have = false;
            clm_fold(acc, have, s_nb[o + s], (fl & 1) != 0);
            clm_fold(acc, have, s_b[o + s], (fl & 2) != 0);
            double total, L;
            if constexpr (WORD) {
                int32_t ctx[LM_CTX];
#pragma unroll
                for (int i = 0; i < LM_CTX; i++) ctx[i] = s_ctx[(o + s) * LM_CTX + i];
                double W = s_W[o + s];
                L = s_L[o + s];
                int nw = s_nw[o + s];
                const int z = s_z[o + s];
                if (z != 0) {   // the pending word, scored as a space would score it
                    const int m = min(nw, LM_CTX);
                    const int32_t tk = lex_word(wa.lex, z);
                    const double v = lm_value_after(a.lm, ctx, m, tk, false, a.flags);
                    W = W + ((a.aln10 * v) + a.beta);
                    L = L + v;
#pragma unroll
                    for (int i = 0; i < LM_CTX; i++) {
                        if (m < LM_CTX) ctx[i] = i == m ? tk : ctx[i];
                        else ctx[i] = i < LM_CTX - 1 ? ctx[i + 1] : tk;
                    }
                    nw++;
                }
                total = acc + W;
                if (a.flags & ASR_LM_EOS) {
                    const double v = lm_value_after(a.lm, ctx, min(nw, LM_CTX), 0, true, a.flags);
                    total = total + (a.aln10 * v);
                    L = L + v;
                }
                wa.fin_nw[ub * KC + s] = nw;
            } else {
                total = acc + s_W[o + s];
                L = s_L[o + s];
                if (a.flags & ASR_LM_EOS) {
                    const double v = lm_value_after(a.lm, s_ctx + (o + s) * LM_CTX, min(s_n[o + s], LM_CTX), 0, true, a.flags);
                    total = total + (a.aln10 * v);
                    L = L + v;
                }
            }
            const long d = ub * KC + s;
            a.fin_node[d] = s_node[o + s];
            a.fin_len[d] = s_n[o + s];
            a.fin_total[d] = total;
            a.fin_ctc[d] = acc;
            a.fin_lm[d] = L;
        }
        if (tid == 0) {
            a.fin_n[ub] = ns;
            a.status[ub] = 0;
        }
    }
}

__global__ __launch_bounds__(CLM_NT) void ctc_lm_kernel(const ClmArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    clm_search<false>(a, ClmWordArgs{}, smem);
}

__global__ __launch_bounds__(CLM_NT) void ctc_wordlm_kernel(const ClmArgs a, const ClmWordArgs wa) {
    extern __shared__ __align__(16) unsigned char smem[];
    clm_search<true>(a, wa, smem);
}

// The label cutoff: one wave per (frame, utterance) ranks the non-blank labels by
// (emission descending, label id ascending) and writes the first nc.
__global__ __launch_bounds__(64) void ctc_lm_topn_kernel(const float* emis, long tstride, long ustride,
                                                         const int32_t* lengths, int T, int V, int blank, int nc,
                                                         int32_t* cand) {
    __shared__ float se[CLM_VMAX];
    const long ub = blockIdx.x / T;
    const int t = (int)(blockIdx.x - ub * T);
    int len = lengths ? lengths[ub] : T;
    len = min(max(len, 1), T);
    if (t >= len) return;   // wave-uniform
    const float* const e = emis + (long)t * tstride + ub * ustride;
    for (int v = threadIdx.x; v < V; v += 64) se[v] = e[v];
    __syncthreads();
    for (int v = threadIdx.x; v < V; v += 64) {
        if (v == blank) continue;
        const float ev = se[v];
        int rank = 0;
        for (int u = 0; u < V; u++) {
            const float eu = se[u];
            rank += (u != blank && (eu > ev || (eu == ev && u < v))) ? 1 : 0;
        }
        if (rank < nc) cand[(ub * T + t) * nc + rank] = v;
    }
}

// Labels of every final hypothesis, by its node chain: lab[b][k][0..len).
__global__ void ctc_lm_trace_kernel(const int2* nodes, long nodes_per_utt, const int32_t* fin_n,
                                    const int32_t* fin_node, const int32_t* fin_len, int kcap, int max_len, int B,
                                    uint16_t* lab) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * kcap) return;
    const long ub = i / kcap;
    const int k = (int)(i - ub * kcap);
    if (k >= fin_n[ub]) return;
    const int2* const nd = nodes + ub * nodes_per_utt;
    int node = fin_node[i];
    uint16_t* const out = lab + i * max_len;
    for (int pos = fin_len[i] - 1; pos >= 0 && node >= 0; pos--) {
        const int2 r = nd[node];
        if (pos < max_len) out[pos] = (uint16_t)r.y;
        node = r.x;
    }
}

// ------------------------------------------------------------------ host twin
typedef std::vector<int32_t> ClmStr;   // a state string: symbol codes

static inline double clm_lse_host(double x, double y) {
    if (x == -INFINITY) return y;
    if (y == -INFINITY) return x;
    const double m = x > y ? x : y;
    return m + std::log1p(std::exp(-std::fabs(x - y)));
}

struct ClmPrefix {
    double W = 0.0, L = 0.0;
    int n = 0;    // tokens scored (word mode: words)
    int z = 0;    // word mode: trie node of the partial word (0: root, LEX_OFF)
    int32_t ctx[LM_CTX] = {};
};

struct ClmHyp {
    std::vector<int32_t> labels;
    ClmStr str;
    double total, ctc, lm;
    int n;
};

}  // namespace asr

struct asr_lexicon {
    int V = 0, space = 0, words = 0, max_children = 0;
    std::vector<uint32_t> first;
    std::vector<int32_t> label, tok;
    std::vector<char> used;   // [V] the label occurs in a spelling
    void* d_blob = nullptr;
    const uint32_t* d_first = nullptr;
    const int32_t *d_label = nullptr, *d_tok = nullptr;

    asr::LexTables tables(bool dev, int closed) const {
        asr::LexTables t;
        t.first = dev ? d_first : first.data();
        t.label = dev ? d_label : label.data();
        t.tok = dev ? d_tok : tok.data();
        t.nodes = (int)label.size();
        t.space = space;
        t.closed = closed;
        return t;
    }
};

struct asr_ctc_lm {
    int V = 0, beam = 0, blank = 0, kcap = 0, nc = 0, top_n = 0, flags = 0;
    double aln10 = 0.0, beta = 0.0;
    const asr_lm* lm = nullptr;
    const asr_lexicon* lex = nullptr;   // word mode
    int closed = 0;
    int32_t* d_fin_nw = nullptr;
    std::vector<int32_t> codes, tok;
    // results of the last decode
    int state = 0;   // 0: none, 1: a device decode is queued, 2: hyps hold the results
    int lastT = 0, lastB = 0;
    std::vector<std::vector<asr::ClmHyp>> hyps;
    std::vector<int> overflow;
    std::vector<double> gaps;   // host decodes only
    // device side (allocated at the first device decode)
    int32_t* d_codes = nullptr;
    int32_t* d_tok = nullptr;
    int32_t* d_lengths = nullptr;
    int32_t* d_cand = nullptr;
    int2* d_nodes = nullptr;
    uint64_t* d_ckey = nullptr;
    double* d_cscore = nullptr;
    double* d_cv = nullptr;
    int32_t *d_fin_n = nullptr, *d_status = nullptr, *d_fin_node = nullptr, *d_fin_len = nullptr;
    double *d_fin_total = nullptr, *d_fin_ctc = nullptr, *d_fin_lm = nullptr;
    uint16_t* d_lab = nullptr;
    size_t lab_elems = 0;
    int capT = 0, capB = 0;
    int32_t* p_lengths = nullptr;   // pinned, [capB]
    hipEvent_t ev_len = nullptr;    // the last copy out of p_lengths
    bool len_queued = false;
    hipStream_t stream = nullptr;
};

namespace asr {

static void clm_free_work(asr_ctc_lm* h) {
    void* p[] = {h->d_lengths, h->d_cand, h->d_nodes, h->d_ckey, h->d_cscore, h->d_cv, h->d_fin_n, h->d_status,
                 h->d_fin_node, h->d_fin_len, h->d_fin_total, h->d_fin_ctc, h->d_fin_lm};
    for (void* q : p)
        if (q) (void)hipFree(q);
    if (h->d_fin_nw) (void)hipFree(h->d_fin_nw);
    h->d_fin_nw = nullptr;
    if (h->p_lengths) (void)hipHostFree(h->p_lengths);
    h->p_lengths = nullptr;
    h->len_queued = false;
    h->d_lengths = h->d_cand = nullptr;
    h->d_nodes = nullptr;
    h->d_ckey = nullptr;
    h->d_cscore = h->d_cv = nullptr;
    h->d_fin_n = h->d_status = h->d_fin_node = h->d_fin_len = nullptr;
    h->d_fin_total = h->d_fin_ctc = h->d_fin_lm = nullptr;
    h->capT = h->capB = 0;
}

// The workspace for T x B, sized once per shape and kept while the next shape fits.
static int clm_reserve(asr_ctc_lm* h, int T, int B) {
    if (!h->d_codes) {
        ASR_HIP_TRY(hipMalloc(&h->d_codes, sizeof(int32_t) * h->V));
        ASR_HIP_TRY(hipMalloc(&h->d_tok, sizeof(int32_t) * h->V));
        ASR_HIP_TRY(hipMemcpy(h->d_codes, h->codes.data(), sizeof(int32_t) * h->V, hipMemcpyHostToDevice));
        ASR_HIP_TRY(hipMemcpy(h->d_tok, h->tok.data(), sizeof(int32_t) * h->V, hipMemcpyHostToDevice));
    }
    if (h->d_nodes && T <= h->capT && B <= h->capB) return ASR_OK;
    ASR_HIP_TRY(hipDeviceSynchronize());   // an earlier decode may still use the old workspace
    clm_free_work(h);
    const size_t kc = (size_t)h->kcap, nb = (size_t)B, pairs = kc * (size_t)h->nc;
    if (!h->ev_len) ASR_HIP_TRY(hipEventCreateWithFlags(&h->ev_len, hipEventDisableTiming));
    ASR_HIP_TRY(hipHostMalloc(&h->p_lengths, 4 * nb, hipHostMallocDefault));
    ASR_HIP_TRY(hipMalloc(&h->d_lengths, 4 * nb));
    if (h->top_n) {
        ASR_HIP_TRY(hipMalloc(&h->d_cand, 4 * nb * (size_t)T * (size_t)h->nc));
        ASR_HIP_TRY(hipMemset(h->d_cand, 0, 4 * nb * (size_t)T * (size_t)h->nc));
    }
    ASR_HIP_TRY(hipMalloc(&h->d_nodes, sizeof(int2) * nb * (size_t)T * kc));
    ASR_HIP_TRY(hipMalloc(&h->d_ckey, 8 * nb * pairs));
    ASR_HIP_TRY(hipMalloc(&h->d_cscore, 8 * nb * pairs));
    ASR_HIP_TRY(hipMalloc(&h->d_cv, 8 * nb * pairs));
    ASR_HIP_TRY(hipMalloc(&h->d_fin_n, 4 * nb));
    ASR_HIP_TRY(hipMalloc(&h->d_status, 4 * nb));
    ASR_HIP_TRY(hipMalloc(&h->d_fin_node, 4 * nb * kc));
    ASR_HIP_TRY(hipMalloc(&h->d_fin_len, 4 * nb * kc));
    ASR_HIP_TRY(hipMalloc(&h->d_fin_total, 8 * nb * kc));
    ASR_HIP_TRY(hipMalloc(&h->d_fin_ctc, 8 * nb * kc));
    ASR_HIP_TRY(hipMalloc(&h->d_fin_lm, 8 * nb * kc));
    if (h->lex) ASR_HIP_TRY(hipMalloc(&h->d_fin_nw, 4 * nb * kc));
    h->capT = T;
    h->capB = B;
    return ASR_OK;
}

// Rank by (total descending, code string ascending).
static void clm_rank(std::vector<ClmHyp>& v) {
    std::sort(v.begin(), v.end(), [](const ClmHyp& x, const ClmHyp& y) {
        if (x.total != y.total) return x.total > y.total;
        return x.str < y.str;
    });
}

// Shared argument checks of the two decodes, in the documented order.
static int clm_check_decode(const asr_ctc_lm* h, const float* emis, int T, int B, long fs, long us,
                            const int32_t* h_lengths) {
    if (!h || !emis || T < 1 || B < 1 || fs < 1 || us < 1) return ASR_ERR_ARG;
    if (h_lengths)
        for (int b = 0; b < B; b++)
            if (h_lengths[b] < 1 || h_lengths[b] > T) return ASR_ERR_ARG;
    return ASR_OK;
}

// One utterance on the host: the rule set of the header over std::set / std::map.
static bool clm_decode_one(const asr_ctc_lm* h, const LmTables& lm, const float* emis, long fs, int len, int is_log,
                           std::vector<ClmHyp>& out, double& gap) {
    gap = INFINITY;
    auto note_gap = [&](double x, double y) {   // two scores that differ: how far apart, relatively
        if (x == y || !std::isfinite(x) || !std::isfinite(y)) return;
        gap = std::min(gap, std::fabs(x - y) / std::max(1.0, std::max(std::fabs(x), std::fabs(y))));
    };
    const int V = h->V, blank = h->blank;
    const int32_t bcode = h->codes[blank];
    std::map<int32_t, int> label_of;
    for (int v = 0; v < V; v++) label_of[h->codes[v]] = v;
    std::set<ClmStr> path, upath;
    std::map<ClmStr, double> score, uscore;
    std::map<ClmStr, ClmPrefix> info, uinfo;   // by prefix
    auto prefix_of = [&](const ClmStr& s) {
        ClmStr p = s;
        if (!p.empty() && p.back() == bcode) p.pop_back();
        return p;
    };
    const bool word = h->lex != nullptr;
    const LexTables lex = word ? h->lex->tables(false, h->closed) : LexTables{};
    // the token `tk` scored after q's context and appended to it
    auto scored = [&](const ClmPrefix& q, int32_t tk) {
        ClmPrefix c = q;
        const int m = std::min(q.n, LM_CTX);
        const double v = lm_value_after(lm, q.ctx, m, tk, false, h->flags);
        c.W = q.W + ((h->aln10 * v) + h->beta);
        c.L = q.L + v;
        c.n = q.n + 1;
        if (m < LM_CTX) c.ctx[m] = tk;
        else {
            for (int i = 0; i + 1 < LM_CTX; i++) c.ctx[i] = q.ctx[i + 1];
            c.ctx[LM_CTX - 1] = tk;
        }
        return c;
    };
    // word mode: q with its pending word (q.z is not the root) scored, back at the root
    auto word_end = [&](const ClmPrefix& q) {
        ClmPrefix c = scored(q, lex_word(lex, q.z));
        c.z = 0;
        return c;
    };
    // closed mode: does the transition q -> q + label exist?
    auto allowed = [&](const ClmPrefix& q, int label) {
        if (!word || !lex.closed) return true;
        if (label == lex.space) return q.z > 0 && lex.tok[q.z] >= 0;
        return lex_child(lex, q.z, label) >= 0;
    };
    auto child = [&](const ClmPrefix& q, int label) {
        if (word) {
            if (label != lex.space) {
                ClmPrefix c = q;
                c.z = lex_child(lex, q.z, label);
                return c;
            }
            return q.z == 0 ? q : word_end(q);   // an empty word is not a word
        }
        return scored(q, h->tok[label]);
    };
    std::vector<double> le(V);
    std::vector<char> inC(V);
    std::vector<int> order;
    auto frame = [&](int t) {
        const float* e = emis + (long)t * fs;
        for (int v = 0; v < V; v++) le[v] = is_log ? (double)e[v] : std::log((double)e[v]);
        std::fill(inC.begin(), inC.end(), 1);
        if (h->top_n && h->nc < V - 1) {
            order.clear();
            for (int v = 0; v < V; v++)
                if (v != blank) order.push_back(v);
            std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return e[x] > e[y]; });
            std::fill(inC.begin(), inC.end(), 0);
            for (int i = 0; i < h->nc; i++) inC[order[i]] = 1;
        }
        inC[blank] = 1;
    };
    // keep every state with fused >= the (beam+1)-th largest; false: more than kcap survive
    auto prune = [&]() {
        std::vector<double> f;
        for (const ClmStr& s : path) f.push_back(score.at(s) + info.at(prefix_of(s)).W);
        if ((int)f.size() > h->beam) {
            std::vector<double> g = f;
            std::sort(g.begin(), g.end(), std::greater<double>());
            const double cutoff = g[h->beam];
            for (double x : g) note_gap(x, cutoff);
            size_t i = 0;
            for (auto it = path.begin(); it != path.end(); i++) {
                if (f[i] < cutoff) {
                    score.erase(*it);
                    it = path.erase(it);
                } else {
                    ++it;
                }
            }
        }
        std::map<ClmStr, ClmPrefix> kept;
        for (const ClmStr& s : path) {
            const ClmStr p = prefix_of(s);
            kept[p] = info.at(p);
        }
        info.swap(kept);
        return (int)path.size() <= h->kcap;
    };
    // frame 0: one state per symbol of C_0 and the blank
    frame(0);
    info[ClmStr()] = ClmPrefix();
    {
        const ClmPrefix root;
        for (int i = 0; i < V; i++) {
            if (!inC[i] || (i != blank && !allowed(root, i))) continue;
            const ClmStr s(1, h->codes[i]);
            path.insert(s);
            score[s] = le[i];
            if (i != blank) info[s] = child(root, i);
        }
    }
    if (!prune()) return false;
    for (int t = 1; t < len; t++) {
        frame(t);
        upath.clear();
        uscore.clear();
        uinfo.clear();
        for (const ClmStr& s : path) {
            const double sc = score.at(s);
            const ClmStr ps = prefix_of(s);
            for (int i = 0; i < V; i++) {
                if (!inC[i]) continue;
                ClmStr ns;
                if (i == blank) {
                    ns = s;
                    if (s.back() != bcode) ns.push_back(bcode);
                } else if (s.back() == h->codes[i]) {
                    ns = s;   // the repeat "qc" + c -> "qc": always exists
                } else {
                    if (!allowed(info.at(ps), i)) continue;   // closed mode: no such extension
                    ns = s;
                    if (s.back() == bcode) ns.back() = h->codes[i];
                    else ns.push_back(h->codes[i]);
                }
                const double x = sc + le[i];
                auto f = uscore.find(ns);
                if (f != uscore.end()) {
                    f->second = clm_lse_host(f->second, x);
                } else {
                    upath.insert(ns);
                    uscore[ns] = x;
                }
                const ClmStr np = prefix_of(ns);
                if (!uinfo.count(np)) {
                    auto g = info.find(np);
                    if (g != info.end()) uinfo[np] = g->second;      // a live prefix keeps its terms
                    else uinfo[np] = child(info.at(ps), i);          // np = ps + label i
                }
            }
        }
        path.swap(upath);
        score.swap(uscore);
        info.swap(uinfo);
        if (!prune()) return false;
    }
    // final merge of "q" with "q$", in set order
    std::map<ClmStr, double> fin;
    for (const ClmStr& s : path) {
        const ClmStr p = prefix_of(s);
        auto f = fin.find(p);
        if (f != fin.end()) f->second = clm_lse_host(f->second, score.at(s));
        else fin[p] = score.at(s);
    }
    out.clear();
    for (const auto& kv : fin) {
        const ClmPrefix& q0 = info.at(kv.first);
        const ClmPrefix q = word && q0.z != 0 ? word_end(q0) : q0;   // the pending word
        ClmHyp hy;
        hy.str = kv.first;
        for (int32_t c : kv.first) hy.labels.push_back(label_of[c]);
        hy.ctc = kv.second;
        hy.total = kv.second + q.W;
        hy.lm = q.L;
        hy.n = q.n;
        if (h->flags & ASR_LM_EOS) {
            const double v = lm_value_after(lm, q.ctx, std::min(q.n, LM_CTX), 0, true, h->flags);
            hy.total = hy.total + (h->aln10 * v);
            hy.lm = hy.lm + v;
        }
        out.push_back(std::move(hy));
    }
    clm_rank(out);
    for (size_t k = 1; k < out.size(); k++) note_gap(out[k - 1].total, out[k].total);
    return true;
}

// Bring the results of a queued device decode to the host and rank them.
static int clm_fetch(asr_ctc_lm* h) {
    const int B = h->lastB, T = h->lastT, kc = h->kcap;
    ASR_HIP_TRY(hipStreamSynchronize(h->stream));
    const size_t need = (size_t)B * kc * (size_t)T;
    if (need > h->lab_elems) {
        if (h->d_lab) (void)hipFree(h->d_lab);
        h->d_lab = nullptr;
        h->lab_elems = 0;
        ASR_HIP_TRY(hipMalloc(&h->d_lab, need * sizeof(uint16_t)));
        h->lab_elems = need;
    }
    const long n = (long)B * kc;
    ctc_lm_trace_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream>>>(
        h->d_nodes, (long)T * kc, h->d_fin_n, h->d_fin_node, h->d_fin_len, kc, T, B, h->d_lab);
    ASR_LAUNCH_TRY();
    std::vector<int32_t> fin_n(B), status(B), fin_len((size_t)n), fin_nw(h->lex ? (size_t)n : 0);
    if (h->lex) ASR_HIP_TRY(hipMemcpyAsync(fin_nw.data(), h->d_fin_nw, 4 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    std::vector<double> total((size_t)n), ctc((size_t)n), lmv((size_t)n);
    std::vector<uint16_t> lab(need);
    ASR_HIP_TRY(hipMemcpyAsync(fin_n.data(), h->d_fin_n, 4 * (size_t)B, hipMemcpyDeviceToHost, h->stream));
    ASR_HIP_TRY(hipMemcpyAsync(status.data(), h->d_status, 4 * (size_t)B, hipMemcpyDeviceToHost, h->stream));
    ASR_HIP_TRY(hipMemcpyAsync(fin_len.data(), h->d_fin_len, 4 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    ASR_HIP_TRY(hipMemcpyAsync(total.data(), h->d_fin_total, 8 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    ASR_HIP_TRY(hipMemcpyAsync(ctc.data(), h->d_fin_ctc, 8 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    ASR_HIP_TRY(hipMemcpyAsync(lmv.data(), h->d_fin_lm, 8 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    ASR_HIP_TRY(hipMemcpyAsync(lab.data(), h->d_lab, need * sizeof(uint16_t), hipMemcpyDeviceToHost, h->stream));
    ASR_HIP_TRY(hipStreamSynchronize(h->stream));
    h->hyps.assign(B, {});
    h->overflow.assign(B, 0);
    h->gaps.clear();
    for (int b = 0; b < B; b++) {
        if (status[b]) {
            h->overflow[b] = 1;
            continue;
        }
        const int nh = std::min(std::max(fin_n[b], 0), kc);
        std::vector<ClmHyp>& v = h->hyps[b];
        v.resize(nh);
        for (int k = 0; k < nh; k++) {
            const size_t i = (size_t)b * kc + k;
            const int len = std::min(std::max(fin_len[i], 0), T);
            ClmHyp& hy = v[k];
            hy.labels.resize(len);
            hy.str.resize(len);
            for (int j = 0; j < len; j++) {
                const int l = std::min((int)lab[i * T + j], h->V - 1);
                hy.labels[j] = l;
                hy.str[j] = h->codes[l];
            }
            hy.total = total[i];
            hy.ctc = ctc[i];
            hy.lm = lmv[i];
            hy.n = h->lex ? fin_nw[i] : fin_len[i];
        }
        clm_rank(v);
    }
    h->state = 2;
    return ASR_OK;
}

// Both creates: tok_of_label (token mode) or lex and lex_mode (word mode).
static int clm_create(const int32_t* codes, int V, int beam_width, int blank_id, int max_states, const asr_lm_t* lm,
                      const int32_t* tok_of_label, const asr_lexicon* lex, int lex_mode, bool word, float alpha,
                      float beta, int lm_flags, int top_n, asr_ctc_lm_t** out) {
    if (!out) return ASR_ERR_ARG;
    *out = nullptr;
    if (!lm || (word ? !lex : !tok_of_label)) return ASR_ERR_ARG;
    if (V < 2 || beam_width < 1 || blank_id < 0 || blank_id >= V) return ASR_ERR_ARG;
    if (!std::isfinite(alpha) || alpha < 0.0f || !std::isfinite(beta)) return ASR_ERR_ARG;
    if ((lm_flags & ~(ASR_LM_BOS | ASR_LM_EOS)) || top_n < 0 || max_states < 0) return ASR_ERR_ARG;
    const asr::LmTables *host, *dev;
    (void)asr_internal_lm_tables(lm, &host, &dev);
    if (((lm_flags & ASR_LM_BOS) && host->bos < 0) || ((lm_flags & ASR_LM_EOS) && host->eos < 0)) return ASR_ERR_ARG;
    if (word) {
        if (lex->V != V || lex->used[blank_id] || lex->space == blank_id) return ASR_ERR_ARG;
        if (lex_mode != ASR_LEX_OPEN && lex_mode != ASR_LEX_CLOSED) return ASR_ERR_ARG;
    }
    if (V > asr::CLM_VMAX) return ASR_ERR_UNSUPPORTED;
    if (codes)
        for (int v = 0; v < V; v++)
            for (int u = 0; u < v; u++)
                if (codes[u] == codes[v]) return ASR_ERR_ARG;
    const int K = beam_width > 1 << 20 ? 1 << 20 : beam_width + 1;
    if (max_states > 0 && max_states < K) return ASR_ERR_ARG;
    const int nc = (top_n && top_n < V - 1) ? top_n : V - 1;
    if (nc > asr::CLM_MAXC) return ASR_ERR_UNSUPPORTED;
    int kcap = max_states > 0 ? max_states : K + std::max(8, K / 8);
    kcap = (kcap + 31) & ~31;
    if (kcap > 256) return ASR_ERR_UNSUPPORTED;
    asr_ctc_lm* h = nullptr;
    try {
        h = new asr_ctc_lm();
        h->codes.resize(V);
        if (word) h->tok.assign(V, -1);   // unused: words carry the tokens
        else h->tok.assign(tok_of_label, tok_of_label + V);
        for (int v = 0; v < V; v++) h->codes[v] = codes ? codes[v] : v;
    } catch (const std::bad_alloc&) {
        delete h;
        return ASR_ERR_OOM;
    }
    h->V = V;
    h->beam = beam_width;
    h->blank = blank_id;
    h->kcap = kcap;
    h->nc = nc;
    h->top_n = nc < V - 1 ? top_n : 0;
    h->flags = lm_flags;
    h->aln10 = (double)alpha * 2.302585092994046;
    h->beta = (double)beta;
    h->lm = lm;
    h->lex = word ? lex : nullptr;
    h->closed = word && lex_mode == ASR_LEX_CLOSED ? 1 : 0;
    *out = h;
    return ASR_OK;
}

}  // namespace asr

extern "C" {

int asr_ctc_lm_create(const int32_t* codes, int V, int beam_width, int blank_id, int max_states, const asr_lm_t* lm,
                      const int32_t* tok_of_label, float alpha, float beta, int lm_flags, int top_n,
                      asr_ctc_lm_t** out) {
    return asr::clm_create(codes, V, beam_width, blank_id, max_states, lm, tok_of_label, nullptr, 0, false, alpha, beta,
                           lm_flags, top_n, out);
}

int asr_ctc_lm_create_word(const int32_t* codes, int V, int beam_width, int blank_id, int max_states,
                           const asr_lm_t* lm, const asr_lexicon_t* lex, float alpha, float beta, int lm_flags,
                           int top_n, int lex_mode, asr_ctc_lm_t** out) {
    return asr::clm_create(codes, V, beam_width, blank_id, max_states, lm, nullptr, lex, lex_mode, true, alpha, beta,
                           lm_flags, top_n, out);
}

int asr_lexicon_create(const int32_t* spell, const int64_t* offsets, const int32_t* tok, int n_words, int V,
                       int space_label, asr_lexicon_t** out) {
    if (!out) return ASR_ERR_ARG;
    *out = nullptr;
    if (!spell || !offsets || !tok) return ASR_ERR_ARG;
    if (V < 2 || n_words < 1 || space_label < 0 || space_label >= V) return ASR_ERR_ARG;
    if (offsets[0] != 0) return ASR_ERR_ARG;
    for (int w = 0; w < n_words; w++)
        if (offsets[w + 1] < offsets[w]) return ASR_ERR_ARG;
    for (int64_t i = 0; i < offsets[n_words]; i++)
        if (spell[i] < 0 || spell[i] >= V || spell[i] == space_label) return ASR_ERR_ARG;
    for (int w = 0; w < n_words; w++)
        if (offsets[w + 1] == offsets[w]) return ASR_ERR_ARG;
    for (int w = 0; w < n_words; w++)
        if (tok[w] < 0) return ASR_ERR_ARG;
    asr_lexicon* h = nullptr;
    try {
        // the trie in insertion order, then renumbered breadth-first
        std::vector<std::map<int32_t, int64_t>> kids(1);
        std::vector<int32_t> wtok(1, -1);
        int words = 0;
        for (int w = 0; w < n_words; w++) {
            int64_t z = 0;
            for (int64_t i = offsets[w]; i < offsets[w + 1]; i++) {
                auto f = kids[(size_t)z].find(spell[i]);
                if (f != kids[(size_t)z].end()) {
                    z = f->second;
                } else {
                    if (kids.size() >= ((size_t)1 << 31) - 1) return ASR_ERR_UNSUPPORTED;   // 2^31 or more nodes
                    const int64_t nz = (int64_t)kids.size();
                    kids[(size_t)z][spell[i]] = nz;
                    kids.emplace_back();
                    wtok.push_back(-1);
                    z = nz;
                }
            }
            if (wtok[(size_t)z] >= 0) {
                if (wtok[(size_t)z] != tok[w]) return ASR_ERR_ARG;   // one spelling, two tokens
            } else {
                wtok[(size_t)z] = tok[w];
                words++;
            }
        }
        h = new asr_lexicon();
        const size_t N = kids.size();
        h->first.resize(N + 1);
        h->label.resize(N);
        h->tok.resize(N);
        h->used.assign((size_t)V, 0);
        std::vector<int64_t> order(1, 0);   // order[new id] = old id
        order.reserve(N);
        h->label[0] = -1;
        for (size_t i = 0; i < N; i++) {
            const int64_t old = order[i];
            h->first[i] = (uint32_t)order.size();
            h->tok[i] = wtok[(size_t)old];
            h->max_children = std::max(h->max_children, (int)kids[(size_t)old].size());
            for (const auto& kv : kids[(size_t)old]) {   // ascending labels
                h->label[order.size()] = kv.first;
                h->used[(size_t)kv.first] = 1;
                order.push_back(kv.second);
            }
        }
        h->first[N] = (uint32_t)N;
        h->V = V;
        h->space = space_label;
        h->words = words;
    } catch (const std::bad_alloc&) {
        delete h;
        return ASR_ERR_OOM;
    }
    *out = h;
    return ASR_OK;
}

int asr_lexicon_upload(asr_lexicon_t* h) {
    if (!h) return ASR_ERR_ARG;
    if (h->d_blob) return ASR_OK;
    const size_t N = h->label.size();
    const size_t b_first = ((N + 1) * 4 + 15) & ~(size_t)15, b_node = (N * 4 + 15) & ~(size_t)15;
    void* d = nullptr;
    ASR_HIP_TRY(hipMalloc(&d, b_first + 2 * b_node));
    hipError_t e = hipMemcpy(d, h->first.data(), (N + 1) * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy((char*)d + b_first, h->label.data(), N * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy((char*)d + b_first + b_node, h->tok.data(), N * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        asr_internal_set_error("hipMemcpy (lexicon tables)", hipGetErrorString(e), __FILE__, __LINE__);
        (void)hipFree(d);
        return ASR_ERR_HIP;
    }
    h->d_first = (const uint32_t*)d;
    h->d_label = (const int32_t*)((char*)d + b_first);
    h->d_tok = (const int32_t*)((char*)d + b_first + b_node);
    h->d_blob = d;
    return ASR_OK;
}

int asr_lexicon_get_info(const asr_lexicon_t* h, asr_lexicon_info* info) {
    if (!h || !info) return ASR_ERR_ARG;
    info->words = h->words;
    info->nodes = (int32_t)h->label.size();
    info->max_children = h->max_children;
    info->space_label = h->space;
    info->table_bytes = (int64_t)(h->first.size() + h->label.size() + h->tok.size()) * 4;
    return ASR_OK;
}

int asr_lexicon_destroy(asr_lexicon_t* h) {
    if (!h) return ASR_ERR_ARG;
    if (h->d_blob) (void)hipFree(h->d_blob);
    delete h;
    return ASR_OK;
}

int asr_ctc_lm_destroy(asr_ctc_lm_t* h) {
    if (!h) return ASR_ERR_ARG;
    if (h->d_nodes || h->d_codes || h->d_lab) {
        (void)hipDeviceSynchronize();
        asr::clm_free_work(h);
        if (h->d_codes) (void)hipFree(h->d_codes);
        if (h->d_tok) (void)hipFree(h->d_tok);
        if (h->d_lab) (void)hipFree(h->d_lab);
        if (h->ev_len) (void)hipEventDestroy(h->ev_len);
    }
    delete h;
    return ASR_OK;
}

int asr_ctc_lm_decode(asr_ctc_lm_t* h, const float* d_emis, int T, int B, long frame_stride, long utt_stride,
                      const int32_t* h_lengths, int is_log, asr_stream_t s) {
    const int rc = asr::clm_check_decode(h, d_emis, T, B, frame_stride, utt_stride, h_lengths);
    if (rc != ASR_OK) return rc;
    const asr::LmTables *host, *dev;
    if (!asr_internal_lm_tables(h->lm, &host, &dev)) return ASR_ERR_STATE;
    if (h->lex && !h->lex->d_blob) return ASR_ERR_STATE;
    hipStream_t st = asr_stream(s);
    // one decode at a time per handle: a queued one on another stream ends before its workspace is reused
    if (h->state == 1 && h->stream != st) ASR_HIP_TRY(hipStreamSynchronize(h->stream));
    h->state = 0;
    const int rr = asr::clm_reserve(h, T, B);
    if (rr != ASR_OK) return rr;
    // the lengths go through a pinned buffer of the handle: wait for the previous decode's copy, not for its kernel
    if (h->len_queued) ASR_HIP_TRY(hipEventSynchronize(h->ev_len));
    for (int b = 0; b < B; b++) h->p_lengths[b] = h_lengths ? h_lengths[b] : T;
    ASR_HIP_TRY(hipMemcpyAsync(h->d_lengths, h->p_lengths, 4 * (size_t)B, hipMemcpyHostToDevice, st));
    ASR_HIP_TRY(hipEventRecord(h->ev_len, st));
    h->len_queued = true;
    if (h->top_n) {
        asr::ctc_lm_topn_kernel<<<dim3((unsigned)((long)B * T)), dim3(64), 0, st>>>(
            d_emis, frame_stride, utt_stride, h->d_lengths, T, h->V, h->blank, h->nc, h->d_cand);
        ASR_LAUNCH_TRY();
    }
    asr::ClmArgs a;
    a.lm = *dev;
    a.emis = d_emis;
    a.tstride = frame_stride;
    a.ustride = utt_stride;
    a.lengths = h->d_lengths;
    a.T = T;
    a.B = B;
    a.is_log = is_log ? 1 : 0;
    a.V = h->V;
    a.blank = h->blank;
    a.beam = h->beam;
    a.kcap = h->kcap;
    a.nc = h->nc;
    a.flags = h->flags;
    a.aln10 = h->aln10;
    a.beta = h->beta;
    a.codes = h->d_codes;
    a.tok = h->d_tok;
    a.cand = h->top_n ? h->d_cand : nullptr;
    a.nodes = h->d_nodes;
    a.ckey = h->d_ckey;
    a.cscore = h->d_cscore;
    a.cv = h->d_cv;
    a.fin_n = h->d_fin_n;
    a.status = h->d_status;
    a.fin_node = h->d_fin_node;
    a.fin_len = h->d_fin_len;
    a.fin_total = h->d_fin_total;
    a.fin_ctc = h->d_fin_ctc;
    a.fin_lm = h->d_fin_lm;
    if (h->lex) {
        asr::ClmWordArgs wa;
        wa.lex = h->lex->tables(true, h->closed);
        wa.fin_nw = h->d_fin_nw;
        asr::ctc_wordlm_kernel<<<dim3((unsigned)B), dim3(asr::CLM_NT), asr::clm_lds_bytes(h->kcap, true), st>>>(a, wa);
    } else {
        asr::ctc_lm_kernel<<<dim3((unsigned)B), dim3(asr::CLM_NT), asr::clm_lds_bytes(h->kcap), st>>>(a);
    }
    ASR_LAUNCH_TRY();
    h->stream = st;
    h->lastT = T;
    h->lastB = B;
    h->state = 1;
    return ASR_OK;
}

int asr_ctc_lm_decode_host(asr_ctc_lm_t* h, const float* h_emis, int T, int B, long frame_stride, long utt_stride,
                           const int32_t* h_lengths, int is_log) {
    const int rc = asr::clm_check_decode(h, h_emis, T, B, frame_stride, utt_stride, h_lengths);
    if (rc != ASR_OK) return rc;
    const asr::LmTables *host, *dev;
    (void)asr_internal_lm_tables(h->lm, &host, &dev);
    h->state = 0;
    try {
        h->hyps.assign(B, {});
        h->overflow.assign(B, 0);
        h->gaps.assign(B, INFINITY);
        for (int b = 0; b < B; b++) {
            const int len = h_lengths ? h_lengths[b] : T;
            if (!asr::clm_decode_one(h, *host, h_emis + (long)b * utt_stride, frame_stride, len, is_log ? 1 : 0,
                                     h->hyps[b], h->gaps[b])) {
                h->overflow[b] = 1;
                h->hyps[b].clear();
            }
        }
    } catch (const std::bad_alloc&) {
        return ASR_ERR_OOM;
    }
    h->lastT = T;
    h->lastB = B;
    h->state = 2;
    return ASR_OK;
}

int asr_ctc_lm_get_beams(asr_ctc_lm_t* h, int max_hyps, int max_len, int32_t* h_n_hyps, int32_t* h_lengths,
                         int32_t* h_labels, double* h_total, double* h_ctc_logp, double* h_lm_log10,
                         int32_t* h_n_tokens) {
    if (!h || max_hyps < 1 || max_len < 1 || !h_n_hyps || !h_lengths || !h_labels) return ASR_ERR_ARG;
    if (h->state == 0) return ASR_ERR_STATE;
    if (h->state == 1) {
        const int rc = asr::clm_fetch(h);
        if (rc != ASR_OK) return rc;
    }
    int rc = ASR_OK;
    for (int b = 0; b < h->lastB; b++) {
        if (h->overflow[b]) rc = ASR_ERR_BEAM_OVERFLOW;
        const std::vector<asr::ClmHyp>& v = h->hyps[b];
        h_n_hyps[b] = (int32_t)v.size();
        const int n = (int)std::min<size_t>(v.size(), (size_t)max_hyps);
        for (int k = 0; k < n; k++) {
            const size_t i = (size_t)b * max_hyps + k;
            h_lengths[i] = (int32_t)v[k].labels.size();
            for (int j = 0; j < (int)v[k].labels.size() && j < max_len; j++) h_labels[i * max_len + j] = v[k].labels[j];
            if (h_total) h_total[i] = v[k].total;
            if (h_ctc_logp) h_ctc_logp[i] = v[k].ctc;
            if (h_lm_log10) h_lm_log10[i] = v[k].lm;
            if (h_n_tokens) h_n_tokens[i] = v[k].n;
        }
    }
    return rc;
}

int asr_ctc_lm_host_gaps(asr_ctc_lm_t* h, double* h_gap) {
    if (!h || !h_gap) return ASR_ERR_ARG;
    if (h->state != 2 || h->gaps.size() != (size_t)h->lastB) return ASR_ERR_STATE;
    for (int b = 0; b < h->lastB; b++) h_gap[b] = h->gaps[b];
    return ASR_OK;
}

int asr_ctc_lm_get_best(asr_ctc_lm_t* h, int32_t* h_labels, int max_len, int32_t* h_lengths, double* h_total) {
    if (!h || max_len < 1 || !h_lengths || !h_labels) return ASR_ERR_ARG;
    if (h->state == 0) return ASR_ERR_STATE;
    std::vector<int32_t> nh((size_t)std::max(h->lastB, 1));
    return asr_ctc_lm_get_beams(h, 1, max_len, nh.data(), h_lengths, h_labels, h_total, nullptr, nullptr, nullptr);
}

}  // extern "C"
