// ============================================================================
// Back-off n-gram language model on gfx950: ARPA loader, an exact reverse trie
// and a scoring kernel, one wave per hypothesis, one launch per call
// (the contract is in include/asr_amd.h).
//
// Table.  The n-gram (w1..wk) sits on the path wk, wk-1, .., w1.  Level 1 is
// indexed by the word id; level k >= 2 holds, per parent, the sorted ids of its
// children (words[k]) and a node (P, back-off, first child) beside each; node
// i's children at level k+1 are [node[i].child, node[i+1].child) (one sentinel
// node ends every level).  A token at position i takes two walks:
//   match:    w_i, w_i-1, ..  the deepest node that carries a probability is
//             the longest n-gram present (its P, its order q);
//   back-off: w_i-1, w_i-2, ..  the back-off of every nested context on the way
//             down, needed only when q <= context length.
// Every step of a walk is a binary search in one parent's child range: a chain
// of dependent reads, hidden by waves per SIMD, not by arithmetic.  A node
// inserted for a missing suffix has P = +inf (a valid P is <= 0) and back-off 0.
//
// lm_position() is the whole per-token computation, __host__ __device__: the
// kernel and asr_lm_score_host run the same code over the same tables, so the
// device and the CPU path agree bit for bit.
// ============================================================================
#include "lm_tables.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

namespace asr {

constexpr int LM_MAX_LEN = 65536;

struct LmScoreArgs {
    const int32_t* tokens;
    long ldt;
    const int32_t* lengths;
    double* logp;
    int32_t* counts;
    double* tok_logp;
    int32_t* tok_order;
    long ldd;
    int N, max_len, flags;
};

constexpr int LM_WAVES = 4;   // hypotheses per workgroup (no LDS, no barrier: waves are independent)

__global__ __launch_bounds__(64 * LM_WAVES) void lm_score_kernel(const LmTables t, const LmScoreArgs a) {
    const int lane = threadIdx.x & 63;
    const long n = (long)blockIdx.x * LM_WAVES + (threadIdx.x >> 6);
    if (n >= a.N) return;   // wave-uniform
    const int32_t* tok = a.tokens + n * a.ldt;
    int L = a.max_len;
    if (a.lengths) L = min(max(a.lengths[n], 0), a.max_len);
    const int total = L + ((a.flags & ASR_LM_EOS) ? 1 : 0);
    double acc = 0.0;
    int n_oov = 0;
    for (int i = lane; i < total; i += 64) {
        const LmTok r = lm_position(t, tok, L, i, a.flags);
        acc += r.v;
        n_oov += r.oov;
        if (a.tok_logp) a.tok_logp[n * a.ldd + i] = r.v;
        if (a.tok_order) a.tok_order[n * a.ldd + i] = r.order;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        acc += __shfl_down(acc, off);
        n_oov += __shfl_down(n_oov, off);
    }
    if (lane == 0) {
        if (a.logp) a.logp[n] = acc;
        if (a.counts) {
            a.counts[2 * n] = total;
            a.counts[2 * n + 1] = n_oov;
        }
    }
}

// ------------------------------------------------------------------ the loader
struct LmEntry {
    int32_t key[ASR_LM_MAX_ORDER];   // reversed: key[0] = last word
    float p, bo;
};

struct LmKeyLess {
    int k;
    bool operator()(const LmEntry& a, const LmEntry& b) const {
        for (int i = 0; i < k; i++)
            if (a.key[i] != b.key[i]) return a.key[i] < b.key[i];
        return (a.p <= 0.0f) && !(b.p <= 0.0f);   // a real n-gram before an inserted node
    }
};

static bool lm_same_key(const LmEntry& a, const LmEntry& b, int k) {
    for (int i = 0; i < k; i++)
        if (a.key[i] != b.key[i]) return false;
    return true;
}

// One decimal fp32: the whole field, digits / sign / point / exponent only, finite.
static bool lm_parse_float(const char* b, const char* e, float* out) {
    if (b == e) return false;
    for (const char* c = b; c < e; c++)
        if (!((*c >= '0' && *c <= '9') || *c == '+' || *c == '-' || *c == '.' || *c == 'e' || *c == 'E'))
            return false;
    const std::string s(b, e);
    char* end = nullptr;
    const float v = std::strtof(s.c_str(), &end);
    if (end != s.c_str() + s.size() || !std::isfinite(v)) return false;
    *out = v;
    return true;
}

}  // namespace asr

struct asr_lm {
    int order = 0, vocab = 0, bos = -1, eos = -1, unk = -1;
    float oov = 0.0f;
    int64_t ngrams[ASR_LM_MAX_ORDER] = {};
    int64_t inserted = 0;
    std::vector<std::string> strings;
    std::unordered_map<std::string, int32_t> ids;
    std::vector<int32_t> words[ASR_LM_MAX_ORDER + 1];
    std::vector<asr::LmNode> nodes[ASR_LM_MAX_ORDER + 1];
    asr::LmTables host{};
    asr::LmTables dev{};
    void* d_blob = nullptr;

    int64_t table_bytes() const {
        int64_t b = 0;
        for (int k = 1; k <= order; k++)
            b += (int64_t)words[k].size() * 4 + (int64_t)nodes[k].size() * (int64_t)sizeof(asr::LmNode);
        return b;
    }
};

namespace asr {

static int lm_parse(asr_lm* h, const char* text, size_t bytes) {
    const char* p = text;
    const char* const end = text + bytes;
    std::vector<LmEntry> level[ASR_LM_MAX_ORDER + 1];
    int64_t declared[ASR_LM_MAX_ORDER + 1] = {};
    bool has_decl[ASR_LM_MAX_ORDER + 1] = {};
    int state = 0;       // 0: before \data\, 1: counts, 2: in a section
    int cur = 0;         // the section's order
    bool ended = false;
    std::vector<std::pair<const char*, const char*>> f;
    while (p < end && !ended) {
        const char* le = (const char*)memchr(p, '\n', (size_t)(end - p));
        if (!le) le = end;
        const char* b = p;
        const char* e = le;
        p = le < end ? le + 1 : end;
        while (b < e && (*b == ' ' || *b == '\t' || *b == '\r')) b++;
        while (e > b && (e[-1] == ' ' || e[-1] == '\t' || e[-1] == '\r')) e--;
        if (b == e) continue;
        const size_t len = (size_t)(e - b);
        if (state == 0) {
            if (len == 6 && !memcmp(b, "\\data\\", 6)) state = 1;
            continue;   // header text before \data\ is ignored
        }
        if (*b == '\\') {
            if (len == 5 && !memcmp(b, "\\end\\", 5)) {
                ended = true;
                continue;
            }
            // \k-grams:
            const char* c = b + 1;
            int k = 0;
            int digits = 0;
            while (c < e && *c >= '0' && *c <= '9' && digits < 6) {
                k = k * 10 + (*c - '0');
                c++;
                digits++;
            }
            if (!digits || (size_t)(e - c) != 7 || memcmp(c, "-grams:", 7)) return ASR_ERR_ARG;
            if (k > ASR_LM_MAX_ORDER) return ASR_ERR_UNSUPPORTED;
            if (k != cur + 1 || !has_decl[k]) return ASR_ERR_ARG;   // sections in order, each declared
            cur = k;
            state = 2;
            continue;
        }
        if (state == 1) {
            // ngram k=count
            if (len < 6 || memcmp(b, "ngram", 5) || (b[5] != ' ' && b[5] != '\t')) return ASR_ERR_ARG;
            const char* c = b + 5;
            while (c < e && (*c == ' ' || *c == '\t')) c++;
            int k = 0, digits = 0;
            while (c < e && *c >= '0' && *c <= '9' && digits < 6) {
                k = k * 10 + (*c - '0');
                c++;
                digits++;
            }
            if (!digits || c == e || *c != '=') return ASR_ERR_ARG;
            c++;
            uint64_t n = 0;
            digits = 0;
            while (c < e && *c >= '0' && *c <= '9' && digits < 18) {
                n = n * 10 + (uint64_t)(*c - '0');
                c++;
                digits++;
            }
            if (!digits || c != e) return ASR_ERR_ARG;
            if (k < 1) return ASR_ERR_ARG;
            if (k > ASR_LM_MAX_ORDER || n >= (1ull << 31)) return ASR_ERR_UNSUPPORTED;
            if (has_decl[k]) return ASR_ERR_ARG;
            has_decl[k] = true;
            declared[k] = (int64_t)n;
            continue;
        }
        // an n-gram line of order cur: P, cur tokens, optional back-off
        f.clear();
        for (const char* c = b; c < e;) {
            while (c < e && (*c == ' ' || *c == '\t')) c++;
            const char* s = c;
            while (c < e && *c != ' ' && *c != '\t') c++;
            if (c > s) f.emplace_back(s, c);
        }
        if ((int)f.size() != cur + 1 && (int)f.size() != cur + 2) return ASR_ERR_ARG;
        LmEntry en{};
        en.bo = 0.0f;
        if (!lm_parse_float(f[0].first, f[0].second, &en.p) || en.p > 0.0f) return ASR_ERR_ARG;
        if ((int)f.size() == cur + 2 && !lm_parse_float(f[cur + 1].first, f[cur + 1].second, &en.bo))
            return ASR_ERR_ARG;
        if ((int64_t)level[cur].size() >= declared[cur]) return ASR_ERR_ARG;   // more lines than declared
        if (cur == 1) {
            std::string s(f[1].first, f[1].second);
            const int32_t id = (int32_t)h->strings.size();
            if (!h->ids.emplace(s, id).second) return ASR_ERR_ARG;   // duplicate unigram
            h->strings.push_back(std::move(s));
            en.key[0] = id;
        } else {
            for (int j = 0; j < cur; j++) {
                const auto it = h->ids.find(std::string(f[1 + j].first, f[1 + j].second));
                if (it == h->ids.end()) return ASR_ERR_ARG;   // no unigram for this token
                en.key[cur - 1 - j] = it->second;
            }
        }
        level[cur].push_back(en);
    }
    if (state == 0 || !ended) return ASR_ERR_ARG;
    int order = 0;
    while (order < ASR_LM_MAX_ORDER && has_decl[order + 1]) order++;
    for (int k = order + 1; k <= ASR_LM_MAX_ORDER; k++)
        if (has_decl[k]) return ASR_ERR_ARG;   // a gap in the orders
    if (order == 0) return ASR_ERR_ARG;
    for (int k = 1; k <= order; k++)
        if ((int64_t)level[k].size() != declared[k]) return ASR_ERR_ARG;
    if (level[1].empty()) return ASR_ERR_ARG;
    while (order > 1 && level[order].empty()) order--;   // "ngram 3=0": an empty top order adds nothing

    h->order = order;
    h->vocab = (int)level[1].size();
    for (int k = 1; k <= order; k++) h->ngrams[k - 1] = (int64_t)level[k].size();
    auto special = [&](const char* s) {
        const auto it = h->ids.find(s);
        return it == h->ids.end() ? -1 : it->second;
    };
    h->bos = special("<s>");
    h->eos = special("</s>");
    h->unk = special("<unk>");

    // Levels from the top down: sort, refuse duplicates, and hand every distinct
    // parent key to the level below, where it is dropped if the n-gram exists and
    // stays as an inserted node (no probability) if not.
    for (int k = order; k >= 2; k--) {
        std::vector<LmEntry>& lv = level[k];
        std::sort(lv.begin(), lv.end(), LmKeyLess{k});
        size_t o = 0;
        for (size_t i = 0; i < lv.size(); i++) {
            if (o && lm_same_key(lv[o - 1], lv[i], k)) {
                if (lv[i].p <= 0.0f) return ASR_ERR_ARG;   // a duplicate n-gram
                continue;                                   // the n-gram exists: no node to insert
            }
            if (!(lv[i].p <= 0.0f)) h->inserted++;
            lv[o++] = lv[i];
        }
        lv.resize(o);
        if (lv.size() >= (1ull << 31)) return ASR_ERR_UNSUPPORTED;
        if (k > 2) {
            for (size_t i = 0; i < lv.size(); i++) {
                if (i && lm_same_key(lv[i - 1], lv[i], k - 1)) continue;
                LmEntry par = lv[i];
                par.key[k - 1] = 0;
                par.p = INFINITY;
                par.bo = 0.0f;
                level[k - 1].push_back(par);
            }
        }
    }
    // Emit.  Level 1 is in id order already.
    for (int k = 1; k <= order; k++) {
        const std::vector<LmEntry>& lv = level[k];
        std::vector<LmNode>& nd = h->nodes[k];
        nd.resize(lv.size() + 1);
        if (k >= 2) h->words[k].resize(lv.size());
        for (size_t i = 0; i < lv.size(); i++) {
            nd[i].p = lv[i].p;
            nd[i].bo = lv[i].bo;
            nd[i].child = 0;
            if (k >= 2) h->words[k][i] = lv[i].key[k - 1];
        }
        nd[lv.size()] = LmNode{INFINITY, 0.0f, 0};
    }
    for (int k = 1; k < order; k++) {
        // node i's children: the run of level k+1 whose first k key words are node i's
        const std::vector<LmEntry>& par = level[k];
        const std::vector<LmEntry>& ch = level[k + 1];
        size_t c = 0;
        for (size_t i = 0; i < par.size(); i++) {
            h->nodes[k][i].child = (uint32_t)c;
            while (c < ch.size() && lm_same_key(par[i], ch[c], k)) c++;
        }
        h->nodes[k][par.size()].child = (uint32_t)c;
        if (c != ch.size()) return ASR_ERR_INTERNAL;   // a child without its parent: cannot happen
    }
    for (int k = 1; k <= order; k++) {
        h->host.words[k] = h->words[k].data();
        h->host.nodes[k] = h->nodes[k].data();
    }
    h->host.order = order;
    h->host.vocab = h->vocab;
    h->host.bos = h->bos;
    h->host.eos = h->eos;
    h->host.unk = h->unk;
    h->host.oov = h->oov;
    return ASR_OK;
}

// The checks asr_lm_score and asr_lm_score_host share, in the documented order.
static int lm_check(const asr_lm* h, const int32_t* tokens, long ldt, int N, int max_len, int flags,
                    const double* logp, const int32_t* counts, const double* tok_logp, const int32_t* tok_order,
                    long ldd) {
    if (!h || !tokens || N <= 0) return ASR_ERR_ARG;
    if (ldt < (long)max_len) return ASR_ERR_ARG;
    if ((tok_logp || tok_order) && ldd < (long)max_len + 1) return ASR_ERR_ARG;
    if (!logp && !counts && !tok_logp && !tok_order) return ASR_ERR_ARG;
    if (((flags & ASR_LM_BOS) && h->bos < 0) || ((flags & ASR_LM_EOS) && h->eos < 0)) return ASR_ERR_ARG;
    if (max_len < 0 || max_len > LM_MAX_LEN) return ASR_ERR_UNSUPPORTED;
    return ASR_OK;
}

}  // namespace asr

int asr_internal_lm_tables(const asr_lm* h, const asr::LmTables** host, const asr::LmTables** dev) {
    *host = &h->host;
    *dev = &h->dev;
    return h->d_blob ? 1 : 0;
}

extern "C" {

int asr_lm_create_arpa_mem(const char* text, size_t bytes, float oov_log10, asr_lm_t** out) {
    if (!out) return ASR_ERR_ARG;
    *out = nullptr;
    if ((!text && bytes) || !std::isfinite(oov_log10) || oov_log10 > 0.0f) return ASR_ERR_ARG;
    asr_lm* h = nullptr;
    int rc;
    try {
        h = new asr_lm();
        h->oov = oov_log10;
        rc = asr::lm_parse(h, text ? text : "", bytes);
    } catch (const std::bad_alloc&) {
        rc = ASR_ERR_OOM;
    } catch (const std::length_error&) {
        rc = ASR_ERR_OOM;
    }
    if (rc != ASR_OK) {
        delete h;
        return rc;
    }
    *out = h;
    return ASR_OK;
}

int asr_lm_create_arpa(const char* path, float oov_log10, asr_lm_t** out) {
    if (!out) return ASR_ERR_ARG;
    *out = nullptr;
    if (!path) return ASR_ERR_ARG;
    FILE* fp = fopen(path, "rb");
    if (!fp) return ASR_ERR_ARG;
    std::string text;
    int rc = ASR_OK;
    try {
        char buf[1 << 16];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, fp)) > 0) text.append(buf, n);
        if (ferror(fp)) rc = ASR_ERR_ARG;
    } catch (const std::bad_alloc&) {
        rc = ASR_ERR_OOM;
    } catch (const std::length_error&) {
        rc = ASR_ERR_OOM;
    }
    fclose(fp);
    if (rc != ASR_OK) return rc;
    return asr_lm_create_arpa_mem(text.data(), text.size(), oov_log10, out);
}

int asr_lm_destroy(asr_lm_t* h) {
    if (!h) return ASR_ERR_ARG;
    int rc = ASR_OK;
    if (h->d_blob && hipFree(h->d_blob) != hipSuccess) rc = ASR_ERR_HIP;
    delete h;
    return rc;
}

int asr_lm_get_info(const asr_lm_t* h, asr_lm_info* info) {
    if (!h || !info) return ASR_ERR_ARG;
    memset(info, 0, sizeof *info);
    info->order = h->order;
    info->vocab = h->vocab;
    info->bos_id = h->bos;
    info->eos_id = h->eos;
    info->unk_id = h->unk;
    for (int k = 0; k < ASR_LM_MAX_ORDER; k++) info->ngrams[k] = h->ngrams[k];
    info->nodes_inserted = h->inserted;
    info->table_bytes = h->table_bytes();
    return ASR_OK;
}

int asr_lm_token_id(const asr_lm_t* h, const char* token, int32_t* id) {
    if (!h || !token || !id) return ASR_ERR_ARG;
    try {
        const auto it = h->ids.find(token);
        *id = it == h->ids.end() ? -1 : it->second;
    } catch (const std::bad_alloc&) {
        return ASR_ERR_OOM;
    }
    return ASR_OK;
}

int asr_lm_token_string(const asr_lm_t* h, int32_t id, const char** token) {
    if (!h || !token || id < 0 || id >= h->vocab) return ASR_ERR_ARG;
    *token = h->strings[(size_t)id].c_str();
    return ASR_OK;
}

int asr_lm_score_host(const asr_lm_t* h, const int32_t* h_tokens, long ldt, const int32_t* h_lengths, int N,
                      int max_len, int flags, double* h_logp, int32_t* h_counts, double* h_tok_logp,
                      int32_t* h_tok_order, long ldd) {
    const int rc = asr::lm_check(h, h_tokens, ldt, N, max_len, flags, h_logp, h_counts, h_tok_logp, h_tok_order, ldd);
    if (rc != ASR_OK) return rc;
    for (long n = 0; n < N; n++) {
        const int32_t* tok = h_tokens + n * ldt;
        int L = max_len;
        if (h_lengths) L = std::min(std::max(h_lengths[n], 0), max_len);
        const int total = L + ((flags & ASR_LM_EOS) ? 1 : 0);
        double part[64];
        for (int l = 0; l < 64; l++) part[l] = 0.0;
        int n_oov = 0;
        for (int i = 0; i < total; i++) {
            const asr::LmTok r = asr::lm_position(h->host, tok, L, i, flags);
            part[i & 63] += r.v;
            n_oov += r.oov;
            if (h_tok_logp) h_tok_logp[n * ldd + i] = r.v;
            if (h_tok_order) h_tok_order[n * ldd + i] = r.order;
        }
        for (int off = 32; off >= 1; off >>= 1)   // the kernel's reduction tree
            for (int l = 0; l < off; l++) part[l] += part[l + off];
        if (h_logp) h_logp[n] = part[0];
        if (h_counts) {
            h_counts[2 * n] = total;
            h_counts[2 * n + 1] = n_oov;
        }
    }
    return ASR_OK;
}

int asr_lm_upload(asr_lm_t* h) {
    if (!h) return ASR_ERR_ARG;
    if (h->d_blob) return ASR_OK;
    // one allocation: every array at a 16-byte aligned offset
    size_t off_w[ASR_LM_MAX_ORDER + 1] = {}, off_n[ASR_LM_MAX_ORDER + 1] = {}, total = 0;
    for (int k = 1; k <= h->order; k++) {
        off_w[k] = total;
        total += (h->words[k].size() * 4 + 15) & ~(size_t)15;
        off_n[k] = total;
        total += (h->nodes[k].size() * sizeof(asr::LmNode) + 15) & ~(size_t)15;
    }
    void* d = nullptr;
    ASR_HIP_TRY(hipMalloc(&d, total));
    for (int k = 1; k <= h->order; k++) {
        hipError_t e = hipSuccess;
        if (!h->words[k].empty())
            e = hipMemcpy((char*)d + off_w[k], h->words[k].data(), h->words[k].size() * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMemcpy((char*)d + off_n[k], h->nodes[k].data(), h->nodes[k].size() * sizeof(asr::LmNode),
                          hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            asr_internal_set_error("hipMemcpy (LM tables)", hipGetErrorString(e), __FILE__, __LINE__);
            (void)hipFree(d);
            return ASR_ERR_HIP;
        }
    }
    h->dev = h->host;
    for (int k = 1; k <= h->order; k++) {
        h->dev.words[k] = (const int32_t*)((char*)d + off_w[k]);
        h->dev.nodes[k] = (const asr::LmNode*)((char*)d + off_n[k]);
    }
    h->d_blob = d;
    return ASR_OK;
}

int asr_lm_score(const asr_lm_t* h, const int32_t* d_tokens, long ldt, const int32_t* d_lengths, int N,
                 int max_len, int flags, double* d_logp, int32_t* d_counts, double* d_tok_logp,
                 int32_t* d_tok_order, long ldd, asr_stream_t s) {
    const int rc = asr::lm_check(h, d_tokens, ldt, N, max_len, flags, d_logp, d_counts, d_tok_logp, d_tok_order, ldd);
    if (rc != ASR_OK) return rc;
    if (!h->d_blob) return ASR_ERR_STATE;
    asr::LmScoreArgs a;
    a.tokens = d_tokens;
    a.ldt = ldt;
    a.lengths = d_lengths;
    a.logp = d_logp;
    a.counts = d_counts;
    a.tok_logp = d_tok_logp;
    a.tok_order = d_tok_order;
    a.ldd = ldd;
    a.N = N;
    a.max_len = max_len;
    a.flags = flags;
    const unsigned grid = (unsigned)(((long)N + asr::LM_WAVES - 1) / asr::LM_WAVES);
    asr::lm_score_kernel<<<dim3(grid), dim3(64 * asr::LM_WAVES), 0, asr_stream(s)>>>(h->dev, a);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

}  // extern "C"
