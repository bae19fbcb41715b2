// The ARPA loader and the host scorer of csrc/lm.hip as a stand-alone program for
// a sanitizer build on the CPU (`make -C gpu-accelerated-speech-recognition_amd
// lmcheck` compiles csrc/lm.hip and this file with -fsanitize=address,undefined
// and runs the result).  It feeds the parser valid and malformed texts —
// truncated at every byte, counts that lie, over-long lines and tokens, missing
// fields, empty input — in heap buffers of the exact size (no terminating NUL:
// a read past the end is an ASan report), and runs asr_lm_score_host on the
// models that load.  No HIP call is made; no GPU is needed or used.
#include "asr_amd.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static int failures = 0;
#define EXPECT(expr, want)                                                              \
    do {                                                                                \
        const long got_ = (long)(expr);                                                 \
        if (got_ != (long)(want)) {                                                     \
            std::printf("FAIL %s:%d %s: got %ld, want %ld\n", __FILE__, __LINE__, #expr, got_, (long)(want)); \
            failures++;                                                                 \
        }                                                                               \
    } while (0)

// Parse `text` from a heap copy of exactly its size.
static int load(const std::string& text, asr_lm_t** out) {
    std::vector<char> buf(text.begin(), text.end());
    return asr_lm_create_arpa_mem(buf.empty() ? nullptr : buf.data(), buf.size(), -7.0f, out);
}

static int load_status(const std::string& text) {
    asr_lm_t* h = nullptr;
    const int rc = load(text, &h);
    if (rc == ASR_OK) asr_lm_destroy(h);
    else if (h) failures++, std::printf("FAIL: a handle came back with status %d\n", rc);
    return rc;
}

// Score a few hypotheses, OOV ids included, every output asked for.
static void score(asr_lm_t* h) {
    asr_lm_info info;
    EXPECT(asr_lm_get_info(h, &info), ASR_OK);
    const int N = 5, max_len = 70, ldt = 72, ldd = 71;
    std::vector<int32_t> tok((size_t)N * ldt), len = {0, 1, 70, 65, 1000}, counts(2 * N), order((size_t)N * ldd);
    std::vector<double> logp(N), tl((size_t)N * ldd);
    for (size_t i = 0; i < tok.size(); i++) tok[i] = (int32_t)(i * 7 % (size_t)(info.vocab + 3)) - 1;
    for (int flags = 0; flags < 4; flags++) {
        const bool ok = (!(flags & ASR_LM_BOS) || info.bos_id >= 0) && (!(flags & ASR_LM_EOS) || info.eos_id >= 0);
        EXPECT(asr_lm_score_host(h, tok.data(), ldt, len.data(), N, max_len, flags, logp.data(), counts.data(),
                                 tl.data(), order.data(), ldd), ok ? ASR_OK : ASR_ERR_ARG);
        if (!ok) continue;
        EXPECT(counts[0], (flags & ASR_LM_EOS) ? 1 : 0);
        EXPECT(counts[8], 70 + ((flags & ASR_LM_EOS) ? 1 : 0));   // a length beyond max_len is clamped
        EXPECT(asr_lm_score_host(h, tok.data(), ldt, nullptr, N, max_len, flags, logp.data(), nullptr, nullptr,
                                 nullptr, 0), ASR_OK);
    }
}

int main() {
    const std::string good =
        "header\n\\data\\\nngram 1=5\nngram 2=5\nngram 3=3\n\n"
        "\\1-grams:\n-99\t<s>\t-0.5\n-1.0\t</s>\n-1.5\ta\t-0.25\n-2.0 b -0.75\n-2.5\tc\t-0.125\n\n"
        "\\2-grams:\n-0.5\t<s> a\t-0.375\n-0.625\ta b\t-0.25\n-0.875\tb c\n-1.125\tc </s>\n-1.25\ta a\t-1.0\n\n"
        "\\3-grams:\n-0.125\t<s> a b\n-0.25\ta b c\n-0.0625\tb a c\n\n\\end\\\n";
    asr_lm_t* h = nullptr;
    EXPECT(load(good, &h), ASR_OK);
    if (h) {
        asr_lm_info info;
        EXPECT(asr_lm_get_info(h, &info), ASR_OK);
        EXPECT(info.order, 3);
        EXPECT(info.vocab, 5);
        EXPECT(info.nodes_inserted, 1);
        int32_t id = 0;
        EXPECT(asr_lm_token_id(h, "c", &id), ASR_OK);
        EXPECT(id, 4);
        EXPECT(asr_lm_token_id(h, "", &id), ASR_OK);
        EXPECT(id, -1);
        const char* s = nullptr;
        EXPECT(asr_lm_token_string(h, 5, &s), ASR_ERR_ARG);
        EXPECT(asr_lm_token_string(h, 1, &s), ASR_OK);
        EXPECT(s && !std::strcmp(s, "</s>"), 1);
        // <s> a b c </s> = -0.5 - 0.125 - 0.25 - 1.125
        const int32_t abc[3] = {2, 3, 4};
        double lp = 0;
        EXPECT(asr_lm_score_host(h, abc, 3, nullptr, 1, 3, ASR_LM_BOS | ASR_LM_EOS, &lp, nullptr, nullptr, nullptr, 0),
               ASR_OK);
        EXPECT(lp == -2.0, 1);
        score(h);
        // the device entry point refuses before any HIP call: not uploaded
        EXPECT(asr_lm_score(h, abc, 3, nullptr, 1, 3, 0, &lp, nullptr, nullptr, nullptr, 0, nullptr), ASR_ERR_STATE);
        EXPECT(asr_lm_destroy(h), ASR_OK);
    }

    // truncated at every byte: never a crash, never a handle with a bad status;
    // the text is complete only once \end\ is
    const size_t end_at = good.find("\\end\\") + 5;
    for (size_t n = 0; n <= good.size(); n++) EXPECT(load_status(good.substr(0, n)), n >= end_at ? ASR_OK : ASR_ERR_ARG);
    // every line removed in turn
    {
        size_t b = 0;
        int ok = 0;
        while (b < good.size()) {
            const size_t e = good.find('\n', b) + 1;
            const int rc = load_status(good.substr(0, b) + good.substr(e));
            if (rc == ASR_OK) ok++;
            else EXPECT(rc, ASR_ERR_ARG);
            b = e;
        }
        EXPECT(ok, 1 + 4);   // only the header line and the four blank lines may go
    }
    // every byte replaced by a NUL, a tab and a digit in turn: any status, no crash
    for (size_t n = 0; n < good.size(); n++)
        for (const char c : {'\0', '\t', '7', '\\', '\n'}) {
            std::string t = good;
            t[n] = c;
            (void)load_status(t);
        }

    // empty input, no sections, no unigrams
    EXPECT(load_status(""), ASR_ERR_ARG);
    EXPECT(load_status("\n\n\n"), ASR_ERR_ARG);
    EXPECT(load_status("\\data\\"), ASR_ERR_ARG);
    EXPECT(load_status("\\data\\\n\\end\\"), ASR_ERR_ARG);
    EXPECT(load_status("\\data\\\nngram 1=0\n\\1-grams:\n\\end\\\n"), ASR_ERR_ARG);
    EXPECT(load_status("\\data\\\nngram 1=1\n\\1-grams:\n-1 a\n\\end\\"), ASR_OK);   // no final newline
    // counts that lie, in both directions and beyond what is supported
    EXPECT(load_status("\\data\\\nngram 1=2\n\\1-grams:\n-1 a\n\\end\\\n"), ASR_ERR_ARG);
    EXPECT(load_status("\\data\\\nngram 1=1\n\\1-grams:\n-1 a\n-1 b\n\\end\\\n"), ASR_ERR_ARG);
    EXPECT(load_status("\\data\\\nngram 1=2147483647\n\\1-grams:\n-1 a\n\\end\\\n"), ASR_ERR_ARG);
    EXPECT(load_status("\\data\\\nngram 1=2147483648\n\\1-grams:\n-1 a\n\\end\\\n"), ASR_ERR_UNSUPPORTED);
    EXPECT(load_status("\\data\\\nngram 1=99999999999999999999999999\n\\1-grams:\n-1 a\n\\end\\\n"), ASR_ERR_ARG);
    EXPECT(load_status("\\data\\\nngram 9=1\n\\end\\\n"), ASR_ERR_UNSUPPORTED);
    EXPECT(load_status("\\data\\\nngram 999999999=1\n\\end\\\n"), ASR_ERR_ARG);
    EXPECT(load_status("\\data\\\nngram 1=1\nngram 3=1\n\\1-grams:\n-1 a\n\\end\\\n"), ASR_ERR_ARG);
    EXPECT(load_status("\\data\\\nngram 1=1\n\\1-grams:\n-1 a\n\\99999999999-grams:\n\\end\\\n"), ASR_ERR_ARG);
    // missing fields, too many fields
    EXPECT(load_status("\\data\\\nngram 1=1\n\\1-grams:\n-1\n\\end\\\n"), ASR_ERR_ARG);
    EXPECT(load_status("\\data\\\nngram 1=1\n\\1-grams:\n-1 a -1 -1\n\\end\\\n"), ASR_ERR_ARG);
    EXPECT(load_status("\\data\\\nngram 1=1\nngram 2=1\n\\1-grams:\n-1 a\n\\2-grams:\n-1 a\n\\end\\\n"), ASR_ERR_ARG);
    // over-long lines and tokens
    {
        const std::string longtok(1 << 20, 'x');
        asr_lm_t* g = nullptr;
        EXPECT(load("\\data\\\nngram 1=2\nngram 2=1\n\\1-grams:\n-1 " + longtok + " -0.5\n-2 </s>\n\\2-grams:\n-0.5 " +
                        longtok + " </s>\n\\end\\\n", &g), ASR_OK);
        if (g) {
            int32_t id = -1;
            EXPECT(asr_lm_token_id(g, longtok.c_str(), &id), ASR_OK);
            EXPECT(id, 0);
            score(g);
            asr_lm_destroy(g);
        }
        EXPECT(load_status("\\data\\\nngram 1=1\n\\1-grams:\n-1 a" + std::string(1 << 20, ' ') + "-0.5\n\\end\\\n"), ASR_OK);
        EXPECT(load_status("\\data\\\nngram 1=1\n\\1-grams:\n-" + std::string(1 << 16, '1') + " a\n\\end\\\n"), ASR_ERR_ARG);
        EXPECT(load_status("\\data\\\nngram 1=1\n\\1-grams:\n-0." + std::string(1 << 16, '1') + " a\n\\end\\\n"), ASR_OK);
        EXPECT(load_status(std::string(1 << 20, '\\')), ASR_ERR_ARG);
        EXPECT(load_status("\\data\\\nngram 1=1\n\\1-grams:\n" + std::string(1 << 20, '\t') + "\n-1 a\n\\end\\"), ASR_OK);
    }
    // an order-8 model whose only 8-gram needs six inserted nodes
    {
        std::string t = "\\data\\\n";
        for (int k = 1; k <= 8; k++) t += "ngram " + std::to_string(k) + "=" + (k == 1 ? "3" : k == 8 ? "1" : "0") + "\n";
        t += "\\1-grams:\n-1 <s>\n-1 </s>\n-1 a\n";
        for (int k = 2; k <= 7; k++) t += "\\" + std::to_string(k) + "-grams:\n";
        t += "\\8-grams:\n-0.5 a a a a a a a a\n\\end\\\n";
        asr_lm_t* g = nullptr;
        EXPECT(load(t, &g), ASR_OK);
        if (g) {
            asr_lm_info info;
            EXPECT(asr_lm_get_info(g, &info), ASR_OK);
            EXPECT(info.order, 8);
            EXPECT(info.nodes_inserted, 6);
            const int32_t a9[9] = {2, 2, 2, 2, 2, 2, 2, 2, 2};
            int32_t ord[10];
            EXPECT(asr_lm_score_host(g, a9, 9, nullptr, 1, 9, 0, nullptr, nullptr, nullptr, ord, 10), ASR_OK);
            EXPECT(ord[6], 1);
            EXPECT(ord[7], 8);
            EXPECT(ord[8], 8);
            score(g);
            asr_lm_destroy(g);
        }
    }
    // bad arguments
    EXPECT(asr_lm_create_arpa_mem(good.data(), good.size(), -1.0f, nullptr), ASR_ERR_ARG);
    EXPECT(asr_lm_create_arpa(nullptr, -1.0f, &h), ASR_ERR_ARG);
    EXPECT(asr_lm_create_arpa("/nonexistent/dir/model.arpa", -1.0f, &h), ASR_ERR_ARG);
    EXPECT(asr_lm_create_arpa_mem(good.data(), good.size(), 1.0f, &h), ASR_ERR_ARG);
    EXPECT(asr_lm_destroy(nullptr), ASR_ERR_ARG);
    EXPECT(asr_lm_get_info(nullptr, nullptr), ASR_ERR_ARG);
    EXPECT(asr_lm_upload(nullptr), ASR_ERR_ARG);

    if (failures) {
        std::printf("lm check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("lm check: ok\n");
    return 0;
}
