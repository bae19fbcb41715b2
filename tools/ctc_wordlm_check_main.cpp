// The word mode of the LM-fused beam search (csrc/ctc_lm.hip: the lexicon trie and
// the host twin on a word handle) as a stand-alone program for a sanitizer build
// on the CPU (`make -C gpu-accelerated-speech-recognition_amd wordlmcheck`
// compiles csrc/ctc_lm.hip, csrc/lm.hip and this file with
// -fsanitize=address,undefined and runs the result).  It runs the worked example
// of DESIGN.md §23, a few hundred random small decodes of asr_ctc_lm_decode_host
// in both lexicon modes (V <= 8, T <= 12, every flag combination, label cutoffs,
// lengths, both layouts) with all arrays in heap buffers of the exact size, and
// every refusal of asr_lexicon_create and asr_ctc_lm_create_word.  No HIP call is
// made; no GPU is needed or used.
#include "asr_amd.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
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
#define EXPECT_NEAR(x, y, tol)                                                          \
    do {                                                                                \
        const double x_ = (x), y_ = (y);                                                \
        if (!(std::fabs(x_ - y_) <= (tol))) {                                           \
            std::printf("FAIL %s:%d %s: got %.12g, want %.12g\n", __FILE__, __LINE__, #x, x_, y_); \
            failures++;                                                                 \
        }                                                                               \
    } while (0)

static uint64_t rng_state = 0xD1B54A32D192ED03ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}
static double unit() { return (rnd() % 1000000 + 0.5) / 1000000.0; }

static asr_lm_t* load(const std::string& text) {
    asr_lm_t* h = nullptr;
    EXPECT(asr_lm_create_arpa_mem(text.data(), text.size(), -3.0f, &h), ASR_OK);
    return h;
}

// P(a | <s>) = P(b | <s>) = 0.05, P(c | <s>) = 0.9 (the worked example); tokens a, b, c = 2, 3, 4
static const char* WORKED =
    "\n\\data\\\nngram 1=5\nngram 2=3\n\n\\1-grams:\n-99\t<s>\t0\n-1.5\t</s>\n-0.7\ta\t0\n-0.7\tb\t0\n-0.7\tc\t0\n\n"
    "\\2-grams:\n-1.30103\t<s> a\n-1.30103\t<s> b\n-0.045757\t<s> c\n\n\\end\\\n";

static void worked_example() {
    asr_lm_t* lm = load(WORKED);
    if (!lm) return;
    const int32_t spell[3] = {1, 2, 3}, tok[3] = {2, 3, 4};
    const int64_t offsets[4] = {0, 1, 2, 3};
    asr_lexicon_t* lex = nullptr;
    EXPECT(asr_lexicon_create(spell, offsets, tok, 3, 5, 4, &lex), ASR_OK);
    const float emis[10] = {0.05f, 0.40f, 0.30f, 0.20f, 0.05f, 0.355f, 0.015f, 0.015f, 0.015f, 0.60f};
    for (int mode = ASR_LEX_OPEN; lex && mode <= ASR_LEX_CLOSED; mode++) {
        asr_ctc_lm_t* h = nullptr;
        EXPECT(asr_ctc_lm_create_word(nullptr, 5, 2, 0, 0, lm, lex, 1.0f, 0.0f, ASR_LM_BOS, 0, mode, &h), ASR_OK);
        if (!h) continue;
        EXPECT(asr_ctc_lm_decode_host(h, emis, 2, 1, 5, 5, nullptr, 0), ASR_OK);
        std::vector<int32_t> nh(1), len(4), lab(8), nt(4);
        std::vector<double> total(4), ctc(4), lm10(4);
        EXPECT(asr_ctc_lm_get_beams(h, 4, 2, nh.data(), len.data(), lab.data(), total.data(), ctc.data(), lm10.data(),
                                    nt.data()), ASR_OK);
        EXPECT(nh[0], 3);
        EXPECT(len[0], 2);
        EXPECT(lab[0], 3);   // "c ": the plain search of the same width pruned it at frame 1
        EXPECT(lab[1], 4);
        EXPECT(nt[0], 1);
        EXPECT_NEAR(ctc[0], std::log(0.20 * 0.60), 1e-6);
        EXPECT_NEAR(lm10[0], -0.045757, 1e-6);
        EXPECT_NEAR(total[0], std::log(0.20 * 0.60) + 2.302585092994046 * -0.045757, 1e-6);
        EXPECT(len[1], 1);
        EXPECT(lab[2], 1);   // "a": its pending word is scored at the final
        EXPECT(nt[1], 1);
        EXPECT_NEAR(total[1], std::log(0.40 * 0.355) + 2.302585092994046 * -1.30103, 1e-6);
        EXPECT(asr_ctc_lm_destroy(h), ASR_OK);
    }
    if (lex) EXPECT(asr_lexicon_destroy(lex), ASR_OK);
    asr_lm_destroy(lm);
}

// A model over the tokens t0 .. t(n-1) with random bigrams and trigrams.
static std::string random_model(int n, bool unk) {
    std::vector<std::string> names = {"<s>", "</s>"};
    if (unk) names.push_back("<unk>");
    for (int i = 0; i < n; i++) names.push_back("t" + std::to_string(i));
    const int nv = (int)names.size();
    std::vector<std::string> bi, tri;
    std::vector<int> seen((size_t)nv * nv, 0);
    for (int k = 0; k < 2 * nv; k++) {
        const int a = (int)(rnd() % nv), b = (int)(rnd() % nv);
        if (a == 1 || b == 0 || seen[(size_t)a * nv + b]) continue;
        seen[(size_t)a * nv + b] = 1;
        bi.push_back(std::to_string(-3.0 * unit()) + "\t" + names[a] + " " + names[b] + "\t" + std::to_string(-unit()));
        if (rnd() % 2 && b != 1) {
            const int c = 1 + (int)(rnd() % (nv - 1));
            tri.push_back(std::to_string(-3.0 * unit()) + "\t" + names[a] + " " + names[b] + " " + names[c]);
        }
    }
    std::string t = "\n\\data\\\nngram 1=" + std::to_string(nv) + "\nngram 2=" + std::to_string(bi.size()) +
                    "\nngram 3=" + std::to_string(tri.size()) + "\n\n\\1-grams:\n";
    for (const std::string& s : names) t += std::to_string(-4.0 * unit()) + "\t" + s + "\t" + std::to_string(-unit()) + "\n";
    t += "\n\\2-grams:\n";
    for (const std::string& s : bi) t += s + "\n";
    t += "\n\\3-grams:\n";
    for (const std::string& s : tri) t += s + "\n";
    return t + "\n\\end\\\n";
}

static void random_decodes() {
    int decodes = 0, overflows = 0, words_seen = 0;
    for (int round = 0; round < 40; round++) {
        const int ntok = 2 + (int)(rnd() % 5);
        asr_lm_t* lm = load(random_model(ntok, rnd() % 2));
        if (!lm) return;
        for (int rep = 0; rep < 8; rep++) {
            const int V = 3 + (int)(rnd() % 6), T = 1 + (int)(rnd() % 12), B = 1 + (int)(rnd() % 3);
            const int beam = 1 + (int)(rnd() % 6), flags = (int)(rnd() % 4), mode = (int)(rnd() % 2);
            const int blank = (int)(rnd() % V);
            int space = (int)(rnd() % V);
            if (space == blank) space = (space + 1) % V;
            const int top_n = rnd() % 2 ? (int)(rnd() % (V + 1)) : 0;
            const bool is_log = rnd() % 2, batch_major = rnd() % 2, with_len = rnd() % 2, quant = rnd() % 2;
            // a lexicon of 1 .. 6 words of 1 .. 3 letters; the same spelling may come twice with its first token
            std::vector<int32_t> letters;
            for (int v = 0; v < V; v++)
                if (v != blank && v != space) letters.push_back(v);
            std::vector<int32_t> spell, tok, codes(V), lengths(B);
            std::vector<int64_t> offsets(1, 0);
            std::vector<std::pair<std::vector<int32_t>, int32_t>> made;
            const int nwords = 1 + (int)(rnd() % 6);
            for (int w = 0; w < nwords; w++) {
                std::vector<int32_t> s;
                const int n = 1 + (int)(rnd() % 3);
                for (int i = 0; i < n; i++) s.push_back(letters[rnd() % letters.size()]);
                int32_t t = (int32_t)(rnd() % (ntok + 5));   // some ids are no token of the model
                for (const auto& m : made)
                    if (m.first == s) t = m.second;
                made.push_back({s, t});
                spell.insert(spell.end(), s.begin(), s.end());
                offsets.push_back((int64_t)spell.size());
                tok.push_back(t);
            }
            for (int v = 0; v < V; v++) codes[v] = 100 - 3 * v;   // string order is not label order
            for (int b = 0; b < B; b++) lengths[b] = 1 + (int)(rnd() % T);
            std::vector<float> emis((size_t)T * B * V);
            for (float& x : emis) {
                double p = quant ? (1 + rnd() % 3) / 8.0 : 0.02 + 0.9 * unit();
                x = (float)(is_log ? std::log(p) : p);
            }
            asr_lexicon_t* lex = nullptr;
            EXPECT(asr_lexicon_create(spell.data(), offsets.data(), tok.data(), nwords, V, space, &lex), ASR_OK);
            if (!lex) continue;
            asr_lexicon_info info;
            EXPECT(asr_lexicon_get_info(lex, &info), ASR_OK);
            EXPECT(info.words >= 1 && info.words <= nwords && info.nodes <= (int)spell.size() + 1, 1);
            asr_ctc_lm_t* h = nullptr;
            EXPECT(asr_ctc_lm_create_word(rnd() % 2 ? codes.data() : nullptr, V, beam, blank, 0, lm, lex,
                                          (float)(2.0 * unit()), (float)(2.0 * unit() - 1.0), flags, top_n, mode, &h),
                   ASR_OK);
            if (!h) {
                asr_lexicon_destroy(lex);
                continue;
            }
            const long fs = batch_major ? V : (long)B * V, us = batch_major ? (long)T * V : V;
            EXPECT(asr_ctc_lm_decode_host(h, emis.data(), T, B, fs, us, with_len ? lengths.data() : nullptr, is_log), ASR_OK);
            const int mh = 1 + (int)(rnd() % 40), ml = T;
            std::vector<int32_t> nh(B), len((size_t)B * mh), lab((size_t)B * mh * ml), nt((size_t)B * mh);
            std::vector<double> total((size_t)B * mh), ctc((size_t)B * mh), lm10((size_t)B * mh), gap(B);
            const int rc = asr_ctc_lm_get_beams(h, mh, ml, nh.data(), len.data(), lab.data(), total.data(), ctc.data(),
                                                lm10.data(), nt.data());
            if (rc == ASR_ERR_BEAM_OVERFLOW) overflows++;
            else EXPECT(rc, ASR_OK);
            for (int b = 0; b < B && rc == ASR_OK; b++) {
                EXPECT(nh[b] >= 1, 1);
                for (int k = 0; k < nh[b] && k < mh; k++) {
                    const size_t i = (size_t)b * mh + k;
                    // n is the number of maximal runs of letters
                    int words = 0;
                    bool in_word = false;
                    for (int j = 0; j < len[i]; j++) {
                        const bool sp = lab[i * ml + j] == space;
                        if (!sp && !in_word) words++;
                        in_word = !sp;
                        if (mode == ASR_LEX_CLOSED && sp) EXPECT(j > 0 && lab[i * ml + j - 1] != space, 1);
                    }
                    EXPECT(nt[i], words);
                    words_seen += words;
                    EXPECT(len[i] <= (with_len ? lengths[b] : T), 1);
                    if (k) EXPECT(total[i] <= total[i - 1], 1);
                    if (!(flags & ASR_LM_EOS) && words == 0) EXPECT(total[i] == ctc[i], 1);
                }
            }
            EXPECT(asr_ctc_lm_host_gaps(h, gap.data()), ASR_OK);
            EXPECT(asr_ctc_lm_destroy(h), ASR_OK);
            EXPECT(asr_lexicon_destroy(lex), ASR_OK);
            decodes++;
        }
        asr_lm_destroy(lm);
    }
    std::printf("ctc_wordlm_check: %d random decodes (%d reported a beam overflow), %d words scored\n", decodes,
                overflows, words_seen);
}

static void refusals() {
    asr_lm_t* lm = load(WORKED);
    asr_lm_t* bare = load("\n\\data\\\nngram 1=1\n\n\\1-grams:\n-1\ta\n\n\\end\\\n");   // neither <s> nor </s>
    if (!lm || !bare) return;
    const int32_t spell[3] = {1, 2, 3}, tok[2] = {2, 3};
    const int64_t offsets[3] = {0, 2, 3};
    asr_lexicon_t* lex = nullptr;
    // asr_lexicon_create
    EXPECT(asr_lexicon_create(spell, offsets, tok, 2, 5, 4, nullptr), ASR_ERR_ARG);
    EXPECT(asr_lexicon_create(nullptr, offsets, tok, 2, 5, 4, &lex), ASR_ERR_ARG);
    EXPECT(asr_lexicon_create(spell, nullptr, tok, 2, 5, 4, &lex), ASR_ERR_ARG);
    EXPECT(asr_lexicon_create(spell, offsets, nullptr, 2, 5, 4, &lex), ASR_ERR_ARG);
    EXPECT(asr_lexicon_create(spell, offsets, tok, 2, 1, 0, &lex), ASR_ERR_ARG);
    EXPECT(asr_lexicon_create(spell, offsets, tok, 0, 5, 4, &lex), ASR_ERR_ARG);
    EXPECT(asr_lexicon_create(spell, offsets, tok, 2, 5, -1, &lex), ASR_ERR_ARG);
    EXPECT(asr_lexicon_create(spell, offsets, tok, 2, 5, 5, &lex), ASR_ERR_ARG);
    {
        const int64_t from_one[3] = {1, 2, 3}, down[3] = {0, 3, 2}, empty[3] = {0, 3, 3}, twice[3] = {0, 2, 4};
        const int32_t neg[3] = {1, -1, 3}, past[3] = {1, 5, 3}, sp[3] = {1, 4, 3}, tneg[2] = {2, -1};
        const int32_t same[4] = {1, 2, 1, 2}, equal_tok[2] = {3, 3};
        EXPECT(asr_lexicon_create(spell, from_one, tok, 2, 5, 4, &lex), ASR_ERR_ARG);
        EXPECT(asr_lexicon_create(spell, down, tok, 2, 5, 4, &lex), ASR_ERR_ARG);
        EXPECT(asr_lexicon_create(neg, offsets, tok, 2, 5, 4, &lex), ASR_ERR_ARG);
        EXPECT(asr_lexicon_create(past, offsets, tok, 2, 5, 4, &lex), ASR_ERR_ARG);
        EXPECT(asr_lexicon_create(sp, offsets, tok, 2, 5, 4, &lex), ASR_ERR_ARG);
        EXPECT(asr_lexicon_create(spell, empty, tok, 2, 5, 4, &lex), ASR_ERR_ARG);
        EXPECT(asr_lexicon_create(spell, offsets, tneg, 2, 5, 4, &lex), ASR_ERR_ARG);
        EXPECT(asr_lexicon_create(same, twice, tok, 2, 5, 4, &lex), ASR_ERR_ARG);   // one spelling, two tokens
        EXPECT(lex == nullptr, 1);
        EXPECT(asr_lexicon_create(same, twice, equal_tok, 2, 5, 4, &lex), ASR_OK);   // the same word twice
        if (lex) {
            asr_lexicon_info info;
            EXPECT(asr_lexicon_get_info(lex, &info), ASR_OK);
            EXPECT(info.words, 1);
            EXPECT(info.nodes, 3);
            EXPECT(info.max_children, 1);
            EXPECT(info.table_bytes, 4 * (4 + 3 + 3));
            EXPECT(asr_lexicon_get_info(nullptr, &info), ASR_ERR_ARG);
            EXPECT(asr_lexicon_get_info(lex, nullptr), ASR_ERR_ARG);
            EXPECT(asr_lexicon_destroy(lex), ASR_OK);
            lex = nullptr;
        }
    }
    EXPECT(asr_lexicon_upload(nullptr), ASR_ERR_ARG);
    EXPECT(asr_lexicon_destroy(nullptr), ASR_ERR_ARG);
    // asr_ctc_lm_create_word: labels 0 blank, 1 2 3 letters, 4 space
    EXPECT(asr_lexicon_create(spell, offsets, tok, 2, 5, 4, &lex), ASR_OK);
    if (!lex) return;
    asr_ctc_lm_t* h = nullptr;
    const float nanf_ = std::nanf(""), inf_ = INFINITY;
    const int32_t same_codes[5] = {4, 5, 4, 6, 7};
    EXPECT(asr_ctc_lm_create_word(nullptr, 5, 2, 0, 0, lm, lex, 0.5f, 0.0f, 1, 0, 0, nullptr), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create_word(nullptr, 5, 2, 0, 0, nullptr, lex, 0.5f, 0.0f, 1, 0, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create_word(nullptr, 5, 2, 0, 0, lm, nullptr, 0.5f, 0.0f, 1, 0, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create_word(nullptr, 1, 2, 0, 0, lm, lex, 0.5f, 0.0f, 1, 0, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create_word(nullptr, 5, 0, 0, 0, lm, lex, 0.5f, 0.0f, 1, 0, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create_word(nullptr, 5, 2, -1, 0, lm, lex, 0.5f, 0.0f, 1, 0, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create_word(nullptr, 5, 2, 5, 0, lm, lex, 0.5f, 0.0f, 1, 0, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create_word(nullptr, 5, 2, 0, 0, lm, lex, -0.5f, 0.0f, 1, 0, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create_word(nullptr, 5, 2, 0, 0, lm, lex, nanf_, 0.0f, 1, 0, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create_word(nullptr, 5, 2, 0, 0, lm, lex, inf_, 0.0f, 1, 0, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create_word(nullptr, 5, 2, 0, 0, lm, lex, 0.5f, nanf_, 1, 0, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create_word(nullptr, 5, 2, 0, 0, lm, lex, 0.5f, -inf_, 1, 0, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create_word(nullptr, 5, 2, 0, 0, lm, lex, 0.5f, 0.0f, 4, 0, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create_word(nullptr, 5, 2, 0, 0, lm, lex, 0.5f, 0.0f, 1, -1, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create_word(nullptr, 5, 2, 0, -1, lm, lex, 0.5f, 0.0f, 1, 0, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create_word(nullptr, 5, 2, 0, 0, bare, lex, 0.5f, 0.0f, ASR_LM_BOS, 0, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create_word(nullptr, 5, 2, 0, 0, bare, lex, 0.5f, 0.0f, ASR_LM_EOS, 0, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create_word(nullptr, 6, 2, 0, 0, lm, lex, 0.5f, 0.0f, 1, 0, 0, &h), ASR_ERR_ARG);   // the lexicon's V
    EXPECT(asr_ctc_lm_create_word(nullptr, 5, 2, 2, 0, lm, lex, 0.5f, 0.0f, 1, 0, 0, &h), ASR_ERR_ARG);   // a spelling uses the blank
    EXPECT(asr_ctc_lm_create_word(nullptr, 5, 2, 4, 0, lm, lex, 0.5f, 0.0f, 1, 0, 0, &h), ASR_ERR_ARG);   // the space is the blank
    EXPECT(asr_ctc_lm_create_word(nullptr, 5, 2, 0, 0, lm, lex, 0.5f, 0.0f, 1, 0, 2, &h), ASR_ERR_ARG);   // lex_mode
    EXPECT(asr_ctc_lm_create_word(nullptr, 5, 2, 0, 0, lm, lex, 0.5f, 0.0f, 1, 0, -1, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create_word(same_codes, 5, 2, 0, 0, lm, lex, 0.5f, 0.0f, 1, 0, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create_word(nullptr, 5, 4, 0, 4, lm, lex, 0.5f, 0.0f, 1, 0, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create_word(nullptr, 5, 250, 0, 0, lm, lex, 0.5f, 0.0f, 1, 0, 0, &h), ASR_ERR_UNSUPPORTED);
    {
        const int32_t one[1] = {1}, t1[1] = {2};
        const int64_t off[2] = {0, 1};
        asr_lexicon_t *wide = nullptr, *huge = nullptr;
        EXPECT(asr_lexicon_create(one, off, t1, 1, 300, 2, &wide), ASR_OK);
        EXPECT(asr_lexicon_create(one, off, t1, 1, 4097, 2, &huge), ASR_OK);
        if (wide && huge) {
            EXPECT(asr_ctc_lm_create_word(nullptr, 300, 2, 0, 0, lm, wide, 0.5f, 0.0f, 1, 0, 0, &h), ASR_ERR_UNSUPPORTED);
            EXPECT(asr_ctc_lm_create_word(nullptr, 300, 2, 0, 0, lm, wide, 0.5f, 0.0f, 1, 256, 0, &h), ASR_ERR_UNSUPPORTED);
            EXPECT(asr_ctc_lm_create_word(nullptr, 4097, 2, 0, 0, lm, huge, 0.5f, 0.0f, 1, 40, 0, &h), ASR_ERR_UNSUPPORTED);
        }
        if (wide) asr_lexicon_destroy(wide);
        if (huge) asr_lexicon_destroy(huge);
    }
    EXPECT(h == nullptr, 1);
    EXPECT(asr_ctc_lm_create_word(nullptr, 5, 2, 0, 0, bare, lex, 0.5f, 0.0f, 0, 0, ASR_LEX_CLOSED, &h), ASR_OK);
    if (h) {
        const float emis[10] = {0.1f, 0.4f, 0.3f, 0.1f, 0.1f, 0.2f, 0.1f, 0.5f, 0.1f, 0.1f};
        int32_t i32[8] = {};
        double gap = 0.0;
        EXPECT(asr_ctc_lm_get_beams(h, 1, 1, i32, i32, i32, nullptr, nullptr, nullptr, nullptr), ASR_ERR_STATE);
        // neither the LM nor the lexicon is uploaded: refused before it would touch the device pointer
        EXPECT(asr_ctc_lm_decode(h, emis, 2, 1, 5, 5, nullptr, 0, nullptr), ASR_ERR_STATE);
        EXPECT(asr_ctc_lm_decode_host(h, emis, 2, 1, 5, 5, nullptr, 0), ASR_OK);
        EXPECT(asr_ctc_lm_get_beams(h, 1, 1, i32, i32 + 1, i32 + 2, nullptr, nullptr, nullptr, nullptr), ASR_OK);
        EXPECT(asr_ctc_lm_get_best(h, i32, 1, i32 + 1, nullptr), ASR_OK);
        EXPECT(asr_ctc_lm_host_gaps(h, &gap), ASR_OK);
        EXPECT(asr_ctc_lm_destroy(h), ASR_OK);
    }
    EXPECT(asr_lexicon_destroy(lex), ASR_OK);
    asr_lm_destroy(lm);
    asr_lm_destroy(bare);
}

int main() {
    worked_example();
    random_decodes();
    refusals();
    if (failures) {
        std::printf("ctc_wordlm_check: %d FAILED\n", failures);
        return 1;
    }
    std::printf("ctc_wordlm_check: ok\n");
    return 0;
}
