// The host twin of the LM-fused beam search (csrc/ctc_lm.hip) as a stand-alone
// program for a sanitizer build on the CPU (`make -C
// gpu-accelerated-speech-recognition_amd ctclmcheck` compiles csrc/ctc_lm.hip,
// csrc/lm.hip and this file with -fsanitize=address,undefined and runs the
// result).  It runs the worked example of DESIGN.md §21, a few hundred random
// small decodes of asr_ctc_lm_decode_host (V <= 8, T <= 12, every flag
// combination, label cutoffs, OOV labels, lengths, both layouts) with all
// arrays in heap buffers of the exact size, and every refusal of the
// asr_ctc_lm_* entry points.  No HIP call is made; no GPU is needed or used.
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

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}
static double unit() { return (rnd() % 1000000 + 0.5) / 1000000.0; }

static asr_lm_t* load(const std::string& text) {
    asr_lm_t* h = nullptr;
    EXPECT(asr_lm_create_arpa_mem(text.data(), text.size(), -7.0f, &h), ASR_OK);
    return h;
}

// P(a | <s>) = 0.1, P(b | <s>) = 0.8, P(a | b) = 0.9 (the worked example)
static const char* WORKED =
    "\n\\data\\\nngram 1=4\nngram 2=3\n\n\\1-grams:\n-99\t<s>\t0\n-1.5\t</s>\n-0.5\ta\t0\n-0.5\tb\t0\n\n"
    "\\2-grams:\n-1\t<s> a\n-0.09691\t<s> b\n-0.045757\tb a\n\n\\end\\\n";

static void worked_example() {
    asr_lm_t* lm = load(WORKED);
    if (!lm) return;
    const int32_t tok[3] = {-1, 2, 3};
    const float emis[6] = {0.35f, 0.40f, 0.25f, 0.20f, 0.70f, 0.10f};
    asr_ctc_lm_t* h = nullptr;
    EXPECT(asr_ctc_lm_create(nullptr, 3, 1, 0, 0, lm, tok, 1.0f, 0.0f, ASR_LM_BOS, 0, &h), ASR_OK);
    if (h) {
        EXPECT(asr_ctc_lm_decode_host(h, emis, 2, 1, 3, 3, nullptr, 0), ASR_OK);
        std::vector<int32_t> nh(1), len(4), lab(8), nt(4);
        std::vector<double> total(4), ctc(4), lm10(4);
        EXPECT(asr_ctc_lm_get_beams(h, 4, 2, nh.data(), len.data(), lab.data(), total.data(), ctc.data(), lm10.data(),
                                    nt.data()), ASR_OK);
        EXPECT(nh[0], 2);
        EXPECT(len[0], 2);
        EXPECT(lab[0], 2);   // "ba": the plain search pruned "b" at frame 0
        EXPECT(lab[1], 1);
        EXPECT(nt[0], 2);
        EXPECT_NEAR(ctc[0], std::log(0.25 * 0.70), 1e-6);
        EXPECT_NEAR(lm10[0], -0.09691 - 0.045757, 1e-6);
        EXPECT_NEAR(total[0], std::log(0.25 * 0.70) + 2.302585092994046 * (-0.09691 - 0.045757), 1e-6);
        EXPECT(len[1], 0);
        EXPECT_NEAR(total[1], std::log(0.07), 1e-6);
        double gap = 0.0;
        EXPECT(asr_ctc_lm_host_gaps(h, &gap), ASR_OK);
        EXPECT(gap > 1e-3, 1);
        EXPECT(asr_ctc_lm_destroy(h), ASR_OK);
    }
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
    int decodes = 0, overflows = 0;
    for (int round = 0; round < 40; round++) {
        const int ntok = 2 + (int)(rnd() % 5);
        const bool unk = rnd() % 2;
        asr_lm_t* lm = load(random_model(ntok, unk));
        if (!lm) return;
        for (int rep = 0; rep < 8; rep++) {
            const int V = 2 + (int)(rnd() % 7), T = 1 + (int)(rnd() % 12), B = 1 + (int)(rnd() % 3);
            const int beam = 1 + (int)(rnd() % 6), blank = (int)(rnd() % V), flags = (int)(rnd() % 4);
            const int top_n = rnd() % 2 ? (int)(rnd() % (V + 1)) : 0;
            const bool is_log = rnd() % 2, batch_major = rnd() % 2, with_len = rnd() % 2, quant = rnd() % 2;
            std::vector<int32_t> tok(V), codes(V), lengths(B);
            for (int v = 0; v < V; v++) {
                tok[v] = (int32_t)(rnd() % (ntok + 5)) - 1;   // some ids are no token of the model
                codes[v] = 100 - 3 * v;                       // string order is not label order
            }
            for (int b = 0; b < B; b++) lengths[b] = 1 + (int)(rnd() % T);
            std::vector<float> emis((size_t)T * B * V);
            for (float& x : emis) {
                double p = quant ? (1 + rnd() % 3) / 8.0 : 0.02 + 0.9 * unit();
                x = (float)(is_log ? std::log(p) : p);
            }
            asr_ctc_lm_t* h = nullptr;
            EXPECT(asr_ctc_lm_create(rnd() % 2 ? codes.data() : nullptr, V, beam, blank, 0, lm, tok.data(),
                                     (float)(2.0 * unit()), (float)(2.0 * unit() - 1.0), flags, top_n, &h), ASR_OK);
            if (!h) continue;
            const long fs = batch_major ? V : (long)B * V, us = batch_major ? (long)T * V : V;
            EXPECT(asr_ctc_lm_decode_host(h, emis.data(), T, B, fs, us, with_len ? lengths.data() : nullptr, is_log), ASR_OK);
            const int mh = 1 + (int)(rnd() % 40), ml = 1 + (int)(rnd() % T);
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
                    EXPECT(nt[i], len[i]);
                    EXPECT(len[i] <= (with_len ? lengths[b] : T), 1);
                    if (k) EXPECT(total[i] <= total[i - 1], 1);
                    if (!(flags & ASR_LM_EOS) && len[i] == 0) EXPECT(total[i] == ctc[i], 1);
                }
            }
            std::vector<int32_t> blab((size_t)B * ml), blen(B);
            std::vector<double> btot(B);
            EXPECT(asr_ctc_lm_get_best(h, blab.data(), ml, blen.data(), btot.data()), rc);
            if (rc == ASR_OK) EXPECT(btot[0] == total[0], 1);
            EXPECT(asr_ctc_lm_host_gaps(h, gap.data()), ASR_OK);
            EXPECT(asr_ctc_lm_destroy(h), ASR_OK);
            decodes++;
        }
        asr_lm_destroy(lm);
    }
    std::printf("ctc_lm_check: %d random decodes (%d reported a beam overflow)\n", decodes, overflows);
}

static void refusals() {
    asr_lm_t* lm = load(WORKED);
    asr_lm_t* bare = load("\n\\data\\\nngram 1=1\n\n\\1-grams:\n-1\ta\n\n\\end\\\n");   // neither <s> nor </s>
    if (!lm || !bare) return;
    const int32_t tok[3] = {-1, 2, 3};
    const int32_t same[3] = {4, 5, 4};
    std::vector<int32_t> big(5000, -1);
    asr_ctc_lm_t* h = nullptr;
    const float nanf_ = std::nanf(""), inf_ = INFINITY;
    EXPECT(asr_ctc_lm_create(nullptr, 3, 2, 0, 0, lm, tok, 0.5f, 0.0f, 1, 0, nullptr), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create(nullptr, 3, 2, 0, 0, nullptr, tok, 0.5f, 0.0f, 1, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create(nullptr, 3, 2, 0, 0, lm, nullptr, 0.5f, 0.0f, 1, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create(nullptr, 1, 2, 0, 0, lm, tok, 0.5f, 0.0f, 1, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create(nullptr, 3, 0, 0, 0, lm, tok, 0.5f, 0.0f, 1, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create(nullptr, 3, 2, -1, 0, lm, tok, 0.5f, 0.0f, 1, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create(nullptr, 3, 2, 3, 0, lm, tok, 0.5f, 0.0f, 1, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create(nullptr, 3, 2, 0, 0, lm, tok, -0.5f, 0.0f, 1, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create(nullptr, 3, 2, 0, 0, lm, tok, nanf_, 0.0f, 1, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create(nullptr, 3, 2, 0, 0, lm, tok, inf_, 0.0f, 1, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create(nullptr, 3, 2, 0, 0, lm, tok, 0.5f, nanf_, 1, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create(nullptr, 3, 2, 0, 0, lm, tok, 0.5f, -inf_, 1, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create(nullptr, 3, 2, 0, 0, lm, tok, 0.5f, 0.0f, 4, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create(nullptr, 3, 2, 0, 0, lm, tok, 0.5f, 0.0f, 1, -1, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create(nullptr, 3, 2, 0, -1, lm, tok, 0.5f, 0.0f, 1, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create(nullptr, 3, 2, 0, 0, bare, tok, 0.5f, 0.0f, ASR_LM_BOS, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create(nullptr, 3, 2, 0, 0, bare, tok, 0.5f, 0.0f, ASR_LM_EOS, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create(nullptr, 4097, 2, 0, 0, lm, big.data(), 0.5f, 0.0f, 1, 0, &h), ASR_ERR_UNSUPPORTED);
    EXPECT(asr_ctc_lm_create(same, 3, 2, 0, 0, lm, tok, 0.5f, 0.0f, 1, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create(nullptr, 3, 4, 0, 4, lm, tok, 0.5f, 0.0f, 1, 0, &h), ASR_ERR_ARG);
    EXPECT(asr_ctc_lm_create(nullptr, 300, 2, 0, 0, lm, big.data(), 0.5f, 0.0f, 1, 0, &h), ASR_ERR_UNSUPPORTED);
    EXPECT(asr_ctc_lm_create(nullptr, 300, 2, 0, 0, lm, big.data(), 0.5f, 0.0f, 1, 256, &h), ASR_ERR_UNSUPPORTED);
    EXPECT(asr_ctc_lm_create(nullptr, 3, 250, 0, 0, lm, tok, 0.5f, 0.0f, 1, 0, &h), ASR_ERR_UNSUPPORTED);
    EXPECT(h == nullptr, 1);
    EXPECT(asr_ctc_lm_create(nullptr, 3, 2, 0, 0, bare, tok, 0.5f, 0.0f, 0, 0, &h), ASR_OK);
    if (h) {
        const float emis[6] = {0.3f, 0.4f, 0.3f, 0.2f, 0.7f, 0.1f};
        const float* fake = emis;   // asr_ctc_lm_decode refuses before it would touch a device pointer
        int32_t len_bad[3] = {0, 3, -1}, i32[8] = {};
        double gap = 0.0;
        EXPECT(asr_ctc_lm_get_beams(h, 1, 1, i32, i32, i32, nullptr, nullptr, nullptr, nullptr), ASR_ERR_STATE);
        EXPECT(asr_ctc_lm_get_best(h, i32, 1, i32, nullptr), ASR_ERR_STATE);
        EXPECT(asr_ctc_lm_host_gaps(h, &gap), ASR_ERR_STATE);
        EXPECT(asr_ctc_lm_decode_host(nullptr, emis, 2, 1, 3, 3, nullptr, 0), ASR_ERR_ARG);
        EXPECT(asr_ctc_lm_decode_host(h, nullptr, 2, 1, 3, 3, nullptr, 0), ASR_ERR_ARG);
        EXPECT(asr_ctc_lm_decode_host(h, emis, 0, 1, 3, 3, nullptr, 0), ASR_ERR_ARG);
        EXPECT(asr_ctc_lm_decode_host(h, emis, 2, 0, 3, 3, nullptr, 0), ASR_ERR_ARG);
        EXPECT(asr_ctc_lm_decode_host(h, emis, 2, 1, 0, 3, nullptr, 0), ASR_ERR_ARG);
        EXPECT(asr_ctc_lm_decode_host(h, emis, 2, 1, 3, 0, nullptr, 0), ASR_ERR_ARG);
        for (int k = 0; k < 3; k++) {
            EXPECT(asr_ctc_lm_decode_host(h, emis, 2, 1, 3, 3, &len_bad[k], 0), ASR_ERR_ARG);
            EXPECT(asr_ctc_lm_decode(h, fake, 2, 1, 3, 3, &len_bad[k], 0, nullptr), ASR_ERR_ARG);
        }
        EXPECT(asr_ctc_lm_decode(nullptr, fake, 2, 1, 3, 3, nullptr, 0, nullptr), ASR_ERR_ARG);
        EXPECT(asr_ctc_lm_decode(h, nullptr, 2, 1, 3, 3, nullptr, 0, nullptr), ASR_ERR_ARG);
        EXPECT(asr_ctc_lm_decode(h, fake, 0, 1, 3, 3, nullptr, 0, nullptr), ASR_ERR_ARG);
        EXPECT(asr_ctc_lm_decode(h, fake, 2, 0, 3, 3, nullptr, 0, nullptr), ASR_ERR_ARG);
        EXPECT(asr_ctc_lm_decode(h, fake, 2, 1, 0, 3, nullptr, 0, nullptr), ASR_ERR_ARG);
        EXPECT(asr_ctc_lm_decode(h, fake, 2, 1, 3, 0, nullptr, 0, nullptr), ASR_ERR_ARG);
        EXPECT(asr_ctc_lm_decode(h, fake, 2, 1, 3, 3, nullptr, 0, nullptr), ASR_ERR_STATE);   // the LM is not uploaded
        EXPECT(asr_ctc_lm_decode_host(h, emis, 2, 1, 3, 3, nullptr, 0), ASR_OK);
        EXPECT(asr_ctc_lm_get_beams(nullptr, 1, 1, i32, i32, i32, nullptr, nullptr, nullptr, nullptr), ASR_ERR_ARG);
        EXPECT(asr_ctc_lm_get_beams(h, 0, 1, i32, i32, i32, nullptr, nullptr, nullptr, nullptr), ASR_ERR_ARG);
        EXPECT(asr_ctc_lm_get_beams(h, 1, 0, i32, i32, i32, nullptr, nullptr, nullptr, nullptr), ASR_ERR_ARG);
        EXPECT(asr_ctc_lm_get_beams(h, 1, 1, nullptr, i32, i32, nullptr, nullptr, nullptr, nullptr), ASR_ERR_ARG);
        EXPECT(asr_ctc_lm_get_beams(h, 1, 1, i32, nullptr, i32, nullptr, nullptr, nullptr, nullptr), ASR_ERR_ARG);
        EXPECT(asr_ctc_lm_get_beams(h, 1, 1, i32, i32, nullptr, nullptr, nullptr, nullptr, nullptr), ASR_ERR_ARG);
        EXPECT(asr_ctc_lm_get_beams(h, 1, 1, i32, i32 + 1, i32 + 2, nullptr, nullptr, nullptr, nullptr), ASR_OK);
        EXPECT(asr_ctc_lm_get_best(nullptr, i32, 1, i32, nullptr), ASR_ERR_ARG);
        EXPECT(asr_ctc_lm_get_best(h, nullptr, 1, i32, nullptr), ASR_ERR_ARG);
        EXPECT(asr_ctc_lm_get_best(h, i32, 0, i32, nullptr), ASR_ERR_ARG);
        EXPECT(asr_ctc_lm_get_best(h, i32, 1, nullptr, nullptr), ASR_ERR_ARG);
        EXPECT(asr_ctc_lm_get_best(h, i32, 1, i32 + 1, nullptr), ASR_OK);
        EXPECT(asr_ctc_lm_host_gaps(nullptr, &gap), ASR_ERR_ARG);
        EXPECT(asr_ctc_lm_host_gaps(h, nullptr), ASR_ERR_ARG);
        EXPECT(asr_ctc_lm_host_gaps(h, &gap), ASR_OK);
        EXPECT(asr_ctc_lm_destroy(h), ASR_OK);
    }
    EXPECT(asr_ctc_lm_destroy(nullptr), ASR_ERR_ARG);
    // ties: 39 states tie at frame 0 of uniform emissions; a capacity of 32 reports it
    {
        std::string t = "\n\\data\\\nngram 1=41\n\n\\1-grams:\n-99\t<s>\n-1\t</s>\n";
        for (int i = 0; i < 39; i++) t += "-1\tu" + std::to_string(i) + "\n";
        asr_lm_t* flat = load(t + "\n\\end\\\n");
        std::vector<int32_t> tk(40);
        for (int v = 0; v < 40; v++) tk[v] = v + 1;
        std::vector<float> emis(2 * 40, 1.0f / 40);
        asr_ctc_lm_t* g = nullptr;
        EXPECT(asr_ctc_lm_create(nullptr, 40, 2, 0, 3, flat, tk.data(), 0.5f, 0.0f, 1, 0, &g), ASR_OK);
        if (g) {
            int32_t nh = -1, len[2], lab[2];
            EXPECT(asr_ctc_lm_decode_host(g, emis.data(), 2, 1, 40, 40, nullptr, 0), ASR_OK);
            EXPECT(asr_ctc_lm_get_beams(g, 2, 1, &nh, len, lab, nullptr, nullptr, nullptr, nullptr), ASR_ERR_BEAM_OVERFLOW);
            EXPECT(nh, 0);
            asr_ctc_lm_destroy(g);
        }
        asr_lm_destroy(flat);
    }
    asr_lm_destroy(lm);
    asr_lm_destroy(bare);
}

int main() {
    worked_example();
    random_decodes();
    refusals();
    if (failures) {
        std::printf("ctc_lm_check: %d FAILED\n", failures);
        return 1;
    }
    std::printf("ctc_lm_check: ok\n");
    return 0;
}
