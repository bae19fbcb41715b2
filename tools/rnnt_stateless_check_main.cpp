// Stand-alone check of the stateless-predictor transducer's host code (make
// rnntstatelesscheck, ASan + UBSan, CPU only, no HIP call): every refusal of
// asr_rnnt_create_stateless in its documented order, the two greedy pairs on a
// handle of the wrong kind, the dual-kind entry points' refusals on a stateless
// handle, and small twin decodes: a chunked decode against the whole one, beam
// 1 against greedy with max_symbols = 1, and the align twin's score of the
// greedy tokens against the greedy total (one alignment is a lower bound).
#define RNNT_CHECK_SEED 20251
#define RNNT_CHECK_BLANK_BIAS 2.0f
#include "rnnt_check_common.h"

#include <cstring>

struct SModel {
    asr_rnnt_stateless_desc d;
    std::vector<float> emb, wctx, bctx, wenc, benc, wpred, bpred, wout, bout;
    asr_rnnt_stateless_weights ptrs(bool conv = true, bool bias = true) const {
        return asr_rnnt_stateless_weights{emb.data(),  conv ? wctx.data() : nullptr, bias ? bctx.data() : nullptr,
                                          wenc.data(), benc.data(), wpred.data(), bpred.data(), wout.data(), bout.data()};
    }
};

static SModel make_stateless(int V, int blank, int E, int D, int Hp, int J, int act, int ms, int C, int fill_tok) {
    SModel m;
    m.d = asr_rnnt_stateless_desc{V, blank, E, D, Hp, J, act, ms, C, fill_tok};
    fill(m.emb, (size_t)V * D, 1.0f);
    fill(m.wctx, (size_t)(C > 0 ? C : 1) * D * Hp, 2.0f * std::sqrt(3.0f / (D * (C > 0 ? C : 1))));
    fill(m.bctx, Hp, 0.1f);
    fill(m.wenc, (size_t)E * J, std::sqrt(3.0f / E));
    fill(m.benc, J, 0.1f);
    fill(m.wpred, (size_t)Hp * J, 4.0f * std::sqrt(3.0f / Hp));
    fill(m.bpred, J, 0.1f);
    fill(m.wout, (size_t)J * V, 4.0f * std::sqrt(3.0f / J));
    fill(m.bout, V, 0.1f);
    m.bout[blank] = RNNT_CHECK_BLANK_BIAS;
    return m;
}

static int create(const SModel& m, asr_rnnt_t** h, bool conv = true, bool bias = true) {
    const asr_rnnt_stateless_weights w = m.ptrs(conv, bias);
    return asr_rnnt_create_stateless(&m.d, &w, h);
}

int main() {
    const int V = 9, E = 8, D = 16, Hp = 16, J = 16, T = 7, B = 3, C = 2;
    SModel m = make_stateless(V, 0, E, D, Hp, J, ASR_RNNT_ACT_TANH, 3, C, -1);
    asr_rnnt_t* h = nullptr;
    const asr_rnnt_stateless_weights w = m.ptrs();

    // asr_rnnt_create_stateless, in the documented order
    EXPECT(asr_rnnt_create_stateless(nullptr, &w, &h), ASR_ERR_ARG);
    EXPECT(asr_rnnt_create_stateless(&m.d, nullptr, &h), ASR_ERR_ARG);
    EXPECT(asr_rnnt_create_stateless(&m.d, &w, nullptr), ASR_ERR_ARG);
    for (int bad = 0; bad < 6; bad++) {
        SModel x = m;
        if (bad == 0) x.d.V = 1;
        if (bad == 1) x.d.blank = V;
        if (bad == 2) x.d.max_symbols = 0;
        if (bad == 3) x.d.context = 0;
        if (bad == 4) x.d.context = ASR_RNNT_MAX_CONTEXT + 1;
        if (bad == 5) x.d.start_fill = V;
        EXPECT(create(x, &h), ASR_ERR_ARG);
        EXPECT_TRUE(h == nullptr);
    }
    {
        SModel x = m;
        x.d.Hp = 24;    // an ARG error in the ranges comes first, then the multiples of 16
        EXPECT(create(x, &h), ASR_ERR_UNSUPPORTED);
        x.d.start_fill = -2;
        EXPECT(create(x, &h), ASR_ERR_ARG);
        x = m;
        x.d.Hp = x.d.J = 1248;   // beyond the LDS limit (1232); refused before a weight is read
        EXPECT(create(x, &h), ASR_ERR_UNSUPPORTED);
        asr_rnnt_stateless_weights nw = w;
        nw.w_out = nullptr;
        EXPECT(asr_rnnt_create_stateless(&m.d, &nw, &h), ASR_ERR_ARG);
        EXPECT(create(m, &h, false), ASR_ERR_ARG);   // no W_ctx with context 2
        x = m;
        x.d.context = 1;
        x.d.Hp = 32;
        x.wpred.resize((size_t)32 * J);
        EXPECT(create(x, &h, false), ASR_ERR_ARG);   // no W_ctx with D != Hp
    }
    EXPECT(create(m, &h, true, false), ASR_OK);      // b_ctx may be NULL
    EXPECT(asr_rnnt_context(h), C);
    EXPECT(asr_rnnt_context(nullptr), 0);
    asr_rnnt_info info{};
    EXPECT(asr_rnnt_get_info(h, &info), ASR_OK);
    EXPECT(info.desc.L, 0);
    EXPECT(info.uploaded, 0);
    EXPECT_TRUE(asr_rnnt_workspace_bytes(h, T, B) == (size_t)(T * B + 32) * J * sizeof(float));
    EXPECT_TRUE(asr_rnnt_beam_workspace_bytes(h, T, B, 4) > 0 && asr_rnnt_align_workspace_bytes(h, T, B, 2, 3) > 0);

    // the wrong kind, each of the four greedy entry points
    Model lm = make_model(V, 0, E, D, Hp, 1, J, ASR_RNNT_ACT_RELU, 3);
    const asr_rnnt_weights lw = lm.ptrs();
    asr_rnnt_t* hl = nullptr;
    EXPECT(asr_rnnt_create(&lm.d, &lw, &hl), ASR_OK);
    EXPECT(asr_rnnt_context(hl), 0);
    std::vector<float> enc;
    fill(enc, (size_t)T * B * E, 1.0f);
    const int mo = T * 3;
    std::vector<int32_t> tok(B * mo), ts(B * mo), cnt(B), ctx(B * C), len = {T, 0, 5};
    std::vector<double> lp(B * mo), tot(B);
    int x = 0;
    void* dummy = &x;
    EXPECT(asr_rnnt_greedy(h, enc.data(), nullptr, T, B, mo, nullptr, nullptr, tok.data(), ts.data(), lp.data(),
                           cnt.data(), tot.data(), dummy, nullptr), ASR_ERR_UNSUPPORTED);
    EXPECT(asr_rnnt_greedy_host(h, enc.data(), nullptr, T, B, mo, nullptr, nullptr, tok.data(), ts.data(), lp.data(),
                                cnt.data(), tot.data(), nullptr), ASR_ERR_UNSUPPORTED);
    EXPECT(asr_rnnt_greedy_stateless(hl, enc.data(), nullptr, T, B, mo, nullptr, nullptr, tok.data(), ts.data(),
                                     lp.data(), cnt.data(), tot.data(), dummy, nullptr), ASR_ERR_UNSUPPORTED);
    EXPECT(asr_rnnt_greedy_stateless_host(hl, enc.data(), nullptr, T, B, mo, nullptr, nullptr, tok.data(), ts.data(),
                                          lp.data(), cnt.data(), tot.data(), nullptr), ASR_ERR_UNSUPPORTED);
    // asr_rnnt_greedy's checks come first, then the state of the handle
    EXPECT(asr_rnnt_greedy_stateless(h, nullptr, nullptr, T, B, mo, nullptr, nullptr, tok.data(), ts.data(), lp.data(),
                                     cnt.data(), tot.data(), dummy, nullptr), ASR_ERR_ARG);
    EXPECT(asr_rnnt_greedy_stateless(h, enc.data(), nullptr, T, B, mo, nullptr, nullptr, tok.data(), ts.data(),
                                     lp.data(), cnt.data(), tot.data(), nullptr, nullptr), ASR_ERR_ARG);
    EXPECT(asr_rnnt_greedy_stateless(h, enc.data(), nullptr, T, B, mo, nullptr, nullptr, tok.data(), ts.data(),
                                     lp.data(), cnt.data(), tot.data(), dummy, nullptr), ASR_ERR_STATE);
    // the dual-kind device entry points on a handle that was not uploaded
    std::vector<int32_t> blen(B * 4), nh(B);
    std::vector<double> bsc(B * 4);
    EXPECT(asr_rnnt_beam(h, enc.data(), nullptr, T, B, 4, 4, T, tok.data(), ts.data(), blen.data(), bsc.data(),
                         nh.data(), dummy, nullptr), ASR_ERR_STATE);
    EXPECT(asr_rnnt_beam(h, enc.data(), nullptr, T, B, 17, 4, T, tok.data(), ts.data(), blen.data(), bsc.data(),
                         nh.data(), dummy, nullptr), ASR_ERR_ARG);

    // whole against chunked (ctx_out -> ctx_in, in place), out-of-range entries clamped
    std::vector<int32_t> tok2(B * mo), ts2(B * mo), cnt2(B), cnt3(B);
    std::vector<double> lp2(B * mo), tot2(B), tot3(B);
    EXPECT(asr_rnnt_greedy_stateless_host(h, enc.data(), len.data(), T, B, mo, nullptr, ctx.data(), tok.data(), ts.data(),
                                          lp.data(), cnt.data(), tot.data(), nullptr), ASR_OK);
    std::vector<int32_t> l1 = {3, 0, 3}, l2 = {T - 3, 0, 2}, c2(B * C);
    EXPECT(asr_rnnt_greedy_stateless_host(h, enc.data(), l1.data(), 3, B, mo, nullptr, c2.data(), tok2.data(), ts2.data(),
                                          lp2.data(), cnt2.data(), tot2.data(), nullptr), ASR_OK);
    std::vector<int32_t> tok3(B * mo), ts3(B * mo);
    std::vector<double> lp3(B * mo);
    EXPECT(asr_rnnt_greedy_stateless_host(h, enc.data() + (size_t)3 * B * E, l2.data(), T - 3, B, mo, c2.data(), c2.data(),
                                          tok3.data(), ts3.data(), lp3.data(), cnt3.data(), tot3.data(), nullptr), ASR_OK);
    EXPECT_TRUE(c2 == ctx);
    int emitted = 0;
    for (int b = 0; b < B; b++) {
        EXPECT(cnt2[b] + cnt3[b], cnt[b]);
        emitted += cnt[b];
        for (int i = 0; i < cnt[b]; i++) {
            const bool first = i < cnt2[b];
            const int j = first ? i : i - cnt2[b];
            EXPECT((first ? tok2 : tok3)[b * mo + j], tok[b * mo + i]);
            EXPECT((first ? ts2[b * mo + j] : ts3[b * mo + j] + 3), ts[b * mo + i]);
            EXPECT_TRUE((first ? lp2 : lp3)[b * mo + j] == lp[b * mo + i]);
        }
    }
    EXPECT_TRUE(emitted > 0);
    std::vector<int32_t> wild = {-7, V + 3, 0, 0, 0, 0}, clamped = {-1, V - 1, 0, 0, 0, 0}, zero = {0, 0, 0};
    EXPECT(asr_rnnt_greedy_stateless_host(h, enc.data(), zero.data(), T, B, 0, wild.data(), wild.data(), nullptr, nullptr,
                                          nullptr, cnt2.data(), tot2.data(), nullptr), ASR_OK);
    EXPECT_TRUE(wild == clamped);

    // beam 1 is greedy with one symbol per frame; the align twin's score bounds the greedy total from above
    asr_rnnt_destroy(h);
    m.d.max_symbols = 1;
    EXPECT(create(m, &h), ASR_OK);
    EXPECT(asr_rnnt_greedy_stateless_host(h, enc.data(), len.data(), T, B, T, nullptr, nullptr, tok.data(), ts.data(),
                                          lp.data(), cnt.data(), tot.data(), nullptr), ASR_OK);
    std::vector<int32_t> btok(B * T), bts(B * T), bl(B), bn(B);
    std::vector<double> bs(B), sc(B);
    EXPECT(asr_rnnt_beam_host(h, enc.data(), len.data(), T, B, 1, 1, T, btok.data(), bts.data(), bl.data(), bs.data(),
                              bn.data(), nullptr), ASR_OK);
    EXPECT(asr_rnnt_align_host(h, enc.data(), len.data(), T, B, tok.data(), T, cnt.data(), nullptr, B, T,
                               ASR_RNNT_LATTICE_ONE_PER_FRAME, sc.data(), nullptr, nullptr), ASR_OK);
    for (int b = 0; b < B; b++) {
        EXPECT(bl[b], cnt[b]);
        EXPECT_TRUE(close(bs[b], tot[b]));
        EXPECT_TRUE(sc[b] >= tot[b] - 1e-9);
        for (int i = 0; i < cnt[b]; i++) {
            EXPECT(btok[b * T + i], tok[b * T + i]);
            EXPECT(bts[b * T + i], ts[b * T + i]);
        }
    }
    asr_rnnt_destroy(h);
    asr_rnnt_destroy(hl);
    if (failures) {
        std::printf("rnnt_stateless_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("rnnt_stateless_check: ok\n");
    return 0;
}
