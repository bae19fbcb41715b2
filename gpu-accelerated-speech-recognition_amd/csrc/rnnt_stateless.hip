// Transducers with a stateless predictor (Ghodsi et al.; the k2 / icefall
// pruned_transducer_stateless* and Zipformer recipes): asr_rnnt_create_stateless
// / asr_rnnt_context / asr_rnnt_greedy_stateless / asr_rnnt_greedy_stateless_host,
// the table upload behind asr_rnnt_upload and the producer of asr_rnnt_align's p.
//
// Model (weights in the project's [in][out] layout; include/asr_amd.h has the
// definition):
//   p = relu(T_0[y_0] + ... + T_{C-1}[y_{C-1}] + b_ctx),  T_c = Emb.W_ctx[c],
//   g = p.W_pred + b_pred, then rnnt.hip's joint.
// (y_0 .. y_{C-1}) are the last C tokens, oldest first; -1 adds nothing.
//
// Device form.  The C tables T_c [V][Hp] are C gemm_launch calls at upload (the
// move asr_rnnt_upload makes for Emb.W_ih), so a predictor step has no product:
// C row gathers from L2, adds and a ReLU into LDS (rt_ctx_gather), no MFMA
// chain, no per-layer barrier.  The greedy walk keeps rnnt.hip's ownership: a
// workgroup of 8 waves owns 16 NRT utterances (NRT row tiles of a
// v_mfma_f32_16x16x4_f32), column tile j belongs to wave j % 8, the weights
// stream from L2 through rt_mma's register ring and every W fragment feeds NRT
// MFMAs; the row reduction joins in the fixed order.  LDS holds p [16 NRT][Hp +
// 4], z [16 NRT][J + 4] and the small area with the contexts; g [16 NRT][J + 4]
// sits in LDS behind z where the model leaves room for it (GL, measured 10 %
// faster), else in the workgroup's slice of the workspace; either way only the
// lane that wrote an element reads it, and the bits are the same.  Per
// iteration: the rows that emitted shifted their context (the row's own thread,
// when it decided) and all 512 threads gather their p again; rows that did not
// emit keep p untouched; g for every row; then the joint at each row's own t
// and one thread per row advances its walk.  A row's bits depend on the model's
// shape only (rows of an MFMA are independent; p is a function of the context).
#include "rnnt_common.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <new>
#include <vector>

// Row tiles per workgroup of the greedy kernel: 2 is the form that was measured against the shipped one
// (the Makefile's RNNTCTXFLAGS builds it).
#ifndef ASR_RNNT_CTX_NRT
#define ASR_RNNT_CTX_NRT 1
#endif

namespace asr {

struct CtxArgs {
    const float* f;          // [T*B][J]
    RtNet net;
    const int32_t* lengths;
    const int32_t* ctx_in;   // [B][C] or NULL
    int32_t* ctx_out;        // the same, or NULL
    int32_t* tokens;
    int32_t* timesteps;
    double* logp;
    int32_t* count;
    double* total;
    float* slices;           // per workgroup: g [16 NRT][J]
    int T, B, max_symbols, max_out, max_iters;
};

template <int NRT, bool GL>
__global__ __launch_bounds__(64 * RT_WAVES) void rnnt_greedy_ctx_kernel(const CtxArgs a) {
    extern __shared__ __attribute__((aligned(16))) float rc_lds[];
    constexpr int R = RT_ROWS * NRT;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    const RtNet& net = a.net;
    const int Hp = net.Hp, J = net.J, V = net.V, B = a.B, C = net.C;
    const int LDH = Hp + 4, LDJ = J + 4;
    const int r0 = blockIdx.x * R;
    // LDS: p [R][LDH], z [R][LDJ], then the small area (NRT * RT_LDS_SMALL bytes)
    float* const pbuf = rc_lds;
    float* const zbuf = pbuf + (size_t)R * LDH;
    float* const glds = zbuf + (size_t)R * LDJ;                                 // g [R][LDJ], with GL only
    float* const small = glds + (GL ? (size_t)R * LDJ : 0);
    double* const row_total = reinterpret_cast<double*>(small);                 // [R]
    float* const red_m = small + 2 * R;                                         // [8][R]
    float* const red_s = red_m + RT_WAVES * R;
    int* const red_i = reinterpret_cast<int*>(red_s + RT_WAVES * R);
    int* const row_t = red_i + RT_WAVES * R;                                    // [R] each
    int* const row_n = row_t + R;
    int* const row_len = row_n + R;
    int* const row_emit = row_len + R;
    int* const row_cnt = row_emit + R;
    int* const row_live = row_cnt + R;
    int* const ctx = row_live + R;                                              // [R][RT_CTX]
    // this workgroup's slice: g [R][J], each element touched by its owner lane only
    float* const gw = GL ? glds : a.slices + (size_t)blockIdx.x * R * J;
    const int ldg = GL ? LDJ : J;

    if (tid < R) {
        const int r = r0 + tid;
        const int len = r < B ? (a.lengths ? min(max(a.lengths[r], 0), a.T) : a.T) : 0;
        row_len[tid] = len;
        row_t[tid] = 0;
        row_n[tid] = 0;
        row_cnt[tid] = 0;
        row_total[tid] = 0.0;
        row_emit[tid] = 1;   // the first p of every row
        row_live[tid] = len > 0;
        for (int i = 0; i < C; i++)   // a given entry outside [-1, V) is clamped into it
            ctx[tid * RT_CTX + i] = (a.ctx_in && r < B) ? min(max(a.ctx_in[(size_t)r * C + i], -1), V - 1)
                                                        : rt_ctx_start(C, i, net.start_fill, net.blank);
    }
    __syncthreads();

    for (int it = 0;; it++) {
        int any_emit = 0, any_live = 0;
#pragma unroll
        for (int x = 0; x < R; x++) {
            any_emit |= row_emit[x];
            any_live |= row_live[x];
        }
        if (any_emit) {
            // p of the rows whose context changed, then g = p.W_pred + b_pred (for every row: a row that kept
            // its p gets its g again)
            rt_ctx_gather(net, pbuf, ctx, R, [&](int row) { return row_emit[row] != 0; }, tid);
            __syncthreads();
            rt_sweep<NRT, false>(pbuf + c * LDH + 4 * g, RT_ROWS * LDH, Hp >> 4, net.wpred, net.bpred, J, w, g, c,
                                 [&](int rt, int n, f32x4 x) {
#pragma unroll
                                     for (int j = 0; j < 4; j++)
                                         gw[(size_t)(RT_ROWS * rt + 4 * g + j) * ldg + n] = x[j];
                                 });
        }
        if (!any_live || it >= a.max_iters) break;

        // z = act(f_t + g): the lane that owns g's element, each row at its own t
#pragma unroll
        for (int rt = 0; rt < NRT; rt++)
            for (int jt = w; jt < (J >> 4); jt += RT_WAVES) {
                const int n = 16 * jt + c;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int row = RT_ROWS * rt + 4 * g + j;
                    const int rr = min(r0 + row, B - 1), tt = min(row_t[row], a.T - 1);
                    const float x = a.f[((size_t)tt * B + rr) * J + n] + gw[(size_t)row * ldg + n];
                    zbuf[row * LDJ + n] = rt_act(x, net.act);
                }
            }
        __syncthreads();

        // logit = z.W_out + b_out over the V column tiles; columns >= V do not exist
        RtTop top[NRT][4];
#pragma unroll
        for (int rt = 0; rt < NRT; rt++)
#pragma unroll
            for (int j = 0; j < 4; j++) top[rt][j] = RtTop{-INFINITY, 0.f, RT_NONE};
        rt_sweep<NRT, true>(zbuf + c * LDJ + 4 * g, RT_ROWS * LDJ, J >> 4, net.wout, net.bout, V, w, g, c,
                            [&](int rt, int n, f32x4 x) {
#pragma unroll
                                for (int j = 0; j < 4; j++) rt_push(top[rt][j], x[j], n);
                            });
        // the 16 lanes of a row, then the waves in the order 0..7
#pragma unroll
        for (int rt = 0; rt < NRT; rt++)
#pragma unroll
            for (int j = 0; j < 4; j++)
                rt_row_partial<true>(top[rt][j], c, w * R + RT_ROWS * rt + 4 * g + j, red_m, red_s, red_i);
        __syncthreads();
        if (tid < R) {
            const int row = tid, r = r0 + row;
            int t = row_t[row], n = row_n[row], em = 0;
            const int len = row_len[row];
            if (t < len) {
                const RtTop b = rt_row_total<true>(row, R, red_m, red_s, red_i);
                const int k = b.i == RT_NONE ? 0 : b.i;
                const float lp = -logf(b.s);   // logit[k] - logsumexp(logit), logit[k] the maximum
                row_total[row] += (double)lp;
                if (k != net.blank) {
                    const int cnt = row_cnt[row];
                    if (cnt < a.max_out) {
                        const size_t o = (size_t)r * a.max_out + cnt;
                        a.tokens[o] = k;
                        a.timesteps[o] = t;
                        a.logp[o] = (double)lp;
                    }
                    row_cnt[row] = cnt + 1;
                    for (int i = 0; i + 1 < C; i++) ctx[row * RT_CTX + i] = ctx[row * RT_CTX + i + 1];
                    ctx[row * RT_CTX + C - 1] = k;
                    em = 1;
                    if (++n == a.max_symbols) {
                        t++;
                        n = 0;
                    }
                } else {
                    t++;
                    n = 0;
                }
                row_t[row] = t;
                row_n[row] = n;
            }
            row_emit[row] = em;
            row_live[row] = t < len;
        }
        __syncthreads();
    }

    if (tid < R && r0 + tid < B) {
        a.count[r0 + tid] = row_cnt[tid];
        a.total[r0 + tid] = row_total[tid];
        if (a.ctx_out)
            for (int i = 0; i < C; i++) a.ctx_out[(size_t)(r0 + tid) * C + i] = ctx[tid * RT_CTX + i];
    }
}

// asr_rnnt_align's p for a stateless handle: one workgroup per target, a float4
// of a row per thread.  Position u takes the last C of start-context + y[:u];
// positions past the target's length repeat the last one, and a label outside
// [0, V) is clamped (such a target is infeasible and its rows are never read).
struct CtxRowsArgs {
    RtNet net;
    const int32_t* targets;
    long ldt;
    const int32_t* target_lengths;
    float* p;   // [(mtl+1)*N][Hp]
    int N, mtl;
};
__global__ __launch_bounds__(256) void rnnt_ctx_rows_kernel(const CtxRowsArgs a) {
    const int n = blockIdx.x, tid = threadIdx.x;
    const RtNet& net = a.net;
    const int Hp = net.Hp, q4 = Hp >> 2, C = net.C;
    const int U = min(max(a.target_lengths[n], 0), a.mtl);
    const int32_t* tgt = a.targets + (long)n * a.ldt;
    for (int x = tid; x < (a.mtl + 1) * q4; x += 256) {
        const int u = x / q4, k = x - u * q4, uu = min(u, U);
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int i = 0; i < C; i++) {
            const int j = uu + i;   // entry i of the context: element j of start-context + y
            const int y = j < C ? rt_ctx_start(C, j, net.start_fill, net.blank) : min(max(tgt[j - C], 0), net.V - 1);
            if (y < 0) continue;
            const float4 t = reinterpret_cast<const float4*>(net.tab + ((size_t)i * net.V + y) * Hp)[k];
            s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
        }
        const float4 b = reinterpret_cast<const float4*>(net.bih[0])[k];
        s.x = fmaxf(s.x + b.x, 0.f); s.y = fmaxf(s.y + b.y, 0.f);
        s.z = fmaxf(s.z + b.z, 0.f); s.w = fmaxf(s.w + b.w, 0.f);
        reinterpret_cast<float4*>(a.p + ((size_t)u * a.N + n) * Hp)[k] = s;
    }
}

int rnnt_ctx_align_rows(const asr_rnnt* h, const int32_t* d_targets, long ldt, const int32_t* d_target_lengths, int N,
                        int mtl, float* d_p, hipStream_t st) {
    CtxRowsArgs a{};
    a.net = rnnt_net(h);
    a.targets = d_targets; a.ldt = ldt; a.target_lengths = d_target_lengths; a.p = d_p; a.N = N; a.mtl = mtl;
    hipLaunchKernelGGL(rnnt_ctx_rows_kernel, dim3((unsigned)N), dim3(256), 0, st, a);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

// The weights to the device, one allocation: the tables [C][V][Hp] first, computed there by gemm_launch.
int rnnt_ctx_upload(asr_rnnt* h) {
    const asr_rnnt_desc& d = h->d;
    struct Piece {
        const std::vector<float>* v;
        const float** dst;
    };
    const float *d_emb = nullptr, *d_wctx = nullptr;
    const Piece pieces[] = {{&h->emb, &d_emb},        {&h->wctx, &d_wctx},      {&h->bctx, &h->d_bctx},
                            {&h->wenc, &h->d_wenc},   {&h->benc, &h->d_benc},   {&h->wpred, &h->d_wpred},
                            {&h->bpred, &h->d_bpred}, {&h->wout, &h->d_wout},   {&h->bout, &h->d_bout}};
    auto up4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
    const size_t tab = (size_t)d.V * d.Hp;   // one table: a multiple of 4 floats
    size_t total = h->C * tab;
    for (const Piece& pc : pieces) total += up4(pc.v->size());
    float* blob = nullptr;
    ASR_HIP_TRY(hipMalloc((void**)&blob, total * sizeof(float)));
    size_t off = h->C * tab;
    hipError_t e = hipSuccess;
    for (const Piece& pc : pieces) {
        *pc.dst = blob + off;
        if (e == hipSuccess && !pc.v->empty())
            e = hipMemcpy(blob + off, pc.v->data(), pc.v->size() * sizeof(float), hipMemcpyHostToDevice);
        off += up4(pc.v->size());
    }
    if (e == hipSuccess && !h->conv)   // C = 1 without a conv: T_0 = Emb (D = Hp)
        e = hipMemcpy(blob, h->emb.data(), tab * sizeof(float), hipMemcpyHostToDevice);
    int rc = ASR_OK;
    if (e != hipSuccess) {
        asr_internal_set_error("hipMemcpy (RNN-T weights)", hipGetErrorString(e), __FILE__, __LINE__);
        rc = ASR_ERR_HIP;
    }
    for (int i = 0; rc == ASR_OK && h->conv && i < h->C; i++) {
        GemmArgs g{};   // T_i = Emb.W_ctx[i]
        g.A = d_emb; g.B = d_wctx + (size_t)i * d.D * d.Hp; g.C = blob + i * tab;
        g.M = d.V; g.N = d.Hp; g.K = d.D;
        g.sam = d.D; g.sak = 1; g.sbk = d.Hp; g.sbn = 1; g.ldc = d.Hp;
        rc = gemm_launch(g, EPI_NONE, nullptr);
    }
    if (rc == ASR_OK && (e = hipStreamSynchronize(nullptr)) != hipSuccess) {
        asr_internal_set_error("hipStreamSynchronize (RNN-T upload)", hipGetErrorString(e), __FILE__, __LINE__);
        rc = ASR_ERR_HIP;
    }
    if (rc != ASR_OK) {
        (void)hipFree(blob);
        return rc;
    }
    h->d_tab = blob;
    h->d_blob = blob;
    return ASR_OK;
}

// The checks the device and the host decode share, before any HIP call (asr_rnnt_greedy's, then the kind).
static int rnnt_ctx_greedy_check(const asr_rnnt* h, const void* enc, int T, int B, int max_out, const void* tokens,
                                 const void* timesteps, const void* logp, const void* count, const void* total) {
    if (!h || !enc || !count || !total || T <= 0 || B <= 0 || max_out < 0) return ASR_ERR_ARG;
    if (max_out > 0 && (!tokens || !timesteps || !logp)) return ASR_ERR_ARG;
    if ((long)T * B > INT_MAX || (long)T * (h->d.max_symbols + 1) >= INT_MAX) return ASR_ERR_UNSUPPORTED;
    if (!h->C) return ASR_ERR_UNSUPPORTED;   // an LSTM handle
    return ASR_OK;
}

// g [16][J + 4] in LDS
static long rnnt_ctx_g_bytes(int J) { return (long)RT_ROWS * (J + 4) * 4; }

template <int NRT, bool GL>
static int rnnt_ctx_greedy_launch(const asr_rnnt* h, CtxArgs& a, hipStream_t st) {
    static AsrAttrOnce attr;
    if (int rc = attr.set((const void*)rnnt_greedy_ctx_kernel<NRT, GL>, RT_LDS_MAX)) return rc;
    const unsigned gx = (unsigned)((a.B + RT_ROWS * NRT - 1) / (RT_ROWS * NRT));
    const long lds = NRT * (rnnt_ctx_lds_bytes(h->d.Hp, h->d.J, RT_LDS_SMALL) + (GL ? rnnt_ctx_g_bytes(h->d.J) : 0));
    hipLaunchKernelGGL((rnnt_greedy_ctx_kernel<NRT, GL>), dim3(gx), dim3(64 * RT_WAVES), (size_t)lds, st, a);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

}  // namespace asr

extern "C" {

int asr_rnnt_create_stateless(const asr_rnnt_stateless_desc* desc, const asr_rnnt_stateless_weights* wt,
                              asr_rnnt_t** out) {
    if (out) *out = nullptr;
    if (!desc || !wt || !out) return ASR_ERR_ARG;
    const asr_rnnt_stateless_desc& d = *desc;
    if (d.V < 2 || d.blank < 0 || d.blank >= d.V || d.E <= 0 || d.D <= 0 || d.Hp <= 0 || d.J <= 0 ||
        d.max_symbols < 1 || (d.act != ASR_RNNT_ACT_RELU && d.act != ASR_RNNT_ACT_TANH) || d.context < 1 ||
        d.context > ASR_RNNT_MAX_CONTEXT || d.start_fill < -1 || d.start_fill >= d.V)
        return ASR_ERR_ARG;
    if ((d.D & 15) || (d.Hp & 15) || (d.J & 15)) return ASR_ERR_UNSUPPORTED;
    if (asr::rnnt_ctx_lds_bytes(d.Hp, d.J, asr::RT_LDS_SMALL) > asr::RT_LDS_MAX) return ASR_ERR_UNSUPPORTED;
    if ((long)d.context * d.V * d.Hp > INT_MAX || (long)d.V * d.J > INT_MAX || (long)d.V * d.D > INT_MAX ||
        (long)d.E * d.J > INT_MAX)
        return ASR_ERR_UNSUPPORTED;
    if (!wt->emb || !wt->w_enc || !wt->b_enc || !wt->w_pred || !wt->b_pred || !wt->w_out || !wt->b_out)
        return ASR_ERR_ARG;
    if (!wt->w_ctx && d.context != 1) return ASR_ERR_ARG;        // only C = 1 has a form without a conv
    if (!wt->w_ctx && d.D != d.Hp) return ASR_ERR_ARG;           // T_0 = Emb needs D = Hp
    asr_rnnt* h = new (std::nothrow) asr_rnnt;
    if (!h) return ASR_ERR_OOM;
    try {
        h->d = asr_rnnt_desc{d.V, d.blank, d.E, d.D, d.Hp, 0, d.J, d.act, d.max_symbols};
        h->C = d.context;
        h->start_fill = d.start_fill;
        h->conv = wt->w_ctx != nullptr;
        h->emb.assign(wt->emb, wt->emb + (size_t)d.V * d.D);
        if (h->conv) h->wctx.assign(wt->w_ctx, wt->w_ctx + (size_t)d.context * d.D * d.Hp);
        if (wt->b_ctx) h->bctx.assign(wt->b_ctx, wt->b_ctx + d.Hp);
        else h->bctx.assign(d.Hp, 0.f);
        h->wenc.assign(wt->w_enc, wt->w_enc + (size_t)d.E * d.J);
        h->benc.assign(wt->b_enc, wt->b_enc + d.J);
        h->wpred.assign(wt->w_pred, wt->w_pred + (size_t)d.Hp * d.J);
        h->bpred.assign(wt->b_pred, wt->b_pred + d.J);
        h->wout.assign(wt->w_out, wt->w_out + (size_t)d.J * d.V);
        h->bout.assign(wt->b_out, wt->b_out + d.V);
    } catch (const std::bad_alloc&) {
        delete h;
        return ASR_ERR_OOM;
    }
    h->lds_bytes = (int)asr::rnnt_ctx_lds_bytes(d.Hp, d.J, asr::RT_LDS_SMALL);
    h->weight_bytes = (int64_t)((h->emb.size() + h->wctx.size() + h->bctx.size() + h->wenc.size() + h->benc.size() +
                                 h->wpred.size() + h->bpred.size() + h->wout.size() + h->bout.size()) * sizeof(float));
    *out = h;
    return ASR_OK;
}

int asr_rnnt_context(const asr_rnnt_t* h) { return h ? h->C : 0; }

int asr_rnnt_greedy_stateless(const asr_rnnt_t* h, const float* d_enc, const int32_t* d_lengths, int T, int B,
                              int max_out, const int32_t* d_ctx_in, int32_t* d_ctx_out, int32_t* d_tokens,
                              int32_t* d_timesteps, double* d_logp, int32_t* d_count, double* d_total, void* d_work,
                              asr_stream_t s) {
    if (int rc = asr::rnnt_ctx_greedy_check(h, d_enc, T, B, max_out, d_tokens, d_timesteps, d_logp, d_count, d_total))
        return rc;
    if (!d_work) return ASR_ERR_ARG;
    if (!h->d_blob) return ASR_ERR_STATE;
    const asr_rnnt_desc& d = h->d;
    float* f = (float*)d_work;
    if (int rc = asr::rnnt_enc_launch(h, d_enc, T, B, f, asr_stream(s))) return rc;
    asr::CtxArgs a{};
    a.f = f;
    a.net = asr::rnnt_net(h);
    a.lengths = d_lengths; a.ctx_in = d_ctx_in; a.ctx_out = d_ctx_out;
    a.tokens = d_tokens; a.timesteps = d_timesteps; a.logp = d_logp; a.count = d_count; a.total = d_total;
    a.slices = f + (size_t)T * B * d.J;
    a.T = T; a.B = B; a.max_symbols = d.max_symbols; a.max_out = max_out;
    a.max_iters = T * (d.max_symbols + 1);   // the hard bound on joint evaluations per row
    const long lds = asr::rnnt_ctx_lds_bytes(d.Hp, d.J, asr::RT_LDS_SMALL), gl = asr::rnnt_ctx_g_bytes(d.J);
    if (ASR_RNNT_CTX_NRT == 2 && 2 * lds <= asr::RT_LDS_MAX)   // the timing variant
        return asr::rnnt_ctx_greedy_launch<ASR_RNNT_CTX_NRT, false>(h, a, asr_stream(s));
    if (lds + gl <= asr::RT_LDS_MAX) return asr::rnnt_ctx_greedy_launch<1, true>(h, a, asr_stream(s));
    return asr::rnnt_ctx_greedy_launch<1, false>(h, a, asr_stream(s));   // no room: g in the workspace slice
}

int asr_rnnt_greedy_stateless_host(const asr_rnnt_t* h, const float* h_enc, const int32_t* h_lengths, int T, int B,
                                   int max_out, const int32_t* h_ctx_in, int32_t* h_ctx_out, int32_t* h_tokens,
                                   int32_t* h_timesteps, double* h_logp, int32_t* h_count, double* h_total,
                                   double* h_gap) {
    if (int rc = asr::rnnt_ctx_greedy_check(h, h_enc, T, B, max_out, h_tokens, h_timesteps, h_logp, h_count, h_total))
        return rc;
    const asr_rnnt_desc& d = h->d;
    const int C = h->C;
    try {
        asr::RnntHost m(*h);
        std::vector<double> ps(d.Hp), cs(C), logit(d.V);
        for (int b = 0; b < B; b++) {
            if (h_ctx_in) {
                for (int i = 0; i < C; i++)
                    cs[i] = (double)std::min(std::max(h_ctx_in[(size_t)b * C + i], -1), d.V - 1);
                m.ctx_pred(cs.data(), ps.data());
            } else {
                m.start(ps.data(), cs.data());
            }
            m.pred_proj(ps.data());
            const int len = h_lengths ? std::min(std::max(h_lengths[b], 0), T) : T;
            int t = 0, n = 0, cnt = 0, tf = -1;
            const long max_iters = (long)T * (d.max_symbols + 1);
            double total = 0.0, gap = HUGE_VAL;
            for (long it = 0; it < max_iters && t < len; it++) {
                if (tf != t) {
                    m.enc_proj(h_enc + ((size_t)t * B + b) * d.E);
                    tf = t;
                }
                m.logits(m.g.data(), logit.data());
                int k = -1;
                double best = -HUGE_VAL, second = -HUGE_VAL;
                for (int v = 0; v < d.V; v++) {
                    const double x = logit[v];
                    if (x != x) continue;   // a NaN never wins
                    if (k < 0 || x > best) {
                        if (k >= 0) second = best;
                        best = x;
                        k = v;
                    } else if (x > second) {
                        second = x;   // an equal maximum: the lower index keeps it, the gap is 0
                    }
                }
                if (k < 0) k = 0;   // every logit a NaN
                double se = 0.0;
                for (int v = 0; v < d.V; v++) se += std::exp(logit[v] - best);
                const double lp = -std::log(se);
                if (best - second < gap) gap = best - second;
                total += lp;
                if (k != d.blank) {
                    if (cnt < max_out) {
                        const size_t o = (size_t)b * max_out + cnt;
                        h_tokens[o] = k;
                        h_timesteps[o] = t;
                        h_logp[o] = lp;
                    }
                    cnt++;
                    m.step(k, ps.data(), cs.data());
                    m.pred_proj(ps.data());
                    if (++n == d.max_symbols) {
                        t++;
                        n = 0;
                    }
                } else {
                    t++;
                    n = 0;
                }
            }
            h_count[b] = cnt;
            h_total[b] = total;
            if (h_gap) h_gap[b] = gap;
            if (h_ctx_out)
                for (int i = 0; i < C; i++) h_ctx_out[(size_t)b * C + i] = (int32_t)cs[i];
        }
    } catch (const std::bad_alloc&) {
        return ASR_ERR_OOM;
    }
    return ASR_OK;
}

}  // extern "C"
