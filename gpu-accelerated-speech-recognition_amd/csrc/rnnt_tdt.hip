// Token-and-duration transducer (TDT; Xu et al. 2023, NeMo's *-tdt models)
// greedy decoding: asr_rnnt_create_tdt / asr_rnnt_tdt_durations /
// asr_rnnt_greedy_tdt / asr_rnnt_greedy_tdt_host.
//
// Model: rnnt.hip's LSTM-predictor transducer plus a duration head on the same
// z: dlogit = z.W_dur + b_dur over D <= 16 columns, and a table durations[D].
// One evaluation gives k = argmax logit, d = argmax dlogit (each the lowest
// index among equal maxima, a NaN never wins) and
//   logp = (logit[k] - logsumexp(logit)) + (dlogit[d] - logsumexp(dlogit)),
// two separate softmaxes.  Walk of utterance b: t = skip_in[b], n = 0; while
// t < len_b: evaluate, dur = durations[d]; k == blank: logp to the total only,
// t += max(dur, 1), n = 0; else record (k, t, dur, logp), step the predictor on
// Emb[k], n += 1, then dur > 0: t += dur, n = 0; else n == max_symbols: t += 1,
// n = 0.  skip_out[b] = t - len_b: frames of the next chunk already consumed.
//
// Device form.  The handle keeps W_out and W_dur side by side, one [J][V + D]
// matrix (and one bias), so the duration head rides the W_out stream: its
// columns V .. V + D - 1 are more columns of the tiles rnnt_greedy_kernel's
// waves sweep already (tile j belongs to wave j % 8), z is read once and W_dur
// has no pass of its own.  The frame is rnnt_greedy_kernel's: a workgroup of 8
// waves owns 16 utterances, the rows of a v_mfma_f32_16x16x4_f32 tile; h and z
// in LDS, c and g in the workgroup's slice of the workspace, each element with
// its owner lane; f for all T one gemm_launch.  The column sweep has two
// pieces.  The V >> 4 tiles that hold token columns only are swept as the
// plain kernel sweeps them, into the one running (max, argmax, sum-exp) per
// row.  The at most two tiles that hold a duration column (D <= 16) come in a
// tail piece, one tile per wave at the most: a lane whose column n < V pushes
// to the token top, a lane with V <= n < V + D to a duration top that is live
// in that piece only and is joined and stored before the token top's join, so
// the two tops never double the registers of the four-tile product.  Both tops
// take the same joins: the 16 lanes of a row by the symmetric xor-shuffle
// join, then the 8 waves through LDS in the order 0..7; a wave without a
// duration column contributes the empty top.  A row's bits depend on the
// model's shape (V, D, J, Hp, L) only.  One thread per row then applies the
// walk rule, adds both -log(sum) terms to the row's total in double and writes
// the record.  row_t may pass len (a jump past the end); the f row address is
// clamped to T - 1 and such a row evaluates nothing more.
//
// Iteration bound (a kernel argument, max_iters = T * max_symbols).  Every
// evaluation of a live row either advances t by at least 1 (a blank; a token
// with dur > 0; a token that brings n to max_symbols) or leaves t and raises n,
// which is 0 after every advance: between two advances a row evaluates at most
// max_symbols times, the last of them advancing.  A row advances at most
// len - skip_in <= T times before t >= len, so it evaluates at most
// T * max_symbols times, whatever the weights and the table hold.
//
// No workgroup reads what another writes, and none waits on another.
#include "rnnt_common.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <new>
#include <vector>

namespace asr {

constexpr int TDT_MAX_D = ASR_RNNT_TDT_MAX_DURATIONS;

struct TdtArgs {
    const float* f;          // [T*B][J]
    RtNet net;               // wout [J][V + nd], bout [V + nd]
    const int32_t* lengths;
    const float* state_in;   // [2][L][B][Hp] or NULL
    float* state_out;        // the same, or NULL
    const int32_t* skip_in;  // [B] or NULL
    int32_t* skip_out;       // [B] or NULL (may be skip_in)
    int32_t* tokens;
    int32_t* timesteps;
    int32_t* durations;
    double* logp;
    int32_t* count;
    double* total;
    float* slices;           // per workgroup: c [L][16][Hp], g [16][J]
    int T, B, nd, max_symbols, max_out, max_iters;
    short dur[TDT_MAX_D];
};

__global__ __launch_bounds__(64 * RT_WAVES) void rnnt_tdt_kernel(const TdtArgs p) {
    extern __shared__ __attribute__((aligned(16))) float td_lds[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    const RtNet& net = p.net;
    const int Hp = net.Hp, J = net.J, V = net.V, L = net.L, B = p.B;
    const int LDH = Hp + 4, LDJ = J + 4;
    const int W = V + p.nd;                       // columns of the one output matrix
    const int ntp = V >> 4, nt = (W + 15) >> 4;   // token-only tiles; all tiles
    const int r0 = blockIdx.x * RT_ROWS;
    // LDS: h [2][L][16][LDH], z [16][LDJ], then the small area (3712 of RT_LDS_SMALL bytes)
    float* const hbuf = td_lds;
    float* const zbuf = hbuf + (size_t)2 * L * RT_ROWS * LDH;
    float* const small = zbuf + (size_t)RT_ROWS * LDJ;
    double* const row_total = reinterpret_cast<double*>(small);                 // [16]
    float* const red_m = small + 2 * RT_ROWS;                                   // [8][16], the token top
    float* const red_s = red_m + RT_WAVES * RT_ROWS;
    int* const red_i = reinterpret_cast<int*>(red_s + RT_WAVES * RT_ROWS);
    float* const dred_m = reinterpret_cast<float*>(red_i + RT_WAVES * RT_ROWS); // [8][16], the duration top
    float* const dred_s = dred_m + RT_WAVES * RT_ROWS;
    int* const dred_i = reinterpret_cast<int*>(dred_s + RT_WAVES * RT_ROWS);
    int* const row_t = dred_i + RT_WAVES * RT_ROWS;                             // [16] each
    int* const row_n = row_t + RT_ROWS;
    int* const row_len = row_n + RT_ROWS;
    int* const row_tok = row_len + RT_ROWS;
    int* const row_emit = row_tok + RT_ROWS;
    int* const row_cnt = row_emit + RT_ROWS;
    int* const row_live = row_cnt + RT_ROWS;
    int* const dur_tab = row_live + RT_ROWS;                                    // [16]
    auto hb = [&](int buf, int l) { return hbuf + ((size_t)buf * L + l) * RT_ROWS * LDH; };
    // this workgroup's slice: c [L][16][Hp], g [16][J], each element touched by its owner lane only
    float* const cw = p.slices + (size_t)blockIdx.x * ((size_t)L * RT_ROWS * Hp + (size_t)RT_ROWS * J);
    float* const gw = cw + (size_t)L * RT_ROWS * Hp;
    const size_t cbase = (size_t)L * B * Hp;   // c block of a state

    if (tid < RT_ROWS) {
        const int r = r0 + tid;
        const int len = r < B ? (p.lengths ? min(max(p.lengths[r], 0), p.T) : p.T) : 0;
        const int t = (p.skip_in && r < B) ? max(p.skip_in[r], 0) : 0;
        row_len[tid] = len;
        row_t[tid] = t;
        row_n[tid] = 0;
        row_cnt[tid] = 0;
        row_total[tid] = 0.0;
        row_tok[tid] = net.blank;
        row_emit[tid] = p.state_in ? 0 : 1;   // no state: the start step on Emb[blank]
        row_live[tid] = t < len;
    }
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < TDT_MAX_D; i++) dur_tab[i] = p.dur[i];   // constant indices: the table stays in SGPRs
    }
    for (int x = tid; x < L * RT_ROWS * Hp; x += 64 * RT_WAVES) {
        const int l = x / (RT_ROWS * Hp), row = (x / Hp) % RT_ROWS, n = x % Hp, r = r0 + row;
        hb(0, l)[row * LDH + n] = (p.state_in && r < B) ? p.state_in[((size_t)l * B + r) * Hp + n] : 0.f;
    }
    for (int l = 0; l < L; l++)
        for (int jt = w; jt < (Hp >> 4); jt += RT_WAVES)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int row = 4 * g + j, r = r0 + row, n = 16 * jt + c;
                cw[((size_t)l * RT_ROWS + row) * Hp + n] =
                    (p.state_in && r < B) ? p.state_in[cbase + ((size_t)l * B + r) * Hp + n] : 0.f;
            }
    __syncthreads();

    int cur = 0;
    bool need_g = true;
    for (int it = 0;; it++) {
        int any_emit = 0, any_live = 0;
#pragma unroll
        for (int x = 0; x < RT_ROWS; x++) {
            any_emit |= row_emit[x];
            any_live |= row_live[x];
        }
        if (any_emit) {
            // predictor step of the rows that emitted; the others copy their h
            rt_lstm_step(net, hb, cur, cw, cw, [](int r) { return r; },
                         [&](int r) { return row_emit[r] ? row_tok[r] : -1; }, w, g, c);
            cur ^= 1;
        }
        if (any_emit || need_g) {
            // g = h_top.W_pred + b_pred (for every row: a row that kept its h gets its g again)
            need_g = false;
            rt_sweep<1, false>(hb(cur, L - 1) + c * LDH + 4 * g, 0, Hp >> 4, net.wpred, net.bpred, J, w, g, c,
                               [&](int, int n, f32x4 x) {
#pragma unroll
                                   for (int j = 0; j < 4; j++) gw[(size_t)(4 * g + j) * J + n] = x[j];
                               });
        }
        if (!any_live || it >= p.max_iters) break;

        // z = act(f_t + g): the lane that owns g's element, each row at its own t (clamped: a row past its end
        // is not live and its z is not used)
        for (int jt = w; jt < (J >> 4); jt += RT_WAVES) {
            const int n = 16 * jt + c;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int row = 4 * g + j;
                const int rr = min(r0 + row, B - 1), tt = min(row_t[row], p.T - 1);
                const float x = p.f[((size_t)tt * B + rr) * J + n] + gw[(size_t)row * J + n];
                zbuf[row * LDJ + n] = rt_act(x, net.act);
            }
        }
        __syncthreads();

        const float* za = zbuf + c * LDJ + 4 * g;
        RtTop top[4];
#pragma unroll
        for (int j = 0; j < 4; j++) top[j] = RtTop{-INFINITY, 0.f, RT_NONE};
        // the token-only tiles: rnnt_greedy_kernel's schedule over ntp whole tiles of the [J][W] matrix
        for (int base = 0; base < ntp; base += 4 * RT_WAVES) {
            const int t0 = base + w;
            const int nv = t0 < ntp ? min(4, (ntp - 1 - t0) / RT_WAVES + 1) : 0;
            if (nv == 4) {
                const int col[4] = {16 * t0 + c, 16 * (t0 + RT_WAVES) + c, 16 * (t0 + 2 * RT_WAVES) + c,
                                    16 * (t0 + 3 * RT_WAVES) + c};
                f32x4 acc[1][4];
#pragma unroll
                for (int q = 0; q < 4; q++) acc[0][q] = f32x4{0.f, 0.f, 0.f, 0.f};
                rt_mma<1, 4>(za, 0, J >> 4, net.wout, (unsigned)W, g, col, acc);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const float b = net.bout[col[q]];
#pragma unroll
                    for (int j = 0; j < 4; j++) rt_push(top[j], acc[0][q][j] + b, col[q]);
                }
            } else {
                for (int q = 0; q < nv; q++) {
                    const int col[1] = {16 * (t0 + q * RT_WAVES) + c};
                    f32x4 acc[1][1] = {{f32x4{0.f, 0.f, 0.f, 0.f}}};
                    rt_mma<1, 1>(za, 0, J >> 4, net.wout, (unsigned)W, g, col, acc);
                    const float b = net.bout[col[0]];
#pragma unroll
                    for (int j = 0; j < 4; j++) rt_push(top[j], acc[0][0][j] + b, col[0]);
                }
            }
        }
        {
            // the tail: the at most two tiles ntp .. nt - 1 that hold a duration column, at most one of them this
            // wave's.  Column n < V is a token, V <= n < W duration n - V; columns >= W do not exist.
            RtTop dtop[4];
#pragma unroll
            for (int j = 0; j < 4; j++) dtop[j] = RtTop{-INFINITY, 0.f, RT_NONE};
            for (int jt = ntp; jt < nt; jt++) {
                if ((jt & (RT_WAVES - 1)) != w) continue;
                const int n = 16 * jt + c;
                const int col[1] = {min(n, W - 1)};
                f32x4 acc[1][1] = {{f32x4{0.f, 0.f, 0.f, 0.f}}};
                rt_mma<1, 1>(za, 0, J >> 4, net.wout, (unsigned)W, g, col, acc);
                if (n >= W) continue;
                const float b = net.bout[n];
                if (n < V) {
#pragma unroll
                    for (int j = 0; j < 4; j++) rt_push(top[j], acc[0][0][j] + b, n);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++) rt_push(dtop[j], acc[0][0][j] + b, n - V);
                }
            }
            // the duration top: the 16 lanes of a row, then (below) the waves in the order 0..7; a wave without a
            // duration column leaves the empty top
#pragma unroll
            for (int j = 0; j < 4; j++) rt_row_partial<true>(dtop[j], c, w * RT_ROWS + 4 * g + j, dred_m, dred_s, dred_i);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) rt_row_partial<true>(top[j], c, w * RT_ROWS + 4 * g + j, red_m, red_s, red_i);
        __syncthreads();
        if (tid < RT_ROWS) {
            const int row = tid, r = r0 + row;
            int t = row_t[row], n = row_n[row], em = 0;
            const int len = row_len[row];
            if (t < len) {
                const RtTop a = rt_row_total<true>(row, RT_ROWS, red_m, red_s, red_i);
                const RtTop b = rt_row_total<true>(row, RT_ROWS, dred_m, dred_s, dred_i);
                const int k = a.i == RT_NONE ? 0 : a.i;
                const int dur = dur_tab[b.i == RT_NONE ? 0 : b.i];
                // logit[k] - logsumexp(logit) and dlogit[d] - logsumexp(dlogit), each maximum its own
                const double lp = (double)-logf(a.s) + (double)-logf(b.s);
                row_total[row] += lp;
                if (k != net.blank) {
                    const int cnt = row_cnt[row];
                    if (cnt < p.max_out) {
                        const size_t o = (size_t)r * p.max_out + cnt;
                        p.tokens[o] = k;
                        p.timesteps[o] = t;
                        p.durations[o] = dur;
                        p.logp[o] = lp;
                    }
                    row_cnt[row] = cnt + 1;
                    row_tok[row] = k;
                    em = 1;
                    n++;
                    if (dur > 0) {
                        t += dur;
                        n = 0;
                    } else if (n == p.max_symbols) {
                        t++;
                        n = 0;
                    }
                } else {
                    t += max(dur, 1);
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

    if (tid < RT_ROWS && r0 + tid < B) {
        p.count[r0 + tid] = row_cnt[tid];
        p.total[r0 + tid] = row_total[tid];
        if (p.skip_out) p.skip_out[r0 + tid] = max(row_t[tid] - row_len[tid], 0);
    }
    if (p.state_out) {
        for (int x = tid; x < L * RT_ROWS * Hp; x += 64 * RT_WAVES) {
            const int l = x / (RT_ROWS * Hp), row = (x / Hp) % RT_ROWS, n = x % Hp, r = r0 + row;
            if (r < B) p.state_out[((size_t)l * B + r) * Hp + n] = hb(cur, l)[row * LDH + n];
        }
        for (int l = 0; l < L; l++)
            for (int jt = w; jt < (Hp >> 4); jt += RT_WAVES)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int row = 4 * g + j, r = r0 + row, n = 16 * jt + c;
                    if (r < B) p.state_out[cbase + ((size_t)l * B + r) * Hp + n] = cw[((size_t)l * RT_ROWS + row) * Hp + n];
                }
    }
}

// The checks the device and the host decode share, before any HIP call (asr_rnnt_greedy's, then the kind).
static int rnnt_tdt_check(const asr_rnnt* h, const void* enc, int T, int B, int max_out, const void* tokens,
                          const void* timesteps, const void* durations, const void* logp, const void* count,
                          const void* total) {
    if (!h || !enc || !count || !total || T <= 0 || B <= 0 || max_out < 0) return ASR_ERR_ARG;
    if (max_out > 0 && (!tokens || !timesteps || !durations || !logp)) return ASR_ERR_ARG;
    if ((long)T * B > INT_MAX || (long)T * (h->d.max_symbols + 1) >= INT_MAX) return ASR_ERR_UNSUPPORTED;
    if (!h->nd) return ASR_ERR_UNSUPPORTED;   // a plain or a stateless handle
    return ASR_OK;
}

// (lowest argmax, -log sum exp(x - max), best - second) of x[0 .. n): the twin's view of one head.
struct TdtHead {
    int k;
    double lp, gap;
};
static TdtHead tdt_head(const double* x, int n) {
    int k = -1;
    double best = -HUGE_VAL, second = -HUGE_VAL;
    for (int v = 0; v < n; v++) {
        if (x[v] != x[v]) continue;   // a NaN never wins
        if (k < 0 || x[v] > best) {
            if (k >= 0) second = best;
            best = x[v];
            k = v;
        } else if (x[v] > second) {
            second = x[v];   // an equal maximum: the lower index keeps it, the gap is 0
        }
    }
    if (k < 0) k = 0;   // every entry a NaN
    double se = 0.0;
    for (int v = 0; v < n; v++) se += std::exp(x[v] - best);
    return TdtHead{k, -std::log(se), best - second};
}

}  // namespace asr

extern "C" {

int asr_rnnt_create_tdt(const asr_rnnt_desc* desc, const asr_rnnt_weights* wt, int num_durations,
                        const int32_t* durations, const float* w_dur, const float* b_dur, asr_rnnt_t** out) {
    if (out) *out = nullptr;
    if (!desc || !wt || !out || !durations || !w_dur || !b_dur) return ASR_ERR_ARG;
    if (num_durations < 1 || num_durations > asr::TDT_MAX_D) return ASR_ERR_ARG;
    bool advance = false;
    for (int i = 0; i < num_durations; i++) {
        if (durations[i] < 0 || durations[i] > 32767) return ASR_ERR_ARG;
        advance |= durations[i] > 0;
    }
    if (!advance) return ASR_ERR_ARG;   // a table of zeros never leaves a frame by its own choice
    asr_rnnt* h = nullptr;
    if (int rc = asr_rnnt_create(desc, wt, &h)) return rc;
    const int J = desc->J, V = desc->V, D = num_durations, W = V + D;
    if ((long)J * W > INT_MAX) {
        delete h;
        return ASR_ERR_UNSUPPORTED;
    }
    try {
        // W_out | W_dur as one [J][V + D] matrix, the biases likewise: what the kernel streams and the twin reads
        std::vector<float> wcat((size_t)J * W), bcat(W);
        for (int j = 0; j < J; j++) {
            std::copy(wt->w_out + (size_t)j * V, wt->w_out + (size_t)(j + 1) * V, wcat.begin() + (size_t)j * W);
            std::copy(w_dur + (size_t)j * D, w_dur + (size_t)(j + 1) * D, wcat.begin() + (size_t)j * W + V);
        }
        std::copy(wt->b_out, wt->b_out + V, bcat.begin());
        std::copy(b_dur, b_dur + D, bcat.begin() + V);
        h->wout.swap(wcat);
        h->bout.swap(bcat);
    } catch (const std::bad_alloc&) {
        delete h;
        return ASR_ERR_OOM;
    }
    h->nd = D;
    std::copy(durations, durations + D, h->durs);
    h->weight_bytes += (int64_t)(((size_t)J * D + D) * sizeof(float));
    *out = h;
    return ASR_OK;
}

int asr_rnnt_tdt_durations(const asr_rnnt_t* h, int32_t* durations) {
    if (!h) return 0;
    if (durations) std::copy(h->durs, h->durs + h->nd, durations);
    return h->nd;
}

int asr_rnnt_greedy_tdt(const asr_rnnt_t* h, const float* d_enc, const int32_t* d_lengths, int T, int B, int max_out,
                        const float* d_state_in, float* d_state_out, const int32_t* d_skip_in, int32_t* d_skip_out,
                        int32_t* d_tokens, int32_t* d_timesteps, int32_t* d_durations, double* d_logp,
                        int32_t* d_count, double* d_total, void* d_work, asr_stream_t s) {
    if (int rc = asr::rnnt_tdt_check(h, d_enc, T, B, max_out, d_tokens, d_timesteps, d_durations, d_logp, d_count,
                                     d_total))
        return rc;
    if (!d_work) return ASR_ERR_ARG;
    if (!h->d_blob) return ASR_ERR_STATE;
    const asr_rnnt_desc& d = h->d;
    float* f = (float*)d_work;
    if (int rc = asr::rnnt_enc_launch(h, d_enc, T, B, f, asr_stream(s))) return rc;
    asr::TdtArgs a{};
    a.f = f;
    a.net = asr::rnnt_net(h);
    a.lengths = d_lengths; a.state_in = d_state_in; a.state_out = d_state_out;
    a.skip_in = d_skip_in; a.skip_out = d_skip_out;
    a.tokens = d_tokens; a.timesteps = d_timesteps; a.durations = d_durations; a.logp = d_logp;
    a.count = d_count; a.total = d_total;
    a.slices = f + (size_t)T * B * d.J;
    a.T = T; a.B = B; a.nd = h->nd; a.max_symbols = d.max_symbols; a.max_out = max_out;
    a.max_iters = T * d.max_symbols;   // the hard bound on joint evaluations per row (the file header derives it)
    for (int i = 0; i < asr::TDT_MAX_D; i++) a.dur[i] = (short)(i < h->nd ? h->durs[i] : 0);
    static AsrAttrOnce attr;
    if (int rc = attr.set((const void*)asr::rnnt_tdt_kernel, asr::RT_LDS_MAX)) return rc;
    const unsigned gx = (unsigned)((B + asr::RT_ROWS - 1) / asr::RT_ROWS);
    hipLaunchKernelGGL(asr::rnnt_tdt_kernel, dim3(gx), dim3(64 * asr::RT_WAVES), (size_t)h->lds_bytes, asr_stream(s),
                       a);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

int asr_rnnt_greedy_tdt_host(const asr_rnnt_t* h, const float* h_enc, const int32_t* h_lengths, int T, int B,
                             int max_out, const double* h_state_in, double* h_state_out, const int32_t* h_skip_in,
                             int32_t* h_skip_out, int32_t* h_tokens, int32_t* h_timesteps, int32_t* h_durations,
                             double* h_logp, int32_t* h_count, double* h_total, double* h_gap, double* h_dgap) {
    if (int rc = asr::rnnt_tdt_check(h, h_enc, T, B, max_out, h_tokens, h_timesteps, h_durations, h_logp, h_count,
                                     h_total))
        return rc;
    const asr_rnnt_desc& d = h->d;
    const int W = d.V + h->nd;
    const size_t LH = (size_t)d.L * d.Hp, cbase = (size_t)d.L * B * d.Hp;
    try {
        asr::RnntHost m(*h);
        std::vector<double> hs(LH), cs(LH), logit(W);
        for (int b = 0; b < B; b++) {
            if (h_state_in) {
                for (int l = 0; l < d.L; l++)
                    for (int n = 0; n < d.Hp; n++) {
                        hs[(size_t)l * d.Hp + n] = h_state_in[((size_t)l * B + b) * d.Hp + n];
                        cs[(size_t)l * d.Hp + n] = h_state_in[cbase + ((size_t)l * B + b) * d.Hp + n];
                    }
            } else {
                std::fill(hs.begin(), hs.end(), 0.0);
                std::fill(cs.begin(), cs.end(), 0.0);
                m.step(d.blank, hs.data(), cs.data());
            }
            m.pred_proj(hs.data());
            const int len = h_lengths ? std::min(std::max(h_lengths[b], 0), T) : T;
            int t = h_skip_in ? std::max(h_skip_in[b], 0) : 0, n = 0, cnt = 0, tf = -1;
            const long max_iters = (long)T * d.max_symbols;
            double total = 0.0, gap = HUGE_VAL, dgap = HUGE_VAL;
            for (long it = 0; it < max_iters && t < len; it++) {
                if (tf != t) {
                    m.enc_proj(h_enc + ((size_t)t * B + b) * d.E);
                    tf = t;
                }
                // both heads from the one [J][V + D] matrix: logit [0, V), dlogit [V, V + D)
                for (int j = 0; j < d.J; j++) {
                    const double v = m.f[j] + m.g[j];
                    m.z[j] = d.act == ASR_RNNT_ACT_TANH ? std::tanh(v) : (v > 0.0 ? v : 0.0);
                }
                asr::RnntHost::matvec(m.z.data(), h->wout.data(), d.J, W, logit.data());
                for (int v = 0; v < W; v++) logit[v] += (double)h->bout[v];
                const asr::TdtHead tk = asr::tdt_head(logit.data(), d.V);
                const asr::TdtHead du = asr::tdt_head(logit.data() + d.V, h->nd);
                const int k = tk.k, dur = h->durs[du.k];
                const double lp = tk.lp + du.lp;
                gap = std::min(gap, tk.gap);
                dgap = std::min(dgap, du.gap);
                total += lp;
                if (k != d.blank) {
                    if (cnt < max_out) {
                        const size_t o = (size_t)b * max_out + cnt;
                        h_tokens[o] = k;
                        h_timesteps[o] = t;
                        h_durations[o] = dur;
                        h_logp[o] = lp;
                    }
                    cnt++;
                    m.step(k, hs.data(), cs.data());
                    m.pred_proj(hs.data());
                    n++;
                    if (dur > 0) {
                        t += dur;
                        n = 0;
                    } else if (n == d.max_symbols) {
                        t++;
                        n = 0;
                    }
                } else {
                    t += std::max(dur, 1);
                    n = 0;
                }
            }
            h_count[b] = cnt;
            h_total[b] = total;
            if (h_skip_out) h_skip_out[b] = std::max(t - len, 0);
            if (h_gap) h_gap[b] = gap;
            if (h_dgap) h_dgap[b] = dgap;
            if (h_state_out)
                for (int l = 0; l < d.L; l++)
                    for (int x = 0; x < d.Hp; x++) {
                        h_state_out[((size_t)l * B + b) * d.Hp + x] = hs[(size_t)l * d.Hp + x];
                        h_state_out[cbase + ((size_t)l * B + b) * d.Hp + x] = cs[(size_t)l * d.Hp + x];
                    }
        }
    } catch (const std::bad_alloc&) {
        return ASR_ERR_OOM;
    }
    return ASR_OK;
}

}  // extern "C"
