// RNN-T (transducer) greedy decoding: asr_rnnt_create / _upload / _get_info /
// _destroy / _workspace_bytes / asr_rnnt_greedy / asr_rnnt_greedy_host.
//
// Model (weights in the project's [in][out] layout):
//   predictor  Emb [V][D], then L <= 2 LSTM layers of asr_lstm_fwd's cell
//              (gates i, f, g, o; (x.W_ih + h.W_hh) + (b_ih + b_hh));
//   joint      f_t = enc_t.W_enc + b_enc,  g = h_top.W_pred + b_pred,
//              z = act(f_t + g),  logit = z.W_out + b_out.
// Greedy walk of utterance b (len_b clamped to [0, T]): without a state h = c =
// 0 and the predictor takes one step on Emb[blank]; t = 0, n = 0; while t <
// len_b: k = argmax logit (lowest index among equal maxima, a NaN never wins),
// logp = logit[k] - logsumexp(logit); k != blank: record (k, t, logp), step the
// predictor on Emb[k], n += 1, and at n == max_symbols t += 1, n = 0; k ==
// blank: logp goes to the total only, t += 1, n = 0.
//
// Device form.  f for all T frames is one gemm_launch (bias fused) into the
// workspace, the split asr_lstm_fwd uses; x.W_ih of layer 0 is a row of
// Emb.W_ih, one gemm_launch at upload, so a predictor step gathers it as the
// LSTM gathers P_t.  The walk is ONE launch: a workgroup of 8 waves owns 16
// utterances, the rows of a v_mfma_f32_16x16x4_f32 tile; its waves split the
// 16-column tiles (tile j belongs to wave j % 8), streaming the weights from L2
// with gated_step_kernel's register ring.  h (two buffers per layer) and z live
// in LDS; c and g are owned by the lane that computes them and sit in the
// workgroup's slice of the workspace.  Each iteration: rows that emitted take a
// predictor step (skipped by a workgroup-uniform branch when none did), every
// row evaluates the joint at its own t (the f row is a per-row address), the
// waves keep a running (max, argmax, sum-exp) per row, combined in a fixed
// order, and one thread per row advances that row's walk.  No workgroup reads
// what another one writes; the loop runs at most T * (max_symbols + 1) + 1
// times, a bound set by the host.  A row's bits depend on the model's shape
// only: MFMA rows are independent, a row that did not emit keeps its state
// whether or not its tile stepped, and g is always h_top.W_pred + b_pred.
#include "rnnt_common.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <new>
#include <vector>

namespace asr {

struct RnntArgs {
    const float* f;          // [T*B][J]
    const float* embw;       // [V][4Hp] = Emb.W_ih of layer 0
    const float* wih1;       // [Hp][4Hp], layer 1 (L = 2)
    const float* whh[2];
    const float* bih[2];
    const float* bhh[2];
    const float* wpred;
    const float* bpred;
    const float* wout;
    const float* bout;
    const int32_t* lengths;
    const float* state_in;   // [2][L][B][Hp] or NULL
    float* state_out;        // the same, or NULL
    int32_t* tokens;
    int32_t* timesteps;
    double* logp;
    int32_t* count;
    double* total;
    float* slices;           // per workgroup: c [L][16][Hp], g [16][J]
    int T, B, Hp, J, V, L, blank, act, max_symbols, max_out, max_iters;
};

// The predictor step, the two column-tile sweeps and the row reduction below are rt_lstm_step (with the row as its
// own parent), rt_sweep and rt_row_partial / rt_row_total of rnnt_common.h written out: called through them this
// kernel gave equal bytes and measured 0.1 to 0.2 % slower.  The k order, the tile-to-wave map and
// the order of the joins must stay theirs (test_beam_one_is_the_greedy_kernel compares the two kernels' walks).
__global__ __launch_bounds__(64 * RT_WAVES) void rnnt_greedy_kernel(const RnntArgs p) {
    extern __shared__ __attribute__((aligned(16))) float rt_lds[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int Hp = p.Hp, J = p.J, V = p.V, L = p.L, B = p.B;
    const int H4 = 4 * Hp, LDH = Hp + 4, LDJ = J + 4;
    const int r0 = blockIdx.x * RT_ROWS;
    // LDS: h [2][L][16][LDH], z [16][LDJ], then the small area
    float* const hbuf = rt_lds;
    float* const zbuf = hbuf + (size_t)2 * L * RT_ROWS * LDH;
    float* const small = zbuf + (size_t)RT_ROWS * LDJ;
    double* const row_total = reinterpret_cast<double*>(small);                 // [16]
    float* const red_m = small + 2 * RT_ROWS;                                   // [8][16]
    float* const red_s = red_m + RT_WAVES * RT_ROWS;
    int* const red_i = reinterpret_cast<int*>(red_s + RT_WAVES * RT_ROWS);
    int* const row_t = red_i + RT_WAVES * RT_ROWS;                              // [16] each
    int* const row_n = row_t + RT_ROWS;
    int* const row_len = row_n + RT_ROWS;
    int* const row_tok = row_len + RT_ROWS;
    int* const row_emit = row_tok + RT_ROWS;
    int* const row_cnt = row_emit + RT_ROWS;
    int* const row_live = row_cnt + RT_ROWS;
    auto hb = [&](int buf, int l) { return hbuf + ((size_t)buf * L + l) * RT_ROWS * LDH; };
    // this workgroup's slice: c [L][16][Hp], g [16][J], each element touched by its owner lane only
    float* const cw = p.slices + (size_t)blockIdx.x * ((size_t)L * RT_ROWS * Hp + (size_t)RT_ROWS * J);
    float* const gw = cw + (size_t)L * RT_ROWS * Hp;
    const size_t cbase = (size_t)L * B * Hp;   // c block of a state

    if (tid < RT_ROWS) {
        const int r = r0 + tid;
        const int len = r < B ? (p.lengths ? min(max(p.lengths[r], 0), p.T) : p.T) : 0;
        row_len[tid] = len;
        row_t[tid] = 0;
        row_n[tid] = 0;
        row_cnt[tid] = 0;
        row_total[tid] = 0.0;
        row_tok[tid] = p.blank;
        row_emit[tid] = p.state_in ? 0 : 1;   // no state: the start step on Emb[blank]
        row_live[tid] = len > 0;
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
            // Predictor step of the rows that emitted; the others copy their h.
            for (int l = 0; l < L; l++) {
                const float* hold = hb(cur, l);
                float* hnew = hb(cur ^ 1, l);
                const float* Whh = p.whh[l];
                for (int jt = w; jt < (Hp >> 4); jt += RT_WAVES) {
                    const int n = 16 * jt + c;
                    const int col[4] = {n, Hp + n, 2 * Hp + n, 3 * Hp + n};
                    f32x4 acc[1][4], accx[1][4];
#pragma unroll
                    for (int q = 0; q < 4; q++) acc[0][q] = accx[0][q] = f32x4{0.f, 0.f, 0.f, 0.f};
                    rt_mma<1, 4>(hold + c * LDH + 4 * g, 0, Hp >> 4, Whh, H4, g, col, acc);
                    if (l > 0)   // x = the layer below's new h
                        rt_mma<1, 4>(hb(cur ^ 1, l - 1) + c * LDH + 4 * g, 0, Hp >> 4, p.wih1, H4, g, col, accx);
                    float bias[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) bias[q] = p.bih[l][col[q]] + p.bhh[l][col[q]];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int row = 4 * g + j;
                        const bool em = row_emit[row] != 0;
                        float px[4];
                        if (l == 0) {
                            const float* e = p.embw + (size_t)row_tok[row] * H4;
#pragma unroll
                            for (int q = 0; q < 4; q++) px[q] = e[col[q]];
                        } else {
#pragma unroll
                            for (int q = 0; q < 4; q++) px[q] = accx[0][q][j];
                        }
                        const size_t cx = ((size_t)l * RT_ROWS + row) * Hp + n;
                        const float cold = cw[cx];
                        const float zi = (px[0] + acc[0][0][j]) + bias[0], zf = (px[1] + acc[0][1][j]) + bias[1];
                        const float zg = (px[2] + acc[0][2][j]) + bias[2], zo = (px[3] + acc[0][3][j]) + bias[3];
                        const float ig = rt_sigmoid(zi), fg = rt_sigmoid(zf), gg = tanhf(zg), og = rt_sigmoid(zo);
                        const float cn = fg * cold + ig * gg;
                        const float hn = og * tanhf(cn);
                        cw[cx] = em ? cn : cold;
                        hnew[row * LDH + n] = em ? hn : hold[row * LDH + n];
                    }
                }
                __syncthreads();   // layer l's new h, before layer l + 1 and g read it
            }
            cur ^= 1;
        }
        if (any_emit || need_g) {
            // g = h_top.W_pred + b_pred (for every row: a row that kept its h gets its g again)
            need_g = false;
            const float* ht = hb(cur, L - 1) + c * LDH + 4 * g;
            const int nt = J >> 4;
            for (int base = 0; base < nt; base += 4 * RT_WAVES) {
                const int t0 = base + w;
                const int nv = t0 < nt ? min(4, (nt - 1 - t0) / RT_WAVES + 1) : 0;
                if (nv == 4) {
                    const int col[4] = {16 * t0 + c, 16 * (t0 + RT_WAVES) + c, 16 * (t0 + 2 * RT_WAVES) + c,
                                        16 * (t0 + 3 * RT_WAVES) + c};
                    f32x4 acc[1][4];
#pragma unroll
                    for (int q = 0; q < 4; q++) acc[0][q] = f32x4{0.f, 0.f, 0.f, 0.f};
                    rt_mma<1, 4>(ht, 0, Hp >> 4, p.wpred, J, g, col, acc);
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const float b = p.bpred[col[q]];
#pragma unroll
                        for (int j = 0; j < 4; j++) gw[(size_t)(4 * g + j) * J + col[q]] = acc[0][q][j] + b;
                    }
                } else {
                    for (int q = 0; q < nv; q++) {
                        const int col[1] = {16 * (t0 + q * RT_WAVES) + c};
                        f32x4 acc[1][1] = {{f32x4{0.f, 0.f, 0.f, 0.f}}};
                        rt_mma<1, 1>(ht, 0, Hp >> 4, p.wpred, J, g, col, acc);
                        const float b = p.bpred[col[0]];
#pragma unroll
                        for (int j = 0; j < 4; j++) gw[(size_t)(4 * g + j) * J + col[0]] = acc[0][0][j] + b;
                    }
                }
            }
        }
        if (!any_live || it >= p.max_iters) break;

        // z = act(f_t + g): the lane that owns g's element, each row at its own t
        for (int jt = w; jt < (J >> 4); jt += RT_WAVES) {
            const int n = 16 * jt + c;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int row = 4 * g + j;
                const int rr = min(r0 + row, B - 1), tt = min(row_t[row], p.T - 1);
                const float x = p.f[((size_t)tt * B + rr) * J + n] + gw[(size_t)row * J + n];
                zbuf[row * LDJ + n] = rt_act(x, p.act);
            }
        }
        __syncthreads();

        // logit = z.W_out + b_out over the V column tiles; columns >= V do not exist
        RtTop top[4];
#pragma unroll
        for (int j = 0; j < 4; j++) top[j] = RtTop{-INFINITY, 0.f, RT_NONE};
        {
            const float* za = zbuf + c * LDJ + 4 * g;
            const int nt = (V + 15) >> 4;
            for (int base = 0; base < nt; base += 4 * RT_WAVES) {
                const int t0 = base + w;
                const int nv = t0 < nt ? min(4, (nt - 1 - t0) / RT_WAVES + 1) : 0;
                if (nv == 4) {
                    int n[4], col[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        n[q] = 16 * (t0 + q * RT_WAVES) + c;
                        col[q] = min(n[q], V - 1);
                    }
                    f32x4 acc[1][4];
#pragma unroll
                    for (int q = 0; q < 4; q++) acc[0][q] = f32x4{0.f, 0.f, 0.f, 0.f};
                    rt_mma<1, 4>(za, 0, J >> 4, p.wout, V, g, col, acc);
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        if (n[q] >= V) continue;
                        const float b = p.bout[n[q]];
#pragma unroll
                        for (int j = 0; j < 4; j++) rt_push(top[j], acc[0][q][j] + b, n[q]);
                    }
                } else {
                    for (int q = 0; q < nv; q++) {
                        const int n = 16 * (t0 + q * RT_WAVES) + c;
                        const int col[1] = {min(n, V - 1)};
                        f32x4 acc[1][1] = {{f32x4{0.f, 0.f, 0.f, 0.f}}};
                        rt_mma<1, 1>(za, 0, J >> 4, p.wout, V, g, col, acc);
                        if (n >= V) continue;
                        const float b = p.bout[n];
#pragma unroll
                        for (int j = 0; j < 4; j++) rt_push(top[j], acc[0][0][j] + b, n);
                    }
                }
            }
        }
        // the 16 lanes of a row, then the waves in the order 0..7
#pragma unroll
        for (int j = 0; j < 4; j++) {
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) {
                RtTop o;
                o.m = __shfl_xor(top[j].m, d);
                o.s = __shfl_xor(top[j].s, d);
                o.i = __shfl_xor(top[j].i, d);
                top[j] = rt_join(top[j], o);
            }
            if (c == 0) {
                red_m[w * RT_ROWS + 4 * g + j] = top[j].m;
                red_s[w * RT_ROWS + 4 * g + j] = top[j].s;
                red_i[w * RT_ROWS + 4 * g + j] = top[j].i;
            }
        }
        __syncthreads();
        if (tid < RT_ROWS) {
            const int row = tid, r = r0 + row;
            int t = row_t[row], n = row_n[row], em = 0;
            const int len = row_len[row];
            if (t < len) {
                RtTop a{red_m[row], red_s[row], red_i[row]};
                for (int x = 1; x < RT_WAVES; x++)
                    a = rt_join(a, RtTop{red_m[x * RT_ROWS + row], red_s[x * RT_ROWS + row], red_i[x * RT_ROWS + row]});
                const int k = a.i == RT_NONE ? 0 : a.i;
                const float lp = -logf(a.s);   // logit[k] - logsumexp(logit), logit[k] the maximum
                row_total[row] += (double)lp;
                if (k != p.blank) {
                    const int cnt = row_cnt[row];
                    if (cnt < p.max_out) {
                        const size_t o = (size_t)r * p.max_out + cnt;
                        p.tokens[o] = k;
                        p.timesteps[o] = t;
                        p.logp[o] = (double)lp;
                    }
                    row_cnt[row] = cnt + 1;
                    row_tok[row] = k;
                    em = 1;
                    if (++n == p.max_symbols) {
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

    if (tid < RT_ROWS && r0 + tid < B) {
        p.count[r0 + tid] = row_cnt[tid];
        p.total[r0 + tid] = row_total[tid];
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

static int rnnt_desc_check(const asr_rnnt_desc& d) {
    if (d.V < 2 || d.blank < 0 || d.blank >= d.V || d.E <= 0 || d.D <= 0 || d.Hp <= 0 || d.J <= 0 || d.L < 1 ||
        d.max_symbols < 1 || (d.act != ASR_RNNT_ACT_RELU && d.act != ASR_RNNT_ACT_TANH))
        return ASR_ERR_ARG;
    if (d.L > ASR_RNNT_MAX_LAYERS || (d.D & 15) || (d.Hp & 15) || (d.J & 15)) return ASR_ERR_UNSUPPORTED;
    if (rnnt_lds_bytes(d.L, d.Hp, d.J, asr::RT_LDS_SMALL) > RT_LDS_MAX) return ASR_ERR_UNSUPPORTED;
    if ((long)d.V * 4 * d.Hp > INT_MAX || (long)d.V * d.J > INT_MAX || (long)d.V * d.D > INT_MAX ||
        (long)d.E * d.J > INT_MAX)
        return ASR_ERR_UNSUPPORTED;
    return ASR_OK;
}

// The checks the device and the host decode share, before any HIP call.
static int rnnt_greedy_check(const asr_rnnt* h, const void* enc, int T, int B, int max_out, const void* tokens,
                             const void* timesteps, const void* logp, const void* count, const void* total) {
    if (!h || !enc || !count || !total || T <= 0 || B <= 0 || max_out < 0) return ASR_ERR_ARG;
    if (max_out > 0 && (!tokens || !timesteps || !logp)) return ASR_ERR_ARG;
    if ((long)T * B > INT_MAX || (long)T * (h->d.max_symbols + 1) >= INT_MAX) return ASR_ERR_UNSUPPORTED;
    return ASR_OK;
}

}  // namespace asr

extern "C" {

int asr_rnnt_create(const asr_rnnt_desc* desc, const asr_rnnt_weights* wt, asr_rnnt_t** out) {
    if (out) *out = nullptr;
    if (!desc || !wt || !out) return ASR_ERR_ARG;
    if (int rc = asr::rnnt_desc_check(*desc)) return rc;
    const asr_rnnt_desc& d = *desc;
    if (!wt->emb || !wt->w_enc || !wt->b_enc || !wt->w_pred || !wt->b_pred || !wt->w_out || !wt->b_out)
        return ASR_ERR_ARG;
    for (int l = 0; l < d.L; l++)
        if (!wt->w_ih[l] || !wt->w_hh[l] || !wt->b_ih[l] || !wt->b_hh[l]) return ASR_ERR_ARG;
    asr_rnnt* h = new (std::nothrow) asr_rnnt;
    if (!h) return ASR_ERR_OOM;
    try {
        h->d = d;
        const size_t H4 = 4 * (size_t)d.Hp;
        h->emb.assign(wt->emb, wt->emb + (size_t)d.V * d.D);
        for (int l = 0; l < d.L; l++) {
            const size_t in = l ? d.Hp : d.D;
            h->wih[l].assign(wt->w_ih[l], wt->w_ih[l] + in * H4);
            h->whh[l].assign(wt->w_hh[l], wt->w_hh[l] + (size_t)d.Hp * H4);
            h->bih[l].assign(wt->b_ih[l], wt->b_ih[l] + H4);
            h->bhh[l].assign(wt->b_hh[l], wt->b_hh[l] + H4);
        }
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
    h->lds_bytes = (int)asr::rnnt_lds_bytes(d.L, d.Hp, d.J, asr::RT_LDS_SMALL);
    size_t n = h->emb.size() + h->wenc.size() + h->benc.size() + h->wpred.size() + h->bpred.size() + h->wout.size() +
               h->bout.size();
    for (int l = 0; l < d.L; l++) n += h->wih[l].size() + h->whh[l].size() + h->bih[l].size() + h->bhh[l].size();
    h->weight_bytes = (int64_t)(n * sizeof(float));
    *out = h;
    return ASR_OK;
}

int asr_rnnt_destroy(asr_rnnt_t* h) {
    if (!h) return ASR_ERR_ARG;
    int rc = ASR_OK;
    if (h->d_blob && hipFree(h->d_blob) != hipSuccess) rc = ASR_ERR_HIP;
    delete h;
    return rc;
}

int asr_rnnt_get_info(const asr_rnnt_t* h, asr_rnnt_info* info) {
    if (!h || !info) return ASR_ERR_ARG;
    info->desc = h->d;
    info->uploaded = h->d_blob ? 1 : 0;
    info->lds_bytes = h->lds_bytes;
    info->weight_bytes = h->weight_bytes;
    return ASR_OK;
}

int asr_rnnt_upload(asr_rnnt_t* h) {
    if (!h) return ASR_ERR_ARG;
    if (h->d_blob) return ASR_OK;
    const asr_rnnt_desc& d = h->d;
    const size_t H4 = 4 * (size_t)d.Hp;
    // one allocation, every array at a 16-byte aligned offset (in floats: a multiple of 4)
    struct Piece {
        const std::vector<float>* v;
        const float** dst;
    };
    const float *d_emb = nullptr, *d_wih0 = nullptr;
    std::vector<Piece> pieces = {{&h->emb, &d_emb},        {&h->wih[0], &d_wih0},    {&h->wenc, &h->d_wenc},
                                 {&h->benc, &h->d_benc},   {&h->wpred, &h->d_wpred}, {&h->bpred, &h->d_bpred},
                                 {&h->wout, &h->d_wout},   {&h->bout, &h->d_bout}};
    for (int l = 0; l < d.L; l++) {
        if (l) pieces.push_back({&h->wih[l], &h->d_wih1});
        pieces.push_back({&h->whh[l], &h->d_whh[l]});
        pieces.push_back({&h->bih[l], &h->d_bih[l]});
        pieces.push_back({&h->bhh[l], &h->d_bhh[l]});
    }
    auto up4 = [](size_t n) { return (n + 3) & ~(size_t)3; };
    size_t total = up4((size_t)d.V * H4);   // Emb.W_ih of layer 0 first
    for (const Piece& pc : pieces) total += up4(pc.v->size());
    float* blob = nullptr;
    ASR_HIP_TRY(hipMalloc((void**)&blob, total * sizeof(float)));
    size_t off = up4((size_t)d.V * H4);
    hipError_t e = hipSuccess;
    for (const Piece& pc : pieces) {
        *pc.dst = blob + off;
        if (e == hipSuccess)
            e = hipMemcpy(blob + off, pc.v->data(), pc.v->size() * sizeof(float), hipMemcpyHostToDevice);
        off += up4(pc.v->size());
    }
    int rc = ASR_OK;
    if (e != hipSuccess) {
        asr_internal_set_error("hipMemcpy (RNN-T weights)", hipGetErrorString(e), __FILE__, __LINE__);
        rc = ASR_ERR_HIP;
    }
    if (rc == ASR_OK) {
        // x.W_ih of layer 0 for every token: asr_lstm_fwd's input projection of the rows of Emb
        asr::GemmArgs g{};
        g.A = d_emb; g.B = d_wih0; g.C = blob;
        g.M = d.V; g.N = (int)H4; g.K = d.D;
        g.sam = d.D; g.sak = 1; g.sbk = (long)H4; g.sbn = 1; g.ldc = (long)H4;
        rc = asr::gemm_launch(g, asr::EPI_NONE, nullptr);
        if (rc == ASR_OK && (e = hipStreamSynchronize(nullptr)) != hipSuccess) {
            asr_internal_set_error("hipStreamSynchronize (RNN-T upload)", hipGetErrorString(e), __FILE__, __LINE__);
            rc = ASR_ERR_HIP;
        }
    }
    if (rc != ASR_OK) {
        (void)hipFree(blob);
        return rc;
    }
    h->d_embw = blob;
    h->d_blob = blob;
    return ASR_OK;
}

size_t asr_rnnt_workspace_bytes(const asr_rnnt_t* h, int T, int B) {
    if (!h || T <= 0 || B <= 0 || (long)T * B > INT_MAX) return 0;
    const size_t tiles = ((size_t)B + asr::RT_ROWS - 1) / asr::RT_ROWS;
    // f [T*B][J], then per workgroup c [L][16][Hp] and g [16][J]
    return ((size_t)T * B * h->d.J + tiles * asr::RT_ROWS * ((size_t)h->d.L * h->d.Hp + h->d.J)) * sizeof(float);
}

int asr_rnnt_greedy(const asr_rnnt_t* h, const float* d_enc, const int32_t* d_lengths, int T, int B, int max_out,
                    const float* d_state_in, float* d_state_out, int32_t* d_tokens, int32_t* d_timesteps,
                    double* d_logp, int32_t* d_count, double* d_total, void* d_work, asr_stream_t s) {
    if (int rc = asr::rnnt_greedy_check(h, d_enc, T, B, max_out, d_tokens, d_timesteps, d_logp, d_count, d_total))
        return rc;
    if (!d_work) return ASR_ERR_ARG;
    if (!h->d_blob) return ASR_ERR_STATE;
    const asr_rnnt_desc& d = h->d;
    float* f = (float*)d_work;
    if (int rc = asr::rnnt_enc_launch(h, d_enc, T, B, f, asr_stream(s))) return rc;
    asr::RnntArgs a{};
    // the model's part from the one place that knows the handle; the kernel's argument layout stays its own
    const asr::RtNet net = asr::rnnt_net(h);
    a.f = f;
    a.embw = net.embw;
    a.wih1 = net.wih1;
    for (int l = 0; l < net.L; l++) {
        a.whh[l] = net.whh[l];
        a.bih[l] = net.bih[l];
        a.bhh[l] = net.bhh[l];
    }
    a.wpred = net.wpred; a.bpred = net.bpred; a.wout = net.wout; a.bout = net.bout;
    a.lengths = d_lengths; a.state_in = d_state_in; a.state_out = d_state_out;
    a.tokens = d_tokens; a.timesteps = d_timesteps; a.logp = d_logp; a.count = d_count; a.total = d_total;
    a.slices = f + (size_t)T * B * d.J;
    a.T = T; a.B = B; a.Hp = net.Hp; a.J = net.J; a.V = net.V; a.L = net.L; a.blank = net.blank; a.act = net.act;
    a.max_symbols = d.max_symbols; a.max_out = max_out;
    a.max_iters = T * (d.max_symbols + 1);   // the hard bound on joint evaluations per row
    static AsrAttrOnce attr;
    if (int rc = attr.set((const void*)asr::rnnt_greedy_kernel, asr::RT_LDS_MAX)) return rc;
    const unsigned gx = (unsigned)((B + asr::RT_ROWS - 1) / asr::RT_ROWS);
    hipLaunchKernelGGL(asr::rnnt_greedy_kernel, dim3(gx), dim3(64 * asr::RT_WAVES), (size_t)h->lds_bytes,
                       asr_stream(s), a);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

int asr_rnnt_greedy_host(const asr_rnnt_t* h, const float* h_enc, const int32_t* h_lengths, int T, int B, int max_out,
                         const double* h_state_in, double* h_state_out, int32_t* h_tokens, int32_t* h_timesteps,
                         double* h_logp, int32_t* h_count, double* h_total, double* h_gap) {
    if (int rc = asr::rnnt_greedy_check(h, h_enc, T, B, max_out, h_tokens, h_timesteps, h_logp, h_count, h_total))
        return rc;
    const asr_rnnt_desc& d = h->d;
    const size_t LH = (size_t)d.L * d.Hp, cbase = (size_t)d.L * B * d.Hp;
    try {
        asr::RnntHost m(*h);
        std::vector<double> hs(LH), cs(LH), logit(d.V);
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
                    m.step(k, hs.data(), cs.data());
                    m.pred_proj(hs.data());
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
