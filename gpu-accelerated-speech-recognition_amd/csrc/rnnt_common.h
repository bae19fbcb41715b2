// The transducer's network for rnnt.hip (greedy), rnnt_beam.hip (beam search,
// with and without an LM) and rnnt_align.hip (lattice scoring): the handle,
// the model's device pointers (RtNet) and the host side of a launch; on the
// device the MFMA column-tile product with its register ring (rt_mma), the
// schedule of the column tiles over the waves (rt_sweep), the running (max,
// argmax, sum-exp) of a row with its reduction (RtTop, rt_row_partial,
// rt_row_total) and the LSTM predictor step (rt_lstm_step); and the fp64 host
// model.  A row's bits depend on the model's shape only, so the k order and the
// tile-to-wave map are the same in every kernel.  The beam kernel calls all of
// it; rnnt_greedy_kernel and rnnt_joint_kernel call rt_mma and keep their own
// text of the schedule, the reduction and the step, for a measured reason
// (DESIGN.md §29): a change here is a change there.
#pragma once
#include "dense.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <vector>

struct asr_rnnt {
    asr_rnnt_desc d{};
    std::vector<float> emb, wih[ASR_RNNT_MAX_LAYERS], whh[ASR_RNNT_MAX_LAYERS], bih[ASR_RNNT_MAX_LAYERS],
        bhh[ASR_RNNT_MAX_LAYERS], wenc, benc, wpred, bpred, wout, bout;
    int lds_bytes = 0;
    int64_t weight_bytes = 0;
    // device copy (asr_rnnt_upload): one allocation
    float* d_blob = nullptr;
    const float *d_embw = nullptr, *d_wih1 = nullptr, *d_whh[ASR_RNNT_MAX_LAYERS] = {}, *d_bih[ASR_RNNT_MAX_LAYERS] = {},
                *d_bhh[ASR_RNNT_MAX_LAYERS] = {}, *d_wenc = nullptr, *d_benc = nullptr, *d_wpred = nullptr,
                *d_bpred = nullptr, *d_wout = nullptr, *d_bout = nullptr;
};

namespace asr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RT_ROWS = 16;     // rows per workgroup (one MFMA row tile)
constexpr int RT_WAVES = 8;     // waves per workgroup; column tile j belongs to wave j % 8
constexpr int RT_DEPTH = 3;     // 16-k chunks of fragments in flight per wave
constexpr int RT_NONE = INT_MAX;    // argmax of an empty set
constexpr int RT_LDS_SMALL = 4096;  // bytes the greedy kernel keeps for the per-row walk state and the wave partials
constexpr int RT_LDS_MAX = 160 * 1024;

// LDS bytes of a decode kernel: h [2][L][16][Hp + 4], z [16][J + 4], then its small area.
static long rnnt_lds_bytes(int L, int Hp, int J, int small) {
    return ((long)2 * L * (Hp + 4) + (J + 4)) * RT_ROWS * 4 + small;
}

// The model as the kernels take it: the device pointers of an uploaded handle and its shape.
struct RtNet {
    const float* embw;       // [V][4Hp] = Emb.W_ih of layer 0
    const float* wih1;       // [Hp][4Hp], layer 1 (L = 2)
    const float* whh[2];
    const float* bih[2];
    const float* bhh[2];
    const float* wpred;
    const float* bpred;
    const float* wout;
    const float* bout;
    int Hp, J, V, L, blank, act;
};
static RtNet rnnt_net(const asr_rnnt* h) {
    RtNet n{};
    n.embw = h->d_embw;
    n.wih1 = h->d_wih1;
    for (int l = 0; l < h->d.L; l++) {
        n.whh[l] = h->d_whh[l];
        n.bih[l] = h->d_bih[l];
        n.bhh[l] = h->d_bhh[l];
    }
    n.wpred = h->d_wpred; n.bpred = h->d_bpred; n.wout = h->d_wout; n.bout = h->d_bout;
    n.Hp = h->d.Hp; n.J = h->d.J; n.V = h->d.V; n.L = h->d.L; n.blank = h->d.blank; n.act = h->d.act;
    return n;
}

// f [T*B][J] = enc.W_enc + b_enc for all frames: one gemm_launch, the bias fused.
static int rnnt_enc_launch(const asr_rnnt* h, const float* d_enc, int T, int B, float* f, hipStream_t st) {
    const asr_rnnt_desc& d = h->d;
    GemmArgs g{};
    g.A = d_enc; g.B = h->d_wenc; g.b1 = h->d_benc; g.C = f;
    g.M = T * B; g.N = d.J; g.K = d.E;
    g.sam = d.E; g.sak = 1; g.sbk = d.J; g.sbn = 1; g.ldc = d.J;
    return gemm_launch(g, EPI_BIAS, st);
}

__device__ __forceinline__ float rt_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }
__device__ __forceinline__ float rt_act(float x, int act) { return act ? tanhf(x) : fmaxf(x, 0.f); }

// acc[rt][q] += A_rt(16 x 16*nch) . W[:, col[q]] for NRT row tiles and the lane's
// column of NQ tiles.  a: this lane's row of tile 0 of A in LDS at k = 4g (row c
// of the tile); tile rt is rts floats further; W: the matrix.  MFMA (i, e) of
// lane group g contracts k = 16i + 4g + e, as in gated_rnn.hip; the fragments of
// chunk i + RT_DEPTH load while chunk i's MFMAs issue (loads past the last chunk
// re-read it and are not used), and every W fragment feeds NRT MFMAs.
template <int NRT, int NQ>
__device__ __forceinline__ void rt_mma(const float* a, int rts, int nch, const float* __restrict__ W, unsigned ldw,
                                       int g, const int (&col)[NQ], f32x4 (&acc)[NRT][NQ]) {
    // one uniform base per k row and a 32-bit lane offset per tile
    unsigned off[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) off[q] = 4u * g * ldw + (unsigned)col[q];
    float4 av[RT_DEPTH][NRT];
    float bv[RT_DEPTH][4][NQ];
    auto fetch = [&](int u, int i) {
        const int ii = min(i, nch - 1);
#pragma unroll
        for (int rt = 0; rt < NRT; rt++) av[u][rt] = *reinterpret_cast<const float4*>(a + rt * rts + 16 * ii);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float* be = W + (size_t)(16 * ii + e) * ldw;
#pragma unroll
            for (int q = 0; q < NQ; q++) bv[u][e][q] = be[off[q]];
        }
    };
#pragma unroll
    for (int u = 0; u < RT_DEPTH; u++) fetch(u, u);
    for (int i0 = 0; i0 < nch; i0 += RT_DEPTH) {
#pragma unroll
        for (int u = 0; u < RT_DEPTH; u++) {
            if (i0 + u < nch) {
#pragma unroll
                for (int rt = 0; rt < NRT; rt++) {
                    const float4 x = av[u][rt];
#pragma unroll
                    for (int q = 0; q < NQ; q++)
                        acc[rt][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, bv[u][0][q], acc[rt][q], 0, 0, 0);
#pragma unroll
                    for (int q = 0; q < NQ; q++)
                        acc[rt][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, bv[u][1][q], acc[rt][q], 0, 0, 0);
#pragma unroll
                    for (int q = 0; q < NQ; q++)
                        acc[rt][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, bv[u][2][q], acc[rt][q], 0, 0, 0);
#pragma unroll
                    for (int q = 0; q < NQ; q++)
                        acc[rt][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, bv[u][3][q], acc[rt][q], 0, 0, 0);
                }
            }
            fetch(u, i0 + u + RT_DEPTH);
        }
    }
}

// NQ column tiles t0, t0 + 8, ... of A . W + bias: sink(rt, n, x) gets column n's
// finished values of the lane's four rows 4g .. 4g + 3 of row tile rt.  PARTIAL:
// ncols need not be a multiple of 16; a lane past the end loads the last column
// and sinks nothing.
template <int NRT, int NQ, bool PARTIAL, class Sink>
__device__ __forceinline__ void rt_tiles(const float* a, int rts, int nch, const float* __restrict__ W,
                                         const float* __restrict__ bias, int ncols, int t0, int g, int c, Sink& sink) {
    int n[NQ], col[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        n[q] = 16 * (t0 + q * RT_WAVES) + c;
        col[q] = PARTIAL ? min(n[q], ncols - 1) : n[q];
    }
    f32x4 acc[NRT][NQ];
#pragma unroll
    for (int rt = 0; rt < NRT; rt++)
#pragma unroll
        for (int q = 0; q < NQ; q++) acc[rt][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    rt_mma<NRT, NQ>(a, rts, nch, W, (unsigned)ncols, g, col, acc);
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        if (PARTIAL && n[q] >= ncols) continue;
        const float b = bias[n[q]];
#pragma unroll
        for (int rt = 0; rt < NRT; rt++) sink(rt, n[q], acc[rt][q] + b);
    }
}

// A(16 NRT x 16 nch) . W(16 nch x ncols) + bias by the workgroup's 8 waves, the
// schedule every kernel shares: column tile j belongs to wave j % 8 (w: this
// wave); of each run of 32 tiles a wave takes its four in one rt_mma while all
// four exist, else its tiles one by one.  a, rts: as rt_mma; sink: as rt_tiles.
template <int NRT, bool PARTIAL, class Sink>
__device__ __forceinline__ void rt_sweep(const float* a, int rts, int nch, const float* __restrict__ W,
                                         const float* __restrict__ bias, int ncols, int w, int g, int c, Sink sink) {
    const int nt = (ncols + 15) >> 4;
    for (int base = 0; base < nt; base += 4 * RT_WAVES) {
        const int t0 = base + w;
        const int nv = t0 < nt ? min(4, (nt - 1 - t0) / RT_WAVES + 1) : 0;
        if (nv == 4) {
            rt_tiles<NRT, 4, PARTIAL>(a, rts, nch, W, bias, ncols, t0, g, c, sink);
        } else {
            for (int q = 0; q < nv; q++)
                rt_tiles<NRT, 1, PARTIAL>(a, rts, nch, W, bias, ncols, t0 + q * RT_WAVES, g, c, sink);
        }
    }
}

// Running (max, lowest argmax, sum of exp(x - max)) of a row.
struct RtTop {
    float m, s;
    int i;
};
__device__ __forceinline__ void rt_push(RtTop& a, float x, int n) {
    if (x > a.m) {
        a.s = (a.s == 0.f ? 0.f : a.s * expf(a.m - x)) + 1.f;
        a.m = x;
        a.i = n;
    } else {
        a.s += x == a.m ? 1.f : expf(x - a.m);
        if (x == a.m && n < a.i) a.i = n;
    }
}
// Symmetric in its arguments, bit for bit (both partners of a shuffle get the same result).
__device__ __forceinline__ RtTop rt_join(const RtTop& a, const RtTop& b) {
    RtTop r;
    r.m = b.m > a.m ? b.m : a.m;
    r.i = b.m > a.m ? b.i : (b.m == a.m ? min(a.i, b.i) : a.i);
    const float sa = a.s == 0.f ? 0.f : (a.m == r.m ? a.s : a.s * expf(a.m - r.m));
    const float sb = b.s == 0.f ? 0.f : (b.m == r.m ? b.s : b.s * expf(b.m - r.m));
    r.s = sa + sb;
    return r;
}

// The row reduction, first half: the 16 lanes that hold a row's columns join,
// and lane c == 0 leaves the wave's partial at [slot] (slot = wave * rows + row).
// ARGMAX = false: every index is 0 and neither travels nor is stored.
template <bool ARGMAX>
__device__ __forceinline__ void rt_row_partial(RtTop t, int c, int slot, float* red_m, float* red_s, int* red_i) {
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) {
        RtTop o;
        o.m = __shfl_xor(t.m, d);
        o.s = __shfl_xor(t.s, d);
        o.i = ARGMAX ? __shfl_xor(t.i, d) : 0;
        t = rt_join(t, o);
    }
    if (c == 0) {
        red_m[slot] = t.m;
        red_s[slot] = t.s;
        if (ARGMAX) red_i[slot] = t.i;
    }
}
// Second half, one thread per row after a barrier: the 8 waves' partials in the order 0..7.
template <bool ARGMAX>
__device__ __forceinline__ RtTop rt_row_total(int row, int rows, const float* red_m, const float* red_s,
                                              const int* red_i) {
    RtTop a{red_m[row], red_s[row], ARGMAX ? red_i[row] : 0};
    for (int x = 1; x < RT_WAVES; x++)
        a = rt_join(a, RtTop{red_m[x * rows + row], red_s[x * rows + row], ARGMAX ? red_i[x * rows + row] : 0});
    return a;
}

// One LSTM predictor step of the workgroup's 16 rows, every layer.  New row r
// takes the state of row prow(r): its h from hb(cur, l) in LDS, its c from
// cold; with tok(r) >= 0 it steps on Emb[tok(r)], else it copies both.  The new
// h goes to hb(cur ^ 1, l), the new c to cnew, which may be cold when prow is
// the identity (the lane that reads an element is then the one that writes it).
// Ends behind a barrier; the caller flips cur.
template <class Hb, class Prow, class Tok>
__device__ __forceinline__ void rt_lstm_step(const RtNet& net, Hb hb, int cur, const float* cold, float* cnew,
                                             Prow prow, Tok tok, int w, int g, int c) {
    const int Hp = net.Hp, H4 = 4 * Hp, LDH = Hp + 4;
    const int prc = prow(c);
    for (int l = 0; l < net.L; l++) {
        const float* hold = hb(cur, l);
        float* hnew = hb(cur ^ 1, l);
        const float* Whh = net.whh[l];
        for (int jt = w; jt < (Hp >> 4); jt += RT_WAVES) {
            const int n = 16 * jt + c;
            const int col[4] = {n, Hp + n, 2 * Hp + n, 3 * Hp + n};
            f32x4 acc[1][4], accx[1][4];
#pragma unroll
            for (int q = 0; q < 4; q++) acc[0][q] = accx[0][q] = f32x4{0.f, 0.f, 0.f, 0.f};
            rt_mma<1, 4>(hold + prc * LDH + 4 * g, 0, Hp >> 4, Whh, H4, g, col, acc);
            if (l > 0)   // x = the layer below's new h, already in the new rows' order
                rt_mma<1, 4>(hb(cur ^ 1, l - 1) + c * LDH + 4 * g, 0, Hp >> 4, net.wih1, H4, g, col, accx);
            float bias[4];
#pragma unroll
            for (int q = 0; q < 4; q++) bias[q] = net.bih[l][col[q]] + net.bhh[l][col[q]];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int row = 4 * g + j, pr = prow(row), tk = tok(row);
                const bool em = tk >= 0;
                float px[4];
                if (l == 0) {
                    const float* e = net.embw + (unsigned)(max(tk, 0) * H4);   // V * 4Hp <= INT_MAX
#pragma unroll
                    for (int q = 0; q < 4; q++) px[q] = e[col[q]];
                } else {
#pragma unroll
                    for (int q = 0; q < 4; q++) px[q] = accx[0][q][j];
                }
                const float co = cold[(unsigned)((l * RT_ROWS + pr) * Hp + n)];
                const float zi = (px[0] + acc[0][0][j]) + bias[0], zf = (px[1] + acc[0][1][j]) + bias[1];
                const float zg = (px[2] + acc[0][2][j]) + bias[2], zo = (px[3] + acc[0][3][j]) + bias[3];
                const float ig = rt_sigmoid(zi), fg = rt_sigmoid(zf), gg = tanhf(zg), og = rt_sigmoid(zo);
                const float cn = fg * co + ig * gg;
                const float hn = og * tanhf(cn);
                cnew[(unsigned)((l * RT_ROWS + row) * Hp + n)] = em ? cn : co;
                hnew[row * LDH + n] = em ? hn : hold[pr * LDH + n];
            }
        }
        __syncthreads();   // layer l's new h, before layer l + 1 and g read it
    }
}

// ---------------------------------------------------------------------------
// Host model: one thread, fp64 accumulation from the fp32 weights.
// ---------------------------------------------------------------------------
struct RnntHost {
    const asr_rnnt& m;
    std::vector<double> gates, gx, x, g, f, z;
    explicit RnntHost(const asr_rnnt& mm) : m(mm) {
        const int in = std::max(m.d.D, m.d.Hp);
        gates.resize(4 * (size_t)m.d.Hp);
        gx.resize(4 * (size_t)m.d.Hp);
        x.resize(in);
        g.resize(m.d.J);
        f.resize(m.d.J);
        z.resize(m.d.J);
    }
    // y[n] = sum_k x[k] * W[k][n], k ascending
    static void matvec(const double* x, const float* W, int K, int N, double* y) {
        for (int n = 0; n < N; n++) y[n] = 0.0;
        for (int k = 0; k < K; k++) {
            const double xv = x[k];
            const float* row = W + (size_t)k * N;
            for (int n = 0; n < N; n++) y[n] += xv * (double)row[n];
        }
    }
    static double sigmoid(double v) { return 1.0 / (1.0 + std::exp(-v)); }
    // one predictor step on Emb[tok]; h, c: [L][Hp]
    void step(int tok, double* h, double* c) {
        const int Hp = m.d.Hp;
        int in = m.d.D;
        for (int k = 0; k < in; k++) x[k] = (double)m.emb[(size_t)tok * in + k];
        for (int l = 0; l < m.d.L; l++) {
            matvec(x.data(), m.wih[l].data(), in, 4 * Hp, gx.data());
            matvec(h + (size_t)l * Hp, m.whh[l].data(), Hp, 4 * Hp, gates.data());
            for (int n = 0; n < 4 * Hp; n++)
                gates[n] = (gx[n] + gates[n]) + ((double)m.bih[l][n] + (double)m.bhh[l][n]);
            for (int n = 0; n < Hp; n++) {
                const double ig = sigmoid(gates[n]), fg = sigmoid(gates[Hp + n]), gg = std::tanh(gates[2 * Hp + n]),
                             og = sigmoid(gates[3 * Hp + n]);
                const double cn = fg * c[(size_t)l * Hp + n] + ig * gg;
                c[(size_t)l * Hp + n] = cn;
                h[(size_t)l * Hp + n] = og * std::tanh(cn);
            }
            in = Hp;
            for (int k = 0; k < in; k++) x[k] = h[(size_t)l * Hp + k];
        }
    }
    void pred_proj(const double* h) {
        matvec(h + (size_t)(m.d.L - 1) * m.d.Hp, m.wpred.data(), m.d.Hp, m.d.J, g.data());
        for (int n = 0; n < m.d.J; n++) g[n] += (double)m.bpred[n];
    }
    void enc_proj(const float* e) {
        std::vector<double> ev(e, e + m.d.E);
        matvec(ev.data(), m.wenc.data(), m.d.E, m.d.J, f.data());
        for (int n = 0; n < m.d.J; n++) f[n] += (double)m.benc[n];
    }
    // logit [V] = act(f + gv).W_out + b_out: the joint at the frame of the last enc_proj and a pred_proj's gv
    void logits(const double* gv, double* logit) {
        for (int j = 0; j < m.d.J; j++) {
            const double v = f[j] + gv[j];
            z[j] = m.d.act == ASR_RNNT_ACT_TANH ? std::tanh(v) : (v > 0.0 ? v : 0.0);
        }
        matvec(z.data(), m.wout.data(), m.d.J, m.d.V, logit);
        for (int v = 0; v < m.d.V; v++) logit[v] += (double)m.bout[v];
    }
};

}  // namespace asr
