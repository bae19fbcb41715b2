// LSTM layer (torch.nn.LSTM semantics, one layer and direction per call):
// asr_lstm_workspace_bytes / asr_lstm_fwd / asr_lstm_recur_fwd.
//
// Weights in the project's [in][out] layout: W_ih [in][4H], W_hh [H][4H], gate
// q (i, f, g, o) of hidden unit j at column q*H + j.  P = x.W_ih for all T
// frames is one gemm_launch (EPI_NONE, N = 4H); each frame then computes
//   z = (P_t + h_{t-1}.W_hh) + (b_ih + b_hh)
//   i, f, o = sigmoid(z_i, z_f, z_o), g = tanh(z_g)
//   c_t = f*c_{t-1} + i*g,  h_t = o*tanh(c_t)
// with the contraction on v_mfma_f32_16x16x4_f32 (exact fp32).  A wave
// computes the i, f, g and o tiles of the SAME 16 hidden columns, so in the
// C-fragment layout (rows 4g + j, column lane & 15) a lane holds all four
// gates of its four (row, column) elements: the cell update is lane-local,
// c_t (and the carried h_t) stay in that lane, nothing is exchanged.
//
// The kernel depends on H only, never on B: an utterance's bits do not depend
// on the batch it runs in.
//   16 <= H <= 128  resident form: the whole recurrence in one launch
//                   (lstm_recur_kernel);
//   128 < H <= 2048 step form: one launch per frame (lstm_step_kernel),
//                   capturable in a graph.
// Neither waits on another workgroup; every loop is bounded by T or H.
//
// reverse: frames run T-1 .. 0 (an index map).  ldh: row stride of the output
// (>= H), so a forward and a reverse call fill the two halves of a [T*B][2H]
// buffer.  lengths (device int32 [B] or NULL): for frames t >= len_b the
// utterance's h and c are carried unchanged and its output row is zeros
// (pack_padded_sequence / pad_packed_sequence semantics; in reverse the
// utterance starts from h0 / c0 at its own last frame).
#include "dense.h"

#include <climits>
#include <cstddef>

namespace asr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Workgroup barrier ordering LDS only (dense.hip lds_barrier): the step's
// global stores and the prefetch of P_{t+1} stay in flight across it.
__device__ __forceinline__ void lstm_lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

__device__ __forceinline__ float lstm_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

constexpr int LS_ROWS = 16;                 // utterances per workgroup (one MFMA row tile)
constexpr int LR_HMAX = 128;                // resident form: H <= 128
constexpr int LR_LD = LR_HMAX + 4;          // LDS row stride (floats) of h
constexpr int LR_NCH = LR_HMAX / 16;        // 16-k chunks at H = 128
constexpr int LS_HMAX = 2048;               // step form: H <= 2048
constexpr int LS_WAVES = 4;                 // step form: j-tiles (waves) per workgroup
constexpr int LS_DEPTH = 3;                 // step form: 16-k chunks of fragments in flight per wave
// P_t is read through one buffer resource per frame (B*4H*4 bytes): lanes of
// rows past B get this offset (+ at most 3*H*4 for the gate), past the
// resource's size, so their loads return 0 without a branch.
constexpr int LSTM_OOB = 0x7ff00000;
constexpr int LSTM_RSRC3 = 0x00020000;      // gfx9 buffer descriptor word 3 (raw 32-bit data)

// One cell update of a lane's element: gates from z, then c and h.
struct LstmCell {
    float c, h;
};
__device__ __forceinline__ LstmCell lstm_cell(float zi, float zf, float zg, float zo, float cprev) {
    const float ig = lstm_sigmoid(zi), fg = lstm_sigmoid(zf), gg = tanhf(zg), og = lstm_sigmoid(zo);
    LstmCell r;
    r.c = fg * cprev + ig * gg;
    r.h = og * tanhf(r.c);
    return r;
}

// ---------------------------------------------------------------------------
// Resident form, 16 <= H <= 128 (H % 16 == 0), in the shape of
// rnn_recur_mfma_kernel: 16 utterances per workgroup, one wave per 16-column
// j-tile (block = 64 * H/16 threads, 8 waves at H = 128).  Wave w keeps the
// four gate tiles of its columns of W_hh in registers for all T: H/4 floats
// per lane and tile, 128 VGPRs at H = 128 (the tanh kernel's budget at
// H = 256), and issues 4 * H/4 MFMAs per step (128 at H = 128).  The four
// gates are four independent accumulator chains, so the dependent MFMA
// latency never stalls the issue.  h_{t-1} (16 x H) is double-buffered in
// LDS, one LDS-only barrier per step; MFMA (i, e) of lane group g contracts
// k = 16i + 4g + e, one ds_read_b128 per 16 k shared by the four gates.
// P_{t+1} is prefetched one step ahead.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64 * LR_NCH) void lstm_recur_kernel(const float* P, const float* __restrict__ h0,
                                                                 const float* __restrict__ c0,
                                                                 const float* __restrict__ Whh,
                                                                 const float* __restrict__ b_ih,
                                                                 const float* __restrict__ b_hh, float* hid, long ldh,
                                                                 float* hT, float* cT,
                                                                 const int32_t* __restrict__ lengths, int T, int B,
                                                                 int H, int reverse) {
    __shared__ __attribute__((aligned(16))) float hs[2][LS_ROWS * LR_LD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int nch = H >> 4;                 // 16-k chunks = waves
    const int r0 = blockIdx.x * LS_ROWS;
    const int n = 16 * w + c;               // this lane's hidden column
    const int H4 = 4 * H;
    // wb[q][i][e] = W_hh[16i + 4g + e][q*H + n]
    float wb[4][LR_NCH][4];
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int i = 0; i < LR_NCH; i++)
#pragma unroll
            for (int e = 0; e < 4; e++)
                wb[q][i][e] = i < nch ? Whh[(long)(16 * i + 4 * g + e) * H4 + q * H + n] : 0.f;
    float bias[4];
#pragma unroll
    for (int q = 0; q < 4; q++) bias[q] = b_ih[q * H + n] + b_hh[q * H + n];
    // this lane's four elements: rows r0 + 4g + j, column n
    bool ok[4];
    int len[4], voff[4];
    long orow[4];
    float hreg[4], creg[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int r = r0 + 4 * g + j;
        ok[j] = r < B;
        const int rr = ok[j] ? r : 0;
        len[j] = !ok[j] ? 0 : lengths ? min(max(lengths[rr], 0), T) : T;
        voff[j] = ok[j] ? (rr * H4 + n) * 4 : LSTM_OOB;
        orow[j] = (long)rr * ldh + n;
        hreg[j] = (ok[j] && h0) ? h0[(long)rr * H + n] : 0.f;
        creg[j] = (ok[j] && c0) ? c0[(long)rr * H + n] : 0.f;
        hs[0][(4 * g + j) * LR_LD + n] = hreg[j];
    }
    const long tstride = (long)B * H4;      // floats of P per frame
    const int nbytes = (int)(tstride * 4);
    const int gstep = H * 4;                // bytes from one gate's column to the next
    float* const Pw = const_cast<float*>(P);
    float pn[4][4];
    {
        const int t0 = reverse ? T - 1 : 0;
        const auto rs = __builtin_amdgcn_make_buffer_rsrc(Pw + t0 * tstride, 0, nbytes, LSTM_RSRC3);
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int j = 0; j < 4; j++)
                pn[q][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff[j] + q * gstep, 0, 0));
    }
    __syncthreads();
    int cur = 0;
    for (int s = 0; s < T; s++) {
        const int t = reverse ? T - 1 - s : s;
        float p[4][4];
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int j = 0; j < 4; j++) p[q][j] = pn[q][j];
        {
            // next frame's P (past the last step: an empty resource, zeros)
            const bool more = s + 1 < T;
            const int tn = more ? (reverse ? t - 1 : t + 1) : t;
            const auto rs = __builtin_amdgcn_make_buffer_rsrc(Pw + tn * tstride, 0, more ? nbytes : 0, LSTM_RSRC3);
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    pn[q][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff[j] + q * gstep, 0, 0));
        }
        const float* hrow = &hs[cur][c * LR_LD + 4 * g];
        f32x4 acc[4];
#pragma unroll
        for (int q = 0; q < 4; q++) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < LR_NCH; i++) {
            if (i < nch) {
                const float4 a = *reinterpret_cast<const float4*>(hrow + 16 * i);
#pragma unroll
                for (int q = 0; q < 4; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, wb[q][i][0], acc[q], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 4; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, wb[q][i][1], acc[q], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 4; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, wb[q][i][2], acc[q], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 4; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, wb[q][i][3], acc[q], 0, 0, 0);
            }
        }
        float* hn = hs[cur ^ 1];
        const long obase = (long)t * B * ldh;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const LstmCell r = lstm_cell((p[0][j] + acc[0][j]) + bias[0], (p[1][j] + acc[1][j]) + bias[1],
                                         (p[2][j] + acc[2][j]) + bias[2], (p[3][j] + acc[3][j]) + bias[3], creg[j]);
            const bool act = t < len[j];
            creg[j] = act ? r.c : creg[j];
            hreg[j] = act ? r.h : hreg[j];
            hn[(4 * g + j) * LR_LD + n] = hreg[j];   // the carried h feeds the next step
            if (ok[j]) hid[obase + orow[j]] = act ? r.h : 0.f;
        }
        cur ^= 1;
        lstm_lds_barrier();
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (!ok[j]) continue;
        const long x = (long)(r0 + 4 * g + j) * H + n;
        if (hT) hT[x] = hreg[j];
        if (cT) cT[x] = creg[j];
    }
}

// ---------------------------------------------------------------------------
// Step form, 128 < H <= 2048 (H % 16 == 0): one launch per frame.  Grid
// (ceil(B / 16) row tiles, ceil(H/16 / 4) groups of j-tiles), 4 waves per
// workgroup, wave w of group y owns j-tile 4y + w for all four gates.  The A
// fragments (h_{t-1}, rows of the tile) come straight from memory as 16-byte
// loads (the group's waves read the same lines), the B fragments are the
// wave's own columns of W_hh.  h_{t-1} of utterance b is the output row of
// the frame it last ran in (the previous frame, or its last valid one when
// this frame is past its length), or h0 before its first: the carried h needs
// no copy.  c is read and written in place in the workspace by the lane that
// owns the element (cin: c0 / NULL at the first step, the workspace after).
// No LDS, no barrier, nothing shared between workgroups within a launch:
// frame t's launch reads frame t -/+ 1's rows and writes frame t's.
// ---------------------------------------------------------------------------
// The row that holds utterance r's h before frame t runs (NULL: zeros).
__device__ __forceinline__ const float* lstm_h_before(const float* hid, long ldh, const float* h0, int t, int r,
                                                      int len, int B, int H, int reverse) {
    const int tp = reverse ? (t + 1 < len ? t + 1 : -1) : min(t, len) - 1;
    if (tp >= 0) return hid + ((long)tp * B + r) * ldh;
    return h0 ? h0 + (long)r * H : nullptr;
}

__global__ __launch_bounds__(64 * LS_WAVES) void lstm_step_kernel(const float* P, const float* __restrict__ h0,
                                                                  const float* cin, float* cout,
                                                                  const float* __restrict__ Whh,
                                                                  const float* __restrict__ b_ih,
                                                                  const float* __restrict__ b_hh, float* hid, long ldh,
                                                                  float* hT, float* cT,
                                                                  const int32_t* __restrict__ lengths, int t, int T,
                                                                  int B, int H, int reverse, int last) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int nch = H >> 4;
    const int tile = blockIdx.y * LS_WAVES + w;
    if (tile >= nch) return;                // no barrier below
    const int r0 = blockIdx.x * LS_ROWS;
    const int n = 16 * tile + c;
    const int H4 = 4 * H;
    // A fragments: row c of the tile (clamped: rows past B feed only their own, unused, results)
    const int ra = min(r0 + c, B - 1);
    const int lena = lengths ? min(max(lengths[ra], 0), T) : T;
    const float* hsrc = lstm_h_before(hid, ldh, h0, t, ra, lena, B, H, reverse);
    const bool hz = hsrc == nullptr;        // zeros: load from a valid address, then discard
    const float* ap = (hz ? Whh : hsrc) + 4 * g;
    const float* bp = Whh + (long)(4 * g) * H4 + n;
    f32x4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    // The fragments of chunk i + LS_DEPTH are loaded while chunk i's MFMAs
    // issue (a ring of LS_DEPTH register stages, 17 loads each; loads past
    // the last chunk re-read it and are not used).
    float4 a[LS_DEPTH];
    float b[LS_DEPTH][4][4];
    auto fetch = [&](int u, int i) {
        const int ii = min(i, nch - 1);
        a[u] = *reinterpret_cast<const float4*>(ap + 16 * ii);
        const float* bi = bp + (long)(16 * ii) * H4;
#pragma unroll
        for (int e = 0; e < 4; e++)
#pragma unroll
            for (int q = 0; q < 4; q++) b[u][e][q] = bi[(long)e * H4 + q * H];
    };
#pragma unroll
    for (int u = 0; u < LS_DEPTH; u++) fetch(u, u);
    for (int i0 = 0; i0 < nch; i0 += LS_DEPTH) {
#pragma unroll
        for (int u = 0; u < LS_DEPTH; u++) {
            if (i0 + u < nch) {
                const float4 x = hz ? float4{0.f, 0.f, 0.f, 0.f} : a[u];
#pragma unroll
                for (int q = 0; q < 4; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, b[u][0][q], acc[q], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 4; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, b[u][1][q], acc[q], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 4; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, b[u][2][q], acc[q], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 4; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, b[u][3][q], acc[q], 0, 0, 0);
            }
            fetch(u, i0 + u + LS_DEPTH);
        }
    }
    float bias[4];
#pragma unroll
    for (int q = 0; q < 4; q++) bias[q] = b_ih[q * H + n] + b_hh[q * H + n];
    const long tstride = (long)B * H4;
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(P) + t * tstride, 0, (int)(tstride * 4),
                                                      LSTM_RSRC3);
    const int gstep = H * 4;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int r = r0 + 4 * g + j;
        const bool ok = r < B;
        const int rr = ok ? r : 0;
        const int voff = ok ? (rr * H4 + n) * 4 : LSTM_OOB;
        float p[4];
#pragma unroll
        for (int q = 0; q < 4; q++)
            p[q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff + q * gstep, 0, 0));
        if (!ok) continue;
        const int len = lengths ? min(max(lengths[r], 0), T) : T;
        const long x = (long)r * H + n;
        const float cold = cin ? cin[x] : 0.f;
        const LstmCell u = lstm_cell((p[0] + acc[0][j]) + bias[0], (p[1] + acc[1][j]) + bias[1],
                                     (p[2] + acc[2][j]) + bias[2], (p[3] + acc[3][j]) + bias[3], cold);
        const bool act = t < len;
        const float cnew = act ? u.c : cold;
        cout[x] = cnew;
        hid[((long)t * B + r) * ldh + n] = act ? u.h : 0.f;
        if (last) {
            if (cT) cT[x] = cnew;
            if (hT) {
                float hc = u.h;
                if (!act) {
                    const float* hb = lstm_h_before(hid, ldh, h0, t, r, len, B, H, reverse);
                    hc = hb ? hb[n] : 0.f;
                }
                hT[x] = hc;
            }
        }
    }
}

static bool lstm_shape_ok(int H) { return H > 0 && (H & 15) == 0 && H <= LS_HMAX; }

static int lstm_recur_launch(const float* P, const float* h0, const float* c0, const float* Whh, const float* b_ih,
                             const float* b_hh, float* hid, long ldh, float* hT, float* cT, const int32_t* lengths,
                             float* cwork, int T, int B, int H, int reverse, hipStream_t s) {
    const unsigned gx = (unsigned)((B + LS_ROWS - 1) / LS_ROWS);
    if (H <= LR_HMAX) {
        hipLaunchKernelGGL(lstm_recur_kernel, dim3(gx), dim3(64 * (H / 16)), 0, s, P, h0, c0, Whh, b_ih, b_hh, hid,
                           ldh, hT, cT, lengths, T, B, H, reverse);
        ASR_LAUNCH_TRY();
        return ASR_OK;
    }
    const unsigned gy = (unsigned)((H / 16 + LS_WAVES - 1) / LS_WAVES);
    for (int k = 0; k < T; k++) {
        const int t = reverse ? T - 1 - k : k;
        hipLaunchKernelGGL(lstm_step_kernel, dim3(gx, gy), dim3(64 * LS_WAVES), 0, s, P, h0, k ? cwork : c0, cwork,
                           Whh, b_ih, b_hh, hid, ldh, hT, cT, lengths, t, T, B, H, reverse, k == T - 1 ? 1 : 0);
        ASR_LAUNCH_TRY();
    }
    return ASR_OK;
}

// The shape checks of both entry points, ahead of any HIP call.
static int lstm_check(const void* work, long ldh, int T, int B, int H, const float* hid, const float* h0) {
    if (T <= 0 || B <= 0 || H <= 0 || ldh < H) return ASR_ERR_ARG;
    if (!lstm_shape_ok(H)) return ASR_ERR_UNSUPPORTED;
    if ((long)B * 4 * H * 4 > (long)LSTM_OOB) return ASR_ERR_UNSUPPORTED;   // one frame of P per buffer resource
    if ((long)T * B > INT_MAX) return ASR_ERR_UNSUPPORTED;
    if (H > LR_HMAX) {
        if (!work) return ASR_ERR_ARG;      // c lives there
        // the step form reads h_{t-1} rows with 16-byte loads
        if ((ldh & 3) != 0 || ((uintptr_t)hid & 15) != 0 || ((uintptr_t)h0 & 15) != 0) return ASR_ERR_UNSUPPORTED;
    }
    return ASR_OK;
}

}  // namespace asr

extern "C" {

size_t asr_lstm_workspace_bytes(int T, int B, int H) {
    if (T <= 0 || B <= 0 || !asr::lstm_shape_ok(H)) return 0;
    // P [T*B][4H], then the step form's c [B][H] (H % 16 == 0: a multiple of 16 bytes)
    return ((size_t)T * B * 4 * H + (size_t)B * H) * sizeof(float);
}

int asr_lstm_recur_fwd(const float* P, const float* h0, const float* c0, const float* W_hh, const float* b_ih,
                       const float* b_hh, float* hid, long ldh, float* hT, float* cT, const int32_t* lengths,
                       void* work, int T, int B, int H, int reverse, asr_stream_t s) {
    if (!P || !W_hh || !b_ih || !b_hh || !hid) return ASR_ERR_ARG;
    if (int rc = asr::lstm_check(work,ldh, T, B, H, hid, h0)) return rc;
    float* cwork = work ? (float*)work + (size_t)T * B * 4 * H : nullptr;
    return asr::lstm_recur_launch(P, h0, c0, W_hh, b_ih, b_hh, hid, ldh, hT, cT, lengths, cwork, T, B, H,
                                  reverse ? 1 : 0, asr_stream(s));
}

int asr_lstm_fwd(const float* x, const float* h0, const float* c0, const float* W_ih, const float* W_hh,
                 const float* b_ih, const float* b_hh, float* hid, long ldh, float* hT, float* cT,
                 const int32_t* lengths, void* work, int T, int B, int in, int H, int reverse, asr_stream_t s) {
    if (!x || !W_ih || !W_hh || !b_ih || !b_hh || !hid || !work || in <= 0) return ASR_ERR_ARG;
    if (int rc = asr::lstm_check(work,ldh, T, B, H, hid, h0)) return rc;
    // P = x.W_ih for all T frames: asr_linear_fwd(x, W_ih, NULL, P, T*B, in, 4H, ASR_EPI_NONE)
    asr::GemmArgs g{};
    g.A = x; g.B = W_ih; g.C = (float*)work;
    g.M = T * B; g.N = 4 * H; g.K = in;
    g.sam = in; g.sak = 1; g.sbk = 4 * H; g.sbn = 1; g.ldc = 4 * H;
    if (int rc = asr::gemm_launch(g, asr::EPI_NONE, asr_stream(s))) return rc;
    return asr_lstm_recur_fwd((const float*)work, h0, c0, W_hh, b_ih, b_hh, hid, ldh, hT, cT, lengths, work, T, B, H,
                              reverse, s);
}

}  // extern "C"
