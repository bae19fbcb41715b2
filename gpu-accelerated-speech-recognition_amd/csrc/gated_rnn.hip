// LSTM and GRU layers (torch.nn.LSTM / torch.nn.GRU semantics, one layer and
// direction per call): asr_lstm_workspace_bytes / asr_lstm_fwd /
// asr_lstm_recur_fwd and asr_gru_workspace_bytes / asr_gru_fwd /
// asr_gru_recur_fwd.  One gated recurrence, written once over a cell type
// (LstmCell, GruCell) that carries what differs between the two layers.
//
// Weights in the project's [in][out] layout, NG gates: W_ih [in][NG*H], W_hh
// [H][NG*H], gate q of hidden unit j at column q*H + j (LSTM: i, f, g, o; GRU:
// r, z, n).  P = x.W_ih for all T frames is one gemm_launch (EPI_NONE, N =
// NG*H); with a = h_{t-1}.W_hh each frame then computes, in this operation
// order in both kernels,
//   LSTM  z   = (P_t + a) + (b_ih + b_hh)
//         i, f, o = sigmoid(z_i, z_f, z_o), g = tanh(z_g)
//         c_t = f*c_{t-1} + i*g,  h_t = o*tanh(c_t)
//   GRU   r   = sigmoid((P_r + a_r) + (b_ir + b_hr))
//         z   = sigmoid((P_z + a_z) + (b_iz + b_hz))
//         n   = tanh((P_n + b_in) + r * (a_n + b_hn))
//         h_t = n + z * (h_{t-1} - n)              ( = (1 - z) n + z h_{t-1} )
// The GRU's reset gate multiplies the hidden contribution of the candidate
// only, so a_n is an accumulator of its own that starts from zero and never
// meets P_n, and b_in / b_hn are not pre-added; r and z use the same code
// shape.  The GRU has no cell state, hence no workspace beyond P.
//
// The contraction runs on v_mfma_f32_16x16x4_f32 (exact fp32).  A wave
// computes the NG gate tiles of the SAME 16 hidden columns, so in the
// C-fragment layout (rows 4g + j, column lane & 15) a lane holds all gates of
// its four (row, column) elements: gates and update are lane-local, c_t (and
// the carried h_t) stay in that lane, nothing is exchanged.  The gate tiles
// are NG independent accumulator chains (the MFMA's 40-cycle dependent latency
// against its 32-cycle issue needs two), so the dependent MFMA latency never
// stalls the issue.
//
// The kernel depends on H only, never on B: an utterance's bits do not depend
// on the batch it runs in.
//   16 <= H <= 128  resident form: the whole recurrence in one launch
//                   (gated_recur_kernel);
//   128 < H <= 2048 step form: one launch per frame (gated_step_kernel),
//                   capturable in a graph.
// Neither waits on another workgroup; every loop is bounded by T or H.
//
// reverse: frames run T-1 .. 0 (an index map).  ldh: row stride of the output
// (>= H), so a forward and a reverse call fill the two halves of a [T*B][2H]
// buffer.  lengths (device int32 [B] or NULL): for frames t >= len_b the
// utterance's h (and c) are carried unchanged and its output row is zeros
// (pack_padded_sequence / pad_packed_sequence semantics; in reverse the
// utterance starts from h0 / c0 at its own last frame).
#include "dense.h"

#include <climits>
#include <cstddef>

namespace asr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Workgroup barrier ordering LDS only (dense.hip lds_barrier): the step's
// global stores and the prefetch of P_{t+1} stay in flight across it.
__device__ __forceinline__ void gated_lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

__device__ __forceinline__ float gated_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

constexpr int GR_ROWS = 16;                 // utterances per workgroup (one MFMA row tile)
constexpr int GR_RHMAX = 128;               // resident form: H <= 128
constexpr int GR_LD = GR_RHMAX + 4;         // LDS row stride (floats) of h
constexpr int GR_NCH = GR_RHMAX / 16;       // 16-k chunks at H = 128
constexpr int GR_HMAX = 2048;               // step form: H <= 2048
constexpr int GR_WAVES = 4;                 // step form: j-tiles (waves) per workgroup
constexpr int GR_DEPTH = 3;                 // step form: 16-k chunks of fragments in flight per wave
// P_t is read through one buffer resource per frame (B*NG*H*4 bytes): lanes of
// rows past B get this offset (+ at most (NG-1)*H*4 for the gate), past the
// resource's size, so their loads return 0 without a branch.
constexpr int GR_OOB = 0x7ff00000;
constexpr int GR_RSRC3 = 0x00020000;        // gfx9 buffer descriptor word 3 (raw 32-bit data)

// A cell type holds the biases of a lane's hidden column and gives
//   NG      the gate count;
//   HAS_C   whether a cell state c is carried beside h;
//   AHEAD   step form: whether the lane's P_t and state element are requested
//           ahead of the contraction or after it;
//   load    the biases of column n;
//   update  one cell update of a lane's element: p[q] from P_t, a[q] from
//           h_{t-1}.W_hh, hprev = h_{t-1}; c is c_{t-1} on entry and c_t on
//           return; returns h_t.
struct LstmCell {
    static constexpr int NG = 4;
    static constexpr bool HAS_C = true;
    static constexpr bool AHEAD = false;
    float b[4];                             // b_ih + b_hh of i, f, g, o
    __device__ __forceinline__ void load(const float* __restrict__ b_ih, const float* __restrict__ b_hh, int H,
                                         int n) {
#pragma unroll
        for (int q = 0; q < 4; q++) b[q] = b_ih[q * H + n] + b_hh[q * H + n];
    }
    __device__ __forceinline__ float update(const float (&p)[4], const float (&a)[4], float, float& c) const {
        const float ig = gated_sigmoid((p[0] + a[0]) + b[0]), fg = gated_sigmoid((p[1] + a[1]) + b[1]),
                    gg = tanhf((p[2] + a[2]) + b[2]), og = gated_sigmoid((p[3] + a[3]) + b[3]);
        c = fg * c + ig * gg;
        return og * tanhf(c);
    }
};

struct GruCell {
    static constexpr int NG = 3;
    static constexpr bool HAS_C = false;
    static constexpr bool AHEAD = true;
    float r, z, in, hn;                     // r and z pre-added, the candidate's apart
    __device__ __forceinline__ void load(const float* __restrict__ b_ih, const float* __restrict__ b_hh, int H,
                                         int n) {
        r = b_ih[n] + b_hh[n];
        z = b_ih[H + n] + b_hh[H + n];
        in = b_ih[2 * H + n];
        hn = b_hh[2 * H + n];
    }
    __device__ __forceinline__ float update(const float (&p)[3], const float (&a)[3], float hprev, float&) const {
        const float rg = gated_sigmoid((p[0] + a[0]) + r);
        const float zg = gated_sigmoid((p[1] + a[1]) + z);
        const float n = tanhf((p[2] + in) + rg * (a[2] + hn));
        return n + zg * (hprev - n);
    }
};

// ---------------------------------------------------------------------------
// Resident form, 16 <= H <= 128 (H % 16 == 0), in the shape of
// rnn_recur_mfma_kernel: 16 utterances per workgroup, one wave per 16-column
// j-tile (block = 64 * H/16 threads, 8 waves at H = 128).  Wave w keeps the NG
// gate tiles of its columns of W_hh in registers for all T: H/4 floats per lane
// and tile, 128 VGPRs at H = 128 for the LSTM (the tanh kernel's budget at
// H = 256) and 96 for the GRU, and issues NG * H/4 MFMAs per step (128 and 96
// at H = 128).  h_{t-1} (16 x H) is double-buffered in LDS, one LDS-only
// barrier per step; MFMA (i, e) of lane group g contracts k = 16i + 4g + e,
// one ds_read_b128 per 16 k shared by the gates.  P_{t+1} is prefetched one
// step ahead.  The lane's own h_{t-1} (and c_{t-1}) element stays in a
// register and is the operand of the update; past its length an utterance
// keeps those registers, writes a zero row and feeds the carried h to LDS.
// ---------------------------------------------------------------------------
template <class Cell>
__global__ __launch_bounds__(64 * GR_NCH) void gated_recur_kernel(const float* P, const float* __restrict__ h0,
                                                                  const float* __restrict__ c0,
                                                                  const float* __restrict__ Whh,
                                                                  const float* __restrict__ b_ih,
                                                                  const float* __restrict__ b_hh, float* hid,
                                                                  long ldh, float* hT, float* cT,
                                                                  const int32_t* __restrict__ lengths, int T, int B,
                                                                  int H, int reverse) {
    constexpr int NG = Cell::NG;
    __shared__ __attribute__((aligned(16))) float hs[2][GR_ROWS * GR_LD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int nch = H >> 4;                 // 16-k chunks = waves
    const int r0 = blockIdx.x * GR_ROWS;
    const int n = 16 * w + c;               // this lane's hidden column
    const int HG = NG * H;
    // wb[q][i][e] = W_hh[16i + 4g + e][q*H + n]
    float wb[NG][GR_NCH][4];
#pragma unroll
    for (int q = 0; q < NG; q++)
#pragma unroll
        for (int i = 0; i < GR_NCH; i++)
#pragma unroll
            for (int e = 0; e < 4; e++)
                wb[q][i][e] = i < nch ? Whh[(long)(16 * i + 4 * g + e) * HG + q * H + n] : 0.f;
    Cell cell;
    cell.load(b_ih, b_hh, H, n);
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
        voff[j] = ok[j] ? (rr * HG + n) * 4 : GR_OOB;
        orow[j] = (long)rr * ldh + n;
        hreg[j] = (ok[j] && h0) ? h0[(long)rr * H + n] : 0.f;
        creg[j] = 0.f;
        if constexpr (Cell::HAS_C) creg[j] = (ok[j] && c0) ? c0[(long)rr * H + n] : 0.f;
        hs[0][(4 * g + j) * GR_LD + n] = hreg[j];
    }
    const long tstride = (long)B * HG;      // floats of P per frame
    const int nbytes = (int)(tstride * 4);
    const int gstep = H * 4;                // bytes from one gate's column to the next
    float* const Pw = const_cast<float*>(P);
    float pn[NG][4];
    // frame tf's P of this lane's elements (bytes = 0: an empty resource, zeros)
    auto prefetch = [&](int tf, int bytes) {
        const auto rs = __builtin_amdgcn_make_buffer_rsrc(Pw + tf * tstride, 0, bytes, GR_RSRC3);
#pragma unroll
        for (int q = 0; q < NG; q++)
#pragma unroll
            for (int j = 0; j < 4; j++)
                pn[q][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff[j] + q * gstep, 0, 0));
    };
    prefetch(reverse ? T - 1 : 0, nbytes);
    __syncthreads();
    int cur = 0;
    for (int s = 0; s < T; s++) {
        const int t = reverse ? T - 1 - s : s;
        float p[NG][4];
#pragma unroll
        for (int q = 0; q < NG; q++)
#pragma unroll
            for (int j = 0; j < 4; j++) p[q][j] = pn[q][j];
        {
            // next frame's P (past the last step: an empty resource, zeros)
            const bool more = s + 1 < T;
            prefetch(more ? (reverse ? t - 1 : t + 1) : t, more ? nbytes : 0);
        }
        const float* hrow = &hs[cur][c * GR_LD + 4 * g];
        f32x4 acc[NG];
#pragma unroll
        for (int q = 0; q < NG; q++) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < GR_NCH; i++) {
            if (i < nch) {
                const float4 a = *reinterpret_cast<const float4*>(hrow + 16 * i);
                const float ae[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
                for (int e = 0; e < 4; e++)
#pragma unroll
                    for (int q = 0; q < NG; q++)
                        acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(ae[e], wb[q][i][e], acc[q], 0, 0, 0);
            }
        }
        float* hn = hs[cur ^ 1];
        const long obase = (long)t * B * ldh;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            float pj[NG], aj[NG];
#pragma unroll
            for (int q = 0; q < NG; q++) pj[q] = p[q][j], aj[q] = acc[q][j];
            float cnew = creg[j];
            const float hnew = cell.update(pj, aj, hreg[j], cnew);
            const bool act = t < len[j];
            creg[j] = act ? cnew : creg[j];
            hreg[j] = act ? hnew : hreg[j];
            hn[(4 * g + j) * GR_LD + n] = hreg[j];   // the carried h feeds the next step
            if (ok[j]) hid[obase + orow[j]] = act ? hnew : 0.f;
        }
        cur ^= 1;
        gated_lds_barrier();
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (!ok[j]) continue;
        const long x = (long)(r0 + 4 * g + j) * H + n;
        if (hT) hT[x] = hreg[j];
        if constexpr (Cell::HAS_C)
            if (cT) cT[x] = creg[j];
    }
}

// ---------------------------------------------------------------------------
// Step form, 128 < H <= 2048 (H % 16 == 0): one launch per frame.  Grid
// (ceil(B / 16) row tiles, ceil(H/16 / 4) groups of j-tiles), 4 waves per
// workgroup, wave w of group y owns j-tile 4y + w for all NG gates.  The A
// fragments (h_{t-1}, rows of the tile) come straight from memory as 16-byte
// loads (the group's waves read the same lines), the B fragments are the
// wave's own columns of W_hh.  h_{t-1} of utterance b is the output row of
// the frame it last ran in (the previous frame, or its last valid one when
// this frame is past its length), or h0 before its first: the carried h needs
// no copy.  The lane that owns an element also loads the state operand of its
// update: the GRU's one h_{t-1} value from that same row (or h0, or zero),
// ahead of the contraction; the LSTM's c, read and written in place in the
// workspace (cin: c0 / NULL at the first step, the workspace after), after it.
// No LDS, no barrier, nothing shared between workgroups within a launch:
// frame t's launch reads frame t -/+ 1's rows and writes frame t's.
// ---------------------------------------------------------------------------
// The row that holds utterance r's h before frame t runs (NULL: zeros).
__device__ __forceinline__ const float* gated_h_before(const float* hid, long ldh, const float* h0, int t, int r,
                                                       int len, int B, int H, int reverse) {
    const int tp = reverse ? (t + 1 < len ? t + 1 : -1) : min(t, len) - 1;
    if (tp >= 0) return hid + ((long)tp * B + r) * ldh;
    return h0 ? h0 + (long)r * H : nullptr;
}

template <class Cell>
__global__ __launch_bounds__(64 * GR_WAVES) void gated_step_kernel(const float* P, const float* __restrict__ h0,
                                                                   const float* cin, float* cout,
                                                                   const float* __restrict__ Whh,
                                                                   const float* __restrict__ b_ih,
                                                                   const float* __restrict__ b_hh, float* hid,
                                                                   long ldh, float* hT, float* cT,
                                                                   const int32_t* __restrict__ lengths, int t, int T,
                                                                   int B, int H, int reverse, int last) {
    constexpr int NG = Cell::NG;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int nch = H >> 4;
    const int tile = blockIdx.y * GR_WAVES + w;
    if (tile >= nch) return;                // no barrier below
    const int r0 = blockIdx.x * GR_ROWS;
    const int n = 16 * tile + c;
    const int HG = NG * H;
    // A fragments: row c of the tile (clamped: rows past B feed only their own, unused, results)
    const int ra = min(r0 + c, B - 1);
    const int lena = lengths ? min(max(lengths[ra], 0), T) : T;
    const float* hsrc = gated_h_before(hid, ldh, h0, t, ra, lena, B, H, reverse);
    const bool hz = hsrc == nullptr;        // zeros: load from a valid address, then discard
    const float* ap = (hz ? Whh : hsrc) + 4 * g;
    const float* bp = Whh + (long)(4 * g) * HG + n;
    // this lane's four elements: rows r0 + 4g + j, column n.  request_p(j)
    // asks for element j's P_t (zeros past B), request_state(j, r) for its
    // length and the state operand of its update (the GRU's h_{t-1}, the
    // LSTM's c_{t-1}) in row r, a valid row; both are used after the
    // contraction.  An AHEAD cell requests all four elements here, with rows
    // past B reading row 0; the others request each element where they use it,
    // the state of rows below B only.
    const long tstride = (long)B * HG;
    const int gstep = H * 4;
    int len[4];
    float p[NG][4], hold[4], cold[4];
    auto h_carried = [&](int r, int ln) {
        const float* hb = gated_h_before(hid, ldh, h0, t, r, ln, B, H, reverse);
        return hb ? hb[n] : 0.f;
    };
    auto request_p = [&](int j) {
        const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(P) + t * tstride, 0,
                                                          (int)(tstride * 4), GR_RSRC3);
        const int r = r0 + 4 * g + j;
        const bool ok = r < B;
        const int rr = ok ? r : 0;
        const int voff = ok ? (rr * HG + n) * 4 : GR_OOB;
#pragma unroll
        for (int q = 0; q < NG; q++)
            p[q][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff + q * gstep, 0, 0));
    };
    auto request_state = [&](int j, int r) {
        len[j] = lengths ? min(max(lengths[r], 0), T) : T;
        hold[j] = cold[j] = 0.f;
        if constexpr (Cell::HAS_C) cold[j] = cin ? cin[(long)r * H + n] : 0.f;
        else hold[j] = h_carried(r, len[j]);
    };
    if constexpr (Cell::AHEAD) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            request_p(j);
            const int r = r0 + 4 * g + j;
            request_state(j, r < B ? r : 0);
        }
    }
    f32x4 acc[NG];
#pragma unroll
    for (int q = 0; q < NG; q++) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    // The fragments of chunk i + GR_DEPTH are loaded while chunk i's MFMAs
    // issue (a ring of GR_DEPTH register stages, 1 + 4 NG loads each; loads
    // past the last chunk re-read it and are not used).
    float4 a[GR_DEPTH];
    float b[GR_DEPTH][4][NG];
    auto fetch = [&](int u, int i) {
        const int ii = min(i, nch - 1);
        a[u] = *reinterpret_cast<const float4*>(ap + 16 * ii);
        const float* bi = bp + (long)(16 * ii) * HG;
#pragma unroll
        for (int e = 0; e < 4; e++)
#pragma unroll
            for (int q = 0; q < NG; q++) b[u][e][q] = bi[(long)e * HG + q * H];
    };
#pragma unroll
    for (int u = 0; u < GR_DEPTH; u++) fetch(u, u);
    for (int i0 = 0; i0 < nch; i0 += GR_DEPTH) {
#pragma unroll
        for (int u = 0; u < GR_DEPTH; u++) {
            if (i0 + u < nch) {
                const float4 x = hz ? float4{0.f, 0.f, 0.f, 0.f} : a[u];
                const float xe[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                for (int e = 0; e < 4; e++)
#pragma unroll
                    for (int q = 0; q < NG; q++)
                        acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(xe[e], b[u][e][q], acc[q], 0, 0, 0);
            }
            fetch(u, i0 + u + GR_DEPTH);
        }
    }
    Cell cell;
    cell.load(b_ih, b_hh, H, n);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if constexpr (!Cell::AHEAD) request_p(j);
        const int r = r0 + 4 * g + j;
        if (r >= B) continue;
        if constexpr (!Cell::AHEAD) request_state(j, r);
        float pj[NG], aj[NG];
#pragma unroll
        for (int q = 0; q < NG; q++) pj[q] = p[q][j], aj[q] = acc[q][j];
        const long x = (long)r * H + n;
        const bool act = t < len[j];
        float cnew = cold[j];
        const float hnew = cell.update(pj, aj, hold[j], cnew);
        cnew = act ? cnew : cold[j];
        if constexpr (Cell::HAS_C) cout[x] = cnew;
        hid[((long)t * B + r) * ldh + n] = act ? hnew : 0.f;
        if (last) {
            if constexpr (Cell::HAS_C)
                if (cT) cT[x] = cnew;
            if (hT) {
                float hc = hnew;            // or the carried value
                if (!act) hc = Cell::HAS_C ? h_carried(r, len[j]) : hold[j];
                hT[x] = hc;
            }
        }
    }
}

static bool gated_shape_ok(int H) { return H > 0 && (H & 15) == 0 && H <= GR_HMAX; }

// The resident form, or one launch per frame (cwork: the step form's c [B][H]).
template <class Cell>
static int gated_launch(const float* P, const float* h0, const float* c0, const float* Whh, const float* b_ih,
                        const float* b_hh, float* hid, long ldh, float* hT, float* cT, const int32_t* lengths,
                        float* cwork, int T, int B, int H, int reverse, hipStream_t s) {
    const unsigned gx = (unsigned)((B + GR_ROWS - 1) / GR_ROWS);
    if (H <= GR_RHMAX) {
        hipLaunchKernelGGL(gated_recur_kernel<Cell>, dim3(gx), dim3(64 * (H / 16)), 0, s, P, h0, c0, Whh, b_ih, b_hh,
                           hid, ldh, hT, cT, lengths, T, B, H, reverse);
        ASR_LAUNCH_TRY();
        return ASR_OK;
    }
    const unsigned gy = (unsigned)((H / 16 + GR_WAVES - 1) / GR_WAVES);
    for (int k = 0; k < T; k++) {
        const int t = reverse ? T - 1 - k : k;
        hipLaunchKernelGGL(gated_step_kernel<Cell>, dim3(gx, gy), dim3(64 * GR_WAVES), 0, s, P, h0,
                           k ? (const float*)cwork : c0, cwork, Whh, b_ih, b_hh, hid, ldh, hT, cT, lengths, t, T, B, H,
                           reverse, k == T - 1 ? 1 : 0);
        ASR_LAUNCH_TRY();
    }
    return ASR_OK;
}

// The shape checks of the entry points, ahead of any HIP call.
template <class Cell>
static int gated_check(const void* work, long ldh, int T, int B, int H, const float* hid, const float* h0,
                       const float* hT) {
    if (T <= 0 || B <= 0 || H <= 0 || ldh < H) return ASR_ERR_ARG;
    if (!gated_shape_ok(H)) return ASR_ERR_UNSUPPORTED;
    if ((long)B * Cell::NG * H * 4 > (long)GR_OOB) return ASR_ERR_UNSUPPORTED;   // one frame of P per buffer resource
    if ((long)T * B > INT_MAX) return ASR_ERR_UNSUPPORTED;
    if (H > GR_RHMAX) {
        if (Cell::HAS_C && !work) return ASR_ERR_ARG;   // c lives there
        // the step form reads h_{t-1} rows with 16-byte loads
        if ((ldh & 3) != 0 || ((uintptr_t)hid & 15) != 0 || ((uintptr_t)h0 & 15) != 0) return ASR_ERR_UNSUPPORTED;
    }
    // hT over h0: the step form's workgroups read whole h0 rows for the
    // contraction while the owners of other columns store hT in the same
    // launch, so it takes no overlap at all; the resident form's lanes read
    // their own h0 element first and write that element last, so hT == h0
    // exactly is in-place streaming there, and any other overlap is refused.
    if (hT && h0) {
        const uintptr_t a = (uintptr_t)hT, b = (uintptr_t)h0, n = (uintptr_t)B * H * sizeof(float);
        if ((a > b ? a - b : b - a) < n && !(a == b && H <= GR_RHMAX)) return ASR_ERR_ARG;
    }
    // hT == h0 (in-place streaming).  A lane of the resident form reads its own
    // h0 element first and writes that element last: legal.  The step form's
    // workgroups read whole h0 rows for the contraction while the owners of
    // other columns store hT in the same launch (T = 1, or a length-1
    // utterance in reverse): refused.  (c0 / cT: the owning lane reads before
    // it writes in both forms.)
    if (hT && hT == h0 && H > GR_RHMAX) return ASR_ERR_ARG;
    return ASR_OK;
}

// P [T*B][NG*H], then the step form's c [B][H] if there is one (H % 16 == 0:
// both a multiple of 16 bytes); 0 for a shape the entry points refuse.
template <class Cell>
static size_t gated_workspace_bytes(int T, int B, int H) {
    if (T <= 0 || B <= 0 || !gated_shape_ok(H) || (long)T * B > INT_MAX) return 0;
    return ((size_t)T * B * Cell::NG * H + (Cell::HAS_C ? (size_t)B * H : 0)) * sizeof(float);
}

// The recurrence on a given P; work (may be NULL without a cell state or at
// H <= 128) is laid out as gated_workspace_bytes says.
template <class Cell>
static int gated_recur_fwd(const float* P, const float* h0, const float* c0, const float* W_hh, const float* b_ih,
                           const float* b_hh, float* hid, long ldh, float* hT, float* cT, const int32_t* lengths,
                           void* work, int T, int B, int H, int reverse, asr_stream_t s) {
    if (!P || !W_hh || !b_ih || !b_hh || !hid) return ASR_ERR_ARG;
    if (int rc = gated_check<Cell>(work, ldh, T, B, H, hid, h0, hT)) return rc;
    float* cwork = Cell::HAS_C && work ? (float*)work + (size_t)T * B * Cell::NG * H : nullptr;
    return gated_launch<Cell>(P, h0, c0, W_hh, b_ih, b_hh, hid, ldh, hT, cT, lengths, cwork, T, B, H,
                              reverse ? 1 : 0, asr_stream(s));
}

template <class Cell>
static int gated_fwd(const float* x, const float* h0, const float* c0, const float* W_ih, const float* W_hh,
                     const float* b_ih, const float* b_hh, float* hid, long ldh, float* hT, float* cT,
                     const int32_t* lengths, void* work, int T, int B, int in, int H, int reverse, asr_stream_t s) {
    if (!x || !W_ih || !W_hh || !b_ih || !b_hh || !hid || !work || in <= 0) return ASR_ERR_ARG;
    if (int rc = gated_check<Cell>(work, ldh, T, B, H, hid, h0, hT)) return rc;
    // P = x.W_ih for all T frames: asr_linear_fwd(x, W_ih, NULL, P, T*B, in, NG*H, ASR_EPI_NONE)
    const int HG = Cell::NG * H;
    GemmArgs g{};
    g.A = x; g.B = W_ih; g.C = (float*)work;
    g.M = T * B; g.N = HG; g.K = in;
    g.sam = in; g.sak = 1; g.sbk = HG; g.sbn = 1; g.ldc = HG;
    if (int rc = gemm_launch(g, EPI_NONE, asr_stream(s))) return rc;
    return gated_recur_fwd<Cell>((const float*)work, h0, c0, W_hh, b_ih, b_hh, hid, ldh, hT, cT, lengths, work, T, B,
                                 H, reverse, s);
}

}  // namespace asr

extern "C" {

size_t asr_lstm_workspace_bytes(int T, int B, int H) { return asr::gated_workspace_bytes<asr::LstmCell>(T, B, H); }

int asr_lstm_recur_fwd(const float* P, const float* h0, const float* c0, const float* W_hh, const float* b_ih,
                       const float* b_hh, float* hid, long ldh, float* hT, float* cT, const int32_t* lengths,
                       void* work, int T, int B, int H, int reverse, asr_stream_t s) {
    return asr::gated_recur_fwd<asr::LstmCell>(P, h0, c0, W_hh, b_ih, b_hh, hid, ldh, hT, cT, lengths, work, T, B, H,
                                               reverse, s);
}

int asr_lstm_fwd(const float* x, const float* h0, const float* c0, const float* W_ih, const float* W_hh,
                 const float* b_ih, const float* b_hh, float* hid, long ldh, float* hT, float* cT,
                 const int32_t* lengths, void* work, int T, int B, int in, int H, int reverse, asr_stream_t s) {
    return asr::gated_fwd<asr::LstmCell>(x, h0, c0, W_ih, W_hh, b_ih, b_hh, hid, ldh, hT, cT, lengths, work, T, B, in,
                                         H, reverse, s);
}

size_t asr_gru_workspace_bytes(int T, int B, int H) { return asr::gated_workspace_bytes<asr::GruCell>(T, B, H); }

int asr_gru_recur_fwd(const float* P, const float* h0, const float* W_hh, const float* b_ih, const float* b_hh,
                      float* hid, long ldh, float* hT, const int32_t* lengths, int T, int B, int H, int reverse,
                      asr_stream_t s) {
    return asr::gated_recur_fwd<asr::GruCell>(P, h0, nullptr, W_hh, b_ih, b_hh, hid, ldh, hT, nullptr, lengths,
                                              nullptr, T, B, H, reverse, s);
}

int asr_gru_fwd(const float* x, const float* h0, const float* W_ih, const float* W_hh, const float* b_ih,
                const float* b_hh, float* hid, long ldh, float* hT, const int32_t* lengths, void* work, int T, int B,
                int in, int H, int reverse, asr_stream_t s) {
    return asr::gated_fwd<asr::GruCell>(x, h0, nullptr, W_ih, W_hh, b_ih, b_hh, hid, ldh, hT, nullptr, lengths, work,
                                        T, B, in, H, reverse, s);
}

}  // extern "C"
