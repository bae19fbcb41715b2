// GRU layer (torch.nn.GRU semantics, one layer and direction per call):
// asr_gru_workspace_bytes / asr_gru_fwd / asr_gru_recur_fwd.
//
// Weights in the project's [in][out] layout: W_ih [in][3H], W_hh [H][3H], gate
// q (r, z, n) of hidden unit j at column q*H + j.  P = x.W_ih for all T frames
// is one gemm_launch (EPI_NONE, N = 3H); with a = h_{t-1}.W_hh each frame then
// computes, in this operation order in both kernels,
//   r   = sigmoid((P_r + a_r) + (b_ir + b_hr))
//   z   = sigmoid((P_z + a_z) + (b_iz + b_hz))
//   n   = tanh((P_n + b_in) + r * (a_n + b_hn))
//   h_t = n + z * (h_{t-1} - n)              ( = (1 - z) n + z h_{t-1} )
// The reset gate multiplies the hidden contribution of the candidate only, so
// a_n is an accumulator of its own that starts from zero and never meets P_n,
// and b_in / b_hn are not pre-added; r and z use the same code shape.  The
// contraction runs on v_mfma_f32_16x16x4_f32 (exact fp32).  A wave computes
// the r, z and n tiles of the SAME 16 hidden columns, so in the C-fragment
// layout (rows 4g + j, column lane & 15) a lane holds a_r, a_z and a_n of its
// four (row, column) elements: gates and update are lane-local, nothing is
// exchanged.  The three tiles are three independent accumulator chains (the
// MFMA's 40-cycle dependent latency against its 32-cycle issue needs two).
// There is no cell state, hence no workspace beyond P.
//
// The kernel depends on H only, never on B: an utterance's bits do not depend
// on the batch it runs in.
//   16 <= H <= 128  resident form: the whole recurrence in one launch
//                   (gru_recur_kernel);
//   128 < H <= 2048 step form: one launch per frame (gru_step_kernel),
//                   capturable in a graph.
// Neither waits on another workgroup; every loop is bounded by T or H.
//
// reverse, ldh, lengths: as in lstm.hip.  For frames t >= len_b the
// utterance's h is carried unchanged and its output row is zeros; in reverse
// the utterance starts from h0 at its own last frame.
#include "dense.h"

#include <climits>
#include <cstddef>

namespace asr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Workgroup barrier ordering LDS only (dense.hip lds_barrier): the step's
// global stores and the prefetch of P_{t+1} stay in flight across it.
__device__ __forceinline__ void gru_lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

__device__ __forceinline__ float gru_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

constexpr int GS_ROWS = 16;                 // utterances per workgroup (one MFMA row tile)
constexpr int GR_HMAX = 128;                // resident form: H <= 128
constexpr int GR_LD = GR_HMAX + 4;          // LDS row stride (floats) of h
constexpr int GR_NCH = GR_HMAX / 16;        // 16-k chunks at H = 128
constexpr int GS_HMAX = 2048;               // step form: H <= 2048
constexpr int GS_WAVES = 4;                 // step form: j-tiles (waves) per workgroup
constexpr int GS_DEPTH = 3;                 // step form: 16-k chunks of fragments in flight per wave
// P_t is read through one buffer resource per frame (B*3H*4 bytes): lanes of
// rows past B get this offset (+ at most 2*H*4 for the gate), past the
// resource's size, so their loads return 0 without a branch.
constexpr int GRU_OOB = 0x7ff00000;
constexpr int GRU_RSRC3 = 0x00020000;       // gfx9 buffer descriptor word 3 (raw 32-bit data)

// The biases of a lane's hidden column: r and z pre-added, the candidate's apart.
struct GruBias {
    float r, z, in, hn;
};
__device__ __forceinline__ GruBias gru_bias(const float* __restrict__ b_ih, const float* __restrict__ b_hh, int H,
                                            int n) {
    GruBias b;
    b.r = b_ih[n] + b_hh[n];
    b.z = b_ih[H + n] + b_hh[H + n];
    b.in = b_ih[2 * H + n];
    b.hn = b_hh[2 * H + n];
    return b;
}

// One cell update of a lane's element: p* from P_t, a* from h_{t-1}.W_hh.
__device__ __forceinline__ float gru_cell(float pr, float pz, float pn, float ar, float az, float an,
                                          const GruBias& b, float hprev) {
    const float r = gru_sigmoid((pr + ar) + b.r);
    const float z = gru_sigmoid((pz + az) + b.z);
    const float n = tanhf((pn + b.in) + r * (an + b.hn));
    return n + z * (hprev - n);
}

// ---------------------------------------------------------------------------
// Resident form, 16 <= H <= 128 (H % 16 == 0), in the shape of
// lstm_recur_kernel: 16 utterances per workgroup, one wave per 16-column
// j-tile (block = 64 * H/16 threads, 8 waves at H = 128).  Wave w keeps the
// three gate tiles of its columns of W_hh in registers for all T: 3*H/4 floats
// per lane, 96 at H = 128, and issues 3 * H/4 MFMAs per step (96 at H = 128).
// h_{t-1} (16 x H) is double-buffered in LDS, one LDS-only barrier per step;
// MFMA (i, e) of lane group g contracts k = 16i + 4g + e, one ds_read_b128 per
// 16 k shared by the three gates.  P_{t+1} is prefetched one step ahead.  The
// lane's own h_{t-1} element stays in a register and is the operand of the
// update; past its length an utterance keeps that register, writes a zero row
// and feeds the carried value to LDS.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64 * GR_NCH) void gru_recur_kernel(const float* P, const float* __restrict__ h0,
                                                                const float* __restrict__ Whh,
                                                                const float* __restrict__ b_ih,
                                                                const float* __restrict__ b_hh, float* hid, long ldh,
                                                                float* hT, const int32_t* __restrict__ lengths, int T,
                                                                int B, int H, int reverse) {
    __shared__ __attribute__((aligned(16))) float hs[2][GS_ROWS * GR_LD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int nch = H >> 4;                 // 16-k chunks = waves
    const int r0 = blockIdx.x * GS_ROWS;
    const int n = 16 * w + c;               // this lane's hidden column
    const int H3 = 3 * H;
    // wb[q][i][e] = W_hh[16i + 4g + e][q*H + n]
    float wb[3][GR_NCH][4];
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
        for (int i = 0; i < GR_NCH; i++)
#pragma unroll
            for (int e = 0; e < 4; e++)
                wb[q][i][e] = i < nch ? Whh[(long)(16 * i + 4 * g + e) * H3 + q * H + n] : 0.f;
    const GruBias bias = gru_bias(b_ih, b_hh, H, n);
    // this lane's four elements: rows r0 + 4g + j, column n
    bool ok[4];
    int len[4], voff[4];
    long orow[4];
    float hreg[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int r = r0 + 4 * g + j;
        ok[j] = r < B;
        const int rr = ok[j] ? r : 0;
        len[j] = !ok[j] ? 0 : lengths ? min(max(lengths[rr], 0), T) : T;
        voff[j] = ok[j] ? (rr * H3 + n) * 4 : GRU_OOB;
        orow[j] = (long)rr * ldh + n;
        hreg[j] = (ok[j] && h0) ? h0[(long)rr * H + n] : 0.f;
        hs[0][(4 * g + j) * GR_LD + n] = hreg[j];
    }
    const long tstride = (long)B * H3;      // floats of P per frame
    const int nbytes = (int)(tstride * 4);
    const int gstep = H * 4;                // bytes from one gate's column to the next
    float* const Pw = const_cast<float*>(P);
    float pn[3][4];
    {
        const int t0 = reverse ? T - 1 : 0;
        const auto rs = __builtin_amdgcn_make_buffer_rsrc(Pw + t0 * tstride, 0, nbytes, GRU_RSRC3);
#pragma unroll
        for (int q = 0; q < 3; q++)
#pragma unroll
            for (int j = 0; j < 4; j++)
                pn[q][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff[j] + q * gstep, 0, 0));
    }
    __syncthreads();
    int cur = 0;
    for (int s = 0; s < T; s++) {
        const int t = reverse ? T - 1 - s : s;
        float p[3][4];
#pragma unroll
        for (int q = 0; q < 3; q++)
#pragma unroll
            for (int j = 0; j < 4; j++) p[q][j] = pn[q][j];
        {
            // next frame's P (past the last step: an empty resource, zeros)
            const bool more = s + 1 < T;
            const int tn = more ? (reverse ? t - 1 : t + 1) : t;
            const auto rs = __builtin_amdgcn_make_buffer_rsrc(Pw + tn * tstride, 0, more ? nbytes : 0, GRU_RSRC3);
#pragma unroll
            for (int q = 0; q < 3; q++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    pn[q][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff[j] + q * gstep, 0, 0));
        }
        const float* hrow = &hs[cur][c * GR_LD + 4 * g];
        f32x4 acc[3];
#pragma unroll
        for (int q = 0; q < 3; q++) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < GR_NCH; i++) {
            if (i < nch) {
                const float4 a = *reinterpret_cast<const float4*>(hrow + 16 * i);
#pragma unroll
                for (int q = 0; q < 3; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, wb[q][i][0], acc[q], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 3; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, wb[q][i][1], acc[q], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 3; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, wb[q][i][2], acc[q], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 3; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, wb[q][i][3], acc[q], 0, 0, 0);
            }
        }
        float* hn = hs[cur ^ 1];
        const long obase = (long)t * B * ldh;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float hnew = gru_cell(p[0][j], p[1][j], p[2][j], acc[0][j], acc[1][j], acc[2][j], bias, hreg[j]);
            const bool act = t < len[j];
            hreg[j] = act ? hnew : hreg[j];
            hn[(4 * g + j) * GR_LD + n] = hreg[j];   // the carried h feeds the next step
            if (ok[j]) hid[obase + orow[j]] = act ? hnew : 0.f;
        }
        cur ^= 1;
        gru_lds_barrier();
    }
    if (hT) {
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (ok[j]) hT[(long)(r0 + 4 * g + j) * H + n] = hreg[j];
    }
}

// ---------------------------------------------------------------------------
// Step form, 128 < H <= 2048 (H % 16 == 0), in the shape of lstm_step_kernel:
// one launch per frame.  Grid (ceil(B / 16) row tiles, ceil(H/16 / 4) groups
// of j-tiles), 4 waves per workgroup, wave w of group y owns j-tile 4y + w for
// all three gates.  The A fragments (h_{t-1}, rows of the tile) come straight
// from memory as 16-byte loads, the B fragments are the wave's own columns of
// W_hh.  h_{t-1} of utterance b is the output row of the frame it last ran in
// (the previous frame, or its last valid one when this frame is past its
// length), or h0 before its first: the carried h needs no copy.  The lane that
// owns an element also loads its one h_{t-1} value from that same row (or h0,
// or takes zero) as the operand of the update, ahead of the contraction.
// No LDS, no barrier, nothing shared between workgroups within a launch:
// frame t's launch reads frame t -/+ 1's rows and writes frame t's.
// ---------------------------------------------------------------------------
// The row that holds utterance r's h before frame t runs (NULL: zeros).
__device__ __forceinline__ const float* gru_h_before(const float* hid, long ldh, const float* h0, int t, int r,
                                                     int len, int B, int H, int reverse) {
    const int tp = reverse ? (t + 1 < len ? t + 1 : -1) : min(t, len) - 1;
    if (tp >= 0) return hid + ((long)tp * B + r) * ldh;
    return h0 ? h0 + (long)r * H : nullptr;
}

__global__ __launch_bounds__(64 * GS_WAVES) void gru_step_kernel(const float* P, const float* __restrict__ h0,
                                                                 const float* __restrict__ Whh,
                                                                 const float* __restrict__ b_ih,
                                                                 const float* __restrict__ b_hh, float* hid, long ldh,
                                                                 float* hT, const int32_t* __restrict__ lengths, int t,
                                                                 int T, int B, int H, int reverse, int last) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int nch = H >> 4;
    const int tile = blockIdx.y * GS_WAVES + w;
    if (tile >= nch) return;                // no barrier below
    const int r0 = blockIdx.x * GS_ROWS;
    const int n = 16 * tile + c;
    const int H3 = 3 * H;
    // A fragments: row c of the tile (clamped: rows past B feed only their own, unused, results)
    const int ra = min(r0 + c, B - 1);
    const int lena = lengths ? min(max(lengths[ra], 0), T) : T;
    const float* hsrc = gru_h_before(hid, ldh, h0, t, ra, lena, B, H, reverse);
    const bool hz = hsrc == nullptr;        // zeros: load from a valid address, then discard
    const float* ap = (hz ? Whh : hsrc) + 4 * g;
    const float* bp = Whh + (long)(4 * g) * H3 + n;
    // this lane's four elements: rows r0 + 4g + j, column n.  Their P_t and
    // h_{t-1} are requested here and used after the contraction.
    const long tstride = (long)B * H3;
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(P) + t * tstride, 0, (int)(tstride * 4),
                                                      GRU_RSRC3);
    const int gstep = H * 4;
    bool act[4];
    float p[3][4], hold[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int r = r0 + 4 * g + j;
        const bool ok = r < B;
        const int rr = ok ? r : 0;
        const int voff = ok ? (rr * H3 + n) * 4 : GRU_OOB;
#pragma unroll
        for (int q = 0; q < 3; q++)
            p[q][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff + q * gstep, 0, 0));
        const int len = lengths ? min(max(lengths[rr], 0), T) : T;
        act[j] = t < len;
        const float* hb = gru_h_before(hid, ldh, h0, t, rr, len, B, H, reverse);
        hold[j] = hb ? hb[n] : 0.f;
    }
    f32x4 acc[3];
#pragma unroll
    for (int q = 0; q < 3; q++) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    // The fragments of chunk i + GS_DEPTH are loaded while chunk i's MFMAs
    // issue (a ring of GS_DEPTH register stages, 13 loads each; loads past
    // the last chunk re-read it and are not used).
    float4 a[GS_DEPTH];
    float b[GS_DEPTH][4][3];
    auto fetch = [&](int u, int i) {
        const int ii = min(i, nch - 1);
        a[u] = *reinterpret_cast<const float4*>(ap + 16 * ii);
        const float* bi = bp + (long)(16 * ii) * H3;
#pragma unroll
        for (int e = 0; e < 4; e++)
#pragma unroll
            for (int q = 0; q < 3; q++) b[u][e][q] = bi[(long)e * H3 + q * H];
    };
#pragma unroll
    for (int u = 0; u < GS_DEPTH; u++) fetch(u, u);
    for (int i0 = 0; i0 < nch; i0 += GS_DEPTH) {
#pragma unroll
        for (int u = 0; u < GS_DEPTH; u++) {
            if (i0 + u < nch) {
                const float4 x = hz ? float4{0.f, 0.f, 0.f, 0.f} : a[u];
#pragma unroll
                for (int q = 0; q < 3; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, b[u][0][q], acc[q], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 3; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, b[u][1][q], acc[q], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 3; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, b[u][2][q], acc[q], 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 3; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, b[u][3][q], acc[q], 0, 0, 0);
            }
            fetch(u, i0 + u + GS_DEPTH);
        }
    }
    const GruBias bias = gru_bias(b_ih, b_hh, H, n);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int r = r0 + 4 * g + j;
        if (r >= B) continue;
        const float hnew = gru_cell(p[0][j], p[1][j], p[2][j], acc[0][j], acc[1][j], acc[2][j], bias, hold[j]);
        hid[((long)t * B + r) * ldh + n] = act[j] ? hnew : 0.f;
        if (last && hT) hT[(long)r * H + n] = act[j] ? hnew : hold[j];   // the carried value
    }
}

static bool gru_shape_ok(int H) { return H > 0 && (H & 15) == 0 && H <= GS_HMAX; }

static int gru_recur_launch(const float* P, const float* h0, const float* Whh, const float* b_ih, const float* b_hh,
                            float* hid, long ldh, float* hT, const int32_t* lengths, int T, int B, int H, int reverse,
                            hipStream_t s) {
    const unsigned gx = (unsigned)((B + GS_ROWS - 1) / GS_ROWS);
    if (H <= GR_HMAX) {
        hipLaunchKernelGGL(gru_recur_kernel, dim3(gx), dim3(64 * (H / 16)), 0, s, P, h0, Whh, b_ih, b_hh, hid, ldh, hT,
                           lengths, T, B, H, reverse);
        ASR_LAUNCH_TRY();
        return ASR_OK;
    }
    const unsigned gy = (unsigned)((H / 16 + GS_WAVES - 1) / GS_WAVES);
    for (int k = 0; k < T; k++) {
        const int t = reverse ? T - 1 - k : k;
        hipLaunchKernelGGL(gru_step_kernel, dim3(gx, gy), dim3(64 * GS_WAVES), 0, s, P, h0, Whh, b_ih, b_hh, hid, ldh,
                           hT, lengths, t, T, B, H, reverse, k == T - 1 ? 1 : 0);
        ASR_LAUNCH_TRY();
    }
    return ASR_OK;
}

// The shape checks of both entry points, ahead of any HIP call.
static int gru_check(long ldh, int T, int B, int H, const float* hid, const float* h0) {
    if (T <= 0 || B <= 0 || H <= 0 || ldh < H) return ASR_ERR_ARG;
    if (!gru_shape_ok(H)) return ASR_ERR_UNSUPPORTED;
    if ((long)B * 3 * H * 4 > (long)GRU_OOB) return ASR_ERR_UNSUPPORTED;   // one frame of P per buffer resource
    if ((long)T * B > INT_MAX) return ASR_ERR_UNSUPPORTED;
    // the step form reads h_{t-1} rows with 16-byte loads
    if (H > GR_HMAX && ((ldh & 3) != 0 || ((uintptr_t)hid & 15) != 0 || ((uintptr_t)h0 & 15) != 0))
        return ASR_ERR_UNSUPPORTED;
    return ASR_OK;
}

}  // namespace asr

extern "C" {

size_t asr_gru_workspace_bytes(int T, int B, int H) {
    if (T <= 0 || B <= 0 || !asr::gru_shape_ok(H) || (long)T * B > INT_MAX) return 0;
    // P [T*B][3H] (H % 16 == 0: a multiple of 16 bytes)
    return (size_t)T * B * 3 * H * sizeof(float);
}

int asr_gru_recur_fwd(const float* P, const float* h0, const float* W_hh, const float* b_ih, const float* b_hh,
                      float* hid, long ldh, float* hT, const int32_t* lengths, int T, int B, int H, int reverse,
                      asr_stream_t s) {
    if (!P || !W_hh || !b_ih || !b_hh || !hid) return ASR_ERR_ARG;
    if (int rc = asr::gru_check(ldh, T, B, H, hid, h0)) return rc;
    return asr::gru_recur_launch(P, h0, W_hh, b_ih, b_hh, hid, ldh, hT, lengths, T, B, H, reverse ? 1 : 0,
                                 asr_stream(s));
}

int asr_gru_fwd(const float* x, const float* h0, const float* W_ih, const float* W_hh, const float* b_ih,
                const float* b_hh, float* hid, long ldh, float* hT, const int32_t* lengths, void* work, int T, int B,
                int in, int H, int reverse, asr_stream_t s) {
    if (!x || !W_ih || !W_hh || !b_ih || !b_hh || !hid || !work || in <= 0) return ASR_ERR_ARG;
    if (int rc = asr::gru_check(ldh, T, B, H, hid, h0)) return rc;
    // P = x.W_ih for all T frames: asr_linear_fwd(x, W_ih, NULL, P, T*B, in, 3H, ASR_EPI_NONE)
    asr::GemmArgs g{};
    g.A = x; g.B = W_ih; g.C = (float*)work;
    g.M = T * B; g.N = 3 * H; g.K = in;
    g.sam = in; g.sak = 1; g.sbk = 3 * H; g.sbn = 1; g.ldc = 3 * H;
    if (int rc = asr::gemm_launch(g, asr::EPI_NONE, asr_stream(s))) return rc;
    return asr_gru_recur_fwd((const float*)work, h0, W_hh, b_ih, b_hh, hid, ldh, hT, lengths, T, B, H, reverse, s);
}

}  // extern "C"
