// Audio front end: waveform -> log-mel / MFCC features with a context window
// (asr_fbank_*; the semantics are in include/asr_amd.h).
//
// fbank_kernel: one wave per frame, WPB waves (frames) per workgroup and
// FB_FRAMES_PER_WG frames per workgroup in all, the whole chain on chip:
//   1. the frame's samples, pre-emphasised from the absolute sample index and
//      windowed, go from global memory straight into the registers of the
//      first butterfly pass: z[j] = x[2j] + i x[2j+1], an M = n_fft/2 point
//      complex sequence;
//   2. Stockham autosort FFT of z in LDS, radix 4 with one closing radix-2
//      pass when log2 M is odd.  A pass reads its inputs lane-contiguously
//      (element j + r*M/R of butterfly j), so only the stores are strided;
//      all of a pass's inputs are in registers before its first store, so one
//      buffer per wave is enough.  Then the split step X[k] = E[k] - i W_N^k
//      O[k] and P[k] = |X[k]|^2 for k = 0 .. M, written over the buffer;
//   3. mel: each filter touches only its own bin range (first bin, bins, offset
//      into the packed weights; a bin is in at most two filters, so the packed
//      weights are at most 2 (M + 1) floats).  The filters are cut into at most
//      64 (128 for n_mels > 64) work items, the widest halved until every lane
//      has one; a lane sums its item, lane m then adds filter m's items in
//      order and takes e = ln(max(E, floor));
//   4. DCT: lane d sums dctT[m][d] e[m] over m (dctT transposed so that lanes
//      read consecutive words, e[m] is a broadcast read), and writes the
//      D-vector.
// The twiddles W_N^j (j < N), the packed mel weights and the DCT matrix are
// loaded into LDS once per workgroup; no sincos on the device.
//
// LDS: re[] and im[] are separate float arrays indexed by fb_pad(i) = i + i/16.
// ds_write_b32 is serviced in two groups of 32 lanes over 32 banks and a 2-way
// store conflict costs nothing extra.  The stores of a pass with Ns = 1, 4,
// 16, ... go to (j / Ns) * Ns * R + j % Ns + r * Ns: without padding lanes hit
// 8 banks (4-way); with one pad word per 16 every pass of every size is at
// most 2-way.  The lane-contiguous loads cross one pad word per 32 lanes (one
// bank read twice: 3 cycles instead of 2).
//
// Waves of a workgroup never wait for each other after the table load: the
// phases of a frame are ordered by wave-level fences only (LDS operations of
// one wave execute in issue order).
//
// fbank_context_kernel (n_context > 0): the first kernel writes base frames
// batch-major [B][T][D] into the workspace, so output row (t, b) is the
// F = D (2C + 1) consecutive floats from base frame t - C of utterance b with
// the blocks outside [0, frames_b) zeroed: one wave copies one row.
#include "asr_internal.h"
#include "fbank_tables.h"

#include <climits>
#include <cmath>
#include <cstddef>
#include <new>
#include <vector>

namespace asr {

constexpr int FB_FRAMES_PER_WG = 64;       // the tables are loaded into LDS once per workgroup
constexpr int FB_MAX_MELS = 128;
constexpr int FB_MAX_CONTEXT = 16;
constexpr int FB_MAX_FEATURES = 4096;
constexpr int FB_DCT_LDS_FLOATS = 4096;   // a larger DCT matrix is read from global memory
constexpr int FB_MEL_SPLIT_MIN = 8;       // a filter piece of fewer bins is not split further
constexpr int FB_CTX_WAVES = 4;           // rows per workgroup of the context kernel

struct FbankArgs {
    const float* wave;
    long ldw;
    const int32_t* nsamples;
    float* out;          // element (t, b, d) at out[t * st + b * sb + d]
    long st, sb;
    int32_t* frames;
    const float* window;
    const float2* tw;    // W_N^j, j < N
    const float* melw;   // packed filter weights
    const int* melitem;  // [n_items][3]: first bin, bins, offset into melw of a work item (a filter or a piece of one)
    const int* melfilt;  // [n_mels][2]: first work item and work items of a filter
    const float* dctT;   // [n_mels][D]
    int B, S, T, nblk, zero_rows;
    int win, hop, n_mels, n_items, n_mfcc, D, nnz, dct_lds;
    float preemph, log_floor;
};

__host__ __device__ static inline int fb_frames(int n, int win, int hop) { return n < win ? 0 : 1 + (n - win) / hop; }

__device__ __forceinline__ int fb_pad(int i) { return i + (i >> 4); }

// Orders the LDS phases of one wave (no instruction: LDS operations of a wave
// execute in issue order; this keeps the compiler from moving them).
__device__ __forceinline__ void fb_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

template <int LOGM>
struct FbShape {
    static constexpr int M = 1 << LOGM, N = 2 * M;
    static constexpr int VN = M / 64 > 4 ? M / 64 : 4;   // complex values a lane holds in a pass
    static constexpr int PADM = M + (M >> 4) + 1;        // fb_pad(M) + 1 floats
    static constexpr int WAVE_FLOATS = 2 * PADM;
};

// One Stockham pass of radix R with Ns = NS: butterfly j reads elements
// j + r*M/R (already in v for the first pass), multiplies by W_M^(r k M/(NS R)),
// k = j % NS, and stores to (j - k) R + k + r NS.
template <int LOGM, int R, int NS>
__device__ __forceinline__ void fb_pass(float (&vr)[FbShape<LOGM>::VN], float (&vi)[FbShape<LOGM>::VN], float* re,
                                        float* im, const float2* tw, int lane) {
    constexpr int M = 1 << LOGM, N = 2 * M;
    constexpr int NBF = M / R;                       // butterflies
    constexpr int NB = NBF >= 64 ? NBF / 64 : 1;     // per lane
    if (NS > 1) {
#pragma unroll
        for (int q = 0; q < NB; q++) {
            const int j = lane + 64 * q;
            if (NBF >= 64 || j < NBF) {
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int x = fb_pad(j + r * NBF);
                    vr[q * R + r] = re[x];
                    vi[q * R + r] = im[x];
                }
            }
        }
        fb_wave_sync();
    }
#pragma unroll
    for (int q = 0; q < NB; q++) {
        const int j = lane + 64 * q;
        if (NBF >= 64 || j < NBF) {
            float* xr = &vr[q * R];
            float* xi = &vi[q * R];
            const int k = j & (NS - 1);
            if (NS > 1) {
#pragma unroll
                for (int r = 1; r < R; r++) {
                    const float2 w = tw[r * k * (N / (NS * R))];
                    const float a = xr[r], b = xi[r];
                    xr[r] = a * w.x - b * w.y;
                    xi[r] = a * w.y + b * w.x;
                }
            }
            const int j0 = (j - k) * R + k;
            if (R == 4) {
                const float a0r = xr[0] + xr[2], a0i = xi[0] + xi[2];
                const float a1r = xr[0] - xr[2], a1i = xi[0] - xi[2];
                const float a2r = xr[1] + xr[3], a2i = xi[1] + xi[3];
                const float a3r = xi[1] - xi[3], a3i = xr[3] - xr[1];   // -i (x1 - x3)
                const int x0 = fb_pad(j0), x1 = fb_pad(j0 + NS), x2 = fb_pad(j0 + 2 * NS), x3 = fb_pad(j0 + 3 * NS);
                re[x0] = a0r + a2r; im[x0] = a0i + a2i;
                re[x1] = a1r + a3r; im[x1] = a1i + a3i;
                re[x2] = a0r - a2r; im[x2] = a0i - a2i;
                re[x3] = a1r - a3r; im[x3] = a1i - a3i;
            } else {
                const int x0 = fb_pad(j0), x1 = fb_pad(j0 + NS);
                re[x0] = xr[0] + xr[1]; im[x0] = xi[0] + xi[1];
                re[x1] = xr[0] - xr[1]; im[x1] = xi[0] - xi[1];
            }
        }
    }
    fb_wave_sync();
}

template <int LOGM, int NS>
__device__ __forceinline__ void fb_passes(float (&vr)[FbShape<LOGM>::VN], float (&vi)[FbShape<LOGM>::VN], float* re,
                                          float* im, const float2* tw, int lane) {
    constexpr int M = 1 << LOGM;
    if constexpr (NS < M) {
        constexpr int R = M / NS >= 4 ? 4 : 2;
        fb_pass<LOGM, R, NS>(vr, vi, re, im, tw, lane);
        fb_passes<LOGM, NS * R>(vr, vi, re, im, tw, lane);
    }
}

// Sample n of the frame at absolute offset off of utterance x: windowed,
// pre-emphasised; 0 past the window (the zero padding to n_fft).
__device__ __forceinline__ float fb_sample(const float* x, const float* window, int off, int n, int win, float a) {
    if (n >= win) return 0.f;
    const int i = off + n;
    const float prev = i > 0 ? x[i - 1] : 0.f;
    return window[n] * (x[i] - a * prev);
}

// c_d = sum_m dctT[m][d] e[m]: lane d reads consecutive words of row m of the
// transposed matrix, e[m] is a broadcast read.
__device__ __forceinline__ void fb_dct(const float* dctT, const float* ev, float* orow, int nm, int D, int lane) {
    for (int d = lane; d < D; d += 64) {
        float acc = 0.f;
#pragma unroll 8
        for (int m = 0; m < nm; m++) acc += dctT[m * D + d] * ev[m];
        orow[d] = acc;
    }
}

// A lane's share of the mel stage, the same for every frame: work items lane
// and lane + 64 (bins [s, s + c) with weights melw[o ..]) and filters lane and
// lane + 64 (work items [f0, f0 + nf)).
struct FbLane {
    int s[2], c[2], o[2], f0[2], nf[2];
};

template <int LOGM>
__device__ __forceinline__ void fb_frame(const FbankArgs& a, const FbLane& ln, const float* x, int off, float* orow, float* re, float* im,
                                         const float2* tw, const float* melw, const float* dctT, int lane) {
    constexpr int M = 1 << LOGM, VN = FbShape<LOGM>::VN;
    constexpr int NBF = M / 4, NB = NBF >= 64 ? NBF / 64 : 1;
    float vr[VN], vi[VN];
    // the first pass's inputs: element p = j + r M/4 is samples 2p, 2p + 1
#pragma unroll
    for (int q = 0; q < NB; q++) {
        const int j = lane + 64 * q;
        if (NBF >= 64 || j < NBF) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int n = 2 * (j + r * NBF);
                vr[q * 4 + r] = fb_sample(x, a.window, off, n, a.win, a.preemph);
                vi[q * 4 + r] = fb_sample(x, a.window, off, n + 1, a.win, a.preemph);
            }
        }
    }
    fb_passes<LOGM, 1>(vr, vi, re, im, tw, lane);

    // split step and power: X[k] = E - i W_N^k O, E = (Z[k] + conj Z[M-k]) / 2, O = (Z[k] - conj Z[M-k]) / 2
    constexpr int NK = M / 64;
    float p[NK], pm = 0.f;
#pragma unroll
    for (int q = 0; q < NK; q++) {
        const int k = lane + 64 * q;
        const int x0 = fb_pad(k), x1 = fb_pad((M - k) & (M - 1));
        const float zr = re[x0], zi = im[x0], cr = re[x1], ci = im[x1];
        const float er = 0.5f * (zr + cr), ei = 0.5f * (zi - ci);
        const float qr = 0.5f * (zr - cr), qi = 0.5f * (zi + ci);
        const float2 w = tw[k];
        const float tr = w.x * qr - w.y * qi, ti = w.x * qi + w.y * qr;
        const float xr = er + ti, xi = ei - tr;
        p[q] = xr * xr + xi * xi;
        if (q == 0) pm = (zr - zi) * (zr - zi);   // lane 0: X[M] = Re Z[0] - Im Z[0]
    }
    fb_wave_sync();
#pragma unroll
    for (int q = 0; q < NK; q++) re[fb_pad(lane + 64 * q)] = p[q];
    if (lane == 0) re[fb_pad(M)] = pm;
    fb_wave_sync();

    // mel: partial sums of the work items into im[] (dead since the split
    // step), then filter m = the sum of its items in order, log
#pragma unroll
    for (int r = 0; r < 2; r++) {
        if (lane + 64 * r < a.n_items) {
            float acc = 0.f;
#pragma unroll 4
            for (int j = 0; j < ln.c[r]; j++) acc += melw[ln.o[r] + j] * re[fb_pad(ln.s[r] + j)];
            im[lane + 64 * r] = acc;
        }
    }
    fb_wave_sync();
    // P is dead: e[] goes over the start of re[]
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const int m = lane + 64 * r;
        if (m < a.n_mels) {
            float acc = 0.f;
            for (int i = 0; i < ln.nf[r]; i++) acc += im[ln.f0[r] + i];
            const float e = logf(fmaxf(acc, a.log_floor));
            if (a.n_mfcc == 0) orow[m] = e;
            else re[m] = e;
        }
    }
    fb_wave_sync();
    if (a.n_mfcc == 0) return;
    if (a.dct_lds) fb_dct(dctT, re, orow, a.n_mels, a.D, lane);
    else fb_dct(a.dctT, re, orow, a.n_mels, a.D, lane);
    fb_wave_sync();   // the reads of e are done before the next frame's stores
}

template <int LOGM, int WPB>
__global__ __launch_bounds__(64 * WPB) void fbank_kernel(const FbankArgs a) {
    constexpr int N = 2 << LOGM;
    extern __shared__ float4 fb_smem[];
    float* smem = (float*)fb_smem;
    float2* tw = (float2*)smem;
    float* melw = smem + 2 * N;
    float* dctT = melw + ((a.nnz + 3) & ~3);
    float* waves = dctT + (a.dct_lds ? ((a.n_mels * a.D + 3) & ~3) : 0);
    for (int i = threadIdx.x; i < N; i += 64 * WPB) tw[i] = a.tw[i];
    for (int i = threadIdx.x; i < a.nnz; i += 64 * WPB) melw[i] = a.melw[i];
    if (a.dct_lds)
        for (int i = threadIdx.x; i < a.n_mels * a.D; i += 64 * WPB) dctT[i] = a.dctT[i];
    __syncthreads();

    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* re = waves + w * FbShape<LOGM>::WAVE_FLOATS;
    float* im = re + FbShape<LOGM>::PADM;
    const int b = blockIdx.x / a.nblk, blk = blockIdx.x - b * a.nblk;
    const int n = a.nsamples ? min(max(a.nsamples[b], 0), a.S) : a.S;
    const int frames = min(fb_frames(n, a.win, a.hop), a.T);
    if (blk == 0 && threadIdx.x == 0 && a.frames) a.frames[b] = frames;
    const float* x = a.wave + (long)b * a.ldw;
    FbLane ln;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const int it = lane + 64 * r;
        const bool hi = it < a.n_items, hm = it < a.n_mels;
        ln.s[r] = hi ? a.melitem[3 * it] : 0;
        ln.c[r] = hi ? a.melitem[3 * it + 1] : 0;
        ln.o[r] = hi ? a.melitem[3 * it + 2] : 0;
        ln.f0[r] = hm ? a.melfilt[2 * it] : 0;
        ln.nf[r] = hm ? a.melfilt[2 * it + 1] : 0;
    }
    for (int i = 0; i < FB_FRAMES_PER_WG / WPB; i++) {
        const int t = blk * FB_FRAMES_PER_WG + i * WPB + w;
        if (t >= a.T) break;
        float* orow = a.out + (long)t * a.st + (long)b * a.sb;
        if (t >= frames) {
            if (a.zero_rows)
                for (int d = lane; d < a.D; d += 64) orow[d] = 0.f;
            continue;
        }
        fb_frame<LOGM>(a, ln, x, t * a.hop, orow, re, im, tw, melw, dctT, lane);
    }
}

// Output row (t, b) = base frames t - C .. t + C of utterance b, a run of F
// consecutive floats of base [B][T][D], zeros outside [0, frames_b).
__global__ __launch_bounds__(64 * FB_CTX_WAVES) void fbank_context_kernel(const float* base, float* out, long ldo,
                                                                          const int32_t* nsamples, int B, int S, int T,
                                                                          int win, int hop, int D, int C) {
    const long row = (long)blockIdx.x * FB_CTX_WAVES + (threadIdx.x >> 6);
    if (row >= (long)T * B) return;
    const int lane = threadIdx.x & 63;
    const int t = (int)(row / B), b = (int)(row - (long)t * B);
    const int n = nsamples ? min(max(nsamples[b], 0), S) : S;
    const int frames = min(fb_frames(n, win, hop), T);
    const int F = D * (2 * C + 1);
    float* o = out + row * ldo;
    // columns [lo, hi) come from frames inside the utterance
    int lo = 0, hi = 0;
    if (t < frames) {
        lo = max(0, C - t) * D;
        hi = min(2 * C + 1, frames - t + C) * D;
    }
    const float* src = base + ((long)b * T + (t - C)) * D;
    for (int f = lane; f < F; f += 64) o[f] = (f >= lo && f < hi) ? src[f] : 0.f;
}

// ---------------------------------------------------------------- host side
static bool fb_cfg_ok(const asr_fbank_config* c) {
    if (!c) return false;
    if (!(c->sample_rate > 0.f) || !std::isfinite(c->sample_rate)) return false;
    if (c->n_fft != 256 && c->n_fft != 512 && c->n_fft != 1024 && c->n_fft != 2048) return false;
    if (c->win_length < 2 || c->win_length > c->n_fft || c->hop_length < 1) return false;
    if (c->window != ASR_FBANK_WIN_HANN && c->window != ASR_FBANK_WIN_HAMMING && c->window != ASR_FBANK_WIN_RECT)
        return false;
    if (!(c->preemph >= 0.f && c->preemph < 1.f)) return false;
    if (c->n_mels < 1 || c->n_mels > FB_MAX_MELS) return false;
    if (!(c->f_min >= 0.f && c->f_min < c->f_max && (double)c->f_max <= 0.5 * (double)c->sample_rate)) return false;
    if (!(c->log_floor > 0.f) || !std::isfinite(c->log_floor)) return false;
    if (c->n_mfcc < 0 || c->n_mfcc > c->n_mels) return false;
    if (c->n_context < 0 || c->n_context > FB_MAX_CONTEXT) return false;
    const int D = c->n_mfcc ? c->n_mfcc : c->n_mels;
    return D * (2 * c->n_context + 1) <= FB_MAX_FEATURES;
}

static int fb_dim(const asr_fbank_config* c) { return c->n_mfcc ? c->n_mfcc : c->n_mels; }

static void fb_window(const asr_fbank_config* c, float* w) {
    const double pi = 3.14159265358979323846;
    for (int n = 0; n < c->win_length; n++) {
        const double cs = std::cos(2.0 * pi * n / (c->win_length - 1));
        w[n] = c->window == ASR_FBANK_WIN_HANN      ? (float)(0.5 - 0.5 * cs)
               : c->window == ASR_FBANK_WIN_HAMMING ? (float)(0.54 - 0.46 * cs)
                                                    : 1.f;
    }
}

// mel [n_mels][n_fft/2 + 1]
static void fb_mel(const asr_fbank_config* c, float* mel) {
    const int nm = c->n_mels, nb = c->n_fft / 2 + 1;
    const double m0 = 2595.0 * std::log10(1.0 + (double)c->f_min / 700.0);
    const double m1 = 2595.0 * std::log10(1.0 + (double)c->f_max / 700.0);
    const double step = (m1 - m0) / (nm + 1);
    std::vector<double> hz(nm + 2);
    for (int i = 0; i < nm + 2; i++) {
        const double m = i == nm + 1 ? m1 : i * step + m0;
        hz[i] = 700.0 * (std::pow(10.0, m / 2595.0) - 1.0);
    }
    for (int m = 0; m < nm; m++) {
        const double lo = hz[m], ce = hz[m + 1], hi = hz[m + 2];
        for (int k = 0; k < nb; k++) {
            const double f = (double)k * (double)c->sample_rate / c->n_fft;
            const double up = (f - lo) / (ce - lo), down = (hi - f) / (hi - ce);
            const double w = std::fmin(up, down);
            mel[(size_t)m * nb + k] = w > 0.0 ? (float)w : 0.f;
        }
    }
}

// dct [D][n_mels], orthonormal DCT-II
static void fb_dct(const asr_fbank_config* c, float* dct) {
    const double pi = 3.14159265358979323846;
    const int nm = c->n_mels;
    for (int k = 0; k < c->n_mfcc; k++) {
        const double s = std::sqrt((k == 0 ? 1.0 : 2.0) / nm);
        for (int m = 0; m < nm; m++) dct[(size_t)k * nm + m] = (float)(s * std::cos(pi * k * (2 * m + 1) / (2.0 * nm)));
    }
}

// The mel work items, the packed weights and the layout of the blob and of the
// kernel's LDS (fbank_tables.h).
void fb_build_tables(const asr_fbank_config* cfg, const float* mel, int wpb, FbTables* t) {
    const int N = cfg->n_fft, M = N / 2, nb = M + 1, nm = cfg->n_mels, D = fb_dim(cfg);
    // each filter's own bin range, weights packed; then work items: one per
    // filter, the widest split in two until every lane of the mel stage has one
    // (a filter's items stay adjacent and in bin order, so its sum has one order)
    typedef FbMelItem Item;
    std::vector<Item>& items = t->items;
    std::vector<float>& packed = t->packed;
    items.clear();
    packed.clear();
    for (int m = 0; m < nm; m++) {
        int first = -1, last = -2;
        for (int k = 0; k < nb; k++)
            if (mel[(size_t)m * nb + k] != 0.f) {
                if (first < 0) first = k;
                last = k;
            }
        items.push_back({first < 0 ? 0 : first, first < 0 ? 0 : last - first + 1, (int)packed.size(), m});
        for (int k = first; first >= 0 && k <= last; k++) packed.push_back(mel[(size_t)m * nb + k]);
    }
    const size_t cap = 64 * (size_t)((nm + 63) / 64);
    while (items.size() < cap) {
        size_t w = 0;
        for (size_t i = 1; i < items.size(); i++)
            if (items[i].c > items[w].c) w = i;
        if (items[w].c < asr::FB_MEL_SPLIT_MIN) break;
        const Item it = items[w];
        const int c0 = (it.c + 1) / 2;
        items[w].c = c0;
        items.insert(items.begin() + w + 1, Item{it.s + c0, it.c - c0, it.o + c0, it.f});
    }
    std::vector<int>& idx = t->idx;
    std::vector<int>& filt = t->filt;
    idx.assign(3 * items.size(), 0);
    filt.assign(2 * nm, 0);
    for (size_t i = 0; i < items.size(); i++) {
        idx[3 * i] = items[i].s; idx[3 * i + 1] = items[i].c; idx[3 * i + 2] = items[i].o;
        if (filt[2 * items[i].f + 1]++ == 0) filt[2 * items[i].f] = (int)i;
    }
    t->n_items = (int)items.size();
    t->nnz = (int)packed.size();
    t->dct_lds = cfg->n_mfcc > 0 && nm * D <= asr::FB_DCT_LDS_FLOATS;
    auto up4 = [](size_t v) { return (v + 3) & ~(size_t)3; };
    const size_t wave_floats = 2 * (size_t)(M + (M >> 4) + 1);
    t->smem = (2 * (size_t)N + up4(t->nnz) + (t->dct_lds ? up4((size_t)nm * D) : 0) + wpb * wave_floats) * 4;
    t->o_tw = up4(cfg->win_length);
    t->o_melw = t->o_tw + 2 * (size_t)N;
    t->o_melidx = t->o_melw + up4(t->nnz);
    t->o_melfilt = t->o_melidx + up4(idx.size());
    t->o_dct = t->o_melfilt + up4(filt.size());
    t->total = t->o_dct + up4((size_t)nm * D);
}

}  // namespace asr

struct asr_fbank {
    asr_fbank_config cfg;
    int D, F, logm, wpb, nnz, n_items, dct_lds;
    size_t smem;
    float* d_blob;   // window | twiddles | packed mel weights | mel work items | filters' items | transposed DCT
    size_t o_tw, o_melw, o_melidx, o_melfilt, o_dct;   // offsets in floats
};

extern "C" {

int asr_fbank_num_frames(const asr_fbank_config* cfg, int n_samples) {
    if (!asr::fb_cfg_ok(cfg) || n_samples < 0) return -1;
    return asr::fb_frames(n_samples, cfg->win_length, cfg->hop_length);
}

int asr_fbank_feature_dim(const asr_fbank_config* cfg) {
    if (!asr::fb_cfg_ok(cfg)) return 0;
    return asr::fb_dim(cfg) * (2 * cfg->n_context + 1);
}

int asr_fbank_host_tables(const asr_fbank_config* cfg, float* h_window, float* h_mel, float* h_dct) {
    if (!cfg) return ASR_ERR_ARG;
    if (!asr::fb_cfg_ok(cfg)) return ASR_ERR_UNSUPPORTED;
    if (h_window) asr::fb_window(cfg, h_window);
    if (h_mel) asr::fb_mel(cfg, h_mel);
    if (h_dct && cfg->n_mfcc > 0) asr::fb_dct(cfg, h_dct);
    return ASR_OK;
}

int asr_fbank_create(const asr_fbank_config* cfg, asr_fbank_t** out) {
    if (!cfg || !out) return ASR_ERR_ARG;
    *out = nullptr;
    if (!asr::fb_cfg_ok(cfg)) return ASR_ERR_UNSUPPORTED;
    asr_fbank* h = new (std::nothrow) asr_fbank();
    if (!h) return ASR_ERR_OOM;
    h->cfg = *cfg;
    h->D = asr::fb_dim(cfg);
    h->F = h->D * (2 * cfg->n_context + 1);
    const int N = cfg->n_fft, M = N / 2, nb = M + 1, nm = cfg->n_mels, D = h->D;
    h->logm = M == 128 ? 7 : M == 256 ? 8 : M == 512 ? 9 : 10;
    h->wpb = h->logm == 10 ? 2 : 4;

    std::vector<float> win(cfg->win_length), mel((size_t)nm * nb), dct((size_t)D * nm);
    asr::fb_window(cfg, win.data());
    asr::fb_mel(cfg, mel.data());
    if (cfg->n_mfcc > 0) asr::fb_dct(cfg, dct.data());
    asr::FbTables tb;
    asr::fb_build_tables(cfg, mel.data(), h->wpb, &tb);
    const std::vector<float>& packed = tb.packed;
    const std::vector<int>&idx = tb.idx, &filt = tb.filt;
    h->n_items = tb.n_items;
    h->nnz = tb.nnz;
    h->dct_lds = tb.dct_lds;
    h->smem = tb.smem;
    if (h->smem > 65536) {   // cannot happen with the limits above; never launch past the static budget
        delete h;
        return ASR_ERR_UNSUPPORTED;
    }
    h->o_tw = tb.o_tw;
    h->o_melw = tb.o_melw;
    h->o_melidx = tb.o_melidx;
    h->o_melfilt = tb.o_melfilt;
    h->o_dct = tb.o_dct;
    const size_t total = tb.total;
    std::vector<float> blob(total, 0.f);
    std::copy(win.begin(), win.end(), blob.begin());
    const double pi = 3.14159265358979323846;
    for (int j = 0; j < N; j++) {
        blob[h->o_tw + 2 * j] = (float)std::cos(2.0 * pi * j / N);
        blob[h->o_tw + 2 * j + 1] = (float)(-std::sin(2.0 * pi * j / N));
    }
    std::copy(packed.begin(), packed.end(), blob.begin() + h->o_melw);
    for (size_t i = 0; i < idx.size(); i++) blob[h->o_melidx + i] = __builtin_bit_cast(float, idx[i]);
    for (size_t i = 0; i < filt.size(); i++) blob[h->o_melfilt + i] = __builtin_bit_cast(float, filt[i]);
    if (cfg->n_mfcc > 0)
        for (int k = 0; k < D; k++)
            for (int m = 0; m < nm; m++) blob[h->o_dct + (size_t)m * D + k] = dct[(size_t)k * nm + m];
    hipError_t e = hipMalloc((void**)&h->d_blob, total * 4);
    if (e == hipSuccess) e = hipMemcpy(h->d_blob, blob.data(), total * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        asr_internal_set_error("asr_fbank_create tables", hipGetErrorString(e), __FILE__, __LINE__);
        if (h->d_blob) (void)hipFree(h->d_blob);
        delete h;
        return e == hipErrorOutOfMemory ? ASR_ERR_OOM : ASR_ERR_HIP;
    }
    *out = h;
    return ASR_OK;
}

int asr_fbank_destroy(asr_fbank_t* h) {
    if (!h) return ASR_ERR_ARG;
    hipError_t e = hipFree(h->d_blob);
    delete h;
    return e == hipSuccess ? ASR_OK : ASR_ERR_HIP;
}

size_t asr_fbank_workspace_bytes(const asr_fbank_t* h, int T, int B) {
    if (!h || T <= 0 || B <= 0 || h->cfg.n_context == 0) return 0;
    return (((size_t)T * B * h->D * sizeof(float)) + 15) & ~(size_t)15;
}

int asr_fbank_fwd(asr_fbank_t* h, const float* d_wave, long ldw, const int32_t* d_nsamples, int B, int S, float* d_out,
                  long ldo, int32_t* d_frames, void* d_work, int T, asr_stream_t s) {
    if (!h || !d_wave || !d_out || B <= 0 || S <= 0 || T <= 0) return ASR_ERR_ARG;
    const asr_fbank_config& c = h->cfg;
    if (ldw < S || ldo < h->F || T < asr::fb_frames(S, c.win_length, c.hop_length)) return ASR_ERR_ARG;
    const int C = c.n_context;
    if (C > 0 && !d_work) return ASR_ERR_ARG;
    const int nblk = (T + asr::FB_FRAMES_PER_WG - 1) / asr::FB_FRAMES_PER_WG;
    // one-dimensional grids: blocks * threads below 2^32
    if ((long)T * B > (1L << 25) || (long)nblk * B > (1L << 23)) return ASR_ERR_UNSUPPORTED;

    asr::FbankArgs a{};
    a.wave = d_wave; a.ldw = ldw; a.nsamples = d_nsamples; a.frames = d_frames;
    if (C > 0) { a.out = (float*)d_work; a.st = h->D; a.sb = (long)T * h->D; a.zero_rows = 0; }
    else       { a.out = d_out; a.st = (long)B * ldo; a.sb = ldo; a.zero_rows = 1; }
    a.window = h->d_blob;
    a.tw = (const float2*)(h->d_blob + h->o_tw);
    a.melw = h->d_blob + h->o_melw;
    a.melitem = (const int*)(h->d_blob + h->o_melidx);
    a.melfilt = (const int*)(h->d_blob + h->o_melfilt);
    a.dctT = h->d_blob + h->o_dct;
    a.B = B; a.S = S; a.T = T; a.nblk = nblk;
    a.win = c.win_length; a.hop = c.hop_length; a.n_mels = c.n_mels; a.n_items = h->n_items; a.n_mfcc = c.n_mfcc; a.D = h->D;
    a.nnz = h->nnz; a.dct_lds = h->dct_lds;
    a.preemph = c.preemph; a.log_floor = c.log_floor;
    const dim3 grid((unsigned)(nblk * B)), block(64 * h->wpb);
    hipStream_t st = asr_stream(s);
    switch (h->logm) {
        case 7: hipLaunchKernelGGL((asr::fbank_kernel<7, 4>), grid, block, h->smem, st, a); break;
        case 8: hipLaunchKernelGGL((asr::fbank_kernel<8, 4>), grid, block, h->smem, st, a); break;
        case 9: hipLaunchKernelGGL((asr::fbank_kernel<9, 4>), grid, block, h->smem, st, a); break;
        default: hipLaunchKernelGGL((asr::fbank_kernel<10, 2>), grid, block, h->smem, st, a); break;
    }
    ASR_LAUNCH_TRY();
    if (C > 0) {
        const long rows = (long)T * B;
        const unsigned gx = (unsigned)((rows + asr::FB_CTX_WAVES - 1) / asr::FB_CTX_WAVES);
        hipLaunchKernelGGL(asr::fbank_context_kernel, dim3(gx), dim3(64 * asr::FB_CTX_WAVES), 0, st,
                           (const float*)d_work, d_out, ldo, d_nsamples, B, S, T, c.win_length, c.hop_length, h->D, C);
        ASR_LAUNCH_TRY();
    }
    return ASR_OK;
}

}  // extern "C"
