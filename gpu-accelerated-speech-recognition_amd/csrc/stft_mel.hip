// torch.stft-style log-mel front end (asr_stft_*) and asr_add_pos_fwd: DESIGN.md section 42.
//
// The STFT of any n_fft (not only powers of two) is a matrix product on the
// fp32 matrix cores: X^T[bin][frame] = G^T[bin][n] . frames^T[n][frame], where
// the basis G[n][2 NBp] (cosine half | minus-sine half, the centred window
// folded in) is built on the host in double and rounded once to fp32.
//
// One workgroup of 4 waves handles 64 consecutive frames of one utterance, 16
// per wave; the tile grid starts at frame 0, so a frame's bits never depend on
// T, B or the utterance's position.
//  - Samples: the 63 hop + n_fft samples the tile covers are staged into LDS
//    once, reflection at both ends and the zero tail resolved by selection
//    (nothing at or past n_samples is read).  The frames are never stored as a
//    matrix: frame f is read at row stride hop.  Sample p sits at address
//    p + skew * (p / hop), skew the smallest value with (hop + skew) % 8 == 4,
//    so the 16 frames of an operand read (stride hop + skew = 4 * odd) and its
//    4 k values fall on 64 different banks for hop = 160; for an odd hop the
//    stride is still 4 * odd, and only the reads where n / hop changes inside a
//    group of 4 collide.  The offsets n + skew * (n / hop) are a small table.
//  - Basis: bins go in groups of at most 8 tiles (128 bins; re and im are 64
//    accumulator registers).  For each group the k loop runs over n_fft in
//    slabs of 16 rows x 256 columns, staged into LDS once per workgroup and
//    shared by the 4 waves; the next slab is fetched global -> registers
//    before the MFMAs of the current one and written after them (one LDS copy,
//    two barriers per slab, as attention.hip's K and V blocks).  Rows past
//    n_fft are zeros (n_fft % 16 != 0).
//  - v_mfma_f32_16x16x4_f32 (A[l & 15][k = l >> 4], B[k = l >> 4][l & 15], C
//    rows 4g + i, column c; g = l >> 4, c = l & 15): A = G^T (lane reads basis
//    row 4 kk + g, column 16 bt + c), B = the sample of frame c at 4 kk + g.
//    Register i of tile bt then holds bin 16 bt + 4 g + i of frame c, for re
//    and im alike, so P = re^2 + im^2 is lane-local, and that layout is the B
//    operand of mel^T[m][frame] = M[m][bin] . P^T[bin][frame]: step r contracts
//    bins 4 g + r over the lane groups g, the mel operand (blocks
//    [bin tile][mel tile][16 m][16 bins], one 16-byte read per lane) is indexed
//    to match.  Mel accumulators (at most 8 tiles) persist across the groups;
//    blocks whose weights are all zero are skipped by a host-built bit table.
//    The order is fixed: groups ascending, bins ascending inside a group.
//  - Epilogue in registers: floor, log, and each lane holds 4 consecutive mel
//    bins of one frame: one 16-byte store where aligned, scalar stores with the
//    same bits otherwise.  With the range clamp on, the workgroup's maximum
//    over its valid frames goes to d_work[b][tile] by a plain vector store and
//    a second kernel reduces them and applies the clamp and the affine step.
#include "asr_internal.h"
#include "gelu.h"

#include <climits>
#include <cmath>
#include <cstddef>
#include <new>
#include <vector>

namespace asr {

typedef float st_f32x4 __attribute__((ext_vector_type(4)));

constexpr int ST_FRAMES = 64;                      // frames per workgroup
constexpr int ST_KC = 16;                          // basis rows per slab
constexpr int ST_GT = 8;                           // bin tiles per group
constexpr int ST_SLAB_LD = 2 * 16 * ST_GT + 16;    // 272: the 4 rows of an operand read sit 16 banks apart
constexpr int ST_LDS_MAX = 160 * 1024;
constexpr int ST_CLAMP_ROWS = 64;

__host__ __device__ static inline int st_frames(int n, int n_fft, int hop, int center, int drop_last) {
    int f = center ? (n <= n_fft / 2 ? 0 : 1 + n / hop) : (n < n_fft ? 0 : 1 + (n - n_fft) / hop);
    if (drop_last && f > 0) f--;
    return f;
}

struct StftArgs {
    const float* wave; long ldw;
    const int32_t* nsamples;
    int32_t* frames;
    float* out; long ldo;
    float* work;
    const float* G;           // [n_fft][2 NBp]
    const float* M;           // [nbt][nmt][16][16]
    const uint32_t* mask;     // [ngroup * ST_GT]: bit mt set when block (bt, mt) has a non-zero weight
    int B, S, T, ntile, pad_to;
    int n_fft, hop, center, drop_last, n_mels, NBp, nbt, nmt, skew, nfftp, nslab, ngroup, span;
    int power, log, floor_mode, clamp, vec;
    float floor, shift, scale, range;
};

__device__ __forceinline__ int st_utt_frames(const StftArgs& a, int b, int* nb_out) {
    const int nb = a.nsamples ? min(max(a.nsamples[b], 0), a.S) : a.S;
    *nb_out = nb;
    return min(st_frames(a.pad_to > 0 ? a.pad_to : nb, a.n_fft, a.hop, a.center, a.drop_last), a.T);
}

template <int NMT>
__global__ __launch_bounds__(256) void stft_mel_kernel(const StftArgs a) {
    extern __shared__ __align__(16) float st_smem[];
    float* samp = st_smem;                              // [span]
    float* slab = samp + a.span;                        // [ST_KC][ST_SLAB_LD]
    int* offt = (int*)(slab + ST_KC * ST_SLAB_LD);      // [nfftp]
    float* wmax = (float*)(offt + a.nfftp);             // [4]

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, g = lane >> 4;
    const int tile = blockIdx.x, b = blockIdx.y;
    int nb;
    const int nfr = st_utt_frames(a, b, &nb);
    if (tile == 0 && tid == 0 && a.frames) a.frames[b] = nfr;
    const int t = tile * ST_FRAMES + 16 * w + c;
    const bool valid = t < nfr;
    const int nmt = a.nmt;

    st_f32x4 mel[NMT];
#pragma unroll
    for (int mt = 0; mt < NMT; mt++) mel[mt] = st_f32x4{0.f, 0.f, 0.f, 0.f};

    if (tile * ST_FRAMES < nfr) {   // workgroup-uniform: a tile without a valid frame only writes zeros
        // ---- samples and the offset table
        const long L = a.pad_to > 0 ? a.pad_to : nb;
        const long pad = a.center ? a.n_fft / 2 : 0, Lp = L + 2 * pad;
        const long p0 = (long)tile * ST_FRAMES * a.hop;
        const int plen = (ST_FRAMES - 1) * a.hop + a.nfftp;
        const float* wrow = a.wave + (long)b * a.ldw;
        for (int p = tid; p < plen; p += 256) {
            const long q = p0 + p;
            long j = q - pad;
            if (j < 0) j = -j;
            if (j >= L) j = 2 * (L - 1) - j;
            float v = 0.f;
            if (q < Lp && j >= 0 && j < nb) v = wrow[j];
            samp[p + a.skew * (p / a.hop)] = v;
        }
        for (int x = tid; x < a.nfftp; x += 256) offt[x] = x + a.skew * (x / a.hop);

        // ---- the DFT, group by group, slab by slab
        const int total = a.ngroup * a.nslab;
        const int srow = tid >> 6, scol = (tid & 63) * 4;        // this thread's slab elements: rows srow + 4 i
        const int half = scol >> 7, gcol = scol & 127;           // re | im half, column inside the group
        st_f32x4 pf[4];
        auto fetch = [&](int grp, int ks) {
            const int t0 = grp * ST_GT, nt = min(ST_GT, a.nbt - t0);
            const float* src = a.G + (half ? a.NBp : 0) + 16 * t0 + gcol;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int row = ks * ST_KC + 4 * i + srow;
                pf[i] = st_f32x4{0.f, 0.f, 0.f, 0.f};
                if (row < a.n_fft && gcol < 16 * nt) pf[i] = *reinterpret_cast<const st_f32x4*>(src + (long)row * 2 * a.NBp);
            }
        };
        auto stash = [&]() {
#pragma unroll
            for (int i = 0; i < 4; i++) *reinterpret_cast<st_f32x4*>(&slab[(4 * i + srow) * ST_SLAB_LD + scol]) = pf[i];
        };
        fetch(0, 0);
        stash();
        __syncthreads();

        st_f32x4 re[ST_GT], im[ST_GT];
        const float* fsamp = samp + (16 * w + c) * (a.hop + a.skew);
        int grp = 0, ks = 0;
        for (int s = 0; s < total; s++) {
            int ngrp = grp, nks = ks + 1;
            if (nks == a.nslab) { nks = 0; ngrp++; }
            if (s + 1 < total) fetch(ngrp, nks);
            if (ks == 0) {
#pragma unroll
                for (int bt = 0; bt < ST_GT; bt++) re[bt] = im[bt] = st_f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int kk = 0; kk < ST_KC / 4; kk++) {
                const float bv = fsamp[offt[ks * ST_KC + 4 * kk + g]];
                const float* arow = &slab[(4 * kk + g) * ST_SLAB_LD + c];
#pragma unroll
                for (int bt = 0; bt < ST_GT; bt++) {   // a last group's missing tiles are zero columns of the slab
                    re[bt] = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[16 * bt], bv, re[bt], 0, 0, 0);
                    im[bt] = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[16 * ST_GT + 16 * bt], bv, im[bt], 0, 0, 0);
                }
            }
            if (ks == a.nslab - 1) {   // the group's bins are complete: power, then the mel product
#pragma unroll
                for (int bt = 0; bt < ST_GT; bt++) {
                    const int BT = grp * ST_GT + bt;
                    st_f32x4 P = re[bt] * re[bt] + im[bt] * im[bt];
                    if (a.power == 1) P = st_f32x4{sqrtf(P[0]), sqrtf(P[1]), sqrtf(P[2]), sqrtf(P[3])};
                    const uint32_t mk = a.mask[BT];   // [ngroup * ST_GT]: zero for a tile that does not exist
#pragma unroll
                    for (int mt = 0; mt < NMT; mt++) {
                        if ((mk >> mt) & 1u) {
                            const st_f32x4 mw = *reinterpret_cast<const st_f32x4*>(
                                a.M + ((long)(BT * nmt + mt) * 256 + 16 * c + 4 * g));
#pragma unroll
                            for (int r = 0; r < 4; r++)
                                mel[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(mw[r], P[r], mel[mt], 0, 0, 0);
                        }
                    }
                }
            }
            __syncthreads();
            if (s + 1 < total) stash();
            __syncthreads();
            grp = ngrp; ks = nks;
        }
    }

    // ---- epilogue: floor, log, (affine), store; rows t >= frames_b are zeros
    float lmax = -INFINITY;
    float* orow = a.out + ((long)t * a.B + b) * a.ldo;
#pragma unroll
    for (int mt = 0; mt < NMT; mt++) {
        if (mt < nmt) {
            const int m0 = 16 * mt + 4 * g;
            st_f32x4 o;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                float x = mel[mt][i];
                if (a.log) {
                    x = a.floor_mode == ASR_STFT_FLOOR_ADD ? x + a.floor : fmaxf(x, a.floor);
                    // in fp64, rounded once: the fp32 logf is up to 1.7 ulp off (ln 1e-5), past the parity bound
                    x = a.log == ASR_STFT_LOG_LN ? (float)log((double)x) : (float)log10((double)x);
                    if (a.log == ASR_STFT_LOG_DB) x = 10.f * x;
                }
                if (a.clamp) {
                    if (valid && m0 + i < a.n_mels) lmax = fmaxf(lmax, x);
                } else {
                    x = (x + a.shift) * a.scale;
                }
                o[i] = valid ? x : 0.f;
            }
            if (t < a.T) {
                if (a.vec && m0 + 3 < a.n_mels) {
                    *reinterpret_cast<st_f32x4*>(orow + m0) = o;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (m0 + i < a.n_mels) orow[m0 + i] = o[i];
                }
            }
        }
    }
    if (a.clamp) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) lmax = fmaxf(lmax, __shfl_xor(lmax, d));
        if (lane == 0) wmax[w] = lmax;
        __syncthreads();
        if (tid == 0) a.work[(long)b * a.ntile + tile] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    }
}

// x = (max(x, max_b - range) + shift) * scale in place over the valid rows of utterance b; max_b is
// the maximum of the utterance's tile maxima, tiles ascending.
__global__ __launch_bounds__(256) void stft_clamp_kernel(const StftArgs a) {
    const int b = blockIdx.y, r0 = blockIdx.x * ST_CLAMP_ROWS;
    int nb;
    const int nfr = st_utt_frames(a, b, &nb);
    if (r0 >= nfr) return;
    float mx = -INFINITY;
    const int nt = (nfr + ST_FRAMES - 1) / ST_FRAMES;
    for (int j = 0; j < nt; j++) mx = fmaxf(mx, a.work[(long)b * a.ntile + j]);
    const float lo = mx - a.range;
    const int rows = min(ST_CLAMP_ROWS, nfr - r0);
    for (int i = threadIdx.x; i < rows * a.n_mels; i += 256) {
        const int r = i / a.n_mels, m = i - r * a.n_mels;
        float* p = a.out + ((long)(r0 + r) * a.B + b) * a.ldo + m;
        *p = (fmaxf(*p, lo) + a.shift) * a.scale;
    }
}

// out[t B + b] = act(x[t B + b]) + pos[t], zeros past the lengths; one wave per row.
__global__ __launch_bounds__(256) void add_pos_kernel(const float* x, long ldx, const float* pos, long ldp,
                                                       const int32_t* lengths, float* out, long ldo, int T, int B, int N,
                                                       int act, long rows) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const int t = (int)(row / B), b = (int)(row - (long)t * B);
    const bool live = t < (lengths ? min(max(lengths[b], 0), T) : T);
    const float* xr = x + row * ldx;
    const float* pr = pos + (long)t * ldp;
    float* orow = out + row * ldo;
    for (int n = lane; n < N; n += 64) {
        float v = 0.f;
        if (live) {
            v = xr[n];
            if (act) v = gelu_f32(v);
            v = v + pr[n];
        }
        orow[n] = v;
    }
}

static bool st_cfg_ok(const asr_stft_config* c) {
    if (c->n_fft < 16 || c->n_fft > 1024 || c->win_length < 2 || c->win_length > c->n_fft) return false;
    if (c->hop_length < 1 || c->hop_length > c->n_fft) return false;
    if ((c->center != 0 && c->center != 1) || (c->power != 1 && c->power != 2)) return false;
    if (c->n_mels < 1 || c->n_mels > 128) return false;
    if (c->log < ASR_STFT_LOG_NONE || c->log > ASR_STFT_LOG_DB) return false;
    if (c->floor_mode != ASR_STFT_FLOOR_CLAMP && c->floor_mode != ASR_STFT_FLOOR_ADD) return false;
    if (c->log != ASR_STFT_LOG_NONE && !(std::isfinite(c->floor) && c->floor > 0.f)) return false;
    if (!(std::isfinite(c->dyn_range) && c->dyn_range >= 0.f)) return false;
    if (!std::isfinite(c->shift) || !std::isfinite(c->scale)) return false;
    return c->drop_last == 0 || c->drop_last == 1;
}

struct StLayout {
    int NB, NBp, nbt, nmt, skew, nfftp, nslab, ngroup, span;
    size_t smem;
};

static StLayout st_layout(const asr_stft_config* c) {
    StLayout l{};
    l.NB = c->n_fft / 2 + 1;
    l.NBp = (l.NB + 15) & ~15;
    l.nbt = l.NBp / 16;
    l.nmt = (c->n_mels + 15) / 16;
    l.skew = (4 - c->hop_length % 8 + 8) % 8;
    l.nfftp = (c->n_fft + ST_KC - 1) / ST_KC * ST_KC;
    l.nslab = l.nfftp / ST_KC;
    l.ngroup = (l.nbt + ST_GT - 1) / ST_GT;
    const long pmax = (long)(ST_FRAMES - 1) * c->hop_length + l.nfftp - 1;
    l.span = (int)((pmax + l.skew * (pmax / c->hop_length) + 1 + 3) & ~3L);
    l.smem = ((size_t)l.span + ST_KC * ST_SLAB_LD + l.nfftp + 4) * 4;
    return l;
}

// G[n][2 NBp] in double, rounded once: w'[n] cos(2 pi ((n k) mod n_fft) / n_fft) | -w'[n] sin(...), w' the
// window centred inside n_fft; columns past n_fft / 2 of each half are zeros.
static void st_basis(const asr_stft_config* c, const float* window, float* G) {
    const StLayout l = st_layout(c);
    const int N = c->n_fft, left = (N - c->win_length) / 2;
    const double two_pi = 6.283185307179586476925286766559;
    for (int n = 0; n < N; n++) {
        const double wv = (n >= left && n < left + c->win_length) ? (double)window[n - left] : 0.0;
        float* row = G + (size_t)n * 2 * l.NBp;
        for (int k = 0; k < l.NBp; k++) {
            double co = 0.0, si = 0.0;
            if (k < l.NB) {
                const double ang = two_pi * (double)(((long)n * k) % N) / N;
                co = wv * std::cos(ang);
                si = -(wv * std::sin(ang));
            }
            row[k] = (float)co;
            row[l.NBp + k] = (float)si;
        }
    }
}

}  // namespace asr

struct asr_stft {
    asr_stft_config cfg;
    asr::StLayout l;
    float* d_blob;           // basis | mel blocks | block bit table
    size_t o_mel, o_mask;    // offsets in floats
};

extern "C" {

int asr_stft_num_frames(const asr_stft_config* cfg, int n_samples) {
    if (!cfg || !asr::st_cfg_ok(cfg) || n_samples < 0) return -1;
    return asr::st_frames(n_samples, cfg->n_fft, cfg->hop_length, cfg->center, cfg->drop_last);
}

int asr_stft_host_basis(const asr_stft_config* cfg, const float* h_window, float* h_G) {
    if (!cfg || !h_window || !h_G) return ASR_ERR_ARG;
    if (!asr::st_cfg_ok(cfg)) return ASR_ERR_UNSUPPORTED;
    asr::st_basis(cfg, h_window, h_G);
    return ASR_OK;
}

int asr_stft_create(const asr_stft_config* cfg, const float* h_window, const float* h_mel, asr_stft_t** out) {
    if (!cfg || !h_window || !h_mel || !out) return ASR_ERR_ARG;
    *out = nullptr;
    if (!asr::st_cfg_ok(cfg)) return ASR_ERR_UNSUPPORTED;
    const asr::StLayout l = asr::st_layout(cfg);
    if (l.smem > (size_t)asr::ST_LDS_MAX) return ASR_ERR_UNSUPPORTED;   // the tile's samples do not fit in LDS
    asr_stft* h = new (std::nothrow) asr_stft();
    if (!h) return ASR_ERR_OOM;
    h->cfg = *cfg;
    h->l = l;
    const size_t nG = (size_t)cfg->n_fft * 2 * l.NBp, nM = (size_t)l.nbt * l.nmt * 256;
    h->o_mel = nG;
    h->o_mask = nG + nM;
    std::vector<float> blob(nG + nM + (size_t)l.ngroup * asr::ST_GT, 0.f);
    asr::st_basis(cfg, h_window, blob.data());
    for (int bt = 0; bt < l.nbt; bt++) {
        uint32_t mk = 0;
        for (int mt = 0; mt < l.nmt; mt++) {
            float* blk = blob.data() + h->o_mel + ((size_t)bt * l.nmt + mt) * 256;
            for (int r = 0; r < 16; r++)
                for (int j = 0; j < 16; j++) {
                    const int m = 16 * mt + r, k = 16 * bt + j;
                    const float v = (m < cfg->n_mels && k < l.NB) ? h_mel[(size_t)m * l.NB + k] : 0.f;
                    blk[16 * r + j] = v;
                    if (v != 0.f) mk |= 1u << mt;
                }
        }
        blob[h->o_mask + bt] = __builtin_bit_cast(float, mk);
    }
    hipError_t e = hipMalloc((void**)&h->d_blob, blob.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(h->d_blob, blob.data(), blob.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        asr_internal_set_error("asr_stft_create tables", hipGetErrorString(e), __FILE__, __LINE__);
        if (h->d_blob) (void)hipFree(h->d_blob);
        delete h;
        return e == hipErrorOutOfMemory ? ASR_ERR_OOM : ASR_ERR_HIP;
    }
    *out = h;
    return ASR_OK;
}

int asr_stft_destroy(asr_stft_t* h) {
    if (!h) return ASR_ERR_ARG;
    hipError_t e = hipFree(h->d_blob);
    delete h;
    return e == hipSuccess ? ASR_OK : ASR_ERR_HIP;
}

size_t asr_stft_workspace_bytes(const asr_stft_t* h, int T, int B) {
    if (!h || T <= 0 || B <= 0 || !(h->cfg.dyn_range > 0.f)) return 0;
    const size_t ntile = ((size_t)T + asr::ST_FRAMES - 1) / asr::ST_FRAMES;
    return (ntile * B * sizeof(float) + 15) & ~(size_t)15;
}

int asr_stft_fwd(asr_stft_t* h, const float* d_wave, long ldw, const int32_t* d_nsamples, int B, int S, int pad_to,
                 float* d_out, long ldo, int32_t* d_frames, void* d_work, int T, asr_stream_t s) {
    if (!h || !d_wave || !d_out || B <= 0 || S <= 0 || T <= 0) return ASR_ERR_ARG;
    const asr_stft_config& c = h->cfg;
    if (pad_to < 0 || (pad_to > 0 && pad_to < S)) return ASR_ERR_ARG;
    if (ldw < S || ldo < c.n_mels ||
        T < asr::st_frames(pad_to > 0 ? pad_to : S, c.n_fft, c.hop_length, c.center, c.drop_last))
        return ASR_ERR_ARG;
    const bool clamp = c.dyn_range > 0.f;
    if (clamp && !d_work) return ASR_ERR_ARG;
    const int ntile = (T + asr::ST_FRAMES - 1) / asr::ST_FRAMES;
    if ((long)T * B > (1L << 25) || B > 65535) return ASR_ERR_UNSUPPORTED;

    const asr::StLayout& l = h->l;
    asr::StftArgs a{};
    a.wave = d_wave; a.ldw = ldw; a.nsamples = d_nsamples; a.frames = d_frames;
    a.out = d_out; a.ldo = ldo; a.work = (float*)d_work;
    a.G = h->d_blob; a.M = h->d_blob + h->o_mel; a.mask = (const uint32_t*)(h->d_blob + h->o_mask);
    a.B = B; a.S = S; a.T = T; a.ntile = ntile; a.pad_to = pad_to;
    a.n_fft = c.n_fft; a.hop = c.hop_length; a.center = c.center; a.drop_last = c.drop_last; a.n_mels = c.n_mels;
    a.NBp = l.NBp; a.nbt = l.nbt; a.nmt = l.nmt; a.skew = l.skew; a.nfftp = l.nfftp; a.nslab = l.nslab;
    a.ngroup = l.ngroup; a.span = l.span;
    a.power = c.power; a.log = c.log; a.floor_mode = c.floor_mode; a.clamp = clamp ? 1 : 0;
    a.vec = (ldo % 4 == 0 && ((uintptr_t)d_out & 15) == 0) ? 1 : 0;
    a.floor = c.floor; a.shift = c.shift; a.scale = c.scale; a.range = c.dyn_range;

    const dim3 grid((unsigned)ntile, (unsigned)B), block(256);
    hipStream_t st = asr_stream(s);
    const int smem = (int)l.smem;
    if (l.nmt <= 2) {
        static AsrAttrOnce once;
        if (int rc = once.set(reinterpret_cast<const void*>(&asr::stft_mel_kernel<2>), asr::ST_LDS_MAX)) return rc;
        hipLaunchKernelGGL((asr::stft_mel_kernel<2>), grid, block, smem, st, a);
    } else if (l.nmt <= 5) {
        static AsrAttrOnce once;
        if (int rc = once.set(reinterpret_cast<const void*>(&asr::stft_mel_kernel<5>), asr::ST_LDS_MAX)) return rc;
        hipLaunchKernelGGL((asr::stft_mel_kernel<5>), grid, block, smem, st, a);
    } else {
        static AsrAttrOnce once;
        if (int rc = once.set(reinterpret_cast<const void*>(&asr::stft_mel_kernel<8>), asr::ST_LDS_MAX)) return rc;
        hipLaunchKernelGGL((asr::stft_mel_kernel<8>), grid, block, smem, st, a);
    }
    ASR_LAUNCH_TRY();
    if (clamp) {
        const dim3 cgrid((unsigned)((T + asr::ST_CLAMP_ROWS - 1) / asr::ST_CLAMP_ROWS), (unsigned)B);
        hipLaunchKernelGGL(asr::stft_clamp_kernel, cgrid, block, 0, st, a);
        ASR_LAUNCH_TRY();
    }
    return ASR_OK;
}

int asr_add_pos_fwd(const float* d_x, long ldx, const float* d_pos, long ldp, const int32_t* d_lengths, float* d_out,
                    long ldo, int T, int B, int N, int act, asr_stream_t s) {
    if (!d_x || !d_pos || !d_out || T <= 0 || B <= 0 || N <= 0) return ASR_ERR_ARG;
    if (ldx < N || ldp < N || ldo < N || (act != ASR_ADD_POS_ACT_NONE && act != ASR_ADD_POS_ACT_GELU)) return ASR_ERR_ARG;
    const long rows = (long)T * B;
    if (rows > INT_MAX) return ASR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(asr::add_pos_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, asr_stream(s), d_x, ldx,
                       d_pos, ldp, d_lengths, d_out, ldo, T, B, N, act, rows);
    ASR_LAUNCH_TRY();
    return ASR_OK;
}

}  // extern "C"
