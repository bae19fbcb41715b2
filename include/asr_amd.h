/*
 * asr_amd.h — C ABI of libasr_amd.so, the MI355X (gfx950) RNN + CTC
 * beam-search decode path.
 *
 * This is the drop-in boundary.  The reference (jrxk/GPU-Accelerated-Speech-
 * Recognition, mounted at /root/reference) is C++/CUDA with no FFI of its own;
 * its callers (main.cpp, nn_test.cpp) use the C++ classes cuMatrix / Linear /
 * RNN / RNN_Cell / CTCBeamSearch.  Those classes are re-implemented in
 * gpu-accelerated-speech-recognition_amd/api/ on top of THIS interface, and
 * every entry point below names the reference member it replaces.
 *
 * Conventions
 *  - Plain pointers and sizes only.  Pointers named d_* are device pointers
 *    (from asr_device_malloc or any other HIP allocation on the current
 *    device); h_* are host pointers.
 *  - Matrices are row-major fp32, exactly as cuMatrix stores them
 *    (cuMatrix.h:12 "rows-major"); weights are [in][out] (Linear.cu:13,
 *    RNN_Cell.cu:16-17).
 *  - Emissions are time-major [T][B][V] (CTCBeamSearch.cu:67-69
 *    getBatchAtT; RNN.cu:20 writes hiddens at offset t*B*H).
 *  - asr_stream_t is a hipStream_t; NULL means the default stream.
 *  - Every call returns an asr_status (0 = ASR_OK).  No exception crosses
 *    this boundary.  The reference prints and calls exit(0) instead
 *    (cuMatrix.h:85,103,207,218; cuMatrix.cpp:35-41; CTCBeamSearch.cu:267-270);
 *    the C++ layer in api/ restores that behaviour for drop-in callers.
 *  - All calls are asynchronous on the given stream unless documented.
 */
#ifndef ASR_AMD_H_
#define ASR_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* asr_stream_t;

typedef enum asr_status {
    ASR_OK = 0,
    ASR_ERR_ARG = 1,            /* bad argument / shape mismatch           */
    ASR_ERR_HIP = 2,            /* HIP runtime error                       */
    ASR_ERR_OOM = 3,            /* device or pinned host allocation failed */
    ASR_ERR_BEAM_OVERFLOW = 4,  /* more tied survivors than max_states     */
    ASR_ERR_UNSUPPORTED = 5,    /* shape outside what the kernels support  */
    ASR_ERR_STATE = 6,          /* call out of order (e.g. no decode yet)  */
    ASR_ERR_INTERNAL = 7        /* a decoder self-check failed (a bug)     */
} asr_status;

const char* asr_status_string(int status);
/* Library build identification ("gfx950 ..."). */
const char* asr_version(void);

/* ---- device / memory: replaces MemoryMonitor (MemoryMonitor.cpp:9-51) and
 *      the cudaMemcpy/cudaMemset calls of cuMatrix (cuMatrix.h:72-130). ---- */
int asr_get_device_count(int* count);
int asr_set_device(int device);
int asr_get_device(int* device);
int asr_device_malloc(void** d_ptr, size_t bytes);     /* MemoryMonitor::gpuMalloc, zero-filled */
int asr_device_free(void* d_ptr);                      /* MemoryMonitor::freeGpuMemory */
int asr_host_malloc(void** h_ptr, size_t bytes);       /* MemoryMonitor::cpuMalloc (pinned) */
int asr_host_free(void* h_ptr);                        /* MemoryMonitor::freeCpuMemory */
int asr_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes, asr_stream_t s); /* cuMatrix::toGpu */
int asr_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes, asr_stream_t s); /* cuMatrix::toCpu */
int asr_memcpy_d2d(void* d_dst, const void* d_src, size_t bytes, asr_stream_t s);
int asr_memset(void* d_ptr, int value, size_t bytes, asr_stream_t s);             /* cuMatrix::gpuClear */
int asr_stream_create(asr_stream_t* s);
int asr_stream_destroy(asr_stream_t s);
int asr_stream_sync(asr_stream_t s);
int asr_device_sync(void);

/* ---- dense ops (MFMA fp32) ---------------------------------------------- */

/* z[M,N] = x[M,K] . y[K,N]  — cuMatrix.cpp:33-70 matrixMul (cublasSgemm). */
int asr_matmul(const float* d_x, const float* d_y, float* d_z, int M, int K, int N,
               asr_stream_t s);
/* matrixMulTA (cuMatrix.cpp:73-107): z[K,N] = x[M,K]^T . y[M,N] */
int asr_matmul_ta(const float* d_x, const float* d_y, float* d_z, int M, int K, int N,
                  asr_stream_t s);
/* matrixMulTB (cuMatrix.cpp:110-145): z[M,N] = x[M,K] . y[N,K]^T */
int asr_matmul_tb(const float* d_x, const float* d_y, float* d_z, int M, int K, int N,
                  asr_stream_t s);
/* z = x + lambda*y over M*N elements — cuMatrix.cpp:147-168 matrixAdd (cublasSgeam). */
int asr_matadd(const float* d_x, const float* d_y, float* d_z, int M, int N, float lambda,
               asr_stream_t s);

typedef enum asr_epilogue {
    ASR_EPI_NONE = 0,            /* y = x.W                                         */
    ASR_EPI_BIAS = 1,            /* y = x.W + b                                     */
    ASR_EPI_BIAS_RELU = 2,       /* y = max(x.W + b, 0)  — Linear.cu:3-10 ReLU      */
    ASR_EPI_BIAS_LOGSOFTMAX = 3, /* y = log_softmax(x.W + b) per row (model.py:49)  */
    ASR_EPI_BIAS_SILU = 4        /* y = v / (1 + exp(-v)), v = x.W + b (SiLU / Swish) */
} asr_epilogue;

/* Linear::forward (Linear.cu:42-49): y[M,N] = epi(x[M,K] . W[K,N] + b[N]).
 * ASR_EPI_BIAS_LOGSOFTMAX is fused into the GEMM for N <= 64 and a row pass
 * after it otherwise.  ASR_EPI_BIAS_SILU (the Conformer's feed-forward
 * activation; no reference member) is applied where the bias is, in every
 * kernel and both arithmetics a bias GEMM can land on, so the kernel choice
 * and a row's independence of M are those of ASR_EPI_BIAS; a pre-activation
 * of -100 gives -0 (exp overflows to +inf), never NaN.  Every epilogue but
 * ASR_EPI_NONE needs d_b (NULL: ASR_ERR_ARG). */
int asr_linear_fwd(const float* d_x, const float* d_W, const float* d_b, float* d_y, int M,
                   int K, int N, int epilogue, asr_stream_t s);

/* RNN_Cell::forward (RNN_Cell.cu:65-74):
 * h_out[B,H] = tanh((x[B,in].W_ih[in,H] + h_prev[B,H].W_hh[H,H]) + (b_hh + b_ih)). */
int asr_rnn_cell_fwd(const float* d_x, const float* d_h_prev, const float* d_W_ih,
                     const float* d_W_hh, const float* d_b_ih, const float* d_b_hh,
                     float* d_h_out, int B, int in, int H, asr_stream_t s);

/* One RNN layer over a whole sequence — RNN::forward (RNN.cu:9-30) for one
 * layer: x time-major [T*B, in], h0 [B,H] (NULL = zeros, RNN.h:15-16),
 * hiddens [T*B, H].  The input projection for all T is one MFMA GEMM; the
 * recurrence runs in one launch with W_hh resident on chip (H <= 256) or as
 * T fused cell launches otherwise. */
int asr_rnn_fwd(const float* d_x, const float* d_h0, const float* d_W_ih, const float* d_W_hh,
                const float* d_b_ih, const float* d_b_hh, float* d_hiddens, int T, int B,
                int in, int H, asr_stream_t s);

/* The recurrence stage of asr_rnn_fwd alone, for callers that run the input
 * projection themselves (e.g. asr_linear_fwd(x, W_ih, NULL, hiddens, ...,
 * ASR_EPI_NONE) on another stream, so that the next batch's projection
 * overlaps this batch's recurrence): on entry d_hiddens [T*B, H] holds
 * P = x.W_ih, on return the hidden states, in place.  asr_rnn_fwd is exactly
 * this after that GEMM (RNN.cu:9-30 split at its two stages). */
int asr_rnn_recur_fwd(const float* d_h0, const float* d_W_hh, const float* d_b_ih,
                      const float* d_b_hh, float* d_hiddens, int T, int B, int H, asr_stream_t s);

/* For 384 <= H <= 1024 (H % 128 == 0, B <= 256) asr_rnn_fwd / asr_rnn_recur_fwd
 * run the whole recurrence in ONE launch whose workgroups hand h_t to each
 * other (W_hh resident in registers); it is taken only when its H/32 x
 * ceil(B/16) workgroups fit the CUs the stream may use (half of them for a
 * plain call, less other such launches in flight; the pipeline's share for
 * its own), never while the stream is capturing.  Residency is still not
 * guaranteed (other processes, other work on those CUs), so a launch that
 * waits 0.5 s without progress gives up and a one-workgroup recovery kernel
 * queued behind it on the same stream finishes the frames it had not
 * published, with the same arithmetic: the call's result is always the
 * complete recurrence, bit for bit (never a partial h with ASR_OK), only
 * slower.  This reports how many such launches ran and how many completed
 * through the recovery (counted once their stream has passed them).
 * (Replaces nothing in the reference: RNN.cu:9-30 launched T steps.) */
int asr_rnn_persist_stats(long long* launches, long long* recoveries);

/* Recurrence kernel choice for H <= 256 (H % 16 == 0), process-wide:
 * ASR_RNN_RECUR_VALU — one utterance per CU, W_hh in registers: the shortest
 *   step (~0.7-0.9 us), a whole CU per utterance;
 * ASR_RNN_RECUR_MFMA — 16 utterances per workgroup on MFMA: ~2.7 us per step
 *   on the split-bf16 arithmetic at H = 256 (~4.6 us on fp32 MFMA)
 *   but ~3x less CU time per utterance (for throughput pipelines whose
 *   production runs beside other work);
 * ASR_RNN_RECUR_AUTO (default) — MFMA from B >= 4 x CUs on.
 * Results agree to fp32 rounding (different summation order), not bit for
 * bit: under AUTO an utterance's hidden states therefore depend on the batch
 * size it runs in (a batch of >= 4 x CUs and a smaller shard of it take
 * different kernels).  Callers that need an utterance's bits to be
 * independent of the batch (utterance sharding over GPUs, re-decoding a
 * shard) pin a kind with asr_rnn_set_recurrence.  Thread-local overrides
 * set by asr_pipeline_* never leak out of the pipeline's own calls. */
enum { ASR_RNN_RECUR_AUTO = 0, ASR_RNN_RECUR_VALU = 1, ASR_RNN_RECUR_MFMA = 2 };
int asr_rnn_set_recurrence(int kind);
int asr_rnn_get_recurrence(int* kind);

/* Arithmetic of the dense fp32 contractions (GEMMs with K <= 256 and N >= 64,
 * the MFMA recurrence and the fused emission recurrence at H = 64 / 128 / 256),
 * process-wide:
 * ASR_DENSE_F32 — v_mfma_f32_16x16x4_f32 (fp32 operands);
 * ASR_DENSE_SPLIT_BF16 (default; ASR_DENSE=f32 in the environment selects
 *   the other at start-up) — every fp32 operand split into three bf16 pieces
 *   (x = h + m + l exactly) and the six significant piece products summed on
 *   v_mfma_f32_16x16x32_bf16 in fp32: as accurate as the fp32 kernels
 *   (max error against fp64 / sum |x.y|: 2.2e-7 vs 3.3e-7 for an fp32 FMA
 *   chain; tests/test_dense_x3_gpu.py), 2.7x their MFMA rate.
 * Both agree with the reference's fp32 cuBLAS to fp32 rounding, not bit for
 * bit; the choice depends on this setting and the shape only (never on M),
 * so an utterance's bits do not depend on its batch.  A pipeline keeps the
 * setting it was created under for all its batches. */
enum { ASR_DENSE_F32 = 0, ASR_DENSE_SPLIT_BF16 = 1 };
int asr_set_dense_arith(int arith);
int asr_get_dense_arith(int* arith);

/* The recurrence and the emission layer in one pass — RNN::forward's
 * recurrence (RNN.cu:9-30) followed by Linear::forward (Linear.cu:42-49) with
 * the log_softmax of baseline/model.py:49, for the acoustic model's last RNN
 * layer when H <= 256 (H % 16 == 0) and V <= 32:
 *   h_t = tanh((P_t + h_{t-1}.W_hh) + (b_hh + b_ih)),
 *   emis_t = log_softmax(h_t.W_out + b_out) per row.
 * d_P [T*B, H] holds x.W_ih (read only; asr_linear_fwd(x, W_ih, NULL, P, ...,
 * ASR_EPI_NONE)); d_emis [T*B, V]; d_hiddens [T*B, H] receives the hidden
 * states, or NULL: they are never stored (the emission projection runs on
 * the recurrence's matrix cores from on-chip h_t).  Always the MFMA
 * recurrence (16 utterances per workgroup).  Emissions agree with
 * asr_rnn_recur_fwd + asr_linear_fwd(..., ASR_EPI_BIAS_LOGSOFTMAX) to fp32
 * rounding (another summation order of h.W_out), not bit for bit.
 * ASR_ERR_UNSUPPORTED outside H <= 256, H % 16 == 0, V <= 32. */
int asr_rnn_emit_fwd(const float* d_h0, const float* d_W_hh, const float* d_b_ih,
                     const float* d_b_hh, const float* d_W_out, const float* d_b_out,
                     const float* d_P, float* d_hiddens, float* d_emis, int T, int B, int H,
                     int V, asr_stream_t s);

/* Bidirectional single-layer RNN — nn.RNN(bidirectional=True) of the Python
 * baseline (baseline/model.py:30, "bidir true"); the C++
 * RNN class (RNN.h:13-20) has no such mode, so this is an added entry point.
 * Direction d = 0 runs t = 0..T-1, d = 1 runs t = T-1..0, each with its own
 * W_ih[d] [in,H], W_hh[d] [H,H], b_ih[d], b_hh[d] (RNN_Cell layout).
 * h0: [2][B][H] (NULL = zeros).  out: [T*B, 2H] time-major, row = (h_fwd, h_bwd)
 * as torch concatenates them.  work: device scratch of
 * asr_rnn_bidir_workspace_bytes(T,B,H) bytes, 16-B aligned; H % 4 == 0.  The
 * two recurrences run concurrently (the reverse one on a library side stream
 * joined back into s). */
size_t asr_rnn_bidir_workspace_bytes(int T, int B, int H);
int asr_rnn_bidir_fwd(const float* d_x, const float* d_h0, const float* const d_W_ih[2],
                      const float* const d_W_hh[2], const float* const d_b_ih[2],
                      const float* const d_b_hh[2], float* d_out, void* d_work, int T, int B,
                      int in, int H, asr_stream_t s);

/* One LSTM layer and direction over a whole sequence — torch.nn.LSTM
 * semantics (gate order i, f, g, o).  The reference has no LSTM (its only
 * recurrent cell is the tanh RNN_Cell), so these entry points replace no
 * reference member; they are what DeepSpeech-style CTC acoustic models need.
 * x time-major [T*B, in]; W_ih [in, 4H], W_hh [H, 4H] in this library's
 * [in][out] layout, gate q of hidden unit j at column q*H + j; b_ih, b_hh [4H].
 *   z = (x_t.W_ih + h_{t-1}.W_hh) + (b_ih + b_hh)
 *   i, f, o = sigmoid(z_i, z_f, z_o), g = tanh(z_g)
 *   c_t = f*c_{t-1} + i*g,  h_t = o*tanh(c_t)
 * d_h0, d_c0 [B,H] (NULL = zeros).  d_hiddens receives h_t at row t*B + b with
 * row stride ldh >= H floats: ldh = 2H lets a forward and a reverse call fill
 * the two halves of one [T*B, 2H] buffer (columns outside [0, H) of a row are
 * not touched).  reverse != 0 runs the frames T-1 .. 0.  d_lengths (device
 * int32 [B], NULL = all T): for frames t >= d_lengths[b] utterance b's h and c
 * are carried unchanged and its output row is zeros, i.e. pack_padded_sequence
 * / pad_packed_sequence; in reverse the utterance starts from h0 / c0 at its
 * own last frame.  d_hT, d_cT [B,H] (NULL = not wanted) receive the state
 * after each utterance's last valid frame (in reverse: after frame 0); pass
 * them as the next call's d_h0 / d_c0 to stream.  In place: d_cT may be d_c0.
 * d_hT may be d_h0 (the same pointer) for H <= 128 only; for H > 128 the
 * per-frame launch reads whole h0 rows while it stores d_hT, so d_hT == d_h0
 * is ASR_ERR_ARG there (alternate two buffers), and a d_hT that overlaps the
 * [B,H] floats of d_h0 without being equal to it is ASR_ERR_ARG for every H.
 * d_work: asr_lstm_workspace_bytes(T,B,H) bytes, 16-B aligned (the input
 * projection for all T, one GEMM that follows asr_set_dense_arith like
 * asr_linear_fwd, then the cell state); the size is 0 for an invalid shape.
 * The recurrence contracts on fp32 MFMA.  16 <= H <= 128: one launch with
 * W_hh resident in registers, 16 utterances per workgroup; 128 < H <= 2048:
 * one launch per frame (capturable in a graph; needs ldh % 4 == 0 and 16-B
 * aligned d_hiddens / d_h0).  The kernel depends on H only, so an utterance's
 * bits do not depend on its batch.
 * ASR_ERR_ARG: a NULL required pointer, a non-positive size, ldh < H;
 * ASR_ERR_UNSUPPORTED: H % 16 != 0, H > 2048, B*4H*4 bytes beyond one buffer
 * resource (0x7ff00000).  No projection (proj_size) or dropout. */
size_t asr_lstm_workspace_bytes(int T, int B, int H);
int asr_lstm_fwd(const float* d_x, const float* d_h0, const float* d_c0, const float* d_W_ih,
                 const float* d_W_hh, const float* d_b_ih, const float* d_b_hh, float* d_hiddens,
                 long ldh, float* d_hT, float* d_cT, const int32_t* d_lengths, void* d_work, int T,
                 int B, int in, int H, int reverse, asr_stream_t s);

/* The recurrence stage of asr_lstm_fwd alone (as asr_rnn_recur_fwd is to
 * asr_rnn_fwd), for callers that run the input projection themselves, e.g.
 * on another stream: d_P [T*B, 4H] holds x.W_ih (asr_linear_fwd(x, W_ih, NULL,
 * P, T*B, in, 4H, ASR_EPI_NONE)) and is read only.  asr_lstm_fwd is exactly
 * that GEMM into d_work followed by this call, bit for bit.  d_work (same
 * size) holds the cell state at its end and is needed for H > 128 only. */
int asr_lstm_recur_fwd(const float* d_P, const float* d_h0, const float* d_c0, const float* d_W_hh,
                       const float* d_b_ih, const float* d_b_hh, float* d_hiddens, long ldh,
                       float* d_hT, float* d_cT, const int32_t* d_lengths, void* d_work, int T,
                       int B, int H, int reverse, asr_stream_t s);

/* One GRU layer and direction over a whole sequence — torch.nn.GRU semantics
 * (gate order r, z, n), the recurrent layer of DeepSpeech2-style and small
 * streaming CTC acoustic models; no reference member.  x time-major
 * [T*B, in]; W_ih [in, 3H], W_hh [H, 3H] in this library's [in][out] layout,
 * gate q of hidden unit j at column q*H + j; b_ih, b_hh [3H].  With
 * P = x_t.W_ih and a = h_{t-1}.W_hh, in this operation order:
 *   r   = sigmoid((P_r + a_r) + (b_ir + b_hr))
 *   z   = sigmoid((P_z + a_z) + (b_iz + b_hz))
 *   n   = tanh((P_n + b_in) + r * (a_n + b_hn))
 *   h_t = n + z * (h_{t-1} - n)            (= (1 - z) n + z h_{t-1})
 * (the reset gate multiplies the hidden contribution of the candidate only,
 * b_hn included).  Everything else is asr_lstm_fwd's contract without the cell
 * state: d_h0 [B,H] (NULL = zeros); d_hiddens receives h_t at row t*B + b with
 * row stride ldh >= H floats (columns outside [0, H) of a row are not
 * touched, so ldh = 2H lets two calls fill the halves of one [T*B, 2H]
 * buffer); reverse != 0 runs the frames T-1 .. 0; d_lengths (device int32
 * [B], clamped to [0, T], NULL = all T): for frames t >= d_lengths[b]
 * utterance b's h is carried unchanged and its output row is zeros, in
 * reverse the utterance starts from h0 at its own last frame; d_hT [B,H]
 * (NULL = not wanted) receives the state after each utterance's last valid
 * frame, h0 for length 0 — pass it as the next call's d_h0 to stream.  In
 * place: d_hT may be d_h0 (the same pointer) for H <= 128 only; for H > 128
 * the per-frame launch reads whole h0 rows while it stores d_hT, so d_hT ==
 * d_h0 is ASR_ERR_ARG there (alternate two buffers), and a d_hT that overlaps
 * the [B,H] floats of d_h0 without being equal to it is ASR_ERR_ARG for every H.
 * d_work: asr_gru_workspace_bytes(T,B,H) bytes, 16-B aligned: the input
 * projection P [T*B, 3H] for all T, one GEMM that follows asr_set_dense_arith
 * like asr_linear_fwd; the size is 0 for an invalid shape.
 * The recurrence contracts on fp32 MFMA.  16 <= H <= 128: one launch with
 * W_hh resident in registers, 16 utterances per workgroup; 128 < H <= 2048:
 * one launch per frame (capturable in a graph; needs ldh % 4 == 0 and 16-B
 * aligned d_hiddens / d_h0).  The kernel depends on H only, so an utterance's
 * bits do not depend on its batch.  Asynchronous on s, no allocation.
 * ASR_ERR_ARG: a NULL required pointer, a non-positive size, ldh < H;
 * ASR_ERR_UNSUPPORTED: H % 16 != 0, H > 2048, B*3H*4 bytes beyond one buffer
 * resource (0x7ff00000), T*B > INT_MAX, the step form's alignment rules.
 * No projection, dropout or torch's legacy GRU variants. */
size_t asr_gru_workspace_bytes(int T, int B, int H);
int asr_gru_fwd(const float* d_x, const float* d_h0, const float* d_W_ih, const float* d_W_hh,
                const float* d_b_ih, const float* d_b_hh, float* d_hiddens, long ldh, float* d_hT,
                const int32_t* d_lengths, void* d_work, int T, int B, int in, int H, int reverse,
                asr_stream_t s);

/* The recurrence stage of asr_gru_fwd alone: d_P [T*B, 3H] holds x.W_ih
 * (asr_linear_fwd(x, W_ih, NULL, P, T*B, in, 3H, ASR_EPI_NONE)) and is read
 * only.  asr_gru_fwd is exactly that GEMM into d_work followed by this call,
 * bit for bit.  It takes no workspace: a GRU has no cell state. */
int asr_gru_recur_fwd(const float* d_P, const float* d_h0, const float* d_W_hh, const float* d_b_ih,
                      const float* d_b_hh, float* d_hiddens, long ldh, float* d_hT,
                      const int32_t* d_lengths, int T, int B, int H, int reverse, asr_stream_t s);

/* One convolution layer over time — torch.nn.Conv1d semantics in this
 * library's time-major layout, with bias and activation fused: the layer
 * between the features (asr_fbank_fwd) and the recurrence (asr_gru_fwd,
 * asr_lstm_fwd) of DeepSpeech2-style models, and the whole body of
 * wav2letter / Jasper / QuartzNet ones; no reference member.
 * Frames out for n frames in, with k = kernel, s = stride, d = dilation,
 * pl / pr = pad_left / pad_right:
 *   out_frames(n) = 0                                        if n <= 0 or n + pl + pr < d (k-1) + 1
 *                 = floor((n + pl + pr - d (k-1) - 1) / s) + 1   otherwise
 * (torch's output length); T_out = out_frames(T).
 * d_x: row t*B + b holds c_in floats, row stride ldx >= c_in.  d_out: row
 * t'*B + b receives c_out floats, row stride ldo >= c_out; columns >= c_out of
 * a row are not touched (ldo = 2 c_out lets two calls fill the halves of one
 * buffer).  d_W [k][c_in / groups][c_out] row-major, the [in][out] layout per
 * tap (depthwise: [k][C]); d_b [c_out] or NULL for zeros.
 *   out(t', b, co) = act((sum_{j<k} sum_{ci} xh(t' s - pl + j d, b, ci) W[j][ci][co]) + b[co])
 * where xh is x inside the utterance and exactly 0 outside it.  The order is
 * fixed: taps ascending, channels ascending within a tap, from a zero
 * accumulator (dense: on fp32 MFMA, channels in groups of 4 with a zero-filled
 * tail when c_in % 4 != 0; depthwise: one fmaf chain over the taps), then the
 * bias is added, then the activation: ASR_CONV_ACT_NONE, _RELU max(v, 0), or
 * _CLIP min(max(v, 0), clip) (DeepSpeech2's Hardtanh(0, 20)).  Always fp32
 * arithmetic, whatever asr_set_dense_arith says.
 * Lengths as in asr_lstm_fwd: d_lengths device int32 [B], clamped to [0, T],
 * NULL = all T.  Input frames t >= len[b] are read as zero whatever the buffer
 * holds (the kernel selects the zero, it does not multiply by a mask: padding
 * may hold NaN).  Output rows t' >= out_frames(len[b]) are all zeros;
 * d_out_lengths (device int32 [B], may be NULL, must not overlap d_lengths)
 * receives out_frames(len[b]) and can be passed unchanged as d_lengths of
 * asr_gru_fwd, asr_lstm_fwd or asr_ctc_align.  For t' below that count the
 * result is torch.nn.functional.conv1d on the utterance's own len[b] frames
 * with zero padding (pl, pr).
 * An output row's bits depend only on the values in its receptive field, the
 * weights, the bias and the descriptor: never on T, B, the row's position,
 * other utterances' lengths, ldx / ldo, pointer alignment, or whether a zero
 * came from padding, from a length or from data (the kernel is chosen by the
 * descriptor alone; 16-byte loads of aligned rows give the scalar path's
 * bits).  So a causal layer (pl = d (k-1), pr = 0) run over chunks with their
 * d (k-1) history frames prepended and pad_left = 0 gives the whole call's bits.
 * One launch, asynchronous on s, no allocation, no workspace, no host sync;
 * d_out must not overlap d_x.  Checks, in this order, all before any HIP call —
 * ASR_ERR_ARG: a NULL descriptor, d_x, d_W or d_out; non-positive T, B, c_in,
 * c_out, kernel, stride or dilation; negative padding; ldx < c_in or
 * ldo < c_out; an unknown act; ASR_CONV_ACT_CLIP with a clip that is not
 * finite or <= 0; T_out = 0.  ASR_ERR_UNSUPPORTED: groups other than 1 or
 * c_in == c_out == groups; kernel > 128; stride or dilation > 16; c_in or
 * c_out > 4096; T + pad_left + pad_right > INT_MAX - 4096; T*B or
 * T_out*B > INT_MAX; depthwise: B * ceil(T_out / 64) * ceil(C / 64) > INT_MAX
 * (one grid dimension).
 * asr_conv1d_out_frames is host only, no HIP call: out_frames(n_frames), or
 * minus the status asr_conv1d_fwd would refuse the descriptor with (< 0). */
enum { ASR_CONV_ACT_NONE = 0, ASR_CONV_ACT_RELU = 1, ASR_CONV_ACT_CLIP = 2 };
typedef struct asr_conv1d_desc {
    int c_in, c_out;          /* channels; rows of x have c_in floats, rows of out c_out */
    int kernel;               /* k taps, 1 .. 128 */
    int stride, dilation;     /* s, d: 1 .. 16 each */
    int pad_left, pad_right;  /* zero frames before frame 0 / after the last frame, >= 0
                                 (causal: pad_left = d (k-1), pad_right = 0) */
    int groups;               /* 1 (dense) or c_in == c_out == groups (depthwise) */
    int act;                  /* ASR_CONV_ACT_* */
    float clip;               /* ASR_CONV_ACT_CLIP: min(max(v, 0), clip), clip > 0 */
} asr_conv1d_desc;
int asr_conv1d_out_frames(const asr_conv1d_desc* d, int n_frames);
int asr_conv1d_fwd(const asr_conv1d_desc* d, const float* d_x, long ldx, const int32_t* d_lengths,
                   const float* d_W, const float* d_b, float* d_out, long ldo,
                   int32_t* d_out_lengths, int T, int B, asr_stream_t s);

/* One convolution layer over the (time, frequency) plane — torch.nn.Conv2d
 * semantics on an input [B][C][T][F], in this library's time-major layout,
 * with bias and activation fused: the layers of the Conv2dSubsampling module
 * that ESPnet, WeNet, NeMo and icefall encoders begin with; no reference
 * member.  The frequency axis lives inside the row, channels innermost:
 * d_x: row t*B + b holds F * c_in floats (F = feat_in), element (f, ci) at
 * f*c_in + ci, row stride ldx >= F * c_in.  d_out: row t'*B + b receives
 * F_out * c_out floats, element (f', co) at f'*c_out + co, row stride
 * ldo >= F_out * c_out; columns past that of a row are not touched.  So a
 * log-mel matrix from asr_fbank_fwd is the c_in = 1 input as it stands, and an
 * output is the next layer's input, or asr_linear_fwd's, as it stands.
 * d_W [kernel_t][kernel_f][c_in / groups][c_out] row-major (depthwise:
 * [kernel_t][kernel_f][C]); d_b [c_out] or NULL for zeros.
 * Counts, with k, s, lo, hi the kernel, stride and pads of an axis (dilation 1):
 *   count(n) = 0                                   if n <= 0 or n + lo + hi < k
 *            = floor((n + lo + hi - k) / s) + 1    otherwise
 * (torch's output size, asr_conv1d_out_frames' formula); out_frames(n) is
 * count(n) on the time axis, T_out = out_frames(T), F_out = out_feats() =
 * count(feat_in) on the frequency axis.  For an unpadded k 3 / s 2 layer
 * out_frames(n) is the number of entries the toolkits' mask[:, :, :-2:2] keeps.
 *   out(t', b, f', co) = act((sum_{jt} sum_{jf} sum_{ci}
 *       xh(t' s_t - pad_t_lo + jt, b, f' s_f - pad_f_lo + jf, ci) W[jt][jf][ci][co]) + b[co])
 * where xh is x inside the utterance's [0, len[b]) x [0, F) and exactly 0
 * outside it.  The zero is selected where x is fetched, never multiplied in:
 * frames t >= len[b] of x (and columns >= F * c_in of a row) may hold NaN.
 * The order of every output element is fixed: from a zero accumulator, jt
 * ascending; within jt the run of kernel_f * c_in consecutive input floats that
 * starts at column (f' s_f - pad_f_lo) * c_in ascending (jf-major, ci-minor) —
 * dense: on fp32 MFMA in groups of 4 counted from the run's start, with a
 * zero-filled tail, groups wholly past the run not issued; depthwise: one
 * fmaf chain, jt ascending, jf ascending — then the bias is added, then the
 * activation (ASR_CONV_ACT_*, as asr_conv1d_fwd).  Always fp32 arithmetic,
 * whatever asr_set_dense_arith says.  Nothing else enters an element's bits:
 * not T, B, the row's position, other utterances, ldx / ldo, pointer
 * alignment (16-byte loads of aligned rows with c_in % 4 == 0 give the scalar
 * path's bits), or whether a zero came from padding, a length or data.  So
 * with feat_in = 1, kernel_f = 1 and no frequency padding the result is
 * asr_conv1d_fwd's bit for bit, and a layer with pad_t_lo = kernel_t - 1,
 * pad_t_hi = 0 run over chunks with their kernel_t - 1 history frames
 * prepended and pad_t_lo = 0 gives the whole call's bits.
 * Lengths as in asr_conv1d_fwd: d_lengths device int32 [B], clamped to [0, T],
 * NULL = all T.  Output rows t' >= out_frames(len[b]) are all zeros;
 * d_out_lengths (device int32 [B], may be NULL, must not overlap d_lengths)
 * receives out_frames(len[b]) and can be passed unchanged as d_lengths of the
 * next layer.  For t' below that count the result is
 * torch.nn.functional.conv2d on the utterance's own len[b] frames, alone, with
 * zero padding.
 * One launch, asynchronous on s, no allocation, no workspace, no host sync;
 * d_out must not overlap d_x.  Checks, in this order, all before any HIP call —
 * ASR_ERR_ARG: a NULL descriptor, d_x, d_W or d_out; non-positive c_in, c_out,
 * feat_in, kernel_t, kernel_f, stride_t or stride_f; a negative pad; an unknown
 * act; ASR_CONV_ACT_CLIP with a clip that is not finite or <= 0; F_out = 0
 * (feat_in + pad_f_lo + pad_f_hi < kernel_f); non-positive T or B;
 * ldx < feat_in * c_in or ldo < F_out * c_out; T_out = 0.
 * ASR_ERR_UNSUPPORTED: groups other than 1 or c_in == c_out == groups;
 * kernel_t or kernel_f > 16; stride_t or stride_f > 16; c_in, c_out or
 * feat_in > 4096; pad_f_lo or pad_f_hi > 4096; T + pad_t_lo + pad_t_hi >
 * INT_MAX - 4096; T*B or T_out*B > INT_MAX; T_out*B*F_out > INT_MAX - 128 (the
 * flat output rows; with these limits every grid dimension fits: at most
 * 2^26 x 64 workgroups).
 * asr_conv2d_out_frames and asr_conv2d_out_feats are host only, no HIP call:
 * the count, or minus the status asr_conv2d_fwd would refuse the descriptor
 * with (< 0; asr_conv2d_out_feats is therefore never 0). */
typedef struct asr_conv2d_desc {
    int c_in, c_out;              /* channels, 1 .. 4096 each */
    int feat_in;                  /* F: frequency bins of the input, 1 .. 4096 */
    int kernel_t, kernel_f;       /* 1 .. 16 each */
    int stride_t, stride_f;       /* 1 .. 16 each */
    int pad_t_lo, pad_t_hi;       /* zero frames before / after the utterance, >= 0
                                     (causal: pad_t_lo = kernel_t - 1, pad_t_hi = 0) */
    int pad_f_lo, pad_f_hi;       /* zero bins below / above, 0 .. 4096 each */
    int groups;                   /* 1, or c_in == c_out == groups (depthwise) */
    int act;                      /* ASR_CONV_ACT_* */
    float clip;                   /* ASR_CONV_ACT_CLIP: min(max(v, 0), clip), clip > 0 */
} asr_conv2d_desc;
int asr_conv2d_out_frames(const asr_conv2d_desc* d, int n_frames);
int asr_conv2d_out_feats(const asr_conv2d_desc* d);
int asr_conv2d_fwd(const asr_conv2d_desc* d, const float* d_x, long ldx, const int32_t* d_lengths,
                   const float* d_W, const float* d_b, float* d_out, long ldo,
                   int32_t* d_out_lengths, int T, int B, asr_stream_t s);

/* The middle of a Conformer convolution module in one launch: GLU -> depthwise
 * convolution over time -> bias (an eval-mode BatchNorm folded into w and b) ->
 * activation.  The two pointwise convolutions around it are asr_linear_fwd; no
 * reference member.
 * d_u: row t*B + b holds >= 2C floats, row stride ldu >= 2C: columns [0, C) the
 * values, [C, 2C) the gates (torch's GLU over the channels of the first
 * pointwise convolution's output); other columns are not read.  d_w [kernel][C]
 * row-major, d_b [C] or NULL for zeros.  d_out: row t*B + b receives C floats,
 * row stride ldo >= C, columns >= C of a row are not touched.
 *   g(t, b, c)   = u[t, b, c] / (1 + exp(-u[t, b, C + c]))  for 0 <= t < len[b], exactly 0 outside
 *   out(t, b, c) = act((sum_{j<k} g(t - pl + j, b, c) w[j][c]) + b[c])
 * Stride 1, dilation 1, pad_left + pad_right = kernel - 1, so T_out = T: "same"
 * is ((k-1)/2, k-1 - (k-1)/2), causal (k-1, 0).  One fmaf chain per element
 * from 0, taps ascending, then the bias, then the activation:
 * ASR_GLU_ACT_NONE, _RELU max(v, 0) or _SILU v / (1 + exp(-v)).  The sigmoid is
 * evaluated once per input element.  fp32 always.
 * d_lengths device int32 [B], clamped to [0, T], NULL = all T.  Frames
 * t >= len[b] of u are never read (the zero is selected, not multiplied: they
 * may hold NaN) and rows t >= len[b] of out are zeros.  A gate of -100 gives 0,
 * one of +100 the value: nothing overflows to NaN.
 * An output row's bits depend only on the values in its receptive field, the
 * weights, the bias and the descriptor: never on T, B, the row's position,
 * other utterances, ldu / ldo or pointer alignment.  So a causal module run
 * over chunks with their k - 1 history frames prepended (and the first k - 1
 * output rows of each later chunk dropped) gives the whole call's bits.
 * One launch, asynchronous on s, no allocation, no workspace, no host sync.
 * Checks, in this order, all before any HIP call — ASR_ERR_ARG: a NULL
 * descriptor, d_u, d_w or d_out; non-positive T, B, channels or kernel; a
 * negative pad; ldu < 2C or ldo < C; an unknown act; d_out == d_u.
 * ASR_ERR_UNSUPPORTED: pad_left + pad_right != kernel - 1; kernel >
 * ASR_GLU_DWCONV_MAX_KERNEL; T*B > INT_MAX or T > INT_MAX - 4096;
 * B * ceil(T / 64) * ceil(C / 64) > INT_MAX (one grid dimension).
 * Not built: stride or dilation other than 1, GroupNorm / LayerNorm in place of
 * the BatchNorm, a split-bf16 variant. */
#define ASR_GLU_DWCONV_MAX_KERNEL 80
enum { ASR_GLU_ACT_NONE = 0, ASR_GLU_ACT_RELU = 1, ASR_GLU_ACT_SILU = 2 };
typedef struct asr_glu_dwconv_desc {
    int channels;             /* C: u rows have 2C floats, out rows C */
    int kernel;               /* k taps, 1 .. ASR_GLU_DWCONV_MAX_KERNEL */
    int pad_left, pad_right;  /* >= 0, pad_left + pad_right == kernel - 1 */
    int act;                  /* ASR_GLU_ACT_* */
} asr_glu_dwconv_desc;
int asr_glu_dwconv_fwd(const asr_glu_dwconv_desc* d, const float* d_u, long ldu, const int32_t* d_lengths,
                       const float* d_w, const float* d_b, float* d_out, long ldo, int T, int B,
                       asr_stream_t s);

/* Scaled dot-product self-attention over time, all heads in one launch —
 * softmax(Q K^T * scale) V per head with per-utterance lengths and an optional
 * chunked window: the hot path of torch.nn.MultiheadAttention in Transformer /
 * Conformer CTC encoders (the projections are asr_linear_fwd, the residual
 * asr_matadd, the norm asr_layernorm_fwd); no reference member.  No workspace:
 * the score matrix is never materialised (online softmax over key blocks).
 * Layout, time-major as everywhere: row i*B + b of d_q holds heads*head_dim
 * floats, row stride ldq, head h at columns [h*head_dim, (h+1)*head_dim); d_k
 * and d_v have Tk frames (strides ldk, ldv), d_out has Tq frames (stride ldo);
 * columns >= heads*head_dim of a row of d_out are not touched.  Q, K and V may
 * be three column ranges of one [T*B, 3E] projection buffer (ld = 3E, pointers
 * offset by E).  d_out must not overlap Q, K or V.
 * Positions and mask: query row i stands at absolute frame p = q_pos0 + i, key
 * row j at r = k_pos0 + j (a plain call: both 0, Tq == Tk).  Key r exists for
 * utterance b iff 0 <= j < Tk and r < len[b]; d_lengths is device int32 [B] in
 * ABSOLUTE frames, negative values clamp to 0, NULL = no bound.  Query p sees
 * key r iff the key exists and
 *   p / chunk - left <= r / chunk <= p / chunk + right      (integer division),
 * a -1 dropping that side: left = right = -1 is full attention, chunk = 1 with
 * right = 0 is causal.  Query rows with p >= len[b], and rows that see no key,
 * are exact zeros (the zero-past-length convention of asr_lstm_fwd and
 * asr_conv1d_fwd).  K and V of keys that do not exist are selected as zero
 * where they are fetched, never multiplied by a mask: padding rows of K and V,
 * and Q rows past the length, may hold NaN.
 * Arithmetic: Q K^T and P V on v_mfma_f32_16x16x4_f32, the softmax in fp32 with
 * a running maximum (online softmax).  Always fp32, whatever
 * asr_set_dense_arith says.  scale = 0 means 1 / sqrt(head_dim).
 * Block grid: keys are walked in ascending blocks of ASR_ATTN_KEY_BLOCK frames
 * aligned on absolute positions (block n = frames [64 n, 64 n + 64)); a block
 * in which a query sees nothing leaves that query's state bit-unchanged.  So an
 * output row's bits depend only on its own query, the keys and values it sees
 * at their absolute positions, and the descriptor: never on Tq, Tk, B, the
 * row's position in the buffer, q_pos0, k_pos0, other utterances, strides or
 * pointer alignment (16-byte loads of aligned rows give the scalar path's
 * bits).  A streaming caller that keeps a K/V cache of the last left*chunk
 * frames and calls chunk by chunk (q_pos0 = first frame of the chunk, k_pos0 =
 * first cached frame) gets the whole call's bits.
 * One launch, asynchronous on s, no allocation, no host sync.  Checks, in this
 * order, all before any HIP call — ASR_ERR_ARG: a NULL descriptor, d_q, d_k,
 * d_v or d_out; non-positive Tq, Tk, B, heads, head_dim or chunk; left or
 * right < -1; negative q_pos0 or k_pos0; a stride below heads*head_dim; a scale
 * that is not finite or < 0.  ASR_ERR_UNSUPPORTED: head_dim % 4 != 0 or > 128;
 * heads*head_dim > 4096; heads or B > 65535 (grid dimensions); q_pos0 + Tq or
 * k_pos0 + Tk > INT_MAX - 64; Tq*B or Tk*B > INT_MAX.
 * Not built: relative-position or rotary terms and additive score biases;
 * the attention probabilities as an output; a split-bf16 variant; training.
 * (Cross-attention with different batch sizes is asr_cross_attention_fwd.) */
#define ASR_ATTN_KEY_BLOCK 64
typedef struct asr_attn_desc {
    int heads, head_dim;   /* head_dim % 4 == 0, 4 .. 128; heads*head_dim <= 4096 */
    float scale;           /* 0 = 1/sqrt(head_dim); else finite, > 0 */
    int chunk;             /* >= 1: mask granularity in frames (1 = per frame) */
    int left, right;       /* chunks visible before / after the query's own; -1 = unlimited;
                              right = 0 with chunk = 1: causal */
} asr_attn_desc;
int asr_attention_fwd(const asr_attn_desc* d, const float* d_q, long ldq, const float* d_k, long ldk,
                      const float* d_v, long ldv, const int32_t* d_lengths, float* d_out, long ldo,
                      int Tq, int q_pos0, int Tk, int k_pos0, int B, asr_stream_t s);

/* Grouped cross-attention, the hot path of attention-decoder rescoring (WeNet's
 * attention_rescoring, ESPnet's joint CTC / attention scoring): N = sum n_b
 * hypotheses attend to the memories of B utterances, hypothesis n to its own
 * utterance's only; no reference member.  The memory is not repeated per
 * hypothesis: the kernel takes the map from utterance to hypotheses instead,
 * d_hyp_offsets device int32 [B + 1], hypotheses off[b] .. off[b+1] - 1 belong
 * to utterance b (so the hypotheses are ordered by utterance).
 * Layout: row u*N + n of d_q and d_out is token u of hypothesis n (time-major
 * with the hypotheses as the batch, as asr_attention_fwd lays out a causal
 * self-attention over them), row j*B + b of d_k and d_v is frame j of utterance
 * b; heads*head_dim floats per row, head h at columns [h*head_dim,
 * (h+1)*head_dim), row strides ldq, ldk, ldv, ldo; columns >= heads*head_dim of
 * a row of d_out are not touched.  K and V may be two column ranges of one
 * [T*B, 2E] projection buffer.  d_out must not overlap Q, K or V.
 *   out(u, n, h, :) = sum_j softmax_j(scale * q(u,n,h).k(j,b,h)) v(j,b,h)
 * over j < klen[b], b the utterance of n.  No window: cross-attention is full.
 * d_q_lengths device int32 [N] (tokens per hypothesis, clamped to [0, U], NULL =
 * U), d_k_lengths device int32 [B] (frames per utterance, clamped to [0, T],
 * NULL = T).  A row is exactly zero when u >= qlen[n] and when klen[b] = 0.  K
 * and V past the length and Q past the length may hold NaN: zeros are selected
 * there, never multiplied.  scale = 0 means 1 / sqrt(head_dim).
 * Grid (ceil(U * max_hyps / 64), heads, B): max_hyps bounds off[b+1] - off[b]
 * and only sizes the grid.  The queries of utterance b are numbered
 * token-major, flat query f = u * cnt_b + j being token u of its j-th
 * hypothesis; workgroup x owns f in [64 x, 64 x + 64), a wave 16 of them, a
 * lane one, and workgroups with 64 x >= U * cnt_b exit at once.  The hypotheses
 * of an utterance so share query tiles and every K / V block a tile stages.
 * The kernel clamps what it reads from d_hyp_offsets: cnt_b into [0, max_hyps],
 * the first hypothesis into [0, N - cnt_b].  A wrong map gives wrong numbers,
 * never an access outside the buffers.  Rows of hypotheses that no utterance
 * covers (after the clamps) are NOT written.
 * Arithmetic: asr_attention_fwd's, unchanged (64-key blocks from frame 0
 * ascending, both products on v_mfma_f32_16x16x4_f32, online softmax in fp32).
 * A row's bits depend only on its query, its utterance's keys and values and
 * the descriptor: never on which hypotheses share its tile, on N, B, U, T,
 * max_hyps, strides or pointer alignment; they equal asr_attention_fwd's bits
 * for that hypothesis alone (B = 1, Tq = qlen, Tk = klen, no window).
 * One launch, asynchronous on s, no allocation, no workspace, no host sync.
 * Checks, in this order, all before any HIP call — ASR_ERR_ARG: a NULL
 * descriptor, d_q, d_k, d_v, d_out or d_hyp_offsets; non-positive U, N, T, B,
 * heads or head_dim; max_hyps outside [1, N]; a stride below heads*head_dim; a
 * scale that is not finite or < 0.  ASR_ERR_UNSUPPORTED: head_dim % 4 != 0 or
 * > 128; heads*head_dim > 4096; heads or B > 65535 (grid dimensions); U*N or
 * T*B > INT_MAX; U*max_hyps > INT_MAX - 64.
 * (Autoregressive decoding with a K/V cache is asr_decode_attention_fwd below.)
 * Not built: a right-to-left decoder (reverse_weight); a compaction of dead
 * query lanes (a lane past qlen[n] stays in its tile); GELU in the decoder's
 * feed-forward. */
typedef struct asr_xattn_desc {
    int heads, head_dim;   /* limits of asr_attn_desc */
    float scale;           /* 0 = 1/sqrt(head_dim); else finite, > 0 */
} asr_xattn_desc;
int asr_cross_attention_fwd(const asr_xattn_desc* d, const float* d_q, long ldq, const float* d_k, long ldk,
                            const float* d_v, long ldv, const int32_t* d_q_lengths, const int32_t* d_k_lengths,
                            const int32_t* d_hyp_offsets, int max_hyps, float* d_out, long ldo, int U, int N,
                            int T, int B, asr_stream_t s);

/* The teacher-forced score of N hypotheses from a log-softmax buffer that stays
 * on the device:  d_scores[n] = sum over u < len[n] of
 * d_logp[(u*N + n)*ld + d_tokens[u*N + n]], in fp64, tokens in ascending u (one
 * thread per hypothesis, so the sum's order is fixed).  d_logp [U*N, V] fp32 with
 * row stride ld >= V, d_tokens device int32 [U*N], d_lengths device int32 [N]
 * clamped to [0, U] (NULL = U), d_scores device fp64 [N].  A token outside
 * [0, V) contributes -inf and nothing is read for it; len[n] = 0 gives 0.
 * One launch, asynchronous on s.  Checks, in this order, before any HIP call —
 * ASR_ERR_ARG: NULL d_logp, d_tokens or d_scores; non-positive U, N or V;
 * ld < V.  ASR_ERR_UNSUPPORTED: U*N > INT_MAX. */
int asr_token_score(const float* d_logp, long ld, const int32_t* d_tokens, const int32_t* d_lengths,
                    double* d_scores, int U, int N, int V, asr_stream_t s);

/* Attention over a K/V cache with ONE query per hypothesis: the attention of an
 * autoregressive decoder step (attention-decoder beam search: WeNet's and
 * ESPnet's `attention` decode mode); no reference member.  Hypothesis n of N
 * attends to keys j < len[n]:
 *   out(n, h, :) = sum_j softmax_j(scale * q(n,h).k(j, col(j,n), h)) v(j, col(j,n), h)
 * Layout: d_q and d_out have N rows of heads*head_dim floats (row strides ldq,
 * ldo; head h at columns [h*head_dim, (h+1)*head_dim)); d_k and d_v are
 * time-major [Tk*S, >= E], key j of column c being row j*S + c, as everywhere in
 * this library.  d_cols device int32 with row stride ldc: col(j, n) =
 * d_cols[j*ldc + n].  ldc = 0: one column d_cols[n] for every j; that is
 * cross-attention, col the hypothesis's utterance, S = B, Tk = T.  ldc >= N:
 * self-attention over the cache of a beam search, the table being the ancestry
 * (which slot wrote this hypothesis's key at step j), Tk rows of it; a beam
 * reorder permutes that small table and never moves K / V.  d_lengths device
 * int32 [N] clamped to [0, Tk], NULL = Tk.
 * A row with len 0 is exact zeros.  K / V rows that no live (j, n) names may
 * hold NaN: they are never read.  Columns >= heads*head_dim of a row of d_out
 * are not touched.  K and V may be column ranges of one buffer.  scale = 0 means
 * 1 / sqrt(head_dim).  d_out must not overlap Q, K or V.
 * The kernel clamps every col into [0, S - 1]: a wrong table gives wrong numbers
 * and never an access outside the buffers.
 * Arithmetic: fp32, online softmax over 64-key blocks from key 0 ascending, a
 * lane per key for q.k (one fmaf per dimension, ascending), a lane per four
 * output dimensions and half block for p.v; no MFMA: the work is one query
 * against a few hundred keys, bound by latency and bandwidth.  Grid (N, heads),
 * one 64-lane workgroup per (hypothesis, head).  A row's bits depend only on its
 * query, the keys and values it sees in order and the descriptor: never on N, S,
 * the row's slot, other hypotheses, ldc, the column numbers, strides or pointer
 * alignment.  They are NOT asr_attention_fwd's bits (another product order).
 * One launch, asynchronous on s, no allocation, no workspace, no host sync.
 * Checks, in this order, all before any HIP call — ASR_ERR_ARG: a NULL
 * descriptor, d_q, d_k, d_v, d_out or d_cols; non-positive N, Tk, S, heads or
 * head_dim; ldc outside {0} and [N, inf); a stride below heads*head_dim; a scale
 * that is not finite or < 0.  ASR_ERR_UNSUPPORTED: head_dim % 4 != 0 or > 128;
 * heads*head_dim > 4096; heads > 65535; Tk*S > INT_MAX.
 * Measured: through an ancestry table the call takes 0.31
 * to 0.39 of a physical gather of the cache followed by asr_attention_fwd; with
 * ldc = 0 it takes 2.4 to 5 times asr_cross_attention_fwd at U = 1, which stages
 * an utterance's K / V once for all of its hypotheses, so a decoder step's
 * cross-attention should call that.
 * Not built: several queries per hypothesis (speculative or chunked decoding);
 * K / V staged once in LDS for the hypotheses of one utterance. */
int asr_decode_attention_fwd(const asr_xattn_desc* d, const float* d_q, long ldq, const float* d_k, long ldk,
                             const float* d_v, long ldv, const int32_t* d_cols, long ldc, const int32_t* d_lengths,
                             float* d_out, long ldo, int N, int Tk, int S, asr_stream_t s);

/* Embedding gather on the device:
 *   d_out[r][e] = fp32( (double)d_emb[tok[r]][e] * scale + d_pe[pos[r]][e] ),  r < R, e < E,
 * the product and the sum two separately rounded fp64 operations (no FMA), so
 * the result equals a float64 host gather rounded once.  d_emb fp32 [V, E] (row
 * stride lde), d_pe fp64 [P, E] (row stride ldp; NULL = 0, and d_pos, ldp and P
 * are then ignored), d_tokens and d_pos device int32 [R], d_out fp32 [R, >= E]
 * (row stride ldo).  A token outside [0, V) or a position outside [0, P) gives a
 * zero row and nothing is read for it.  One launch, asynchronous on s.
 * Checks, in this order, before any HIP call — ASR_ERR_ARG: NULL d_emb, d_tokens
 * or d_out, or d_pe without d_pos; non-positive R, E, V (P with d_pe); lde, ldo
 * (ldp with d_pe) below E; a scale that is not finite.  ASR_ERR_UNSUPPORTED:
 * R*E > INT_MAX. */
int asr_embed_fwd(const float* d_emb, long lde, const double* d_pe, long ldp, const int32_t* d_tokens,
                  const int32_t* d_pos, double scale, float* d_out, long ldo, int R, int E, int V, int P,
                  asr_stream_t s);

/* One prune of an attention-decoder beam search.  B utterances have K slots
 * each, slot n = b*K + k, N = B*K.  d_logp fp32 [N, V] (row stride ld) are the
 * decoder's log-probs of this step, d_scores fp64 [N] the hypotheses' scores
 * (-inf: an empty slot; at step 0 only slot k = 0 of each utterance is live),
 * d_finished int32 [N], and d_tokens_in / d_anc_in the int32 history tables
 * [max_len][N]: the token chosen at step j, and the slot that wrote the
 * hypothesis's self-attention key at step j (asr_decode_attention_fwd's d_cols).
 * Candidates: a live, unfinished slot gives V of them, token v scoring
 * score + (double)logp[v] (one that comes out -inf or NaN is dropped); a
 * finished slot exactly one, itself, score unchanged, token eos (WeNet's masking
 * of ended hypotheses); an empty slot none.  Kept: the exact top K per
 * utterance, by score descending, ties by parent slot ascending, then by token
 * ascending; slot k of the utterance gets the k-th.  Remaining slots are empty:
 * score -inf, finished 0, parent the slot itself, token eos.
 * Outputs: d_scores_out, d_finished_out (the parent's flag, or token == eos),
 * d_parent [N] (a slot of the same utterance), d_token [N]; the tables through
 * parent, tokens_out[j][n] = tokens_in[j][parent[n]] for j < step,
 * tokens_out[step][n] = token[n], anc_out[j][n] = anc_in[j][parent[n]] for
 * j <= step, anc_out[step + 1][n] = n when step + 1 < max_len (later rows are
 * not touched; the out tables must not be the in tables); d_all_finished, one
 * int32: the number of live unfinished slots after the prune (0: the search is
 * over).  asr_attn_beam_step: device pointers, one kernel launch (one workgroup
 * per utterance; K rounds, each taking the best candidate after the last) behind
 * a 4-byte memset, asynchronous on s, no host sync.  asr_attn_beam_step_host:
 * the same rule on host pointers (a partial sort), the CPU path; the two agree
 * exactly.
 * Checks, in this order, before any HIP call — ASR_ERR_ARG: a NULL pointer; B or
 * V or max_len <= 0; K outside [1, ASR_ATTN_BEAM_MAX_K]; step outside
 * [0, max_len); eos outside [0, V); ld < V; an out table that is its in table.
 * ASR_ERR_UNSUPPORTED: B*K*max_len > INT_MAX.
 * Not built: joint CTC / attention decoding with a CTC prefix scorer; length
 * penalties. */
#define ASR_ATTN_BEAM_MAX_K 16
typedef struct asr_attn_beam_desc {
    int B, K, V;           /* utterances, slots per utterance, vocabulary */
    int max_len;           /* rows of the history tables */
    int step;              /* this prune's step, 0 .. max_len - 1 */
    int eos;
} asr_attn_beam_desc;
int asr_attn_beam_step(const asr_attn_beam_desc* d, const float* d_logp, long ld, const double* d_scores,
                       const int32_t* d_finished, const int32_t* d_tokens_in, const int32_t* d_anc_in,
                       double* d_scores_out, int32_t* d_finished_out, int32_t* d_parent, int32_t* d_token,
                       int32_t* d_tokens_out, int32_t* d_anc_out, int32_t* d_all_finished, asr_stream_t s);
int asr_attn_beam_step_host(const asr_attn_beam_desc* d, const float* logp, long ld, const double* scores,
                            const int32_t* finished, const int32_t* tokens_in, const int32_t* anc_in,
                            double* scores_out, int32_t* finished_out, int32_t* parent, int32_t* token,
                            int32_t* tokens_out, int32_t* anc_out, int32_t* all_finished);

/* LayerNorm over the N columns of each row of a time-major [T*B, N] buffer,
 * with an optional fused residual (torch.nn.LayerNorm semantics):
 *   v = x + res (x when d_res is NULL); mean = sum(v) / N;
 *   var = sum((v - mean)^2) / N   (two-pass, biased, as torch; the fp32 mean is
 *   refined once by the mean of the centred values, so a row far from zero
 *   (1000 +- 1) is centred as accurately as one around zero);
 *   out = ((v - mean) * (1 / sqrt(var + eps))) * gamma + beta,
 * d_gamma / d_beta [N], NULL = 1 / 0.  Row strides ldx, ldr, ldo >= N; columns
 * >= N of d_out are not touched.  Rows t >= len[b] are zeros whatever x holds
 * (d_lengths device int32 [B], clamped to [0, T], NULL = all rows).  d_out may
 * be exactly d_x or d_res (in place).  One wave per row; the sums are a fixed
 * tree (a lane's columns l, l + 64, ... ascending, then the butterfly over the
 * lanes, as asr_lm_score's), so a row's bits never depend on T, B or the
 * row's position.  fp32 always.  GELU is not built (asr_linear_fwd fuses ReLU
 * and Swish / SiLU; GLU is in asr_glu_dwconv_fwd: DESIGN.md section 30).
 * One launch, asynchronous on s.  Checks, in this order, before any HIP call —
 * ASR_ERR_ARG: NULL d_x or d_out; non-positive T, B or N; a stride < N; eps not
 * finite or < 0.  ASR_ERR_UNSUPPORTED: N > 4096; T*B > INT_MAX. */
int asr_layernorm_fwd(const float* d_x, long ldx, const float* d_res, long ldr, const float* d_gamma,
                      const float* d_beta, float eps, const int32_t* d_lengths, float* d_out, long ldo,
                      int T, int B, int N, asr_stream_t s);

/* Zero columns [0, N) of the rows t >= len[b] of a time-major [T*B, >= N]
 * buffer in place (row stride ldx; d_lengths device int32 [B], clamped to
 * [0, T]; NULL: nothing to do, no launch).  It gives the output of a
 * projection with a bias (asr_linear_fwd after asr_attention_fwd, or the
 * residual sum of a pre-norm Transformer layer) the zero-past-length
 * convention of the other layers; the rows may hold NaN before.  One launch,
 * asynchronous on s.  ASR_ERR_ARG: NULL d_x, non-positive T, B or N, ldx < N;
 * ASR_ERR_UNSUPPORTED: T*B > INT_MAX. */
int asr_mask_rows(float* d_x, long ldx, const int32_t* d_lengths, int T, int B, int N, asr_stream_t s);

/* ---- CTC prefix beam search: replaces CTCBeamSearch (CTCBeamSearch.h:107-150,
 *      CTCBeamSearch.cu:220-312) with the semantics of the CPU decoder
 *      CTCBeamSearch.cpp:50-187 (fixes F1-F3, fp64 log domain). ---- */
typedef struct asr_ctc asr_ctc_t;

/* Constructor CTCBeamSearch(char* vocab, int vocabSize, int beamWidth, int blankID)
 * (h:107).  codes[V] is the symbol code of each label (the vocab char as
 * unsigned char for the reference API; NULL = label id, the label-id
 * overload SURVEY a2 asks for large vocabularies).  Hypothesis order on
 * ties is code-string order, as std::string order in the reference.
 * V up to 4096 (V > 63 runs the large-vocabulary kernel, e.g. C5 V=1000);
 * beam_width + 1 + ties <= 256.  max_states bounds the beam incl. ties at the
 * cutoff (0 = automatic, >= beamWidth+1). */
int asr_ctc_create(const int32_t* codes, int V, int beam_width, int blank_id, int max_states,
                   asr_ctc_t** out);
int asr_ctc_destroy(asr_ctc_t* h);

/* CTCBeamSearch::decode(seqProb, timestep, batchSize) (cu:262): decode B
 * utterances of d_emis[T][B][V] (probabilities, or log-probabilities if
 * is_log).  Enqueues the decode and the best-path traceback on stream s; the
 * workspace is sized once and reused (the reference re-allocated per call,
 * cu:263).  Fetch results with asr_ctc_get_best / asr_ctc_get_beams.
 * Lifetime: d_emis must stay allocated and unmodified until the results of
 * this decode have been fetched (asr_ctc_get_best / asr_ctc_get_beams
 * returned), because an automatic-capacity handle re-decodes it when ties
 * at the cutoff overflow the beam (see asr_ctc_get_best).  Work the caller
 * queues that writes d_emis must be ordered after that fetch. */
int asr_ctc_decode(asr_ctc_t* h, const float* d_emis, int T, int B, int is_log, asr_stream_t s);

/* General form (ctcdecode-style batches): element
 * (t, b, v) of the emissions is d_emis[t*frame_stride + b*utt_stride + v]
 * (time-major [T][B][V]: B*V, V; batch-major [B][T][V]: V, T*V), and
 * utterance b has h_lengths[b] <= T frames (host array; NULL = T for all).
 * asr_ctc_decode(h, e, T, B, is_log, s) is this with time-major strides. */
int asr_ctc_decode_ex(asr_ctc_t* h, const float* d_emis, int T, int B, long frame_stride,
                      long utt_stride, const int32_t* h_lengths, int is_log, asr_stream_t s);

/* Segmented (streaming) decode — no reference counterpart (the reference
 * decodes whole utterances, CTCBeamSearch.cu:262-312): frames [t0, t1) of a
 * T-frame batch, the beam of every utterance carried on the device from one
 * segment to the next, so a producer can hand over emissions segment by
 * segment and the decode of a batch starts after its first T/S frames.
 * Segments come in order on one handle: t0 = 0 first (h_lengths is read
 * then), each next t0 = the previous t1, the last ends at t1 = T; then the
 * results are fetched as after asr_ctc_decode (asr_ctc_get_best ...; before
 * that, ASR_ERR_STATE).  d_emis addresses frame t0: element (t, b, v) of the
 * segment is d_emis[(t - t0)*frame_stride + b*utt_stride + v].  T, B, the
 * strides and is_log must be the same for every segment.  Results are
 * bit-identical to a whole decode of the same frames.  Runs the one-wave
 * kernel (ASR_CTC_WAVES_LIST) for V <= 63 and the large-vocabulary kernel
 * for 63 < V <= 4096 (each frame's first vocabulary tile precomputed per
 * segment); CPU semantics and timesteps off, else ASR_ERR_UNSUPPORTED;
 * ASR_ERR_STATE for a segment out of order.  Overflow
 * retry (automatic capacity): asr_ctc_get_best re-decodes the whole batch
 * from the FIRST segment's d_emis over T frames, so that pointer must then
 * address all T frames (e.g. segments of one [T][B][V] buffer); a caller
 * with a ring buffer creates the handle with an explicit max_states (an
 * overflow is then reported as ASR_ERR_BEAM_OVERFLOW).
 * asr_ctc_last_kernel_ms reports the sum of the segments' kernel times. */
int asr_ctc_decode_segment(asr_ctc_t* h, const float* d_emis, int T, int t0, int t1, int B,
                           long frame_stride, long utt_stride, const int32_t* h_lengths, int is_log,
                           asr_stream_t s);

/* Best hypothesis of each utterance (cpp:74-84: max score, first in string
 * order on ties).  Synchronises the decode stream.  h_labels[B][max_len]
 * (label ids), h_lengths[B], h_logp[B] (fp64 log-probability).
 * If an utterance had more tied survivors than max_states, the batch is
 * decoded again with a wider beam capacity (up to 256 states) before
 * returning; ASR_ERR_BEAM_OVERFLOW only if that is not enough (the result is
 * then not the reference's) or if the handle was created with an explicit
 * max_states. */
int asr_ctc_get_best(asr_ctc_t* h, int32_t* h_labels, int max_len, int32_t* h_lengths,
                     double* h_logp);

/* Full final beam of every utterance, ranked by (logp desc, string asc):
 * h_n_hyps[B], h_lengths[B][max_hyps], h_labels[B][max_hyps][max_len],
 * h_logp[B][max_hyps].  Runs a traceback over all final hypotheses. */
int asr_ctc_get_beams(asr_ctc_t* h, int max_hyps, int max_len, int32_t* h_n_hyps,
                      int32_t* h_lengths, int32_t* h_labels, double* h_logp);

/* Timesteps mode (ctcdecode's `timesteps` output, baseline/main.py:46; the
 * reference C++ decoder has none): when on, decodes also record the frame at
 * which every label of every live prefix was appended (a continuing prefix
 * keeps its frames; a new prefix is its parent's plus the current frame), at
 * 16 extra bytes per node record and slot.  Off by default; the one-wave
 * list kernel is not used while it is on.  asr_ctc_get_beams_ts returns them
 * as h_timesteps[B][max_hyps][max_len] next to the ranked labels
 * (ASR_ERR_STATE if the decode ran without timesteps).  Frames are stored in
 * 16 bits: with timesteps on, a decode of T > ASR_CTC_TS_MAX_T frames returns
 * ASR_ERR_UNSUPPORTED (nothing is enqueued). */
#define ASR_CTC_TS_MAX_T 65536
int asr_ctc_set_timesteps(asr_ctc_t* h, int on);

/* Stream for the best-path traceback and the copy of its results to host
 * memory (default NULL: the decode's own stream).  With a separate stream
 * the decode stream is free for the next batch as soon as the beam search
 * ends; asr_ctc_get_best waits for the results either way, and the next
 * decode on this handle waits for its traceback.  No reference
 * counterpart (a scheduling option). */
int asr_ctc_set_result_stream(asr_ctc_t* h, asr_stream_t s);
int asr_ctc_get_beams_ts(asr_ctc_t* h, int max_hyps, int max_len, int32_t* h_n_hyps,
                         int32_t* h_lengths, int32_t* h_labels, double* h_logp, int32_t* h_timesteps);

/* Device time of the last decode's beam-search kernel (ms, HIP events on the
 * decode stream) and its launch geometry; for roofline accounting. */
int asr_ctc_last_kernel_ms(asr_ctc_t* h, float* ms);
/* Search semantics.  ASR_CTC_SEMANTICS_CPU (default):
 * CTCBeamSearch.cpp with fixes F1-F3 — beam+1 states plus ties at the cutoff,
 * final "q"/"q$" merge after the last prune; the parity target.
 * ASR_CTC_SEMANTICS_CUDA: what CTCBeamSearch.cu computes when it works —
 * exactly min(beam, n) states per step (stable descending sort, cu:174-196;
 * ties at the cutoff resolved in a fixed slot order instead of the .cu's
 * string order), and on the last step the trailing blank is stripped before
 * the merge and the prune (cu:452-456).  Any V (the reference's char vocabs
 * have up to 256 symbols, CTCBeamSearch.h:43). */
enum { ASR_CTC_SEMANTICS_CPU = 0, ASR_CTC_SEMANTICS_CUDA = 1 };
int asr_ctc_set_semantics(asr_ctc_t* h, int semantics);

/* Tuning knobs: waves per utterance (1, 2, 4 or 8; 0 = automatic), or
 * ASR_CTC_WAVES_LIST: one wave per utterance with live-label candidate lists
 * (faster on peaked emissions, slower on flat ones).
 * get_config reports the schedule a decode will use (ASR_CTC_WAVES_LIST or 1..8). */
#define ASR_CTC_WAVES_LIST (-1)
int asr_ctc_set_waves(asr_ctc_t* h, int waves);
/* Scheduling hint: n decodes of this handle's batch size are in flight on
 * the device at once (e.g. a caller pipelining n batches on n streams;
 * default 1).  The automatic schedule is then chosen for n x B utterances
 * sharing the CUs — from two per CU on, the 4-wave kernel several
 * workgroups to a CU.  Never changes results. */
int asr_ctc_set_concurrency(asr_ctc_t* h, int n);
int asr_ctc_get_config(asr_ctc_t* h, int* max_states, int* waves, int* lds_bytes);

/* ---- CTC forced alignment and exact transcript scoring ---------------------
 * No reference member is replaced (the reference only searches): the dynamic
 * programme over the CTC lattice of a GIVEN transcript, in fp64 log domain
 * with the decoder's lse.  The extended target ext has S = 2L+1 states
 * (ext[2i] = blank, ext[2i+1] = target[i]); with lp(t, c) the log-probability
 * of label c at frame t and skip(s) = ext[s] != blank && ext[s] != ext[s-2],
 *   frame 0:  a[0] = lp(0, blank), a[1] = lp(0, ext[1]), every other state -inf
 *   forward:  a_t[s] = lse(lse(a[s], a[s-1]), a[s-2] if skip(s)) + lp(t, ext[s])
 *             score = lse(a[S-1], a[S-2]) after the last frame (a[0] for L = 0):
 *             log p(target | emissions), the CTC loss negated
 *   Viterbi:  the same with max for lse (torchaudio.functional.forced_align);
 *             ties take the smallest jump (stay, then s-1, then s-2), and the
 *             final state is S-1 unless v[S-2] > v[S-1] strictly.
 * Emissions as in asr_ctc_decode_ex: element (t, b, v) at d_emis[t*frame_stride
 * + b*utt_stride + v], probabilities (lp = log((double)p), p = 0 gives -inf) or
 * log-probabilities if is_log.  d_lengths: device int32 [B] frames per
 * utterance, clamped to [0, T], NULL = T (the convention of asr_lstm_fwd and
 * asr_fbank_fwd: d_frames passes straight through).  d_targets [N][ldt] label
 * ids, ldt >= max_target_len; d_target_lengths [N], clamped to
 * [0, max_target_len]; d_utt [N]: the utterance target n is scored against,
 * NULL = utterance n (then N <= B); an n-best list is N = B*K targets with
 * d_utt[n] = n / K.
 * Outputs, each may be NULL, at least one given:
 *   d_score [N]   forward log-likelihood;
 *   d_vscore [N]  log-probability of the best alignment;
 *   d_path [N][ldp], ldp >= T: the label emitted at each frame, blank
 *     included; frames t >= the utterance's length are -1, columns >= T are
 *     not touched;
 *   d_spans [N][ldt][2]: first frame and one past the last frame of target
 *     label i; entries L_n <= i < max_target_len are (-1, -1), entries
 *     >= max_target_len are not touched.
 * Infeasible target (fewer frames than L + adjacent repeats, every alignment
 * of probability 0, a label that is the blank or outside [0, V), d_utt[n]
 * outside [0, B)): scores -inf, path -1 over the utterance's frames, spans
 * (-1, -1); never an out-of-range read.  No frames: score 0.0 for L = 0, else
 * infeasible.
 * d_work: asr_ctc_align_workspace_bytes(T, N, max_target_len) bytes (a
 * multiple of 16, 0 for an invalid shape, at most N*T*256 bytes, N*T*64 for
 * max_target_len <= 127), needed only when a path or spans are wanted: the
 * Viterbi choices, 2 bits per state and frame.
 * One launch, one wave per target, the lattice column in registers (lane l
 * owns 1, 2, 4, 8 or 16 contiguous states by max_target_len); the traceback is
 * the tail of the same kernel.  Asynchronous on s, no allocation, no host
 * sync.  A target's results depend only on its own emissions, labels and
 * frame count: never on N, its position, max_target_len, T, or which outputs
 * were asked for.
 * ASR_ERR_ARG: a NULL d_emis / d_targets / d_target_lengths, a non-positive
 * T, B, V or N, blank outside [0, V), ldt < max_target_len, ldp < T with a
 * path wanted, no output, NULL d_work with a path or spans wanted, NULL d_utt
 * with N > B; ASR_ERR_UNSUPPORTED: max_target_len > 511 or < 0, V > 4096.
 * Both are decided before any HIP call. */
size_t asr_ctc_align_workspace_bytes(int T, int N, int max_target_len);
int asr_ctc_align(const float* d_emis, int T, int B, int V, long frame_stride, long utt_stride,
                  const int32_t* d_lengths, int is_log, int blank, const int32_t* d_targets, long ldt,
                  const int32_t* d_target_lengths, const int32_t* d_utt, int N, int max_target_len,
                  double* d_score, double* d_vscore, int32_t* d_path, long ldp, int32_t* d_spans,
                  void* d_work, asr_stream_t s);

/* ---- throughput pipeline (no reference counterpart: the reference runs one
 *      batch at a time with host syncs between calls, main.cpp:40-72,
 *      RNN.cu:9-30, CTCBeamSearch.cu:262-312) ---------------------------------
 * RNN (one layer, h0 = 0) -> Linear + log_softmax -> CTC beam search over a
 * stream of equal-shape batches.  The library owns the streams, buffers and
 * decoder handles and overlaps the production of later batches with the
 * decodes of earlier ones, placing the kernels on the CUs for the shape
 * (DESIGN.md §7a-§7c).  Weights are caller-owned device arrays in the layouts of
 * asr_rnn_fwd / asr_linear_fwd and must outlive the pipeline. */
typedef struct asr_pipeline asr_pipeline_t;
typedef struct asr_pipeline_config {
    int T, B;            /* frames and utterances per batch */
    int in, H, V;        /* feature, hidden and vocabulary (incl. blank) sizes */
    int beam, blank;     /* decoder beam width and blank id (CPU semantics) */
    int inflight;        /* decodes in flight (0 = automatic) */
    int prod_streams;    /* production streams (0 = automatic) */
    int decode_cus;      /* chip-filling batches: CUs given to decoding (0 = automatic,
                            -1 = every stream on every CU) */
    int segments;        /* T-segments per batch (0 = automatic, 1 = whole utterances): the
                            fused production hands emissions over segment by segment and
                            the decode of a batch starts after its first T / segments
                            frames (asr_ctc_decode_segment); chip-filling batches with the
                            fused production only, else 1 */
} asr_pipeline_config;
int asr_pipeline_create(const asr_pipeline_config* cfg, const float* d_W_ih, const float* d_W_hh,
                        const float* d_b_ih, const float* d_b_hh, const float* d_W_out,
                        const float* d_b_out, asr_pipeline_t** out);
/* Enqueue one batch: features d_x [T*B, in] (time-major, device; read by the
 * batch's production, so it must stay unmodified until the batch is
 * collected).  Returns once the work is queued; when the caller is as many
 * batches behind as the pipeline has buffers, the oldest batch's results are
 * fetched internally first (asr_pipeline_collect still returns them).
 * Errors: a batch whose production could not be queued is not accepted (the
 * error is returned and the pipeline is unchanged: submit it again or
 * destroy).  If the rest of an accepted batch's work (this one's decode, or
 * the previous batch's emission projection + decode in the split schedule)
 * fails to queue, the pipeline is failed from that batch on: this and every
 * later submit, and the collect of that batch and every later one, return
 * the error; earlier batches are still collected normally. */
int asr_pipeline_submit(asr_pipeline_t* p, const float* d_x);
/* Results of the oldest uncollected batch, in submission order (blocks):
 * h_labels[B][max_len], h_lengths[B], h_logp[B] as asr_ctc_get_best, and the
 * batch's beam-search kernel time (ms; may be NULL). */
int asr_pipeline_collect(asr_pipeline_t* p, int32_t* h_labels, int max_len, int32_t* h_lengths,
                         double* h_logp, float* decode_ms);
int asr_pipeline_pending(asr_pipeline_t* p, int* n_uncollected);
/* Dynamic batching: a pipeline whose submits carry cfg->B utterances each
 * and whose launches carry group * cfg->B — `group` consecutive submits are
 * copied side by side into one batch (time-major [T][group * B][in]) and go
 * through one production and one decode; asr_pipeline_collect returns each
 * submit's B rows in submission order.  Collecting a submit whose batch is
 * not complete queues that batch with zero features in the missing columns
 * (their rows are decoded and dropped).  The results are the per-submit
 * pipeline's bits (every utterance is independent).  group = 1 is
 * asr_pipeline_create.  ASR_ERR_UNSUPPORTED unless the batch of
 * group * B runs the chip-filling schedule with the fused production
 * (H <= 256, V <= 32: the production whose bits do not depend on the batch
 * shape, its input projection on the batch's production stream).  (The
 * reference decodes one batch per call: CTCBeamSearch.cu:262-312.) */
int asr_pipeline_create_coalesced(const asr_pipeline_config* cfg, int group, const float* d_W_ih,
                                  const float* d_W_hh, const float* d_b_ih, const float* d_b_hh,
                                  const float* d_W_out, const float* d_b_out, asr_pipeline_t** out);
/* group, utterances per submit, and the column (0 .. group - 1) of the
 * submit collected last inside its batch (asr_pipeline_peek_emissions then
 * returns the whole batch's [T][group * B][V] emissions). */
int asr_pipeline_get_coalesce(asr_pipeline_t* p, int* group, int* batch, int* column);
/* The schedule chosen: mode (0 CU groups for small batches, 1 chip-filling
 * batches, 2 CU groups for H > 256), decodes in flight, production streams,
 * CUs per decode group / decode partition, and the decoder's waves per
 * utterance in the last decode.  Any pointer may be NULL.
 * asr_pipeline_get_segments: T-segments per batch in use.
 * asr_pipeline_get_groups: batches whose recurrences run as one (mode 2,
 * H > 256: one per-frame step launch for G batches; a batch's production
 * then starts when its group is complete or its results are asked for). */
int asr_pipeline_get_segments(asr_pipeline_t* p, int* segments);
/* The drain schedule (T-segmented batches): the last decode segment of the
 * newest `held_batches` batches is held back; a newer batch releases the
 * oldest onto its decode stream, and when the caller drains (collects a
 * batch within `inflight` of a held one) every held segment is queued on its
 * batch's production stream behind that stream's last production, so the
 * drain's decodes also use the production CUs.  first_segment_share: the
 * first T-segment's share of T (0.5 = equal halves).  Either may be NULL. */
int asr_pipeline_get_drain(asr_pipeline_t* p, int* held_batches, double* first_segment_share);
int asr_pipeline_get_groups(asr_pipeline_t* p, int* group);
int asr_pipeline_describe(asr_pipeline_t* p, int* mode, int* inflight, int* prod_streams, int* decode_cus,
                          int* decode_waves);
/* How the pipeline produces a batch's emissions: fused = 1 when the
 * recurrence and the emission projection + log_softmax run as one kernel
 * (chip-filling batches with H % 16 == 0, V <= 32: asr_linear_fwd(x, W_ih,
 * NULL, P, ..., ASR_EPI_NONE) then asr_rnn_emit_fwd(NULL, W_hh, b_ih, b_hh,
 * W_out, b_out, P, NULL, emis, ...) gives its bits), 0 when it is
 * asr_rnn_fwd then asr_linear_fwd(..., ASR_EPI_BIAS_LOGSOFTMAX);
 * decode_cu_rows: input-projection rows run on the decode CUs; recurrence:
 * the recurrence kind the unfused production pins (ASR_RNN_RECUR_*; AUTO =
 * the process-wide choice), so a caller can reproduce the emissions bit for
 * bit.  Any pointer may be NULL. */
int asr_pipeline_get_production(asr_pipeline_t* p, int* fused, long long* decode_cu_rows, int* recurrence);
/* Streams the pipeline created and the process's HIP hardware queues
 * (GPU_MAX_HW_QUEUES as read at create; HIP's default is 4).  HIP maps the
 * UNMASKED streams round-robin onto those queues (streams that share a queue
 * serialise); a CU-masked stream gets a hardware queue of its own.  The
 * pipeline's chip-filling and CU-group schedules mask their decode and
 * production streams, so they need no GPU_MAX_HW_QUEUES setting (measured
 * at HIP's default of 4: the same frames/s as at 24);
 * only the unmasked ones (every stream with decode_cus = -1, the small-batch
 * mode's GEMM streams) are fitted to the queues (no input-projection share
 * on the decode CUs, then fewer production streams down to half the
 * decodes in flight, then both), unless the caller fixed inflight /
 * prod_streams.  asr_pipeline_get_queue_use: how many of the streams share
 * HIP's queues and how many have a queue of their own. */
int asr_pipeline_get_streams(asr_pipeline_t* p, int* streams, int* hw_queues);
int asr_pipeline_get_queue_use(asr_pipeline_t* p, int* shared_queue_streams, int* dedicated_queue_streams);
/* Where the pipeline's streams run: for each stream it created, its role
 * (ASR_PIPE_ROLE_*) and the CU range [cu_lo, cu_hi) of its CU mask
 * (hipExtStreamCreateWithCUMask bits; [0, ncu) = unmasked).  *n = streams
 * created; the first min(cap, *n) entries are written. */
enum { ASR_PIPE_ROLE_DECODE = 0, ASR_PIPE_ROLE_PRODUCTION = 1, ASR_PIPE_ROLE_DECODE_CU_GEMM = 2,
       ASR_PIPE_ROLE_GEMM = 3 };
#define ASR_MAX_XCC 16
int asr_pipeline_get_placement(asr_pipeline_t* p, int cap, int* n, int* role, int* cu_lo, int* cu_hi);
/* Diagnostic: the physical CUs the first stream of `role` reaches, counted per
 * XCD (cus_per_xcc[ASR_MAX_XCC], *n_xcc = XCDs seen): one probe launch of
 * 8192 short workgroups on that stream that read HW_REG_XCC_ID / HW_REG_HW_ID
 * (synchronises the stream).  Workgroups are dealt round-robin over the XCDs
 * whatever the mask, so a role runs evenly only when its mask holds the same
 * number of CUs in every XCD (mask bit i lands on XCD i % 8; an XCD the mask
 * leaves out gets all of its CUs); DESIGN.md §10c. */
int asr_pipeline_probe_placement(asr_pipeline_t* p, int role, int* cus_per_xcc, int* n_xcc);
/* The emissions [T][B][V] (log-probabilities, device) that the decode of the
 * batch last returned by asr_pipeline_collect consumed — the exact bytes, for
 * parity checks of the pipelined path.  Valid until the next submit that
 * reuses the buffer; ASR_ERR_STATE if nothing was collected yet or the
 * buffer has been reused. */
int asr_pipeline_peek_emissions(asr_pipeline_t* p, const float** d_emis);
/* Timeline (measurement): with timing on, every batch submitted from now on
 * records four timing events — its production's start and end on the
 * production stream(s) and its decode's start (the first decode kernel
 * queued behind its emissions) and end on its decode stream — read back when
 * the batch is collected, as ms after the moment of this call.  Call it on
 * a drained pipeline (it synchronises the device); it clears the timeline.
 * A decode's "start" is when its stream reached it, which may be before
 * its workgroups get CUs.  asr_pipeline_get_timeline: *n = batches recorded;
 * the first min(cap, *n) as batch[i] and t[i][4] = (production start,
 * production end, decode start, decode end). */
int asr_pipeline_set_timing(asr_pipeline_t* p, int on);
int asr_pipeline_get_timeline(asr_pipeline_t* p, int cap, int* n, long long* batch, float* t);
int asr_pipeline_destroy(asr_pipeline_t* p);

/* ---- audio front end: waveform -> log-mel / MFCC features -----------------
 * No reference member is replaced: the reference has no feature extraction
 * (baseline/main.py:39 feeds torch.rand in place of the 26 MFCCs with a
 * +-n_context window that baseline/model.py:23 is sized for).  One handle per
 * configuration; its tables (window, twiddles, mel weights, DCT) are computed
 * on the host in double, rounded once to fp32 and uploaded at create.
 *
 * Framing: an utterance of n samples has n < win_length ? 0 :
 * 1 + (n - win_length) / hop_length frames, no centring, no padding; frame t
 * is samples [t*hop, t*hop + win) of the pre-emphasised signal
 * (y[i] = x[i] - preemph * x[i-1] over the whole utterance, x[-1] = 0) times
 * the window, zero-padded at the end to n_fft (unlike torch.stft, which for
 * win < n_fft centres the window inside n_fft samples).
 * Power: P[k] = re^2 + im^2, k = 0 .. n_fft/2, no 1/N scaling.
 * Mel: mel(f) = 2595 log10(1 + f/700); n_mels + 2 points equally spaced in
 * mel from f_min to f_max, back in Hz; filter m has corners (lo, c, hi) =
 * points m, m+1, m+2 and weight max(0, min((f_k - lo)/(c - lo),
 * (hi - f_k)/(hi - c))) at f_k = k * sample_rate / n_fft, no area
 * normalisation; e[m] = ln(max(sum_k w[m][k] P[k], log_floor)).
 * n_mfcc > 0: c_k = s_k sum_m e[m] cos(pi k (2m+1) / (2 n_mels)), s_0 =
 * sqrt(1/n_mels), s_k = sqrt(2/n_mels) (orthonormal DCT-II, no liftering).
 * Context: output row t is base frames t-C .. t+C, D floats each, zeros for
 * a frame outside [0, frames_b); rows t >= frames_b are all zeros (the
 * padding asr_lstm_fwd writes and asr_ctc_decode_ex skips). */
typedef enum asr_fbank_window {
    ASR_FBANK_WIN_HANN = 0,     /* symmetric: 0.5 - 0.5 cos(2 pi n / (win - 1)) */
    ASR_FBANK_WIN_HAMMING = 1,  /* 0.54 - 0.46 cos(2 pi n / (win - 1))          */
    ASR_FBANK_WIN_RECT = 2
} asr_fbank_window;

typedef struct asr_fbank_config {
    float sample_rate;          /* Hz, > 0                                       */
    int win_length, hop_length; /* samples: 2 <= win <= n_fft, hop >= 1          */
    int n_fft;                  /* 256, 512, 1024 or 2048                        */
    int window;                 /* ASR_FBANK_WIN_*                               */
    float preemph;              /* 0 <= a < 1; 0 = off                           */
    int n_mels;                 /* 1 .. 128                                      */
    float f_min, f_max;         /* 0 <= f_min < f_max <= sample_rate / 2         */
    float log_floor;            /* > 0                                           */
    int n_mfcc;                 /* 0: log-mel output (D = n_mels); else D = n_mfcc <= n_mels */
    int n_context;              /* C = 0 .. 16; F = D (2C + 1) <= 4096           */
} asr_fbank_config;

typedef struct asr_fbank asr_fbank_t;

/* Host only.  Frames of an n_samples utterance (< 0: bad configuration) and
 * the feature dimension F (0: bad configuration). */
int asr_fbank_num_frames(const asr_fbank_config* cfg, int n_samples);
int asr_fbank_feature_dim(const asr_fbank_config* cfg);
/* Host only, no HIP call: the fp32 tables the device uses (any pointer may be
 * NULL): h_window[win_length], h_mel[n_mels][n_fft/2 + 1], h_dct[D][n_mels]
 * (n_mfcc > 0 only). */
int asr_fbank_host_tables(const asr_fbank_config* cfg, float* h_window, float* h_mel, float* h_dct);
/* Validates cfg before any HIP call, then uploads the tables (synchronous). */
int asr_fbank_create(const asr_fbank_config* cfg, asr_fbank_t** out);
int asr_fbank_destroy(asr_fbank_t* h);
/* Bytes of d_work for asr_fbank_fwd: the base frames [B][T][D] when
 * n_context > 0, 0 otherwise (and for a non-positive T or B). */
size_t asr_fbank_workspace_bytes(const asr_fbank_t* h, int T, int B);
/* d_wave batch-major [B][ldw], ldw >= S; d_nsamples device int32 [B] with
 * values <= S (NULL: S for all); d_out time-major [T][B][ldo], ldo >= F,
 * columns >= F of a row are not touched; T >= asr_fbank_num_frames(cfg, S):
 * all T rows are written, zeros past an utterance's frames; d_frames device
 * int32 [B] (may be NULL) receives frames_b and can be passed unchanged as
 * d_lengths of asr_lstm_fwd.  One launch does a frame's whole chain on chip
 * (one wave per frame: window, real FFT in LDS, power, sparse mel sums, log,
 * DCT); with n_context > 0 it writes base frames to d_work and a second
 * launch gathers the context rows.  Asynchronous on s, no allocation, no
 * host sync: capturable as a linear chain.  An utterance's bits depend on
 * the configuration only, never on B, its position in the batch, or T.
 * ASR_ERR_ARG: a NULL required pointer, a non-positive size, ldw < S,
 * ldo < F, T too small; ASR_ERR_UNSUPPORTED: a configuration outside the
 * ranges above (asr_fbank_create), more than 2^25 output rows T*B in one
 * call.  Both are decided before any HIP call. */
int asr_fbank_fwd(asr_fbank_t* h, const float* d_wave, long ldw, const int32_t* d_nsamples, int B, int S,
                  float* d_out, long ldo, int32_t* d_frames, void* d_work, int T, asr_stream_t s);

/* ---- back-off n-gram language model: ARPA loader, exact table, scoring -----
 * No reference member is replaced: the reference decodes without a language
 * model, while every ctcdecode caller (baseline/main.py:10) passes one.  These
 * entry points score given hypotheses (n-best rescoring of the final beam, with
 * asr_ctc_align's exact CTC score); no decoder kernel uses them.
 *
 * Model: a back-off n-gram model in ARPA text format, orders 1 ..
 * ASR_LM_MAX_ORDER.  Log10 probabilities and back-off weights are the fp32
 * nearest to the decimal text; a missing back-off field is 0.  Tabs or spaces
 * separate fields; -99 is a value like any other.  A token's id is the 0-based
 * position of its line in the \1-grams: section; <s>, </s> and <unk> get ids
 * like any other token and are reported as bos / eos / unk (-1 when absent).
 *
 * Recursion: let n = min(order, available context + 1) and the context h the
 * last n-1 tokens, <s> included while it is within reach and ASR_LM_BOS is set.
 *   p(w | h) = P(h w)               if the n-gram (h w) is in the model
 *            = bo(h) + p(w | h')    otherwise
 * with bo(h) = 0 when h is not in the model, h' = h without its earliest token,
 * p(w | empty) = P(w).  The longest n-gram present wins even when its own
 * suffix is absent (pruned models; no suffix closure is assumed).  A token's
 * value is computed in fp64 from the widened fp32 entries, added left to right
 * from 0.0: the back-offs from the longest context downward (0.0 for an absent
 * one), then P.  Its matched order (1 .. n) is the length of the n-gram whose P
 * was used.
 * OOV: an id outside [0, vocab).  With <unk> in the model it is replaced by unk
 * and scored as such, in contexts too; without, it scores oov_log10 (given at
 * create; finite, <= 0), its matched order is 0 and it cuts the context: later
 * tokens see no token at or before it.  It counts in n_oov either way.
 * Flags: ASR_LM_BOS — the context starts as [<s>], <s> itself is never scored;
 * ASR_LM_EOS — </s> is scored after the last token, also for an empty
 * hypothesis.  A flag whose token the model lacks: ASR_ERR_ARG.
 *
 * Table: a trie keyed in reverse — the n-gram (w1..wk) sits on
 * the path wk, wk-1, .., w1 — so that the walk w_i, w_i-1, .. finds the longest
 * matching n-gram and the walk w_i-1, w_i-2, .. reads every nested context's
 * back-off on the way down.  Per order: the word ids of every parent's
 * children, sorted, and (P, back-off, first child) per node; unigrams are
 * indexed directly.  Exact: no hashing.  Where an n-gram's suffix is absent the
 * missing nodes are inserted without a probability (nodes_inserted); a match
 * on one does not count as a match. */
#define ASR_LM_MAX_ORDER 8
enum { ASR_LM_BOS = 1, ASR_LM_EOS = 2 };
typedef struct asr_lm asr_lm_t;
typedef struct asr_lm_info {
    int32_t order, vocab;
    int32_t bos_id, eos_id, unk_id;           /* -1: absent */
    int32_t reserved;
    int64_t ngrams[ASR_LM_MAX_ORDER];         /* n-grams of order k+1 in the file */
    int64_t nodes_inserted;                   /* trie nodes that carry no probability */
    int64_t table_bytes;                      /* bytes of the tables (host = device) */
} asr_lm_info;

/* Host only, no HIP call (they work on a machine without a GPU): parse the
 * file / the `bytes` bytes at `text` and build the tables.
 * ASR_ERR_ARG: a NULL argument, oov_log10 not finite or > 0, an unreadable
 * file, a missing \data\ or \end\, no unigram, orders that are not 1 .. n
 * without a gap, a section whose count differs from its `ngram k=` line, a
 * non-numeric, NaN or infinite value, a probability > 0, a token of a
 * higher-order n-gram that has no unigram, a duplicate n-gram, a wrong number
 * of fields (k + 1 or k + 2 for order k; a back-off given at the top order is
 * read and never used); ASR_ERR_UNSUPPORTED: an order above
 * ASR_LM_MAX_ORDER, 2^31 or more n-grams (or trie nodes) in one order;
 * ASR_ERR_OOM: a host allocation failed.  Text before the \data\ line and
 * after the \end\ line is ignored; a top order declared with 0 n-grams does
 * not count as an order. */
int asr_lm_create_arpa(const char* path, float oov_log10, asr_lm_t** out);
int asr_lm_create_arpa_mem(const char* text, size_t bytes, float oov_log10, asr_lm_t** out);
int asr_lm_destroy(asr_lm_t* h);
int asr_lm_get_info(const asr_lm_t* h, asr_lm_info* info);
/* *id = -1 when the token is absent (still ASR_OK). */
int asr_lm_token_id(const asr_lm_t* h, const char* token, int32_t* id);
/* *token points into the handle (valid until asr_lm_destroy); ASR_ERR_ARG for
 * an id outside [0, vocab). */
int asr_lm_token_string(const asr_lm_t* h, int32_t id, const char** token);

/* Score N hypotheses.  tokens [N][ldt] token ids, ldt >= max_len; lengths [N]
 * clamped to [0, max_len], NULL = max_len for every hypothesis.  Outputs, each
 * may be NULL, at least one given:
 *   logp [N]            total log10 probability (fp64);
 *   counts [N][2]       tokens scored (</s> included) and OOVs;
 *   tok_logp [N][ldd]   per-token log10 probability (fp64);
 *   tok_order [N][ldd]  per-token matched order;
 * ldd >= max_len + 1: the </s> entry is at index L; entries past the scored
 * ones are not touched.  The total is the sum of 64 partial sums in a fixed
 * tree (partial l: positions l, l+64, .. in increasing order, from 0.0; then
 * partial[l] += partial[l + 32], + 16, .. + 1), so a hypothesis' results depend
 * only on its own tokens and the flags: never on N, its row, ldt, max_len or
 * which outputs were asked for.
 * asr_lm_score_host: host arrays, plain C++ over the same tables, one thread,
 * no HIP call — the library's CPU path; same results as the device, bit for
 * bit.
 * asr_lm_upload: copies the tables to the current device (synchronous; a
 * second call is a no-op).  A handle serves the device it was uploaded on.
 * asr_lm_score: device arrays; one launch, one wave per hypothesis (lane l
 * takes positions l, l+64, ..), asynchronous on s, no allocation, no host sync.
 * Checks, in this order, all before any HIP call — ASR_ERR_ARG: a NULL handle
 * or tokens, a non-positive N, ldt < max_len, ldd < max_len + 1 with a detail
 * output, no output, a flag whose token is absent; ASR_ERR_UNSUPPORTED:
 * max_len > 65536 or < 0; ASR_ERR_STATE (asr_lm_score only): not uploaded. */
int asr_lm_score_host(const asr_lm_t* h, const int32_t* h_tokens, long ldt, const int32_t* h_lengths, int N,
                      int max_len, int flags, double* h_logp, int32_t* h_counts, double* h_tok_logp,
                      int32_t* h_tok_order, long ldd);
int asr_lm_upload(asr_lm_t* h);
int asr_lm_score(const asr_lm_t* h, const int32_t* d_tokens, long ldt, const int32_t* d_lengths, int N,
                 int max_len, int flags, double* d_logp, int32_t* d_counts, double* d_tok_logp,
                 int32_t* d_tok_order, long ldd, asr_stream_t s);

/* ---- edit distance, WER counts and n-best minimum-Bayes-risk rescoring -----
 * No reference member is replaced: the reference neither scores a decode
 * against a transcript nor re-ranks its beam.  These entry points score given
 * token rows; no decoder kernel uses them.
 *
 * Sequences are rows of int32 tokens (label ids, word ids, anything); tokens
 * are compared by equality only, so every int32 value is legal.  For a pair
 * (reference a of length la, hypothesis b of length lb):
 *   D[i][0] = i (i deletions)      D[0][j] = j (j insertions)
 *   D[i][j] = min( D[i-1][j-1] + (a_i != b_j),    diagonal: hit or substitution
 *                  D[i-1][j]   + 1,               up: deletion (a_i has no partner)
 *                  D[i][j-1]   + 1 )              left: insertion (b_j has no partner)
 * The distance is D[la][lb].  The counts (hits, substitutions, deletions,
 * insertions) are those of the one alignment fixed by the tie rule: at every
 * cell the diagonal wins among equal minima, then up, then left.  The counts
 * are carried forward with the cell (a cell's counts are its chosen
 * predecessor's plus its own operation); no back-pointers are kept.  Always
 * S + D + I = distance, H + S + D = la, H + S + I = lb.  kitten / sitting: 3 and
 * (4, 2, 0, 1); ab / ba: 2 and (0, 2, 0, 0); abcd / bcde: 2 and (3, 0, 1, 1).
 * Lengths are clamped to [0, the call's maximum length]; a NULL length array
 * means the maximum length for every row.
 *
 * asr_edit_distance: pair p scores row d_ref_idx[p] of ref [n_ref][ldr]
 * against row d_hyp_idx[p] of hyp [n_hyp][ldh]; a NULL index array means row
 * p (then P <= that table's row count).  Outputs, each may be NULL, at least
 * one given: dist [P]; ops [P][4] = (H, S, D, I).  An index outside its table
 * gives distance -1 and counts -1 and is never used for a read.  One launch,
 * one wave per pair (the DP in registers), asynchronous on s, no allocation,
 * no workspace, no host sync.
 *
 * asr_nbest_mbr: group g is rows [gs[g], gs[g+1]) of tokens [N][ldt], gs =
 * group_start [G + 1]; a group with gs[g] < 0, gs[g+1] > N or gs[g+1] < gs[g]
 * is empty; rows of a group beyond its first max_hyps are not part of it and
 * nothing of theirs is written.  Hypothesis j of a group of n has the natural-
 * log weight w_j (weight [N], by row; NULL: uniform).  A NaN weight counts as
 * -inf; with m = max_j w_j: e_j = exp(w_j - m) for a finite m, e_j = 1 for
 * every j when m = -inf, e_j = (w_j == +inf) when m = +inf.  Then
 *   Z = sum_j e_j     risk_k = (sum_j e_j * d(k, j)) / Z
 * both sums in asr_lm_score's fixed tree (partial l: j = l, l+64, l+128, l+192
 * in increasing order from 0.0; then partial[l] += partial[l + 32], + 16, ..
 * + 1), e_j * d one rounded product and one rounded add (no fma).
 *   dist [N][ldm], ldm >= max_hyps, required: row k, column j - gs[g] is
 *     d(k, j) over the group's members (symmetric, 0 diagonal); columns >= n
 *     are not touched.  It is the intermediate and an output.
 *   risk [N] and best [G] (the row, within its group, of the smallest risk,
 *     the lowest on ties; -1 for an empty group) may each be NULL, not both.
 * Two launches (the pair distances, then the risks), a linear chain on s that
 * can be captured; no allocation, no host sync.
 *
 * The _host twins take host arrays: plain C++ on one thread, no HIP call — the
 * library's CPU path.  The cell update and the risk sum are the kernels' own
 * functions, so integers agree exactly and risks differ only through exp().
 * A pair's results depend on its two sequences only — never on P, N, its
 * position, the leading dimensions, the maximum lengths of the call or which
 * outputs were asked for; a group's on its own rows and weights only.
 * Checks, in this order, all before any HIP call — ASR_ERR_ARG: a NULL
 * required pointer (ref, hyp; tokens, group_start, dist), a non-positive P, N,
 * G, row count or max_hyps, a leading dimension below its maximum length or
 * ldm < max_hyps, no output, a NULL index array with P above that table's row
 * count; ASR_ERR_UNSUPPORTED: a maximum length above ASR_EDIT_MAX_LEN or
 * negative, max_hyps > ASR_MBR_MAX_HYPS. */
#define ASR_EDIT_MAX_LEN 1024
#define ASR_MBR_MAX_HYPS 256
int asr_edit_distance(const int32_t* d_ref, long ldr, const int32_t* d_ref_len, int n_ref, int max_ref_len,
                      const int32_t* d_hyp, long ldh, const int32_t* d_hyp_len, int n_hyp, int max_hyp_len,
                      const int32_t* d_ref_idx, const int32_t* d_hyp_idx, int P,
                      int32_t* d_dist, int32_t* d_ops, asr_stream_t s);
int asr_edit_distance_host(const int32_t* h_ref, long ldr, const int32_t* h_ref_len, int n_ref, int max_ref_len,
                           const int32_t* h_hyp, long ldh, const int32_t* h_hyp_len, int n_hyp, int max_hyp_len,
                           const int32_t* h_ref_idx, const int32_t* h_hyp_idx, int P,
                           int32_t* h_dist, int32_t* h_ops);
int asr_nbest_mbr(const int32_t* d_tokens, long ldt, const int32_t* d_lengths, int N, int max_len,
                  const int32_t* d_group_start, int G, int max_hyps, const double* d_weight,
                  int32_t* d_dist, long ldm, double* d_risk, int32_t* d_best, asr_stream_t s);
int asr_nbest_mbr_host(const int32_t* h_tokens, long ldt, const int32_t* h_lengths, int N, int max_len,
                       const int32_t* h_group_start, int G, int max_hyps, const double* h_weight,
                       int32_t* h_dist, long ldm, double* h_risk, int32_t* h_best);

/* ---- CTC beam search with n-gram LM shallow fusion ---------------------------
 * No reference member is replaced (the reference decodes without a language
 * model).  A decoder of its own (csrc/ctc_lm.hip): asr_ctc_* and
 * its kernels are untouched.  Rescoring (CTCDecoder.lm_rescore) can only reorder
 * what an acoustic-only beam kept; here the LM takes part in every prune.
 *
 * Search: the reference search of asr_ctc_* (states "q" / "q$",
 * one initial state per symbol, extension and merge in the std::set fold order,
 * fp64 lse, the final "q" / "q$" merge).  Only what the prune and the final
 * ranking compare changes.
 *
 * Tokens: tok_of_label[V] maps every non-blank label to one LM token id (the
 * blank's entry is ignored): character, BPE and word-piece models.  An id
 * outside [0, vocab) is an OOV under asr_lm_*'s rule above (<unk> if present,
 * else oov_log10, order 0, and it cuts the context).
 *
 * Per-prefix LM weight: aln10 = (double)alpha * 2.302585092994046, computed once
 * on the host.  For a prefix q of labels c1..cn let v_i be the value of position
 * i of the token row tok(c1)..tok(ci) under asr_lm_score's per-token rule, with
 * ASR_LM_BOS as configured and ASR_LM_EOS off.  Then
 *   W(empty) = 0.0    W(q+c) = W(q) + ((aln10 * v) + beta)
 *   L(empty) = 0.0    L(q+c) = L(q) + v            n(q+c) = n(q) + 1
 * every operation a rounded fp64 operation (no fma).  A prefix has one parent,
 * so W, L and n depend on q only, never on the lineage that reached q.
 *
 * Prune: a state s is compared by fused(s) = pathScore(s) + W(prefix of s).
 * Every state with fused >= the (beam_width+1)-th largest fused survives (ties
 * at the cutoff all survive; all states survive when there are at most
 * beam_width).  The merge of equal strings is unchanged: an lse fold of
 * pathScore in the reference's set order.
 *
 * Label cutoff top_n (ctcdecode's cutoff_top_n): 0 or >= V-1 means every label.
 * Otherwise C_t is the top_n non-blank labels with the largest emission (the
 * fp32 values as given) at frame t of that utterance, the smaller label id
 * first among equal values.  A non-blank label outside C_t takes part in no
 * transition at t: neither the extension nor the repeat "qc"+c -> "qc".  Blank
 * always takes part.  Frame 0's initial states are "$" and one per label of C_0.
 *
 * Final ranking: after the last prune and the "q" / "q$" merge,
 * total(q) = ctc(q) + W(q); with ASR_LM_EOS, total(q) + (aln10 * v_eos) where
 * v_eos is </s> scored after q (no beta for it, not counted in n, added into L).
 * Ranked by (total descending, code string ascending); best is rank 0.  Per
 * hypothesis: labels, total, ctc_logp, lm_log10 = L, n_tokens = n.  L is a
 * left-to-right sum while asr_lm_score's total is a tree of 64 partial sums:
 * the two agree to rounding only.
 *
 * With alpha = 0 and beta = 0, W is exactly 0.0 for every prefix and the search
 * is asr_ctc_*'s.
 *
 * Limits: alpha >= 0 and finite, beta finite; V <= 4096; at most 255 candidate
 * non-blank labels per frame (top_n ? min(top_n, V-1) : V-1); beam_width + 1 +
 * ties <= 256, max_states as in asr_ctc_create (0 = automatic).  If the states
 * that survive a prune exceed max_states, the fetch returns
 * ASR_ERR_BEAM_OVERFLOW (the utterance then reports 0 hypotheses), for an
 * automatic and an explicit capacity alike: there is no automatic re-decode.
 * Per-utterance lengths are in [1, T].
 *
 * asr_ctc_lm_create: host only, no HIP call.  The LM handle must outlive the
 * decoder handle.  Checks, in this order — ASR_ERR_ARG: out NULL; lm or
 * tok_of_label NULL; V < 2, beam_width < 1, blank_id outside [0, V); alpha
 * negative or not finite, beta not finite; lm_flags with other bits than
 * ASR_LM_BOS | ASR_LM_EOS, top_n < 0, max_states < 0; a flag whose token the
 * model lacks.  ASR_ERR_UNSUPPORTED: V > 4096.  ASR_ERR_ARG: two equal codes;
 * 0 < max_states < beam_width + 1.  ASR_ERR_UNSUPPORTED: more than 255
 * candidate labels; a capacity (rounded up to a multiple of 32) above 256.
 *
 * asr_ctc_lm_decode: device emissions, addressed as in asr_ctc_decode_ex
 * (element (t, b, v) at d_emis[t*frame_stride + b*utt_stride + v]; h_lengths a
 * host array, NULL = T for all).  Asynchronous on s: the label cutoff (one wave
 * per frame and utterance, only with top_n) and the search (one workgroup per
 * utterance).  The workspace is sized once per shape and reused while the next
 * shape fits.  An utterance's results depend on its own frames only: never on
 * its row, B, the strides or the other utterances.  d_emis must stay in place
 * until the stream has run the decode.  A handle holds one decode at a time: the
 * next decode (either kind) discards the results of the previous one, and waits
 * for it first when it was queued on another stream.
 * asr_ctc_lm_decode_host: the host twin — host emissions, plain C++ over
 * std::map / std::set with the LM's host tables, one thread, no HIP call: the
 * library's CPU path.  Labels, ranks and n_tokens equal the device's; scores
 * differ only through exp / log / log1p.
 * Checks of both, in this order, before any HIP call — ASR_ERR_ARG: h or the
 * emissions NULL, T < 1, B < 1, a stride < 1, a length outside [1, T];
 * ASR_ERR_STATE (asr_ctc_lm_decode only): the LM was not uploaded
 * (asr_lm_upload).
 *
 * asr_ctc_lm_get_beams: the ranked final beam of every utterance of the last
 * decode (either kind; waits for a device decode): h_n_hyps[B],
 * h_lengths[B][max_hyps], h_labels[B][max_hyps][max_len], and, each may be
 * NULL, h_total, h_ctc_logp, h_lm_log10 (fp64) and h_n_tokens [B][max_hyps].
 * asr_ctc_lm_get_best: rank 0 only: h_labels[B][max_len], h_lengths[B],
 * h_total[B] (may be NULL).  Checks, in this order — ASR_ERR_ARG: h NULL,
 * max_hyps < 1, max_len < 1, h_n_hyps, h_lengths or h_labels NULL;
 * ASR_ERR_STATE: no decode yet on this handle.  ASR_ERR_BEAM_OVERFLOW as above
 * (the other utterances' results are written).
 * asr_ctc_lm_host_gaps: h_gap[B], per utterance of the last HOST decode, the
 * smallest relative distance |x - y| / max(1, |x|, |y|) it met between two
 * finite scores that differ and whose order decides something: at every prune
 * the cutoff against every other fused score, and adjacent final totals
 * (+inf: none met).  A caller comparing two implementations learns from it
 * whether a difference in ranks can be rounding.  ASR_ERR_ARG: h or h_gap NULL;
 * ASR_ERR_STATE: the last decode on this handle was not a host decode.
 * asr_ctc_lm_destroy: ASR_ERR_ARG for NULL. */
typedef struct asr_ctc_lm asr_ctc_lm_t;
int asr_ctc_lm_create(const int32_t* codes, int V, int beam_width, int blank_id, int max_states,
                      const asr_lm_t* lm, const int32_t* tok_of_label, float alpha, float beta, int lm_flags,
                      int top_n, asr_ctc_lm_t** out);
int asr_ctc_lm_destroy(asr_ctc_lm_t* h);
int asr_ctc_lm_decode(asr_ctc_lm_t* h, const float* d_emis, int T, int B, long frame_stride, long utt_stride,
                      const int32_t* h_lengths, int is_log, asr_stream_t s);
int asr_ctc_lm_decode_host(asr_ctc_lm_t* h, const float* h_emis, int T, int B, long frame_stride,
                           long utt_stride, const int32_t* h_lengths, int is_log);
int asr_ctc_lm_get_beams(asr_ctc_lm_t* h, int max_hyps, int max_len, int32_t* h_n_hyps, int32_t* h_lengths,
                         int32_t* h_labels, double* h_total, double* h_ctc_logp, double* h_lm_log10,
                         int32_t* h_n_tokens);
int asr_ctc_lm_get_best(asr_ctc_lm_t* h, int32_t* h_labels, int max_len, int32_t* h_lengths, double* h_total);
int asr_ctc_lm_host_gaps(asr_ctc_lm_t* h, double* h_gap);

/* ---- Word-level LM fused through a lexicon trie ----------------
 * Character labels, a word-level n-gram model: the search is the fused search
 * above, unchanged (states, fold order, fp64 lse, fused(s) = pathScore(s) +
 * W(prefix of s), the prune with ties kept, top_n, the final merge, the ranking).
 * Only what a prefix carries, and when W moves, changes.  One non-blank label is
 * the space label sp.
 *
 * Lexicon: a set of words, each a non-empty sequence of non-blank, non-space
 * labels with one LM token id, kept as a trie.  An id outside the model's
 * [0, vocab) is an OOV under asr_lm_*'s rule.
 *
 * Every prefix q carries z(q), a trie node: the root (the partial word is empty),
 * a node, or OFF (the partial word is no prefix of a lexicon word); n(q), the
 * words scored; the last min(n, 7) word tokens; W and L.  All depend on the
 * string q only.
 *   q + c, c != sp:  z = child(z(q), c), OFF if there is none or z(q) is OFF;
 *                    W, L, n and the context are unchanged.
 *   q + sp, the partial word empty (q empty or ending in sp): nothing changes
 *                    (an empty word is not a word).
 *   q + sp otherwise: w = the word token of z(q) if z(q) is terminal, else -1 (an
 *                    OOV); v = the per-token value of w after the word context,
 *                    ASR_LM_BOS as configured, ASR_LM_EOS off;
 *                    W = W(q) + ((aln10 * v) + beta), L = L(q) + v,
 *                    n = n(q) + 1, z = the root.
 * every operation a rounded fp64 operation.  Final: a hypothesis whose partial
 * word is not empty gets that word scored by the same rule (with beta, counted in
 * n) before the totals; then ASR_LM_EOS applies as above.
 *
 * lex_mode ASR_LEX_OPEN: every transition of the plain search exists; words
 * outside the lexicon cost the OOV value.  ASR_LEX_CLOSED: a transition q -> q+c,
 * c != sp, exists only if z(q+c) is not OFF, and q -> q+sp only if z(q) is
 * terminal (so no leading or doubled space and no unfinished word before a
 * space).  A removed transition takes part in nothing at that frame, like a label
 * outside C_t.  Blank and the repeat "qc"+c -> "qc" always exist.  At the final a
 * partial word that is not terminal is still scored as an OOV: closed mode
 * constrains transitions, not final states.
 *
 * With alpha = 0 and beta = 0 in open mode W is exactly 0.0 and the search is
 * asr_ctc_*'s.  The limits are those above.
 *
 * asr_lexicon_create: host only.  spell holds the words' label ids one after
 * another, offsets[n_words + 1] delimits them (offsets[0] = 0), tok[n_words] are
 * their LM token ids.  Checks, in this order — ASR_ERR_ARG: out NULL; spell,
 * offsets or tok NULL; V < 2, n_words < 1, space_label outside [0, V);
 * offsets[0] != 0 or decreasing offsets; a label outside [0, V) or equal to
 * space_label; an empty word; a negative token; one spelling with two different
 * tokens (the same spelling with the same token counts once).
 * ASR_ERR_UNSUPPORTED: 2^31 or more trie nodes.
 * asr_lexicon_upload: copies the trie to the current device (synchronous; a
 * second call does nothing).  asr_lexicon_get_info: words, nodes (the root
 * included), the largest child count, bytes of the three tables.
 * asr_lexicon_destroy: ASR_ERR_ARG for NULL.
 *
 * asr_ctc_lm_create_word: an asr_ctc_lm_t on which asr_ctc_lm_decode,
 * _decode_host, _get_beams, _get_best, _host_gaps and _destroy work as above;
 * n_tokens is then n (words), lm_log10 is L, lengths stay label counts.  The
 * lexicon and the LM must outlive the handle.  Checks: asr_ctc_lm_create's, with
 * lex in the place of tok_of_label, and, after "a flag whose token the model
 * lacks" — ASR_ERR_ARG: the lexicon's V differs from V; a spelling uses
 * blank_id; space_label == blank_id; lex_mode neither ASR_LEX_OPEN nor
 * ASR_LEX_CLOSED.  asr_ctc_lm_decode returns ASR_ERR_STATE until both
 * asr_lm_upload and asr_lexicon_upload have run. */
enum { ASR_LEX_OPEN = 0, ASR_LEX_CLOSED = 1 };
typedef struct asr_lexicon asr_lexicon_t;
typedef struct asr_lexicon_info {
    int32_t words;         /* distinct spellings */
    int32_t nodes;         /* trie nodes, the root included */
    int32_t max_children;  /* the widest sibling run */
    int32_t space_label;
    int64_t table_bytes;
} asr_lexicon_info;
int asr_lexicon_create(const int32_t* spell, const int64_t* offsets, const int32_t* tok, int n_words, int V,
                       int space_label, asr_lexicon_t** out);
int asr_lexicon_upload(asr_lexicon_t* h);
int asr_lexicon_get_info(const asr_lexicon_t* h, asr_lexicon_info* info);
int asr_lexicon_destroy(asr_lexicon_t* h);
int asr_ctc_lm_create_word(const int32_t* codes, int V, int beam_width, int blank_id, int max_states,
                           const asr_lm_t* lm, const asr_lexicon_t* lex, float alpha, float beta, int lm_flags,
                           int top_n, int lex_mode, asr_ctc_lm_t** out);

/* ---- RNN-T (transducer) greedy decoding on the device ----------
 * The model: an embedding Emb [V][D]; L (1 or 2) LSTM layers of asr_lstm_fwd's
 * cell (W_ih [in][4Hp], W_hh [Hp][4Hp], b_ih, b_hh [4Hp]; gates i, f, g, o;
 * (x.W_ih + h.W_hh) + (b_ih + b_hh)); and the joint
 *   f_t = enc_t.W_enc + b_enc      W_enc [E][J]
 *   g   = h_top.W_pred + b_pred    W_pred [Hp][J]
 *   z   = act(f_t + g)             ReLU or tanh
 *   logit = z.W_out + b_out        W_out [J][V]
 * all weights in this library's [in][out] layout.  k = argmax logit, the lowest
 * index among equal maxima (a NaN never wins); logp = logit[k] -
 * logsumexp(logit).
 *
 * The greedy walk of utterance b (length len_b, clamped to [0, T]): with no
 * state given h = c = 0 and the predictor takes one step on Emb[blank] (NeMo's
 * blank_as_pad start is the case of a zero row there); with a state given,
 * (h, c) is used as it stands.  t = 0, n = 0; while t < len_b the joint is
 * evaluated: k != blank records (k, t, logp), steps the predictor on Emb[k] and
 * counts n += 1, and at n == max_symbols moves on (t += 1, n = 0) without
 * another evaluation; k == blank adds its logp to the total only, t += 1,
 * n = 0.  max_symbols >= 1 is required: there is no unbounded mode.
 *
 * Outputs per utterance: tokens, timesteps (frames of this call, from 0) and
 * token log-probs, rows of max_out; the count of emissions, which keeps
 * counting past max_out (records beyond max_out are dropped while the walk and
 * the state go on); the total log-prob (emissions and blanks); the state after
 * the last frame.  A state is [2][L][B][Hp]: h of every layer, then c.
 * Streaming: a call ends at a frame boundary (n = 0), so passing a call's
 * state to the next and adding the frame offset to its timesteps reproduces a
 * whole decode bit for bit.
 *
 * asr_rnnt_create takes host pointers and keeps a host copy (for
 * asr_rnnt_greedy_host).  Checks, in this order — ASR_ERR_ARG: a NULL
 * argument; V < 2; blank outside [0, V); a non-positive E, D, Hp, J;
 * L < 1; max_symbols < 1; act neither ASR_RNNT_ACT_RELU nor _TANH.
 * ASR_ERR_UNSUPPORTED: L > 2; D, Hp or J not a multiple of 16; the limit of the
 * decode kernel, whose rows live in LDS:
 *     64 * (2 * L * (Hp + 4) + (J + 4)) + 4096 <= 160 KiB
 * (L = 1: up to Hp = J = 816, or e.g. 1024 / 432; L = 2: up to
 * Hp = J = 480).  Then ASR_ERR_ARG: a NULL weight of a layer in use.
 * asr_rnnt_upload copies the weights to the current device and computes
 * Emb.W_ih of layer 0 there (one GEMM under the asr_set_dense_arith setting of
 * that moment; synchronous; a second call does nothing).
 * asr_rnnt_workspace_bytes(h, T, B): f [T*B][J] and 16 * (L * Hp + J) floats
 * per 16 utterances; 0 for a NULL handle, a non-positive size or T*B > INT_MAX.
 *
 * asr_rnnt_greedy: device pointers.  d_enc [T*B][E] time-major; d_lengths
 * int32 [B] or NULL (= T); d_state_in NULL or a state; d_state_out NULL or a
 * state (may be d_state_in); d_tokens, d_timesteps int32 [B][max_out], d_logp
 * double [B][max_out] (entries at and beyond the count are not written; the
 * three may be NULL when max_out = 0); d_count int32 [B]; d_total double [B];
 * d_work of asr_rnnt_workspace_bytes(h, T, B) bytes, 16-byte aligned.  f for
 * all T is one GEMM that follows asr_set_dense_arith (bias fused); the walk is
 * one launch, 16 utterances per workgroup, at most T * (max_symbols + 1) joint
 * evaluations per utterance by a bound the host sets.  Asynchronous on s, no
 * allocation, no host synchronisation.  An utterance's bits depend on the
 * model's shape only, never on B or on the utterances beside it.
 * asr_rnnt_greedy_host: the same on host memory, one thread, fp64 accumulation
 * from the fp32 weights; its states and every floating-point output are double
 * (so that a chunked host decode equals a whole one); h_gap (optional,
 * double [B]): the smallest gap between the best and the second-best logit met
 * on the utterance's walk (HUGE_VAL when it evaluated nothing).
 * Checks of both, in this order, before any HIP call — ASR_ERR_ARG: h, the
 * encoder output, the count or the total NULL; non-positive T or B;
 * max_out < 0; max_out > 0 with a NULL token, timestep or log-prob array.
 * ASR_ERR_UNSUPPORTED: T*B > INT_MAX; T * (max_symbols + 1) >= INT_MAX.
 * asr_rnnt_greedy only, then: ASR_ERR_ARG for a NULL d_work; ASR_ERR_STATE
 * when the weights were not uploaded. */
enum { ASR_RNNT_ACT_RELU = 0, ASR_RNNT_ACT_TANH = 1 };
#define ASR_RNNT_MAX_LAYERS 2
typedef struct asr_rnnt asr_rnnt_t;
typedef struct asr_rnnt_desc {
    int32_t V, blank, E, D, Hp, L, J, act, max_symbols;
} asr_rnnt_desc;
typedef struct asr_rnnt_weights {
    const float* emb;                          /* [V][D] */
    const float* w_ih[ASR_RNNT_MAX_LAYERS];    /* [D or Hp][4Hp] */
    const float* w_hh[ASR_RNNT_MAX_LAYERS];    /* [Hp][4Hp] */
    const float* b_ih[ASR_RNNT_MAX_LAYERS];    /* [4Hp] */
    const float* b_hh[ASR_RNNT_MAX_LAYERS];
    const float* w_enc;                        /* [E][J] */
    const float* b_enc;
    const float* w_pred;                       /* [Hp][J] */
    const float* b_pred;
    const float* w_out;                        /* [J][V] */
    const float* b_out;
} asr_rnnt_weights;
typedef struct asr_rnnt_info {
    asr_rnnt_desc desc;
    int32_t uploaded;      /* 1 after asr_rnnt_upload */
    int32_t lds_bytes;     /* of the decode kernel */
    int64_t weight_bytes;  /* of the host copy */
} asr_rnnt_info;
int asr_rnnt_create(const asr_rnnt_desc* desc, const asr_rnnt_weights* weights, asr_rnnt_t** out);
int asr_rnnt_upload(asr_rnnt_t* h);
int asr_rnnt_get_info(const asr_rnnt_t* h, asr_rnnt_info* info);
int asr_rnnt_destroy(asr_rnnt_t* h);
size_t asr_rnnt_workspace_bytes(const asr_rnnt_t* h, int T, int B);
int asr_rnnt_greedy(const asr_rnnt_t* h, const float* d_enc, const int32_t* d_lengths, int T, int B, int max_out,
                    const float* d_state_in, float* d_state_out, int32_t* d_tokens, int32_t* d_timesteps,
                    double* d_logp, int32_t* d_count, double* d_total, void* d_work, asr_stream_t s);
int asr_rnnt_greedy_host(const asr_rnnt_t* h, const float* h_enc, const int32_t* h_lengths, int T, int B, int max_out,
                         const double* h_state_in, double* h_state_out, int32_t* h_tokens, int32_t* h_timesteps,
                         double* h_logp, int32_t* h_count, double* h_total, double* h_gap);

/* RNN-T beam search, one symbol per frame (the "modified beam search" of k2 /
 * icefall), on an asr_rnnt handle.  The model and the start are the greedy
 * walk's (h = c = 0, then one predictor step on Emb[blank]); desc.max_symbols
 * plays no part.
 *
 * Utterance b has beam width K, 1 <= K <= 16, and length len_b clamped to
 * [0, T].  A hypothesis is its tokens ys, one timestep per token, a score (a
 * log-probability, double) and the predictor state after ys.  The beam A is
 * ordered by rank and starts as one hypothesis: empty ys, score 0.  Each frame
 * t < len_b: (1) for every hypothesis i in rank order logit_i = joint(f_t,
 * h_top_i) and lp_i[v] = logit_i[v] - logsumexp(logit_i); (2) candidate (i, v)
 * has score s_i + lp_i[v]; (3) the best min(K, |A| V) candidates are kept, in
 * the order score descending, then i ascending, then v ascending, a NaN score
 * after every number; (4) a kept (i, blank) is hypothesis i unchanged but for
 * its score; (5) a kept (i, v != blank) is ys_i + [v] with timestep t and the
 * state of i stepped on Emb[v]; (6) kept candidates with equal token sequences
 * merge: the score is logaddexp of the two in double, the timesteps are those
 * of the constituent with the higher score (the earlier in candidate order on
 * equal scores); at most two candidates can share a sequence (A + blank and
 * B + v); sequences are compared as sequences, not by parentage, so a prefix
 * that was pruned and created again still merges; (7) the new A is the merged
 * set by score descending, ties by the position of the earlier constituent in
 * candidate order; it may hold fewer than K hypotheses.  The result is the
 * final A, best first.  K = 1 is the greedy walk with max_symbols = 1.
 *
 * asr_rnnt_beam_workspace_bytes(h, T, B, K): f [T*B][J]; per workgroup of
 * 16 / R utterances (R the smallest power of two >= K) 16 * (2 * L * Hp + J + V)
 * floats; per utterance T*K + 1 node records of 16 bytes.  0 for a NULL handle,
 * a non-positive size, K outside [1, 16], T*B > INT_MAX or T*K + 1 > INT_MAX.
 *
 * asr_rnnt_beam: device pointers.  d_enc [T*B][E] time-major; d_lengths int32
 * [B] or NULL (= T); d_tokens, d_timesteps int32 [B][nbest][max_out] (may be
 * NULL when max_out = 0; a hypothesis longer than max_out is cut there);
 * d_len int32 [B][nbest], the uncut lengths; d_score double [B][nbest]; d_nhyp
 * int32 [B], min(|A|, nbest); entries of hypotheses at and beyond d_nhyp[b] and
 * tokens at and beyond a length are not written.  len_b = 0 gives one empty
 * hypothesis with score 0.  d_work of asr_rnnt_beam_workspace_bytes bytes,
 * 16-byte aligned.  f for all T is one GEMM that follows asr_set_dense_arith;
 * the search is one launch.  Asynchronous on s, no allocation, no host
 * synchronisation.  An utterance's bits depend on the model's shape and on K
 * only, never on B or on the utterances beside it.
 * asr_rnnt_beam_host: the same on host memory, one thread, fp64 from the fp32
 * weights, sequences compared as such.  h_margin (optional, double [B]): the
 * smallest over the utterance's search of (a) the score of the last kept
 * candidate minus that of the best rejected one, (b) the absolute score
 * difference of the two constituents of a merge, (c) the gaps between
 * neighbouring final scores; HUGE_VAL when none occurred.
 * Checks of both, in this order, before any HIP call — ASR_ERR_ARG: h, the
 * encoder output, the lengths, scores or counts NULL, or non-positive T or B;
 * K outside [1, 16]; nbest outside [1, K]; max_out < 0; max_out > 0 with a
 * NULL token or timestep array.  ASR_ERR_UNSUPPORTED: T*B > INT_MAX or
 * T*K + 1 > INT_MAX.  asr_rnnt_beam only, then: ASR_ERR_ARG for a NULL d_work;
 * ASR_ERR_UNSUPPORTED when the search kernel's rows do not fit in LDS,
 *     64 * (2 * L * (Hp + 4) + (J + 4)) + 8192 <= 160 KiB
 * (the greedy limit with 8192 in place of 4096, for any K; L = 1: up to
 * Hp = J = 800); ASR_ERR_STATE when the weights were not uploaded. */
size_t asr_rnnt_beam_workspace_bytes(const asr_rnnt_t* h, int T, int B, int K);
int asr_rnnt_beam(const asr_rnnt_t* h, const float* d_enc, const int32_t* d_lengths, int T, int B, int K, int nbest,
                  int max_out, int32_t* d_tokens, int32_t* d_timesteps, int32_t* d_len, double* d_score,
                  int32_t* d_nhyp, void* d_work, asr_stream_t s);
int asr_rnnt_beam_host(const asr_rnnt_t* h, const float* h_enc, const int32_t* h_lengths, int T, int B, int K,
                       int nbest, int max_out, int32_t* h_tokens, int32_t* h_timesteps, int32_t* h_len,
                       double* h_score, int32_t* h_nhyp, double* h_margin);

/* RNN-T beam search with n-gram LM shallow fusion: the LM takes part in every
 * per-frame prune.  The search is the one above, steps (1) to
 * (7); only what the prune and the rankings compare changes, by the conventions
 * of asr_ctc_lm_*.
 *
 * Tokens.  tok_of_label[V] maps every non-blank label to one LM token id; the
 * blank's entry is ignored.  An id outside [0, vocab) is an OOV under
 * asr_lm_score's rule: it scores as <unk> if the model has one, else as
 * oov_log10 at order 0, and it cuts the context.
 *
 * LM weight of a hypothesis.  aln10 = (double)alpha * 2.302585092994046, once
 * on the host.  For tokens ys = y1..yn let v_i be the per-token value of
 * asr_lm_score at position i of the row tok(y1)..tok(yi), ASR_LM_BOS as
 * configured and ASR_LM_EOS off.  Then
 *     W(empty) = 0.0,  W(ys + [y]) = W(ys) + ((aln10 * v) + beta),
 *     L(empty) = 0.0,  L(ys + [y]) = L(ys) + v,  n = len(ys),
 * every operation a rounded fp64 operation, no fma.  W, L and n depend on the
 * sequence only, so the two constituents of a merge carry equal W and L bit for
 * bit.
 *
 * A hypothesis carries its acoustic score s (the score of the search above), W
 * and L; its fused score is s + W.  Candidate (i, blank) has acoustic
 * s_i + lp_i[blank] and weight W_i; candidate (i, v) has acoustic s_i + lp_i[v]
 * and weight W(ys_i + [v]).  Candidates are kept and ordered by fused =
 * acoustic + weight, ties as above (i ascending, then v ascending, a NaN last).
 * A merge takes logaddexp of the two acoustic scores in double; the timesteps
 * are those of the constituent with the higher fused score (the earlier on
 * equal ones).  The new A is ordered by fused score, ties by the earlier
 * constituent.
 *
 * Result.  total = s + W; with ASR_LM_EOS total = (s + W) + (aln10 * v_eos),
 * v_eos the value of </s> after ys: no beta, not counted in n, added into L.
 * The final A is ranked again by total descending, ties by rank in A, and cut
 * at nbest.  Each hypothesis returns tokens, timesteps, length, total, am = s,
 * lm_log10 = L and n_tokens = n.  len_b = 0 gives one empty hypothesis with
 * am = 0 and total 0 or the </s> term.  With alpha = beta = 0 and no
 * ASR_LM_EOS every W is exactly 0.0 and the search is asr_rnnt_beam's: equal
 * bytes in tokens, timesteps, lengths, counts and scores.
 *
 * asr_rnnt_lm_create: host only, no HIP call; the model and the LM must outlive
 * the handle; tok_of_label (V entries) is copied.  Checks, in this order —
 * ASR_ERR_ARG: out NULL; the model, the LM or tok_of_label NULL; alpha negative
 * or not finite, beta not finite; a flag other than ASR_LM_BOS | ASR_LM_EOS; a
 * flag whose token (<s>, </s>) the model does not have.
 *
 * asr_rnnt_beam_lm_workspace_bytes(z, T, B, K): asr_rnnt_beam_workspace_bytes
 * plus, per workgroup, 16 LM rows of V doubles; 0 in the same cases and for a
 * NULL handle.
 *
 * asr_rnnt_beam_lm: device pointers, as asr_rnnt_beam with d_total in place of
 * d_score; d_am, d_lm_log10 (double [B][nbest]) and d_ntok (int32 [B][nbest])
 * may each be NULL.  One GEMM and one launch, asynchronous on s, no host
 * synchronisation; the first call on a handle copies tok_of_label to the
 * device (one allocation, synchronous), every later call allocates nothing.
 * An utterance's bits depend on the model's shape, K, the LM and the weights
 * only, never on B or on the utterances beside it.
 * asr_rnnt_beam_lm_host: the same on host memory over the LM's host tables, one
 * thread, fp64.  h_margin (optional, double [B]) is asr_rnnt_beam_host's over
 * fused scores: (a) the last kept candidate against the best rejected one,
 * (b) the difference of a merge's constituents, (c) the gaps between
 * neighbouring final totals.
 * Checks of both, in this order, before any HIP call — ASR_ERR_ARG for a NULL
 * handle; then asr_rnnt_beam's checks with the totals in the scores' place.
 * asr_rnnt_beam_lm only, then: ASR_ERR_ARG for a NULL d_work;
 * ASR_ERR_UNSUPPORTED beyond asr_rnnt_beam's LDS limit; ASR_ERR_STATE when the
 * weights (asr_rnnt_upload) or the LM (asr_lm_upload) were not uploaded. */
typedef struct asr_rnnt_lm asr_rnnt_lm_t;
int asr_rnnt_lm_create(const asr_rnnt_t* model, const asr_lm_t* lm, const int32_t* tok_of_label, float alpha,
                       float beta, int lm_flags, asr_rnnt_lm_t** out);
int asr_rnnt_lm_destroy(asr_rnnt_lm_t* z);
size_t asr_rnnt_beam_lm_workspace_bytes(const asr_rnnt_lm_t* z, int T, int B, int K);
int asr_rnnt_beam_lm(asr_rnnt_lm_t* z, const float* d_enc, const int32_t* d_lengths, int T, int B, int K, int nbest,
                     int max_out, int32_t* d_tokens, int32_t* d_timesteps, int32_t* d_len, double* d_total,
                     double* d_am, double* d_lm_log10, int32_t* d_ntok, int32_t* d_nhyp, void* d_work, asr_stream_t s);
int asr_rnnt_beam_lm_host(const asr_rnnt_lm_t* z, const float* h_enc, const int32_t* h_lengths, int T, int B, int K,
                          int nbest, int max_out, int32_t* h_tokens, int32_t* h_timesteps, int32_t* h_len,
                          double* h_total, double* h_am, double* h_lm_log10, int32_t* h_ntok, int32_t* h_nhyp,
                          double* h_margin);

/* ---- RNN-T lattice scoring and forced alignment --------------
 * What comes after a transducer search: the exact log-likelihood of a GIVEN
 * transcript, its best alignment and the frames at which that alignment emits
 * each label, in fp64 log domain with the decoder's lse.  The model is an
 * asr_rnnt handle as asr_rnnt_create / asr_rnnt_upload make it.  Target n is
 * scored against utterance b = utt[n]; its labels are y_1 .. y_U, the
 * utterance has len_b frames.
 *   Predictor, teacher-forced: the greedy walk's start (h = c = 0, then one
 *     step on Emb[blank]), then one step on each of y_1 .. y_U; h_top(u) is the
 *     top layer's h after u labels, u = 0 .. U; g_u = h_top(u).W_pred + b_pred.
 *   Joint: f_t = enc_t.W_enc + b_enc, z = act(f_t + g_u), logit = z.W_out +
 *     b_out, lpb(t, u) = logit[blank] - lse(logit), and for u < U
 *     lpy(t, u) = logit[y_{u+1}] - lse(logit).
 *   Lattice, selected by topology:
 *   ASR_RNNT_LATTICE_STANDARD (0): a label arc stays in the frame: the training
 *     lattice, and the one the greedy walk moves in while it never reaches
 *     max_symbols.
 *       a(0, 0) = 0
 *       a(t, u) = lse(a(t-1, u) + lpb(t-1, u), a(t, u-1) + lpy(t, u-1))
 *       score   = a(len-1, U) + lpb(len-1, U)
 *   ASR_RNNT_LATTICE_ONE_PER_FRAME (1): a label arc consumes the frame too: the
 *     lattice asr_rnnt_beam searches.
 *       a(0, 0) = 0
 *       a(t+1, u)   (+)= a(t, u) + lpb(t, u)
 *       a(t+1, u+1) (+)= a(t, u) + lpy(t, u)          ((+) is lse)
 *       score = a(len, U); the target is infeasible when U > len.
 *   Viterbi: the same recursion with max for lse; where the two candidates of a
 *     node are exactly equal the blank predecessor wins.  vscore is the
 *     log-probability of that best alignment, and frames[i] the frame whose
 *     label arc emits label i: the convention of the timesteps of
 *     asr_rnnt_greedy / asr_rnnt_beam, so they are non-decreasing under
 *     topology 0 and strictly increasing under topology 1.
 * d_enc [T*B][E] time-major, as asr_rnnt_greedy takes it; d_lengths int32 [B],
 * clamped to [0, T], NULL = T; d_targets int32 [N][ldt], ldt >=
 * max_target_len; d_target_lengths int32 [N], clamped to [0, max_target_len];
 * d_utt int32 [N], NULL = utterance n (then N <= B); an n-best list is N = B*K
 * targets with d_utt[n] = n / K.
 * Outputs, each may be NULL, at least one given: d_score [N] double, the
 * forward log-likelihood log p(y | x); d_vscore [N] double; d_frames int32
 * [N][ldt]: entries U_n <= i < max_target_len are -1, entries at and beyond
 * max_target_len are not touched.
 * Infeasible target (a label that is the blank or outside [0, V), utt[n]
 * outside [0, B), U > len under topology 1, no frames with U > 0): scores
 * -inf, frames -1; never an out-of-range read.  No frames and U = 0: both
 * scores 0.0.
 * max_target_len is at most 255.
 * d_work: asr_rnnt_align_workspace_bytes(h, T, B, N, max_target_len) bytes,
 * 16-byte aligned; with U1 = max_target_len + 1 and up4 rounding up to a
 * multiple of 4,
 *     4 * (T*B*J + U1*N*(4*Hp + L*Hp + J) + N*Hp + 2*up4(N*T*U1) + up4(2*N))
 *       + 64 * N * (T + U1)
 * bytes: f, the predictor's input projections with its cell state, its hidden
 * states per layer, g, the two node values lpb and lpy, two int32 per target,
 * and one byte of back-pointers per lane and lattice step.  0 for an argument
 * the call refuses.
 * The device call is four stages on s: f by one GEMM; the predictor over the
 * N targets through the library's LSTM recurrence (asr_lstm_recur_fwd /
 * asr_lstm_fwd with the lengths U_n + 1) and g by one GEMM, both GEMMs
 * following asr_set_dense_arith; the fused joint kernel, which forms z in LDS,
 * multiplies by W_out on the fp32 matrix cores with a running log-sum-exp over
 * V and writes two floats per lattice node (no logit reaches memory); and the
 * lattice kernel, one wave per target.  Asynchronous on s, no allocation, no
 * host synchronisation.  A target's results depend only on its own encoder
 * frames, labels and lengths: never on N, its position, max_target_len, T, or
 * which outputs were asked for.
 * asr_rnnt_align_host: the same on host memory, one thread, fp64 from the fp32
 * weights, the same tie rule; needs no upload.
 * Checks of both, before any HIP call — ASR_ERR_ARG: h, the encoder output, the
 * targets or their lengths NULL; non-positive T, B or N; max_target_len < 0;
 * ldt < max_target_len; no output given; a topology other than 0 or 1; NULL
 * d_utt with N > B.  ASR_ERR_UNSUPPORTED: max_target_len > 255; T*B, N*U1, T*U1
 * or N * ceil(T*U1 / 16) beyond INT_MAX; N*16*Hp bytes beyond one buffer
 * resource of the recurrence (0x7ff00000).  asr_rnnt_align only, then:
 * ASR_ERR_ARG for a NULL d_work; ASR_ERR_STATE when the weights were not
 * uploaded. */
enum { ASR_RNNT_LATTICE_STANDARD = 0, ASR_RNNT_LATTICE_ONE_PER_FRAME = 1 };
size_t asr_rnnt_align_workspace_bytes(const asr_rnnt_t* h, int T, int B, int N, int max_target_len);
int asr_rnnt_align(const asr_rnnt_t* h, const float* d_enc, const int32_t* d_lengths, int T, int B,
                   const int32_t* d_targets, long ldt, const int32_t* d_target_lengths, const int32_t* d_utt, int N,
                   int max_target_len, int topology, double* d_score, double* d_vscore, int32_t* d_frames,
                   void* d_work, asr_stream_t s);
int asr_rnnt_align_host(const asr_rnnt_t* h, const float* h_enc, const int32_t* h_lengths, int T, int B,
                        const int32_t* h_targets, long ldt, const int32_t* h_target_lengths, const int32_t* h_utt,
                        int N, int max_target_len, int topology, double* h_score, double* h_vscore,
                        int32_t* h_frames);

#ifdef __cplusplus
}
#endif
#endif /* ASR_AMD_H_ */
