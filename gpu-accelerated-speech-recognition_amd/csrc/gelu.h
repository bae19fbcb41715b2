// The library's one GELU: the GEMM epilogue ASR_EPI_BIAS_GELU (dense.hip,
// dense_x3.hip), asr_layernorm_gelu_fwd (attention.hip), asr_wave_conv_fwd
// (wave_conv.hip) and asr_grouped_conv1d_fwd (grouped_conv.hip) all call this
// expression, so the same pre-activation gives the same bits everywhere.
#pragma once
#include <hip/hip_runtime.h>

namespace asr {

// Exact GELU of a pre-activation, v/2 * (1 + erf(v / sqrt 2)), written with
// 1 + erf(x) = erfc(-x): one expression for both signs and no cancellation in
// the negative tail (1 + erf(x) loses every digit below x = -3.5).  v -> -inf:
// erfc -> 0 and the product is -0; v -> +inf: erfc -> 2 and the product is v.
__device__ __forceinline__ float gelu_f32(float v) { return (0.5f * v) * erfcf(-0.70710678118654752f * v); }

}  // namespace asr
