// The Zipformer's activations, one expression for the GEMM epilogues
// ASR_EPI_BIAS_SWOOSHL / _SWOOSHR (dense.hip, dense_x3.hip) and for
// asr_glu_dwconv_fwd's ASR_GLU_ACT_SWOOSHR (glu_conv.hip), so the same
// pre-activation gives the same bits everywhere:
//   SwooshL(v) = log(1 + exp(v - 4)) - 0.08 v - 0.035
//   SwooshR(v) = log(1 + exp(v - 1)) - 0.08 v - 0.313261687
// For v - c > 20 the log term is v - c itself (exp(-20) is below half an ulp of
// 1 + it): v = +100 stays finite.  For v -> -inf exp underflows to 0, log1p(0) is
// 0 and the result is -0.08 v - const: never NaN or inf for a finite v.
#pragma once
#include <hip/hip_runtime.h>

namespace asr {

__device__ __forceinline__ float swoosh_f32(float v, float c, float k) {
    const float z = v - c;
    const float sp = z > 20.f ? z : log1pf(__expf(z));
    return (sp - 0.08f * v) - k;
}
__device__ __forceinline__ float swooshl_f32(float v) { return swoosh_f32(v, 4.f, 0.035f); }
__device__ __forceinline__ float swooshr_f32(float v) { return swoosh_f32(v, 1.f, 0.313261687f); }

}  // namespace asr
