// The row statistics of asr_layernorm_fwd as a device function: the one copy that
// layernorm_kernel (attention.hip: asr_layernorm_fwd, asr_layernorm_gelu_fwd) and the
// channel mode of asr_wave_conv_fwd (wave_conv.hip) call, so the same row gives the same
// bits in all three.
#pragma once
#include <hip/hip_runtime.h>

namespace asr {

__device__ __forceinline__ float ln_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// One wave, one row: lane l holds columns l, l + 64, ... in v[0 .. NU) (0 where the column is
// >= N).  Centres v in place and returns 1 / sqrt(var + eps) (two-pass, biased).
// mean = mean0 + corr: the residual mean of v - mean0 takes out mean0's own rounding error,
// which is relative to |v| (a row at 1000 +- 1 would otherwise be centred 5e-5 off).
template <int NU>
__device__ __forceinline__ float ln_row_centre(float (&v)[NU], int lane, int N, float eps) {
    float sum = 0.f;
#pragma unroll
    for (int u = 0; u < NU; u++) sum += v[u];
    const float mean0 = ln_wave_sum(sum) / (float)N;
    float rs = 0.f;
#pragma unroll
    for (int u = 0; u < NU; u++) {
        v[u] = (lane + 64 * u < N) ? v[u] - mean0 : 0.f;
        rs += v[u];
    }
    const float corr = ln_wave_sum(rs) / (float)N;
    float sq = 0.f;
#pragma unroll
    for (int u = 0; u < NU; u++) {
        v[u] = (lane + 64 * u < N) ? v[u] - corr : 0.f;
        sq += v[u] * v[u];
    }
    const float var = ln_wave_sum(sq) / (float)N;
    return 1.f / sqrtf(var + eps);
}

}  // namespace asr
