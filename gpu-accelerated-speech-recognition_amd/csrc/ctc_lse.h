// The decoder's fp64 log-sum-exp routines, shared by the beam-search kernels
// (ctc_beam_kernel.inc) and the forced-alignment kernel (ctc_align.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace asr {

// log(exp(a) + exp(b)) = max + log1p(exp(-|a - b|)): the oracle's lse()
// formula (oracle/ctc_oracle.cpp, CTCBeamSearch.cpp:160's `+=` in the log
// domain), with exp and log1p evaluated by the two short fp64 routines below
// instead of the device library's general ones (~150 VALU per lse, a fifth of
// a decoder frame's VALU work).  Both are branch-free FMA
// chains: e = exp(-d) for d in [0, 746] (Cody-Waite reduction, degree-13
// Taylor on |r| <= ln2/2, exact ldexp), then log1p(e) for e in [0, 1] as
// log(u) of u = 1 + e (atanh series of s = (f - 1) / (f + 1), f = u or u / 2,
// |s| <= 0.172, ten terms) plus the rounding error of u divided by u.  Max
// error of log1p(exp(-d)) 3.2 ulp (glibc's 1.6) over 2e7 random d; the lse
// result equals glibc's bit for bit in 97.8 % of random pairs and is within
// one ulp otherwise (the parity tolerance is 1e-9 relative).  lse >= max
// holds exactly (the log1p term is >= 0), which the bound-based filters need.
__device__ __forceinline__ double lse_exp_neg(double x) {   // exp(x), x in [-746, 0]
    const double k = __builtin_rint(x * 1.4426950408889634074);
    double r = __builtin_fma(-k, 6.93147180369123816490e-01, x);
    r = __builtin_fma(-k, 1.90821492927058770002e-10, r);
    double p = 1.0 / 6227020800.0;
    p = __builtin_fma(p, r, 1.0 / 479001600.0);
    p = __builtin_fma(p, r, 1.0 / 39916800.0);
    p = __builtin_fma(p, r, 1.0 / 3628800.0);
    p = __builtin_fma(p, r, 1.0 / 362880.0);
    p = __builtin_fma(p, r, 1.0 / 40320.0);
    p = __builtin_fma(p, r, 1.0 / 5040.0);
    p = __builtin_fma(p, r, 1.0 / 720.0);
    p = __builtin_fma(p, r, 1.0 / 120.0);
    p = __builtin_fma(p, r, 1.0 / 24.0);
    p = __builtin_fma(p, r, 1.0 / 6.0);
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    return __builtin_ldexp(p, (int)k);
}
__device__ __forceinline__ double lse_log1p01(double e) {   // log1p(e), e in [0, 1]
    const double u = 1.0 + e;
    const double c = e - (u - 1.0);   // the rounding error of u, exact
    const bool hi = u > 1.4142135623730951;
    const double f = hi ? 0.5 * u : u;
    const double kk = hi ? 1.0 : 0.0;
    const double num = f - 1.0, den = f + 1.0;   // den in [1.7, 2.42]
    double y = __builtin_amdgcn_rcp(den);
    y = __builtin_fma(y, __builtin_fma(-den, y, 1.0), y);
    y = __builtin_fma(y, __builtin_fma(-den, y, 1.0), y);
    double q = num * y;
    q = __builtin_fma(__builtin_fma(-den, q, num), y, q);
    const double s2 = q * q;
    double P = 2.0 / 21.0;
    P = __builtin_fma(P, s2, 2.0 / 19.0);
    P = __builtin_fma(P, s2, 2.0 / 17.0);
    P = __builtin_fma(P, s2, 2.0 / 15.0);
    P = __builtin_fma(P, s2, 2.0 / 13.0);
    P = __builtin_fma(P, s2, 2.0 / 11.0);
    P = __builtin_fma(P, s2, 2.0 / 9.0);
    P = __builtin_fma(P, s2, 2.0 / 7.0);
    P = __builtin_fma(P, s2, 2.0 / 5.0);
    P = __builtin_fma(P, s2, 2.0 / 3.0);
    const double lf = __builtin_fma(q * s2, P, 2.0 * q);
    const double cu = c * __builtin_amdgcn_rcp(u);   // |c| <= 2^-53: the approximate reciprocal suffices
    return __builtin_fma(kk, 6.93147180369123816490e-01, lf + __builtin_fma(kk, 1.90821492927058770002e-10, cu));
}
__device__ __forceinline__ double lse2(double a, double b) {
    if (a == -INFINITY) return b;
    if (b == -INFINITY) return a;
    const double m = fmax(a, b);
#ifdef ASR_CTC_OCML_LSE   // A/B build: the device library's exp / log1p
    return m + log1p(exp(-fabs(a - b)));
#else
    return m + lse_log1p01(lse_exp_neg(-fabs(a - b)));
#endif
}

}  // namespace asr
