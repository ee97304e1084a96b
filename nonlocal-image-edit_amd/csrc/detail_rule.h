// The pieces of the detail rule and the tone rule (include/nle.h at nle_detail_combine / nle_tone_combine) that more than one
// kernel file states: the layer sum S, the gain curve g and the base tone curve.  detail.hip (one set of parameters per
// launch) and local.hip (one set per region row) both build their y from these, so a single row of the local rule is the
// detail / tone rule bit for bit.  Device only; the including file sets #pragma clang fp contract(off) before its own rule,
// and this header sets it for what it states.
#pragma once

#include <hip/hip_runtime.h>

#include "nle.h"
#include "plane_combine.h"

#pragma clang fp contract(off)

namespace nlek {

// g(d) with the curve on: d (1 + (gain - 1) exp(-(t t))), t = d / sigma
__device__ __forceinline__ double detail_remap(double sigma, double gain_m1, double d) {
    const double t = d / sigma;
    return d * (1.0 + gain_m1 * exp(-(t * t)));
}

// one step of S = ((Y_0 + Y_1) + ..) + Y_{L-1} on P pixels: layer l joins the sum.  The caller's loop over l is unrolled
// under its uniform guard l < L, so that l is a constant here
template <int P>
__device__ __forceinline__ void detail_sum_step(int l, const Pack<P>& Yl, double (&S)[P]) {
#pragma unroll
    for (int j = 0; j < P; ++j) S[j] = l == 0 ? (double)Yl.v[j] : S[j] + (double)Yl.v[j];
}

// the base term of the tone rule: the piecewise-linear curve through the knots T (in LDS), end segments continued linearly.
// A NaN Bw fails both comparisons: j = 0, f = NaN, B' = NaN.
struct ToneBase {
    const double* T;
    double lo, ks;
    __device__ __forceinline__ double operator()(double Bw) const {
        constexpr int N = NLE_TONE_KNOTS - 1;
        const double u = (Bw - lo) * ks;
        const int j = u >= 0.0 ? (u < (double)N ? (int)u : N - 1) : 0;
        const double f = u - (double)j;
        const double t0 = T[j], t1 = T[j + 1];
        return t0 + f * (t1 - t0);
    }
};

}  // namespace nlek
