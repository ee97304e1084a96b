// The pieces of the detail rule and the tone rule (include/nle.h at nle_detail_combine / nle_tone_combine) that more than one
// kernel file states: the layer sum S, the gain curve g and the base tone curve.  detail.hip (one set of parameters per
// launch) and local.hip (one set per region row) both build their y from these, so a single row of the local rule is the
// detail / tone rule bit for bit.  Device only; the including file sets #pragma clang fp contract(off) before its own rule,
// and this header sets it for what it states.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels.h"
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

// nle_plane_histogram's counter of x under a scale (include/nle.h; k_plane_hist in tone.hip and k_region_hist in
// region_hist.hip): 0 the underflow, 1 + b bin b, kToneCounts - 1 the overflow and NaN
__device__ __forceinline__ int tone_bin(float x, double scale) {
    const double v = (double)x * scale;
    const double t = (v + 256.0) * 4.0;
    if (t != t) return kToneCounts - 1;
    if (t < 0.0) return 0;
    if (t >= (double)NLE_TONE_BINS) return kToneCounts - 1;
    return 1 + (int)t;  // t >= 0: the conversion truncates to the floor
}

// The memberships of nle_region_combine as the local rules use them (k_local_combine and k_local_chroma in local.hip,
// k_region_hist in region_hist.hip).  MMAX: the planes the kernel holds at most, M <= MMAX of them are read.
// the memberships' source planes of P pixels, as read, and what every row needs of them
template <int P, int MMAX = kRegionMax>
struct Memberships {
    Pack<P> q[MMAX];
    double d[P], a0[P];

    __device__ __forceinline__ void load(const float* base, long long stride, int M, long long i) {
#pragma unroll
        for (int m = 0; m < MMAX; ++m)
            if (m < M) q[m].load(base + (long long)m * stride + i);
    }
    // a NaN or non-positive q counts as 0 from here on; sigma, d and alpha_0 as region.hip forms them
    __device__ __forceinline__ void prepare(int M, double floor) {
        double sigma[P];
#pragma unroll
        for (int j = 0; j < P; ++j) sigma[j] = 0.0;
#pragma unroll
        for (int m = 0; m < MMAX; ++m) {
            if (m < M) {
#pragma unroll
                for (int j = 0; j < P; ++j) {
                    q[m].v[j] = q[m].v[j] > 0.f ? q[m].v[j] : 0.f;
                    sigma[j] = m == 0 ? (double)q[m].v[j] : sigma[j] + (double)q[m].v[j];
                }
            } else {
#pragma unroll
                for (int j = 0; j < P; ++j) q[m].v[j] = 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < P; ++j) {
            d[j] = sigma[j] > floor ? sigma[j] : floor;
            a0[j] = 1.0 - sigma[j] / d[j];
        }
    }
    // alpha_m of the P pixels for m = 0, 1, .. M, one call per row in that order; false when none of them is > 0 (the row
    // has no influence here).  Region m's plane is always read from q[0] and the planes move down one place behind it: every
    // index is a constant, so the planes stay in registers whatever m is (a pick by the uniform m would become an indexed
    // access to memory, that is scratch)
    __device__ __forceinline__ bool next_alpha(int m, double (&al)[P]) {
        bool any = false;
        if (m == 0) {
#pragma unroll
            for (int j = 0; j < P; ++j) al[j] = a0[j];
        } else {
#pragma unroll
            for (int j = 0; j < P; ++j) al[j] = (double)q[0].v[j] / d[j];
#pragma unroll
            for (int k = 0; k + 1 < MMAX; ++k) q[k] = q[k + 1];
        }
#pragma unroll
        for (int j = 0; j < P; ++j) any = any || al[j] > 0.0;
        return any;
    }
};

}  // namespace nlek
