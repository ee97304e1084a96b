// Region edits: the pointwise combine of nle_region_combine / nle_apply_regions (the rule is stated in include/nle.h).
// Per pixel the M spread stroke planes q_m become memberships alpha_0 .. alpha_M (alpha_0 the background), the memberships
// blend the rows of Wt ((M + 1) x L) into one weight per layer, and the L layer planes are summed under those weights:
//   u_m = q_m > 0 ? (double)q_m : 0;  sigma = u_1 + .. + u_M;  d = sigma > floor ? sigma : floor
//   alpha_m = u_m / d;  alpha_0 = 1 - sigma / d
//   w_l = alpha_0 Wt[0][l] + .. + alpha_M Wt[M][l];  y = w_0 (double)Y_0 + .. + w_{L-1} (double)Y_{L-1}
// in fp64, sums in ascending m and l, every operation rounded on its own (no fma): the numpy restatement of the tests is
// reproduced bit for bit.  Memory bound: L + M fp32 planes in, one plane out, nothing kept between pixels.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "nle.h"
#include "plane_combine.h"

// the rule fixes where every rounding happens: a contracted fma would round a product and a sum once instead of twice
#pragma clang fp contract(off)

namespace nlek {

namespace {

struct RegionArgs {
    const float* layers;
    const float* q;
    long long layer_stride, q_stride, n;
    int L, M;
    double floor;
    RegionWeights w;
};

// y of the P consecutive pixels from i on.  The loop over the regions is unrolled to kRegionMax under the uniform guard
// m < M, so that the memberships stay in registers (a runtime-indexed array would go to scratch); the loop over the layers
// is a runtime loop, its Wt entries uniform loads from the kernel arguments.
template <int P>
__device__ __forceinline__ void region_pixels(const RegionArgs& a, long long i, double (&y)[P]) {
    const int L = a.L, M = a.M;
    double al[kRegionMax][P], sigma[P];
#pragma unroll
    for (int j = 0; j < P; ++j) sigma[j] = 0.0;
#pragma unroll
    for (int m = 0; m < kRegionMax; ++m) {
        if (m < M) {
            Pack<P> q;
            q.load(a.q + (long long)m * a.q_stride + i);
#pragma unroll
            for (int j = 0; j < P; ++j) {
                al[m][j] = q.v[j] > 0.f ? (double)q.v[j] : 0.0;  // a NaN compares false: it counts as 0
                sigma[j] = m == 0 ? al[m][j] : sigma[j] + al[m][j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < P; ++j) al[m][j] = 0.0;
        }
    }
    double a0[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const double d = sigma[j] > a.floor ? sigma[j] : a.floor;
        a0[j] = 1.0 - sigma[j] / d;
#pragma unroll
        for (int m = 0; m < kRegionMax; ++m)
            if (m < M) al[m][j] = al[m][j] / d;
    }
    for (int l = 0; l < L; ++l) {
        Pack<P> Y;
        Y.load(a.layers + (long long)l * a.layer_stride + i);
        double w[P];
        const double w0 = a.w.wt[l];
#pragma unroll
        for (int j = 0; j < P; ++j) w[j] = a0[j] * w0;
#pragma unroll
        for (int m = 0; m < kRegionMax; ++m) {
            if (m < M) {
                const double wm = a.w.wt[(m + 1) * L + l];
#pragma unroll
                for (int j = 0; j < P; ++j) w[j] = w[j] + al[m][j] * wm;
            }
        }
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const double t = w[j] * (double)Y.v[j];
            y[j] = l == 0 ? t : y[j] + t;
        }
    }
}

}  // namespace

// plane_combine.h's skeleton over region_pixels; the 16-byte loads need both base pointers and both plane strides aligned
template <int OUT>
__global__ __launch_bounds__(256) void k_region_combine(const RegionArgs a, void* __restrict__ out) {
    const size_t misaligned = ((reinterpret_cast<size_t>(a.layers) | reinterpret_cast<size_t>(a.q)) & 15) |
                              (size_t)((a.layer_stride | a.q_stride) & 3);
    combine_planes<OUT>(a.n, misaligned, out, [&a](long long i, auto& y) { region_pixels(a, i, y); });
}

hipError_t region_combine(hipStream_t s, const float* d_layers, long long layer_stride, int L, const float* d_q,
                          long long q_stride, int M, long long n, const RegionWeights& wt, double floor, int out_kind,
                          void* d_out) {
    if (L < 1 || L > kRegionLayersMax || M < 1 || M > kRegionMax || n < 0 || layer_stride < 0 || q_stride < 0)
        return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    RegionArgs a;
    a.layers = d_layers;
    a.q = d_q;
    a.layer_stride = layer_stride;
    a.q_stride = q_stride;
    a.n = n;
    a.L = L;
    a.M = M;
    a.floor = floor;
    a.w = wt;
    return launch_for_out_kind(out_kind, [&](auto out) {
        hipLaunchKernelGGL(k_region_combine<decltype(out)::value>, dim3(combine_grid(n)), dim3(256), 0, s, a, d_out);
    });
}

}  // namespace nlek
