// Region edits: the pointwise combine of nle_region_combine / nle_apply_regions (the rule is stated in include/nle.h).
// Per pixel the M spread stroke planes q_m become memberships alpha_0 .. alpha_M (alpha_0 the background), the memberships
// blend the rows of Wt ((M + 1) x L) into one weight per layer, and the L layer planes are summed under those weights:
//   u_m = q_m > 0 ? (double)q_m : 0;  sigma = u_1 + .. + u_M;  d = sigma > floor ? sigma : floor
//   alpha_m = u_m / d;  alpha_0 = 1 - sigma / d
//   w_l = alpha_0 Wt[0][l] + .. + alpha_M Wt[M][l];  y = w_0 (double)Y_0 + .. + w_{L-1} (double)Y_{L-1}
// in fp64, sums in ascending m and l, every operation rounded on its own (no fma): the numpy restatement of the tests is
// reproduced bit for bit.  Memory bound: L + M fp32 planes in, one plane out, nothing kept between pixels.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "nle.h"

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

__device__ __forceinline__ float sat8f(float v) {
    return fminf(255.f, fmaxf(0.f, rintf(v)));  // k_plane_to_u8's rule: round half to even, saturate
}

template <int P>
struct Pack;
template <>
struct Pack<1> {
    float v[1];
    __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
};
template <>
struct Pack<4> {
    float v[4];
    __device__ __forceinline__ void load(const float* p) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    }
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

template <int OUT>
__device__ __forceinline__ void region_store1(void* out, long long i, double y) {
    const float v = (float)y;
    if constexpr (OUT == NLE_REGION_OUT_F32) static_cast<float*>(out)[i] = v;
    else if constexpr (OUT == NLE_REGION_OUT_ROUNDED8) static_cast<float*>(out)[i] = sat8f(v);
    else static_cast<unsigned char*>(out)[i] = (unsigned char)(int)sat8f(v);
}

}  // namespace

// Four pixels per thread (16-byte loads, one 16-byte store, or one 4-byte store of four bytes) where every plane allows
// it; the last n mod 4 pixels, and everything when a base pointer or a plane stride breaks the alignment, go one pixel at a
// time, as in k_plane_to_u8.  Grid-stride.
template <int OUT>
__global__ __launch_bounds__(256) void k_region_combine(const RegionArgs a, void* __restrict__ out) {
    const long long n = a.n, n4 = n >> 2;
    const size_t out_mask = OUT == NLE_REGION_OUT_U8 ? 3 : 15;
    const bool vec = (((reinterpret_cast<size_t>(a.layers) | reinterpret_cast<size_t>(a.q)) & 15) |
                      (reinterpret_cast<size_t>(out) & out_mask) | (size_t)((a.layer_stride | a.q_stride) & 3)) == 0;
    const long long step = (long long)gridDim.x * 256;
    if (vec) {
        for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < n4; g += step) {
            double y[4];
            region_pixels<4>(a, g * 4, y);
            if constexpr (OUT == NLE_REGION_OUT_U8) {
                const unsigned r = (unsigned)(int)sat8f((float)y[0]) | ((unsigned)(int)sat8f((float)y[1]) << 8) |
                                   ((unsigned)(int)sat8f((float)y[2]) << 16) | ((unsigned)(int)sat8f((float)y[3]) << 24);
                static_cast<unsigned*>(out)[g] = r;
            } else {
                float4 r = make_float4((float)y[0], (float)y[1], (float)y[2], (float)y[3]);
                if constexpr (OUT == NLE_REGION_OUT_ROUNDED8) r = make_float4(sat8f(r.x), sat8f(r.y), sat8f(r.z), sat8f(r.w));
                static_cast<float4*>(out)[g] = r;
            }
        }
    }
    for (long long i = (vec ? n4 * 4 : 0) + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
        double y[1];
        region_pixels<1>(a, i, y);
        region_store1<OUT>(out, i, y[0]);
    }
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
    const unsigned grid = (unsigned)std::min<long long>((n / 4 + 255) / 256 + 1, 4096);  // plane_to_u8's cap
    switch (out_kind) {
        case NLE_REGION_OUT_F32:
            hipLaunchKernelGGL(k_region_combine<NLE_REGION_OUT_F32>, dim3(grid), dim3(256), 0, s, a, d_out);
            break;
        case NLE_REGION_OUT_ROUNDED8:
            hipLaunchKernelGGL(k_region_combine<NLE_REGION_OUT_ROUNDED8>, dim3(grid), dim3(256), 0, s, a, d_out);
            break;
        case NLE_REGION_OUT_U8:
            hipLaunchKernelGGL(k_region_combine<NLE_REGION_OUT_U8>, dim3(grid), dim3(256), 0, s, a, d_out);
            break;
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace nlek
