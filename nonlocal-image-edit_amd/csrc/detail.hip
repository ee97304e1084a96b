// The out-of-span detail layer and the detail curve: the pointwise combine of nle_detail_combine / nle_apply_detail (the rule
// is stated in include/nle.h).  Per pixel, from the plane x and the L layer planes Y_0 .. Y_{L-1}:
//   S = ((Y_0 + Y_1) + ..) + Y_{L-1};  rho = x - S          what the K trained eigenvectors do not span
//   g(d) = d                                                 curve off (sigma == 0 or gain == 1: no exp is evaluated)
//   g(d) = d (1 + (gain - 1) exp(-(t t))),  t = d / sigma    curve on; gain - 1 comes from the host
//   y = w_rho g(rho) + w_0 g(Y_0) + .. + w_{L-2} g(Y_{L-2}) + w_{L-1} Y_{L-1}      (the base layer is never remapped)
// in fp64, the sums left to right, every operation rounded on its own (no fma): the numpy restatement of the tests is
// reproduced bit for bit with the curve off, and up to the last bit of exp with it on.  Memory bound: L + 1 fp32 planes in,
// one plane out, nothing kept between pixels.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "nle.h"

// the rule fixes where every rounding happens: a contracted fma would round a product and a sum once instead of twice
#pragma clang fp contract(off)

namespace nlek {

namespace {

struct DetailArgs {
    const float* x;
    const float* layers;
    long long layer_stride, n;
    int L, curve;  // curve != 0: sigma > 0 and gain != 1
    double w_rho, gain_m1, sigma;
    DetailWeights w;
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

__device__ __forceinline__ double remap(const DetailArgs& a, double d) {
    const double t = d / a.sigma;
    return d * (1.0 + a.gain_m1 * exp(-(t * t)));
}

// y of the P consecutive pixels from i on.  rho needs every layer before the first term of y is formed, and each plane is
// read once: the loop over the layers is unrolled to LMAX >= L under the uniform guard l < L, so that the loaded values
// stay in registers (a runtime-indexed array would go to scratch) and all L + 1 loads are in flight together.  LMAX is 4 or
// kRegionLayersMax: the registers of sixteen layers would halve the occupancy of the usual four.
// CURVE is the uniform switch a.curve as a template argument: with the curve off no exp is in the instruction stream.
template <int P, int LMAX, bool CURVE>
__device__ __forceinline__ void detail_pixels(const DetailArgs& a, long long i, double (&y)[P]) {
    const int L = a.L;
    Pack<P> X, Y[LMAX];
    X.load(a.x + i);
#pragma unroll
    for (int l = 0; l < LMAX; ++l)
        if (l < L) Y[l].load(a.layers + (long long)l * a.layer_stride + i);
    double S[P];
#pragma unroll
    for (int l = 0; l < LMAX; ++l)
        if (l < L) {
#pragma unroll
            for (int j = 0; j < P; ++j) S[j] = l == 0 ? (double)Y[l].v[j] : S[j] + (double)Y[l].v[j];
        }
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const double rho = (double)X.v[j] - S[j];
        y[j] = a.w_rho * (CURVE ? remap(a, rho) : rho);
    }
#pragma unroll
    for (int l = 0; l < LMAX; ++l)
        if (l < L) {
            const double wl = a.w.w[l];
            const bool curved = CURVE && l < L - 1;  // uniform
#pragma unroll
            for (int j = 0; j < P; ++j) {
                const double d = (double)Y[l].v[j];
                y[j] = y[j] + wl * (curved ? remap(a, d) : d);
            }
        }
}

template <int OUT>
__device__ __forceinline__ void detail_store1(void* out, long long i, double y) {
    const float v = (float)y;
    if constexpr (OUT == NLE_REGION_OUT_F32) static_cast<float*>(out)[i] = v;
    else if constexpr (OUT == NLE_REGION_OUT_ROUNDED8) static_cast<float*>(out)[i] = sat8f(v);
    else static_cast<unsigned char*>(out)[i] = (unsigned char)(int)sat8f(v);
}

}  // namespace

// Four pixels per thread (16-byte loads, one 16-byte store, or one 4-byte store of four bytes) where every plane allows
// it; the last n mod 4 pixels, and everything when a base pointer or the layer stride breaks the alignment, go one pixel at
// a time, as in k_region_combine.  Grid-stride.
template <int OUT, int LMAX>
__global__ __launch_bounds__(256) void k_detail_combine(const DetailArgs a, void* __restrict__ out) {
    const long long n = a.n, n4 = n >> 2;
    const size_t out_mask = OUT == NLE_REGION_OUT_U8 ? 3 : 15;
    const bool vec = (((reinterpret_cast<size_t>(a.layers) | reinterpret_cast<size_t>(a.x)) & 15) |
                      (reinterpret_cast<size_t>(out) & out_mask) | (size_t)(a.L > 1 ? a.layer_stride & 3 : 0)) == 0;
    const long long step = (long long)gridDim.x * 256;
    if (vec) {
        for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < n4; g += step) {
            double y[4];
            if (a.curve) detail_pixels<4, LMAX, true>(a, g * 4, y);
            else detail_pixels<4, LMAX, false>(a, g * 4, y);
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
        if (a.curve) detail_pixels<1, LMAX, true>(a, i, y);
        else detail_pixels<1, LMAX, false>(a, i, y);
        detail_store1<OUT>(out, i, y[0]);
    }
}

namespace {

constexpr int kDetailFewLayers = 4;  // up to here the LMAX = 4 instantiation runs

template <int OUT>
void detail_launch(bool few, unsigned grid, hipStream_t s, const DetailArgs& a, void* d_out) {
    if (few) hipLaunchKernelGGL((k_detail_combine<OUT, kDetailFewLayers>), dim3(grid), dim3(256), 0, s, a, d_out);
    else hipLaunchKernelGGL((k_detail_combine<OUT, kRegionLayersMax>), dim3(grid), dim3(256), 0, s, a, d_out);
}

}  // namespace

hipError_t detail_combine(hipStream_t s, const float* d_x, const float* d_layers, long long layer_stride, int L, long long n,
                          const DetailWeights& w, double w_rho, double gain, double sigma, int out_kind, void* d_out) {
    if (L < 1 || L > kRegionLayersMax || n < 0 || layer_stride < 0) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    DetailArgs a;
    a.x = d_x;
    a.layers = d_layers;
    a.layer_stride = layer_stride;
    a.n = n;
    a.L = L;
    a.curve = sigma != 0.0 && gain != 1.0;
    a.w_rho = w_rho;
    a.gain_m1 = gain - 1.0;
    a.sigma = sigma;
    a.w = w;
    const unsigned grid = (unsigned)std::min<long long>((n / 4 + 255) / 256 + 1, 4096);  // k_region_combine's cap
    const bool few = L <= kDetailFewLayers;
    switch (out_kind) {
        case NLE_REGION_OUT_F32:
            detail_launch<NLE_REGION_OUT_F32>(few, grid, s, a, d_out);
            break;
        case NLE_REGION_OUT_ROUNDED8:
            detail_launch<NLE_REGION_OUT_ROUNDED8>(few, grid, s, a, d_out);
            break;
        case NLE_REGION_OUT_U8:
            detail_launch<NLE_REGION_OUT_U8>(few, grid, s, a, d_out);
            break;
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace nlek
