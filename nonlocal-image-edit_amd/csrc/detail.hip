// The out-of-span detail layer and the detail curve: the pointwise combine of nle_detail_combine / nle_apply_detail (the rule
// is stated in include/nle.h).  Per pixel, from the plane x and the L layer planes Y_0 .. Y_{L-1}:
//   S = ((Y_0 + Y_1) + ..) + Y_{L-1};  rho = x - S          what the K trained eigenvectors do not span
//   g(d) = d                                                 curve off (sigma == 0 or gain == 1: no exp is evaluated)
//   g(d) = d (1 + (gain - 1) exp(-(t t))),  t = d / sigma    curve on; gain - 1 comes from the host
//   y = w_rho g(rho) + w_0 g(Y_0) + .. + w_{L-2} g(Y_{L-2}) + w_{L-1} Y_{L-1}      (the base layer is never remapped)
// in fp64, the sums left to right, every operation rounded on its own (no fma): the numpy restatement of the tests is
// reproduced bit for bit with the curve off, and up to the last bit of exp with it on.  Memory bound: L + 1 fp32 planes in,
// one plane out, nothing kept between pixels.
// The base tone curve of nle_tone_combine / nle_apply_tone is the same rule with the last term replaced:
//   Bw = w_{L-1} Y_{L-1};  u = (Bw - lo) ks;  j = min(max(floor(u), 0), N - 1);  f = u - j;  B' = T_j + f (T_{j+1} - T_j)
// k_tone_combine is k_detail_combine with that term: one statement of the detail rule (detail_pixels), the base term a
// functor.  Its NLE_TONE_KNOTS knots come from a device buffer and are staged into LDS once per workgroup (8 KB).
#include <hip/hip_runtime.h>

#include "detail_rule.h"
#include "kernels.h"
#include "nle.h"
#include "plane_combine.h"

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

// the base term of the detail rule: w_{L-1} Y_{L-1} as it is
struct PlainBase {};

// g with the curve on, and ToneBase, the base term of the tone rule (the curve through the knots T in LDS), are stated in
// detail_rule.h, which local.hip shares
__device__ __forceinline__ double remap(const DetailArgs& a, double d) { return detail_remap(a.sigma, a.gain_m1, d); }

// y of the P consecutive pixels from i on.  rho needs every layer before the first term of y is formed, and each plane is
// read once: the loop over the layers is unrolled to LMAX >= L under the uniform guard l < L, so that the loaded values
// stay in registers (a runtime-indexed array would go to scratch) and all L + 1 loads are in flight together.  LMAX is 4 or
// kRegionLayersMax: the registers of sixteen layers would halve the occupancy of the usual four.
// CURVE is the uniform switch a.curve as a template argument: with the curve off no exp is in the instruction stream.
// Base: PlainBase, or the functor the last layer's weighted value passes (ToneBase).
template <int LMAX, bool CURVE, int P, class Base>
__device__ __forceinline__ void detail_pixels(const DetailArgs& a, long long i, double (&y)[P], const Base& base) {
    const int L = a.L;
    Pack<P> X, Y[LMAX];
    X.load(a.x + i);
#pragma unroll
    for (int l = 0; l < LMAX; ++l)
        if (l < L) Y[l].load(a.layers + (long long)l * a.layer_stride + i);
    double S[P];
#pragma unroll
    for (int l = 0; l < LMAX; ++l)
        if (l < L) detail_sum_step(l, Y[l], S);
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
                if constexpr (std::is_same_v<Base, PlainBase>) y[j] = y[j] + wl * (curved ? remap(a, d) : d);
                else y[j] = y[j] + (l < L - 1 ? wl * (curved ? remap(a, d) : d) : base(wl * d));
            }
        }
}

}  // namespace

// plane_combine.h's skeleton over detail_pixels; the 16-byte loads need both base pointers aligned, and the layer stride
// where a second layer is read
template <int OUT, int LMAX>
__global__ __launch_bounds__(256) void k_detail_combine(const DetailArgs a, void* __restrict__ out) {
    const size_t misaligned = ((reinterpret_cast<size_t>(a.layers) | reinterpret_cast<size_t>(a.x)) & 15) |
                              (size_t)(a.L > 1 ? a.layer_stride & 3 : 0);
    combine_planes<OUT>(a.n, misaligned, out, [&a](long long i, auto& y) {
        if (a.curve) detail_pixels<LMAX, true>(a, i, y, PlainBase());
        else detail_pixels<LMAX, false>(a, i, y, PlainBase());
    });
}

// the same over the tone rule: d_knots holds T_0 .. T_N
template <int OUT, int LMAX>
__global__ __launch_bounds__(256) void k_tone_combine(const DetailArgs a, const double* __restrict__ d_knots, double lo, double ks,
                                                      void* __restrict__ out) {
    __shared__ double sT[NLE_TONE_KNOTS];
    for (int k = threadIdx.x; k < NLE_TONE_KNOTS; k += 256) sT[k] = d_knots[k];
    __syncthreads();
    const ToneBase base{sT, lo, ks};
    const size_t misaligned = ((reinterpret_cast<size_t>(a.layers) | reinterpret_cast<size_t>(a.x)) & 15) |
                              (size_t)(a.L > 1 ? a.layer_stride & 3 : 0);
    combine_planes<OUT>(a.n, misaligned, out, [&a, &base](long long i, auto& y) {
        if (a.curve) detail_pixels<LMAX, true>(a, i, y, base);
        else detail_pixels<LMAX, false>(a, i, y, base);
    });
}

constexpr int kDetailFewLayers = 4;  // up to here the LMAX = 4 instantiation runs

namespace {
DetailArgs detail_args(const float* d_x, const float* d_layers, long long layer_stride, int L, long long n, const DetailWeights& w,
                       double w_rho, double gain, double sigma) {
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
    return a;
}
}  // namespace

hipError_t detail_combine(hipStream_t s, const float* d_x, const float* d_layers, long long layer_stride, int L, long long n,
                          const DetailWeights& w, double w_rho, double gain, double sigma, int out_kind, void* d_out) {
    if (L < 1 || L > kRegionLayersMax || n < 0 || layer_stride < 0) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const DetailArgs a = detail_args(d_x, d_layers, layer_stride, L, n, w, w_rho, gain, sigma);
    return launch_for_out_kind(out_kind, [&](auto out) {
        constexpr int OUT = decltype(out)::value;
        if (L <= kDetailFewLayers)
            hipLaunchKernelGGL((k_detail_combine<OUT, kDetailFewLayers>), dim3(combine_grid(n)), dim3(256), 0, s, a, d_out);
        else hipLaunchKernelGGL((k_detail_combine<OUT, kRegionLayersMax>), dim3(combine_grid(n)), dim3(256), 0, s, a, d_out);
    });
}

hipError_t tone_combine(hipStream_t s, const float* d_x, const float* d_layers, long long layer_stride, int L, long long n,
                        const DetailWeights& w, double w_rho, double gain, double sigma, const double* d_knots, double lo, double ks,
                        int out_kind, void* d_out) {
    if (L < 1 || L > kRegionLayersMax || n < 0 || layer_stride < 0 || !d_knots) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const DetailArgs a = detail_args(d_x, d_layers, layer_stride, L, n, w, w_rho, gain, sigma);
    return launch_for_out_kind(out_kind, [&](auto out) {
        constexpr int OUT = decltype(out)::value;
        if (L <= kDetailFewLayers)
            hipLaunchKernelGGL((k_tone_combine<OUT, kDetailFewLayers>), dim3(combine_grid(n)), dim3(256), 0, s, a, d_knots, lo, ks, d_out);
        else hipLaunchKernelGGL((k_tone_combine<OUT, kRegionLayersMax>), dim3(combine_grid(n)), dim3(256), 0, s, a, d_knots, lo, ks, d_out);
    });
}

}  // namespace nlek
