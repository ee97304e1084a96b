// The skeleton of the pointwise plane combines (k_region_combine, k_detail_combine): fp32 planes in, one plane of n pixels
// out in one of the three NLE_REGION_OUT_* kinds, a rule that gives the fp64 value of P consecutive pixels.
//   device   combine_planes<OUT>(n, misaligned, out, pixels): four pixels per thread (16-byte loads, one 16-byte store, or
//            one 4-byte store of four bytes) where every plane allows it; the last n mod 4 pixels, and everything when
//            something breaks the alignment, go one pixel at a time, as in k_plane_to_u8.  Grid-stride, 256 threads.
//   host     combine_grid(n), the grid that goes with it; launch_for_out_kind(out_kind, launch), the kernel's OUT from the
//            run-time kind.
// A kernel file keeps its argument struct, its rule `*_pixels<P>` (under its own #pragma clang fp contract(off)), the
// alignment bits of its inputs and its validation.  Nothing here knows which kernel it serves.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "nle.h"

namespace nlek {

__device__ __forceinline__ float sat8f(float v) {
    return fminf(255.f, fmaxf(0.f, rintf(v)));  // k_plane_to_u8's rule: round half to even, saturate
}

// P consecutive floats of a plane
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

// pixel i
template <int OUT>
__device__ __forceinline__ void store_pixels(void* out, long long i, const double (&y)[1]) {
    const float v = (float)y[0];
    if constexpr (OUT == NLE_REGION_OUT_F32) static_cast<float*>(out)[i] = v;
    else if constexpr (OUT == NLE_REGION_OUT_ROUNDED8) static_cast<float*>(out)[i] = sat8f(v);
    else static_cast<unsigned char*>(out)[i] = (unsigned char)(int)sat8f(v);
}

// the pixels 4 g .. 4 g + 3; out is aligned to their 16 (U8: 4) bytes
template <int OUT>
__device__ __forceinline__ void store_pixels(void* out, long long g, const double (&y)[4]) {
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

// The body of a combine kernel.  `misaligned`: non-zero when an input forbids the 16-byte loads (a base pointer's low four
// bits, the low two bits of a stride the rule uses); out's own alignment is looked at here.  `pixels(i, y)` fills
// double y[P] for the P pixels from i on, P = 4 or 1 taken from y's type.
template <int OUT, class Pixels>
__device__ __forceinline__ void combine_planes(long long n, size_t misaligned, void* out, const Pixels& pixels) {
    const long long n4 = n >> 2;
    const size_t out_mask = OUT == NLE_REGION_OUT_U8 ? 3 : 15;
    const bool vec = (misaligned | (reinterpret_cast<size_t>(out) & out_mask)) == 0;
    const long long step = (long long)gridDim.x * 256;
    if (vec) {
        for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < n4; g += step) {
            double y[4];
            pixels(g * 4, y);
            store_pixels<OUT>(out, g, y);
        }
    }
    for (long long i = (vec ? n4 * 4 : 0) + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
        double y[1];
        pixels(i, y);
        store_pixels<OUT>(out, i, y);
    }
}

// blocks of 256 threads for n pixels: one thread per group of four, capped (plane_to_u8's cap)
inline unsigned combine_grid(long long n) { return (unsigned)std::min<long long>((n / 4 + 255) / 256 + 1, 4096); }

// launch(std::integral_constant<int, OUT>) for the OUT that out_kind names; hipErrorInvalidValue, and no launch, for any other
template <class Launch>
hipError_t launch_for_out_kind(int out_kind, const Launch& launch) {
    switch (out_kind) {
        case NLE_REGION_OUT_F32:
            launch(std::integral_constant<int, NLE_REGION_OUT_F32>());
            break;
        case NLE_REGION_OUT_ROUNDED8:
            launch(std::integral_constant<int, NLE_REGION_OUT_ROUNDED8>());
            break;
        case NLE_REGION_OUT_U8:
            launch(std::integral_constant<int, NLE_REGION_OUT_U8>());
            break;
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace nlek
