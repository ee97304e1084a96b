// HDR tone mapping on the device: the colour ends for linear-light float input either side of the hot path (new here: the
// reference is 8-bit only, so DESIGN.md section 3.14 is the definition).  A range pass finds the largest and the smallest
// positive finite luminance, the forward kernel writes the log-luminance plane on the scale of an 8-bit L plane and its
// 256-level guide, the inverse kernel turns the filtered plane and the original colours into 16-bit sRGB codes.  All of it
// is fp64 per pixel, every operation rounded on its own and in the order written (no contraction in this file): a test
// restates it in numpy.  The encoder is the deep-colour one (srgb16_device.h) on the same per-ctx threshold pairs.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "srgb16.h"

#pragma clang fp contract(off)

#include "srgb16_device.h"

namespace nlek {

namespace {

constexpr int kHdrMaxBlocks = 2048;  // one full residency of 256-thread blocks (8 per CU), as in colour16.hip

// the luminance of linear-light B, G, R: the Y row of the matrix section 3.13 uses, not renormalised
__device__ __forceinline__ double lum(float b, float g, float r) {
    return (0.212671 * (double)r + 0.715160 * (double)g) + 0.072169 * (double)b;
}

// the largest and the smallest admissible luminance seen so far: admissible is finite and > 0 (a NaN fails both tests).
// mx = 0 and mn = +inf stand for "none yet"
struct Range {
    double mx, mn;
};
__device__ __forceinline__ void take(Range& r, double Y) {
    if (Y > 0.0 && Y < __builtin_huge_val()) {
        r.mx = fmax(r.mx, Y);
        r.mn = fmin(r.mn, Y);
    }
}

// the block's range in thread 0: the waves on the shuffle network, then the four waves' values in a fixed order (max and min
// do not depend on the order anyway)
__device__ __forceinline__ Range block_range(Range r) {
    __shared__ double s_mx[4], s_mn[4];
    for (int off = 32; off > 0; off >>= 1) {
        r.mx = fmax(r.mx, __shfl_xor(r.mx, off));
        r.mn = fmin(r.mn, __shfl_xor(r.mn, off));
    }
    if ((threadIdx.x & 63) == 0) {
        s_mx[threadIdx.x >> 6] = r.mx;
        s_mn[threadIdx.x >> 6] = r.mn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        r.mx = fmax(fmax(s_mx[0], s_mx[1]), fmax(s_mx[2], s_mx[3]));
        r.mn = fmin(fmin(s_mn[0], s_mn[1]), fmin(s_mn[2], s_mn[3]));
    }
    return r;
}

// one pixel of the forward direction: x = 255 ((log2 Y - l_hi) / R) + 255 clamped into [0, 255] -- the clamp of Y into
// [2^(l_hi - R), 2^l_hi], taken where it is exact -- and the guide.  Y <= 0, -inf and NaN are the floor, +inf the ceiling.
struct LogLum {
    float x, guide;
};
__device__ __forceinline__ LogLum to_loglum(float b, float g, float r, double l_hi, double range) {
    const double Y = lum(b, g, r);
    double x = 0.0;
    if (Y > 0.0) {
        x = 255.0 * ((log2(Y) - l_hi) / range) + 255.0;
        x = x > 0.0 ? (x < 255.0 ? x : 255.0) : 0.0;
    }
    LogLum o;
    o.x = (float)x;
    o.guide = (float)rint(x);
    return o;
}

// the constants of one inverse call, made once on the host
struct Inverse {
    double range, white, sat, y_lo, y_hi;  // white = 255 c; [y_lo, y_hi] = [2^(l_hi - R), 2^l_hi]
};

// one pixel of the inverse direction: the codes of B, G and R
__device__ __forceinline__ void to_codes(float yf, float b, float g, float r, const Inverse& k,
                                         const double2* __restrict__ pairs, unsigned* cb, unsigned* cg, unsigned* cr) {
    const double y = (double)yf;
    const double Yout = y == y ? exp2(((y - k.white) * k.range) / 255.0) : 0.0;
    const double Y = lum(b, g, r);
    const double Yin = Y > k.y_lo ? (Y < k.y_hi ? Y : k.y_hi) : k.y_lo;  // a NaN counts as the floor
    const double rb = (b > 0.f ? (double)b : 0.0) / Yin, rg = (g > 0.f ? (double)g : 0.0) / Yin,
                 rr = (r > 0.f ? (double)r : 0.0) / Yin;  // a NaN channel counts as 0
    const bool plain = k.sat == 1.0;
    *cb = (unsigned)code_of((plain ? rb : pow(rb, k.sat)) * Yout, pairs);
    *cg = (unsigned)code_of((plain ? rg : pow(rg, k.sat)) * Yout, pairs);
    *cr = (unsigned)code_of((plain ? rr : pow(rr, k.sat)) * Yout, pairs);
}

}  // namespace

// interleaved BGR fp32 -> one (max, min) pair of the admissible luminances per block.  A thread takes two neighbouring
// pixels -- 24 bytes in three 8-byte loads -- where the image is 8-byte aligned, single pixels otherwise and for an odd
// last one.  No atomics: the second stage below reads the pairs in a fixed order.
__global__ __launch_bounds__(256) void k_hdr_range(const float* __restrict__ bgr, long long n, double* __restrict__ partial) {
    Range r{0.0, __builtin_huge_val()};
    const long long npair = (reinterpret_cast<size_t>(bgr) & 7) == 0 ? n / 2 : 0;
    const long long t0 = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
    for (long long p = t0; p < npair; p += stride) {
        const float2* q = reinterpret_cast<const float2*>(bgr) + 3 * p;
        const float2 u = q[0], v = q[1], w = q[2];
        take(r, lum(u.x, u.y, v.x));
        take(r, lum(v.y, w.x, w.y));
    }
    for (long long i = 2 * npair + t0; i < n; i += stride) take(r, lum(bgr[3 * i + 0], bgr[3 * i + 1], bgr[3 * i + 2]));
    r = block_range(r);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x + 0] = r.mx;
        partial[2 * blockIdx.x + 1] = r.mn;
    }
}

// the nb pairs of the first stage -> out[0] = Ymax (0: no admissible pixel), out[1] = Ymin+; one block
__global__ __launch_bounds__(256) void k_hdr_range_final(const double* __restrict__ partial, int nb, double* __restrict__ out) {
    Range r{0.0, __builtin_huge_val()};
    for (int b = threadIdx.x; b < nb; b += 256) {
        r.mx = fmax(r.mx, partial[2 * b + 0]);
        r.mn = fmin(r.mn, partial[2 * b + 1]);
    }
    r = block_range(r);
    if (threadIdx.x == 0) {
        out[0] = r.mx;
        out[1] = r.mn;
    }
}

// interleaved BGR fp32 -> x (fp32, unrounded) and the guide (x rounded half to even: the integer plane a train takes).
// Either output may be NULL.  Two pixels per thread where the image and the planes are 8-byte aligned, as above.
__global__ __launch_bounds__(256) void k_hdr_to_loglum(const float* __restrict__ bgr, long long n, double l_hi, double range,
                                                       float* __restrict__ xo, float* __restrict__ guide) {
    const size_t align = reinterpret_cast<size_t>(bgr) | reinterpret_cast<size_t>(xo) | reinterpret_cast<size_t>(guide);
    const long long npair = (align & 7) == 0 ? n / 2 : 0;
    const long long t0 = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
    for (long long p = t0; p < npair; p += stride) {
        const float2* q = reinterpret_cast<const float2*>(bgr) + 3 * p;
        const float2 u = q[0], v = q[1], w = q[2];
        const LogLum a = to_loglum(u.x, u.y, v.x, l_hi, range), b = to_loglum(v.y, w.x, w.y, l_hi, range);
        if (xo != nullptr) reinterpret_cast<float2*>(xo)[p] = make_float2(a.x, b.x);
        if (guide != nullptr) reinterpret_cast<float2*>(guide)[p] = make_float2(a.guide, b.guide);
    }
    for (long long i = 2 * npair + t0; i < n; i += stride) {
        const LogLum a = to_loglum(bgr[3 * i + 0], bgr[3 * i + 1], bgr[3 * i + 2], l_hi, range);
        if (xo != nullptr) xo[i] = a.x;
        if (guide != nullptr) guide[i] = a.guide;
    }
}

// the filtered plane y and the original colours -> interleaved BGR uint16: Yout = 2^((y - 255 c) R / 255) (a NaN y gives 0),
// every channel max(C, 0) / Yin (to the power s unless s = 1) times Yout, encoded through the threshold pairs, which
// saturate at 0 and 65535.  Two pixels per thread where y and the image are 8-byte and the output is 4-byte aligned.
__global__ __launch_bounds__(256) void k_loglum_to_bgr16(const float* __restrict__ yi, const float* __restrict__ bgr, long long n,
                                                         Inverse k, const double* __restrict__ tab,
                                                         unsigned short* __restrict__ out) {
    const double2* __restrict__ pairs = reinterpret_cast<const double2*>(tab + nlesrgb16::kOffPairs);
    const size_t align = ((reinterpret_cast<size_t>(yi) | reinterpret_cast<size_t>(bgr)) & 7) | (reinterpret_cast<size_t>(out) & 3);
    const long long npair = align == 0 ? n / 2 : 0;
    const long long t0 = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
    for (long long p = t0; p < npair; p += stride) {
        const float2* q = reinterpret_cast<const float2*>(bgr) + 3 * p;
        const float2 u = q[0], v = q[1], w = q[2], y = reinterpret_cast<const float2*>(yi)[p];
        unsigned b0, g0, r0, b1, g1, r1;
        to_codes(y.x, u.x, u.y, v.x, k, pairs, &b0, &g0, &r0);
        to_codes(y.y, v.y, w.x, w.y, k, pairs, &b1, &g1, &r1);
        reinterpret_cast<uint3*>(out)[p] = make_uint3(b0 | (g0 << 16), r0 | (b1 << 16), g1 | (r1 << 16));
    }
    for (long long i = 2 * npair + t0; i < n; i += stride) {
        unsigned cb, cg, cr;
        to_codes(yi[i], bgr[3 * i + 0], bgr[3 * i + 1], bgr[3 * i + 2], k, pairs, &cb, &cg, &cr);
        out[3 * i + 0] = (unsigned short)cb;
        out[3 * i + 1] = (unsigned short)cg;
        out[3 * i + 2] = (unsigned short)cr;
    }
}

int hdr_range_blocks(long long n) { return (int)std::max<long long>(1, std::min<long long>((n + 511) / 512, kHdrMaxBlocks)); }

hipError_t hdr_range(hipStream_t s, const float* d_bgr, long long n, double* d_partial, double* d_pair) {
    const int nb = hdr_range_blocks(n);
    hipLaunchKernelGGL(k_hdr_range, dim3(nb), dim3(256), 0, s, d_bgr, n, d_partial);
    hipLaunchKernelGGL(k_hdr_range_final, dim3(1), dim3(256), 0, s, d_partial, nb, d_pair);
    return hipGetLastError();
}

hipError_t hdr_to_loglum(hipStream_t s, const float* d_bgr, long long n, double l_hi, double range, float* d_x, float* d_guide) {
    if (n <= 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<long long>((n + 255) / 256, kHdrMaxBlocks);
    hipLaunchKernelGGL(k_hdr_to_loglum, dim3(grid), dim3(256), 0, s, d_bgr, n, l_hi, range, d_x, d_guide);
    return hipGetLastError();
}

hipError_t loglum_to_bgr16(hipStream_t s, const float* d_y, const float* d_bgr, long long n, double range, double white,
                           double saturation, double y_lo, double y_hi, const double* d_tab, unsigned short* d_bgr16) {
    if (n <= 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<long long>((n + 255) / 256, kHdrMaxBlocks);
    hipLaunchKernelGGL(k_loglum_to_bgr16, dim3(grid), dim3(256), 0, s, d_y, d_bgr, n, Inverse{range, white, saturation, y_lo, y_hi},
                       d_tab, d_bgr16);
    return hipGetLastError();
}

}  // namespace nlek
