// 16-bit sRGB <-> float Lab on the device: the deep-colour wrapper either side of the hot path (new here: the reference is
// 8-bit only, so DESIGN.md section 3.13 is the definition).  Both directions are fp64 per pixel, every operation rounded
// on its own and in the order written (no contraction in this file), from the host's tables (srgb16_tables.cpp): a test
// restates them in numpy from the same numbers.  lin is 512 KB, the threshold pairs 1 MB -- gathers that an XCD's L2 holds,
// not LDS.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "srgb16.h"

#pragma clang fp contract(off)

#include "srgb16_device.h"  // code_of: the threshold search, shared with tonemap.hip

namespace nlek {

namespace {

// f(t) of L*a*b*
__device__ __forceinline__ double lab_f(double t) {
    if (t > 216.0 / 24389.0) return cbrt(t);
    return ((24389.0 / 27.0) * t + 16.0) / 116.0;
}

// its inverse
__device__ __forceinline__ double lab_finv(double f) {
    if (f > 6.0 / 29.0) return (f * f) * f;
    return ((116.0 * f - 16.0) * 27.0) / 24389.0;
}

// one pixel of the forward direction: codes -> L, a, b rounded once to fp32 and the guide (m: rows X, Y, Z of the matrix)
struct Lab16 {
    float L, a, b, guide;
};
__device__ __forceinline__ Lab16 to_lab(unsigned cb, unsigned cg, unsigned cr, const double* __restrict__ lin, const double (&m)[9],
                                        bool want_a, bool want_b) {
    const double B = lin[cb], G = lin[cg], R = lin[cr];
    const double fy = lab_f((m[3] * R + m[4] * G) + m[5] * B);
    const double L = ((116.0 * fy - 16.0) * 255.0) / 100.0;
    Lab16 o;
    o.L = (float)L;
    o.guide = (float)fmin(255.0, fmax(0.0, rint(L)));
    o.a = want_a ? (float)(500.0 * (lab_f((m[0] * R + m[1] * G) + m[2] * B) - fy) + 128.0) : 0.f;
    o.b = want_b ? (float)(200.0 * (fy - lab_f((m[6] * R + m[7] * G) + m[8] * B)) + 128.0) : 0.f;
    return o;
}

// one pixel of the inverse direction: the codes of B, G and R (m: rows R, G, B of the inverse matrix)
__device__ __forceinline__ void to_codes(float Lf, float af, float bf, const double2* __restrict__ pairs, const double (&m)[9],
                                         unsigned* cb, unsigned* cg, unsigned* cr) {
    const double Lr = (double)Lf;
    const double L = Lr > 0.0 ? (Lr < 255.0 ? Lr : 255.0) : 0.0;
    const double fy = ((L * 100.0) / 255.0 + 16.0) / 116.0;
    const double fx = fy + ((double)af - 128.0) / 500.0;
    const double fz = fy - ((double)bf - 128.0) / 200.0;
    const double X = lab_finv(fx), Y = lab_finv(fy), Z = lab_finv(fz);
    *cb = (unsigned)code_of((m[6] * X + m[7] * Y) + m[8] * Z, pairs);
    *cg = (unsigned)code_of((m[3] * X + m[4] * Y) + m[5] * Z, pairs);
    *cr = (unsigned)code_of((m[0] * X + m[1] * Y) + m[2] * Z, pairs);
}

}  // namespace

// interleaved BGR uint16 -> L, a, b on the 8-bit path's scales (L in [0, 255], a and b around 128), each rounded once to
// fp32, and the guide: round-half-even of the fp64 L, clamped to [0, 255].  a, b and guide may each be NULL.  A thread
// takes two neighbouring pixels -- twelve bytes in one load, eight out per plane -- where the pointers allow it (the image
// 4-byte, the planes 8-byte aligned), and single pixels otherwise and for an odd last one: per-lane 2-byte accesses at a
// 6-byte stride cost the memory pipeline as much as the table gathers.
__global__ __launch_bounds__(256) void k_bgr16_to_lab(const unsigned short* __restrict__ bgr, long long n,
                                                      const double* __restrict__ tab, float* __restrict__ Lo,
                                                      float* __restrict__ ao, float* __restrict__ bo,
                                                      float* __restrict__ guide) {
    const double* __restrict__ lin = tab + nlesrgb16::kOffLin;
    double m[9];
    for (int k = 0; k < 9; ++k) m[k] = tab[nlesrgb16::kOffCoeffs + k];
    const bool wa = ao != nullptr, wb = bo != nullptr;
    const size_t planes = reinterpret_cast<size_t>(Lo) | reinterpret_cast<size_t>(ao) | reinterpret_cast<size_t>(bo) |
                          reinterpret_cast<size_t>(guide);
    const long long npair = ((reinterpret_cast<size_t>(bgr) & 3) | (planes & 7)) == 0 ? n / 2 : 0;
    const long long t0 = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
    for (long long p = t0; p < npair; p += stride) {
        const uint3 w = reinterpret_cast<const uint3*>(bgr)[p];
        const Lab16 u = to_lab(w.x & 0xffffu, w.x >> 16, w.y & 0xffffu, lin, m, wa, wb);
        const Lab16 v = to_lab(w.y >> 16, w.z & 0xffffu, w.z >> 16, lin, m, wa, wb);
        reinterpret_cast<float2*>(Lo)[p] = make_float2(u.L, v.L);
        if (guide != nullptr) reinterpret_cast<float2*>(guide)[p] = make_float2(u.guide, v.guide);
        if (wa) reinterpret_cast<float2*>(ao)[p] = make_float2(u.a, v.a);
        if (wb) reinterpret_cast<float2*>(bo)[p] = make_float2(u.b, v.b);
    }
    for (long long i = 2 * npair + t0; i < n; i += stride) {
        const Lab16 u = to_lab(bgr[3 * i + 0], bgr[3 * i + 1], bgr[3 * i + 2], lin, m, wa, wb);
        Lo[i] = u.L;
        if (guide != nullptr) guide[i] = u.guide;
        if (wa) ao[i] = u.a;
        if (wb) bo[i] = u.b;
    }
}

// L' (clamped to [0, 255]; a NaN counts as 0), a, b (not clamped) -> interleaved BGR uint16.  Out-of-gamut values
// saturate at 0 and 65535 through thr itself.  Two pixels per thread where the pointers allow it, as above.
__global__ __launch_bounds__(256) void k_lab_to_bgr16(const float* __restrict__ Li, const float* __restrict__ ai,
                                                      const float* __restrict__ bi, long long n,
                                                      const double* __restrict__ tab, unsigned short* __restrict__ bgr) {
    const double2* __restrict__ pairs = reinterpret_cast<const double2*>(tab + nlesrgb16::kOffPairs);
    double m[9];
    for (int k = 0; k < 9; ++k) m[k] = tab[nlesrgb16::kOffCoeffs + 9 + k];
    const size_t planes = reinterpret_cast<size_t>(Li) | reinterpret_cast<size_t>(ai) | reinterpret_cast<size_t>(bi);
    const long long npair = ((reinterpret_cast<size_t>(bgr) & 3) | (planes & 7)) == 0 ? n / 2 : 0;
    const long long t0 = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
    for (long long p = t0; p < npair; p += stride) {
        const float2 L = reinterpret_cast<const float2*>(Li)[p], a = reinterpret_cast<const float2*>(ai)[p],
                     b = reinterpret_cast<const float2*>(bi)[p];
        unsigned b0, g0, r0, b1, g1, r1;
        to_codes(L.x, a.x, b.x, pairs, m, &b0, &g0, &r0);
        to_codes(L.y, a.y, b.y, pairs, m, &b1, &g1, &r1);
        reinterpret_cast<uint3*>(bgr)[p] = make_uint3(b0 | (g0 << 16), r0 | (b1 << 16), g1 | (r1 << 16));
    }
    for (long long i = 2 * npair + t0; i < n; i += stride) {
        unsigned cb, cg, cr;
        to_codes(Li[i], ai[i], bi[i], pairs, m, &cb, &cg, &cr);
        bgr[3 * i + 0] = (unsigned short)cb;
        bgr[3 * i + 1] = (unsigned short)cg;
        bgr[3 * i + 2] = (unsigned short)cr;
    }
}

// 2048 blocks of 256 threads are one full residency (8 per CU); a sweep of the pair loop covers 2^20 pixels
hipError_t bgr16_to_lab(hipStream_t s, const unsigned short* d_bgr, long long n, const double* d_tab, float* d_L,
                        float* d_a, float* d_b, float* d_guide) {
    if (n <= 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<long long>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(k_bgr16_to_lab, dim3(grid), dim3(256), 0, s, d_bgr, n, d_tab, d_L, d_a, d_b, d_guide);
    return hipGetLastError();
}

hipError_t lab_to_bgr16(hipStream_t s, const float* d_L, const float* d_a, const float* d_b, long long n,
                        const double* d_tab, unsigned short* d_bgr) {
    if (n <= 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<long long>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(k_lab_to_bgr16, dim3(grid), dim3(256), 0, s, d_L, d_a, d_b, n, d_tab, d_bgr);
    return hipGetLastError();
}

}  // namespace nlek
