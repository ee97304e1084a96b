// The base tone curve's own pieces (include/nle.h "base tone curve"): the histogram of a scaled fp32
// plane (k_plane_hist) and the host rule that turns its counts and four numbers into the knots of a curve (tone_curve).  The
// curve's term in the pointwise combine lives with the detail rule it extends, in detail.hip.
//   v = (double)x scale;  t = (v + 256) 4;  NaN -> counts[4097], t < 0 -> counts[0], t >= 4096 -> counts[4097], else
//   counts[1 + floor(t)]: NLE_TONE_BINS bins of a quarter level over [-256, 768), integer counts -- exact in any order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "detail_rule.h"
#include "kernels.h"
#include "nle.h"

// the rules fix where every rounding happens (x scale + 256 must not become one fma; the host rule is restated by a test)
#pragma clang fp contract(off)

namespace nlek {

namespace {

constexpr int kHistThreads = 512, kHistMaxBlocks = 1024;

// One pixel per lane, b < 0 for a lane without one.  Every lane of the wave calls this together.  A run of lanes with the same
// bin is counted once, by its first lane, with the run's length: a flat region costs one LDS atomic per wave instead of 64
// serialised ones on one address (the idea of wave_group_levels in tables.hip; integer counts need no fixed order, so the
// runs of neighbours are enough and no search for equal levels further apart is made).
__device__ __forceinline__ void count_run(unsigned* sh, int b) {
    const int lane = (int)(threadIdx.x & 63);
    const int prev = __shfl_up(b, 1);
    const bool head = lane == 0 || prev != b;
    const unsigned long long heads = __ballot(head);
    if (head && b >= 0) {
        const unsigned long long rest = lane == 63 ? 0ull : heads >> (lane + 1);
        const int len = rest ? __ffsll((long long)rest) : 64 - lane;  // lanes up to the next run's first one
        atomicAdd(&sh[b], (unsigned)len);
    }
}

}  // namespace

// Grid-stride over the n pixels at x: the floats before the first 16-byte boundary (`head`, everything when x is not even
// float aligned) and those behind the last whole group of four go one pixel per lane, the n4 groups between them as
// 16-byte loads, two in flight per lane (the kernel waits on HBM latency, not on LDS: 512 threads and two loads fill it).  The workgroup's histogram sits in LDS as 32-bit counts (a workgroup sees far fewer than 2^32 pixels:
// the grid grows with n up to kHistMaxBlocks) and is added to the global 64-bit counters once, bin by bin where it is not zero.
// Every loop has a trip count that is uniform over the workgroup: count_run needs whole waves.
__global__ __launch_bounds__(kHistThreads) void k_plane_hist(const float* __restrict__ x, long long n, long long head, long long n4,
                                                             double scale, unsigned long long* __restrict__ counts) {
    __shared__ unsigned sh[kToneCounts];
    const int tid = threadIdx.x;
    for (int i = tid; i < kToneCounts; i += kHistThreads) sh[i] = 0u;
    __syncthreads();
    const long long step = (long long)gridDim.x * kHistThreads;
    const float4* x4 = reinterpret_cast<const float4*>(x + head);
    for (long long g0 = (long long)blockIdx.x * kHistThreads; g0 < n4; g0 += 2 * step) {  // two loads in flight per lane
        const long long ga = g0 + tid, gb = ga + step;
        const bool ina = ga < n4, inb = gb < n4;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (ina) a = x4[ga];
        if (inb) b = x4[gb];
        count_run(sh, ina ? tone_bin(a.x, scale) : -1);
        count_run(sh, ina ? tone_bin(a.y, scale) : -1);
        count_run(sh, ina ? tone_bin(a.z, scale) : -1);
        count_run(sh, ina ? tone_bin(a.w, scale) : -1);
        count_run(sh, inb ? tone_bin(b.x, scale) : -1);
        count_run(sh, inb ? tone_bin(b.y, scale) : -1);
        count_run(sh, inb ? tone_bin(b.z, scale) : -1);
        count_run(sh, inb ? tone_bin(b.w, scale) : -1);
    }
    const long long body_end = head + n4 * 4, n1 = n - n4 * 4;  // n1: the pixels of the one-pixel path
    for (long long i0 = (long long)blockIdx.x * kHistThreads; i0 < n1; i0 += step) {
        const long long i = i0 + tid;
        const bool in = i < n1;
        const long long at = i < head ? i : body_end + (i - head);
        count_run(sh, in ? tone_bin(x[at], scale) : -1);
    }
    __syncthreads();
    for (int i = tid; i < kToneCounts; i += kHistThreads) {
        const unsigned c = sh[i];
        if (c != 0u) atomicAdd(&counts[i], (unsigned long long)c);
    }
}

hipError_t plane_hist(hipStream_t s, const float* d_x, long long n, double scale, unsigned long long* d_counts) {
    if (n < 1) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(d_counts, 0, sizeof(unsigned long long) * kToneCounts, s);
    if (e != hipSuccess) return e;
    const size_t addr = reinterpret_cast<size_t>(d_x);
    const long long head = (addr & 3) ? n : std::min<long long>(n, (long long)(((16 - (addr & 15)) & 15) / 4));
    const long long n4 = (n - head) / 4;
    const long long blocks = std::max<long long>((n4 + 2 * kHistThreads - 1) / (2 * kHistThreads), 1);  // two groups of four per lane
    hipLaunchKernelGGL(k_plane_hist, dim3((unsigned)std::min<long long>(blocks, kHistMaxBlocks)), dim3(kHistThreads), 0, s, d_x, n,
                       head, n4, scale, d_counts);
    return hipGetLastError();
}

// ---- the host rule (include/nle.h at nle_tone_curve): fp64, every operation on its own, in the order written there
namespace {

// C(t) = (t + (s t)(u u)) - (h (t t)) u,  u = 1 - t
double tone_c(double t, double s, double h) {
    const double u = 1.0 - t;
    return (t + (s * t) * (u * u)) - (h * (t * t)) * u;
}

// F(v): the share of pixels below v, linear inside a bin
double tone_share(const long long* counts, const long long* prefix, double n, double v) {
    const double q = (v + 256.0) * 4.0;
    const int k = (int)std::min(std::max(std::floor(q), 0.0), (double)(NLE_TONE_BINS - 1));
    const double phi = q - (double)k;
    return ((double)prefix[k] + phi * (double)counts[1 + k]) / n;
}

}  // namespace

const char* tone_check(double shadows, double highlights, double clip_percent, double equalise) {
    if (!std::isfinite(shadows) || shadows < -1 || shadows > 1) return "nle_tone_curve: shadows must be finite and in [-1, 1]";
    if (!std::isfinite(highlights) || highlights < -1 || highlights > 1)
        return "nle_tone_curve: highlights must be finite and in [-1, 1]";
    if (!std::isfinite(clip_percent)) return "nle_tone_curve: clip_percent must be finite (negative: no levels)";
    if (clip_percent > 25) return "nle_tone_curve: clip_percent must be at most 25";
    if (!std::isfinite(equalise) || equalise < 0 || equalise > 1) return "nle_tone_curve: equalise must be finite and in [0, 1]";
    return nullptr;
}

const char* tone_curve(const long long* counts, double shadows, double highlights, double clip_percent, double equalise,
                       double* curve) {
    if (!curve) return "nle_tone_curve: NULL pointer";
    if (const char* refused = tone_check(shadows, highlights, clip_percent, equalise)) return refused;
    const bool levels = clip_percent >= 0, eq = equalise != 0;
    if ((levels || eq) && !counts) return "nle_tone_curve: the counts are needed (clip_percent >= 0 or equalise > 0) and are NULL";
    constexpr int N = NLE_TONE_KNOTS - 1, B = NLE_TONE_BINS;
    std::vector<long long> prefix;  // prefix[k] = counts[0] + sum_{j < k} counts[1 + j], k = 0 .. B
    double n = 0.0;
    if (levels || eq) {
        for (int i = 0; i < B + 2; ++i)
            if (counts[i] < 0) return "nle_tone_curve: a count is negative";
        prefix.resize(B + 1);
        prefix[0] = counts[0];
        for (int k = 0; k < B; ++k) prefix[k + 1] = prefix[k] + counts[1 + k];
        const long long sum = prefix[B] + counts[B + 1];
        if (sum == 0) return "nle_tone_curve: the counts sum to 0";
        n = (double)sum;
    }
    double lo = 0.0, hi = 255.0;
    if (levels) {
        const double need = clip_percent / 100.0 * n;
        int klo = -1, khi = -1;
        long long cum = counts[0];
        for (int k = 0; k < B; ++k) {
            cum += counts[1 + k];
            if ((double)cum > need) {
                klo = k;
                break;
            }
        }
        cum = counts[B + 1];
        for (int k = B - 1; k >= 0; --k) {
            cum += counts[1 + k];
            if ((double)cum > need) {
                khi = k;
                break;
            }
        }
        if (klo >= 0 && khi >= 0) {
            const double l = -256.0 + 0.25 * (double)klo, h = -256.0 + 0.25 * (double)(khi + 1);
            if (!(h - l < 1.0)) lo = l, hi = h;
        }
    }
    curve[0] = lo, curve[1] = hi;
    double F_lo = 0.0, den = 0.0;
    if (eq) {
        F_lo = tone_share(counts, prefix.data(), n, lo);
        den = tone_share(counts, prefix.data(), n, hi) - F_lo;
    }
    for (int k = 0; k <= N; ++k) {
        const double t = (double)k / (double)N;
        double m = t;
        if (eq) {
            const double E = den == 0.0 ? t : (tone_share(counts, prefix.data(), n, lo + t * (hi - lo)) - F_lo) / den;
            m = (1.0 - equalise) * t + equalise * E;
        }
        curve[2 + k] = 255.0 * tone_c(m, shadows, highlights);
    }
    return nullptr;
}

}  // namespace nlek
