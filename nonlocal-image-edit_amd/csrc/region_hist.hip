// Per-region auto levels and equalise (include/nle.h "per-region histograms"): the membership-weighted
// histograms of the base layer, one per row m = 0 .. M, in one pass over y and the M membership planes.
//   alpha_m as nle_region_combine forms it (Memberships of detail_rule.h);  omega_m = (long long)(alpha_m 65536 + 0.5)
//   bin_m   = nle_plane_histogram's counter of (double)y scale_m (tone_bin of detail_rule.h)
//   counts[m][bin_m] += omega_m   for the rows that are switched on and where omega_m > 0
// Integer counts: exact, independent of every order, bit-equal from run to run.
// Only the rows that are on have counters: `slot[m]` is the row's place among them (< 0: off), and both the LDS image and the
// device result are slot-major, kToneCounts counters per slot; the host puts the slots back into their rows.
// Counter width: the workgroup's counters are 32 bit in LDS (nine rows are 147 528 B of the CU's 160 KiB; 64-bit ones would
// not fit).  A pixel adds at most 65536 to one counter of a row, so a counter holds fewer than 65536 pixels.  The GRID RULE
// bounds what a workgroup sees: workgroup b counts the pixels [b kRegionHistPixels, (b + 1) kRegionHistPixels) and nothing
// else, 32768 x 65536 = 2^31 at the most in one counter, and merges once at its end.  The grid grows with n and is not capped.
// The merge into the global 64-bit counters is k_plane_hist's: one vector atomic per counter that is not zero.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "detail_rule.h"
#include "kernels.h"
#include "launch.h"
#include "nle.h"

// the rule fixes where every rounding happens (alpha 65536 + 0.5 and y scale + 256 must not become one fma each)
#pragma clang fp contract(off)

namespace nlek {

namespace {

constexpr int kRegionHistThreads = 1024;
constexpr long long kRegionHistPixels = 32768;  // per workgroup, a multiple of 4: see "Counter width" above

static_assert(kRegionHistPixels * (long long)NLE_REGION_WEIGHT_ONE < (1ll << 32), "a 32-bit counter must hold a workgroup's pixels");
static_assert(kRegionHistPixels % 4 == 0, "a workgroup's first pixel keeps the planes' 16-byte alignment");

struct RegionHistArgs {
    const float* y;
    const float* q;
    long long q_stride, n;
    double floor;
    double scale[kRegionMax + 1];
    int slot[kRegionMax + 1];  // < 0: the row is off
    int nslots;
};

// the P pixels from i on, into the workgroup's counters.  The loop over the rows is unrolled (M is the instantiation's), so
// slot[m] and scale[m] are read at constant places and the planes' move down inside next_alpha is a renaming.
template <int M, int P>
__device__ __forceinline__ void hist_pixels(const RegionHistArgs& a, unsigned* sh, long long i) {
    Pack<P> Y;
    Memberships<P, M> mem;
    Y.load(a.y + i);
    mem.load(a.q, a.q_stride, M, i);
    mem.prepare(M, a.floor);
#pragma unroll
    for (int m = 0; m <= M; ++m) {
        double al[P];
        const bool any = mem.next_alpha(m, al);
        const int slot = a.slot[m];
        if (slot >= 0 && any) {
            unsigned* row = sh + slot * kToneCounts;
            const double scale = a.scale[m];
#pragma unroll
            for (int j = 0; j < P; ++j) {
                // alpha in (0, 1]: the conversion truncates, so this is the round half up of alpha 65536.  A NaN alpha (an
                // infinite q) fails the comparison and counts nothing
                const long long w = al[j] > 0.0 ? (long long)(al[j] * (double)NLE_REGION_WEIGHT_ONE + 0.5) : 0ll;
                if (w > 0) atomicAdd(&row[tone_bin(Y.v[j], scale)], (unsigned)w);
            }
        }
    }
}

}  // namespace

// 16-byte loads where y, q and (beyond one plane) the stride allow them, as the combine kernels decide it; the last n mod 4
// pixels, and everything when something breaks the alignment, go one pixel per lane.
template <int M>
__global__ __launch_bounds__(kRegionHistThreads) void k_region_hist(const RegionHistArgs a, unsigned long long* __restrict__ counts) {
    extern __shared__ unsigned sh_hist[];
    const int tid = threadIdx.x, nc = a.nslots * kToneCounts;
    for (int k = tid; k < nc; k += kRegionHistThreads) sh_hist[k] = 0u;
    __syncthreads();
    const long long i0 = (long long)blockIdx.x * kRegionHistPixels, i1 = i0 + kRegionHistPixels < a.n ? i0 + kRegionHistPixels : a.n;
    const bool vec = (((reinterpret_cast<size_t>(a.y) | reinterpret_cast<size_t>(a.q)) & 15) | (size_t)(M > 1 ? a.q_stride & 3 : 0)) == 0;
    long long rest = i0;
    if (vec) {
        rest = i0 + ((i1 - i0) & ~3ll);
        for (long long i = i0 + 4ll * tid; i < rest; i += 4ll * kRegionHistThreads) hist_pixels<M, 4>(a, sh_hist, i);
    }
    for (long long i = rest + tid; i < i1; i += kRegionHistThreads) hist_pixels<M, 1>(a, sh_hist, i);
    __syncthreads();
    for (int k = tid; k < nc; k += kRegionHistThreads) {
        const unsigned c = sh_hist[k];
        if (c != 0u) atomicAdd(&counts[k], (unsigned long long)c);
    }
}

hipError_t region_hist(hipStream_t s, const float* d_y, const float* d_q, long long q_stride, int M, long long n, const double* scale,
                       const int* slot, int nslots, double floor, unsigned long long* d_counts) {
    if (M < 1 || M > kRegionMax || n < 1 || q_stride < 0 || nslots < 1 || nslots > M + 1) return hipErrorInvalidValue;
    const long long blocks = (n + kRegionHistPixels - 1) / kRegionHistPixels;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    RegionHistArgs a{};
    a.y = d_y;
    a.q = d_q;
    a.q_stride = q_stride;
    a.n = n;
    a.floor = floor;
    a.nslots = nslots;
    for (int m = 0; m <= kRegionMax; ++m) {
        a.scale[m] = m <= M ? scale[m] : 0.0;
        a.slot[m] = m <= M ? slot[m] : -1;
        if (a.slot[m] >= nslots) return hipErrorInvalidValue;
    }
    hipError_t e = hipMemsetAsync(d_counts, 0, sizeof(unsigned long long) * (size_t)nslots * kToneCounts, s);
    if (e != hipSuccess) return e;
    const size_t shm = (size_t)nslots * kToneCounts * sizeof(unsigned);
    const bool known = dispatch_columns<1, kRegionMax>(M, [&](auto m) {
        e = launch(k_region_hist<decltype(m)::value>, dim3((unsigned)blocks), dim3(kRegionHistThreads), shm, s, a, d_counts);
    });
    return known ? e : hipErrorInvalidValue;
}

}  // namespace nlek
