// Device helpers and layout constants of the level-sorted rows, shared by the kernels that walk them (sorted.hip,
// sorted_planes.hip): the LDS distance table and the column factors of a pixel, the chunk descriptor, the slot pitch of a
// row and the LDS layout of the pass kernels.  Not installed, not part of kernels.h: only those two files include it.
#pragma once
#include "kernels.h"

#define NLE_PIXEL_FENCE() __builtin_amdgcn_sched_barrier(0)

namespace nlek {

namespace {
constexpr int kLevels = 256;
constexpr int kT = kSortedThreads;

// E[|c - c_b|] from the LDS table, given the pre-scaled 16-bit operands c8 = 8 c, cb8 = 8 c_b (8 W <= 65536) and the LDS
// byte address of the table: ONE v_sad_u16 (|c8 - cb8| + base) makes the address -- no subtract / negate / max / shift /
// base add -- and the value is read through an LDS-address-space pointer
using lds_cdouble_ptr = const __attribute__((address_space(3))) double*;
__device__ __forceinline__ unsigned lds_addr(const void* p) {
    return (unsigned)(unsigned long long)(const __attribute__((address_space(3))) char*)p;
}
__device__ __forceinline__ double e_at(unsigned sE_addr, unsigned c8, unsigned cb8) {
    const unsigned a = __builtin_amdgcn_sad_u16(c8, cb8, sE_addr);
    return *(lds_cdouble_ptr)a;
}

// f(b, e_b) for b = 0 .. NC-1, e_b = exp(-(c - c_b)^2 / hx^2), c_b = cb0 + b cs: the column factors of one pixel.
//   REC == false: NC reads of the E table.  64 lanes read 64 unrelated addresses: ~3 lanes per bank on average, and at
//     NC reads per pixel the LDS pipe, not the VALU, bounds the pass kernels (round 2: 10 reads -> 84 us at cfg4).
//   REC == true: e_0 and e_1 from the table, the rest from the exact recurrence of a Gaussian on an equispaced grid,
//       e_{b+1} = e_b rho_b,   rho_{b+1} = rho_b kappa,   rho_0 = e_1 / e_0,   kappa = exp(-2 cs^2 / hx^2)
//     (2 reads + 2 (NC - 2) multiplies + one reciprocal).  Rounding: e_b carries O(b^2 / 2) ulp (NC = 10: ~5e-15
//     relative) -- the probes of profiles/r2_readme_pair_sensitivity.txt put 1e-13 affinity noise at 1e-11 on the layers.
//     The host enables it only where no e_b, rho_b leaves the normal range (sorted_recurrence).
template <int NC, bool REC, class F>
__device__ __forceinline__ void column_factors(unsigned sEa, unsigned c8, int cb0, int cs, double kappa, F&& f) {
    if constexpr (!REC || NC <= 2) {
#pragma unroll
        for (int b = 0; b < NC; ++b) f(b, e_at(sEa, c8, (unsigned)(cb0 + b * cs) << 3));
    } else {
        const double e0 = e_at(sEa, c8, (unsigned)cb0 << 3);
        double eb = e_at(sEa, c8, (unsigned)(cb0 + cs) << 3);
        f(0, e0);
        f(1, eb);
        double r = __builtin_amdgcn_rcp(e0);  // 1 / e_0 to 1 ulp: two Newton steps (e_0 is a normal number here)
        r = fma(fma(-e0, r, 1.0), r, r);
        r = fma(fma(-e0, r, 1.0), r, r);
        double rho = eb * r;
#pragma unroll
        for (int b = 2; b < NC; ++b) {
            rho *= kappa;
            eb *= rho;
            f(b, eb);
        }
    }
}
}  // namespace

// Chunk length bound: CH is the smallest length with sum_x ceil(tot[x] / CH) <= kT; with at most 256 non-empty levels
// that sum is <= wn / CH + 256, so CH <= ceil(W / 256) and a slot never needs more than sorted_chp_max(W) entries.
__host__ __device__ inline int sorted_chp_max(int W) { return (((W + 255) / 256) + 3) & ~3; }
constexpr int kMaxBlocks = 8;  // blocks of four indices per chunk: sorted_chp_max(sorted_max_width()) / 4
// entries per row of the scol buffer: kT slots of the largest size + the 4 entries a thread reads ahead of its slot
__host__ __device__ inline size_t sorted_row_pitch(int W) { return (size_t)kT * sorted_chp_max(W) + 4; }

// chunk descriptor: x = len | level << 6 | j << 14 | steps << 23,  y = m | CHP << 16
//   len    pixels of the chunk (0: idle thread),  j, m: the chunk is number j of the m chunks of its level,
//   steps  ceil(log2(max m of the row)) = depth of the combine tree,  CHP: slot size of this row (entries)
__device__ __forceinline__ int dsc_len(uint2 d) { return (int)(d.x & 63u); }
__device__ __forceinline__ int dsc_level(uint2 d) { return (int)((d.x >> 6) & 255u); }
__device__ __forceinline__ int dsc_j(uint2 d) { return (int)((d.x >> 14) & 511u); }
__device__ __forceinline__ int dsc_steps(uint2 d) { return (int)((d.x >> 23) & 15u); }
__device__ __forceinline__ int dsc_m(uint2 d) { return (int)(d.y & 0xffffu); }
__device__ __forceinline__ int dsc_chp(uint2 d) { return (int)(d.y >> 16); }

// ------------------------------------------------------------------ LDS layout shared by the pass kernels
// sE [W + 1] doubles | sP [kT][PS] doubles | sfirst [2][260] u16 (this row's and the next row's) | sCk [40] doubles (the
// quadratic factors of the moment form of k_sorted_pass)
__host__ __device__ inline size_t sorted_lds_bytes(int W, int ps) {
    return ((size_t)((W + 2) & ~1) + (size_t)kT * ps + 40) * sizeof(double) + 2 * 260 * sizeof(unsigned short);
}

// workgroups of a persistent pass over `nrows` rows: sr.wgs_per_cu per compute unit, at most one per row
int sorted_grid(int nrows, const SortedRows& sr);

}  // namespace nlek
