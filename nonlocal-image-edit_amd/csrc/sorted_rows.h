// The level-sorted rows and their walk, shared by the kernels that walk them (sorted.hip, sorted_planes.hip).  This header
// owns the layout -- the chunk descriptor, the slot pitch of a row, the LDS layout of the pass kernels -- and every step of
// the walk that does not depend on who walks: the LDS distance table and the column factors of a pixel, the index load of a
// chunk, the software pipeline of a persistent workgroup over its rows (RowWalk), the wave's chunk bound, the per-pixel loop
// over a chunk and the LDS carve-up with its fills.  A kernel brings its per-pixel arithmetic, what it prefetches beyond the
// walk and its combine.  (The level sum of the two pass kernels and the loop and store tail of the three Gram kernels are
// still written out in each: as shared functions they changed scratch or occupancy of some instantiations,
// profiles/r15_sorted_rows_refactor.txt.)
// Not installed, not part of kernels.h: only those two files include it.
#pragma once
#include "kernels.h"
#include "launch.h"

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

template <int NC>
constexpr int kPassSlice = NC < 11 ? NC : 11;  // sums of the pass kernels combined at a time (slices of the nC sums when nC > 11)
template <int NC>
constexpr int kPassStride = kPassSlice<NC> | 1;  // PS, odd: consecutive threads' rows of sP start on different banks
struct RowLds {
    double* sE;
    double* sP;
    unsigned short* sfirst;  // [2][260], rows alternate
    double* sCk;             // [NC] C_b = kappa^(b (b - 1) / 2)
    __device__ __forceinline__ RowLds(unsigned char* smem, int W, int ps) {
        sE = reinterpret_cast<double*>(smem);
        sP = sE + ((W + 2) & ~1);
        sfirst = reinterpret_cast<unsigned short*>(sP + (size_t)kT * ps);
        sCk = reinterpret_cast<double*>(sfirst + 2 * 260);
    }
};
__device__ __forceinline__ void fill_dist_table(double* sE, const double* __restrict__ Etab, int W, int tid) {
    for (int i = tid; i <= W; i += kT) sE[i] = Etab[i];
}
template <int NC>
__device__ __forceinline__ void fill_moment_factors(double* sCk, double kappa, int tid) {
    if (tid == 0) {
        double ck = 1.0, kp = 1.0;  // C_{b+1} = C_b kappa^b
        for (int b = 0; b < NC; ++b) {
            sCk[b] = ck;
            ck *= kp;
            kp *= kappa;
        }
    }
}

// ------------------------------------------------------------------ the walk
// all indices of a chunk (<= kMaxBlocks blocks of four) into registers: the pixel loops themselves load nothing
__device__ __forceinline__ void load_chunk_idx(uint2 (&dst)[kMaxBlocks], const unsigned short* __restrict__ scol, size_t pitch,
                                               int row, int tid, uint2 d) {
    const uint2* slot = reinterpret_cast<const uint2*>(scol + (size_t)row * pitch + (size_t)tid * dsc_chp(d));
    const int ln = dsc_len(d);
#pragma unroll
    for (int b = 0; b < kMaxBlocks; ++b) {  // blocks past the chunk: column 0 (the wave may walk further than this lane)
        uint2 v = make_uint2(0u, 0u);
        if (4 * b < ln) v = slot[b];
        dst[b] = v;
    }
}

// Software pipeline over the rows of a persistent workgroup (rows blockIdx.x, + gridDim.x, ...; gridDim.x <= nrows):
// everything a row needs from global memory is requested while the PREVIOUS row is being worked on -- its indices one row
// ahead and, because their address needs the row's chunk descriptor, the descriptor two rows ahead -- and taken in before
// that row's stores.  Nothing foreign is pending during the pixel loop, so its waits (the counter retires in order) are exact.
//     RowWalk w(...);  w.start(more);
//     for (;;) { RowWalk::Next nx;  w.request_next(nx, more);  <pixel loop over w.idx>  ... barrier, w.take_in(nx), stores ...
//                if (!w.has_next()) break;  w.advance(nx); }
// `more`: what else the kernel wants requested, between the descriptor and the indices (loads return in that order).
struct RowWalk {
    const unsigned short* __restrict__ scol;
    const uint2* __restrict__ desc;
    const size_t pitch;
    const int nrows, tid, G;
    int lrow, nrow;
    uint2 dsc, dsc_n;        // this row's chunk of the thread and the next row's
    uint2 idx[kMaxBlocks];   // this row's indices
    struct Next {            // in flight under the pixel loop
        int nnrow;
        uint2 dsc_nn;
        uint2 idx[kMaxBlocks];
    };
    __device__ __forceinline__ RowWalk(const unsigned short* __restrict__ scol_, const uint2* __restrict__ desc_, int W, int nrows_,
                                       int tid_)
        : scol(scol_), desc(desc_), pitch(sorted_row_pitch(W)), nrows(nrows_), tid(tid_), G((int)gridDim.x) {}
    __device__ __forceinline__ bool has_next() const { return nrow < nrows; }
    // component by component: an 8-byte copy between members of one struct becomes a 64-bit integer, kept whole in
    // registers where only a half is still needed
    static __device__ __forceinline__ void set(uint2& d, const uint2 s) { d.x = s.x, d.y = s.y; }
    template <class More>
    __device__ __forceinline__ void start(More&& more) {
        lrow = blockIdx.x, nrow = lrow + G;
        set(dsc, desc[(size_t)lrow * kT + tid]);
        set(dsc_n, dsc);
        if (nrow < nrows) set(dsc_n, desc[(size_t)nrow * kT + tid]);
        more();
        load_chunk_idx(idx, scol, pitch, lrow, tid, dsc);
    }
    // requested BEFORE the pixel loop, in flight under it (the loop has no wait on the memory counter): the descriptor of
    // the row after next and the next row's indices
    template <class More>
    __device__ __forceinline__ void request_next(Next& nx, More&& more) const {
        nx.nnrow = nrow + G;
        set(nx.dsc_nn, dsc_n);
        if (has_next()) {
            if (nx.nnrow < nrows) set(nx.dsc_nn, desc[(size_t)nx.nnrow * kT + tid]);
            more();
            load_chunk_idx(nx.idx, scol, pitch, nrow, tid, dsc_n);
        }
    }
    // Were the requested loads still pending behind the stores that end a row, the next row's first pixel would wait for
    // those stores to be acknowledged.  Take them in before (all lanes: a divergent use would leave a load pending for the
    // others).
    __device__ __forceinline__ void take_in(const Next& nx) const {
        asm volatile("" ::"v"(nx.dsc_nn.x), "v"(nx.dsc_nn.y));
#pragma unroll
        for (int b = 0; b < kMaxBlocks; ++b) asm volatile("" ::"v"(nx.idx[b].x), "v"(nx.idx[b].y));
    }
    __device__ __forceinline__ void advance(const Next& nx) {
        lrow = nrow;
        nrow = nx.nnrow;
        set(dsc, dsc_n);
        set(dsc_n, nx.dsc_nn);
#pragma unroll
        for (int b = 0; b < kMaxBlocks; ++b) idx[b] = nx.idx[b];
    }
};

// the longest chunk of the WAVE: a scalar bound for the pixel loop, so that a wave whose chunks are all short skips the
// rest without per-lane bookkeeping
__device__ __forceinline__ int wave_max_len(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    return __builtin_amdgcn_readfirstlane(v);
}

// pixel(c8, at) for the pixels of a chunk up to the wave's bound, `at` the pixel's place in the chunk.  One pixel at a time:
// the scheduling barrier keeps the unrolled bodies from being interleaved (the column factors of one pixel fill the
// registers).  Lanes past their own chunk (and the padding of the last block) get column 0 and must add exact zeros.
template <class Pixel>
__device__ __forceinline__ void for_chunk_pixels(const uint2 (&idx)[kMaxBlocks], int wlen, Pixel&& pixel) {
#pragma unroll
    for (int b = 0; b < kMaxBlocks; ++b) {
        if (4 * b >= wlen) break;
        const unsigned cs4[4] = {idx[b].x & 0xffffu, idx[b].x >> 16, idx[b].y & 0xffffu, idx[b].y >> 16};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (4 * b + k < wlen) {
                pixel(cs4[k], 4 * b + k);
                NLE_PIXEL_FENCE();
            }
        }
    }
}

// workgroups of a persistent pass over `nrows` rows: sr.wgs_per_cu per compute unit, at most one per row
int sorted_grid(int nrows, const SortedRows& sr);

}  // namespace nlek
