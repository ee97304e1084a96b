// Reduce half of the sample-space apply for a GROUP of planes in one pass over the level-sorted rows.
//
// k_sorted_pass in XVEC mode (sorted.hip) turns one plane x into the per-row, per-level tables h_r[x][b] = sum_i e_b(c_i) c_i x_i.
// Per pixel it reads a 2-byte column index and the 8-byte scaling c_i and forms the column factors e_b -- none of which
// depends on the plane; only y_i = c_i x_i and the sums do.  k_sorted_reduce_planes walks the rows ONCE for NP planes: the
// index, c_i and the factors (e_0, rho, rho^2 of the moment form, or the e_b of the table / recurrence forms) are made once
// per pixel, then each plane's y and its nC sums are updated.  10 + 4 NP bytes per pixel instead of 14 NP.
//
// Bitwise contract: the tables of every plane are the bits k_sorted_pass<NC, CF> writes for that plane alone.  The order of a
// plane's sums is a function of the sorted rows only (one chunk per thread, chunks of a level combined in chunk order), and
// the per-plane arithmetic below is k_sorted_pass's, operation by operation.  That kernel is compiled with contraction on,
// and what the compiler makes of its expressions is pinned here instead of left to a second compilation: contraction is OFF
// in this file's kernel and every fused multiply-add is written out --
//     moment form     acc_0 = fma(y, e_0, acc_0),  te = y e_0;   acc_1 = fma(te, rho, acc_1),  to = te rho;
//                     acc_b = fma(t, rho^2, acc_b),  t = t rho^2   (t = te for even b, to for odd b);   acc_b *= C_b at the end
//     table / recurrence forms   acc_b = fma(e_b, y, acc_b)
// (read off the ISA of k_sorted_pass<3,2>, <10,2>, <10,0>, <20,1>, <36,0>, <36,1>: no v_add_f64 in any pixel loop).
// tests/test_apply_planes.py compares the outputs bit for bit on every form and at every column count where a path changes.
#include "sorted_rows.h"

#include <algorithm>

namespace nlek {

// Structure of k_sorted_pass: persistent workgroups, one level chunk per thread, the chunk's indices in registers, the next
// row's descriptor and indices requested under the current row's pixel loop.  XVEC only: no g tables, no reciprocal, no ybuf.
// CF as in k_sorted_pass (0 table reads, 1 recurrence, 2 moments).  Plane m of the group: x at pg.x[m] (virtual base of the
// full image), table out at pg.h[m] ([nrows][b][x], k_sorted_pass's layout).
// Registers: 2 NC NP for the sums beside ~70 for the indices of two rows and the pixel's temporaries: four waves per SIMD
// (two workgroups per CU, as k_sorted_pass up to 12 columns) while that fits 128 without scratch, else two (one workgroup
// per CU; <10, 2, 3> at four spilled 12 bytes).  No instantiation uses scratch (-Rpass-analysis=kernel-resource-usage).
__host__ __device__ constexpr int planes_waves_per_simd(int nc, int np) { return nc * np <= 28 ? 4 : 2; }

template <int NC, int CF, int NP>
__global__ __launch_bounds__(kT, planes_waves_per_simd(NC, NP)) void k_sorted_reduce_planes(
    const unsigned short* __restrict__ scol, const uint2* __restrict__ desc, const unsigned short* __restrict__ first, GridSpec gs,
    int row0, int nrows, const double* __restrict__ Etab, const double* __restrict__ cvec, PlaneGroup pg, double kappa,
    int lev_t0, int lev_nt) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int n = kLevels * NC;
    constexpr bool REC = CF == 1, MOM = CF == 2;
    static_assert(!MOM || NC > 1, "the moment form needs two columns");
    const int W = gs.W;
    const RowLds lds(smem_raw, W, kPassStride<NC>);
    double* const sP = lds.sP;
    unsigned short* const sfirst = lds.sfirst;
    double* const sCk = lds.sCk;
    const int tid = threadIdx.x;
    fill_dist_table(lds.sE, Etab, W, tid);
    if (MOM) fill_moment_factors<NC>(sCk, kappa, tid);
    const int cb0 = gs.colOff, cs = gs.colStep;
    const unsigned sEa = lds_addr(lds.sE);

    RowWalk w(scol, desc, W, nrows, tid);
    w.start([&] {
        if (tid < 258) sfirst[tid] = first[(size_t)w.lrow * 258 + tid];
    });
    __syncthreads();  // sE, sfirst, sCk visible
    for (int par = 0;; par ^= 1) {
        const bool has_next = w.has_next();
        const int lrow = w.lrow;
        const unsigned short* sfc = sfirst + par * 260;
        const int len = dsc_len(w.dsc);
        double acc[NP][NC];
#pragma unroll
        for (int m = 0; m < NP; ++m)
#pragma unroll
            for (int b = 0; b < NC; ++b) acc[m][b] = 0.0;
        const double* cv_row = cvec + (size_t)lrow * W;
        const float* xv_row[NP];
#pragma unroll
        for (int m = 0; m < NP; ++m) xv_row[m] = pg.x[m] + (size_t)(row0 + lrow) * W;
        // in flight under the pixel loop, with the walk's requests: the next row's first-chunk table
        unsigned short sf_n = 0;
        RowWalk::Next nx;
        w.request_next(nx, [&] { sf_n = first[(size_t)w.nrow * 258 + (tid < 258 ? tid : 257)]; });
        // One pixel at a time for all planes of the group.  The plane-independent part first, exactly k_sorted_pass's; then
        // per plane y = c x and the sums.  Lanes past their own chunk work on column 0 and add exact zeros.
        auto pixel_mom = [&](const unsigned c8, const int at) {
            if constexpr (!MOM) return;
            else {
                const double e0 = e_at(sEa, c8, (unsigned)cb0 << 3);
                double rho = e_at(sEa, c8, (unsigned)(cb0 + cs) << 3);
                const bool keep = at < len;
                const double cv = cv_row[c8 >> 3];
                float xs[NP];
#pragma unroll
                for (int m = 0; m < NP; ++m) xs[m] = xv_row[m][c8 >> 3];
                double r0 = __builtin_amdgcn_rcp(e0);  // e_0 is a normal number here (sorted_moments_ok)
                r0 = fma(fma(-e0, r0, 1.0), r0, r0);
                r0 = fma(fma(-e0, r0, 1.0), r0, r0);
                rho = rho * r0;
                const double rho2 = rho * rho;
#pragma unroll
                for (int m = 0; m < NP; ++m) {
                    double y = cv * (double)xs[m];  // apply: y_i = c_i x_i
                    y = keep ? y : 0.0;             // the padding of the slot adds exact zeros
                    double te = y * e0;
                    acc[m][0] = fma(y, e0, acc[m][0]);
                    double to = te * rho;
                    acc[m][1] = fma(te, rho, acc[m][1]);
#pragma unroll
                    for (int b = 2; b < NC; b += 2) {
                        acc[m][b] = fma(te, rho2, acc[m][b]);
                        te = te * rho2;
                        if (b + 1 < NC) {
                            acc[m][b + 1] = fma(to, rho2, acc[m][b + 1]);
                            to = to * rho2;
                        }
                    }
                }
            }
        };
        auto pixel = [&](const unsigned c8, const bool on) {
            const double cv = cv_row[c8 >> 3];
            double y[NP];
#pragma unroll
            for (int m = 0; m < NP; ++m) {
                const double v = cv * (double)xv_row[m][c8 >> 3];  // apply: y_i = c_i x_i
                y[m] = on ? v : 0.0;                               // the padding of the slot adds exact zeros
            }
            column_factors<NC, REC>(sEa, c8, cb0, cs, kappa, [&](const int b, const double ev) {
#pragma unroll
                for (int m = 0; m < NP; ++m) acc[m][b] = fma(ev, y[m], acc[m][b]);
            });
        };
        for_chunk_pixels(w.idx, wave_max_len(len), [&](const unsigned c8, const int at) {
            if constexpr (MOM) pixel_mom(c8, at);
            else pixel(c8, at < len);
        });
        if constexpr (MOM) {
#pragma unroll
            for (int m = 0; m < NP; ++m)
#pragma unroll
                for (int b = 2; b < NC; ++b) acc[m][b] = acc[m][b] * sCk[b];  // C_0 = C_1 = 1
        }
        __builtin_amdgcn_s_setprio(3);
        constexpr int SL = kPassSlice<NC>, PS = kPassStride<NC>;  // sums combined per slice, as k_sorted_pass
        // The combine of k_sorted_pass, plane after plane through the same sP: the partial sums of a level's chunks are
        // written to LDS and every table entry is summed by ONE thread in chunk order, then stored.  No atomics.
        const int nlev = lev_nt * 16, xlo = lev_t0 * 16;
        const float inv_nlev = 1.0f / (float)nlev;
#pragma unroll
        for (int m = 0; m < NP; ++m) {
            double* hrow = pg.h[m] + (size_t)lrow * n;
#pragma unroll
            for (int s0 = 0; s0 < NC; s0 += SL) {
#pragma unroll
                for (int i = 0; i < SL; ++i) sP[tid * PS + i] = (s0 + i < NC) ? acc[m][s0 + i] : 0.0;
                __syncthreads();
                if (m == 0 && s0 == 0) {
                    // take the next row's loads in before the table stores below (all lanes), as k_sorted_pass does
                    asm volatile("" ::"v"(sf_n));
                    w.take_in(nx);
                    // next row's first-chunk table: its last readers left before the previous row's end barrier, its next
                    // readers come after the barriers of the next row's combine
                    if (has_next && tid < 258) sfirst[(par ^ 1) * 260 + tid] = sf_n;
                }
                const int ns = (NC - s0 < SL) ? NC - s0 : SL;
                for (int i = tid; i < ns * nlev; i += kT) {
                    const int bb = (int)(((float)i + 0.5f) * inv_nlev);  // i / nlev, exact (see k_sorted_pass)
                    const int xx = xlo + (i - bb * nlev);
                    const int f0 = sfc[xx], f1 = sfc[xx + 1];
                    double sum = 0.0;
                    for (int t = f0; t < f1; ++t) sum += sP[t * PS + bb];
                    hrow[(size_t)(s0 + bb) * kLevels + xx] = sum;
                }
                __syncthreads();  // before the next slice / plane / row overwrites sP and sfirst
            }
        }
        __builtin_amdgcn_s_setprio(0);
        if (!has_next) break;
        w.advance(nx);
    }
}

// planes one launch takes: four up to 12 columns, two beyond (registers: 2 NC NP for the sums; no scratch in any instantiation)
int sorted_planes_per_launch(GridSpec gs) { return gs.nSelCols <= 12 ? kPlanesPerLaunch : 2; }

hipError_t sorted_reduce_planes(hipStream_t s, GridSpec gs, int row0, int nrows_local, const SortedRows& sr, const double* d_cvec,
                                const PlaneGroup& pg, int np) {
    const int nC = gs.nSelCols, lev_t0 = sr.lev_t0, lev_nt = sr.lev_nt;
    if (!tables_apply(gs) || gs.W > sorted_max_width() || lev_t0 < 0 || lev_nt < 1 || lev_t0 + lev_nt > kLevels / 16 || np < 2 ||
        np > sorted_planes_per_launch(gs))
        return hipErrorInvalidValue;
    if (nrows_local <= 0) return hipSuccess;
    const size_t shm = sorted_lds_bytes(gs.W, (nC < 11 ? nC : 11) | 1);
    // the grid of the single-plane pass, or one workgroup per CU where the registers leave room for one only
    SortedRows one = sr;
    if (planes_waves_per_simd(nC, np) < 4) one.wgs_per_cu = 1;
    const int grid = sorted_grid(nrows_local, one);
    const auto run = [&](auto kernel) {
        return launch(kernel, dim3((unsigned)grid), dim3(kT), shm, s, sr.scol, sr.desc, sr.first, gs, row0, nrows_local, sr.E, d_cvec,
                      pg, sr.kappa, lev_t0, lev_nt);
    };
    hipError_t e = hipErrorInvalidValue;
    dispatch_columns<1, 36>(nC, [&](auto nc) {
        constexpr int NC = decltype(nc)::value;
        // NP: 2, 3 or 4 up to 12 columns, 2 beyond
        const auto planes = [&](auto cf) {
            constexpr int CF = decltype(cf)::value;
            if constexpr (NC <= 12) {
                if (np == 4) return run(k_sorted_reduce_planes<NC, CF, 4>);
                if (np == 3) return run(k_sorted_reduce_planes<NC, CF, 3>);
            }
            return run(k_sorted_reduce_planes<NC, CF, 2>);
        };
        // the form a single call would take: sorted_pass's rules on sr.mom / sr.rec
        if constexpr (NC > 1) {
            if (sr.mom) {
                e = planes(std::integral_constant<int, 2>{});
                return;
            }
        }
        if constexpr (NC > 12) e = sr.rec ? planes(std::integral_constant<int, 1>{}) : planes(std::integral_constant<int, 0>{});
        else if (!sr.rec) e = planes(std::integral_constant<int, 0>{});
    });
    return e;
}

}  // namespace nlek
