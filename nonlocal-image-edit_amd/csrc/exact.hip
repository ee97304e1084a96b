// The exact (Nystrom-free) filter, opt-in NLE_MODE_EXACT_F64: Y = K X with the full N x N pixel affinity K regenerated on
// the fly and never stored, plus the element-wise helpers of its eigensolver (pipeline.hip: train_exact64).
//
//   K_ij = exp(-sw (double)((r_i - r_j)^2 + (c_i - c_j)^2) - pw (y_i - y_j)^2),  sw = 1/hx^2, pw = 1/hy^2
//
// The plane is integer valued in [0, 255] (the L channel of 8-bit Lab), so K_ij = Es[|dr|] Es[|dc|] El[|dy|] with
// Es[d] = exp(-sw d^2) (max(H, W) entries) and El[d] = exp(-pw d^2) (256 entries): no exp in the loop, within a few ulp
// of the exponential of the sum.
//
// Two forms, both deterministic (no atomics, fixed summation orders) and both segmented over the source pixels so that
// no launch runs much longer than ~50 ms at the size cap; segments accumulate into Y in ascending order.
//   k_affprod64_mfma    ncols >= 3: a workgroup owns 64 output pixels (one 16-pixel tile per wave) and NT 16-column
//                       tiles, walks the segment's source pixels 32 at a time through LDS (X tile and the pixels'
//                       coordinates) and makes the 16 x 4 affinity tile in registers as the A operand of
//                       v_mfma_f64_16x16x4_f64; the X tile is the B operand.  D layout: col = lane & 15,
//                       row = (lane >> 4) + 4 e.
//   k_affprod64_narrow  ncols 1 or 2 (the Sinkhorn products): one output pixel per thread, a sequential fp64 sum over a
//                       sub-segment of the source pixels (staged 256 at a time in LDS); per-sub-segment partials are
//                       summed in ascending order by k_affprod64_reduce.  These products are bound by making
//                       affinities, not by arithmetic, so they run on the VALU.
// The spatial table lives in LDS when max(H, W) <= kExactTabLds, else it is read through the L1/L2.
#include "kernels.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace nlek {

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {
constexpr int kExactTabLds = 4096;  // spatial table entries held in LDS (32 KB)
constexpr int kMfmaSrc = 32;        // source pixels per LDS stage of the MFMA form
constexpr int kNarrowSrc = 256;     // source pixels per LDS stage of the VALU form
constexpr int kMaxSub = 16;         // sub-segments (partials) of the VALU form per launch
// per-launch work budgets (~50 ms each at rates well below the measured ones: DESIGN.md section 3.7)
constexpr double kMfmaFlopPerLaunch = 1.0e12;
constexpr double kNarrowAffPerLaunch = 1.0e11;

__device__ __forceinline__ int level_of(float v) { return min(max((int)v, 0), 255); }
__device__ __forceinline__ double recip0_x(double s, double eps) { return (fabs(s) >= eps) ? 1.0 / s : 0.0; }

template <int NT, bool TAB_LDS>
__global__ __launch_bounds__(256) void k_affprod64_mfma(const float* __restrict__ lum, int W, long long N,
                                                        const double* __restrict__ Es_g, int es_len,
                                                        const double* __restrict__ El_g, const double* __restrict__ X,
                                                        int ldx, int ncols, double* __restrict__ Y, int ldy,
                                                        long long s_lo, long long s_hi, int beta) {
    constexpr int C = NT * 16, CS = C + 4;  // X tile columns, LDS row stride (doubles)
    __shared__ double xs[kMfmaSrc * CS];
    __shared__ double el[256];
    __shared__ int4 src[kMfmaSrc];
    __shared__ double es_l[TAB_LDS ? kExactTabLds : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kq = lane >> 4;
    const long long out0 = (long long)blockIdx.x * 64 + wave * 16;
    const int col0 = blockIdx.y * C;
    for (int k = tid; k < 256; k += 256) el[k] = El_g[k];
    if (TAB_LDS)
        for (int k = tid; k < es_len; k += 256) es_l[k] = Es_g[k];
    const double* Es = TAB_LDS ? es_l : Es_g;
    // this lane's A-operand row: output pixel out0 + l15 (clamped: rows >= N are computed but never stored)
    const long long ia = min(out0 + l15, N - 1);
    const int ra = (int)(ia / W), ca = (int)(ia - (long long)ra * W), ya = level_of(lum[ia]);
    f64x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (long long s0 = s_lo; s0 < s_hi; s0 += kMfmaSrc) {
        __syncthreads();  // the previous stage's readers are done (and the tables are in place)
        for (int f = tid; f < kMfmaSrc * C; f += 256) {
            const int jl = f / C, cl = f - jl * C;
            const long long j = s0 + jl;
            const int col = col0 + cl;
            xs[jl * CS + cl] = (j < s_hi && col < ncols) ? X[(size_t)j * ldx + col] : 0.0;
        }
        if (tid < kMfmaSrc) {
            const long long j = s0 + tid;
            int4 v = make_int4(ra, ca, ya, 0);  // a padded source pixel: any in-range indices (its X row is zero)
            if (j < s_hi) {
                const int r = (int)(j / W);
                v = make_int4(r, (int)(j - (long long)r * W), level_of(lum[j]), 0);
            }
            src[tid] = v;
        }
        __syncthreads();
#pragma unroll 2
        for (int q = 0; q < kMfmaSrc / 4; ++q) {
            const int jl = 4 * q + kq;
            const int4 sv = src[jl];
            const double a = Es[abs(ra - sv.x)] * Es[abs(ca - sv.y)] * el[abs(ya - sv.z)];
            const double* xrow = xs + jl * CS + l15;
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, xrow[t * 16], acc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = col0 + t * 16 + l15;
        if (col >= ncols) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long long row = out0 + kq + 4 * e;
            if (row < N) {
                double* y = Y + (size_t)row * ldy + col;
                *y = beta ? *y + acc[t][e] : acc[t][e];
            }
        }
    }
}

template <int NC, bool TAB_LDS>
__global__ __launch_bounds__(256) void k_affprod64_narrow(const float* __restrict__ lum, int W, long long N,
                                                          const double* __restrict__ Es_g, int es_len,
                                                          const double* __restrict__ El_g, const double* __restrict__ X,
                                                          int ldx, long long s_lo, long long s_hi, long long sub_len,
                                                          double* __restrict__ part) {
    __shared__ double el[256];
    __shared__ int4 src[kNarrowSrc];
    __shared__ double xs[kNarrowSrc * NC];
    __shared__ double es_l[TAB_LDS ? kExactTabLds : 1];
    const int tid = threadIdx.x;
    for (int k = tid; k < 256; k += 256) el[k] = El_g[k];
    if (TAB_LDS)
        for (int k = tid; k < es_len; k += 256) es_l[k] = Es_g[k];
    const double* Es = TAB_LDS ? es_l : Es_g;
    const long long i = (long long)blockIdx.x * 256 + tid;
    const long long ic = min(i, N - 1);
    const int ri = (int)(ic / W), ci = (int)(ic - (long long)ri * W), yi = level_of(lum[ic]);
    const long long a0 = s_lo + (long long)blockIdx.y * sub_len, a1 = min(s_hi, a0 + sub_len);
    double acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.0;
    for (long long s0 = a0; s0 < a1; s0 += kNarrowSrc) {
        const int n = (int)min((long long)kNarrowSrc, a1 - s0);
        __syncthreads();
        if (tid < n) {
            const long long j = s0 + tid;
            const int r = (int)(j / W);
            src[tid] = make_int4(r, (int)(j - (long long)r * W), level_of(lum[j]), 0);
#pragma unroll
            for (int c = 0; c < NC; ++c) xs[tid * NC + c] = X[(size_t)j * ldx + c];
        }
        __syncthreads();
        for (int k = 0; k < n; ++k) {
            const int4 sv = src[k];
            const double a = Es[abs(ri - sv.x)] * Es[abs(ci - sv.y)] * el[abs(yi - sv.z)];
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[c] += a * xs[k * NC + c];
        }
    }
    if (i < N)
#pragma unroll
        for (int c = 0; c < NC; ++c) part[((size_t)blockIdx.y * N + i) * NC + c] = acc[c];
}

// Y[i][c] (+)= sum over the sub-segments in ascending order
template <int NC>
__global__ void k_affprod64_reduce(const double* __restrict__ part, int nsub, long long N, double* __restrict__ Y, int ldy,
                                   int beta) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        double s = 0.0;
        for (int k = 0; k < nsub; ++k) s += part[((size_t)k * N + i) * NC + c];
        double* y = Y + (size_t)i * ldy + c;
        *y = beta ? *y + s : s;
    }
}

template <int NT, bool TAB>
hipError_t launch_mfma(hipStream_t st, const ExactPlane& pl, const double* X, int ldx, int ncols, double* Y, int ldy) {
    const long long N = (long long)pl.H * pl.W;
    const int cblocks = (ncols + NT * 16 - 1) / (NT * 16);
    const double flop_per_src = 2.0 * (double)N * cblocks * NT * 16;
    long long seg = (long long)(kMfmaFlopPerLaunch / flop_per_src);
    seg = std::max<long long>(kMfmaSrc, (seg / kMfmaSrc) * kMfmaSrc);
    const dim3 grid((unsigned)((N + 63) / 64), (unsigned)cblocks);
    for (long long s = 0; s < N; s += seg) {
        hipLaunchKernelGGL((k_affprod64_mfma<NT, TAB>), grid, dim3(256), 0, st, pl.lum, pl.W, N, pl.d_es, pl.es_len, pl.d_el,
                           X, ldx, ncols, Y, ldy, s, std::min(N, s + seg), s > 0 ? 1 : 0);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <int NC, bool TAB>
hipError_t launch_narrow(hipStream_t st, const ExactPlane& pl, const double* X, int ldx, double* Y, int ldy) {
    const long long N = (long long)pl.H * pl.W;
    const long long nb = (N + 255) / 256;
    // enough workgroups to fill the device (~8 waves per CU) when N is small: split the sources into sub-segments
    const int nsub = (int)std::min<long long>(kMaxSub, std::max<long long>(1, 2048 / nb));
    long long seg = (long long)(kNarrowAffPerLaunch / (double)N);
    seg = std::max<long long>(kNarrowSrc, seg);
    for (long long s = 0; s < N; s += seg) {
        const long long s1 = std::min(N, s + seg);
        const long long sub = (s1 - s + nsub - 1) / nsub;
        hipLaunchKernelGGL((k_affprod64_narrow<NC, TAB>), dim3((unsigned)nb, (unsigned)nsub), dim3(256), 0, st, pl.lum, pl.W,
                           N, pl.d_es, pl.es_len, pl.d_el, X, ldx, s, s1, sub, pl.d_part);
        hipLaunchKernelGGL((k_affprod64_reduce<NC>), dim3((unsigned)nb), dim3(256), 0, st, pl.d_part, nsub, N, Y, ldy,
                           s > 0 ? 1 : 0);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <bool TAB>
hipError_t product_tab(hipStream_t st, const ExactPlane& pl, const double* X, int ldx, int ncols, double* Y, int ldy) {
    if (ncols == 1) return launch_narrow<1, TAB>(st, pl, X, ldx, Y, ldy);
    if (ncols == 2) return launch_narrow<2, TAB>(st, pl, X, ldx, Y, ldy);
    if (ncols <= 16) return launch_mfma<1, TAB>(st, pl, X, ldx, ncols, Y, ldy);
    if (ncols <= 32) return launch_mfma<2, TAB>(st, pl, X, ldx, ncols, Y, ldy);
    if (ncols <= 64) return launch_mfma<4, TAB>(st, pl, X, ldx, ncols, Y, ldy);
    return launch_mfma<8, TAB>(st, pl, X, ldx, ncols, Y, ldy);
}

// ---- element-wise helpers of the eigensolver
// the start block: a fixed function of (pixel, column), uniform in [-1, 1)
__global__ void k_exact_start(double* __restrict__ X, long long N, int ld, int col0, int ncols, unsigned seed) {
    const long long n = N * ncols;
    for (long long f = blockIdx.x * (long long)blockDim.x + threadIdx.x; f < n; f += (long long)gridDim.x * blockDim.x) {
        const long long i = f / ncols;
        const int c = (int)(f - i * ncols);
        unsigned long long h = (unsigned long long)i * 0x9E3779B97F4A7C15ull ^
                               ((unsigned long long)(col0 + c) + 1ull) * 0xC2B2AE3D27D4EB4Full ^ (unsigned long long)seed;
        h ^= h >> 33;
        h *= 0xFF51AFD7ED558CCDull;
        h ^= h >> 33;
        h *= 0xC4CEB9FE1A85EC53ull;
        h ^= h >> 33;
        X[(size_t)i * ld + col0 + c] = (double)(h >> 11) * 0x1.0p-52 - 1.0;
    }
}

// Z (N x 2b, ld 2b) = [c o Q | r o Q] for Q = X[:, 0:b] (ld ldx)
__global__ void k_exact_scale2(const double* __restrict__ X, int ldx, long long N, int b, const double* __restrict__ cv,
                               const double* __restrict__ rv, double* __restrict__ Z) {
    const long long n = N * b;
    for (long long f = blockIdx.x * (long long)blockDim.x + threadIdx.x; f < n; f += (long long)gridDim.x * blockDim.x) {
        const long long i = f / b;
        const int k = (int)(f - i * b);
        const double x = X[(size_t)i * ldx + k];
        Z[(size_t)i * 2 * b + k] = cv[i] * x;
        Z[(size_t)i * 2 * b + b + k] = rv[i] * x;
    }
}

// A[:, 0:b] (ld lda) = (r o Y[:, 0:b] + c o Y[:, b:2b]) / 2   -- Ws X = (r o K(c o X) + c o K(r o X)) / 2
__global__ void k_exact_combine(const double* __restrict__ Yv, long long N, int b, const double* __restrict__ cv,
                                const double* __restrict__ rv, double* __restrict__ A, int lda) {
    const long long n = N * b;
    for (long long f = blockIdx.x * (long long)blockDim.x + threadIdx.x; f < n; f += (long long)gridDim.x * blockDim.x) {
        const long long i = f / b;
        const int k = (int)(f - i * b);
        A[(size_t)i * lda + k] = 0.5 * (rv[i] * Yv[(size_t)i * 2 * b + k] + cv[i] * Yv[(size_t)i * 2 * b + b + k]);
    }
}

// v[i] = recip(v[i])  (inplaceReciprocal, src/filter.cpp:42-54)
__global__ void k_exact_recip(double* __restrict__ v, long long N, double eps) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x)
        v[i] = recip0_x(v[i], eps);
}

// D[:, 0:n] (ld ldd) = alpha S[:, 0:n] (ld lds) + (B ? beta B[:, 0:n] (ld ldb) : 0); D may be B; columns [n, pad) of D are zeroed
__global__ void k_exact_axpby(const double* S, int lds, double alpha, const double* B, int ldb, double beta,
                              double* D, int ldd, long long N, int n, int pad) {
    const long long m = N * pad;
    for (long long f = blockIdx.x * (long long)blockDim.x + threadIdx.x; f < m; f += (long long)gridDim.x * blockDim.x) {
        const long long i = f / pad;
        const int k = (int)(f - i * pad);
        double v = 0.0;
        if (k < n) {
            v = alpha * S[(size_t)i * lds + k];
            if (B) v += beta * B[(size_t)i * ldb + k];
        }
        D[(size_t)i * ldd + k] = v;
    }
}

constexpr int kColRows = 1024;  // rows per partial of the column reductions below

// part[blk][k] = sum over the block's rows of (A[i][k] - theta[k] B[i][k])^2   (B null: A^2)
__global__ __launch_bounds__(256) void k_exact_colnorm2(const double* __restrict__ A, int lda, const double* __restrict__ B,
                                                        int ldb, const double* __restrict__ theta, long long N, int n,
                                                        double* __restrict__ part) {
    const long long i0 = (long long)blockIdx.x * kColRows, i1 = min(N, i0 + kColRows);
    for (int k = threadIdx.x; k < n; k += 256) {
        double s = 0.0;
        for (long long i = i0; i < i1; ++i) {
            double v = A[(size_t)i * lda + k];
            if (B) v -= theta[k] * B[(size_t)i * ldb + k];
            s += v * v;
        }
        part[(size_t)blockIdx.x * n + k] = s;
    }
}

// per block and column: the entry of largest magnitude (the first one on ties), signed
__global__ __launch_bounds__(256) void k_exact_colmaxabs(const double* __restrict__ A, int lda, long long N, int n,
                                                         double* __restrict__ pv) {
    const long long i0 = (long long)blockIdx.x * kColRows, i1 = min(N, i0 + kColRows);
    for (int k = threadIdx.x; k < n; k += 256) {
        double bv = 0.0;
        for (long long i = i0; i < i1; ++i) {
            const double v = A[(size_t)i * lda + k];
            if (fabs(v) > fabs(bv)) bv = v;
        }
        pv[(size_t)blockIdx.x * n + k] = bv;
    }
}

// A[i][k] *= s[k]
__global__ void k_exact_scale_cols(double* __restrict__ A, int lda, long long N, int n, const double* __restrict__ sv) {
    const long long m = N * n;
    for (long long f = blockIdx.x * (long long)blockDim.x + threadIdx.x; f < m; f += (long long)gridDim.x * blockDim.x) {
        const long long i = f / n;
        const int k = (int)(f - i * n);
        A[(size_t)i * lda + k] *= sv[k];
    }
}

unsigned ew_grid(long long n) { return (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, 16384)); }
}  // namespace

void exact_tables(int H, int W, double hx, double hy, std::vector<double>* es, std::vector<double>* el) {
    const double sw = 1.0 / (hx * hx), pw = 1.0 / (hy * hy);
    es->resize(std::max(H, W));
    for (size_t d = 0; d < es->size(); ++d) (*es)[d] = std::exp(-sw * (double)(d * d));
    el->resize(256);
    for (int d = 0; d < 256; ++d) (*el)[d] = std::exp(-pw * (double)(d * d));
}

size_t exact_part_elems(long long N) {
    const long long nb = (N + 255) / 256;
    const long long nsub = std::min<long long>(kMaxSub, std::max<long long>(1, 2048 / nb));
    return (size_t)(nsub * N * 2);
}

hipError_t affinity_product64(hipStream_t s, const ExactPlane& pl, const double* d_X, int ldx, int ncols, double* d_Y,
                              int ldy) {
    if ((long long)pl.H * pl.W <= 0 || ncols <= 0) return hipSuccess;
    if (ldx < ncols || ldy < ncols || pl.es_len < std::max(pl.H, pl.W)) return hipErrorInvalidValue;
    return pl.es_len <= kExactTabLds ? product_tab<true>(s, pl, d_X, ldx, ncols, d_Y, ldy)
                                     : product_tab<false>(s, pl, d_X, ldx, ncols, d_Y, ldy);
}

hipError_t exact_start(hipStream_t s, double* d_X, long long N, int ld, int col0, int ncols, unsigned seed) {
    hipLaunchKernelGGL(k_exact_start, dim3(ew_grid(N * ncols)), dim3(256), 0, s, d_X, N, ld, col0, ncols, seed);
    return hipGetLastError();
}
hipError_t exact_scale2(hipStream_t s, const double* d_X, int ldx, long long N, int b, const double* d_c, const double* d_r,
                        double* d_Z) {
    hipLaunchKernelGGL(k_exact_scale2, dim3(ew_grid(N * b)), dim3(256), 0, s, d_X, ldx, N, b, d_c, d_r, d_Z);
    return hipGetLastError();
}
hipError_t exact_combine(hipStream_t s, const double* d_Y, long long N, int b, const double* d_c, const double* d_r, double* d_A,
                         int lda) {
    hipLaunchKernelGGL(k_exact_combine, dim3(ew_grid(N * b)), dim3(256), 0, s, d_Y, N, b, d_c, d_r, d_A, lda);
    return hipGetLastError();
}
hipError_t exact_recip(hipStream_t s, double* d_v, long long N, double eps) {
    hipLaunchKernelGGL(k_exact_recip, dim3(ew_grid(N)), dim3(256), 0, s, d_v, N, eps);
    return hipGetLastError();
}
hipError_t exact_axpby(hipStream_t s, const double* d_S, int lds, double alpha, const double* d_B, int ldb, double beta,
                       double* d_D, int ldd, long long N, int n, int pad) {
    if (N <= 0 || pad <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_exact_axpby, dim3(ew_grid(N * pad)), dim3(256), 0, s, d_S, lds, alpha, d_B, ldb, beta, d_D, ldd, N, n,
                       pad);
    return hipGetLastError();
}
int exact_col_blocks(long long N) { return (int)((N + kColRows - 1) / kColRows); }
hipError_t exact_colnorm2(hipStream_t s, const double* d_A, int lda, const double* d_B, int ldb, const double* d_theta,
                          long long N, int n, double* d_part) {
    hipLaunchKernelGGL(k_exact_colnorm2, dim3((unsigned)exact_col_blocks(N)), dim3(256), 0, s, d_A, lda, d_B, ldb, d_theta, N, n,
                       d_part);
    return hipGetLastError();
}
hipError_t exact_colmaxabs(hipStream_t s, const double* d_A, int lda, long long N, int n, double* d_pv) {
    hipLaunchKernelGGL(k_exact_colmaxabs, dim3((unsigned)exact_col_blocks(N)), dim3(256), 0, s, d_A, lda, N, n, d_pv);
    return hipGetLastError();
}
hipError_t exact_scale_cols(hipStream_t s, double* d_A, int lda, long long N, int n, const double* d_s) {
    hipLaunchKernelGGL(k_exact_scale_cols, dim3(ew_grid(N * n)), dim3(256), 0, s, d_A, lda, N, n, d_s);
    return hipGetLastError();
}

}  // namespace nlek
