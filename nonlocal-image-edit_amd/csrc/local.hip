// Local adjustments: the pointwise combine of nle_local_combine / nle_apply_local and the chroma blend of nle_local_chroma
// (the rule is stated in include/nle.h).  Every row m = 0 .. M (row 0 the background) carries a whole edit of its own --
// layer weights, residual weight, detail curve, base tone curve -- and the memberships of region.hip blend the rows' results:
//   u_m = q_m > 0 ? (double)q_m : 0;  sigma = u_1 + .. + u_M;  d = sigma > floor ? sigma : floor
//   alpha_m = u_m / d;  alpha_0 = 1 - sigma / d
//   y_m = the detail rule (detail.hip) with row m's parameters, its base term through row m's tone curve where it has one
//   c_m = alpha_m > 0 ? alpha_m y_m : 0;  y = ((c_0 + c_1) + ..) + c_M
// in fp64, sums in ascending m and l, every operation rounded on its own (no fma).  A row without influence on any of a
// thread's pixels is not evaluated (its c_m is the 0 of the rule); a row whose curve is off carries no exp.
// x, the L layers and the M membership planes are read once, all loads in flight together; the planes stay in registers:
// the layers in loops unrolled to LMAX under the uniform guard l < L, the memberships as the fp32 values they were read as
// (alpha_m is formed when row m is reached; the planes move down one register place per row, so that every index is a
// constant: no runtime-indexed array, no scratch).  The rows are a runtime loop, so the instruction stream holds one row
// whatever M is.
// Only the tone curves that are switched on are staged into LDS, NLE_TONE_KNOTS fp64 knots each: dynamic LDS, up to
// 9 x 8200 B = 73.8 KB (the launch goes through launch.h, which raises the limit).
// k_local_chroma is the same blend on a scalar: c = sum over alpha_m > 0 of alpha_m s_m, a' = 128 + c (a - 128), b' alike.
#include <hip/hip_runtime.h>

#include "detail_rule.h"
#include "kernels.h"
#include "launch.h"
#include "nle.h"
#include "plane_combine.h"

// the rule fixes where every rounding happens: a contracted fma would round a product and a sum once instead of twice
#pragma clang fp contract(off)

namespace nlek {

namespace {

struct LocalArgs {
    const float* x;
    const float* layers;
    const float* q;
    const double* knots;  // the active curves' knots, NLE_TONE_KNOTS each, in the order of their slots
    long long layer_stride, q_stride, n;
    int L, M, ncurves;
    double floor;
    LocalRows rows;
};

// y_m of the P pixels: detail.hip's detail_pixels on the values already loaded, with row r's parameters.  CURVE as there;
// the base term passes the row's tone curve when it has one (r.slot >= 0, uniform).
template <int LMAX, bool CURVE, int P>
__device__ __forceinline__ void local_row(const LocalRow& r, const double* wt, int L, const double* sT, const double (&rho)[P],
                                          const Pack<P> (&Y)[LMAX], double (&y)[P]) {
#pragma unroll
    for (int j = 0; j < P; ++j) y[j] = r.w_rho * (CURVE ? detail_remap(r.sigma, r.gain_m1, rho[j]) : rho[j]);
#pragma unroll
    for (int l = 0; l < LMAX; ++l)
        if (l < L) {
            const double wl = wt[l];
            if (l < L - 1) {
#pragma unroll
                for (int j = 0; j < P; ++j) {
                    const double dd = (double)Y[l].v[j];
                    y[j] = y[j] + wl * (CURVE ? detail_remap(r.sigma, r.gain_m1, dd) : dd);
                }
            } else if (r.slot >= 0) {
                const ToneBase base{sT + r.slot * NLE_TONE_KNOTS, r.lo, r.ks};
#pragma unroll
                for (int j = 0; j < P; ++j) y[j] = y[j] + base(wl * (double)Y[l].v[j]);
            } else {
#pragma unroll
                for (int j = 0; j < P; ++j) y[j] = y[j] + wl * (double)Y[l].v[j];
            }
        }
}

template <int LMAX, int P>
__device__ __forceinline__ void local_pixels(const LocalArgs& a, const double* sT, long long i, double (&y)[P]) {
    const int L = a.L, M = a.M;
    Pack<P> X, Y[LMAX];
    Memberships<P> mem;
    X.load(a.x + i);
#pragma unroll
    for (int l = 0; l < LMAX; ++l)
        if (l < L) Y[l].load(a.layers + (long long)l * a.layer_stride + i);
    mem.load(a.q, a.q_stride, M, i);
    mem.prepare(M, a.floor);
    double rho[P];
#pragma unroll
    for (int l = 0; l < LMAX; ++l)
        if (l < L) detail_sum_step(l, Y[l], rho);
#pragma unroll
    for (int j = 0; j < P; ++j) rho[j] = (double)X.v[j] - rho[j];
    for (int m = 0; m <= M; ++m) {
        double al[P], c[P];
#pragma unroll
        for (int j = 0; j < P; ++j) c[j] = 0.0;
        if (mem.next_alpha(m, al)) {
            const LocalRow& r = a.rows.row[m];
            const double* wt = a.rows.wt + m * L;
            double ym[P];
            if (r.curve) local_row<LMAX, true>(r, wt, L, sT, rho, Y, ym);
            else local_row<LMAX, false>(r, wt, L, sT, rho, Y, ym);
#pragma unroll
            for (int j = 0; j < P; ++j) c[j] = al[j] > 0.0 ? al[j] * ym[j] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < P; ++j) y[j] = m == 0 ? c[j] : y[j] + c[j];
    }
}

}  // namespace

// plane_combine.h's skeleton over local_pixels; the 16-byte loads need the three base pointers aligned, and the stride of
// every family of planes that has a second member
template <int OUT, int LMAX>
__global__ __launch_bounds__(256) void k_local_combine(const LocalArgs a, void* __restrict__ out) {
    extern __shared__ double sT[];
    const int nk = a.ncurves * NLE_TONE_KNOTS;
    for (int k = threadIdx.x; k < nk; k += 256) sT[k] = a.knots[k];
    __syncthreads();
    const size_t misaligned =
        ((reinterpret_cast<size_t>(a.layers) | reinterpret_cast<size_t>(a.x) | reinterpret_cast<size_t>(a.q)) & 15) |
        (size_t)(a.L > 1 ? a.layer_stride & 3 : 0) | (size_t)(a.M > 1 ? a.q_stride & 3 : 0);
    combine_planes<OUT>(a.n, misaligned, out, [&a](long long i, auto& y) { local_pixels<LMAX>(a, sT, i, y); });
}

namespace {

struct ChromaArgs {
    const float* a;
    const float* b;
    const float* q;
    float* b_out;
    long long q_stride, n;
    int M;
    double floor;
    double s[kRegionMax + 1];
};

// a' of the P pixels into y (the skeleton stores it); b' is stored here: four pixels only on the skeleton's aligned path,
// whose condition k_local_chroma extends by b_out's own alignment
template <int P>
__device__ __forceinline__ void chroma_pixels(const ChromaArgs& g, long long i, double (&y)[P]) {
    const int M = g.M;
    Pack<P> A, B;
    Memberships<P> mem;
    A.load(g.a + i);
    B.load(g.b + i);
    mem.load(g.q, g.q_stride, M, i);
    mem.prepare(M, g.floor);
    double c[P];
    for (int m = 0; m <= M; ++m) {
        double al[P];
        mem.next_alpha(m, al);
        const double sm = g.s[m];
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const double t = al[j] > 0.0 ? al[j] * sm : 0.0;
            c[j] = m == 0 ? t : c[j] + t;
        }
    }
    float bo[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        y[j] = 128.0 + c[j] * ((double)A.v[j] - 128.0);
        bo[j] = (float)(128.0 + c[j] * ((double)B.v[j] - 128.0));
    }
    if constexpr (P == 4) *reinterpret_cast<float4*>(g.b_out + i) = make_float4(bo[0], bo[1], bo[2], bo[3]);
    else g.b_out[i] = bo[0];
}

}  // namespace

// in place is allowed (a_out == a, b_out == b): a thread reads its pixels before it writes them, and no other thread's
__global__ __launch_bounds__(256) void k_local_chroma(const ChromaArgs g, float* a_out) {
    const size_t misaligned = ((reinterpret_cast<size_t>(g.a) | reinterpret_cast<size_t>(g.b) | reinterpret_cast<size_t>(g.q) |
                                reinterpret_cast<size_t>(g.b_out)) & 15) | (size_t)(g.M > 1 ? g.q_stride & 3 : 0);
    combine_planes<NLE_REGION_OUT_F32>(g.n, misaligned, a_out, [&g](long long i, auto& y) { chroma_pixels(g, i, y); });
}

constexpr int kLocalFewLayers = 4;  // up to here the LMAX = 4 instantiation runs, as for the detail kernels

hipError_t local_combine(hipStream_t s, const float* d_x, const float* d_layers, long long layer_stride, int L, const float* d_q,
                         long long q_stride, int M, long long n, const LocalRows& rows, const double* d_knots, int ncurves,
                         double floor, int out_kind, void* d_out) {
    if (L < 1 || L > kRegionLayersMax || M < 1 || M > kRegionMax || n < 0 || layer_stride < 0 || q_stride < 0 || ncurves < 0 ||
        ncurves > kRegionMax + 1 || (ncurves && !d_knots))
        return hipErrorInvalidValue;
    for (int m = 0; m <= M; ++m)
        if (rows.row[m].slot >= ncurves) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    LocalArgs a;
    a.x = d_x;
    a.layers = d_layers;
    a.q = d_q;
    a.knots = d_knots;
    a.layer_stride = layer_stride;
    a.q_stride = q_stride;
    a.n = n;
    a.L = L;
    a.M = M;
    a.ncurves = ncurves;
    a.floor = floor;
    a.rows = rows;
    const size_t shm = (size_t)ncurves * NLE_TONE_KNOTS * sizeof(double);
    hipError_t e = hipSuccess;
    const hipError_t known = launch_for_out_kind(out_kind, [&](auto out) {
        constexpr int OUT = decltype(out)::value;
        if (L <= kLocalFewLayers) e = launch(k_local_combine<OUT, kLocalFewLayers>, dim3(combine_grid(n)), dim3(256), shm, s, a, d_out);
        else e = launch(k_local_combine<OUT, kRegionLayersMax>, dim3(combine_grid(n)), dim3(256), shm, s, a, d_out);
    });
    return known != hipSuccess ? known : e;
}

hipError_t local_chroma(hipStream_t s, const float* d_a, const float* d_b, const float* d_q, long long q_stride, int M, long long n,
                        const double* saturation, double floor, float* d_a_out, float* d_b_out) {
    if (M < 1 || M > kRegionMax || n < 0 || q_stride < 0) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    ChromaArgs g;
    g.a = d_a;
    g.b = d_b;
    g.q = d_q;
    g.b_out = d_b_out;
    g.q_stride = q_stride;
    g.n = n;
    g.M = M;
    g.floor = floor;
    for (int m = 0; m <= kRegionMax; ++m) g.s[m] = m <= M ? saturation[m] : 0.0;
    return launch(k_local_chroma, dim3(combine_grid(n)), dim3(256), 0, s, g, d_a_out);
}

}  // namespace nlek
