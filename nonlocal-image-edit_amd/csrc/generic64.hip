// The literal decomposition of the hot path with every N-sized matrix in fp64 (gfx950).
//
// Why it exists.  The table formulation (tables.hip / sorted.hip) is all-fp64 but needs an integer-valued luminance plane
// and a sample grid of at most 32 x 36; the fp32 formulations (kernels.hip: Phi, V and the affinities in fp32) miss the
// 1e-4 per-layer bar on some well-posed inputs (profiles/r1_parity_fuzz.txt: detail layers that are small differences
// 1 - lambda at spatial bandwidths of a few pixels).  This file is what auto mode falls back to for any other input
// and what the stage-level API of include/nle/filter.hpp runs on, so that the reference's own unit tests
// (test/test_filter.cpp, tolerance 1e-10) hold unchanged: same stages as the reference, same fp64 arithmetic,
//   k_affinity64      src/filter.cpp:104-112,139-145   Kab(i,j) = exp(negativeWeightedDistance), libm exp
//   k_tsgemm64        :275, :327, :250                  tall-skinny products on v_mfma_f64_16x16x4_f64
//   k_rowpass64       :239,243 + :42-54, :456           phi (D (phi^T r)) with inplaceReciprocal, one pass; V^T x
//   k_gram64d         :296                              Wab Wab^T (its N-sized part) on the fp64 MFMA
//   k_apply_expand64  :456                              V (diag f) (V^T x), as many layers per pass as fit in LDS
// It is a fallback, sized for correctness first: operands come straight from global memory (L2), one wave per 16 x 16
// output tile; N x r fp64 is 26.8 GB at cfg4, which 288 GB of HBM holds comfortably.
#include "kernels.h"
#include "launch.h"

#include <algorithm>

namespace nlek {

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {
__device__ __forceinline__ double recip0_g(double s, double eps) {
    return (fabs(s) >= eps) ? 1.0 / s : 0.0;  // inplaceReciprocal, src/filter.cpp:42-54
}
}  // namespace

// ------------------------------------------------------------------ affinity rows, fp64
// kab[i][s] = exp(-sw (dr^2 + dc^2) - pw (x_i - y_s)^2), natural pixel order, i in [pix0, pix0 + M); columns >= p zero
// (skip_samples != 0: the rows of the sample pixels themselves come out as zeros -- the sample-space algebra sums over
// the non-sample pixels only and treats the samples exactly on its p-sized side)
// A workgroup covers 64 consecutive pixels at a time (one contiguous 64 * ld * 8-byte span), a thread one double2 of one
// pixel's row: 16-byte coalesced stores, 32-bit index arithmetic, the samples (row, col, value as doubles) in LDS.
constexpr int kAff64Pix = 64;

// CHROMA (nle_ctx_set_chroma, radius 0): the samples' (a, b) sit beside their (row, col, L) in LDS, the pixel's a and b are
// loaded once, and the exponent is (-sw d2 - pw dL^2) - cw (da^2 + db^2), every operation rounded on its own (the order of
// the definition in include/nle.h and of build_Ka on the host).  The CHROMA = false instantiation is the kernel as it was.
template <bool CHROMA>
__global__ __launch_bounds__(256) void k_affinity64(const float* __restrict__ lum, GridSpec gs,
                                                    const Sample4* __restrict__ samples, int p, int ld, double sw,
                                                    double pw, long long pix0, long long M, double* __restrict__ kab,
                                                    int skip_samples, const unsigned* __restrict__ smask,
                                                    const float* __restrict__ pa, const float* __restrict__ pb,
                                                    const float2* __restrict__ sab, double cw) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw64[];
    int2* srow_col = reinterpret_cast<int2*>(smem_raw64);                       // [ld]
    double* sval = reinterpret_cast<double*>(smem_raw64 + (size_t)ld * sizeof(int2));  // [ld]
    float2* schroma = reinterpret_cast<float2*>(sval + ld);                     // [ld], CHROMA only
    for (int k = threadIdx.x; k < ld; k += 256) {
        Sample4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < p) v = samples[k];
        srow_col[k] = make_int2((int)v.x, (int)v.y);
        sval[k] = (double)v.z;
        if constexpr (CHROMA) schroma[k] = k < p ? sab[k] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    const unsigned nq = (unsigned)ld >> 1, per_group = kAff64Pix * nq;
    const long long ngroups = (M + kAff64Pix - 1) / kAff64Pix;
    for (long long grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const long long i0 = grp * kAff64Pix;
        double* __restrict__ out = kab + i0 * ld;
        const unsigned nvalid = (unsigned)min((long long)kAff64Pix, M - i0) * nq;
        for (unsigned f = threadIdx.x; f < per_group; f += 256) {
            if (f >= nvalid) break;
            const unsigned il = f / nq, q = f - il * nq;
            const long long gi = pix0 + i0 + il;
            const int row = (int)(gi / gs.W), col = (int)(gi - (long long)row * gs.W);
            const double x = (double)lum[gi];
            const bool zero_row = skip_samples && is_sample(gs, smask, gi, row, col);
            double2 o = make_double2(0.0, 0.0);
            const unsigned s0 = 2 * q;
            if constexpr (CHROMA) {
#pragma clang fp contract(off)
                if (!zero_row) {
                    const float xa = pa[gi], xb = pb[gi];
                    double v[2] = {0.0, 0.0};
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const unsigned s = s0 + e;
                        if (s < (unsigned)p) {
                            const int2 rc = srow_col[s];
                            const float2 ab = schroma[s];
                            const long long dr = row - rc.x, dc = col - rc.y;
                            const double dv = x - sval[s];
                            const double da = (double)(xa - ab.x), db = (double)(xb - ab.y);  // integers: exact
                            const double e0 = -sw * (double)(dr * dr + dc * dc) - pw * (dv * dv);
                            v[e] = exp(e0 - cw * (da * da + db * db));
                        }
                    }
                    o = make_double2(v[0], v[1]);
                }
            } else {
                if (!zero_row) {
                    if (s0 < (unsigned)p) {
                        const int2 rc = srow_col[s0];
                        const long long dr = row - rc.x, dc = col - rc.y;  // integer spatial term (:109)
                        const double dv = x - sval[s0];
                        o.x = exp(-sw * (double)(dr * dr + dc * dc) - pw * (dv * dv));
                    }
                    if (s0 + 1 < (unsigned)p) {
                        const int2 rc = srow_col[s0 + 1];
                        const long long dr = row - rc.x, dc = col - rc.y;
                        const double dv = x - sval[s0 + 1];
                        o.y = exp(-sw * (double)(dr * dr + dc * dc) - pw * (dv * dv));
                    }
                }
            }
            *reinterpret_cast<double2*>(out + (size_t)f * 2) = o;
        }
    }
}

size_t affinity64_chroma_lds_bytes(int ld) { return (size_t)ld * (sizeof(int2) + sizeof(double) + sizeof(float2)); }

namespace {
hipError_t launch_affinity64(hipStream_t s, const Affinity64Args& a, long long pix0, long long M, double* d_kab,
                             bool skip_samples) {
    if (a.ld & 1) return hipErrorInvalidValue;   // rows are written two doubles at a time (ld = nle_ld(p) is a multiple of 4)
    const long long ngroups = (M + kAff64Pix - 1) / kAff64Pix;
    const int grid = (int)std::min<long long>(ngroups, 16384);
    // not through launch(): no template dispatch, and a sample set whose tables pass the default dynamic-LDS allowance is
    // left to fail at the launch as before (ADVICE.md lists the limit as a fix of its own)
    hipLaunchKernelGGL(k_affinity64<false>, dim3((unsigned)grid), dim3(256), (size_t)a.ld * (sizeof(int2) + sizeof(double)), s,
                       a.lum, a.gs, a.samples, a.p, a.ld, a.sw, a.pw, pix0, M, d_kab, skip_samples ? 1 : 0, a.smask, nullptr,
                       nullptr, nullptr, 0.0);
    return hipGetLastError();
}

hipError_t launch_affinity64_chroma(hipStream_t s, const Affinity64Args& a, long long pix0, long long M, double* d_kab,
                                    bool skip_samples) {
    // the launch takes the default dynamic-LDS allowance (the caller refuses a larger sample set with a message)
    if ((a.ld & 1) || a.ld < a.p || !a.a || !a.b || !a.sab || affinity64_chroma_lds_bytes(a.ld) > kDynLdsDefault)
        return hipErrorInvalidValue;
    const long long ngroups = (M + kAff64Pix - 1) / kAff64Pix;
    const int grid = (int)std::min<long long>(ngroups, 16384);
    hipLaunchKernelGGL(k_affinity64<true>, dim3((unsigned)grid), dim3(256), affinity64_chroma_lds_bytes(a.ld), s, a.lum, a.gs,
                       a.samples, a.p, a.ld, a.sw, a.pw, pix0, M, d_kab, skip_samples ? 1 : 0, a.smask, a.a, a.b, a.sab, a.cw);
    return hipGetLastError();
}
}  // namespace

// the R > 0 half of the launcher below, next to its kernels in patch.hip; declared here and not in kernels.h: nothing else
// calls it
hipError_t patch_affinity_rows64(hipStream_t s, const Affinity64Args& a, long long pix0, long long M, double* d_kab,
                                 bool skip_samples);
// the one launcher of the fp64 affinity rows: R > 0 goes to patch.hip, chroma (both planes given) to the CHROMA forms
hipError_t affinity_rows64(hipStream_t s, const Affinity64Args& a, long long pix0, long long M, double* d_kab,
                           bool skip_samples) {
    if (M <= 0) return hipSuccess;
    if (a.R > 0) return patch_affinity_rows64(s, a, pix0, M, d_kab, skip_samples);
    return a.a ? launch_affinity64_chroma(s, a, pix0, M, d_kab, skip_samples)
               : launch_affinity64(s, a, pix0, M, d_kab, skip_samples);
}

// y[i] += x[i]
__global__ void k_add64(double* __restrict__ y, const double* __restrict__ x, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) y[i] += x[i];
}
hipError_t add64(hipStream_t s, double* d_y, const double* d_x, size_t n) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_add64, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, s, d_y, d_x, n);
    return hipGetLastError();
}

// ------------------------------------------------------------------ per-row scalings
// out[i] = recip(X_i . u)  (one wave per row)
__global__ __launch_bounds__(256) void k_row_scalings64(const double* __restrict__ X, long long M, int ld, int r,
                                                        const double* __restrict__ u, double eps, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long wv = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long long)gridDim.x * 4;
    for (long long i = wv; i < M; i += nw) {
        double s = 0.0;
        for (int j = lane; j < r; j += 64) s += X[(size_t)i * ld + j] * u[j];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if (lane == 0) out[i] = recip0_g(s, eps);
    }
}

hipError_t row_scalings64(hipStream_t s, const double* d_X, long long M, int ld, int r, const double* d_u, double eps,
                          double* d_out) {
    if (M <= 0) return hipSuccess;
    const long long nb = std::min<long long>((M + 3) / 4, 8192);
    hipLaunchKernelGGL(k_row_scalings64, dim3((unsigned)nb), dim3(256), 0, s, d_X, M, ld, r, d_u, eps, d_out);
    return hipGetLastError();
}

// ------------------------------------------------------------------ tall-skinny product on the fp64 MFMA
// C (M x ldc, columns < nc) = diag(rs) A (M x lda, logical width kd) B (kd x nc, COLUMN-major, leading dimension kd)
// rs: optional per-row scale (null: 1).  One wave per 16 rows x 16 columns; v_mfma_f64_16x16x4_f64: lane (l15, kq)
// feeds A[row l15][k kq] and B[k kq][col l15] and receives rows kq + 4 e of column l15.
__global__ __launch_bounds__(256) void k_tsgemm64(const double* __restrict__ A, long long M, int lda, int kd,
                                                  const double* __restrict__ B, int nc, const double* __restrict__ rs,
                                                  double* __restrict__ C, int ldc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, kq = lane >> 4;
    const int ctiles = (nc + 15) / 16;
    const long long rtiles = (M + 15) / 16, ntiles = rtiles * ctiles;
    for (long long t = (long long)blockIdx.x * 4 + wave; t < ntiles; t += (long long)gridDim.x * 4) {
        const long long rt = t / ctiles;
        const int ct = (int)(t - rt * ctiles);
        const long long arow = rt * 16 + l15;
        const int bcol = ct * 16 + l15;
        const bool aok = arow < M, bok = bcol < nc;
        f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < kd; k0 += 4) {
            const int k = k0 + kq;
            const double a = (aok && k < kd) ? A[(size_t)arow * lda + k] : 0.0;
            const double b = (bok && k < kd) ? B[(size_t)bcol * kd + k] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
        if (bok) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long long ro = rt * 16 + kq + 4 * e;
                if (ro < M) C[(size_t)ro * ldc + bcol] = (rs ? rs[ro] : 1.0) * acc[e];
            }
        }
    }
}

hipError_t ts_gemm64(hipStream_t s, const double* d_A, long long M, int lda, int kd, const double* d_B, int nc,
                     const double* d_rs, double* d_C, int ldc) {
    if (M <= 0 || nc <= 0) return hipSuccess;
    const long long ntiles = ((M + 15) / 16) * ((nc + 15) / 16);
    const long long nb = std::min<long long>((ntiles + 3) / 4, 65535);
    hipLaunchKernelGGL(k_tsgemm64, dim3((unsigned)nb), dim3(256), 0, s, d_A, M, lda, kd, d_B, nc, d_rs, d_C, ldc);
    return hipGetLastError();
}

// ------------------------------------------------------------------ small dense products (p-, q-sized), fp64 MFMA
// C(i,j) = dl[i] (sum_k A(i,k) dk[k] B(k,j)) dr[j] + add(i,j), every matrix given by (pointer, row stride, column
// stride) so that transposes, sub-blocks and row- or column-major outputs need no copies; dl, dk, dr, add optional.
// One wave per 16 x 16 tile of C.  These products are latency-bound (a 200^3 one is 16 MFLOP): what a tile costs is
// the number of dependent memory round trips, so the k range is cut into windows of kGemm64sWin k, every a/b (and dk)
// operand of a window is loaded into registers before its MFMA chain starts, and the next window's loads are issued
// before the current window's MFMAs.  Two windows are therefore in flight together: kk <= 2 kGemm64sWin (cfg4:
// kk <= 200) is ONE round trip, kk = 900 five instead of 57.  The epilogue's dl / dr / add are loaded up front too.
// Register budget: a workgroup is 4 waves, one per SIMD, so a wave may use the SIMD's whole file (512 registers);
// two windows hold 2 x 32 steps x (a, b, dk) x 2 registers = 384 (256 without dk).  No scratch.
// It runs where a tile's latency is what the product costs: up to kGemm64sWindowedMaxTiles output tiles (one workgroup per
// CU); larger outputs take k_gemm64s_stream below.  A launch with kk well under a window still issues the whole first
// window's loads (the lanes past kk re-read k = 0): kk = 32 costs ~3 us more than in the streaming form.
// Arithmetic is what the four-steps-at-a-time loop does: k ascending in one accumulator chain, a scaled by dk
// before the MFMA, MFMA steps issued in groups of four up to the first group that starts at k >= kk, operands of
// k >= kk (and of rows / columns outside the matrix) exactly 0.  Out-of-range lanes load from a clamped, valid
// address and select 0 afterwards (a load under a per-element condition would be waited for one by one).
constexpr int kGemm64sWinSteps = 32;                    // MFMA steps (of 4 k) per window
constexpr int kGemm64sWin = 4 * kGemm64sWinSteps;       // k per window
constexpr int kGemm64sWindowedMaxTiles = 4 * 256;       // output tiles up to which the windowed kernel runs: one workgroup per CU

namespace {
template <bool HAS_DK>
struct Gemm64sWindow {
    double a[kGemm64sWinSteps], b[kGemm64sWinSteps], d[HAS_DK ? kGemm64sWinSteps : 1];
    // issues the loads of k in [k0, k0 + kGemm64sWin); kq = this lane's k within a step; kk >= 1.  The lane's pointers
    // advance four k at a time (one add each: a product per load would cost more than the loads); a lane past the
    // end reads k = 0 instead
    __device__ __forceinline__ void load(const double* __restrict__ ap, long long csA, const double* __restrict__ bp,
                                         long long rsB, const double* __restrict__ dk, int k0, int kq, int kk) {
        const double* pa = ap + (long long)(k0 + kq) * csA;
        const double* pb = bp + (long long)(k0 + kq) * rsB;
        const double* pd = dk + (k0 + kq);
#pragma unroll
        for (int u = 0; u < kGemm64sWinSteps; ++u) {
            const bool kok = k0 + 4 * u + kq < kk;
            a[u] = *(kok ? pa : ap);
            b[u] = *(kok ? pb : bp);
            if constexpr (HAS_DK) d[u] = *(kok ? pd : dk);
            pa += 4 * csA;
            pb += 4 * rsB;
            pd += 4;
        }
    }
    // the window's MFMA chain, in groups of four steps like the loop it replaces (a group that starts at k >= kk is
    // not issued: wave-uniform)
    __device__ __forceinline__ void mfma(f64x4& acc, int k0, int kq, int kk, bool aok, bool bok) const {
#pragma unroll
        for (int g = 0; g < kGemm64sWinSteps / 4; ++g) {
            if (k0 + 16 * g >= kk) break;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int u = 4 * g + v;
                const bool kok = k0 + 4 * u + kq < kk;
                double av = a[u];
                if constexpr (HAS_DK) av *= d[u];
                av = (aok && kok) ? av : 0.0;
                const double bv = (bok && kok) ? b[u] : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
            }
        }
    }
};
}  // namespace

template <bool HAS_DK>
__global__ __launch_bounds__(256) void k_gemm64s(int m, int n, int kk, const double* __restrict__ A, long long rsA,
                                                 long long csA, const double* __restrict__ B, long long rsB, long long csB,
                                                 double* C, long long rsC, long long csC, const double* __restrict__ dl,
                                                 const double* __restrict__ dk, const double* __restrict__ dr,
                                                 const double* add, long long rsD, long long csD) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, kq = lane >> 4;
    const int ct = (n + 15) / 16, rt = (m + 15) / 16;
    const int t = blockIdx.x * 4 + wave;
    if (t >= rt * ct) return;  // wave-uniform
    const int ti = t / ct, tj = t - ti * ct;
    const int ai = ti * 16 + l15, bj = tj * 16 + l15;
    const bool aok = ai < m, bok = bj < n;
    const int bjc = min(bj, n - 1);
    const double* ap = A + (long long)min(ai, m - 1) * rsA;
    const double* bp = B + (long long)bjc * csB;
    Gemm64sWindow<HAS_DK> w0, w1;
    if (kk > 0) w0.load(ap, csA, bp, rsB, dk, 0, kq, kk);
    if (kk > kGemm64sWin) w1.load(ap, csA, bp, rsB, dk, kGemm64sWin, kq, kk);
    // the epilogue's operands, in flight with the first windows (add may be C itself: an entry is read and written by
    // one lane only).  An absent operand is loaded from a valid address (C: m, n >= 1) and replaced afterwards: a branch round the
    // load would put a full wait behind it
    const double srv = *(dr ? dr + bjc : C);
    const double sr = dr ? srv : 1.0;
    double sl[4], ad[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int roc = min(ti * 16 + kq + 4 * e, m - 1);
        const double slv = *(dl ? dl + roc : C);
        const double adv = *(add ? add + ((long long)roc * rsD + (long long)bjc * csD) : C);
        sl[e] = dl ? slv : 1.0;
        ad[e] = adv;
    }
    f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < kk; k0 += 2 * kGemm64sWin) {
        w0.mfma(acc, k0, kq, kk, aok, bok);
        if (k0 + 2 * kGemm64sWin < kk) w0.load(ap, csA, bp, rsB, dk, k0 + 2 * kGemm64sWin, kq, kk);
        if (k0 + kGemm64sWin < kk) {
            w1.mfma(acc, k0 + kGemm64sWin, kq, kk, aok, bok);
            if (k0 + 3 * kGemm64sWin < kk) w1.load(ap, csA, bp, rsB, dk, k0 + 3 * kGemm64sWin, kq, kk);
        }
    }
    if (bok) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ro = ti * 16 + kq + 4 * e;
            if (ro < m) {
                double v = sl[e] * acc[e] * sr;
                if (add) v += ad[e];
                C[(long long)ro * rsC + (long long)bj * csC] = v;
            }
        }
    }
}

// The same product for outputs of many tiles: four MFMA steps' operands in flight per wave, few registers, up to eight
// waves per SIMD.  Beyond about one workgroup per CU the product is bound by throughput, not by one tile's latency, and
// the windowed kernel's one wave per SIMD loses (m = n = 800 .. 900: measured ~30 % slower).  Same arithmetic, same bits.
__global__ __launch_bounds__(256) void k_gemm64s_stream(int m, int n, int kk, const double* __restrict__ A, long long rsA,
                                                        long long csA, const double* __restrict__ B, long long rsB,
                                                        long long csB, double* C, long long rsC, long long csC,
                                                        const double* __restrict__ dl, const double* __restrict__ dk,
                                                        const double* __restrict__ dr, const double* add, long long rsD,
                                                        long long csD) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, kq = lane >> 4;
    const int ct = (n + 15) / 16, rt = (m + 15) / 16;
    const int t = blockIdx.x * 4 + wave;
    if (t >= rt * ct) return;  // wave-uniform
    const int ti = t / ct, tj = t - ti * ct;
    const int ai = ti * 16 + l15, bj = tj * 16 + l15;
    const bool aok = ai < m, bok = bj < n;
    const double* ap = A + (long long)ai * rsA;
    const double* bp = B + (long long)bj * csB;
    f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < kk; k0 += 16) {
        double a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 4 * u + kq;
            const bool kok = k < kk;
            a[u] = (aok && kok) ? ap[(long long)k * csA] * (dk ? dk[k] : 1.0) : 0.0;
            b[u] = (bok && kok) ? bp[(long long)k * rsB] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
    }
    if (bok) {
        const double sr = dr ? dr[bj] : 1.0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ro = ti * 16 + kq + 4 * e;
            if (ro < m) {
                double v = (dl ? dl[ro] : 1.0) * acc[e] * sr;
                if (add) v += add[(long long)ro * rsD + (long long)bj * csD];
                C[(long long)ro * rsC + (long long)bj * csC] = v;
            }
        }
    }
}

int gemm64s_window() { return kGemm64sWin; }

hipError_t gemm64s(hipStream_t s, int m, int n, int kk, const double* A, long long rsA, long long csA, const double* B,
                   long long rsB, long long csB, double* C, long long rsC, long long csC, const double* dl, const double* dk,
                   const double* dr, const double* add, long long rsD, long long csD) {
    if (m <= 0 || n <= 0) return hipSuccess;
    const long long ntiles = (long long)((m + 15) / 16) * ((n + 15) / 16);
    const dim3 grid((unsigned)((ntiles + 3) / 4));
    if (ntiles > kGemm64sWindowedMaxTiles)
        hipLaunchKernelGGL(k_gemm64s_stream, grid, dim3(256), 0, s, m, n, kk, A, rsA, csA, B, rsB, csB, C, rsC, csC, dl, dk, dr,
                           add, rsD, csD);
    else if (dk)
        hipLaunchKernelGGL(k_gemm64s<true>, grid, dim3(256), 0, s, m, n, kk, A, rsA, csA, B, rsB, csB, C, rsC, csC, dl, dk, dr,
                           add, rsD, csD);
    else
        hipLaunchKernelGGL(k_gemm64s<false>, grid, dim3(256), 0, s, m, n, kk, A, rsA, csA, B, rsB, csB, C, rsC, csC, dl, dk, dr,
                           add, rsD, csD);
    return hipGetLastError();
}

// ------------------------------------------------------------------ one pass over X (M x ld fp64)
// partial[b][j] = sum over the rows of block b of X[i][j] y_i;  COLSUM: y = 1;  RECIP: y_i = recip(X_i . (lam o t_in));
// XVEC: y_i = xvec[i].  One wave per row at a time; lane l owns columns l, l + 64, ... (<= kRp64Cols per lane).
// ld is the row stride of X only: columns >= w (the logical width) are never loaded, so whatever they hold -- NaN
// included -- stays out of the sums.  t_in, lam and the rows of partial have lw = (w + 3) & ~3 entries, those >= w zero.
constexpr int kRp64Cols = 32;  // w <= 2048

template <int NCL>  // columns per lane: w <= 64 NCL
__global__ __launch_bounds__(256) void k_rowpass64(int mode, const double* __restrict__ X, long long M, int ld, int w, int lw,
                                                   const double* __restrict__ t_in, const double* __restrict__ lam,
                                                   const float* __restrict__ xvec, double eps, double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* sred = reinterpret_cast<double*>(smem_raw);  // [4][lw]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double u[NCL], acc[NCL];
#pragma unroll
    for (int k = 0; k < NCL; ++k) {
        const int j = lane + 64 * k;
        u[k] = (mode == ROWPASS_RECIP && j < w) ? lam[j] * t_in[j] : 0.0;
        acc[k] = 0.0;
    }
    const long long wv = (long long)blockIdx.x * 4 + wave, nw = (long long)gridDim.x * 4;
    for (long long i = wv; i < M; i += nw) {
        double v[NCL];
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < NCL; ++k) {
            const int j = lane + 64 * k;
            v[k] = (j < w) ? X[(size_t)i * ld + j] : 0.0;
            s += v[k] * u[k];
        }
        double y = 1.0;
        if (mode == ROWPASS_RECIP) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
            y = recip0_g(s, eps);
        } else if (mode == ROWPASS_XVEC) {
            y = (double)xvec[i];
        }
#pragma unroll
        for (int k = 0; k < NCL; ++k) acc[k] += v[k] * y;
    }
#pragma unroll
    for (int k = 0; k < NCL; ++k) {
        const int j = lane + 64 * k;
        if (j < lw) sred[wave * lw + j] = acc[k];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < lw; j += 256)
        partial[(size_t)blockIdx.x * lw + j] = (sred[j] + sred[lw + j]) + (sred[2 * lw + j] + sred[3 * lw + j]);
}

hipError_t rowpass64(hipStream_t s, int mode, const double* d_X, long long M, int ld, int w, const double* d_t_in,
                     const double* d_lam, const float* d_xvec, double eps, double* d_partial, int* nblocks) {
    if (w < 1 || w > ld || w > 64 * kRp64Cols) return hipErrorInvalidValue;
    const int lw = (w + 3) & ~3;
    long long nb = (M + 3) / 4;
    nb = std::max<long long>(1, std::min<long long>(nb, kRowpassMaxBlocks));
    *nblocks = (int)nb;
    const size_t shm = (size_t)4 * lw * sizeof(double);
    int ncl = 1;  // columns per lane: the smallest power of two that covers lw, at most kRp64Cols by the check on w above
    while (64 * ncl < lw) ncl *= 2;
    hipError_t e = hipErrorInvalidValue;
    dispatch_values<1, 2, 4, 8, 16, 32>(ncl, [&](auto nclv) {
        e = launch(k_rowpass64<decltype(nclv)::value>, dim3((unsigned)nb), dim3(256), shm, s, mode, d_X, M, ld, w, lw, d_t_in, d_lam,
                   d_xvec, eps, d_partial);
    });
    return e;
}

// ------------------------------------------------------------------ Gram on the fp64 MFMA
// G (r x r, full, column-major == row-major: symmetric) = sum_i c_i^2 x_i x_i^T, c_i = cs[i] (null: 1).
// grid (upper-triangular 16 x 16 tile pairs, row chunks); partial[chunk][r*r]; a second kernel sums the chunks in order
// and mirrors the triangle.
__global__ __launch_bounds__(256) void k_gram64d(const double* __restrict__ X, long long M, int ld, int r,
                                                 const double* __restrict__ cs, long long rows_per_chunk,
                                                 double* __restrict__ partial) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, kq = lane >> 4;
    const int nt = (r + 15) / 16;
    // tile pair index -> (ti <= tj)
    int t = blockIdx.x * 4 + wave;
    const int npairs = nt * (nt + 1) / 2;
    if (t >= npairs) return;  // wave-uniform
    int ti = 0;
    while (t >= nt - ti) {
        t -= nt - ti;
        ++ti;
    }
    const int tj = ti + t;
    const long long i0 = (long long)blockIdx.y * rows_per_chunk, i1 = min(M, i0 + rows_per_chunk);
    const int ca = ti * 16 + l15, cb = tj * 16 + l15;
    f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
    for (long long i = i0; i < i1; i += 4) {
        const long long row = i + kq;
        const bool ok = row < i1;
        const double c = ok ? (cs ? cs[row] : 1.0) : 0.0;
        const double a = (ok && ca < r) ? c * X[(size_t)row * ld + ca] : 0.0;
        const double b = (ok && cb < r) ? c * X[(size_t)row * ld + cb] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
    double* out = partial + (size_t)blockIdx.y * r * r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int ra = ti * 16 + kq + 4 * e;
        if (ra < r && cb < r) out[(size_t)cb * r + ra] = acc[e];  // entry (ra, cb), ra in tile ti, cb in tile tj
    }
}

__global__ void k_gram64d_reduce(const double* __restrict__ partial, int nchunks, int r, double* __restrict__ G) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)r * r) return;
    const int a = (int)(idx % r), b = (int)(idx / r);       // column-major (a, b)
    const int ta = a / 16, tb = b / 16;
    // the kernel above wrote entry (ra, cb) for tiles ti <= tj only: read the mirrored entry below the tile diagonal
    const size_t src = (ta <= tb) ? (size_t)b * r + a : (size_t)a * r + b;
    double s = 0.0;
    for (int c = 0; c < nchunks; ++c) s += partial[(size_t)c * r * r + src];
    G[idx] = s;
}

long long gram64d_chunk_rows(long long M) {
    long long rows = (M + 255) / 256;  // up to 256 chunks
    rows = std::max<long long>(((rows + 3) / 4) * 4, 256);
    return rows;
}
size_t gram64d_partial_elems(long long M, int r) {
    const long long rows = gram64d_chunk_rows(M);
    const long long nchunks = std::max<long long>(1, (M + rows - 1) / rows);
    return (size_t)nchunks * r * r;
}

hipError_t gram64d(hipStream_t s, const double* d_X, long long M, int ld, int r, const double* d_cs, double* d_partial,
                   double* d_G) {
    const long long rows = gram64d_chunk_rows(M);
    const int nchunks = (int)std::max<long long>(1, (M + rows - 1) / rows);
    const int nt = (r + 15) / 16, npairs = nt * (nt + 1) / 2;
    hipError_t e = hipMemsetAsync(d_partial, 0, (size_t)nchunks * r * r * sizeof(double), s);
    if (e != hipSuccess) return e;
    if (M > 0)
        hipLaunchKernelGGL(k_gram64d, dim3((unsigned)((npairs + 3) / 4), (unsigned)nchunks), dim3(256), 0, s, d_X, M, ld, r, d_cs,
                           rows, d_partial);
    hipLaunchKernelGGL(k_gram64d_reduce, dim3((unsigned)(((long long)r * r + 255) / 256)), dim3(256), 0, s, d_partial, nchunks, r,
                       d_G);
    return hipGetLastError();
}

// ------------------------------------------------------------------ apply, expand half: Y[l][i] = V_i . g_l
__global__ __launch_bounds__(256) void k_apply_expand64(const double* __restrict__ V, long long M, int ld, int K,
                                                        const double* __restrict__ g, int L, float* __restrict__ Y,
                                                        long long ystride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* sg = reinterpret_cast<double*>(smem_raw);  // [L][K]
    for (int j = threadIdx.x; j < L * K; j += 256) sg[j] = g[(size_t)(j / K) * ld + (j % K)];
    __syncthreads();
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < M; i += (long long)gridDim.x * 256) {
        const double* v = V + (size_t)i * ld;
        for (int l = 0; l < L; ++l) {
            double s0 = 0.0, s1 = 0.0;
            int k = 0;
            for (; k + 1 < K; k += 2) {
                s0 += v[k] * sg[l * K + k];
                s1 += v[k + 1] * sg[l * K + k + 1];
            }
            if (k < K) s0 += v[k] * sg[l * K + k];
            Y[(size_t)l * ystride + i] = (float)(s0 + s1);
        }
    }
}

// The [L][K] table of a launch lives in LDS: the layers go out in equal groups whose table fits kApplyLdsBytes (64 KiB,
// two workgroups per CU; one layer at K = 2048 is 16 KiB, so a group always exists).  Every layer is summed in the same
// order whatever group it lands in.
hipError_t apply_expand64(hipStream_t s, const double* d_V, long long M, int ld, int K, const double* d_g, int L, float* d_Y,
                          long long ystride) {
    if (M <= 0 || L <= 0) return hipSuccess;
    const size_t per_layer = (size_t)K * sizeof(double);
    if (per_layer > kApplyLdsBytes) return hipErrorInvalidValue;
    const int lmax = per_layer ? (int)std::min<size_t>(kApplyLdsBytes / per_layer, (size_t)L) : L;
    const int ngroups = (L + lmax - 1) / lmax, lg = (L + ngroups - 1) / ngroups;
    const long long nb = std::min<long long>((M + 255) / 256, 4096);
    hipError_t e = hipSuccess;
    for (int l0 = 0; l0 < L && e == hipSuccess; l0 += lg) {
        const int ln = std::min(lg, L - l0);
        e = launch(k_apply_expand64, dim3((unsigned)nb), dim3(256), (size_t)ln * per_layer, s, d_V, M, ld, K, d_g + (size_t)l0 * ld, ln,
                   d_Y + (size_t)l0 * ystride, ystride);
    }
    return e;
}

// X[idx[k]][0..ld) = src[k][0..ld)
__global__ void k_scatter_rows64(const double* __restrict__ src, const long long* __restrict__ idx, int n, int ld,
                                 double* __restrict__ X, long long M) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= (long long)n * ld) return;
    const int k = (int)(f / ld), j = (int)(f % ld);
    const long long row = idx[k];
    if (row >= 0 && row < M) X[(size_t)row * ld + j] = src[f];
}

hipError_t scatter_rows64(hipStream_t s, const double* d_src, const long long* d_idx, int n, int ld, double* d_X, long long M) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_scatter_rows64, dim3((unsigned)(((long long)n * ld + 255) / 256)), dim3(256), 0, s, d_src, d_idx, n, ld,
                       d_X, M);
    return hipGetLastError();
}

// Y(i, j) = X[j m + i] dl[i]: X m x n column-major (leading dimension m), Y in any layout (row stride, column stride)
__global__ void k_scale_rows64_to(const double* __restrict__ X, int m, int n, const double* __restrict__ dl,
                                  double* __restrict__ Y, long long rsY, long long csY) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= (long long)m * n) return;
    const int i = (int)(f % m), j = (int)(f / m);
    Y[i * rsY + j * csY] = X[f] * dl[i];
}
hipError_t scale_rows64_to(hipStream_t s, const double* d_X, int m, int n, const double* d_dl, double* d_Y, long long rsY,
                           long long csY) {
    if (m <= 0 || n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_scale_rows64_to, dim3((unsigned)(((long long)m * n + 255) / 256)), dim3(256), 0, s, d_X, m, n, d_dl, d_Y,
                       rsY, csY);
    return hipGetLastError();
}

// out[i] = (float) X[i]  (nle_filter_eigvecs of an fp64 filter)
__global__ void k_to_f32(const double* __restrict__ X, long long n, float* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        out[i] = (float)X[i];
}
hipError_t to_f32(hipStream_t s, const double* d_X, long long n, float* d_out) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_to_f32, dim3((unsigned)std::min<long long>((n + 255) / 256, 8192)), dim3(256), 0, s, d_X, n, d_out);
    return hipGetLastError();
}

}  // namespace nlek
