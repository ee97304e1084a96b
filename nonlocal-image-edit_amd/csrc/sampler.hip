// Farthest-point sample selection (opt-in NLE_SAMPLER_FARTHEST, nle_ctx_set_sampler): p samples chosen greedily by the
// monotone argument of the affinity instead of the reference's Cartesian grid (src/filter.cpp:56-80).
//
//   D(i, j) = sw (double)(dr^2 + dc^2) + pw (dy^2),  sw = 1/hx^2, pw = 1/hy^2, dr dc int64, dy = (double)y_i - (double)y_j
//   s_0 = (H/2, W/2);  m_i = min over the chosen samples s of D(i, s), and -1 for a chosen pixel;
//   s_k = argmax_i m_i, ties to the smallest row-major index.
//
// One launch per round, the kernel boundary the only synchronisation (no workgroup ever waits for another).  Launch k:
// every workgroup reduces the previous launch's per-workgroup partials (m value, index) in the same fixed order -- max
// with smallest-index ties is associative and commutative, so all of them find the same s_k and workgroup 0 appends it to
// the device list -- then updates m over its pixels in fp64 (launch 0 initialises it from s_0) and writes its own
// partial.  The partials are double-buffered by round parity: a launch reads one buffer and writes the other.  Per round
// and pixel: 4 bytes of the plane, 8 bytes of m read and 8 written.
#include "kernels.h"

#include <algorithm>
#include <climits>
#include <cstdint>

namespace nlek {

namespace {
constexpr int kFpsThreads = 256;
constexpr int kFpsMaxBlocks = 2048;

__device__ __forceinline__ void fps_take(double& bv, int& bi, double v, int i) {
    if (v > bv || (v == bv && i < bi)) {
        bv = v;
        bi = i;
    }
}

// argmax over the workgroup (smallest index on ties), the same in every thread
__device__ void fps_block_argmax(double& bv, int& bi) {
    __shared__ double sv[kFpsThreads / 64];
    __shared__ int si[kFpsThreads / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        fps_take(bv, bi, ov, oi);
    }
    if ((threadIdx.x & 63) == 0) {
        sv[threadIdx.x >> 6] = bv;
        si[threadIdx.x >> 6] = bi;
    }
    __syncthreads();
    bv = sv[0];
    bi = si[0];
#pragma unroll
    for (int w = 1; w < kFpsThreads / 64; ++w) fps_take(bv, bi, sv[w], si[w]);
    __syncthreads();  // the slots are reused by the next call
}

// the new running minimum of pixel i (row r, column c, value y) after sample s = (sr, sc, ys) of round `round`
__device__ __forceinline__ double fps_update(const double* __restrict__ m, int i, int r, int c, float y, int s, int sr, int sc,
                                             double ys, double sw, double pw, int round) {
    // in exactly the stated order: a contracted fma would round sw d2 + pw dy^2 once instead of twice
#pragma clang fp contract(off)
    const long long dr = r - sr, dc = c - sc;
    const double dy = (double)y - ys;
    const double d = sw * (double)(dr * dr + dc * dc) + pw * (dy * dy);
    double v = d;
    if (round > 0) {
        const double o = m[i];
        v = d < o ? d : o;
    }
    return i == s ? -1.0 : v;
}

// VEC: the plane is 16-byte aligned and pixels go four at a time (float4 of y, two double2 of m); the N % 4 last pixels
// and the unaligned case go one at a time
template <bool VEC>
__global__ __launch_bounds__(kFpsThreads) void k_farthest_round(const float* __restrict__ lum, int W, int N, double sw,
                                                                 double pw, int round, int s0, int last,
                                                                 const double* __restrict__ pv_in,
                                                                 const int* __restrict__ pi_in, double* __restrict__ m,
                                                                 double* __restrict__ pv_out, int* __restrict__ pi_out,
                                                                 int* __restrict__ list) {
    int s = s0;
    if (round > 0) {
        double bv = -2.0;
        int bi = INT_MAX;
        for (int k = threadIdx.x; k < (int)gridDim.x; k += kFpsThreads) fps_take(bv, bi, pv_in[k], pi_in[k]);
        fps_block_argmax(bv, bi);
        s = min(bi, N - 1);  // bi is INT_MAX only if no m compared (a plane of NaNs): stay in bounds
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) list[round] = s;
    if (last) return;
    const int sr = s / W, sc = s - sr * W;
    const double ys = (double)lum[s];
    double bv = -2.0;
    int bi = INT_MAX;
    const unsigned stride = gridDim.x * kFpsThreads;
    unsigned tail0 = 0;
    if (VEC) {
        const unsigned nq = (unsigned)N >> 2;
        for (unsigned q = blockIdx.x * kFpsThreads + threadIdx.x; q < nq; q += stride) {
            const int i0 = (int)(q << 2);
            int r = i0 / W, c = i0 - r * W;
            const float4 y4 = *reinterpret_cast<const float4*>(lum + i0);
            const float ys4[4] = {y4.x, y4.y, y4.z, y4.w};
            double v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = fps_update(m, i0 + j, r, c, ys4[j], s, sr, sc, ys, sw, pw, round);
                if (++c == W) {
                    c = 0;
                    ++r;
                }
            }
            *reinterpret_cast<double2*>(m + i0) = make_double2(v[0], v[1]);
            *reinterpret_cast<double2*>(m + i0 + 2) = make_double2(v[2], v[3]);
#pragma unroll
            for (int j = 0; j < 4; ++j) fps_take(bv, bi, v[j], i0 + j);
        }
        tail0 = nq << 2;
    }
    for (unsigned i = tail0 + blockIdx.x * kFpsThreads + threadIdx.x; i < (unsigned)N; i += stride) {
        const int r = (int)i / W, c = (int)i - r * W;
        const double v = fps_update(m, (int)i, r, c, lum[i], s, sr, sc, ys, sw, pw, round);
        m[i] = v;
        fps_take(bv, bi, v, (int)i);
    }
    fps_block_argmax(bv, bi);
    if (threadIdx.x == 0) {
        pv_out[blockIdx.x] = bv;
        pi_out[blockIdx.x] = bi;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// Residual-greedy selection (opt-in NLE_SAMPLER_RESIDUAL): Cholesky with diagonal pivoting on the N x N affinity, the rule
// of include/nle.h.  Same model as above: one launch per round, the kernel boundary the only synchronisation.  Launch k of
// k_residual_round<VEC>:
//   pick (resid_pick, repeated by every workgroup as k_farthest_round repeats its reduction)  folds the partials launch
//       k - 1 left, in a fixed order, decides residual round / fallback from them and from the state launch k - 1 left,
//       finds s_k and its pivot, and gathers the row l_j[s_k], j < k, of the factor into LDS; workgroup 0 appends s_k and
//       the pivot to the lists and writes the state {fallen back, n_residual, statistics} for launch k + 1;
//   pixels  column k of the factor for the workgroup's pixels (the row broadcast from LDS, the columns l_j[i] streamed
//       coalesced, 4 pixels = 4 independent accumulators per thread), d and m updated, and the workgroup's partials: (max d,
//       index) over the pixels not chosen, (max m, index), sum max(d, 0).  After the fallback: the farthest-point update
//       of m alone.
// Partials and state are double-buffered by round parity: a launch reads one buffer and writes the other.
// Per residual round k and pixel: 8 k bytes of the factor read and 8 written, 16 for d, 16 for m, 4 of the plane.
// (A one-workgroup pick launch in front of every pixel launch, which writes the row and the state once, was measured
// against this: equal at 4096^2 and 2048^2, 5 % slower at 512^2 -- DESIGN.md section 3.12.)
constexpr int kResidRowMax = kResidMaxSamples;  // the row in LDS: 16 KB
// the state a launch hands to the next (kResidHead doubles): fallen back (0 / 1), n_residual, then the statistics after the
// last residual round: max d over the pixels not chosen, its first index, sum max(d, 0)
enum { kStFallen = 0, kStResidual = 1, kStMax = 2, kStArg = 3, kStSum = 4 };

// sum over the workgroup in a fixed order, the same in every thread
__device__ double resid_block_sum(double v) {
    __shared__ double ss[kFpsThreads / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) ss[threadIdx.x >> 6] = v;
    __syncthreads();
    v = ss[0];
#pragma unroll
    for (int w = 1; w < kFpsThreads / 64; ++w) v += ss[w];
    __syncthreads();
    return v;
}

// The pick of round `round`, the same in every workgroup: s_k, the square root of its pivot and whether the rule has fallen
// back; `writer` (one workgroup) records them.  pv: [0, kFpsMaxBlocks) max d, [kFpsMaxBlocks, 2 kFpsMaxBlocks) max m, then
// sum max(d, 0), and pi the two indices, as launch round - 1 left them (nb workgroups).  final_fold: nothing is picked, only
// the statistics of the whole set are folded.  srow (LDS): the row l_j[s_k], j < round, unless fallen back
__device__ void resid_pick(int round, int final_fold, int nb, int N, int s0, double eps, const double* __restrict__ pv,
                           const int* __restrict__ pi, const double* L, size_t ld, double* srow,
                           const double* __restrict__ st_in, double* __restrict__ st_out, int* __restrict__ list,
                           double* __restrict__ pivot, bool writer, int& s_out, double& sq_out, bool& fallen_out) {
    writer = writer && threadIdx.x == 0;
    int fallen = 0, nres = 1, s = s0;
    double piv = 1.0;
    if (round > 0) {
        fallen = (int)st_in[kStFallen];
        nres = (int)st_in[kStResidual];
        if (!fallen) {
            double bv = -2.0, sum = 0.0;
            int bi = INT_MAX;
            for (int k = threadIdx.x; k < nb; k += kFpsThreads) {
                fps_take(bv, bi, pv[k], pi[k]);
                sum += pv[2 * kFpsMaxBlocks + k];
            }
            fps_block_argmax(bv, bi);
            sum = resid_block_sum(sum);
            if (writer) {  // after residual round `round - 1`: they stay once the rule has fallen back
                st_out[kStMax] = bi == INT_MAX ? 0.0 : bv;  // (no pixel left: p = N)
                st_out[kStArg] = bi == INT_MAX ? -1.0 : (double)bi;
                st_out[kStSum] = sum;
            }
            if (!(bv >= eps)) {
                fallen = 1;
            } else if (!final_fold) {
                s = bi;
                piv = bv;
                ++nres;
            }
        } else if (writer) {
            st_out[kStMax] = st_in[kStMax], st_out[kStArg] = st_in[kStArg], st_out[kStSum] = st_in[kStSum];
        }
        if (fallen && !final_fold) {
            double bv = -2.0;
            int bi = INT_MAX;
            for (int k = threadIdx.x; k < nb; k += kFpsThreads) fps_take(bv, bi, pv[kFpsMaxBlocks + k], pi[kFpsMaxBlocks + k]);
            fps_block_argmax(bv, bi);
            s = min(bi, N - 1);  // INT_MAX only if no m compared (a plane of NaNs): stay in bounds
            piv = bv;
        }
    }
    s_out = s, sq_out = sqrt(piv), fallen_out = fallen != 0;
    if (writer) {
        st_out[kStFallen] = (double)fallen;
        st_out[kStResidual] = (double)nres;
    }
    if (final_fold) return;
    if (writer) {
        list[round] = s;
        pivot[round] = piv;
    }
    if (!fallen)
        for (int j = threadIdx.x; j < round; j += kFpsThreads) srow[j] = L[(size_t)j * ld + (size_t)s];
}

// NP consecutive pixels from i0 (NP = 4: i0 a multiple of 4, 16-byte accesses), round k of the residual rule
template <int NP>
__device__ __forceinline__ void resid_pixels(int W, int i0, const float* y, int k,
                                             double* __restrict__ L, size_t ld, const double* srow, double sq, int s, int sr,
                                             int sc, double ys, double sw, double pw, double* __restrict__ d,
                                             double* __restrict__ m, double& bdv, int& bdi, double& bmv, int& bmi,
                                             double& sum) {
    // every operation rounded on its own, j ascending, one accumulator per pixel: the rule's order
#pragma clang fp contract(off)
    double acc[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) acc[q] = 0.0;
    double* col = L + i0;
#pragma unroll 4
    for (int j = 0; j < k; ++j, col += ld) {
        const double lj = srow[j];
        if (NP == 4) {
            const double2 a = *reinterpret_cast<const double2*>(col);
            const double2 b = *reinterpret_cast<const double2*>(col + 2);
            acc[0] = acc[0] + a.x * lj;
            acc[1] = acc[1] + a.y * lj;
            acc[2] = acc[2] + b.x * lj;
            acc[3] = acc[3] + b.y * lj;
        } else {
            acc[0] = acc[0] + col[0] * lj;
        }
    }
    int r = i0 / W, c = i0 - r * W;
    double l[NP], dn[NP], mn[NP], dold[NP], mold[NP];
    if (k > 0) {
        if (NP == 4) {
            const double2 d0 = *reinterpret_cast<const double2*>(d + i0), d1 = *reinterpret_cast<const double2*>(d + i0 + 2);
            const double2 m0 = *reinterpret_cast<const double2*>(m + i0), m1 = *reinterpret_cast<const double2*>(m + i0 + 2);
            dold[0] = d0.x, dold[1] = d0.y, dold[2] = d1.x, dold[3] = d1.y;
            mold[0] = m0.x, mold[1] = m0.y, mold[2] = m1.x, mold[3] = m1.y;
        } else {
            dold[0] = d[i0];
            mold[0] = m[i0];
        }
    }
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int i = i0 + q;
        const long long dr = r - sr, dc = c - sc;
        const double dy = (double)y[q] - ys;
        const double D = sw * (double)(dr * dr + dc * dc) + pw * (dy * dy);
        // K = exp(-sw d2 - pw dy^2): (-a) - b = -(a + b) bit for bit, so D serves the affinity and the farthest-point m
        l[q] = (exp(-D) - acc[q]) / sq;
        double v = D;
        if (k > 0) v = D < mold[q] ? D : mold[q];
        dn[q] = (k > 0 ? dold[q] : 1.0) - l[q] * l[q];
        mn[q] = i == s ? -1.0 : v;
        if (++c == W) {
            c = 0;
            ++r;
        }
    }
    if (NP == 4) {
        *reinterpret_cast<double2*>(col) = make_double2(l[0], l[1]);  // col is column k by now
        *reinterpret_cast<double2*>(col + 2) = make_double2(l[2], l[3]);
        *reinterpret_cast<double2*>(d + i0) = make_double2(dn[0], dn[1]);
        *reinterpret_cast<double2*>(d + i0 + 2) = make_double2(dn[2], dn[3]);
        *reinterpret_cast<double2*>(m + i0) = make_double2(mn[0], mn[1]);
        *reinterpret_cast<double2*>(m + i0 + 2) = make_double2(mn[2], mn[3]);
    } else {
        col[0] = l[0];
        d[i0] = dn[0];
        m[i0] = mn[0];
    }
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        if (mn[q] != -1.0) fps_take(bdv, bdi, dn[q], i0 + q);  // m = -1 marks the chosen pixels
        fps_take(bmv, bmi, mn[q], i0 + q);
        sum = sum + (dn[q] > 0.0 ? dn[q] : 0.0);
    }
}

// skip_pixels: the last sample of a selection whose statistics nobody asked for -- it is picked and nothing else
template <bool VEC>
__global__ __launch_bounds__(kFpsThreads) void k_residual_round(const float* __restrict__ lum, int W, int N, double sw,
                                                                 double pw, int round, int final_fold, int skip_pixels, int nb,
                                                                 int s0, double eps, double* L, size_t ld,
                                                                 const double* __restrict__ st_in, double* __restrict__ st_out,
                                                                 double* __restrict__ d, double* __restrict__ m,
                                                                 const double* __restrict__ pv_in, const int* __restrict__ pi_in,
                                                                 double* __restrict__ pv, int* __restrict__ pi,
                                                                 int* __restrict__ list, double* __restrict__ pivot) {
    __shared__ double srow[kResidRowMax];
    int s;
    double sq;
    bool fallen;
    resid_pick(round, final_fold, nb, N, s0, eps, pv_in, pi_in, L, ld, srow, st_in, st_out, list, pivot, blockIdx.x == 0, s, sq,
               fallen);
    if (final_fold || skip_pixels) return;
    const int sr = s / W, sc = s - sr * W;
    const double ys = (double)lum[s];
    double bdv = -2.0, bmv = -2.0, sum = 0.0;
    int bdi = INT_MAX, bmi = INT_MAX;
    const unsigned stride = gridDim.x * kFpsThreads;
    const unsigned nq = VEC ? (unsigned)N >> 2 : 0u, tail0 = nq << 2;
    if (!fallen) {
        __syncthreads();  // srow is complete
        for (unsigned q = blockIdx.x * kFpsThreads + threadIdx.x; q < nq; q += stride) {
            const int i0 = (int)(q << 2);
            const float4 y4 = *reinterpret_cast<const float4*>(lum + i0);
            const float y[4] = {y4.x, y4.y, y4.z, y4.w};
            resid_pixels<4>(W, i0, y, round, L, ld, srow, sq, s, sr, sc, ys, sw, pw, d, m, bdv, bdi, bmv, bmi, sum);
        }
        for (unsigned i = tail0 + blockIdx.x * kFpsThreads + threadIdx.x; i < (unsigned)N; i += stride) {
            const float y = lum[i];
            resid_pixels<1>(W, (int)i, &y, round, L, ld, srow, sq, s, sr, sc, ys, sw, pw, d, m, bdv, bdi, bmv, bmi, sum);
        }
    } else {  // the farthest-point step on m alone (round > 0 here: round 0 is a residual round)
        for (unsigned q = blockIdx.x * kFpsThreads + threadIdx.x; q < nq; q += stride) {
            const int i0 = (int)(q << 2);
            int r = i0 / W, c = i0 - r * W;
            const float4 y4 = *reinterpret_cast<const float4*>(lum + i0);
            const float y[4] = {y4.x, y4.y, y4.z, y4.w};
            double v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = fps_update(m, i0 + j, r, c, y[j], s, sr, sc, ys, sw, pw, round);
                if (++c == W) {
                    c = 0;
                    ++r;
                }
            }
            *reinterpret_cast<double2*>(m + i0) = make_double2(v[0], v[1]);
            *reinterpret_cast<double2*>(m + i0 + 2) = make_double2(v[2], v[3]);
#pragma unroll
            for (int j = 0; j < 4; ++j) fps_take(bmv, bmi, v[j], i0 + j);
        }
        for (unsigned i = tail0 + blockIdx.x * kFpsThreads + threadIdx.x; i < (unsigned)N; i += stride) {
            const int r = (int)i / W, c = (int)i - r * W;
            const double v = fps_update(m, (int)i, r, c, lum[i], s, sr, sc, ys, sw, pw, round);
            m[i] = v;
            fps_take(bmv, bmi, v, (int)i);
        }
    }
    fps_block_argmax(bmv, bmi);
    if (!fallen) {  // (uniform over the grid) after the fallback d, its partials and the statistics stay as they are
        fps_block_argmax(bdv, bdi);
        sum = resid_block_sum(sum);
    }
    if (threadIdx.x == 0) {
        pv[kFpsMaxBlocks + blockIdx.x] = bmv;
        pi[kFpsMaxBlocks + blockIdx.x] = bmi;
        if (!fallen) {
            pv[blockIdx.x] = bdv;
            pi[blockIdx.x] = bdi;
            pv[2 * kFpsMaxBlocks + blockIdx.x] = sum;
        }
    }
}

__global__ void k_gather_pix(const float* __restrict__ lum, const long long* __restrict__ pix, int n, float* __restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = lum[pix[k]];
}

__global__ void k_sample_mask(const long long* __restrict__ pix, int n, unsigned* __restrict__ mask) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) atomicOr(mask + (pix[k] >> 5), 1u << (unsigned)(pix[k] & 31));
}
}  // namespace

int farthest_max_blocks() { return kFpsMaxBlocks; }

hipError_t residual_samples(hipStream_t s, const float* d_lum, int H, int W, int p, double sw, double pw, double eps,
                            bool want_stats, double* d_L, double* d_d, double* d_m, double* d_pv, int* d_pi, double* d_state,
                            int* d_list, double* d_pivot, const double** d_state_final) {
    const long long N = (long long)H * W;
    if (H <= 0 || W <= 0 || N >= (1ll << 31) || p < 1 || p > N || p > kResidRowMax) return hipErrorInvalidValue;
    const int s0 = (H / 2) * W + W / 2;
    const size_t ld = (size_t)residual_ld(N);
    const bool vec = (reinterpret_cast<uintptr_t>(d_lum) & 15) == 0;
    const long long per_block = (long long)kFpsThreads * (vec ? 4 : 1);
    const int nb = (int)std::min<long long>((N + per_block - 1) / per_block, kFpsMaxBlocks);
    // want_stats: the last sample's own column and one more fold, so that the statistics are those of the whole set
    const int rounds = want_stats ? p + 1 : p;
    for (int k = 0; k < rounds; ++k) {
        // launch k reads the partials and the state launch k - 1 wrote (parity k & 1) and writes the other parity
        const size_t in = (size_t)(k & 1), out = (size_t)((k + 1) & 1);
        const int fin = k == p ? 1 : 0, skip = (k == p - 1 && !want_stats) ? 1 : 0;
        const unsigned grid = (fin || skip) ? 1u : (unsigned)nb;
        if (vec)
            hipLaunchKernelGGL(k_residual_round<true>, dim3(grid), dim3(kFpsThreads), 0, s, d_lum, W, (int)N, sw, pw, k, fin, skip,
                               nb, s0, eps, d_L, ld, d_state + in * kResidHead, d_state + out * kResidHead, d_d, d_m,
                               d_pv + in * 3 * kFpsMaxBlocks, d_pi + in * 2 * kFpsMaxBlocks, d_pv + out * 3 * kFpsMaxBlocks,
                               d_pi + out * 2 * kFpsMaxBlocks, d_list, d_pivot);
        else
            hipLaunchKernelGGL(k_residual_round<false>, dim3(grid), dim3(kFpsThreads), 0, s, d_lum, W, (int)N, sw, pw, k, fin, skip,
                               nb, s0, eps, d_L, ld, d_state + in * kResidHead, d_state + out * kResidHead, d_d, d_m,
                               d_pv + in * 3 * kFpsMaxBlocks, d_pi + in * 2 * kFpsMaxBlocks, d_pv + out * 3 * kFpsMaxBlocks,
                               d_pi + out * 2 * kFpsMaxBlocks, d_list, d_pivot);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    *d_state_final = d_state + (size_t)(rounds & 1) * kResidHead;  // what the last launch wrote
    return hipGetLastError();
}

hipError_t farthest_samples(hipStream_t s, const float* d_lum, int H, int W, int p, double sw, double pw, double* d_m,
                            double* d_pv, int* d_pi, int* d_list) {
    const long long N = (long long)H * W;
    if (H <= 0 || W <= 0 || N >= (1ll << 31) || p < 1 || p > N) return hipErrorInvalidValue;
    const int s0 = (H / 2) * W + W / 2;
    const bool vec = (reinterpret_cast<uintptr_t>(d_lum) & 15) == 0;
    const long long per_block = (long long)kFpsThreads * (vec ? 4 : 1);
    const int nb = (int)std::min<long long>((N + per_block - 1) / per_block, kFpsMaxBlocks);
    for (int k = 0; k < p; ++k) {
        // launch k reads the partials launch k - 1 wrote (buffer k & 1) and writes the other buffer
        const double* pv_in = d_pv + (size_t)(k & 1) * kFpsMaxBlocks;
        const int* pi_in = d_pi + (size_t)(k & 1) * kFpsMaxBlocks;
        double* pv_out = d_pv + (size_t)((k + 1) & 1) * kFpsMaxBlocks;
        int* pi_out = d_pi + (size_t)((k + 1) & 1) * kFpsMaxBlocks;
        const int last = k == p - 1 ? 1 : 0;
        if (vec)
            hipLaunchKernelGGL(k_farthest_round<true>, dim3((unsigned)nb), dim3(kFpsThreads), 0, s, d_lum, W, (int)N, sw, pw, k,
                               s0, last, pv_in, pi_in, d_m, pv_out, pi_out, d_list);
        else
            hipLaunchKernelGGL(k_farthest_round<false>, dim3((unsigned)nb), dim3(kFpsThreads), 0, s, d_lum, W, (int)N, sw, pw,
                               k, s0, last, pv_in, pi_in, d_m, pv_out, pi_out, d_list);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t gather_pix(hipStream_t s, const float* d_lum, const long long* d_pix, int n, float* d_out) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_gather_pix, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_lum, d_pix, n, d_out);
    return hipGetLastError();
}

hipError_t sample_mask(hipStream_t s, const long long* d_pix, int n, long long N, unsigned* d_mask) {
    const hipError_t e = hipMemsetAsync(d_mask, 0, (size_t)((N + 31) / 32) * sizeof(unsigned), s);
    if (e != hipSuccess || n <= 0) return e;
    hipLaunchKernelGGL(k_sample_mask, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_pix, n, d_mask);
    return hipGetLastError();
}

}  // namespace nlek
