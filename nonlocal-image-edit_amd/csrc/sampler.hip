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
