// The MSE-guided denoiser's own pieces (include/nle.h "MSE-guided denoise"): the non-local-means
// pre-filter of an 8-bit plane (k_nlm8), Immerkaer's noise sum (k_noise_partial + k_noise_fold) and the host-only search for
// the shrinkage power (nle_mse_shrink).  nle_filter_coefficients, the fourth piece, lives with the applies in pipeline.hip.
#include <hip/hip_runtime.h>

#include <cmath>

#include "pipeline_internal.h"

namespace nlek {

namespace {
__device__ __forceinline__ int reflect101(int i, int n) {  // BORDER_REFLECT_101, any distance (colour.hip's rule)
    if (n == 1) return 0;
    const int period = 2 * n - 2;
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - i;
}
}  // namespace

// ---- non-local means.  A workgroup takes a 64 x 16 tile of pixels; a thread takes 4 pixels below one another, and the 64
// lanes of a wave read 64 consecutive floats of one tile row: every LDS read is conflict free.  SSD(p, q) = S_p + S_q - 2 <p, q>
// (S_* the patches' sums of squares, all exact integers below 2^24, so fp32 fma arithmetic is exact): S_q comes from a second
// LDS tile made once, and the dot products of the thread's 4 pixels with the patch at one offset share their row products --
// row r of the stacked patches meets the same q row for every pixel that owns it -- so one offset costs (4 + 2P)(2P + 1) LDS
// reads and as many fmas for 4 pixels where brute force takes 4 (2P + 1)^2 reads and twice the arithmetic.
constexpr int kNlmTx = 64, kNlmTy = 4, kNlmRows = 4;  // threads in x, threads in y, pixel rows per thread
constexpr int kNlmTileH = kNlmTy * kNlmRows;

template <int P>
__global__ __launch_bounds__(kNlmTx* kNlmTy) void k_nlm8(const float* __restrict__ src, int H, int W, int S, float Tf,
                                                        float cf, float* __restrict__ dst, float* __restrict__ raw) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int D = 2 * P + 1, NR = kNlmRows + 2 * P;
    const int R = P + S, tw = kNlmTx + 2 * R, th = kNlmTileH + 2 * R, qw = kNlmTx + 2 * S, qh = kNlmTileH + 2 * S;
    float* tile = reinterpret_cast<float*>(smem_raw);  // [th][tw]: the tile with its halo of P + S
    float* sq = tile + tw * th;                         // [qh][qw]: S_q of the patch whose top-left corner is tile (qy, qx)
    const int tid = threadIdx.y * kNlmTx + threadIdx.x, nthr = kNlmTx * kNlmTy;
    const int x0 = blockIdx.x * kNlmTx - R, y0 = blockIdx.y * kNlmTileH - R;
    for (int i = tid; i < tw * th; i += nthr) {
        const int ty = i / tw, tx = i - ty * tw;
        tile[i] = src[(size_t)reflect101(y0 + ty, H) * W + reflect101(x0 + tx, W)];
    }
    __syncthreads();
    for (int i = tid; i < qw * qh; i += nthr) {
        const int qy = i / qw, qx = i - qy * qw;
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < D; ++r)
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const float v = tile[(qy + r) * tw + qx + k];
                s = fmaf(v, v, s);
            }
        sq[i] = s;
    }
    __syncthreads();
    const int tx = threadIdx.x, ty = threadIdx.y * kNlmRows;  // the thread's first pixel, tile-local
    // the thread's own patches, stacked: rows ty + S .. ty + S + NR of the tile, columns tx + S .. tx + S + D
    float c[NR][D], Sp[kNlmRows];
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int k = 0; k < D; ++k) c[r][k] = tile[(ty + S + r) * tw + tx + S + k];
#pragma unroll
    for (int j = 0; j < kNlmRows; ++j) Sp[j] = sq[(ty + j + S) * qw + tx + S];
    float num[kNlmRows], den[kNlmRows];
#pragma unroll
    for (int j = 0; j < kNlmRows; ++j) num[j] = den[j] = 0.f;
    const int nd = 2 * S + 1;
    for (int dy = 0; dy < nd; ++dy) {
        float rn[kNlmRows], rd[kNlmRows];  // this window row's sums
#pragma unroll
        for (int j = 0; j < kNlmRows; ++j) rn[j] = rd[j] = 0.f;
        const float* trow = tile + (ty + dy) * tw + tx;
        const float* qrow = sq + (ty + dy) * qw + tx;
        for (int dx = 0; dx < nd; ++dx) {
            float rowdot[NR], centre[kNlmRows];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    const float v = trow[r * tw + dx + k];
                    s = fmaf(c[r][k], v, s);
                    if (k == P && r >= P && r < P + kNlmRows) centre[r - P] = v;  // u(q) of pixel r - P
                }
                rowdot[r] = s;
            }
#pragma unroll
            for (int j = 0; j < kNlmRows; ++j) {
                float dot = 0.f;
#pragma unroll
                for (int r = 0; r < D; ++r) dot += rowdot[j + r];
                const float ssd = (Sp[j] + qrow[j * qw + dx]) - 2.f * dot;  // exact
                const float d = fmaxf(ssd - Tf, 0.f);
                const float w = d == 0.f ? 1.f : __expf(-(d * cf));
                rn[j] = fmaf(w, centre[j], rn[j]);
                rd[j] += w;
            }
        }
#pragma unroll
        for (int j = 0; j < kNlmRows; ++j) {
            num[j] += rn[j];
            den[j] += rd[j];
        }
    }
    const int x = blockIdx.x * kNlmTx + tx;
    if (x >= W) return;
#pragma unroll
    for (int j = 0; j < kNlmRows; ++j) {
        const int y = blockIdx.y * kNlmTileH + ty + j;
        if (y >= H) break;
        const float v = __fdiv_rn(num[j], den[j]);
        if (raw != nullptr) raw[(size_t)y * W + x] = v;
        dst[(size_t)y * W + x] = rintf(v);
    }
}

hipError_t nlm8(hipStream_t s, const float* d_src, int H, int W, int P, int S, float Tf, float cf, float* d_dst, float* d_raw) {
    if (H <= 0 || W <= 0) return hipSuccess;
    if (P < 1 || P > NLE_NLM_PATCH_RADIUS_MAX || S < 1 || S > NLE_NLM_SEARCH_RADIUS_MAX) return hipErrorInvalidValue;
    const int R = P + S;
    const size_t shm = ((size_t)(kNlmTx + 2 * R) * (kNlmTileH + 2 * R) + (size_t)(kNlmTx + 2 * S) * (kNlmTileH + 2 * S)) * sizeof(float);
    const dim3 grid((unsigned)((W + kNlmTx - 1) / kNlmTx), (unsigned)((H + kNlmTileH - 1) / kNlmTileH)), block(kNlmTx, kNlmTy);
    if (P == 1) hipLaunchKernelGGL(k_nlm8<1>, grid, block, shm, s, d_src, H, W, S, Tf, cf, d_dst, d_raw);
    else if (P == 2) hipLaunchKernelGGL(k_nlm8<2>, grid, block, shm, s, d_src, H, W, S, Tf, cf, d_dst, d_raw);
    else hipLaunchKernelGGL(k_nlm8<3>, grid, block, shm, s, d_src, H, W, S, Tf, cf, d_dst, d_raw);
    return hipGetLastError();
}

// ---- Immerkaer's sum: |x * M| over the interior, 64-bit integer partials per block, folded by one block in a fixed order
constexpr int kNoiseMaxBlocks = 1024;

__global__ __launch_bounds__(256) void k_noise_partial(const float* __restrict__ x, int H, int W, long long* __restrict__ partial) {
    __shared__ long long sh[256];
    const int iw = W - 2;
    const long long n = (long long)(H - 2) * iw;
    long long acc = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int r = (int)(i / iw), cc = (int)(i - (long long)r * iw);
        const float* p0 = x + (size_t)r * W + cc;
        const float* p1 = p0 + W;
        const float* p2 = p1 + W;
        const int v = ((int)p0[0] + (int)p0[2] + (int)p2[0] + (int)p2[2]) - 2 * ((int)p0[1] + (int)p1[0] + (int)p1[2] + (int)p2[1]) +
                      4 * (int)p1[1];
        acc += v < 0 ? -v : v;
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}

__global__ __launch_bounds__(256) void k_noise_fold(const long long* __restrict__ partial, int nb, long long* __restrict__ out) {
    __shared__ long long sh[256];
    long long acc = 0;
    for (int i = threadIdx.x; i < nb; i += 256) acc += partial[i];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sh[0];
}

// d_ws: kNoiseMaxBlocks + 1 values; the sum arrives in d_ws[kNoiseMaxBlocks]
hipError_t plane_noise(hipStream_t s, const float* d_x, int H, int W, long long* d_ws) {
    if (H < 3 || W < 3) return hipErrorInvalidValue;
    const long long n = (long long)(H - 2) * (W - 2);
    const int nb = (int)std::min<long long>((n + 255) / 256, kNoiseMaxBlocks);
    hipLaunchKernelGGL(k_noise_partial, dim3(nb), dim3(256), 0, s, d_x, H, W, d_ws);
    hipLaunchKernelGGL(k_noise_fold, dim3(1), dim3(256), 0, s, d_ws, nb, d_ws + kNoiseMaxBlocks);
    return hipGetLastError();
}

}  // namespace nlek

using namespace nlep;

namespace {
// the plane must hold integers 0..255 (the kernels index and sum them as such): check_levels, as nle_bilateral8 asks it
void require_levels(nle_ctx* ctx, const float* d_x, int H, int W, const char* who) {
    DevBuf<int> d_flag(2);  // verdict, level tiles (unused here)
    int flag = 1;
    HIP_OK(nlek::check_levels(ctx->stream, d_x, (long long)H * W, d_flag.p));
    HIP_OK(hipMemcpyAsync(&flag, d_flag.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(hipStreamSynchronize(ctx->stream));
    if (flag != 0) throw Fail{NLE_ERR_INVALID, std::string(who) + ": the plane must be integer valued in [0, 255] (CV_8UC1)"};
}

bool overlap(const float* a, const float* b, long long n) { return a && b && a < b + n && b < a + n; }
}  // namespace

extern "C" {

int nle_nlm8(nle_ctx* ctx, const float* d_src, int H, int W, int patch_radius, int search_radius, double sigma, double h,
             float* d_dst, float* d_raw) {
    if (!ctx) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        if (!d_src || !d_dst) throw Fail{NLE_ERR_INVALID, "nle_nlm8: d_src and d_dst must not be NULL"};
        if (H < 1 || W < 1) throw Fail{NLE_ERR_INVALID, "nle_nlm8: H and W must be >= 1"};
        check_image_size(H, W);
        if (patch_radius < 1 || patch_radius > NLE_NLM_PATCH_RADIUS_MAX)
            throw Fail{NLE_ERR_INVALID, "nle_nlm8: patch_radius must be in [1, " + std::to_string(NLE_NLM_PATCH_RADIUS_MAX) + "], got " +
                                            std::to_string(patch_radius)};
        if (search_radius < 1 || search_radius > NLE_NLM_SEARCH_RADIUS_MAX)
            throw Fail{NLE_ERR_INVALID, "nle_nlm8: search_radius must be in [1, " + std::to_string(NLE_NLM_SEARCH_RADIUS_MAX) +
                                            "], got " + std::to_string(search_radius)};
        if (!std::isfinite(sigma) || sigma < 0) throw Fail{NLE_ERR_INVALID, "nle_nlm8: sigma must be finite and >= 0"};
        if (!std::isfinite(h) || !(h > 0)) throw Fail{NLE_ERR_INVALID, "nle_nlm8: h must be finite and > 0"};
        const long long n = (long long)H * W;
        if (overlap(d_src, d_dst, n) || overlap(d_src, d_raw, n) || overlap(d_dst, d_raw, n))
            throw Fail{NLE_ERR_INVALID, "nle_nlm8: d_dst and d_raw must not alias d_src or each other"};
        const double np = (double)((2 * patch_radius + 1) * (2 * patch_radius + 1));
        const float Tf = (float)(2.0 * sigma * sigma * np), cf = (float)(1.0 / (np * h * h));
        if (!std::isfinite(Tf) || !std::isfinite(cf))
            throw Fail{NLE_ERR_INVALID, "nle_nlm8: 2 sigma^2 n and 1 / (n h^2) must be finite in fp32"};
        HIP_OK(hipSetDevice(ctx->device));
        require_levels(ctx, d_src, H, W, "nle_nlm8");
        PROFILED(ctx, NLE_K_NLM8, nlek::nlm8(ctx->stream, d_src, H, W, patch_radius, search_radius, Tf, cf, d_dst, d_raw));
        HIP_OK(hipStreamSynchronize(ctx->stream));
        prof_flush(ctx);
    });
}

int nle_plane_noise(nle_ctx* ctx, const float* d_x, int H, int W, long long* h_abs_sum, double* h_sigma) {
    if (!ctx) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        if (!d_x || !h_sigma) throw Fail{NLE_ERR_INVALID, "nle_plane_noise: d_x and h_sigma must not be NULL"};
        if (H < 3 || W < 3) throw Fail{NLE_ERR_INVALID, "nle_plane_noise: H and W must be >= 3 (the 3 x 3 mask needs an interior)"};
        check_image_size(H, W);
        HIP_OK(hipSetDevice(ctx->device));
        require_levels(ctx, d_x, H, W, "nle_plane_noise");
        DevBuf<long long> d_ws(nlek::kNoiseMaxBlocks + 1);
        long long S = 0;
        PROFILED(ctx, NLE_K_PLANE_NOISE, nlek::plane_noise(ctx->stream, d_x, H, W, d_ws.p));
        HIP_OK(hipMemcpyAsync(&S, d_ws.p + nlek::kNoiseMaxBlocks, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
        HIP_OK(hipStreamSynchronize(ctx->stream));
        prof_flush(ctx);
        if (h_abs_sum) *h_abs_sum = S;
        *h_sigma = std::sqrt(M_PI / 2.0) * (double)S / (6.0 * (double)(H - 2) * (double)(W - 2));
    });
}

int nle_mse_shrink(const double* h_eigvals, const double* h_b, int K, double sigma, double k_max, int n_grid, double* h_k,
                   double* h_mse) {
    if (!h_eigvals || !h_b || !h_k || K < 1 || n_grid < 1 || n_grid > 65536) return NLE_ERR_INVALID;
    if (!std::isfinite(sigma) || sigma < 0 || !std::isfinite(k_max) || k_max < 0) return NLE_ERR_INVALID;
    const double s2 = sigma * sigma;
    double best = 0.0, best_k = 0.0;
    for (int i = 0; i <= n_grid; ++i) {
        const double k = k_max * (double)i / (double)n_grid;
        double mse = 0.0;
        for (int j = 0; j < K; ++j) {
            const double mu = std::min(std::max(h_eigvals[j], 0.0), 1.0);
            const double a = std::pow(mu, k), bias = (1.0 - a) * h_b[j];
            mse += bias * bias + s2 * std::pow(mu, 2.0 * k);
        }
        if (h_mse) h_mse[i] = mse;
        if (i == 0 || mse < best) best = mse, best_k = k;
    }
    *h_k = best_k;
    return NLE_OK;
}

}  // extern "C"
