// Patch (non-local-means) affinity rows in fp64 on the int8 matrix cores (gfx950): the opt-in patch radius R > 0 of
// nle_ctx_set_patch_radius.  R = 0 is the reference's single-value affinity and never comes here (k_affinity64).
//
//   S_ij = sum_{dy,dx in [-R, R]} (y[rho(r+dy), rho(c+dx)] - y[rho(rs+dy), rho(cs+dx)])^2       (exact integer)
//   K_ij = exp(-sw (double)((r-rs)^2 + (c-cs)^2) - pwd (double)S_ij),  sw = 1/hx^2, pwd = (1/hy^2) / (2R+1)^2
//
// rho is reflect-101 (OpenCV BORDER_DEFAULT).  The plane is integer valued in [0, 255] (checked by the caller), so every
// value shifted by -128 is an int8 and S = |x'|^2 + |s'|^2 - 2 x'.s' with the dot products on v_mfma_i32_16x16x64_i8
// (i32 accumulation is exact: |x's'| <= 128^2 (2R+1)^2 < 2^22 for R <= 7).  The patch length d = (2R+1)^2 is zero-padded
// to KS x 64 (the MFMA K); padded entries are 0 on both sides and add nothing to the dot products or the norms.
//
// k_patch_affinity64: a workgroup of four waves covers 64 consecutive pixels at a time (natural order), wave w rows
// 16w..16w+15 as the A operand.  Each lane gathers its A fragment (16 patch bytes of one pixel per K step) straight from
// the fp32 plane: neighbouring pixels share almost all of their patch, so these loads hit L1 / L2.  The sample patches
// (B operand, p rounded up to 16 rows of KS x 64 bytes) are pre-packed on the host and read through the cache.  Column
// block by column block (kPatchCols samples), the int32 dot products go to LDS; the epilogue is k_affinity64's: one
// thread per double2 of the group's contiguous output span, fp64 exponent in the same order (not contracted), libm exp,
// 16-byte stores.
//
// With chroma planes (nle_ctx_set_chroma, R <= 3) the KC > 0 instantiations add the term cwd S_ab of the a and b patches:
// see the comment at the kernel.
#include "kernels.h"
#include "launch.h"

#include <algorithm>

namespace nlek {

typedef int i32x4 __attribute__((ext_vector_type(4)));

namespace {
constexpr int kPatchPix = 64;         // pixels per group (4 waves x 16-row MFMA tiles)
constexpr int kPatchCols = 128;       // samples per column block of the LDS dot-product tile
constexpr int kPatchDotLd = kPatchCols + 4;  // row stride of that tile (ints): the 4-row lane groups fall on other banks
constexpr int kPatchChromaCols = kPatchCols / 2;  // chroma form: two tiles (L and ab dot products), each half as wide

// reflect-101 for |overhang| <= n - 1 (the caller checks R <= min(H, W) - 1); the clamp only keeps a bad argument in bounds
__device__ __forceinline__ int reflect101(int t, int n) {
    t = t < 0 ? -t : (t >= n ? 2 * n - 2 - t : t);
    return min(max(t, 0), n - 1);
}
}  // namespace

int patch_kpad(int R) {
    const int d = (2 * R + 1) * (2 * R + 1);
    return (d + 63) & ~63;
}

// out[j d + k] = y at offset k of sample j's patch (k = (dy + R)(2R + 1) + dx + R), as an integer
__global__ void k_patch_gather(const float* __restrict__ lum, int H, int W, int R, const long long* __restrict__ pix, int n,
                               int* __restrict__ out) {
    const int P = 2 * R + 1, d = P * P;
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n * d; idx += gridDim.x * blockDim.x) {
        const int j = idx / d, k = idx - j * d;
        const int r = (int)(pix[j] / W), c = (int)(pix[j] - (long long)r * W);
        const int rr = reflect101(r + k / P - R, H), cc = reflect101(c + k % P - R, W);
        out[idx] = (int)lum[(size_t)rr * W + cc];
    }
}

hipError_t patch_gather(hipStream_t s, const float* d_lum, int H, int W, int R, const long long* d_pix, int n, int* d_out) {
    if (n <= 0) return hipSuccess;
    const int total = n * (2 * R + 1) * (2 * R + 1);
    hipLaunchKernelGGL(k_patch_gather, dim3((unsigned)std::min((total + 255) / 256, 1024)), dim3(256), 0, s, d_lum, H, W, R,
                       d_pix, n, d_out);
    return hipGetLastError();
}

// KC > 0: the chroma form (nle_ctx_set_chroma, R <= 3).  S_L and S_ab carry different weights, so S_ab is a second i32
// accumulation of KC K steps over the a patch followed by the b patch (2 d values, zero padded to KC x 64), gathered from
// the a and b planes as the L fragment is from L.  Both dot-product tiles live in LDS side by side, each half as wide
// (64 samples per column block instead of 128), so the kernel's LDS and occupancy are those of the chroma-off form; the
// epilogue subtracts cwd S_ab last.  KC = 0 is the kernel as it was (its launch bounds ask for nothing: same code).
template <int KS, int KC>
__global__ __launch_bounds__(256, KC > 0 ? 4 : 1) void k_patch_affinity64(const float* __restrict__ lum, GridSpec gs, int R,
                                                          const Sample4* __restrict__ samples,
                                                          const signed char* __restrict__ spatch,
                                                          const int* __restrict__ snorm, int p, int ld, double sw, double pwd,
                                                          long long pix0, long long M, double* __restrict__ kab,
                                                          int skip_samples, const unsigned* __restrict__ smask,
                                                          const float* __restrict__ pa, const float* __restrict__ pb,
                                                          const signed char* __restrict__ cpatch,
                                                          const int* __restrict__ cnorm, double cwd) {
    // the exponent is rounded operation by operation, as the definition (and build_Ka on the host) evaluates it: a
    // contracted fma would round -sw d2 - pwd S once instead of twice, ~1 ulp of a large exponent
#pragma clang fp contract(off)
    constexpr bool CHROMA = KC > 0;
    constexpr int COLS = CHROMA ? kPatchChromaCols : kPatchCols;  // samples per column block of a dot-product tile
    constexpr int DLD = COLS + 4;                               // its row stride (ints), as kPatchDotLd
    constexpr int KCN = CHROMA ? KC : 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_patch[];
    int2* srow_col = reinterpret_cast<int2*>(smem_patch);                                  // [ld]
    int* sn = reinterpret_cast<int*>(smem_patch + (size_t)ld * sizeof(int2));               // [ld]
    int* pn = sn + ld;                                                                      // [kPatchPix]
    int* dot = pn + kPatchPix;                                                              // [kPatchPix][DLD]
    int* dotc = dot + kPatchPix * DLD;                                                      // CHROMA: [kPatchPix][DLD]
    int* pcn = dotc + kPatchPix * DLD;                                                      // CHROMA: [kPatchPix]
    int* scn = pcn + kPatchPix;                                                             // CHROMA: [ld]
    for (int k = threadIdx.x; k < ld; k += 256) {
        Sample4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < p) v = samples[k];
        srow_col[k] = make_int2((int)v.x, (int)v.y);
        sn[k] = k < p ? snorm[k] : 0;
        if constexpr (CHROMA) scn[k] = k < p ? cnorm[k] : 0;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int P = 2 * R + 1, d = P * P, KP = KS * 64;
    const int ntiles = (p + 15) >> 4;
    const long long ngroups = (M + kPatchPix - 1) / kPatchPix;
    for (long long grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const long long i0 = grp * kPatchPix;
        // ---- A fragments of this wave's 16 pixels: lane holds pixel 16 wv + (lane & 15), patch entries
        //      k = 64 ks + 16 (lane >> 4) + e, e < 16 (v - 128, 0 beyond d or beyond M), and their partial norm
        i32x4 a[KS];
        i32x4 ac[KCN];
        int nrm = 0, nrmc = 0;
        {
            const long long il = i0 + 16 * wv + (lane & 15);
            const bool live = il < M;
            const long long gi = pix0 + (live ? il : 0);
            const int row = (int)(gi / gs.W), col = (int)(gi - (long long)row * gs.W);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                int words[4];
                const int kb = 64 * ks + 16 * (lane >> 4);
                int dy = kb / P, dx = kb - dy * P;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    unsigned wd = 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int k = kb + 4 * w + e;
                        int v = 0;
                        if (live && k < d) {
                            const int rr = reflect101(row + dy - R, gs.H), cc = reflect101(col + dx - R, gs.W);
                            v = (int)lum[(size_t)rr * gs.W + cc] - 128;
                        }
                        nrm += v * v;
                        wd |= ((unsigned)v & 0xffu) << (8 * e);
                        if (++dx == P) {
                            dx = 0;
                            ++dy;
                        }
                    }
                    words[w] = (int)wd;
                }
                a[ks] = i32x4{words[0], words[1], words[2], words[3]};
            }
            if constexpr (CHROMA) {
                // entries k < d: the a patch at offset k; d <= k < 2 d: the b patch at offset k - d; beyond: 0.  One
                // word (four loads) at a time: with the K steps' 16 loads each unrolled and hoisted like the L fragment's,
                // the kernel held 180 (KC = 1) and 256 (KC = 2) registers, 2 and 1 waves per SIMD where the chroma-off
                // kernel of the same radius runs 4; this way, and asked for 4 by its launch bounds, it keeps 4 without scratch
#pragma unroll
                for (int ks = 0; ks < KC; ++ks) {
                    i32x4 frag = {0, 0, 0, 0};
                    const int kb = 64 * ks + 16 * (lane >> 4);
                    const float* __restrict__ pl = kb < d ? pa : pb;
                    const int ko = kb < d ? kb : kb - d;
                    int dy = ko / P, dx = ko - dy * P;
#pragma unroll 1
                    for (int w = 0; w < 4; ++w) {
                        unsigned wd = 0;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int k = kb + 4 * w + e;
                            int v = 0;
                            if (live && k < 2 * d) {
                                const int rr = reflect101(row + dy - R, gs.H), cc = reflect101(col + dx - R, gs.W);
                                v = (int)pl[(size_t)rr * gs.W + cc] - 128;
                            }
                            nrmc += v * v;
                            wd |= ((unsigned)v & 0xffu) << (8 * e);
                            if (++dx == P) {
                                dx = 0;
                                if (++dy == P) {  // the a patch is done: on to the b patch
                                    dy = 0;
                                    pl = pb;
                                }
                            }
                        }
                        frag[w] = (int)wd;
                    }
                    ac[ks] = frag;
                }
            }
        }
        nrm += __shfl_xor(nrm, 16);
        nrm += __shfl_xor(nrm, 32);
        if constexpr (CHROMA) {
            nrmc += __shfl_xor(nrmc, 16);
            nrmc += __shfl_xor(nrmc, 32);
        }
        __syncthreads();  // the previous group's epilogue is done with pn / dot (and the sample tables are in on the first)
        if (lane < 16) {
            pn[16 * wv + lane] = nrm;
            if constexpr (CHROMA) pcn[16 * wv + lane] = nrmc;
        }
        for (int cb0 = 0; cb0 < ld; cb0 += COLS) {
            // ---- dot products of the column block: dot[row][s - cb0] = x'_row . s'_s
            const int t1 = min(ntiles, (cb0 + COLS) >> 4);
            for (int t = cb0 >> 4; t < t1; ++t) {
                const signed char* bp = spatch + (size_t)(16 * t + (lane & 15)) * KP + 16 * (lane >> 4);
                i32x4 acc = {0, 0, 0, 0};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const i32x4 b = *reinterpret_cast<const i32x4*>(bp + 64 * ks);
                    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[ks], b, acc, 0, 0, 0);
                }
                // C/D: column = lane & 15, row = 4 (lane >> 4) + reg
                int* dp = dot + (16 * wv + 4 * (lane >> 4)) * DLD + 16 * t - cb0 + (lane & 15);
#pragma unroll
                for (int g = 0; g < 4; ++g) dp[g * DLD] = acc[g];
                if constexpr (CHROMA) {
                    const signed char* cp = cpatch + (size_t)(16 * t + (lane & 15)) * (KC * 64) + 16 * (lane >> 4);
                    i32x4 accc = {0, 0, 0, 0};
#pragma unroll
                    for (int ks = 0; ks < KC; ++ks) {
                        const i32x4 b = *reinterpret_cast<const i32x4*>(cp + 64 * ks);
                        accc = __builtin_amdgcn_mfma_i32_16x16x64_i8(ac[ks], b, accc, 0, 0, 0);
                    }
#pragma unroll
                    for (int g = 0; g < 4; ++g) dp[(kPatchPix + g) * DLD] = accc[g];  // the same place in dotc
                }
            }
            __syncthreads();
            // ---- epilogue over the group's rows x this block's columns: one double2 per thread per step
            const int ncols = min(COLS, ld - cb0), nq = ncols >> 1;
            const unsigned per_group = (unsigned)(kPatchPix * nq);
            const unsigned nvalid = (unsigned)min((long long)kPatchPix, M - i0) * nq;
            for (unsigned f = threadIdx.x; f < per_group; f += 256) {
                if (f >= nvalid) break;
                const unsigned il = f / nq, q = f - il * nq;
                const long long gi = pix0 + i0 + il;
                const int row = (int)(gi / gs.W), col = (int)(gi - (long long)row * gs.W);
                const bool zero_row = skip_samples && is_sample(gs, smask, gi, row, col);
                double v[2] = {0.0, 0.0};
                if (!zero_row) {
                    const int xn = pn[il];
                    const int2 dd = *reinterpret_cast<const int2*>(dot + il * DLD + 2 * q);
                    int xcn = 0;
                    int2 ddc = make_int2(0, 0);
                    if constexpr (CHROMA) {
                        xcn = pcn[il];
                        ddc = *reinterpret_cast<const int2*>(dotc + il * DLD + 2 * q);
                    }
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const int s = cb0 + 2 * (int)q + e;
                        if (s < p) {
                            const int2 rc = srow_col[s];
                            const long long dr = row - rc.x, dc = col - rc.y;
                            const int S = xn + sn[s] - 2 * (e ? dd.y : dd.x);
                            if constexpr (CHROMA) {
                                const int Sc = xcn + scn[s] - 2 * (e ? ddc.y : ddc.x);
                                const double e0 = -sw * (double)(dr * dr + dc * dc) - pwd * (double)S;
                                v[e] = exp(e0 - cwd * (double)Sc);
                            } else {
                                v[e] = exp(-sw * (double)(dr * dr + dc * dc) - pwd * (double)S);
                            }
                        }
                    }
                }
                *reinterpret_cast<double2*>(kab + (size_t)(i0 + il) * ld + cb0 + 2 * q) = make_double2(v[0], v[1]);
            }
            __syncthreads();  // dot is rewritten by the next block
        }
    }
}

size_t patch_spatch_bytes(int p, int R) { return (size_t)((p + 15) & ~15) * patch_kpad(R); }

int patch_ckpad(int R) {
    const int d2 = 2 * (2 * R + 1) * (2 * R + 1);
    return (d2 + 63) & ~63;
}

size_t patch_cpatch_bytes(int p, int R) { return (size_t)((p + 15) & ~15) * patch_ckpad(R); }

size_t patch_affinity64_chroma_lds_bytes(int ld) {
    return (size_t)ld * (sizeof(int2) + 2 * sizeof(int)) + 2 * kPatchPix * sizeof(int) +
           2 * (size_t)kPatchPix * (kPatchChromaCols + 4) * sizeof(int);
}

namespace {
hipError_t launch_patch_affinity64(hipStream_t s, const Affinity64Args& a, long long pix0, long long M, double* d_kab,
                                   bool skip_samples) {
    if ((a.ld & 1) || a.R < 1 || a.R > 7 || a.ld < a.p) return hipErrorInvalidValue;
    const long long ngroups = (M + kPatchPix - 1) / kPatchPix;
    const int grid = (int)std::min<long long>(ngroups, 8192);
    const size_t lds = (size_t)a.ld * (sizeof(int2) + sizeof(int)) + kPatchPix * sizeof(int) +
                       (size_t)kPatchPix * kPatchDotLd * sizeof(int);
    hipError_t e = hipErrorInvalidValue;  // patch_kpad(R) / 64 is one of 1 .. 4 for the R in 1 .. 7 admitted above
    dispatch_columns<1, 4>(patch_kpad(a.R) / 64, [&](auto ks) {
        e = launch(k_patch_affinity64<decltype(ks)::value, 0>, dim3((unsigned)grid), dim3(256), lds, s, a.lum, a.gs, a.R, a.samples,
                   a.spatch, a.snorm, a.p, a.ld, a.sw, a.pw, pix0, M, d_kab, skip_samples ? 1 : 0, a.smask, nullptr, nullptr, nullptr,
                   nullptr, 0.0);
    });
    return e;
}

hipError_t launch_patch_affinity64_chroma(hipStream_t s, const Affinity64Args& a, long long pix0, long long M, double* d_kab,
                                          bool skip_samples) {
    // R <= 3: one K step for L; one (R = 1) or two (R = 2, 3) for the concatenated a and b patches
    if ((a.ld & 1) || a.R < 1 || a.R > 3 || a.ld < a.p || !a.a || !a.b || !a.cpatch || !a.cnorm) return hipErrorInvalidValue;
    // 34.5 KiB of tiles + 16 bytes per sample: past 1888 samples the launch asks for more than the default allowance
    const size_t lds = patch_affinity64_chroma_lds_bytes(a.ld);
    if (lds > kPatchChromaLdsMax) return hipErrorInvalidValue;  // (the caller refuses such a sample set with a message)
    const long long ngroups = (M + kPatchPix - 1) / kPatchPix;
    const int grid = (int)std::min<long long>(ngroups, 8192);
    hipError_t e = hipErrorInvalidValue;  // patch_ckpad(R) / 64 is 1 or 2 for the R in 1 .. 3 admitted above
    dispatch_columns<1, 2>(patch_ckpad(a.R) / 64, [&](auto kc) {
        e = launch(k_patch_affinity64<1, decltype(kc)::value>, dim3((unsigned)grid), dim3(256), lds, s, a.lum, a.gs, a.R, a.samples,
                   a.spatch, a.snorm, a.p, a.ld, a.sw, a.pw, pix0, M, d_kab, skip_samples ? 1 : 0, a.smask, a.a, a.b, a.cpatch,
                   a.cnorm, a.cw);
    });
    return e;
}
}  // namespace

hipError_t patch_affinity_rows64(hipStream_t s, const Affinity64Args& a, long long pix0, long long M, double* d_kab,
                                 bool skip_samples) {
    return a.a ? launch_patch_affinity64_chroma(s, a, pix0, M, d_kab, skip_samples)
               : launch_patch_affinity64(s, a, pix0, M, d_kab, skip_samples);
}

}  // namespace nlek
