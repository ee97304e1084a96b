// Variants of the table Sinkhorn pixel kernel (k_hist_pix<10>, tables.hip) on a cfg4-shaped problem: which LDS
// accumulation is fastest?  Timing experiment only (round-2 VERDICT item 3: "measure, don't argue").
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -o /tmp/hpv tools/micro/hist_pix_variants.hip
//   V0  the shipping kernel: ds_add_f64 + wave-level pre-reduction of levels shared by >= 12 lanes
//   V1  ds_add_u64 on fixed-point terms (one scale), same pre-reduction
//   V2  V1 without the pre-reduction
//   V3  ds_add_f64, two sub-histograms (even / odd lanes)
//   V4  ds_add_u64, two sub-histograms
#include "../../nonlocal-image-edit_amd/csrc/tables.hip"

#include <cmath>
#include <cstdio>
#include <vector>

using namespace nlek;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

template <int NC, int VAR>
__global__ __launch_bounds__(kPixThreads) void k_var(const float* __restrict__ lum, GridSpec gs, int row0,
                                                     const double* __restrict__ ecT, const double* __restrict__ g,
                                                     double eps, double scale, double* __restrict__ hout) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int n = kLevels * NC;
    constexpr int NS = NC | 1;
    constexpr bool U64 = (VAR == 1 || VAR == 2 || VAR == 4);
    constexpr bool TWO = (VAR == 3 || VAR == 4);
    constexpr bool GROUP = (VAR == 1 || VAR == 3 || VAR == 4);
    const int W = gs.W;
    double* sg = reinterpret_cast<double*>(smem_raw);
    double* sh = sg + kLevels * NS;
    double* sh2 = TWO ? sh + kLevels * NS + 1 : sh;  // second copy, shifted by one bank pair
    const int tid = threadIdx.x, lrow = blockIdx.x, r = row0 + lrow;
    const double* grow = g + (size_t)lrow * n;
    for (int i = tid; i < n; i += kPixThreads) {
        const int bb = i / kLevels, xx = i & (kLevels - 1);
        sh[xx * NS + bb] = 0.0;
        if (TWO) sh2[xx * NS + bb] = 0.0;
        sg[xx * NS + bb] = grow[i];
    }
    __syncthreads();
    double* mysh = (TWO && (tid & 1)) ? sh2 : sh;
    for (int c0 = 0; c0 < W; c0 += kPixThreads) {
        const bool inside = c0 + tid < W;
        const int c = inside ? c0 + tid : W - 1;
        const int x = (int)lum[(size_t)r * W + c];
        double e[NC];
#pragma unroll
        for (int b = 0; b < NC; ++b) e[b] = ecT[(size_t)b * W + c];
        double gv[NC];
#pragma unroll
        for (int b = 0; b < NC; ++b) gv[b] = sg[x * NS + b];
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int b = 0; b < NC; ++b) {
            if (b & 1) s1 += e[b] * gv[b];
            else s0 += e[b] * gv[b];
        }
        double y = recip_or_zero_d(s0 + s1, eps);
        if (!inside) y = 0.0;
        bool own = y != 0.0;
        if (GROUP) {
            own = wave_group_levels(y != 0.0, x, [&](int lx, bool mine) {
#pragma unroll
                for (int b = 0; b < NC; ++b) {
                    const double t = wave_sum63(mine ? e[b] * y : 0.0);
                    if ((tid & 63) == 63) {
                        if (U64) atomicAdd(reinterpret_cast<unsigned long long*>(&sh[lx * NS + b]), (unsigned long long)(t * scale));
                        else atomicAdd(&sh[lx * NS + b], t);
                    }
                }
            });
        }
        if (own) {
#pragma unroll
            for (int b = 0; b < NC; ++b) {
                if (U64) atomicAdd(reinterpret_cast<unsigned long long*>(&mysh[x * NS + b]), (unsigned long long)(e[b] * y * scale));
                else atomicAdd(&mysh[x * NS + b], e[b] * y);
            }
        }
    }
    __syncthreads();
    double* hrow = hout + (size_t)lrow * n;
    const double inv = 1.0 / scale;
    for (int i = tid; i < n; i += kPixThreads) {
        const int bb = i / kLevels, xx = i & (kLevels - 1);
        double v;
        if (U64) {
            unsigned long long a = *reinterpret_cast<unsigned long long*>(&sh[xx * NS + bb]);
            if (TWO) a += *reinterpret_cast<unsigned long long*>(&sh2[xx * NS + bb]);
            v = (double)a * inv;
        } else {
            v = sh[xx * NS + bb] + (TWO ? sh2[xx * NS + bb] : 0.0);
        }
        hrow[i] = v;
    }
}

// V5: level-sorted rows, thread = chunk of <= CH pixels of ONE level; accumulation in registers, no atomics.
//   scol:  [H][W] u16 columns of the row sorted by level (stable)
//   desc:  [H][T] {start, len | level << 16} one chunk per thread (len 0: idle)
//   first: [H][257] first chunk (= thread) of each level
// E[d] = exp(-d^2/hx^2), d = |c - c_b| <= W: the column factors ec[c][b] as ONE LDS table.
template <int NC, int T>
__global__ __launch_bounds__(T) void k_sorted(const unsigned short* __restrict__ scol, const uint2* __restrict__ desc,
                                              const unsigned short* __restrict__ first, GridSpec gs,
                                              const double* __restrict__ Etab, const double* __restrict__ g, double eps,
                                              double* __restrict__ hout) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int n = kLevels * NC;
    const int W = gs.W;
    double* sE = reinterpret_cast<double*>(smem_raw);   // [W + 1]
    double* sP = sE + ((W + 2) & ~1);                    // [T][NC | 1]
    constexpr int PS = NC | 1;
    const int tid = threadIdx.x, lrow = blockIdx.x;
    for (int i = tid; i <= W; i += T) sE[i] = Etab[i];
    const uint2 dsc = desc[(size_t)lrow * T + tid];
    const int start = (int)(dsc.x & 0xffff), stride = (int)(dsc.x >> 16), len = (int)(dsc.y & 0xffff), x = (int)(dsc.y >> 16);
    const double* grow = g + (size_t)lrow * n;
    double gv[NC], acc[NC];
#pragma unroll
    for (int b = 0; b < NC; ++b) {
        gv[b] = grow[b * kLevels + x];
        acc[b] = 0.0;
    }
    __syncthreads();
    const unsigned short* sc = scol + (size_t)lrow * W + start;
    const int cb0 = gs.colOff, cs = gs.colStep;
    for (int t = 0; t < len; ++t) {
        const int c = sc[t * stride];
        double e[NC];
#pragma unroll
        for (int b = 0; b < NC; ++b) e[b] = sE[__sad(c, cb0 + b * cs, 0)];
        double s0 = 0.0, s1 = 0.0;
#pragma unroll
        for (int b = 0; b < NC; ++b) {
            if (b & 1) s1 += e[b] * gv[b];
            else s0 += e[b] * gv[b];
        }
        const double y = recip_or_zero_d(s0 + s1, eps);
#pragma unroll
        for (int b = 0; b < NC; ++b) acc[b] += e[b] * y;
    }
#pragma unroll
    for (int b = 0; b < NC; ++b) sP[tid * PS + b] = acc[b];
    __syncthreads();
    const unsigned short* fr = first + (size_t)lrow * 257;
    double* hrow = hout + (size_t)lrow * n;
    for (int i = tid; i < n; i += T) {
        const int bb = i / kLevels, xx = i & (kLevels - 1);
        double sum = 0.0;
        for (int k = fr[xx]; k < fr[xx + 1]; ++k) sum += sP[k * PS + bb];
        hrow[i] = sum;
    }
}

static unsigned long long splitmix(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main(int argc, char** argv) {
    const int H = 4096, W = 4096, NC = 10, NR = 20;
    const char* image = argc > 1 ? argv[1] : "synthetic";
    GridSpec gs{};
    gs.H = H; gs.W = W; gs.rowStep = H / NR; gs.colStep = W / NC;
    gs.rowOff = (gs.rowStep - 1 + (H - gs.rowStep * NR)) / 2; gs.colOff = (gs.colStep - 1 + (W - gs.colStep * NC)) / 2;
    gs.nSelRows = NR; gs.nSelCols = NC;
    std::vector<float> lum((size_t)H * W);
    const double PI = 3.14159265358979323846;
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) {
            const double a = (double)r / H, b = (double)c / W;
            const double s = 0.5 * sin(2 * PI * (1.5 * a + 0.5 * b)) + 0.5 * cos(2 * PI * (0.7 * a - 2.2 * b));
            const double u = (double)(splitmix(((unsigned long long)r * W + c) ^ 1234ull) >> 11) * (1.0 / 9007199254740992.0);
            double v = std::nearbyint(128.0 + 70.0 * s + 40.0 * (u - 0.5));
            if (std::string(image) == "checker") v = ((r + c) & 1) ? 60 : 200;
            if (std::string(image) == "blocks") v = std::nearbyint(40 + 25 * (((r / 64) * 7 + (c / 64) * 13) % 8) + (u < 0.05 ? 3 : 0));
            if (std::string(image) == "uniform") v = (double)(splitmix(((unsigned long long)r * W + c) ^ 99ull) & 255);
            lum[(size_t)r * W + c] = (float)std::fmin(255.0, std::fmax(0.0, v));
        }
    std::vector<double> ecT((size_t)NC * W), g((size_t)H * 256 * NC);
    const double hx = W / 4.0;
    for (int b = 0; b < NC; ++b)
        for (int c = 0; c < W; ++c) {
            const double d = c - (gs.colOff + b * gs.colStep);
            ecT[(size_t)b * W + c] = exp(-d * d / (hx * hx));
        }
    for (size_t i = 0; i < g.size(); ++i) g[i] = 0.5 + (double)(splitmix(i) >> 11) * (1.0 / 9007199254740992.0);
    float* d_lum; double *d_ecT, *d_g, *d_h;
    CK(hipMalloc(&d_lum, lum.size() * 4)); CK(hipMalloc(&d_ecT, ecT.size() * 8)); CK(hipMalloc(&d_g, g.size() * 8)); CK(hipMalloc(&d_h, g.size() * 8));
    CK(hipMemcpy(d_lum, lum.data(), lum.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_ecT, ecT.data(), ecT.size() * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_g, g.data(), g.size() * 8, hipMemcpyHostToDevice));
    hipEvent_t ea, eb; CK(hipEventCreate(&ea)); CK(hipEventCreate(&eb));
    const size_t shm1 = (size_t)2 * kLevels * 11 * 8, shm2 = (size_t)3 * kLevels * 11 * 8 + 16;
    std::vector<double> ref(g.size()), out(g.size());
    auto timeit = [&](const char* name, auto launch, bool is_ref) {
        for (int i = 0; i < 3; ++i) launch();
        CK(hipEventRecord(ea, 0));
        const int reps = 20;
        for (int i = 0; i < reps; ++i) launch();
        CK(hipEventRecord(eb, 0)); CK(hipEventSynchronize(eb));
        float ms = 0; CK(hipEventElapsedTime(&ms, ea, eb));
        CK(hipMemcpy(out.data(), d_h, out.size() * 8, hipMemcpyDeviceToHost));
        double num = 0, den = 0;
        if (is_ref) ref = out;
        for (size_t i = 0; i < out.size(); ++i) { num += (out[i] - ref[i]) * (out[i] - ref[i]); den += ref[i] * ref[i]; }
        printf("{\"image\": \"%s\", \"variant\": \"%s\", \"us_per_launch\": %.1f, \"rel_l2_vs_V0\": %.2e}\n", image, name, ms * 1000 / reps, sqrt(num / den));
    };
    const double scale = ldexp(1.0, 44);
    timeit("V0 shipping (f64 atomics + pre-reduction)", [&] { hipLaunchKernelGGL((k_hist_pix<10>), dim3(H), dim3(kPixThreads), shm1, 0, ROWPASS_RECIP, d_lum, gs, 0, d_ecT, d_g, 1e-10, nullptr, d_h, nullptr, nullptr); }, true);
    timeit("V1 u64 + pre-reduction", [&] { hipLaunchKernelGGL((k_var<10, 1>), dim3(H), dim3(kPixThreads), shm1, 0, d_lum, gs, 0, d_ecT, d_g, 1e-10, scale, d_h); }, false);
    timeit("V2 u64, no pre-reduction", [&] { hipLaunchKernelGGL((k_var<10, 2>), dim3(H), dim3(kPixThreads), shm1, 0, d_lum, gs, 0, d_ecT, d_g, 1e-10, scale, d_h); }, false);
    timeit("V3 f64, two sub-histograms", [&] { hipLaunchKernelGGL((k_var<10, 3>), dim3(H), dim3(kPixThreads), shm2, 0, d_lum, gs, 0, d_ecT, d_g, 1e-10, scale, d_h); }, false);
    auto run_v5 = [&](auto Tc, bool interleave) {   // host-side preprocessing for V5 (a device kernel in the product; once per train)
        constexpr int T = decltype(Tc)::value;
        std::vector<unsigned short> scol((size_t)H * W), first((size_t)H * 257);
        std::vector<uint2> desc((size_t)H * T);
        long long sumCH = 0; int maxCH = 0;
        for (int r = 0; r < H; ++r) {
            int cnt[256] = {0}, off[257];
            for (int c = 0; c < W; ++c) cnt[(int)lum[(size_t)r * W + c]]++;
            off[0] = 0;
            for (int x = 0; x < 256; ++x) off[x + 1] = off[x] + cnt[x];
            int pos[256];
            for (int x = 0; x < 256; ++x) pos[x] = off[x];
            for (int c = 0; c < W; ++c) scol[(size_t)r * W + pos[(int)lum[(size_t)r * W + c]]++] = (unsigned short)c;
            int CH = (W + T - 1) / T;
            for (;; ++CH) {
                int nch = 0;
                for (int x = 0; x < 256; ++x) nch += (cnt[x] + CH - 1) / CH;
                if (nch <= T) break;
            }
            sumCH += CH; maxCH = std::max(maxCH, CH);
            int k = 0;
            for (int x = 0; x < 256; ++x) {
                first[(size_t)r * 257 + x] = (unsigned short)k;
                const int m = (cnt[x] + CH - 1) / CH;
                for (int j = 0; j < m; ++j, ++k) {
                    if (interleave)   // chunk j of m takes sorted positions j, j + m, j + 2m, ...
                        desc[(size_t)r * T + k] = make_uint2((unsigned)(off[x] + j) | ((unsigned)m << 16), (unsigned)((cnt[x] - j + m - 1) / m) | ((unsigned)x << 16));
                    else
                        desc[(size_t)r * T + k] = make_uint2((unsigned)(off[x] + j * CH) | (1u << 16), (unsigned)std::min(CH, cnt[x] - j * CH) | ((unsigned)x << 16));
                }
            }
            first[(size_t)r * 257 + 256] = (unsigned short)k;
            for (; k < T; ++k) desc[(size_t)r * T + k] = make_uint2(1u << 16, 0);
        }
        std::vector<double> Etab(W + 1);
        for (int d = 0; d <= W; ++d) Etab[d] = exp(-(double)d * d / (hx * hx));
        unsigned short *d_scol, *d_first; uint2* d_desc; double* d_E;
        CK(hipMalloc(&d_scol, scol.size() * 2)); CK(hipMalloc(&d_first, first.size() * 2)); CK(hipMalloc(&d_desc, desc.size() * 8)); CK(hipMalloc(&d_E, Etab.size() * 8));
        CK(hipMemcpy(d_scol, scol.data(), scol.size() * 2, hipMemcpyHostToDevice));
        CK(hipMemcpy(d_first, first.data(), first.size() * 2, hipMemcpyHostToDevice));
        CK(hipMemcpy(d_desc, desc.data(), desc.size() * 8, hipMemcpyHostToDevice));
        CK(hipMemcpy(d_E, Etab.data(), Etab.size() * 8, hipMemcpyHostToDevice));
        const size_t shm5 = (size_t)(((W + 2) & ~1) + T * 11) * 8;
        CK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_sorted<10, T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm5));
        printf("{\"image\": \"%s\", \"V5_mean_chunk\": %.2f, \"V5_max_chunk\": %d}\n", image, (double)sumCH / H, maxCH);
        char nm[128];
        snprintf(nm, sizeof nm, "V5 level-sorted rows, register accumulation, T=%d %s", T, interleave ? "interleaved" : "blocked");
        timeit(nm, [&] { hipLaunchKernelGGL((k_sorted<10, T>), dim3(H), dim3(T), shm5, 0, d_scol, d_desc, d_first, gs, d_E, d_g, 1e-10, d_h); }, false);
        CK(hipFree(d_scol)); CK(hipFree(d_first)); CK(hipFree(d_desc)); CK(hipFree(d_E));
    };
    run_v5(std::integral_constant<int, 512>{}, false);
    run_v5(std::integral_constant<int, 512>{}, true);
    run_v5(std::integral_constant<int, 256>{}, true);
    run_v5(std::integral_constant<int, 1024>{}, true);
    timeit("V4 u64, two sub-histograms", [&] { hipLaunchKernelGGL((k_var<10, 4>), dim3(H), dim3(kPixThreads), shm2, 0, d_lum, gs, 0, d_ecT, d_g, 1e-10, scale, d_h); }, false);
    return 0;
}
