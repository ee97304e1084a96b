// The Nystrom residual map (nle_nystrom_residual): for pixel i with fp64 affinity row k_i (p entries)
//   r_i = 1 - || F^T k_i ||^2,   F (p x m) with F F^T = pinv(K_A) at the reference's cut (solve_Ka: B diag(sqrt(lambda)), or
//   L^-T on the Cholesky route),
// the diagonal of K - K~ for the extension a train uses.  Two device routes:
//   k_nystrom_resid64   FUSED: the affinities are generated in fp64 inside the fp64-MFMA kernel, nothing N x p or N x m is stored
//   k_resid_rows        ROWS:  the per-row epilogue behind AffinityRows64 + ts_gemm64 (any affinity option, p <= 2048)
// Both write (float)r_i and one summary partial {sum r, max r, index of the first maximum, count r > thresh} per tile of
// kResidTile pixels, all from the unrounded fp64 r_i; k_resid_finish folds the partials in a fixed order.
#include "kernels.h"
#include "launch.h"

#include <algorithm>

namespace nlek {

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {
struct Summary {
    double sum, mx, idx, cnt;  // idx, cnt: integers < 2^31, exact in a double
};
// the later operand wins only when it is larger, or as large at a smaller index: the first maximum
__device__ __forceinline__ void fold(Summary& a, const Summary& b) {
    a.sum += b.sum;
    a.cnt += b.cnt;
    if (b.mx > a.mx || (b.mx == a.mx && b.idx < a.idx)) a.mx = b.mx, a.idx = b.idx;
}
__device__ __forceinline__ Summary shfl_xor(const Summary& a, int off) {
    return Summary{__shfl_xor(a.sum, off), __shfl_xor(a.mx, off), __shfl_xor(a.idx, off), __shfl_xor(a.cnt, off)};
}
__device__ __forceinline__ Summary summary_of(double r, long long gi, bool valid, double thresh) {
    // 2^62: larger than any pixel index
    return valid ? Summary{r, r, (double)gi, r > thresh ? 1.0 : 0.0} : Summary{0.0, -__builtin_inf(), 4611686018427387904.0, 0.0};
}
// The summary partial of one tile: every thread of the workgroup brings at most one pixel.  Butterfly inside the wave (each
// level adds the same two values on both lanes, so all lanes hold the same bits), then wave by wave in LDS: one order.
template <int NWAVES>
__device__ __forceinline__ void tile_summary(Summary v, double* sred /* NWAVES * 4 */, double* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const Summary o = shfl_xor(v, off);
        // both lanes of a pair fold (lower lane's value, upper lane's value) in that order
        Summary lo = (lane & off) ? o : v;
        const Summary hi = (lane & off) ? v : o;
        fold(lo, hi);
        v = lo;
    }
    if (lane == 0) sred[wave * 4 + 0] = v.sum, sred[wave * 4 + 1] = v.mx, sred[wave * 4 + 2] = v.idx, sred[wave * 4 + 3] = v.cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        Summary t{sred[0], sred[1], sred[2], sred[3]};
#pragma unroll
        for (int w = 1; w < NWAVES; ++w) fold(t, Summary{sred[w * 4 + 0], sred[w * 4 + 1], sred[w * 4 + 2], sred[w * 4 + 3]});
        out[0] = t.sum, out[1] = t.mx, out[2] = t.idx, out[3] = t.cnt;
    }
}

// K(i, s) in fp64, k_affinity64's operations in k_affinity64's order (and build_Ka's on the host): integer spatial term,
// every operation rounded on its own, libm exp
__device__ __forceinline__ double affinity64_value(int row, int col, double x, int2 rc, double sv, double sw, double pw) {
#pragma clang fp contract(off)
    const long long dr = row - rc.x, dc = col - rc.y;
    const double dv = x - sv;
    return exp(-sw * (double)(dr * dr + dc * dc) - pw * (dv * dv));
}
}  // namespace

// ------------------------------------------------------------------ FUSED: r_i on the fp64 MFMA, affinities in registers
// k_project64's mapping: lane (l15, kq) makes the A operand of v_mfma_f64_16x16x4_f64 -- the affinity of pixel l15 of the
// wave's 16 to sample k0 + kq -- and reads B = F[sample][column n*16 + l15] from LDS, where F is staged in chunks of
// kResidKB samples (the next chunk's loads are in flight while the current one is contracted).  A wave keeps ALL NT = m / 16
// column tiles of its 16 pixels in registers (NT <= 16: 128 accumulator registers), so every fp64 exponential is computed once
// -- with the libm exp on the VALU that, not the MFMA count, is what a second pixel tile per wave or a second column panel
// would double.  Epilogue: per accumulator row the squares are summed over the tiles in ascending n, then over the 16 lanes
// of the row by xor-shuffles; lane (kq, e < 4) owns pixel kq + 4 e.  Workgroup = 8 waves = one tile of kResidTile pixels.
constexpr int kResidKB = 32;
constexpr int kResidWaves = kResidTile / 16;
constexpr int kResidMaxP = 256;
__host__ __device__ constexpr int resid_ldb(int nt) { return nt * 16 + ((nt & 1) ? 0 : 16); }  // == 16 (mod 32) doubles
__host__ __device__ constexpr size_t resid_lds_bytes(int nt) {
    return (size_t)kResidKB * resid_ldb(nt) * sizeof(double) + (size_t)kResidMaxP * (sizeof(double) + sizeof(int2)) +
           (size_t)kResidWaves * 4 * sizeof(double);
}

template <int NT>
__global__ __launch_bounds__(kResidWaves * 64) void k_nystrom_resid64(const float* __restrict__ lum, GridSpec gs,
                                                                      const Sample4* __restrict__ samples, int p, double sw,
                                                                      double pw, long long N, const double* __restrict__ F,
                                                                      int ldf, double thresh, float* __restrict__ r_out,
                                                                      double* __restrict__ part) {
    constexpr int LDB = resid_ldb(NT);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_resid[];
    double* sB = reinterpret_cast<double*>(smem_resid);               // [kResidKB][LDB]
    double* sval = sB + (size_t)kResidKB * LDB;                       // [kResidMaxP]
    int2* src = reinterpret_cast<int2*>(sval + kResidMaxP);           // [kResidMaxP]
    double* sred = reinterpret_cast<double*>(src + kResidMaxP);       // [kResidWaves * 4]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kq = lane >> 4;
    const int pk = (p + kResidKB - 1) / kResidKB * kResidKB;  // <= kResidMaxP; samples >= p: zeros (their rows of F are zero)
    for (int k = tid; k < pk; k += kResidWaves * 64) {
        const Sample4 v = k < p ? samples[k] : make_float4(0.f, 0.f, 0.f, 0.f);
        src[k] = make_int2((int)v.x, (int)v.y);
        sval[k] = (double)v.z;
    }
    const long long m0 = (long long)blockIdx.x * kResidTile + wave * 16;
    long long li = m0 + l15;
    if (li >= N) li = N - 1;
    const int row = (int)(li / gs.W), col = (int)(li - (long long)row * gs.W);
    const double x = (double)lum[li];

    f64x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = f64x4{0.0, 0.0, 0.0, 0.0};
    // staging: thread -> row tid / 16 of the chunk, columns n * 16 + tid % 16 (kResidKB * 16 == the workgroup's threads)
    const int srow = tid >> 4, scol = tid & 15;
    double pre[NT];
    auto fetch = [&](int k0) {
        const bool ok = k0 + srow < p;
        const double* f = F + (size_t)(ok ? k0 + srow : 0) * ldf + scol;
#pragma unroll
        for (int n = 0; n < NT; ++n) {
            const double v = f[n * 16];
            pre[n] = ok ? v : 0.0;
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < p; k0 += kResidKB) {
        __syncthreads();  // the previous chunk is contracted (first pass: the sample tables are written)
#pragma unroll
        for (int n = 0; n < NT; ++n) sB[srow * LDB + n * 16 + scol] = pre[n];
        __syncthreads();
        if (k0 + kResidKB < p) fetch(k0 + kResidKB);
#pragma unroll 2
        for (int kk = 0; kk < kResidKB; kk += 4) {
            const int s = k0 + kk + kq;
            const double a = affinity64_value(row, col, x, src[s], sval[s], sw, pw);
            const double* brow = sB + (kk + kq) * LDB + l15;
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, brow[n * 16], acc[n], 0, 0, 0);
        }
    }
    // || t ||^2 of the rows kq + 4 e: ascending column tile, then the 16 lanes of the row
    double ss[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int e = 0; e < 4; ++e) ss[e] += acc[n][e] * acc[n][e];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) ss[e] += __shfl_xor(ss[e], off);
    double mine = ss[0];
#pragma unroll
    for (int e = 1; e < 4; ++e) mine = (l15 == e) ? ss[e] : mine;
    const double r = 1.0 - mine;
    const long long gi = m0 + kq + 4 * l15;  // (l15 < 4)
    const bool valid = l15 < 4 && gi < N;
    if (valid && r_out) r_out[gi] = (float)r;
    tile_summary<kResidWaves>(summary_of(r, gi, valid, thresh), sred, part + (size_t)blockIdx.x * 4);
}

bool resid_fused_applies(int p) { return p >= 1 && p <= kResidMaxP; }
int resid_fused_ld(int m) { return (m + 15) & ~15; }

// Not through launch(): the LDS size is a constant of the instantiation, so its limit is raised once per process and not
// asked about again on every call of a map that is launched chunk after chunk.
template <int NT>
static hipError_t launch_nystrom_resid64(hipStream_t s, const float* d_lum, GridSpec gs, const Sample4* d_samples, int p,
                                         double sw, double pw, long long N, const double* d_F, int ldf, double thresh,
                                         float* d_r, double* d_part) {
    constexpr size_t shm = resid_lds_bytes(NT);
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(k_nystrom_resid64<NT>),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);  // once
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL((k_nystrom_resid64<NT>), dim3((unsigned)resid_num_parts(N)), dim3(kResidWaves * 64), shm, s, d_lum, gs,
                       d_samples, p, sw, pw, N, d_F, ldf, thresh, d_r, d_part);
    return hipGetLastError();
}

hipError_t nystrom_resid64(hipStream_t s, const float* d_lum, GridSpec gs, const Sample4* d_samples, int p, double sw, double pw,
                           long long N, const double* d_F, int m, double thresh, float* d_r, double* d_part) {
    if (N <= 0) return hipSuccess;
    if (!resid_fused_applies(p) || m < 1 || m > p) return hipErrorInvalidValue;
    const int ldf = resid_fused_ld(m);
    hipError_t e = hipErrorInvalidValue;  // m beyond 256 columns: no launch
    dispatch_columns<1, 16>(ldf / 16, [&](auto nt) {
        e = launch_nystrom_resid64<decltype(nt)::value>(s, d_lum, gs, d_samples, p, sw, pw, N, d_F, ldf, thresh, d_r, d_part);
    });
    return e;
}

// ------------------------------------------------------------------ ROWS: r_i = 1 - sum_j T(i, j)^2, j ascending
// T (M x ldt, logical width m) = the chunk's affinity rows times F.  A workgroup takes kResidTile rows: 32 columns at a time
// go through LDS (coalesced 256-byte row segments in, one thread per row out), so that a row's squares are added in ascending
// j in one chain.  i0: the chunk's first pixel, a multiple of kResidTile -- the tiles, and with them the summary partials, are
// the same however the plane is cut into chunks.
__global__ __launch_bounds__(256) void k_resid_rows(const double* __restrict__ T, long long M, int ldt, int m, long long i0,
                                                    double thresh, float* __restrict__ r_out, double* __restrict__ part) {
    __shared__ double sT[kResidTile][33];
    __shared__ double sred[4 * 4];
    const int tid = threadIdx.x, c = tid & 31, g = tid >> 5;
    const long long b0 = (long long)blockIdx.x * kResidTile;
    double ss = 0.0;
    for (int j0 = 0; j0 < m; j0 += 32) {
        __syncthreads();
#pragma unroll 4
        for (int rr = g; rr < kResidTile; rr += 8) {
            const long long i = b0 + rr;
            sT[rr][c] = (i < M && j0 + c < m) ? T[(size_t)i * ldt + j0 + c] : 0.0;
        }
        __syncthreads();
        if (tid < kResidTile) {
            const int w = min(32, m - j0);
            for (int j = 0; j < w; ++j) ss += sT[tid][j] * sT[tid][j];
        }
    }
    const double r = 1.0 - ss;
    const long long li = b0 + tid, gi = i0 + li;
    const bool valid = tid < kResidTile && li < M;
    if (valid && r_out) r_out[gi] = (float)r;
    tile_summary<4>(summary_of(r, gi, valid, thresh), sred, part + (size_t)(i0 / kResidTile + blockIdx.x) * 4);
}

hipError_t resid_rows64(hipStream_t s, const double* d_T, long long M, int ldt, int m, long long i0, double thresh, float* d_r,
                        double* d_part) {
    if (M <= 0) return hipSuccess;
    if (i0 % kResidTile || m < 1 || ldt < m) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_resid_rows, dim3((unsigned)resid_num_parts(M)), dim3(256), 0, s, d_T, M, ldt, m, i0, thresh, d_r, d_part);
    return hipGetLastError();
}

// ------------------------------------------------------------------ second stage: the partials in one fixed order
// thread t folds partials t, t + 256, ... in ascending order, then the 256 threads fold pairwise in LDS
__global__ __launch_bounds__(256) void k_resid_finish(const double* __restrict__ part, long long nparts, double* __restrict__ out) {
    __shared__ double sm[256][4];
    const int t = threadIdx.x;
    Summary v = summary_of(0.0, 0, false, 0.0);
    for (long long b = t; b < nparts; b += 256) fold(v, Summary{part[b * 4 + 0], part[b * 4 + 1], part[b * 4 + 2], part[b * 4 + 3]});
    sm[t][0] = v.sum, sm[t][1] = v.mx, sm[t][2] = v.idx, sm[t][3] = v.cnt;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if (t < half) {
            Summary a{sm[t][0], sm[t][1], sm[t][2], sm[t][3]};
            fold(a, Summary{sm[t + half][0], sm[t + half][1], sm[t + half][2], sm[t + half][3]});
            sm[t][0] = a.sum, sm[t][1] = a.mx, sm[t][2] = a.idx, sm[t][3] = a.cnt;
        }
        __syncthreads();
    }
    if (t == 0) out[0] = sm[0][0], out[1] = sm[0][1], out[2] = sm[0][2], out[3] = sm[0][3];
}

hipError_t resid_finish(hipStream_t s, const double* d_part, long long nparts, double* d_out) {
    if (nparts <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_resid_finish, dim3(1), dim3(256), 0, s, d_part, nparts, d_out);
    return hipGetLastError();
}

}  // namespace nlek
