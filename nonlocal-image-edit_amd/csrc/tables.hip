// The table formulation: the tiled Sinkhorn pass, the sample-space apply and the Gram on look-up tables
// of the quantised plane; the composite launchers take one nlek::TableView (kernels.h).  Level-sorted pixel halves: sorted.hip.
#include "kernels.h"
#include "launch.h"

#include <algorithm>

namespace nlek {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// ==================================================================== quantised-luminance fast path
// When the luminance plane is integer valued in [0, 255] -- it always is in the reference's
// pipeline, where it is the L channel of an 8-bit Lab image (src/filter.cpp:460-469) -- and
// because the sample set is a Cartesian grid (samplePixels, :56-80: sample s = (a, b), row a of
// nR, column b of nC), the affinity factorises into three table look-ups
//     k_i[s] = er[row_i][a] * ec[col_i][b] * Ep[x_i][s],
//     er[r][a] = exp(-(r - row_a)^2/hx^2), ec[c][b] = exp(-(c - col_b)^2/hx^2), Ep[x][s] = exp(-(x - y_s)^2/hy^2)
// (all fp64, exact integer arguments).  A Sinkhorn half-iteration for one image row r becomes
//     g[x][b]   = sum_a er[r][a] w[a,b] Ep[x][a,b]                       (256 x nC table, LDS)
//     d_i       = sum_b ec[c_i][b] g[x_i][b],  y_i = recip(d_i)          (nC fma per pixel)
//     h[x][b]  += ec[c_i][b] y_i                                          (LDS histogram)
//     z[a,b]   += er[r][a] sum_x Ep[x][a,b] h[x][b]
// i.e. 2 nC multiply-adds per pixel instead of p exponentials and 2p fp64 fma, in fp64 throughout.
constexpr int kLevels = 256;

// ---- wave-level pre-reduction for the LDS histograms
// Flat image regions put many lanes of a wave on ONE histogram level, and same-address LDS atomics
// serialise (a flat row ran the pass 4.5x slower than a noisy one).  Before the atomics, up to
// kGroupRounds levels that at least kGroupMin lanes of the wave share are summed across the wave on
// the VALU (DPP) and added once by lane 63; the remaining lanes use their own atomics.
constexpr int kGroupMin = 12;
constexpr int kGroupRounds = 3;

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64(double v) {  // lanes without a source (or masked rows) read 0
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xf, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xf, true);
    return __hiloint2double(hi, lo);
}
// sum over the 64 lanes, valid in lane 63 (all lanes must be active)
__device__ __forceinline__ double wave_sum63(double v) {
    v += dpp_f64<0xB1, 0xf>(v);   // quad_perm [1,0,3,2]
    v += dpp_f64<0x4E, 0xf>(v);   // quad_perm [2,3,0,1]
    v += dpp_f64<0x141, 0xf>(v);  // row_half_mirror
    v += dpp_f64<0x140, 0xf>(v);  // row_mirror: every lane holds its row's sum
    v += dpp_f64<0x142, 0xa>(v);  // row_bcast15 into rows 1 and 3
    v += dpp_f64<0x143, 0xc>(v);  // row_bcast31 into rows 2 and 3
    return v;
}
// Calls grouped(level, mine) for each level handled by a wave sum (wave-uniform call, `mine` marks the
// lanes of that level) and returns whether this lane still has to add its own value.
template <class G>
__device__ __forceinline__ bool wave_group_levels(bool active, int x, G&& grouped) {
    bool pend = active, tried = false;
#pragma unroll 1
    for (int round = 0; round < kGroupRounds; ++round) {
        const unsigned long long cand = __ballot(pend && !tried);
        if (cand == 0) break;
        const int lx = __builtin_amdgcn_readlane(x, __ffsll((long long)cand) - 1);
        const bool mine = pend && x == lx;
        const int cnt = __popcll(__ballot(mine));
        if (cnt >= kGroupMin) {
            grouped(lx, mine);
            if (mine) pend = false;
        } else {
            if (cnt < 3) break;  // a noisy stretch: no point in trying further leaders
            if (mine) tried = true;
        }
    }
    return pend;
}

__global__ __launch_bounds__(256) void k_check_levels(const float* __restrict__ lum, long long n,
                                                      int* __restrict__ flag) {
    bool bad = false;
    unsigned tiles = 0;  // bit t: some pixel has a level in [16 t, 16 t + 16)
    auto look = [&](const float v) {
        const bool ok = v >= 0.f && v <= (float)(kLevels - 1) && v == floorf(v);
        bad = bad || !ok;
        if (ok) tiles |= 1u << ((int)v >> 4);
    };
    // 16-byte loads on the aligned body of the plane (4-byte loads ran this 67 MB read at 0.6 TB/s), scalars at both ends
    const long long head = min(n, (long long)((4 - ((reinterpret_cast<unsigned long long>(lum) >> 2) & 3)) & 3));
    const long long nv = (n - head) >> 2;
    const float4* body = reinterpret_cast<const float4*>(lum + head);
    const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x, gsz = (long long)gridDim.x * blockDim.x;
    for (long long i = gtid; i < nv; i += gsz) {
        const float4 v = body[i];
        look(v.x);
        look(v.y);
        look(v.z);
        look(v.w);
    }
    for (long long i = gtid; i < head; i += gsz) look(lum[i]);
    for (long long i = head + 4 * nv + gtid; i < n; i += gsz) look(lum[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tiles |= __shfl_xor(tiles, off);
    const bool any_bad = __any(bad);  // a vote of the whole wave: taken before the lanes part ways
    // one atomic per workgroup (one per wave, 16k of them on the same word, cost more than the 67 MB read)
    __shared__ unsigned s_tiles[4];
    __shared__ int s_bad[4];
    if ((threadIdx.x & 63) == 0) {
        s_tiles[threadIdx.x >> 6] = tiles;
        s_bad[threadIdx.x >> 6] = any_bad ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]) atomicOr(flag, 1);
        atomicOr(flag + 1, (int)(s_tiles[0] | s_tiles[1] | s_tiles[2] | s_tiles[3]));
    }
}

// d_flag: 2 ints.  [0] != 0: the plane is not integer valued in [0, 255]; [1]: which 16-level tiles occur (bit t)
hipError_t check_levels(hipStream_t s, const float* d_lum, long long n, int* d_flag) {
    hipError_t e = hipMemsetAsync(d_flag, 0, 2 * sizeof(int), s);
    if (e != hipSuccess) return e;
    long long g = (n + 255) / 256;
    if (g > 1024) g = 1024;
    hipLaunchKernelGGL(k_check_levels, dim3((unsigned)g), dim3(256), 0, s, d_lum, n, d_flag);
    return hipGetLastError();
}

// er: [nrows_local][nR], ecT: [nC][W], Ep: [256][p]
__global__ void k_hist_tables(GridSpec gs, const Sample4* __restrict__ samples, int p, double inv_hx2,
                              double inv_hy2, int row0, int nrows_local, double* __restrict__ er,
                              double* __restrict__ ecT, double* __restrict__ Ep) {
    const long long n_er = (long long)nrows_local * gs.nSelRows, n_ec = (long long)gs.nSelCols * gs.W,
                    n_ep = (long long)kLevels * p;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_er + n_ec + n_ep;
         i += (long long)gridDim.x * blockDim.x) {
        if (i < n_er) {
            const int r = row0 + (int)(i / gs.nSelRows), a = (int)(i % gs.nSelRows);
            const double d = (double)(r - (gs.rowOff + a * gs.rowStep));
            er[i] = exp(-(d * d) * inv_hx2);
        } else if (i < n_er + n_ec) {
            const long long j = i - n_er;
            const int b = (int)(j / gs.W), c = (int)(j % gs.W);
            const double d = (double)(c - (gs.colOff + b * gs.colStep));
            ecT[j] = exp(-(d * d) * inv_hx2);
        } else {
            const long long j = i - n_er - n_ec;
            const int x = (int)(j / p), sidx = (int)(j % p);
            const double d = (double)x - (double)samples[sidx].z;
            Ep[j] = exp(-(d * d) * inv_hy2);
        }
    }
}

hipError_t hist_tables(hipStream_t s, GridSpec gs, const Sample4* d_samples, int p, double hx, double hy, int row0,
                       int nrows_local, double* d_er, double* d_ecT, double* d_Ep) {
    hipLaunchKernelGGL(k_hist_tables, dim3(256), dim3(256), 0, s, gs, d_samples, p, 1.0 / (hx * hx), 1.0 / (hy * hy),
                       row0, nrows_local, d_er, d_ecT, d_Ep);
    return hipGetLastError();
}

// -------------------------------------------------------------------- tiled form of the table pass
// As one kernel with a workgroup per image row, the pass re-reads the whole Ep table (256 x p doubles) twice per row
// from L2, which is what bounds it.  The tiled form splits the pass into three kernels so that Ep is read ~once:
//   k_hist_g   : g[r][b,x] = sum_a er[r][a] w[a,b] Ep[x][a,b]   (fp64 MFMA; table columns are b-major)
//   k_hist_pix : per image row: d_i, y_i, h[r][x,b] += ec y      (g row and h row in LDS)
//   k_hist_hh  : HH[slab][x,b][a] = sum_{r in slab} er[r][a] h[r][x,b]
//   k_hist_z   : z[a,b] = sum_x Ep[x][a,b] sum_slab HH[slab][x,b][a]
// G (nrows x 256 nC) = er (nrows x nR) * WE (nR x 256 nC), WE[a][x,b] = w[a,b] Ep[x][a,b], on the fp64
// MFMA: a wave keeps the WE operands of its 16 columns in registers (nR <= 32: 8 k-steps of 4) and walks
// down `tiles_per_wave` 16-row tiles -- five loads, five MFMAs and one 16 x 16 store per tile at cfg4, so
// the kernel runs at the speed of its 8 B/element output stream.
// lev_t0, lev_nt: the 16-level tiles [lev_t0, lev_t0 + lev_nt) that occur in the image -- columns of other levels are never
// read by anybody and are not made.
__global__ __launch_bounds__(256) void k_hist_g(GridSpec gs, int p, int nrows, int tiles_per_wave, int lev_t0, int lev_nt,
                                                const double* __restrict__ er, const double* __restrict__ Ep,
                                                const double* __restrict__ w, double* __restrict__ g) {
    // the er rows of this workgroup's row range, staged once (coalesced) -- a per-tile global load of the A operand put
    // one memory latency on every 16-row tile, which is what bounded the kernel (25 us for an 84 MB stream at cfg4)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* sEr = reinterpret_cast<double*>(smem_raw);  // [tiles_per_wave * 16][nR]
    const int nC = gs.nSelCols, nR = gs.nSelRows, n = kLevels * nC;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kq = lane >> 4;
    const int t0 = blockIdx.y * tiles_per_wave, ntiles = (nrows + 15) >> 4;
    const int rbase = t0 * 16, rcount = min(nrows - rbase, tiles_per_wave * 16);
    for (int i = tid; i < rcount * nR; i += 256) sEr[i] = er[(size_t)rbase * nR + i];
    const int q = blockIdx.x * 4 + wave;  // column tile: sample column b = q / lev_nt, level tile lev_t0 + q % lev_nt
    const bool col_ok = q < nC * lev_nt;
    const int b = col_ok ? q / lev_nt : 0, x = (lev_t0 + (col_ok ? q % lev_nt : 0)) * 16 + l15;
    const int col = b * kLevels + x;  // table columns are b-major: col = b*256 + x
    double bop[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        const int a = ks * 4 + kq;
        bop[ks] = (col_ok && a < nR) ? w[a * nC + b] * Ep[(size_t)x * p + a * nC + b] : 0.0;
    }
    __syncthreads();
    if (!col_ok) return;  // wave-uniform (after the barrier)
    const int ksteps = (nR + 3) >> 2;
    for (int t = t0; t < min(ntiles, t0 + tiles_per_wave); ++t) {
        const int rl = (t - t0) * 16 + l15;  // row within the staged range
        double aop[8];
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const int a = ks * 4 + kq;
            aop[ks] = (ks < ksteps && rl < rcount && a < nR) ? sEr[rl * nR + a] : 0.0;
        }
        f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
            if (ks < ksteps) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[ks], bop[ks], acc, 0, 0, 0);
        if (col_ok) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int ro = t * 16 + kq + 4 * e;
                if (ro < nrows) g[(size_t)ro * n + col] = acc[e];
            }
        }
    }
}

static hipError_t launch_hist_g(hipStream_t s, GridSpec gs, int p, int nrows_local, const double* d_er, const double* d_Ep,
                                const double* d_w, double* d_g, int lev_t0 = 0, int lev_nt = kLevels / 16) {
    const int ntiles = (nrows_local + 15) / 16;
    const int gx = (gs.nSelCols * lev_nt + 3) / 4;
    // ~2560 waves on the chip (or one row tile per wave if the slab is short); at most 16 tiles (256 rows x nR <= 32
    // doubles = 64 KB of LDS) per workgroup
    const int cap = gs.nSelRows > 24 ? 8 : 16;  // the staged er rows: <= 32 KB of LDS per workgroup (cfg5: -3 % on the Sinkhorn stage)
    const int chunks = std::max(1, std::min(ntiles, std::max((640 + gx - 1) / gx, (ntiles + cap - 1) / cap)));
    const int tpw = (ntiles + chunks - 1) / chunks;
    const size_t shm = (size_t)tpw * 16 * gs.nSelRows * sizeof(double);
    return launch(k_hist_g, dim3((unsigned)gx, (unsigned)((ntiles + tpw - 1) / tpw)), dim3(256), shm, s, gs, p, nrows_local, tpw,
                  lev_t0, lev_nt, d_er, d_Ep, d_w, d_g);
}

constexpr int kPixThreads = 512;
template <int NC>  // NC = nSelCols: compile-time so that the per-pixel loops carry no branches
__global__ __launch_bounds__(kPixThreads) void k_hist_pix(int mode, const float* __restrict__ lum, GridSpec gs, int row0,
                                                  const double* __restrict__ ecT, const double* __restrict__ g,
                                                  double eps, double* __restrict__ ybuf, double* __restrict__ hout,
                                                  const double* __restrict__ cvec, const float* __restrict__ xvec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int n = kLevels * NC;
    constexpr int NS = NC | 1;  // odd row stride (in doubles): spreads the levels of a wave over the LDS banks
    const int W = gs.W;
    double* sg = reinterpret_cast<double*>(smem_raw);  // [256][NS]
    double* sh = sg + kLevels * NS;                     // [256][NS]
    const int tid = threadIdx.x, lrow = blockIdx.x, r = row0 + lrow;
    const double* grow = g + (size_t)lrow * n;
    for (int i = tid; i < n; i += kPixThreads) {
        const int bb = i / kLevels, xx = i & (kLevels - 1);  // global tables are b-major, the LDS copies level-major
        sh[xx * NS + bb] = 0.0;
        sg[xx * NS + bb] = (mode == ROWPASS_RECIP) ? grow[i] : 0.0;
    }
    __syncthreads();
    const int dr = r - gs.rowOff;
    const bool sample_row = dr >= 0 && (dr % gs.rowStep) == 0 && (dr / gs.rowStep) < gs.nSelRows;
    for (int c0 = 0; c0 < W; c0 += kPixThreads) {  // wave-uniform trip count: the body uses cross-lane sums
        const bool inside = c0 + tid < W;
        const int c = inside ? c0 + tid : W - 1;
        const int x = (int)lum[(size_t)r * W + c];
        bool smp = !inside;
        if (sample_row) {
            const int dc = c - gs.colOff;
            smp = smp || (dc >= 0 && (dc % gs.colStep) == 0 && (dc / gs.colStep) < NC);
        }
        double e[NC];
#pragma unroll
        for (int b = 0; b < NC; ++b) e[b] = ecT[(size_t)b * W + c];
        double y = 1.0;
        if (mode == ROWPASS_XVEC) {  // apply: y_i = c_i x_i; c at a sample pixel is not read (kernels.h)
            y = smp ? 0.0 : cvec[(size_t)lrow * W + c] * (double)xvec[(size_t)r * W + c];
        } else if (mode == ROWPASS_RECIP) {
            double gv[NC];
#pragma unroll
            for (int b = 0; b < NC; ++b) gv[b] = sg[x * NS + b];
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int b = 0; b < NC; ++b) {
                if (b & 1) s1 += e[b] * gv[b];
                else s0 += e[b] * gv[b];
            }
            y = recip_or_zero_d(s0 + s1, eps);
        }
        if (smp) y = 0.0;
        if (ybuf != nullptr && inside) ybuf[(size_t)lrow * W + c] = y;
        const bool own = wave_group_levels(y != 0.0, x, [&](int lx, bool mine) {
#pragma unroll
            for (int b = 0; b < NC; ++b) {
                const double t = wave_sum63(mine ? e[b] * y : 0.0);
                if ((tid & 63) == 63) atomicAdd(&sh[lx * NS + b], t);
            }
        });
        if (own) {
#pragma unroll
            for (int b = 0; b < NC; ++b) atomicAdd(&sh[x * NS + b], e[b] * y);
        }
    }
    __syncthreads();
    double* hrow = hout + (size_t)lrow * n;
    for (int i = tid; i < n; i += kPixThreads) {
        const int bb = i / kLevels, xx = i & (kLevels - 1);
        hrow[i] = sh[xx * NS + bb];
    }
}

// apply, expand half: out[i] = (float)(c_i * sum_b ec[c_i][b] g_r[x_i][b]) with g built from w' = D (f o t)
// Up to kDotLayers layers per launch: the tables of the launch's layers sit side by side in LDS, so the pixel's
// level, its nC column factors and c_i are loaded once for all of them.
constexpr int kDotLayers = 4;
constexpr int kDotThreads = 512;
template <int NC>
__global__ __launch_bounds__(kDotThreads) void k_hist_dot(const float* __restrict__ lum, GridSpec gs, int row0,
                                                          const double* __restrict__ ecT, const double* __restrict__ g,
                                                          size_t gstride, int nl, const double* __restrict__ cvec,
                                                          float* __restrict__ out, long long ostride, int round8) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr int n = kLevels * NC;
    constexpr int NS = NC | 1;  // odd row stride, as in k_hist_pix
    constexpr int TS = kLevels * NS;
    const int W = gs.W;
    double* sg = reinterpret_cast<double*>(smem_raw);  // [nl][256][NS]
    const int tid = threadIdx.x, lrow = blockIdx.x, r = row0 + lrow;
    for (int l = 0; l < nl; ++l) {
        const double* grow = g + (size_t)l * gstride + (size_t)lrow * n;
        for (int i = tid; i < n; i += kDotThreads) sg[l * TS + (i & (kLevels - 1)) * NS + i / kLevels] = grow[i];  // b-major -> level-major
    }
    __syncthreads();
    const int dr = r - gs.rowOff;
    const bool sample_row = dr >= 0 && (dr % gs.rowStep) == 0 && (dr / gs.rowStep) < gs.nSelRows;
    for (int c = tid; c < W; c += kDotThreads) {
        const int x = (int)lum[(size_t)r * W + c];
        const int dc = c - gs.colOff;
        const bool smp = sample_row && dc >= 0 && (dc % gs.colStep) == 0 && (dc / gs.colStep) < NC;
        const double cv = smp ? 0.0 : cvec[(size_t)lrow * W + c];  // c at a sample pixel is nobody's to read (kernels.h)
        double e[NC];
#pragma unroll
        for (int b = 0; b < NC; ++b) e[b] = ecT[(size_t)b * W + c];
#pragma unroll 1
        for (int l = 0; l < nl; ++l) {
            const double* t = sg + l * TS + x * NS;
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int b = 0; b < NC; ++b) {
                if (b & 1) s1 += e[b] * t[b];
                else s0 += e[b] * t[b];
            }
            double v = cv * (s0 + s1);
            if (round8) v = rint(fmin(255.0, fmax(0.0, v)));  // src/filter.cpp:434-436 on the fp64 value (k_sorted_expand)
            out[(size_t)l * ostride + (size_t)lrow * W + c] = (float)v;
        }
    }
}

// p-, K-sized half of the sample-space apply (one workgroup):
//   t = D^T m + Vrows^T x_A,  W'[l] = D (resp_l o t),  YA[l][a] = Vrows[a] . (resp_l o t)
// D, Vrows: p x ldk row-major fp64; m: p column sums sum_i k_i c_i x_i; xA: x at the p sample pixels
__global__ __launch_bounds__(256) void k_apply_small(int p, int K, int ldk, int L, int ldw, const double* __restrict__ m,
                                                     const double* __restrict__ Dm, const double* __restrict__ Vrows,
                                                     const double* __restrict__ xA, const double* __restrict__ resp,
                                                     double* __restrict__ t_out, double* __restrict__ Wp,
                                                     double* __restrict__ YA, const int* __restrict__ differs,
                                                     const double* __restrict__ m_same, const double* __restrict__ xA_same) {
    if (differs != nullptr && *differs == 0) m = m_same, xA = xA_same;  // the plane training left its reduce half for
    // one workgroup per layer l = blockIdx.x; each recomputes t (K values, p terms each: cheaper than a second launch)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* sm = reinterpret_cast<double*>(smem_raw);  // [p]
    double* sx = sm + p;                                // [p]
    double* st = sx + p;                                // [K]
    double* sp = st + K;                                // [G][KP] partial sums of t
    const int tid = threadIdx.x, l = blockIdx.x;
    const int KP = K <= 64 ? 64 : 128, G = 256 / KP;
    for (int a = tid; a < p; a += 256) {
        sm[a] = m[a];
        sx[a] = xA[a];
    }
    __syncthreads();
    {
        const int k = tid % KP, g = tid / KP;
        double s0 = 0.0, s1 = 0.0;
        if (k < K)
            for (int a = g; a < p; a += G) {
                s0 += Dm[(size_t)a * ldk + k] * sm[a];
                s1 += Vrows[(size_t)a * ldk + k] * sx[a];
            }
        sp[g * KP + k] = s0 + s1;
    }
    __syncthreads();
    for (int k = tid; k < K; k += 256) {
        double s = 0.0;
        for (int g = 0; g < G; ++g) s += sp[g * KP + k];  // fixed order
        st[k] = s;
        if (l == 0) t_out[k] = s;
    }
    __syncthreads();
    const double* rl = resp + (size_t)l * K;
    for (int a = tid; a < ldw; a += 256) {
        double w = 0.0, ya = 0.0;
        if (a < p) {
            for (int k = 0; k < K; ++k) {
                const double gk = rl[k] * st[k];
                w += Dm[(size_t)a * ldk + k] * gk;
                ya += Vrows[(size_t)a * ldk + k] * gk;
            }
            YA[(size_t)l * p + a] = ya;
        }
        Wp[(size_t)l * ldw + a] = w;
    }
}

// Y[l][loc[a]] = YA[l][a] for the samples this rank owns (loc < 0: not local)
__global__ void k_scatter_samples(int p, int L, const long long* __restrict__ loc, const double* __restrict__ YA,
                                  float* __restrict__ Y, long long ystride, int round8) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= L * p) return;
    const int l = o / p, a = o - l * p;
    double v = YA[o];
    if (round8) v = rint(fmin(255.0, fmax(0.0, v)));
    if (loc[a] >= 0) Y[(size_t)l * ystride + loc[a]] = (float)v;
}

// HH[slab][a][col] = sum over the slab's image rows of er[r][a] h[r][col], col = x*nC + b: per slab a
// (nR x slab_rows) x (slab_rows x 256 nC) product on the fp64 MFMA.  One wave per 16 columns and slab; the
// slab's 16 row loads of a lane are independent, so they are all in flight together.
// grid (ceil(16 nC / 4), nslabs), slab_rows == 64.
// Epilogue: instead of storing the slab's HH tile (and re-reading all of them in a k_hist_z pass), the wave contracts its
// 16 levels with Ep on the spot: zpart[slab][x tile][a, b] = sum_{x in tile} Ep[x][a, b] HH[a][b, x]; a fixed-order reduce
// over the slabs and the 16 level tiles (reduce_partials) then gives z.  26 MB of HH written and read per pass become
// < 1 MB of partials, and one launch goes away.
__global__ __launch_bounds__(256) void k_hist_hh(int nC, int nR, int nrows, int slab_rows, int lev_t0, int lev_nt,
                                                 const double* __restrict__ er, const double* __restrict__ h,
                                                 const double* __restrict__ Ep, int p, int ldp, double* __restrict__ zpart,
                                                 const int* __restrict__ run_if) {
    if (run_if != nullptr && *run_if == 0) return;
    // the slab's er rows, staged once for the four waves (they were re-read from global memory inside the MFMA loop: a
    // second dependent latency per 32 rows), and all of a lane's h loads of a 64-row half slab in flight together
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* sEr = reinterpret_cast<double*>(smem_raw);  // [slab_rows][nR]
    const int n = kLevels * nC;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kq = lane >> 4;
    const int r0 = blockIdx.y * slab_rows, rcount = min(nrows - r0, slab_rows);
    for (int i = tid; i < rcount * nR; i += 256) sEr[i] = er[(size_t)r0 * nR + i];
    const int q = blockIdx.x * 4 + wave;  // column tile, as in k_hist_g: only the level tiles that occur
    const bool col_ok = q < nC * lev_nt;
    const int b = col_ok ? q / lev_nt : 0, xt = lev_t0 + (col_ok ? q % lev_nt : 0), x = xt * 16 + l15;
    const int col = b * kLevels + x;
    const bool two = nR > 16;
    f64x4 acc0 = f64x4{0.0, 0.0, 0.0, 0.0}, acc1 = acc0;
    __syncthreads();
    if (!col_ok) return;  // wave-uniform (after the barrier)
    for (int k0 = 0; k0 < slab_rows; k0 += 64) {
        double bop[16];
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            const int rl = k0 + ks * 4 + kq;
            bop[ks] = (col_ok && rl < rcount) ? h[(size_t)(r0 + rl) * n + col] : 0.0;
        }
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            const int rl = k0 + ks * 4 + kq;
            const bool rok = rl < rcount;
            const double a0 = (rok && l15 < nR) ? sEr[rl * nR + l15] : 0.0;
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, bop[ks], acc0, 0, 0, 0);
            if (two) {
                const double a1 = (rok && 16 + l15 < nR) ? sEr[rl * nR + 16 + l15] : 0.0;
                acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, bop[ks], acc1, 0, 0, 0);
            }
        }
    }
    // table columns are b-major (col = b * 256 + x) and a wave's 16 columns share b: lane (l15, kq) holds, for its level
    // x = x0 + l15, the sums of sample rows a = kq + 4 e (and 16 + kq + 4 e)
    double v[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int a0 = kq + 4 * e, a1 = 16 + kq + 4 * e;
        v[e] = (col_ok && a0 < nR) ? acc0[e] * Ep[(size_t)x * p + a0 * nC + b] : 0.0;
        v[4 + e] = (two && col_ok && a1 < nR) ? acc1[e] * Ep[(size_t)x * p + a1 * nC + b] : 0.0;
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1)  // sum over the 16 levels of the tile (lanes l15 of one kq group), fixed tree
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += __shfl_xor(v[e], off);
    if (l15 == 0 && col_ok) {
        double* out = zpart + ((size_t)blockIdx.y * lev_nt + (xt - lev_t0)) * ldp;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int a0 = kq + 4 * e, a1 = 16 + kq + 4 * e;
            if (a0 < nR) out[a0 * nC + b] = v[e];
            if (two && a1 < nR) out[a1 * nC + b] = v[4 + e];
        }
    }
}

// z[s] = sum over the nparts (slab, level tile) partial rows, in a fixed order; columns s >= p come out as 0.
// 8 columns x 32 row groups per workgroup: ldp / 8 workgroups, each thread adds nparts / 32 values.
__global__ __launch_bounds__(256) void k_z_reduce(const double* __restrict__ zpart, int nparts, int p, int ldp,
                                                  double* __restrict__ z, const int* __restrict__ run_if) {
    if (run_if != nullptr && *run_if == 0) return;
    __shared__ double sm[32][8];
    const int c = threadIdx.x & 7, g = threadIdx.x >> 3, col = blockIdx.x * 8 + c;
    double s = 0.0;
    if (col < p)
        for (int r = g; r < nparts; r += 32) s += zpart[(size_t)r * ldp + col];
    sm[g][c] = s;
    __syncthreads();
    if (g == 0 && col < ldp) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 32; ++k) t += sm[k][c];
        z[col] = t;
    }
}

// image rows per slab of the HH stage: enough slabs to fill the chip's 1024 SIMDs about four times over with one wave
// per (16 table columns, slab), no more -- k_hist_z reads every slab's HH again (cfg4: 128 rows, 32 slabs, 5120 waves)
static int hist_slab_rows(GridSpec gs, int nrows_local) {
    const int ncoltiles = kLevels * gs.nSelCols / 16;
    const int want = std::max(1, (4096 + ncoltiles - 1) / ncoltiles);   // slabs wanted
    int rows = (nrows_local + want - 1) / want;
    rows = std::max(64, ((rows + 31) / 32) * 32);
    const int lds_rows = ((8192 / std::max(gs.nSelRows, 1)) / 32) * 32;  // k_hist_hh stages the slab's er rows: <= 64 KB
    return std::min(rows, std::max(64, lds_rows));
}
size_t hist_tiled_workspace_elems(GridSpec gs, int nrows_local) {
    const size_t n = (size_t)kLevels * gs.nSelCols;
    const int sr = hist_slab_rows(gs, nrows_local);
    const int nslabs = (nrows_local + sr - 1) / sr;
    const size_t ldp = ((size_t)gs.nSelRows * gs.nSelCols + 63) & ~(size_t)63;
    return 2 * (size_t)nrows_local * n + (size_t)nslabs * std::max(n * gs.nSelRows, (size_t)(kLevels / 16) * ldp);
}

// the HH stage and the column sums behind a pixel kernel's tables d_h: d_z = the p column sums (ldp doubles)
static hipError_t launch_hist_hh_z(hipStream_t s, const TableView& v, const double* d_h, double* d_HH, double* d_z,
                                   const int* d_run_if = nullptr) {
    const GridSpec gs = v.gs;
    const int nC = gs.nSelCols, nR = gs.nSelRows, p = v.p, ldp = v.ldp, nrows_local = v.nrows;
    const int slab_rows = hist_slab_rows(gs, nrows_local), nslabs = (nrows_local + slab_rows - 1) / slab_rows;
    const int lev_t0 = v.sorted ? v.sorted->lev_t0 : 0, lev_nt = v.sorted ? v.sorted->lev_nt : kLevels / 16;
    const size_t shm_hh = (size_t)slab_rows * nR * sizeof(double);  // slab_rows <= 1024 in practice; nR <= 32
    hipError_t e = launch(k_hist_hh, dim3((unsigned)((nC * lev_nt + 3) / 4), (unsigned)nslabs), dim3(256), shm_hh, s, nC, nR,
                          nrows_local, slab_rows, lev_t0, lev_nt, v.er, d_h, v.Ep, p, ldp, d_HH, d_run_if);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_z_reduce, dim3((unsigned)((ldp + 7) / 8)), dim3(256), 0, s, d_HH, nslabs * lev_nt, p, ldp, d_z, d_run_if);
    return hipGetLastError();
}

// one Sinkhorn half-iteration, tiled form; d_ws: hist_tiled_workspace_elems doubles; d_z: ldp doubles
hipError_t sink_hist_tiled(hipStream_t s, int mode, const TableView& v, const double* d_w, double eps, double* d_ybuf,
                           double* d_ws, double* d_z, LaunchObserver* obs, const float* d_xvec, const int* d_run_if) {
    if (!tables_apply(v.gs) || (d_run_if != nullptr && v.sorted == nullptr)) return hipErrorInvalidValue;
    const GridSpec gs = v.gs;
    const int nC = gs.nSelCols, p = v.p, row0 = v.row0, nrows_local = v.nrows;
    const SortedRows* sorted = v.sorted;
    const double* d_cvec = mode == ROWPASS_XVEC ? v.cvec : nullptr;  // the other modes do not read it
    struct Scope {
        LaunchObserver* o;
        Scope(LaunchObserver* ob, int sub) : o(ob) { if (o) o->begin(sub); }
        ~Scope() { if (o) o->end(); }
    };
    const size_t n = (size_t)kLevels * nC;
    double* d_g = d_ws;
    double* d_h = d_g + (size_t)nrows_local * n;
    double* d_HH = d_h + (size_t)nrows_local * n;
    // the 16-level tiles that occur in the image (known with the sorted rows): the tables' other columns are neither made
    // (k_hist_g), stored (pass kernel) nor contracted (k_hist_hh)
    const int lev_t0 = sorted ? sorted->lev_t0 : 0, lev_nt = sorted ? sorted->lev_nt : kLevels / 16;
    if (mode == ROWPASS_RECIP) {
        Scope sc(obs, SUB_HIST_G);
        hipError_t eg = launch_hist_g(s, gs, p, nrows_local, v.er, v.Ep, d_w, d_g, lev_t0, lev_nt);
        if (eg != hipSuccess) return eg;
    }
    if (sorted != nullptr) {
        Scope sc(obs, SUB_HIST_PIX);
        hipError_t ep = sorted_pass(s, mode, gs, row0, nrows_local, *sorted, d_g, eps, d_ybuf, d_h, d_cvec, d_xvec, d_run_if);
        if (ep != hipSuccess) return ep;
    } else {
        Scope sc(obs, SUB_HIST_PIX);
        hipError_t ep = hipErrorInvalidValue;
        dispatch_columns<1, 36>(nC, [&](auto nc) {
            constexpr int NC = decltype(nc)::value;  // from 12 columns the two tables are beyond 48 KB of LDS
            ep = launch(k_hist_pix<NC>, dim3((unsigned)nrows_local), dim3(kPixThreads), (size_t)2 * kLevels * (NC | 1) * sizeof(double),
                        s, mode, v.lum, gs, row0, v.ecT, d_g, eps, d_ybuf, d_h, d_cvec, d_xvec);
        });
        if (ep != hipSuccess) return ep;
    }
    Scope sc(obs, SUB_HIST_HH);
    return launch_hist_hh_z(s, v, d_h, d_HH, d_z, d_run_if);
}

size_t apply_reduce_planes_workspace_elems(GridSpec gs, int nrows_local, int np) {
    // np tables in place of the g and h tables of a single pass
    return hist_tiled_workspace_elems(gs, nrows_local) + (size_t)std::max(np - 2, 0) * nrows_local * kLevels * gs.nSelCols;
}

// reduce half of the sample-space apply for np planes on the level-sorted rows: ONE pixel kernel for the group
// (sorted_reduce_planes), then the HH stage and the column sums of sink_hist_tiled plane by plane, through the same HH buffer
hipError_t apply_reduce_planes(hipStream_t s, const TableView& v, const float* const* d_x, int np, double* d_ws, double* d_m,
                               LaunchObserver* obs) {
    if (!tables_apply(v.gs) || v.sorted == nullptr || np < 2 || np > sorted_planes_per_launch(v.gs)) return hipErrorInvalidValue;
    const size_t tab = (size_t)v.nrows * kLevels * v.gs.nSelCols;
    double* d_HH = d_ws + (size_t)np * tab;
    PlaneGroup pg{};
    for (int m = 0; m < np; ++m) pg.x[m] = d_x[m], pg.h[m] = d_ws + (size_t)m * tab;
    if (obs) obs->begin(SUB_HIST_PIX);
    hipError_t ep = sorted_reduce_planes(s, v.gs, v.row0, v.nrows, *v.sorted, v.cvec, pg, np);
    if (obs) obs->end();
    if (ep != hipSuccess) return ep;
    for (int m = 0; m < np; ++m) {
        if (obs) obs->begin(SUB_HIST_HH);
        hipError_t eh = launch_hist_hh_z(s, v, pg.h[m], d_HH, d_m + (size_t)m * v.ldp);
        if (obs) obs->end();
        if (eh != hipSuccess) return eh;
    }
    return hipSuccess;
}

// layers of the sample-space apply's expand half that one launch handles: on the level-sorted rows what sorted_expand takes,
// else what fits k_hist_dot's LDS (one table each)
int apply_layers_per_launch(const TableView& v) {
    if (v.sorted != nullptr) return sorted_expand_layers(v.gs);
    const size_t table = (size_t)kLevels * (v.gs.nSelCols | 1) * sizeof(double);
    return (int)std::max<size_t>(1, std::min<size_t>(kDotLayers, (size_t)(144 * 1024) / table));
}

// expand half of the sample-space apply for `nl` <= apply_layers_per_launch(v) layers: the g tables from the w' vectors
// (d_wl: nl vectors, stride ldw), then one pixel kernel (sorted_expand on the level-sorted rows, else k_hist_dot);
// d_ws: nl * v.nrows * 256 nC doubles; d_out: layer l at d_out + l * ostride
hipError_t apply_hist_layers(hipStream_t s, const TableView& v, const double* d_wl, int ldw, int nl, double* d_ws, float* d_out,
                             long long ostride, LaunchObserver* obs, bool round8) {
    if (v.nrows <= 0) return hipSuccess;
    if (!tables_apply(v.gs) || nl < 1 || nl > apply_layers_per_launch(v)) return hipErrorInvalidValue;
    const GridSpec gs = v.gs;
    const int nC = gs.nSelCols, p = v.p, row0 = v.row0, nrows_local = v.nrows;
    const SortedRows* sorted = v.sorted;
    const size_t n = (size_t)kLevels * nC, gstride = (size_t)nrows_local * n;
    if (obs) obs->begin(SUB_HIST_G);
    for (int l = 0; l < nl; ++l) {
        hipError_t eg = launch_hist_g(s, gs, p, nrows_local, v.er, v.Ep, d_wl + (size_t)l * ldw, d_ws + (size_t)l * gstride,
                                      sorted ? sorted->lev_t0 : 0, sorted ? sorted->lev_nt : kLevels / 16);
        if (eg != hipSuccess) return eg;
    }
    if (obs) obs->end(), obs->begin(SUB_HIST_PIX);
    if (sorted != nullptr) {
        hipError_t ex = sorted_expand(s, gs, nrows_local, *sorted, d_ws, gstride, nl, v.cvec, d_out, ostride, round8);
        if (obs) obs->end();
        return ex;
    }
    hipError_t ed = hipErrorInvalidValue;
    dispatch_columns<1, 36>(nC, [&](auto nc) {
        constexpr int NC = decltype(nc)::value;
        ed = launch(k_hist_dot<NC>, dim3((unsigned)nrows_local), dim3(kDotThreads), (size_t)nl * kLevels * (NC | 1) * sizeof(double), s,
                    v.lum, gs, row0, v.ecT, d_ws, gstride, nl, v.cvec, d_out, ostride, round8 ? 1 : 0);
    });
    if (obs) obs->end();
    return ed;
}

hipError_t apply_small(hipStream_t s, int p, int K, int ldk, int L, int ldw, const double* d_m, const double* d_D,
                       const double* d_Vrows, const double* d_xA, const double* d_resp, double* d_t, double* d_Wp,
                       double* d_YA, const int* d_differs, const double* d_m_same, const double* d_xA_same) {
    const size_t shm = (size_t)(2 * p + K + 256) * sizeof(double);
    hipLaunchKernelGGL(k_apply_small, dim3((unsigned)L), dim3(256), shm, s, p, K, ldk, L, ldw, d_m, d_D, d_Vrows, d_xA,
                       d_resp, d_t, d_Wp, d_YA, d_differs, d_m_same, d_xA_same);
    return hipGetLastError();
}

hipError_t scatter_samples(hipStream_t s, int p, int L, const long long* d_loc, const double* d_YA, float* d_Y,
                           long long ystride, bool round8) {
    hipLaunchKernelGGL(k_scatter_samples, dim3((unsigned)((L * p + 255) / 256)), dim3(256), 0, s, p, L, d_loc, d_YA, d_Y,
                       ystride, round8 ? 1 : 0);
    return hipGetLastError();
}

// -------------------------------------------------------------------- Gram via the same tables
// Gk[(a,b),(a',b')] = sum_r er[r][a] er[r][a'] sum_x Ep[x][a,b] Ep[x][a',b'] A_r[x][b,b'],
// A_r[x][b,b'] = sum over the non-sample pixels of image row r with level x of c^2 ec[c][b] ec[c][b'].
//   1. k_ghist_rows : A_r (256 x NP histogram in LDS, NP = nC(nC+1)/2 products per pixel) -> global
//   2. k_ghist_gemm : C[(a,a')][(b,b'),x] = sum_r EE[r][(a,a')] A_r[(b,b'),x]   (fp64 MFMA GEMM,
//                     M = nR(nR+1)/2, N = 256 NP, K = local image rows)
//   3. k_ghist_final: Gk[s][s'] = sum_x Ep[x][s] Ep[x][s'] C[(a,a')][x,(b,b')]
// ~NP LDS adds per pixel plus a 46 GFLOP GEMM at cfg4, instead of p^2/2 = 20 kFLOP per pixel.
__device__ __forceinline__ int tri_index(int i, int j, int n) {  // i <= j < n, row-major upper triangle
    return i * n - (i * (i - 1)) / 2 + (j - i);
}

// (the histogram takes most of a CU's LDS, so one workgroup per CU: 512 threads keep 8 waves on it)
constexpr int kGhistRowsThreads = 512;
__global__ __launch_bounds__(kGhistRowsThreads) void k_ghist_rows(const float* __restrict__ lum, GridSpec gs, int row0,
                                                    const double* __restrict__ ecT,
                                                    const double* __restrict__ cvec, double* __restrict__ Aout) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* A = reinterpret_cast<double*>(smem_raw);  // [256][NP]
    const int nC = gs.nSelCols, W = gs.W, NP = nC * (nC + 1) / 2;
    const int tid = threadIdx.x, lrow = blockIdx.x, r = row0 + lrow;
    for (int i = tid; i < kLevels * NP; i += kGhistRowsThreads) A[i] = 0.0;
    __syncthreads();
    const int dr = r - gs.rowOff;
    const bool sample_row = dr >= 0 && (dr % gs.rowStep) == 0 && (dr / gs.rowStep) < gs.nSelRows;
    for (int c0 = 0; c0 < W; c0 += kGhistRowsThreads) {  // wave-uniform trip count: the body uses cross-lane sums
        const bool inside = c0 + tid < W;
        const int c = inside ? c0 + tid : W - 1;
        const int dc = c - gs.colOff;
        const bool smp = sample_row && dc >= 0 && (dc % gs.colStep) == 0 && (dc / gs.colStep) < nC;
        const double cf = (inside && !smp) ? cvec[(size_t)lrow * W + c] : 0.0;  // c at a sample pixel is not read (kernels.h)
        const int x = (int)lum[(size_t)r * W + c];
        double q[11];
#pragma unroll
        for (int b = 0; b < 11; ++b) q[b] = (b < nC) ? cf * ecT[(size_t)b * W + c] : 0.0;
        const bool own = wave_group_levels(cf != 0.0, x, [&](int lx, bool mine) {
            double* Al = A + (size_t)lx * NP;
            int idx = 0;
#pragma unroll
            for (int b = 0; b < 11; ++b)
#pragma unroll
                for (int b2 = b; b2 < 11; ++b2)
                    if (b2 < nC) {
                        const double t = wave_sum63(mine ? q[b] * q[b2] : 0.0);
                        if ((tid & 63) == 63) atomicAdd(&Al[idx], t);
                        ++idx;
                    }
        });
        if (own) {
            double* Ax = A + (size_t)x * NP;
            int idx = 0;
#pragma unroll
            for (int b = 0; b < 11; ++b)
#pragma unroll
                for (int b2 = b; b2 < 11; ++b2)
                    if (b2 < nC) atomicAdd(&Ax[idx++], q[b] * q[b2]);
        }
    }
    __syncthreads();
    double* out = Aout + (size_t)lrow * kLevels * NP;  // global layout [pair][level]: k_ghist_final streams levels
    for (int i = tid; i < kLevels * NP; i += kGhistRowsThreads) out[i] = A[(i & (kLevels - 1)) * NP + i / kLevels];
}

// General form for 12 <= nC <= 36: the pair list does not fit in LDS at once, so a launch handles the
// pairs (b, b..nC-1) of sample columns b in [b0, b1) (<= kGhistChunkPairs pairs, chosen by the host) and
// writes that slice of A.
constexpr int kGhistMaxCols = 36;
constexpr int kGhistChunkPairs = 72;  // 256 * 72 * 8 B = 147 KB of LDS

__global__ __launch_bounds__(kGhistRowsThreads) void k_ghist_rows_chunk(const float* __restrict__ lum, GridSpec gs, int row0, int b0,
                                                          int b1, int pair_off, int npairs,
                                                          const double* __restrict__ ecT,
                                                          const double* __restrict__ cvec,
                                                          double* __restrict__ Aout) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    double* A = reinterpret_cast<double*>(smem_raw);  // [256][npairs]
    const int nC = gs.nSelCols, W = gs.W, NP = nC * (nC + 1) / 2;
    const int tid = threadIdx.x, lrow = blockIdx.x, r = row0 + lrow;
    for (int i = tid; i < kLevels * npairs; i += kGhistRowsThreads) A[i] = 0.0;
    __syncthreads();
    const int dr = r - gs.rowOff;
    const bool sample_row = dr >= 0 && (dr % gs.rowStep) == 0 && (dr / gs.rowStep) < gs.nSelRows;
    for (int c0 = 0; c0 < W; c0 += kGhistRowsThreads) {  // wave-uniform trip count: the body uses cross-lane sums
        const bool inside = c0 + tid < W;
        const int c = inside ? c0 + tid : W - 1;
        const int dc = c - gs.colOff;
        const bool smp = sample_row && dc >= 0 && (dc % gs.colStep) == 0 && (dc / gs.colStep) < nC;
        const double cf = (inside && !smp) ? cvec[(size_t)lrow * W + c] : 0.0;  // c at a sample pixel is not read (kernels.h)
        const int x = (int)lum[(size_t)r * W + c];
        double q[kGhistMaxCols];
#pragma unroll
        for (int b = 0; b < kGhistMaxCols; ++b) q[b] = (b < nC) ? cf * ecT[(size_t)b * W + c] : 0.0;
        // (no wave-level pre-reduction here: with 36 x 36 unrolled products it would double an already large
        // kernel and spill; flat regions cost this kernel their same-address serialisation)
        const bool own = cf != 0.0;
        if (own) {
            double* Ax = A + (size_t)x * npairs;
            int idx = 0;
#pragma unroll
            for (int b = 0; b < kGhistMaxCols; ++b) {
                if (b >= b0 && b < b1) {  // wave-uniform
#pragma unroll
                    for (int b2 = b; b2 < kGhistMaxCols; ++b2)
                        if (b2 < nC) atomicAdd(&Ax[idx++], q[b] * q[b2]);
                }
            }
        }
    }
    __syncthreads();
    double* out = Aout + (size_t)lrow * kLevels * NP + (size_t)pair_off * kLevels;  // [pair][level]
    for (int i = tid; i < kLevels * npairs; i += kGhistRowsThreads) {
        const int j = i / kLevels, x = i & (kLevels - 1);
        out[i] = A[x * npairs + j];
    }
}

// EE[r][m] = er[r][a] er[r][a'] for the m-th pair a <= a' (row stride ldm, zero padded)
__global__ void k_ghist_ee(const double* __restrict__ er, int nrows, int nR, int ldm, double* __restrict__ EE) {
    const long long n = (long long)nrows * ldm;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(i / ldm), m = (int)(i % ldm);
        double v = 0.0;
        if (m < nR * (nR + 1) / 2) {
            int a = 0, t = m;
            while (t >= nR - a) {
                t -= nR - a;
                ++a;
            }
            v = er[(size_t)r * nR + a] * er[(size_t)r * nR + a + t];
        }
        EE[i] = v;
    }
}

// C[z] (ldm x N) = EE^T (rows [z ksplit, (z+1) ksplit) of K x ldm) * A (same rows of K x N); one 16-column
// tile per wave, MT m-tiles per wave.  The image rows are split over gridDim.z so that the launch fills the
// chip (N/64 blocks alone are fewer than the CUs); k_ghist_final adds the gridDim.z partial products in order.
template <int MT>
__global__ __launch_bounds__(256) void k_ghist_gemm(const double* __restrict__ EE, int ldm, const double* __restrict__ A,
                                                    long long N, int Ktot, int ksplit, double* __restrict__ Cz) {
    constexpr int KB = 16;
    constexpr int EPT = (KB * MT * 16 + 255) / 256;  // EE values staged per thread and k block
    __shared__ __attribute__((aligned(16))) double sE[KB][MT * 16 + 16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kq = lane >> 4;
    const long long n0 = ((long long)blockIdx.x * 4 + wave) * 16;
    const int m0 = blockIdx.y * MT * 16;
    const bool ncol_ok = n0 + l15 < N;
    const int kbeg = blockIdx.z * ksplit, K = min(Ktot, kbeg + ksplit);
    double* C = Cz + (size_t)blockIdx.z * ldm * N;
    f64x4 acc[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
    // software pipeline over the 16-row k blocks: the next block's EE slice and A operands are fetched into
    // registers while the MFMAs of the current one run; LDS is rewritten between two barriers
    double e_next[EPT], b_next[KB / 4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < EPT; ++q) {
            const int idx = tid + q * 256, kk = idx / (MT * 16), mm = idx % (MT * 16);
            e_next[q] = (idx < KB * MT * 16 && k0 + kk < K && m0 + mm < ldm) ? EE[(size_t)(k0 + kk) * ldm + m0 + mm] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < KB / 4; ++q) {
            const int kr = k0 + 4 * q + kq;
            b_next[q] = (ncol_ok && kr < K) ? A[(size_t)kr * N + n0 + l15] : 0.0;
        }
    };
    if (kbeg < K) fetch(kbeg);
    for (int k0 = kbeg; k0 < K; k0 += KB) {
        __syncthreads();  // everybody is done reading the previous block's sE
#pragma unroll
        for (int q = 0; q < EPT; ++q) {
            const int idx = tid + q * 256;
            if (idx < KB * MT * 16) sE[idx / (MT * 16)][idx % (MT * 16)] = e_next[q];
        }
        double bcur[KB / 4];
#pragma unroll
        for (int q = 0; q < KB / 4; ++q) bcur[q] = b_next[q];
        __syncthreads();
        if (k0 + KB < K) fetch(k0 + KB);
#pragma unroll
        for (int q = 0; q < KB / 4; ++q) {
#pragma unroll
            for (int j = 0; j < MT; ++j)
                acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(sE[4 * q + kq][j * 16 + l15], bcur[q], acc[j], 0, 0, 0);
        }
    }
    if (ncol_ok) {
#pragma unroll
        for (int j = 0; j < MT; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int m = m0 + j * 16 + kq + 4 * e;
                if (m < ldm) C[(size_t)m * N + n0 + l15] = acc[j][e];
            }
    }
}

// One wave per (row pair m = (a1 <= a2), column pair pc = (b1 <= b2)): its 256-level vector of C (summed over the
// GEMM's row splits in a fixed order) is read once, coalesced, and contracted with Ep for the one or two entries of
// Gk it feeds -- (a1,b1)x(a2,b2) and, when both pairs are off-diagonal, (a1,b2)x(a2,b1) -- plus their transposes.
__global__ __launch_bounds__(256) void k_ghist_final(const double* __restrict__ C, long long N, int nsplit, size_t zstride,
                                                     const double* __restrict__ Ep, int p, int nR, int nC,
                                                     double* __restrict__ Gk) {
    const int NP = nC * (nC + 1) / 2, NM = nR * (nR + 1) / 2;
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (long long)NM * NP) return;  // wave-uniform
    const int m = (int)(w / NP), pc = (int)(w % NP);
    int a1 = 0, t = m;
    while (t >= nR - a1) {
        t -= nR - a1;
        ++a1;
    }
    const int a2 = a1 + t;
    int b1 = 0;
    t = pc;
    while (t >= nC - b1) {
        t -= nC - b1;
        ++b1;
    }
    const int b2 = b1 + t;
    const int s11 = a1 * nC + b1, s22 = a2 * nC + b2, s12 = a1 * nC + b2, s21 = a2 * nC + b1;
    const bool two = (a1 != a2) && (b1 != b2);
    const double* Cm = C + (size_t)m * N + (size_t)pc * kLevels;  // columns are [pair][level]
    double u = 0.0, v = 0.0;
#pragma unroll
    for (int j = 0; j < kLevels / 64; ++j) {
        const int x = j * 64 + lane;
        double cx = 0.0;
        for (int z = 0; z < nsplit; ++z) cx += Cm[z * zstride + x];  // fixed order
        const double* e = Ep + (size_t)x * p;
        u += e[s11] * e[s22] * cx;
        if (two) v += e[s12] * e[s21] * cx;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        u += __shfl_xor(u, off);
        v += __shfl_xor(v, off);
    }
    if (lane == 0) {
        Gk[(size_t)s11 * p + s22] = u;
        Gk[(size_t)s22 * p + s11] = u;
        if (two) {
            Gk[(size_t)s12 * p + s21] = v;
            Gk[(size_t)s21 * p + s12] = v;
        }
    }
}

// ---- Gram by index sums (sorted.hip: k_sorted_gsum has the derivation).  Rows: er[r][a] er[r][a'] =
// exp(-(a - a')^2 rs^2 / (2 hx^2)) F_{a+a'}(r), F_s(r) = exp(-2 (r - rowOff - s rs / 2)^2 / hx^2): the GEMM over image rows needs
// 2 nR - 1 rows instead of nR (nR + 1) / 2.
//   k_gsum_rowf : F[r][s] (row stride ldm, zero padded)
//   k_ghist_gemm: T[s][t, x] = sum_r F[r][s] S_r[t, x]
//   k_gsum_final: Gk[(a,b)][(a',b')] = kr_{|a-a'|} kc_{|b-b'|} sum_x Ep[x][a,b] Ep[x][a',b'] T[a+a'][b+b', x]
__global__ void k_gsum_rowf(GridSpec gs, int row0, int nrows, int ldm, double inv_hx2, double* __restrict__ F) {
    const long long n = (long long)nrows * ldm;
    const int ns = 2 * gs.nSelRows - 1;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(i / ldm), sidx = (int)(i % ldm);
        double v = 0.0;
        if (sidx < ns) {
            const double d = (double)(row0 + r - gs.rowOff) - 0.5 * (double)sidx * (double)gs.rowStep;
            v = exp(-2.0 * d * d * inv_hx2);
        }
        F[i] = v;
    }
}

// one wave per pair of samples i <= j (grid: x = groups of 4 j's, y = i)
__global__ __launch_bounds__(256) void k_gsum_final(const double* __restrict__ T, long long N, int nsplit, size_t zstride,
                                                    const double* __restrict__ Ep, int p, int nC, double kr2, double kc2,
                                                    double* __restrict__ Gk) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.y, j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j < i || j >= p) return;  // wave-uniform
    const int a1 = i / nC, b1 = i - a1 * nC, a2 = j / nC, b2 = j - a2 * nC;
    const int da = a1 - a2, db = b1 - b2;
    const double kappa = exp(-(double)(da * da) * kr2 - (double)(db * db) * kc2);
    const double* Tm = T + (size_t)(a1 + a2) * N + (size_t)(b1 + b2) * kLevels;
    double u = 0.0;
#pragma unroll
    for (int q = 0; q < kLevels / 64; ++q) {
        const int x = q * 64 + lane;
        double tx = 0.0;
        for (int z = 0; z < nsplit; ++z) tx += Tm[z * zstride + x];  // fixed order
        const double* e = Ep + (size_t)x * p;
        u += e[i] * e[j] * tx;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) u += __shfl_xor(u, off);
    if (lane == 0) {
        u *= kappa;
        Gk[(size_t)i * p + j] = u;
        Gk[(size_t)j * p + i] = u;
    }
}

int ghist_ldm(int nR) { return ((nR * (nR + 1) / 2) + 15) & ~15; }
constexpr int kGhistMT = 14;
// image rows per GEMM split (a multiple of the 16-row k step) and the number of splits: ~4 workgroups per CU
static void ghist_split(long long N, int ldm, int nrows_local, int* ksplit, int* nsplit) {
    const long long base = ((N / 16 + 3) / 4) * ((ldm / 16 + kGhistMT - 1) / kGhistMT);
    int ns = (int)std::min<long long>(16, std::max<long long>(1, (1024 + base - 1) / base));
    int ks = (((nrows_local + ns - 1) / ns) + 15) & ~15;
    ks = std::max(ks, 16);
    *ksplit = ks;
    *nsplit = std::max(1, (nrows_local + ks - 1) / ks);
}
static int gsum_ldm(int nR) { return ((2 * nR - 1) + 15) & ~15; }
size_t ghist_workspace_elems(GridSpec gs, int nrows_local) {
    const size_t NP = (size_t)gs.nSelCols * (gs.nSelCols + 1) / 2, N = 256 * NP;
    const size_t ldm = (size_t)ghist_ldm(gs.nSelRows);
    int ks, ns;
    ghist_split((long long)N, (int)ldm, nrows_local, &ks, &ns);
    const size_t pairs = (size_t)nrows_local * N + (size_t)nrows_local * ldm + (size_t)ns * ldm * N;
    // the index-sum form (2 nC - 1 tables, 2 nR - 1 GEMM rows) needs less of each, but may split the rows further
    const size_t N2 = (size_t)256 * (2 * gs.nSelCols - 1), ldm2 = (size_t)gsum_ldm(gs.nSelRows);
    ghist_split((long long)N2, (int)ldm2, nrows_local, &ks, &ns);
    const size_t sums = (size_t)nrows_local * N2 + (size_t)nrows_local * ldm2 + (size_t)ns * ldm2 * N2;
    return std::max(pairs, sums);
}

// the split of the image rows gram_hist's GEMM takes for this view, in the form it takes (pairs or index sums)
void gram_hist_split(const TableView& v, int* ksplit, int* nsplit) {
    const int nC = v.gs.nSelCols, nR = v.gs.nSelRows;
    if (v.sorted != nullptr && v.sorted->E2 != nullptr) ghist_split((long long)kLevels * (2 * nC - 1), gsum_ldm(nR), v.nrows, ksplit, nsplit);
    else ghist_split((long long)kLevels * (nC * (nC + 1) / 2), ghist_ldm(nR), v.nrows, ksplit, nsplit);
}

// d_ws: ghist_workspace_elems doubles; d_Gk: p x p doubles (full symmetric matrix of this rank's rows)
hipError_t gram_hist(hipStream_t s, const TableView& v, double* d_ws, double* d_Gk, LaunchObserver* obs) {
    if (!tables_apply(v.gs)) return hipErrorInvalidValue;
    const GridSpec gs = v.gs;
    const int nC = gs.nSelCols, nR = gs.nSelRows, p = v.p, row0 = v.row0, nrows_local = v.nrows;
    const SortedRows* sorted = v.sorted;
    if (sorted != nullptr && sorted->E2 != nullptr) {  // index sums: 2 nC - 1 tables, 2 nR - 1 GEMM rows (sorted_gsum_ok)
        const long long N2 = (long long)kLevels * (2 * nC - 1);
        const int ldm2 = gsum_ldm(nR);
        double* d_S = d_ws;
        double* d_F = d_S + (size_t)nrows_local * N2;
        double* d_T = d_F + (size_t)nrows_local * ldm2;
        const double hx = sorted->hx;
        if (obs) obs->begin(SUB_GHIST_ROWS);
        hipError_t e2 = sorted_gram_sums(s, gs, nrows_local, *sorted, v.cvec, d_S);
        if (e2 != hipSuccess) return e2;
        if (obs) obs->end(), obs->begin(SUB_GHIST_EE);
        hipLaunchKernelGGL(k_gsum_rowf, dim3(256), dim3(256), 0, s, gs, row0, nrows_local, ldm2, 1.0 / (hx * hx), d_F);
        constexpr int MT2 = 4;  // 2 nR - 1 <= 63: one group of four 16-row tiles
        int ksplit2, nsplit2;
        ghist_split(N2, ldm2, nrows_local, &ksplit2, &nsplit2);
        const dim3 grid2((unsigned)((N2 / 16 + 3) / 4), (unsigned)((ldm2 / 16 + MT2 - 1) / MT2), (unsigned)nsplit2);
        if (obs) obs->end(), obs->begin(SUB_GHIST_GEMM);
        hipLaunchKernelGGL((k_ghist_gemm<MT2>), grid2, dim3(256), 0, s, d_F, ldm2, d_S, N2, nrows_local, ksplit2, d_T);
        if (obs) obs->end(), obs->begin(SUB_GHIST_FINAL);
        const double rs = gs.rowStep, cs2 = gs.colStep;
        hipLaunchKernelGGL(k_gsum_final, dim3((unsigned)((p + 3) / 4), (unsigned)p), dim3(256), 0, s, d_T, N2, nsplit2,
                           (size_t)ldm2 * N2, v.Ep, p, nC, rs * rs / (2.0 * hx * hx), cs2 * cs2 / (2.0 * hx * hx), d_Gk);
        if (obs) obs->end();
        return hipGetLastError();
    }
    const int NP = nC * (nC + 1) / 2;
    const long long N = (long long)kLevels * NP;
    const int ldm = ghist_ldm(nR);
    double* d_A = d_ws;
    double* d_EE = d_A + (size_t)nrows_local * N;
    double* d_C = d_EE + (size_t)nrows_local * ldm;
    hipError_t e;
    if (obs) obs->begin(SUB_GHIST_ROWS);
    if (sorted != nullptr) {
        e = sorted_gram_rows(s, gs, nrows_local, *sorted, v.cvec, d_A);
        if (e != hipSuccess) return e;
    } else if (nC <= 11) {
        e = launch(k_ghist_rows, dim3((unsigned)nrows_local), dim3(kGhistRowsThreads), (size_t)kLevels * NP * sizeof(double), s, v.lum,
                   gs, row0, v.ecT, v.cvec, d_A);
        if (e != hipSuccess) return e;
    } else {
        // not through launch(): the chunks differ in size, so the limit is raised once, to the largest, ahead of the loop
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_ghist_rows_chunk),
                                hipFuncAttributeMaxDynamicSharedMemorySize, kLevels * kGhistChunkPairs * (int)sizeof(double));
        if (e != hipSuccess) return e;
        int b0 = 0, off = 0;
        while (b0 < nC) {  // greedy: as many whole rows of the pair triangle as fit
            int b1 = b0, np = 0;
            while (b1 < nC && np + (nC - b1) <= kGhistChunkPairs) {
                np += nC - b1;
                ++b1;
            }
            if (b1 == b0) return hipErrorInvalidValue;  // cannot happen for nC <= 36 < 72
            hipLaunchKernelGGL(k_ghist_rows_chunk, dim3((unsigned)nrows_local), dim3(kGhistRowsThreads),
                               (size_t)kLevels * np * sizeof(double), s, v.lum, gs, row0, b0, b1, off, np, v.ecT, v.cvec, d_A);
            off += np;
            b0 = b1;
        }
    }
    if (obs) obs->end(), obs->begin(SUB_GHIST_EE);
    hipLaunchKernelGGL(k_ghist_ee, dim3(512), dim3(256), 0, s, v.er, nrows_local, nR, ldm, d_EE);
    constexpr int MT = kGhistMT;
    int ksplit, nsplit;
    ghist_split(N, ldm, nrows_local, &ksplit, &nsplit);
    const dim3 grid((unsigned)((N / 16 + 3) / 4), (unsigned)((ldm / 16 + MT - 1) / MT), (unsigned)nsplit);
    if (obs) obs->end(), obs->begin(SUB_GHIST_GEMM);
    hipLaunchKernelGGL((k_ghist_gemm<MT>), grid, dim3(256), 0, s, d_EE, ldm, d_A, N, nrows_local, ksplit, d_C);
    if (obs) obs->end(), obs->begin(SUB_GHIST_FINAL);
    const long long nwaves = (long long)(nR * (nR + 1) / 2) * NP;
    hipLaunchKernelGGL(k_ghist_final, dim3((unsigned)((nwaves + 3) / 4)), dim3(256), 0, s, d_C, N, nsplit,
                       (size_t)ldm * N, v.Ep, p, nR, nC, d_Gk);
    if (obs) obs->end();
    return hipGetLastError();
}

}  // namespace nlek
