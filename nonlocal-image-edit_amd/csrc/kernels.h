// Launch wrappers of the gfx950 kernels (kernels.hip and, by section, the other device files).  Internal to libnle_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace nlek {

// Closed form of samplePixels (reference src/filter.cpp:56-80).
struct GridSpec {
    int H, W;
    int rowStep, rowOff, nSelRows;
    int colStep, colOff, nSelCols;
    __host__ __device__ int p() const { return nSelRows * nSelCols; }
};

// {row, col, luminance, 0} of one sample, fp32 (coordinates are exact in fp32)
typedef float4 Sample4;  // x = row, y = col, z = luminance, w = 0

#if defined(__HIPCC__)
// K(i, s) = exp(negativeWeightedDistance) (reference src/filter.cpp:104-112,144-145) in base 2:
// nsw = -log2(e)/hx^2, npw = -log2(e)/hy^2, one v_exp_f32.  The spatial term is exact in fp32
// (integer coordinates, H*W < 2^24 keeps dr^2+dc^2 < 2^25; it is rounded once above that).
__device__ __forceinline__ float affinity_value(float pr, float pc, float px, Sample4 s, float nsw, float npw) {
    const float dr = pr - s.x, dc = pc - s.y, dv = px - s.z;
    return __builtin_amdgcn_exp2f(nsw * (dr * dr + dc * dc) + npw * (dv * dv));
}
__device__ __forceinline__ double recip_or_zero_d(double s, double eps) {
    return (fabs(s) >= eps) ? 1.0 / s : 0.0;  // inplaceReciprocal, src/filter.cpp:42-54
}
// closed form of the selection predicate of samplePixels (src/filter.cpp:68-70)
__device__ __forceinline__ bool is_sample_pixel(const GridSpec& gs, int row, int col) {
    const int dr = row - gs.rowOff, dc = col - gs.colOff;
    if (dr < 0 || dc < 0) return false;
    const int qr = dr / gs.rowStep, qc = dc / gs.colStep;
    return (qr * gs.rowStep == dr) && (qc * gs.colStep == dc) && qr < gs.nSelRows && qc < gs.nSelCols;
}
// the sample predicate of pixel gi = (row, col): bit gi of a listed set's mask (NLE_SAMPLER_FARTHEST), or the grid's
// closed form when there is no mask
__device__ __forceinline__ bool is_sample(const GridSpec& gs, const unsigned* smask, long long gi, int row, int col) {
    return smask ? ((smask[gi >> 5] >> (unsigned)(gi & 31)) & 1u) != 0 : is_sample_pixel(gs, row, col);
}
#endif

// composite launchers report each kernel they enqueue so that the caller can time them separately
struct LaunchObserver {
    virtual void begin(int sub) = 0;  // sub: index of the kernel inside the composite
    virtual void end() = 0;
    virtual ~LaunchObserver() = default;
};
enum { SUB_HIST_G = 0, SUB_HIST_PIX = 1, SUB_HIST_HH = 2, SUB_HIST_Z = 3 };
enum { SUB_GHIST_ROWS = 0, SUB_GHIST_EE = 1, SUB_GHIST_GEMM = 2, SUB_GHIST_FINAL = 3 };

constexpr int kRowpassMaxBlocks = 1024;
// LDS one launch of the apply-expand kernels may take for its [layers][K] fp64 table: more layers go out in several launches
constexpr size_t kApplyLdsBytes = 64 * 1024;
constexpr int kGramTilesPerWave = 7;
constexpr int kGramRowsPerStage = 32;

enum RowpassMode { ROWPASS_COLSUM = 0, ROWPASS_RECIP = 1, ROWPASS_XVEC = 2 };

// out[k] = lum[sel_index(k)] for the p samples
hipError_t gather_samples(hipStream_t s, const float* d_lum, GridSpec gs, float* d_out);
// fp64, 0 for samples outside rows [row0, row1) (d_lum: virtual base of the full image, only those rows exist)
hipError_t gather_samples_slab(hipStream_t s, const float* d_lum, GridSpec gs, int row0, int row1, double* d_out,
                               const int* d_run_if = nullptr);  // d_run_if: as sink_hist_tiled's

// K_AB rows, natural order: kab[i][s] = exp2(nsw*d2 + npw*dv^2), i in [pix0, pix0+M)
hipError_t affinity(hipStream_t s, const float* d_lum, GridSpec gs, const Sample4* d_samples,
                    int p, int ld, float nsw, float npw, long long pix0, long long M,
                    float* d_kab);

// C (M x ldc) = rowscale o (A x B).  B: kd x ldb fp32 row-major (zero padded to ldc cols).
// fused != 0: A rows are affinities computed on the fly from (lum, samples); else A is
// read from d_A (M x lda).  d_u != null (non-fused): rowscale_i = recip(A_i . u);
// d_c != null (fused): rowscale_i = c_i.
hipError_t ts_gemm(hipStream_t s, bool fused, const float* d_A, int lda, const float* d_lum,
                   GridSpec gs, const Sample4* d_samples, float nsw, float npw, long long pix0,
                   const float* d_B, int ldb, int kd, float* d_C, int ldc, long long M,
                   const double* d_u, double eps, const float* d_c = nullptr);

// The fused form on the bf16 matrix cores with split operands (tsgemm_bf16x3.hip: hi + mid + lo, six products, fp32
// accumulate): d_Bs = ts_gemm_bf16x3_split of the kd x ldb fp32 matrix B (ts_gemm_bf16x3_bsplit_elems shorts)
size_t ts_gemm_bf16x3_bsplit_elems(int kd, int ldb);
hipError_t ts_gemm_bf16x3_split(hipStream_t s, const float* d_B, int kd, int ldb, unsigned short* d_Bs);
hipError_t ts_gemm_bf16x3(hipStream_t s, const float* d_lum, GridSpec gs, const Sample4* d_samples, float nsw, float npw,
                          long long pix0, const unsigned short* d_Bs, int ldb, int kd, float* d_C, int ldc, long long M,
                          const float* d_c = nullptr);

// One pass over X (M x ld): partial[b][j] = sum_{rows of block b} X[i][j] * y_i,
//   mode COLSUM: y=1; RECIP: y_i = recip(X_i . (lam o t_in)); XVEC: y_i = xvec[i].
// Returns the number of blocks used in *nblocks.
hipError_t rowpass(hipStream_t s, int mode, const float* d_X, long long M, int ld,
                   const double* d_t_in, const double* d_lam, const float* d_xvec, double eps,
                   double* d_partial, int* nblocks);
// t_out[sl][j] = sum over the sl-th slice of blocks of partial[b][j], j < ld (nslices rows out;
// nslices == 1: the full column sums)
hipError_t reduce_partials(hipStream_t s, const double* d_partial, int nblocks, int ld,
                           double* d_t_out, int nslices = 1);
// u[j] = lam[j] * t[j]
hipError_t scale_vec(hipStream_t s, const double* d_lam, const double* d_t, int n, double* d_u);
// out[i] = recip(X_i . u)
hipError_t row_scalings(hipStream_t s, const float* d_X, long long M, int ld, const double* d_u,
                        double eps, double* d_out);

// Gram: tiles of G = sum_i c_i^2 x_i x_i^T, c_i = recip(x_i . u); upper-triangular 32x32
// tiles, chunked fp32 MFMA accumulation, fp64 across chunks.
// workspace: d_partial [nchunks][ntiles][1024] doubles; result d_tiles [ntiles][1024].
int gram_num_tiles(int ld);
int gram_chunk_rows(long long M);
size_t gram_partial_elems(long long M, int ld);
hipError_t gram(hipStream_t s, const float* d_X, long long M, int ld, const double* d_u,
                double eps, double* d_partial, double* d_tiles);
hipError_t gram_reduce(hipStream_t s, const double* d_partial, int nchunks, int ntiles, double* d_tiles);

// ---- Phi-free ("sample space") passes, fused.hip ----
// Sinkhorn half-iteration without Phi: z[s] = sum_i k_i[s] y_i over non-sample local pixels,
// y_i = 1 (COLSUM) or recip(k_i . w); partial: [sink_pass_rows(M)][sink_pass_ld(p)] doubles.
// d_ybuf (optional): y_i per local pixel, fp64 (0 at sample pixels).  p <= sink_pass_max_p().
int sink_pass_ld(int p);
int sink_pass_rows(long long M);
int sink_pass_max_p();
hipError_t sink_pass(hipStream_t s, int mode, const float* d_lum, GridSpec gs, const Sample4* d_samples,
                     int p, const double* d_w, float nsw, float npw, long long pix0, long long M, double eps,
                     double* d_ybuf, double* d_partial);
// p-sized update between passes in factored form: u' = lambda o (X1^T [z; y_A]), [w'; s_A'] = X2 u' (see fused.hip)
// d_z: zrows x zld partial column sums, added in row order; d_X1: 2p x r column-major, d_X2: 2p x r row-major;
// d_v (2p) and d_u (r): scratch
hipError_t sink_update(hipStream_t s, int mode, int p, int r, bool chol, const double* d_X1, const double* d_X2,
                       const double* d_lam, const double* d_z, int zrows, int zld, const double* d_sA_cur, double eps,
                       double* d_v, double* d_u, double* d_sA_next, double* d_w_next);
// Gk = sum over non-sample local pixels of c_i^2 k_i k_i^T on the fp64 MFMA; upper-triangular
// 16x16 tiles (row-major 256 doubles each), p <= 256.
constexpr int kG64TilesPerWave = 23;
int gram64_ld(int p);
int gram64_num_tiles(int p);
size_t gram64_partial_elems(long long M, int p);
hipError_t gram64(hipStream_t s, const float* d_lum, GridSpec gs, const Sample4* d_samples, int p, float nsw,
                  float npw, long long pix0, long long M, const double* d_c, double* d_partial, double* d_tiles);
// V (M x ldv fp32) = diag(c) K D on the fp64 MFMA; D: p x project64_ld(K) fp64 row-major, K <= 128
// The rule for V's padding, stated here for every route that builds V (project64's 28 forms, ts_gemm, ts_gemm64 behind a
// memset, scatter_sample_rows): columns [K, ldv) are ZERO, K <= ldv <= project64_ld(K).  apply_dense, rowpass_any and
// k_apply_expand read whole rows of ldv against a zero-padded g: a NaN bit pattern left there would reach the output.
int project64_ld(int K);
hipError_t project64(hipStream_t s, const float* d_lum, GridSpec gs, const Sample4* d_samples, int p, float nsw,
                     float npw, long long pix0, long long M, const double* d_D, int K, const double* d_c, float* d_V,
                     int ldv);

// ---- the table formulation (tables.hip, sorted.hip): quantised luminance (integer 0..255) on a Cartesian sample grid --
// table look-ups instead of exponentials.  Its limits, stated once: a grid of at most 32 x 36 samples (LDS and registers of
// the k_hist_* / k_ghist_* / k_sorted_* kernels) and at most 128 eigenvectors (project64, when V is asked for).
inline bool tables_apply(GridSpec gs, int K = 1) {
    return gs.nSelRows >= 1 && gs.nSelRows <= 32 && gs.nSelCols >= 1 && gs.nSelCols <= 36 && K <= 128;
}
hipError_t check_levels(hipStream_t s, const float* d_lum, long long n, int* d_flag);  // 2 ints: [0] != 0: not quantised, [1]: 16-level tiles that occur (bit t)
hipError_t hist_tables(hipStream_t s, GridSpec gs, const Sample4* d_samples, int p, double hx, double hy, int row0,
                       int nrows_local, double* d_er, double* d_ecT, double* d_Ep);

// ---- the literal decomposition in fp64 (generic64.hip): auto mode's fallback and the stage-level API
// What a launch of the fp64 affinity-row kernels takes (filled once per sample set: samples.hip, AffinityRows64).  Rows of
// ld columns, kab[i][j] = exp((-sw d2 - pw I_ij) - cw S_ab), every operation rounded on its own, with
//   R = 0 (k_affinity64, generic64.hip): I = dL^2, pw = 1/hy^2; chroma: S_ab = da^2 + db^2, sab[j] = sample j's (a, b), the
//     tables in affinity64_chroma_lds_bytes(ld) of LDS, at most kDynLdsDefault (what a launch gets without opting in to more);
//   1 <= R <= 7 (k_patch_affinity64, patch.hip): I = S_ij, the integer sum of squared differences of the (2R + 1)^2 patches
//     (reflect-101 borders, plane integer valued in [0, 255]), pw = (1/hy^2) / (2R + 1)^2.  spatch: patch_spatch_bytes(p, R)
//     bytes, sample j's patch values - 128 as int8 in row j (patch_kpad(R) bytes, zero padded; rows p .. roundup16(p) zero);
//     snorm[j] = the sum of the squares of those int8 values.  Chroma (R <= 3): S_ab likewise of the a and of the b patches,
//     cw = (1/hc^2) / (2R + 1)^2, a second i32 accumulation on the same MFMA; cpatch: patch_cpatch_bytes(p, R) bytes, row j
//     = sample j's a patch then its b patch, padded to patch_ckpad(R) bytes, cnorm as snorm; the tables take
//     patch_affinity64_chroma_lds_bytes(ld) of LDS, at most kPatchChromaLdsMax.
// A sample set that does not fit the LDS bound is hipErrorInvalidValue: the caller refuses it with a message first.
struct Affinity64Args {
    const float* lum = nullptr;  // the full H x W plane
    GridSpec gs{};
    const Sample4* samples = nullptr;
    int p = 0, ld = 0;
    double sw = 0.0, pw = 0.0;
    int R = 0;
    const signed char *spatch = nullptr, *cpatch = nullptr;  // R > 0; cpatch: with chroma
    const int *snorm = nullptr, *cnorm = nullptr;
    const float *a = nullptr, *b = nullptr;  // chroma (both set): the full a and b planes, integer valued in [0, 255]
    double cw = 0.0;
    const float2* sab = nullptr;  // chroma, R = 0
    // optional, with skip_samples: the rows zeroed are the pixels whose bit is set (bit i % 32 of word i / 32), not the grid's
    const unsigned* smask = nullptr;
};
constexpr size_t kDynLdsDefault = 64 * 1024;
constexpr size_t kPatchChromaLdsMax = 128 * 1024;  // dynamic LDS the chroma patch kernel may ask for (160 KiB per CU)
size_t affinity64_chroma_lds_bytes(int ld);
size_t patch_affinity64_chroma_lds_bytes(int ld);
int patch_kpad(int R);
int patch_ckpad(int R);
size_t patch_spatch_bytes(int p, int R);
size_t patch_cpatch_bytes(int p, int R);
// rows [pix0, pix0 + M) into d_kab; skip_samples: the rows of the sample pixels themselves come out as zeros
hipError_t affinity_rows64(hipStream_t s, const Affinity64Args& a, long long pix0, long long M, double* d_kab,
                           bool skip_samples);
// d_out (n x (2R + 1)^2 ints): the patch values around pixels d_pix[0 .. n) of the full plane
hipError_t patch_gather(hipStream_t s, const float* d_lum, int H, int W, int R, const long long* d_pix, int n, int* d_out);
// farthest-point sample selection (sampler.hip): the p pixels of NLE_SAMPLER_FARTHEST in the order chosen, into d_list (p
// ints), for the full H x W plane d_lum.  Workspace: d_m (H W doubles), d_pv / d_pi (2 farthest_max_blocks() each).
int farthest_max_blocks();
hipError_t farthest_samples(hipStream_t s, const float* d_lum, int H, int W, int p, double sw, double pw, double* d_m,
                            double* d_pv, int* d_pi, int* d_list);
// residual-greedy (pivoted-Cholesky) sample selection (sampler.hip): the p pixels of NLE_SAMPLER_RESIDUAL in the order
// chosen into d_list (p ints), their pivots into d_pivot (p doubles), for the full H x W plane d_lum; eps: the pivot below
// which the rule falls back to the farthest-point step.  Workspace: d_L, the factor (residual_ld(N) * p doubles, column j
// contiguous over the pixels), d_d and d_m (N doubles each), d_pv (6 farthest_max_blocks() doubles), d_pi (4
// farthest_max_blocks() ints), d_state (2 kResidHead doubles).  *d_state_final points at the kResidHead doubles the last
// launch left: {fallen back (0 / 1), n_residual, max d over the pixels not chosen, its first index, sum max(d, 0)}, the last
// three after the last residual round; with want_stats they include the last sample's own column (one more round)
constexpr int kResidHead = 8;
constexpr int kResidMaxSamples = 2048;
inline long long residual_ld(long long N) { return (N + 1) & ~1ll; }
hipError_t residual_samples(hipStream_t s, const float* d_lum, int H, int W, int p, double sw, double pw, double eps,
                            bool want_stats, double* d_L, double* d_d, double* d_m, double* d_pv, int* d_pi, double* d_state,
                            int* d_list, double* d_pivot, const double** d_state_final);
// d_out[k] = d_lum[d_pix[k]]
hipError_t gather_pix(hipStream_t s, const float* d_lum, const long long* d_pix, int n, float* d_out);
// d_mask (ceil(N / 32) words) = the bitmask of the pixels d_pix[0 .. n)
hipError_t sample_mask(hipStream_t s, const long long* d_pix, int n, long long N, unsigned* d_mask);
hipError_t add64(hipStream_t s, double* d_y, const double* d_x, size_t n);  // y += x
hipError_t row_scalings64(hipStream_t s, const double* d_X, long long M, int ld, int r, const double* d_u, double eps,
                          double* d_out);
// C (M x ldc) = diag(rs) A (M x lda, width kd) B (kd x nc column-major on the DEVICE); rs may be null
hipError_t ts_gemm64(hipStream_t s, const double* d_A, long long M, int lda, int kd, const double* d_B, int nc,
                     const double* d_rs, double* d_C, int ldc);
// C(i,j) = dl[i] (sum_k A(i,k) dk[k] B(k,j)) dr[j] + add(i,j); matrices by (pointer, row stride, column stride)
hipError_t gemm64s(hipStream_t s, int m, int n, int kk, const double* A, long long rsA, long long csA, const double* B,
                   long long rsB, long long csB, double* C, long long rsC, long long csC, const double* dl = nullptr,
                   const double* dk = nullptr, const double* dr = nullptr, const double* add = nullptr, long long rsD = 0,
                   long long csD = 0);
// Two kernels, one arithmetic (bit-identical results): up to 1024 16 x 16 output tiles (one workgroup per CU) the windowed
// form (all of a tile's operands in flight before its MFMA chain; one wave per SIMD), beyond it the streaming loop
int gemm64s_window();  // k per operand window of k_gemm64s (two windows are in flight together)
// one pass over X (M x ld, logical width w <= 2048: columns >= w are never read); d_t_in, d_lam and the rows of
// d_partial have (w + 3) & ~3 entries
hipError_t rowpass64(hipStream_t s, int mode, const double* d_X, long long M, int ld, int w, const double* d_t_in,
                     const double* d_lam, const float* d_xvec, double eps, double* d_partial, int* nblocks);
// G (r x r, full symmetric) = sum_i cs_i^2 x_i x_i^T (cs null: 1); d_partial: gram64d_partial_elems doubles
size_t gram64d_partial_elems(long long M, int r);
hipError_t gram64d(hipStream_t s, const double* d_X, long long M, int ld, int r, const double* d_cs, double* d_partial,
                   double* d_G);
hipError_t apply_expand64(hipStream_t s, const double* d_V, long long M, int ld, int K, const double* d_g, int L, float* d_Y,
                          long long ystride);
hipError_t scatter_rows64(hipStream_t s, const double* d_src, const long long* d_idx, int n, int ld, double* d_X, long long M);
hipError_t to_f32(hipStream_t s, const double* d_X, long long n, float* d_out);
// Y(i, j) = X(i, j) dl[i], X m x n col-major (leading dimension m), Y by (row stride, column stride)
hipError_t scale_rows64_to(hipStream_t s, const double* d_X, int m, int n, const double* d_dl, double* d_Y, long long rsY,
                           long long csY);

// ---- the Nystrom residual map (resid.hip): r_i = 1 - || F^T k_i ||^2 per pixel, F (p x m) with F F^T = pinv(K_A)
// Both routes write (float)r_i to d_r (may be null) and, per tile of kResidTile pixels, the summary partial {sum r, max r, index
// of the first maximum, count of r > thresh} from the fp64 r_i to d_part (4 resid_num_parts(N) doubles); resid_finish folds
// the partials into d_out (4 doubles) in a fixed order.
constexpr int kResidTile = 128;
inline long long resid_num_parts(long long N) { return (N + kResidTile - 1) / kResidTile; }
// fused (grid samples, single-value affinities, p <= 256): the fp64 affinities are generated inside the fp64-MFMA kernel.
// d_F: p x resid_fused_ld(m) row-major, columns >= m zero; sw = 1/hx^2, pw = 1/hy^2; the whole plane (N = H W pixels)
bool resid_fused_applies(int p);
int resid_fused_ld(int m);
hipError_t nystrom_resid64(hipStream_t s, const float* d_lum, GridSpec gs, const Sample4* d_samples, int p, double sw, double pw,
                           long long N, const double* d_F, int m, double thresh, float* d_r, double* d_part);
// rows: d_T (M x ldt, logical width m) = affinity rows [i0, i0 + M) times F (ts_gemm64); i0 a multiple of kResidTile
hipError_t resid_rows64(hipStream_t s, const double* d_T, long long M, int ldt, int m, long long i0, double thresh, float* d_r,
                        double* d_part);
hipError_t resid_finish(hipStream_t s, const double* d_part, long long nparts, double* d_out);

// ---- one-workgroup Householder tridiagonalisation (tridiag.hip): Q n x n col-major (lower triangle read), n <= tridiag_max_n();
// outputs in the conventions of nleh::tridiag_reduce (V: u_i in column i rows 0..i-1; hs; d, e)
int tridiag_max_n();
hipError_t tridiag(hipStream_t s, int n, const double* d_Q, const double* d_diag_add, double* d_V, double* d_d, double* d_e,
                   double* d_hs);

// ---- dense fp64 algebra of order n <= sytrd_max_n() on the device (dense64.hip)
// Householder tridiagonalisation in one persistent launch of G workgroups (0: sytrd_groups(n)); d_A n x n column-major, lower
// triangle read, d_diag_add (n, optional) added to the diagonal; d_pub: sytrd_pub_elems(n) doubles (the Householder vectors
// and scales stay there for sytrd_back); d_d[i] = T(i,i), d_e[i] = T(i,i-1), d_e[0] = 0; *d_status != 0 afterwards: a
// hand-off between workgroups timed out (the outputs are then meaningless)
int sytrd_max_n();
int sytrd_groups(int n);
size_t sytrd_pub_elems(int n);
hipError_t sytrd_dist(hipStream_t s, int n, int G, const double* d_A, const double* d_diag_add, double* d_pub, double* d_d,
                      double* d_e, int* d_status);
// all n eigenvalues of the tridiagonal matrix, DESCENDING, by multi-section Sturm counts (absolute accuracy ~ulp ||T||)
hipError_t tridiag_bisect(hipStream_t s, int n, const double* d_d, const double* d_e, double* d_D);
// Z (n x K, column stride ldz) <- Q Z with the orthogonal factor of sytrd_dist's reduction
hipError_t sytrd_back(hipStream_t s, int n, const double* d_pub, int K, double* d_Z, int ldz);
// Cholesky factor L of d_A (lower triangle read; d_A untouched), L^-1 and d_scal[0] = trace(A^-1); *d_status |= 2 when a pivot
// is not positive; d_tmp: potrf_tmp_elems(n) doubles of scratch
size_t potrf_tmp_elems(int n);
hipError_t potrf_inverse(hipStream_t s, int n, const double* d_A, double* d_L, double* d_Linv, double* d_tmp, double* d_scal,
                         int* d_status);
// d_dst = d_src^T, n x n column-major with column strides lds / ldd (0: n)
hipError_t transpose64(hipStream_t s, int n, const double* d_src, double* d_dst, int lds = 0, int ldd = 0);
hipError_t symm_lower64(hipStream_t s, int n, const double* d_src, double* d_dst);  // mirror the lower triangle
hipError_t fill64(hipStream_t s, double* d_p, size_t n, double v);
// d_dst (n x n) = diag(dl) src[:n, :n] diag(dr); src column stride lds
hipError_t scale_rc64(hipStream_t s, int n, const double* d_src, int lds, const double* d_dl, const double* d_dr, double* d_dst);

// ---- level-sorted rows (sorted.hip): the pixel halves of the table passes without LDS atomics
constexpr int kSortedThreads = 512;
struct SortedRows {
    const unsigned short* scol;   // [nrows][pitch] per row: one slot of 8 x column per chunk (sample pixels left out)
    const uint2* desc;            // [nrows][kSortedThreads] chunk of each pass thread
    const unsigned short* first;  // [nrows][258] first chunk of each level; [257] tree steps
    const double* E;              // [W + 1] exp(-d^2 / hx^2)
    bool rec;                     // column factors by recurrence from two table reads (sorted_recurrence)
    double kappa;                 // exp(-2 colStep^2 / hx^2)
    const double* E2 = nullptr;   // [W + 1] exp(-2 d^2 / hx^2): set (with hx) where the Gram runs on index sums (sorted_gsum_ok)
    double hx = 0.0;
    int lev_t0 = 0, lev_nt = 16;  // the 16-level tiles [lev_t0, lev_t0 + lev_nt) that occur in the image (check_levels)
    bool mom = false;             // the pass kernel's pixel loop in its moment form (sorted_moments_ok)
    int wgs_per_cu = 2;           // workgroups per compute unit of the sorted kernels' grids: two of 512 threads, each walks its rows
};
// What the composite launchers below take: the table path's state on one rank, rows [row0, row0 + nrows) of the image;
// non-owning (pipeline_internal.h: TableFilter owns it)
struct TableView {
    const float* lum;              // virtual base of the full image: only this rank's rows are ever dereferenced
    GridSpec gs;
    int p, ldp;                    // samples; ldp = sink_pass_ld(p), the stride of the p-sized vectors
    int row0, nrows;
    const double *er, *ecT, *Ep;   // hist_tables
    // c_i per local pixel: the last Sinkhorn pass writes it.  The rule for the sample pixels: no kernel uses c there -- the
    // sorted rows leave them out, the LDS-atomic kernels (k_hist_pix, k_hist_dot, k_ghist_rows*) test the grid's predicate
    // before they read -- so whatever the buffer holds at a sample pixel, a NaN included, reaches no sum and no output
    const double* cvec;
    const SortedRows* sorted;      // null: the pixel kernels are the LDS-atomic ones (k_hist_pix, k_hist_dot, k_ghist_rows*)
};

// sorted_gsum_ok, sorted_recurrence, sorted_moments_ok: pure functions of the grid and the bandwidth -- where the form
// named stays inside fp64's normal range.  Whoever fills a SortedRows combines them with what else decides the form.
// Gram by index sums (sorted.hip: k_sorted_gsum): S_r[t][x] = sum c_i^2 G_t(col_i), t < 2 nC - 1; layout [row][t][level]
bool sorted_gsum_ok(GridSpec gs, double hx);
hipError_t sorted_gram_sums(hipStream_t s, GridSpec gs, int nrows, const SortedRows& sr, const double* d_cvec, double* d_Aout);
bool sorted_recurrence(GridSpec gs, double hx, double* kappa);
int sorted_max_width();
size_t sorted_scol_elems(int W, int nrows_local);  // allocation size of SortedRows::scol
// the inverse of sort_rows: this rank's rows of the plane (nrows_local x W fp32 at d_out) from the sorted rows and the
// sample values (the sample pixels are not in the sorted rows); exact for the integer-valued plane sort_rows took
hipError_t rows_from_sorted(hipStream_t s, GridSpec gs, int row0, int nrows_local, const SortedRows& sr, const Sample4* d_samples,
                            int p, float* d_out);
// expand half of the sample-space apply on the sorted rows (nl <= sorted_expand_layers() layers per launch)
int sorted_expand_layers(GridSpec gs);
hipError_t sorted_expand(hipStream_t s, GridSpec gs, int nrows, const SortedRows& sr, const double* d_g, size_t gstride, int nl,
                         const double* d_cvec, float* d_out, long long ostride, bool round8);
hipError_t dist_table(hipStream_t s, int W, double hx, double* d_E);
// d_lev (optional, nrows_local x W bytes): the level of EVERY pixel of this rank's rows, sample pixels included -- the
// plane itself, it being integer valued in [0, 255]
hipError_t sort_rows(hipStream_t s, const float* d_lum, GridSpec gs, int row0, int nrows_local, unsigned short* d_scol,
                     uint2* d_desc, unsigned short* d_first, unsigned char* d_lev = nullptr);
// *d_flag |= 1 unless d_x[i] has the bits of (float)d_lev[i] for every i < n (d_x: first pixel of the rows d_lev holds);
// the caller zeroes the flag.  (A -0.0f where the level is 0 counts as different.)
hipError_t plane_matches_levels(hipStream_t s, const float* d_x, const unsigned char* d_lev, long long n, int* d_flag);
// gather_samples_slab's values from the level plane of rows [row0, row0 + nrows_local): d_out[k] = the level of sample k
hipError_t gather_sample_levels(hipStream_t s, const unsigned char* d_lev, GridSpec gs, int row0, int nrows_local, double* d_out);
// the table columns of sr's level tiles only; the pixel loop in the form sr.mom / sr.rec say
hipError_t sorted_pass(hipStream_t s, int mode, GridSpec gs, int row0, int nrows, const SortedRows& sr, const double* d_g,
                       double eps, double* d_ybuf, double* d_h, const double* d_cvec, const float* d_xvec,
                       const int* d_run_if = nullptr);
bool sorted_moments_ok(GridSpec gs, double hx);
// the XVEC pass for a group of planes in ONE walk over the sorted rows (sorted_planes.hip: k_sorted_reduce_planes): plane m
// of the group is read at x[m] (virtual base of the full image) and its tables go to h[m], in sorted_pass's layout and with
// sorted_pass's bits.  2 <= np <= sorted_planes_per_launch(gs): four planes up to 12 columns, two beyond.
constexpr int kPlanesPerLaunch = 4;
struct PlaneGroup {
    const float* x[kPlanesPerLaunch];
    double* h[kPlanesPerLaunch];
};
int sorted_planes_per_launch(GridSpec gs);
hipError_t sorted_reduce_planes(hipStream_t s, GridSpec gs, int row0, int nrows, const SortedRows& sr, const double* d_cvec,
                                const PlaneGroup& pg, int np);
hipError_t sorted_gram_rows(hipStream_t s, GridSpec gs, int nrows, const SortedRows& sr, const double* d_cvec, double* d_Aout);

// the table pass (three kernels, Ep read once per pass); writes the full column sums to d_z.  d_ybuf (optional): y_i per
// local pixel; mode XVEC (apply, reduce half): y_i = cvec_i * xvec_i
size_t hist_tiled_workspace_elems(GridSpec gs, int nrows_local);
// d_run_if (optional, sorted rows only): a device int; where it is 0 when the kernels start, they return at once and
// d_ws, d_z stay as they were -- the caller has the result from elsewhere (apply_sample_space)
hipError_t sink_hist_tiled(hipStream_t s, int mode, const TableView& v, const double* d_w, double eps, double* d_ybuf,
                           double* d_ws, double* d_z, LaunchObserver* obs = nullptr, const float* d_xvec = nullptr,
                           const int* d_run_if = nullptr);
// reduce half of the sample-space apply for 2 <= np <= sorted_planes_per_launch(v.gs) planes on the level-sorted rows
// (v.sorted != null): one pixel kernel for the group, then the HH stage and the column sums plane by plane; d_x: np planes
// (virtual full bases); d_ws: apply_reduce_planes_workspace_elems doubles; d_m: np vectors of stride v.ldp, each the bits
// sink_hist_tiled(ROWPASS_XVEC) gives that plane
size_t apply_reduce_planes_workspace_elems(GridSpec gs, int nrows_local, int np);
hipError_t apply_reduce_planes(hipStream_t s, const TableView& v, const float* const* d_x, int np, double* d_ws, double* d_m,
                               LaunchObserver* obs = nullptr);
// sample-space apply (tables): expand half for nl <= apply_layers_per_launch(v) layers (decided there and nowhere else), the
// p/K-sized middle, and the sample-pixel outputs
int apply_layers_per_launch(const TableView& v);
hipError_t apply_hist_layers(hipStream_t s, const TableView& v, const double* d_wl, int ldw, int nl, double* d_ws, float* d_out,
                             long long ostride, LaunchObserver* obs, bool round8 = false);
// d_differs (optional): a device int; where it is 0, d_m_same and d_xA_same stand in for d_m and d_xA
hipError_t apply_small(hipStream_t s, int p, int K, int ldk, int L, int ldw, const double* d_m, const double* d_D,
                       const double* d_Vrows, const double* d_xA /* x at the p sample pixels */, const double* d_resp,
                       double* d_t, double* d_Wp, double* d_YA, const int* d_differs = nullptr, const double* d_m_same = nullptr,
                       const double* d_xA_same = nullptr);
hipError_t scatter_samples(hipStream_t s, int p, int L, const long long* d_loc, const double* d_YA, float* d_Y,
                           long long ystride, bool round8 = false);  // round8: clamp to [0, 255], round half to even, in fp64

// Gram in sample space through the same tables; d_Gk: p x p
size_t ghist_workspace_elems(GridSpec gs, int nrows_local);
hipError_t gram_hist(hipStream_t s, const TableView& v, double* d_ws, double* d_Gk, LaunchObserver* obs = nullptr);
// image rows per split and number of splits of gram_hist's GEMM on this view (the C or T part of d_ws holds nsplit products)
void gram_hist_split(const TableView& v, int* ksplit, int* nsplit);

// 8-bit BGR <-> Lab (colour.hip): d_lut = the fixed-point tables of nle_lab8_tables as one blob; d_lab / d_L optional outputs
hipError_t bgr2lab8(hipStream_t s, const unsigned char* d_bgr, long long n, const double* d_lut, unsigned char* d_lab,
                    float* d_L);
hipError_t lab2bgr8(hipStream_t s, const unsigned char* d_lab, const float* d_L, const float* d_a, const float* d_b,
                    long long n, const double* d_lut, unsigned char* d_bgr);
hipError_t channel8(hipStream_t s, const unsigned char* d_img, long long n, int ch, float* d_out);
// cv::max(y, 0) / cv::min(y, 255) / convertTo(CV_8U) of a filtered plane (src/filter.cpp:434-436): round half to even
hipError_t plane_to_u8(hipStream_t s, const float* d_y, long long n, unsigned char* d_out);
hipError_t channel8_plane(hipStream_t s, const unsigned char* d_u8, long long n, float* d_out);  // bytes -> fp32 levels
// 16-bit sRGB <-> float Lab (colour16.hip): d_tab = lin | coeffs | threshold pairs as one blob
// (srgb16.h: the tables of nle_srgb16_tables in the form the kernels read); d_a, d_b, d_guide optional outputs of the forward direction
hipError_t bgr16_to_lab(hipStream_t s, const unsigned short* d_bgr, long long n, const double* d_tab, float* d_L,
                        float* d_a, float* d_b, float* d_guide);
hipError_t lab_to_bgr16(hipStream_t s, const float* d_L, const float* d_a, const float* d_b, long long n,
                        const double* d_tab, unsigned short* d_bgr);
// HDR tone mapping (tonemap.hip): interleaved linear-light BGR fp32 in.  hdr_range: d_partial holds
// 2 * hdr_range_blocks(n) doubles of workspace, d_pair receives (Ymax, Ymin+), Ymax = 0 when no luminance is finite and > 0.
// hdr_to_loglum: d_x and d_guide optional.  loglum_to_bgr16: white = 255 c, [y_lo, y_hi] = [2^(l_hi - range), 2^l_hi];
// d_tab as for lab_to_bgr16 (its threshold pairs).
int hdr_range_blocks(long long n);
hipError_t hdr_range(hipStream_t s, const float* d_bgr, long long n, double* d_partial, double* d_pair);
hipError_t hdr_to_loglum(hipStream_t s, const float* d_bgr, long long n, double l_hi, double range, float* d_x, float* d_guide);
hipError_t loglum_to_bgr16(hipStream_t s, const float* d_y, const float* d_bgr, long long n, double range, double white,
                           double saturation, double y_lo, double y_hi, const double* d_tab, unsigned short* d_bgr16);
// region edits (region.hip; the rule is stated in include/nle.h at nle_region_combine): per pixel the memberships of the M
// spread stroke planes d_q blend the rows of wt ((M + 1) x L, row 0 the background) into one weight per layer, and the L
// layer planes d_layers are summed under those weights -- fp64, every operation rounded on its own.  Planes by base pointer
// and plane stride (in floats); out_kind: NLE_REGION_OUT_*; d_out n floats, or n bytes for NLE_REGION_OUT_U8.
constexpr int kRegionLayersMax = 16, kRegionMax = 8;  // NLE_REGION_LAYERS_MAX, NLE_REGION_MAX
struct RegionWeights {
    double wt[(kRegionMax + 1) * kRegionLayersMax];  // the first (M + 1) * L entries are read
};
hipError_t region_combine(hipStream_t s, const float* d_layers, long long layer_stride, int L, const float* d_q,
                          long long q_stride, int M, long long n, const RegionWeights& wt, double floor, int out_kind,
                          void* d_out);
// the out-of-span detail layer and the detail curve (detail.hip; the rule is stated in include/nle.h at nle_detail_combine):
// per pixel rho = x - sum of the L layers joins them as one more weighted layer, and rho and every layer but the last pass
// the gain curve g first -- fp64, every operation rounded on its own.  Planes and out_kind as for region_combine.
struct DetailWeights {
    double w[kRegionLayersMax];  // the first L entries are read
};
hipError_t detail_combine(hipStream_t s, const float* d_x, const float* d_layers, long long layer_stride, int L, long long n,
                          const DetailWeights& w, double w_rho, double gain, double sigma, int out_kind, void* d_out);
// the base tone curve (tone.hip, detail.hip; the rule is stated in include/nle.h at nle_tone_combine).  plane_hist: d_counts
// receives the kToneCounts counters of nle_plane_histogram (zeroed on the stream first).  tone_curve: the host rule of
// nle_tone_curve; null, or the message of its refusal (tone_check: of the four parameters alone).  tone_combine: detail_combine with the base term passed through the
// curve of the NLE_TONE_KNOTS knots at d_knots (device), u = (Bw - lo) ks.
constexpr int kToneCounts = 4098;  // NLE_TONE_BINS + 2: underflow, the bins, overflow and NaN
hipError_t plane_hist(hipStream_t s, const float* d_x, long long n, double scale, unsigned long long* d_counts);
const char* tone_check(double shadows, double highlights, double clip_percent, double equalise);
const char* tone_curve(const long long* counts, double shadows, double highlights, double clip_percent, double equalise,
                       double* curve);
hipError_t tone_combine(hipStream_t s, const float* d_x, const float* d_layers, long long layer_stride, int L, long long n,
                        const DetailWeights& w, double w_rho, double gain, double sigma, const double* d_knots, double lo, double ks,
                        int out_kind, void* d_out);
// local adjustments (local.hip; the rule is stated in include/nle.h at nle_local_combine): region_combine's memberships blend
// the results of M + 1 rows, each the detail / tone rule with parameters of its own.  Row m: curve != 0 when sigma > 0 and
// gain != 1; slot >= 0 is the index of its tone curve among the ncurves active ones (NLE_TONE_KNOTS knots each at d_knots,
// device), u = (Bw - lo) ks; slot < 0: no base curve.  wt as RegionWeights.  local_chroma: a' = 128 + c (a - 128) with
// c = the memberships' blend of saturation[0 .. M]; in place allowed.
struct LocalRow {
    double w_rho, gain_m1, sigma, lo, ks;
    int curve, slot;
};
struct LocalRows {
    LocalRow row[kRegionMax + 1];                    // the first M + 1 entries are read
    double wt[(kRegionMax + 1) * kRegionLayersMax];  // the first (M + 1) * L entries are read
};
hipError_t local_combine(hipStream_t s, const float* d_x, const float* d_layers, long long layer_stride, int L, const float* d_q,
                         long long q_stride, int M, long long n, const LocalRows& rows, const double* d_knots, int ncurves,
                         double floor, int out_kind, void* d_out);
hipError_t local_chroma(hipStream_t s, const float* d_a, const float* d_b, const float* d_q, long long q_stride, int M, long long n,
                        const double* saturation, double floor, float* d_a_out, float* d_b_out);
// per-region histograms (region_hist.hip; the rule is stated in include/nle.h at nle_region_histograms): the memberships of
// local_combine weigh every pixel's count, omega_m = the round half up of alpha_m NLE_REGION_WEIGHT_ONE, into the histogram of
// y scale[m] of every row m = 0 .. M that is on.  slot[m]: the row's place among the nslots rows that are on, < 0 for a row
// that is off; d_counts receives nslots x kToneCounts counters, slot-major (zeroed on the stream first).
hipError_t region_hist(hipStream_t s, const float* d_y, const float* d_q, long long q_stride, int M, long long n, const double* scale,
                       const int* slot, int nslots, double floor, unsigned long long* d_counts);
// automatic regions (segment.hip; the rule is stated in include/nle.h at nle_filter_segment).  Labels are one byte per
// pixel, planes go by base pointer and stride in floats, C is 1 .. kRegionMax.  Everything a step leaves for the host sits
// in one SegmentResult on the device (zeroed by the launcher where the kernels add to it).
//   segment_init    label = the number of cuts b_1 <= .. <= b_{C-1} the pixel's quarter-level bin has reached
//   segment_stats   count[c], sum[c] = the fp64 sum of q_{label}[i] over the members, mean[c] = sum / count (+inf for an
//                   empty cluster), bad = the labels >= C (never used as an index).  The sums go through
//                   segment_stats_blocks(n) x kRegionMax per-workgroup partials at d_partial and are folded in a fixed order.
//   segment_assign  label' = the smallest c with the smallest mean[c] - 2 q_c[i], read from r->mean; d_ind (may be null)
//                   receives the C indicator planes of the new labels; new_count, changed and bad_new are added to.  d_q
//                   null: no plane is read and no label moves -- the indicator planes and counts of the labels as they are.
struct SegmentResult {
    unsigned long long count[kRegionMax], bad;
    double sum[kRegionMax], mean[kRegionMax];
    unsigned long long new_count[kRegionMax], changed, bad_new;
};
struct SegmentCuts {
    int b[kRegionMax - 1];  // the first C - 1 entries are read
};
int segment_stats_blocks(long long n);
hipError_t segment_init(hipStream_t s, const float* d_x, long long n, int C, const SegmentCuts& cuts, unsigned char* d_labels);
hipError_t segment_stats(hipStream_t s, const float* d_q, long long q_stride, int C, long long n, const unsigned char* d_labels,
                         double* d_partial, SegmentResult* d_r);
hipError_t segment_assign(hipStream_t s, const float* d_q, long long q_stride, int C, long long n, unsigned char* d_labels,
                          float* d_ind, long long ind_stride, SegmentResult* d_r);
// single-channel 8-bit bilateral filter (fp32 planes holding integers); tables from the host: space_w (2r+1)^2 with 0
// outside the circle, colour_w 256 entries
int bilateral8_max_radius();
hipError_t bilateral8(hipStream_t s, const float* d_src, int H, int W, int radius, const float* d_space_w,
                      const float* d_colour_w, float* d_dst);

// out[block][2*ncols] = {min, max} of the first ncols columns of X over the block's rows
hipError_t col_range(hipStream_t s, const float* d_X, long long M, int ld, int ncols, float* d_out, int nblocks);

// Y[l][i] = sum_k V[i][k] * g[l][k]   (g: L x ld doubles, device)
hipError_t apply_expand(hipStream_t s, const float* d_V, long long M, int ld, const double* d_g,
                        int L, float* d_Y, long long ystride);

// X[idx[k]] = src[k] (ld floats each) for idx[k] in [0, M)
hipError_t scatter_rows(hipStream_t s, const float* d_src, const long long* d_idx, int n, int ld,
                        float* d_X, long long M);

// ---- the exact filter (exact.hip, NLE_MODE_EXACT_F64): Y = K X with the N x N affinity regenerated on the fly
// lum: the H x W plane (integer valued in [0, 255]); d_es / d_el: exact_tables' spatial (es_len >= max(H, W)) and
// level (256) tables on the device; d_part: exact_part_elems(H W) doubles of workspace for the one- and two-column form
struct ExactPlane {
    const float* lum;
    int H, W;
    const double* d_es;
    int es_len;
    const double* d_el;
    double* d_part;
};
void exact_tables(int H, int W, double hx, double hy, std::vector<double>* es, std::vector<double>* el);
size_t exact_part_elems(long long N);
// Y (N x ldy, columns < ncols) = K X (N x ldx, columns < ncols); deterministic, segmented over the source pixels
hipError_t affinity_product64(hipStream_t s, const ExactPlane& pl, const double* d_X, int ldx, int ncols, double* d_Y, int ldy);
// the eigensolver's element-wise steps (exact_train.hip: ExactSolver)
hipError_t exact_start(hipStream_t s, double* d_X, long long N, int ld, int col0, int ncols, unsigned seed);
hipError_t exact_scale2(hipStream_t s, const double* d_X, int ldx, long long N, int b, const double* d_c, const double* d_r,
                        double* d_Z);
hipError_t exact_combine(hipStream_t s, const double* d_Y, long long N, int b, const double* d_c, const double* d_r, double* d_A,
                         int lda);
hipError_t exact_recip(hipStream_t s, double* d_v, long long N, double eps);
hipError_t exact_axpby(hipStream_t s, const double* d_S, int lds, double alpha, const double* d_B, int ldb, double beta,
                       double* d_D, int ldd, long long N, int n, int pad);
int exact_col_blocks(long long N);
hipError_t exact_colnorm2(hipStream_t s, const double* d_A, int lda, const double* d_B, int ldb, const double* d_theta,
                          long long N, int n, double* d_part);
hipError_t exact_colmaxabs(hipStream_t s, const double* d_A, int lda, long long N, int n, double* d_pv);
hipError_t exact_scale_cols(hipStream_t s, double* d_A, int lda, long long N, int n, const double* d_s);

}  // namespace nlek
