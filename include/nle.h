/*
 * nle.h -- C ABI of the MI355X-native nonlocal-filter hot path.
 *
 * This is the drop-in boundary for the path `src/filter.cpp` of
 * lightalchemist/nonlocal-image-edit names (computeKernel -> nystromApproximation ->
 * sinkhorn -> orthogonalize -> P*V, then NLEFilter::apply).  The reference has no FFI
 * of its own (it is one C++ translation unit calling Eigen/OpenCV); the symbols below
 * are what a binding for this path binds, and `include/nle/filter.hpp` is the C++
 * surface with the reference's own names layered over them.  Each entry point cites
 * the reference interface it replaces (paths relative to the reference tree).
 *
 * Conventions
 *   - plain C types only; every function returns an int status (0 == NLE_OK);
 *     the message for the last failure is `nle_last_error(ctx)`.
 *   - "d_" pointers are DEVICE (HIP) pointers, "h_" pointers are HOST pointers.
 *   - N-sized matrices are fp32, ROW-PER-PIXEL (row-major, leading dimension `ld`,
 *     a multiple of 4; columns >= the logical width are zero), in NATURAL pixel order
 *     (row-major image scan), not the reference's [selected; rest] order.
 *   - small (p x p, r x r, r- and K-sized) quantities are fp64 on the host, matrices
 *     COLUMN-MAJOR like the reference's Eigen::MatrixXd (include/filter.hpp:10-12).
 *   - all device work is stream-ordered on the ctx's stream; a ctx is used by one
 *     host thread at a time (the reference is single-threaded and keeps no globals).
 *   - there is NO CPU fallback: without a HIP device every compute entry point fails
 *     with NLE_ERR_HIP.
 */
#ifndef NLE_H
#define NLE_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NLE_OK 0
#define NLE_ERR_INVALID 1  /* bad argument / shape; message mirrors the reference's runtime_error text */
#define NLE_ERR_HIP 2      /* HIP runtime failure (incl. no device) */
#define NLE_ERR_NUMERIC 3  /* eigensolver did not converge / empty spectrum */
#define NLE_ERR_COMM 4     /* all-reduce callback failed */

#define NLE_EPS 1e-10 /* include/filter.hpp:14 */

typedef struct nle_ctx nle_ctx;
typedef struct nle_filter nle_filter;

/* ---- context ------------------------------------------------------------------- */
/* `stream` is a hipStream_t to run on, or NULL to let the ctx create and own a non-blocking
 * stream.  NB: the handle of HIP's legacy default stream IS NULL, so it cannot be passed; a host
 * that wants its own collectives ordered with the ctx's kernels (torch.distributed) creates a
 * stream, hands its handle over and issues the collectives on it (the Python mirror does). */
int nle_ctx_create(int device, void* stream, nle_ctx** out);
void nle_ctx_destroy(nle_ctx* ctx);
const char* nle_last_error(const nle_ctx* ctx); /* ctx may be NULL: last create error */
int nle_ctx_synchronize(nle_ctx* ctx);
/* The ctx keeps the device workspace of finished calls (and of destroyed filters) for reuse by
 * the next call; nle_ctx_trim returns it to the driver (nle_ctx_destroy does so too). */
int nle_ctx_trim(nle_ctx* ctx);

/* Device memory helpers for hosts that do not link the HIP runtime themselves (the C++ surface in
 * include/nle/filter.hpp, a cgo/JNI/ctypes binding): plain hipMalloc / hipFree / hipMemcpy on
 * the ctx's device, synchronous with respect to the ctx's stream. */
int nle_dev_alloc(nle_ctx* ctx, size_t bytes, void** d_ptr);
void nle_dev_free(nle_ctx* ctx, void* d_ptr);
/* page-locked host memory (hipHostMalloc): host buffers handed to the *_host entry points are copied at PCIe speed
 * and asynchronously only when they are pinned */
int nle_host_alloc(nle_ctx* ctx, size_t bytes, void** h_ptr);
void nle_host_free(nle_ctx* ctx, void* h_ptr);
int nle_dev_upload(nle_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int nle_dev_download(nle_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);

/* Which formulation nle_train uses for the N-sized passes:
 *   NLE_MODE_AUTO          the table form of NLE_MODE_PHI_FREE when it applies (integer-valued luminance plane -- what the
 *                          reference always feeds, the L channel of 8-bit Lab, src/filter.cpp:460-469 -- a sample grid of at
 *                          most 32 x 36, <= 128 eigenvectors), else NLE_MODE_MATERIALISED_F64.  Both are fp64 from the
 *                          affinities to the last reduction and meet the 1e-4 per-layer bar wherever the reference
 *                          algorithm itself is well posed; nle_filter_diag reports which one ran.  The two fp32
 *                          formulations below run only when asked for: they are the north star's literal kernels
 *                          (fp32 MFMA GEMMs, HBM-streamed Sinkhorn) and can miss the bar on inputs whose detail layers
 *                          are small differences (DESIGN.md "Numerics").
 *   NLE_MODE_MATERIALISED  Phi = K_AB^T V_A Lambda^-1 is written once (N x r fp32) and streamed
 *   NLE_MODE_PHI_FREE      every pass regenerates its affinity rows in registers; when the luminance
 *                          plane is integer valued in [0, 255] (the L channel of 8-bit Lab, what the
 *                          reference always feeds, src/filter.cpp:460-469) the Sinkhorn passes use
 *                          fp64 look-up tables instead of exponentials
 *   NLE_MODE_PHI_FREE_EXP  Phi-free without the look-up-table specialisation */
#define NLE_MODE_AUTO 0
#define NLE_MODE_MATERIALISED 1
#define NLE_MODE_PHI_FREE 2
#define NLE_MODE_PHI_FREE_EXP 3
/*   NLE_MODE_MATERIALISED_F64  the literal decomposition with Phi (N x r) and V (N x K') in fp64: fp64 affinities,
 *                          fp64-MFMA products, any luminance, up to 2048 samples (Phi must fit in device memory) */
#define NLE_MODE_MATERIALISED_F64 4
/*   NLE_MODE_STREAMED_F64  fp64 like NLE_MODE_MATERIALISED_F64 but without the N x r matrix: the sample-space algebra of
 *                          NLE_MODE_PHI_FREE on fp64 affinity rows regenerated chunk by chunk (libm exp) in every pass; the
 *                          workspace is bounded (NLE_STREAM64_CHUNK_MB, default 2048), V (N x K') is fp64.  Any plane, any
 *                          grid with <= 2048 samples, any K: what auto mode takes when Phi would not fit the device. */
#define NLE_MODE_STREAMED_F64 5
/*   NLE_MODE_EXACT_F64     the exact filter, opt-in (new in this build; auto mode never takes it): the reference algorithm
 *                          with the full pixel affinity in place of the Nystrom extension -- no samples (nRow, nCol are
 *                          checked as the reference checks them, :117-119, and not used).  For the plane y (H x W, N = HW,
 *                          pixel i at (r_i, c_i), row-major), sw = 1/hx^2, pw = 1/hy^2:
 *                            K_ij = exp(-sw (double)((r_i - r_j)^2 + (c_i - c_j)^2) - pw (y_i - y_j)^2), all N x N entries
 *                            r = 1;  T times: c = recip(K r);  r = recip(K c)   (recip: inplaceReciprocal, :42-54, EPS 1e-10)
 *                            W = diag(r) K diag(c);  Ws = (W + W^T) / 2
 *                            (lambda_k, v_k) = the min(K, N) largest eigenpairs of Ws by algebraic value, descending; the
 *                            leading ones with lambda >= 1e-10 are kept (K', :213-215)
 *                          each v_k unit norm, its entry of largest magnitude positive (ties: the lowest index); every
 *                          kept pair has ||Ws v - lambda v||_2 <= 1e-10 by an explicit operator application, else the train
 *                          returns NLE_ERR_NUMERIC.  K is regenerated on the fp64 matrix cores, never stored (O(N^2) work
 *                          per product); bitwise reproducible on one device.  Needs an integer-valued plane in [0, 255],
 *                          N <= NLE_EXACT_MAX_PIXELS, 1 <= nEigenVectors <= 256, patch radius 0, NLE_SAMPLER_GRID and
 *                          world == 1; anything else returns NLE_ERR_INVALID before any collective.  V (N x K') is fp64;
 *                          nle_filter_diag gives {6, 0, 0, 0, K', K', 0, 0}; nle_filter_timings [0] 0, [1] Sinkhorn, [2] the
 *                          eigensolver's operator products, [3] orthogonalisation, Ritz and V assembly, [4] host algebra,
 *                          [5] wall total. */
#define NLE_MODE_EXACT_F64 6
#define NLE_EXACT_MAX_PIXELS 1048576 /* 1 << 20 */
int nle_ctx_set_mode(nle_ctx* ctx, int mode);
/* Patch (non-local-means) affinities, opt-in (new in this build: the reference compares single pixel values,
 * src/filter.cpp:94-112).  With radius R > 0 the intensity term of every affinity, K_A and K_AB alike, compares the
 * (2R + 1)^2 neighbourhoods of the two pixels (reflect-101 borders, OpenCV BORDER_DEFAULT):
 *   S_ij = sum_{dy,dx in [-R, R]} (y[rho(r+dy), rho(c+dx)] - y[rho(rs+dy), rho(cs+dx)])^2    (an exact integer)
 *   K_ij = exp(-(1/hx^2) (double)((r-rs)^2 + (c-cs)^2) - ((1/hy^2) / (2R+1)^2) (double)S_ij)
 * so hy keeps its meaning (an intensity difference per pixel); R = 0 (default) is the reference's kernel bit for bit and
 * leaves every code path unchanged.  Every later stage is the reference's.  R > 0 applies to nle_train* and
 * nle_compute_kernel64 and needs an integer-valued plane in [0, 255] (the L channel of 8-bit Lab), R <= min(H, W) - 1,
 * NLE_MODE_AUTO (which then takes NLE_MODE_MATERIALISED_F64, or NLE_MODE_STREAMED_F64 by the memory rule),
 * NLE_MODE_MATERIALISED_F64 or NLE_MODE_STREAMED_F64, and full-plane input at world > 1 (no slab input); anything else,
 * nle_compute_kernel and nle_nystrom included, returns NLE_ERR_INVALID.  0 <= radius <= NLE_PATCH_RADIUS_MAX. */
#define NLE_PATCH_RADIUS_MAX 7
int nle_ctx_set_patch_radius(nle_ctx* ctx, int radius);
/* Chroma-aware (Lab) affinities, opt-in (new in this build: the reference compares two pixels by position and luminance
 * only, src/filter.cpp:94-112, so two regions of equal lightness and different colour are one tone to the filter).  With
 * the a and b planes of 8-bit Lab set (d_a, d_b: device pointers to the full H x W planes, fp32, integer valued in
 * [0, 255] -- what nle_lab8_channel gives; BORROWED until they are replaced or cleared) every affinity, K_A and K_AB
 * alike, gets one more term.  With R the patch radius (0: single values), rho reflect-101 and e0 the exponent this build
 * computes without chroma (R = 0: -(1/hx^2) (double)d2 - (1/hy^2) dL^2; R > 0: -(1/hx^2) (double)d2 - pwd (double)S_L):
 *   S_ab = sum_{dy,dx in [-R, R]} (a[rho(r+dy), rho(c+dx)] - a[rho(rs+dy), rho(cs+dx)])^2 + (b[..] - b[..])^2   (exact integer)
 *   K_ij = exp(e0 - cwd (double)S_ab),   cwd = (1/hc^2) / (2R+1)^2
 * the chroma term subtracted last, every operation rounded on its own (no fma).  hc > 0 is the chroma bandwidth: a chroma
 * difference per pixel, the same unit as hy.  Every later stage is the reference's.  NULL, NULL and any hc: off (the
 * default), and then none of this runs: every code path and every number is what it was.  One pointer NULL and the other
 * not, or hc not finite or <= 0, is NLE_ERR_INVALID.  The planes describe the trains (nle_train, nle_train_host,
 * nle_train_host_u8) and nle_compute_kernel64 calls that follow, exactly where patch affinities run: NLE_MODE_AUTO (which
 * then takes NLE_MODE_MATERIALISED_F64, or NLE_MODE_STREAMED_F64 by the memory rule) and those two modes; the grid and the
 * farthest sampler; full-plane input at world > 1.  A train checks that L, a and b are integer valued in [0, 255] (agreed
 * by every rank).  Anything else returns NLE_ERR_INVALID before any collective and leaves the ctx usable: the other modes
 * (a 256-level table cannot index a colour triple), nle_compute_kernel, nle_nystrom, slab input at world > 1, a
 * non-integer plane, and a patch radius above NLE_CHROMA_PATCH_RADIUS_MAX (S_ab is a second int8 MFMA accumulation over
 * 2 (2R+1)^2 values; radius 4-7 would add three or more K steps where the plane gather already dominates).  The farthest
 * sampler keeps its luminance-only distance D below: chroma applies to the affinities only, as a patch radius does.
 * The affinity kernels keep the samples' tables in LDS: with chroma nle_compute_kernel64 takes at most 2728 samples at patch
 * radius 0 and 5984 above (NLE_ERR_INVALID beyond; a train takes at most 2048 anyway).
 * Applying a filter needs nothing: V is explicit in both fp64 forms.  nle_filter_chroma: the hc a filter was trained with,
 * 0.0 when it was trained without. */
#define NLE_CHROMA_PATCH_RADIUS_MAX 3
int nle_ctx_set_chroma(nle_ctx* ctx, const float* d_a, const float* d_b, double hc);
int nle_filter_chroma(const nle_filter* f, double* hc);
/* Sample selection, opt-in (new in this build: the reference always takes its Cartesian grid, src/filter.cpp:56-80).
 *   NLE_SAMPLER_GRID      the reference's grid (default; bit for bit what this build always computed)
 *   NLE_SAMPLER_FARTHEST  farthest-point selection in the affinity's own metric, same count p as the grid would take:
 *     D(i, j) = (1/hx^2) (double)(dr^2 + dc^2) + (1/hy^2) dy^2   (dr dc integer, dy = (double)y_i - (double)y_j, no fma)
 *     s_0 = pixel (H/2, W/2); then p - 1 times the pixel whose smallest D to the samples chosen so far is largest (ties
 *     to the smallest row-major index).  The set is used in ascending row-major order (the reference's [selected; rest]).
 * It always uses the single-value, luminance-only distance above, also with a patch radius R > 0 or with chroma planes
 * set (which then apply to the affinities only).  Farthest applies to nle_train* and nle_compute_kernel64, in NLE_MODE_AUTO (which takes NLE_MODE_MATERIALISED_F64,
 * or NLE_MODE_STREAMED_F64 by the memory rule), NLE_MODE_MATERIALISED_F64 and NLE_MODE_STREAMED_F64; the other modes, slab
 * input at world > 1, nle_compute_kernel and nle_nystrom return NLE_ERR_INVALID.  At world > 1 (full-plane input) rank 0
 * selects and the set reaches the other ranks through the fp64 all-reduce.
 *   NLE_SAMPLER_RESIDUAL  residual-greedy selection: Cholesky with diagonal pivoting on the N x N affinity, same count p as
 *     the grid would take, p <= 2048.  Every sample is the pixel the samples so far explain worst (the largest Nystrom
 *     residual r_i = 1 - k_i^T K_A^-1 k_i of nle_nystrom_residual), every pivot is that residual:
 *       K(i, j) = exp(-(1/hx^2) (double)(dr^2 + dc^2) - (1/hy^2) dy^2)   (dr dc integer, dy = (double)y_i - (double)y_j,
 *                 single luminance values, libm exp, every operation rounded on its own: no fma)
 *       d_i = 1 for all i;  s_0 = pixel (H/2, W/2)
 *       round k:  l_k[i] = (K(i, s_k) - sum_{j<k} l_j[i] l_j[s_k]) / sqrt(d_{s_k})   (j ascending, one accumulator, no fma)
 *                 d_i -= l_k[i]^2
 *                 s_{k+1} = argmax over the pixels not chosen of d_i, ties to the smallest row-major index
 *     while that maximum is >= NLE_EPS (a smaller pivot would put an eigenvalue below the train's own cut into K_A).  From
 *     the first round whose maximum is below NLE_EPS on, every remaining sample is NLE_SAMPLER_FARTHEST's step: with m_i the
 *     smallest D(i, s) over ALL samples chosen so far (-1 for a chosen pixel; kept from round 0), the next sample is argmax
 *     m, ties to the smallest index; once fallen back the rule stays there (no further columns, d is left as it is).  The
 *     set is used ascending.  Like farthest it keeps this single-value K with a patch radius or chroma planes set, runs
 *     where farthest runs and is refused where farthest is; NLE_MODE_EXACT_F64 refuses both.  The factor (N rounded up to
 *     even, times p, doubles: nle_residual_sampler_bytes) is held in device memory: a selection that does not fit returns
 *     NLE_ERR_INVALID with the bytes needed, before anything runs.
 * The value 2 is unused (and refused). */
#define NLE_SAMPLER_GRID 0
#define NLE_SAMPLER_FARTHEST 1
#define NLE_SAMPLER_RESIDUAL 3
int nle_ctx_set_sampler(nle_ctx* ctx, int sampler);
/* The sample set the ctx's sampler takes on the FULL H x W plane d_lum (fp32; may be NULL for the grid): *p samples, their
 * row-major indices ascending in h_idx (room for nle_sample_grid's n_sel_rows * n_sel_cols; may be NULL to learn *p).  A
 * collective at world > 1 under NLE_SAMPLER_FARTHEST and NLE_SAMPLER_RESIDUAL. */
int nle_sample_pixels(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, double hx,
                      double hy, long long* h_idx, int* p);
/* Device bytes NLE_SAMPLER_RESIDUAL's factor takes on an H x W plane with this sample grid: ((H W + 1) & ~1) * p * 8, p the
 * grid's sample count; -1 for arguments nle_sample_grid refuses.  Host only, no ctx. */
long long nle_residual_sampler_bytes(int H, int W, int n_row_samples, int n_col_samples);
/* NLE_SAMPLER_RESIDUAL's selection with its order and pivots (NLE_ERR_INVALID under the other samplers, and at world > 1
 * before any collective).  h_order (p): the samples in the order chosen.  h_pivot[k]: d of s_k when it was chosen (1 for
 * k = 0) for k < *n_residual; for later k the farthest-point m of s_k when it was chosen.  *n_residual: how many samples the
 * residual rule chose, s_0 included.  h_stats (3, may be NULL): {the largest d over the pixels not chosen (0 if there is
 * none), its first index (-1 if none), sum_i max(d_i, 0)} after the last residual round, folded from per-workgroup
 * partials in a fixed order.  With *n_residual == *p these are max r and the trace-norm error sum r of nle_nystrom_residual
 * for the set returned; after a fallback they are upper bounds of them (more samples only lower r).  Two calls give the
 * same bits. */
int nle_sample_pixels_order(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, double hx,
                            double hy, long long* h_order, double* h_pivot, int* p, int* n_residual, double* h_stats);
/* The Nystrom-extension GEMM Phi = K_AB^T (V_A Lambda^-1) (src/filter.cpp:275) of NLE_MODE_MATERIALISED and of nle_nystrom on
 * the bf16 matrix cores with SPLIT operands (each fp32 value as three bf16, six products, fp32 accumulate: fp32 accuracy at
 * ~2.7x the exact-fp32 MFMA's rate; plain bf16 operands miss the parity bar).  Off by default. */
int nle_ctx_set_nystrom_bf16x3(nle_ctx* ctx, int on);
/* Reuse of training's work in apply (default formulation on one rank, level-sorted rows; on by default).  A train leaves the
 * reduce half of apply for the plane it trained on, computed behind its Gram kernels, and the plane in one byte per pixel; an
 * apply whose input equals that plane bit for bit (compared by content on the device, never by pointer) takes it over instead
 * of computing its own.  Outputs are the same bits either way.  on == 0: trains on this ctx leave nothing (one byte per pixel
 * and ~3 % of a train saved for a caller who filters other planes only) and applies on it compute their own whatever the
 * filter holds. */
int nle_ctx_set_train_reduce(nle_ctx* ctx, int on);

/* Slab input (multi-GPU, SURVEY.md section 8e "each GPU uploads / downloads only its slab"): with on != 0 every plane
 * handed to nle_train*, nle_apply* on this ctx holds ONLY the rows [row0, row1) of this rank (nle_slab_rows), n_local
 * values, instead of the full H x W image; H and W stay the full image's.  The p sample values (and x at the sample
 * pixels in apply) are then completed across the ranks by one small all-reduce each.  Set it after the shard /
 * communicator; it has no effect at world == 1. */
int nle_ctx_set_slab_input(nle_ctx* ctx, int on);

/* How orthogonalize finds the top eigenpairs of Q (src/filter.cpp:310-317).  0 (default): the reference's default build,
 * eigenDecomposition(Q) -- a full eigensolve, the first min(nEigenVectors, kept) pairs.  1 (opt-in; also
 * NLE_Q_SOLVER=lanczos in the environment): the reference's USE_SPECTRA build, topkEigenDecomposition (:170-199) --
 * Lanczos for the nev = min(nEigenVectors, q - 1) pairs of largest magnitude, Krylov dimension min(2 nev, q), tolerance
 * 1e-10, at most 1000 restarts, the FULL (not triangle-mirrored) Q, converged pairs only.  Results agree with the
 * full solver to the tolerance; K' is capped at q - 1. */
int nle_ctx_set_topk_solver(nle_ctx* ctx, int solver);

/* Multi-GPU (one process per GPU).  Rank `rank` of `world` owns image rows
 * [rank*H/world, (rank+1)*H/world).  `allreduce(user, d_buf, count)` must sum, in place
 * and stream-ordered with the ctx's stream, `count` doubles at DEVICE pointer d_buf over
 * all ranks (torch.distributed / RCCL all_reduce on that stream).  `d_comm` is a device
 * buffer of `comm_len` doubles owned by the caller, comm_len >= nle_comm_len(p).
 * world == 1 (default) needs no callback.  New in this build (the reference is
 * single-process). */
/* Native form (preferred): the library calls RCCL itself -- ncclAllReduce, fp64 sum, IN PLACE on the ctx's stream, no
 * staging copies and no host callback.  librccl.so is loaded on first use.  One process per GPU: rank 0 obtains an id
 * with nle_rccl_unique_id and hands the 128 bytes to the other ranks by whatever channel the launcher has (an MPI /
 * torch.distributed broadcast, a file); every rank then calls nle_ctx_init_rccl (collective: ncclCommInitRank).  A host
 * that already owns a communicator for the ctx's device passes it to nle_ctx_set_rccl_comm instead (borrowed). */
#define NLE_RCCL_UNIQUE_ID_BYTES 128
int nle_rccl_unique_id(void* h_id, size_t size);
int nle_ctx_init_rccl(nle_ctx* ctx, int rank, int world, const void* h_id, size_t size);
int nle_ctx_set_rccl_comm(nle_ctx* ctx, int rank, int world, void* nccl_comm);
/* Error path of a multi-rank host: aborts the ctx's own communicator (ncclCommAbort) so that collectives of this ctx that
 * are waiting for a rank that has failed end instead of blocking for ever; callable from another thread than the one using
 * the ctx.  Afterwards every call on the ctx that needs a collective returns NLE_ERR_COMM until nle_ctx_init_rccl binds a
 * new communicator.  No-op without an own communicator. */
int nle_ctx_abort_rccl(nle_ctx* ctx);
/* Callback form (any transport, e.g. gloo in the CPU rehearsal tests): */
typedef int (*nle_allreduce_fn)(void* user, void* d_buf, size_t count);
int nle_ctx_set_shard(nle_ctx* ctx, int rank, int world, nle_allreduce_fn allreduce,
                      void* user, double* d_comm, size_t comm_len);
size_t nle_comm_len(int n_samples);

/* ---- host-only helpers (no GPU needed) ----------------------------------------- */
/* samplePixels, src/filter.cpp:56-80, in closed form: the selected set is
 * {row_off + i*row_step, i < n_sel_rows} x {col_off + j*col_step, j < n_sel_cols}. */
int nle_sample_grid(int H, int W, int n_row_samples, int n_col_samples, int* row_step,
                    int* row_off, int* n_sel_rows, int* col_step, int* col_off,
                    int* n_sel_cols);
/* rows [*row0, *row1) owned by `rank` of `world` */
int nle_slab_rows(int H, int rank, int world, int* row0, int* row1);
/* eigenDecomposition, src/filter.cpp:204-228 (decl include/filter.hpp:23-24): symmetric
 * n x n (col-major, LOWER triangle read), eigenvalues DESCENDING, leading run >= eps kept.
 * h_U: n x n col-major (first *r columns valid), h_D: n (first *r valid). */
int nle_eigen_decomposition(const double* h_M, int n, double eps, double* h_U, double* h_D,
                            int* r);
/* the same when only the first kmax eigenvectors are wanted (orthogonalize keeps nEigVectors columns of Q's, :313-316):
 * h_D receives ALL n eigenvalues (descending), h_U (n x min(kmax, n)) the first min(kmax, n) eigenvectors, *r the length
 * of the leading run >= eps.  For kmax <= n / 2 the eigenvectors come from inverse iteration on the tridiagonal form. */
int nle_eigen_decomposition_top(const double* h_M, int n, double eps, int kmax, double* h_U, double* h_D, int* r);
/* the form the train path itself uses for Q on the host: h_Dk receives only the min(kmax, n) LARGEST eigenvalues (descending),
 * h_U (n x min(kmax, n)) their eigenvectors, *r the number of eigenvalues >= eps -- all orthogonalize reads of Q's
 * decomposition (:313-316).  For 2 kmax <= n the eigenvalues come from bisection on Sturm counts of the tridiagonal form
 * (the count at eps is *r) instead of a QL run for all n; otherwise this is nle_eigen_decomposition_top. */
int nle_eigen_decomposition_topk(const double* h_M, int n, double eps, int kmax, double* h_U, double* h_Dk, int* r);
/* the same with the Householder reduction to tridiagonal form on the GPU (one workgroup, the matrix in registers; n <= 224)
 * and the O(n^2) rest on the host -- what nle_train* uses for Q when K <= q / 2 and q <= 224 (NLE_HOST_TRIDIAG=1 keeps
 * the whole solve on the host).  Same conventions; results agree with the host form to rounding. */
int nle_eigen_decomposition_top_device(nle_ctx* ctx, const double* h_M, int n, double eps, int kmax, double* h_U, double* h_D,
                                       int* r);
/* eigenDecomposition (:204-228) with the O(n^3) part on the GPU, 3 <= n <= 1152: Householder reduction in one persistent
 * multi-workgroup launch, all eigenvalues by Sturm bisection, the eigenvectors of h_D[first .. first + count) by inverse
 * iteration on the tridiagonal form (host) and their back-transformation (device).  h_D: all n eigenvalues descending;
 * h_U: n x count col-major (may be NULL when count == 0); *r = length of the leading run >= eps.  What nle_train* uses
 * for Wa and Q from 288 samples on (NLE_DEV_SOLVER_MIN; NLE_HOST_SOLVER=1 keeps the host solver). */
int nle_sym_eigen_device(nle_ctx* ctx, const double* h_M, int n, double eps, int first, int count, double* h_U, double* h_D,
                         int* r);
/* Cholesky factor of a symmetric matrix (lower triangle read) and its inverse on the GPU (blocked, fp64 MFMA updates):
 * h_L, h_Linv n x n col-major lower triangular, *inv_trace = trace(M^-1), *ok = 0 if a pivot was not positive. */
int nle_cholesky_device(nle_ctx* ctx, const double* h_M, int n, double* h_L, double* h_Linv, double* inv_trace, int* ok);
/* topkEigenDecomposition, src/filter.cpp:170-199 (the USE_SPECTRA build's solver for Q): the min(n_largest, n - 1)
 * eigenpairs of largest magnitude of the FULL n x n matrix by Lanczos (tolerance 1e-10, <= 1000 restarts), algebraic
 * value descending, leading run >= eps kept.  h_U: n x min(n_largest, n - 1) col-major, h_D likewise; *r valid pairs. */
int nle_topk_eigen_decomposition(const double* h_M, int n, int n_largest, double eps, double* h_U, double* h_D, int* r);
/* transformEigenValues, src/filter.cpp:334-347 */
int nle_transform_eigenvalues(const double* h_eigvals, int K, const double* h_weights, int L,
                              double* h_fS);
/* per-layer spectral responses implied by :334-347: h_resp[l*K + k] */
int nle_layer_responses(const double* h_eigvals, int K, int L, double* h_resp);

/* ---- stage-level entry points (unit parity; all sizes generic) ------------------- */
/* computeKernel, src/filter.cpp:114-167 (decl include/filter.hpp:20-21), for this rank's
 * slab.  d_lum: FULL H x W luminance plane (fp32).  Outputs: h_Ka (p x p col-major fp64,
 * may be NULL), d_kab: n_local x ld fp32 affinity rows k_i[s] = exp(negDist(pixel i,
 * sample s)) for EVERY local pixel in natural order (sample pixels included: their rows
 * are rows of Ka).  ld = nle_ld(p).  The permutation `P` (:156-164) is implicit:
 * nle_sample_grid gives it in closed form. */
int nle_compute_kernel(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples,
                       int n_col_samples, double hx, double hy, double* h_Ka, float* d_kab);
/* nystromApproximation, src/filter.cpp:257-280 (decl include/filter.hpp:26-27), fused with
 * the affinity evaluation (K_AB is never written): h_eigvals[r], d_phi n_local x nle_ld(r)
 * (allocated by the caller for r = p, i.e. n_local * nle_ld(p) floats). */
int nle_nystrom(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples,
                int n_col_samples, double hx, double hy, double* h_eigvals, int* r,
                float* d_phi);
/* Leading dimension of the fp32 device matrices below (d_A / lda of nle_ts_gemm; d_phi / ld of nle_sinkhorn_scalings,
 * nle_gram, nle_row_scalings).  The kernels read whole rows, one float4 at a time, padding columns included, so
 *   - the row stride must be a multiple of 4 and >= the logical width, the base pointer 16-byte aligned (nle_ld(width) and
 *     a fresh device allocation are both): any other stride returns NLE_ERR_INVALID before anything is launched;
 *   - the columns from the logical width up to the stride must hold ZEROS, as every matrix this library writes (d_kab,
 *     d_phi, d_C) does.  They enter the sums with a zero weight: a NaN or an Inf there makes the result non-finite, no
 *     other value is promised to be harmless.  Nothing is ever read beyond M rows of the stride;
 *   - nle_sinkhorn_scalings and nle_row_scalings take a stride of at most 2048 floats (more returns an error with
 *     nle_last_error set), nle_gram what 136 * ld bytes of LDS allow.
 * The fp64 entry points further down take any stride and never read the padding.
 *
 * Generic tall-skinny product of :275 for caller-supplied matrices:
 * d_C (M x nle_ld(nc)) = d_A (M x lda, logical width kd) * h_B (kd x nc col-major fp64). */
int nle_ts_gemm(nle_ctx* ctx, const float* d_A, long long M, int lda, int kd,
                const double* h_B, int nc, float* d_C);
/* sinkhorn iterations, src/filter.cpp:238-245 (decl include/filter.hpp:29-30), on a
 * device-resident phi (M x ld, logical width r): returns the two r-vectors
 * u_c = lambda o Phi^T r_{T-1}, u_r = lambda o Phi^T c_T that define the final scalings
 * c_i = recip(phi_i . u_c), r_i = recip(phi_i . u_r).  max_iter >= 1. */
int nle_sinkhorn_scalings(nle_ctx* ctx, const float* d_phi, long long M, int ld, int r,
                          const double* h_eigvals, int max_iter, double* h_u_c,
                          double* h_u_r);
/* Gram matrix of the scaled rows, the N-sized half of `Wab*Wab^T` (src/filter.cpp:296):
 * h_G (r x r col-major) = sum_i c_i^2 phi_i phi_i^T, c_i = recip(phi_i . h_u) (all rows);
 * h_u == NULL: c_i = 1 (plain X^T X, used for `Wab*Wab^T` on a caller-supplied Wab). */
int nle_gram(nle_ctx* ctx, const float* d_phi, long long M, int ld, int r, const double* h_u,
             double* h_G);
/* per-row scalings c_i = recip(phi_i . h_u) (inplaceReciprocal, src/filter.cpp:42-54) */
int nle_row_scalings(nle_ctx* ctx, const float* d_phi, long long M, int ld, int r,
                     const double* h_u, double* d_out);

/* The same stages on fp64 device matrices (row-per-pixel, leading dimension any value >= the logical width; outputs use
 * nle_ld(width)), all products and sums in fp64: what include/nle/filter.hpp's free functions run on, so that the
 * reference's unit tests (test/test_filter.cpp, tolerance 1e-10) hold at their own tolerance.  The leading dimension is a
 * row stride only: columns >= the logical width are never read, whatever they hold (a sub-block of a wider matrix, an
 * uninitialised buffer, NaN); nle_sinkhorn_scalings64 takes r <= 2048 (any ld), more returns NLE_ERR_INVALID. */
int nle_compute_kernel64(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, double hx,
                         double hy, double* h_Ka, double* d_kab);
/* The Nystrom residual map (new in this build): where the samples fail to explain a pixel.  For pixel i of the FULL H x W plane
 * with fp64 affinity row k_i (p entries, exactly what nle_compute_kernel64 writes under the ctx's patch radius, chroma planes
 * and sampler, with the same refusals) and K_A the samples' own affinities:
 *   r_i = K_ii - k_i^T pinv(K_A) k_i = 1 - sum_{k kept} (v_k^T k_i)^2 / lambda_k
 * pinv at the reference's cut: the leading run of eigenvalues >= NLE_EPS (src/filter.cpp:213-215,262-271).  In the reference's
 * terms r_i = 1 - sum_k lambda_k phi_ik^2 with (lambda, phi) of nystromApproximation: the diagonal of K - K~ for exactly the
 * extension a train uses.  K - K~ is positive semi-definite, so r_i is in [0, 1] up to rounding, |K_ij - K~_ij| <=
 * sqrt(r_i r_j), and sum_i r_i is the trace-norm error of the extension.  It is computed as 1 - || F^T k_i ||^2 with F F^T =
 * pinv(K_A): F = V diag(1 / sqrt(lambda)), or L^-T where K_A is certified full rank at the cut and factored by Cholesky, as the
 * default train factors it (both are legitimate; they differ by rounding).
 *   d_r        H W floats or NULL: d_r[i] = (float)r_i in natural pixel order, sample pixels included (the same formula),
 *              not clamped (a few ulp below 0 can occur)
 *   h_summary  [0] sum_i r_i, [1] max_i r_i, [2] row-major index of the first maximum, [3] number of pixels with r_i > thresh
 *              -- all from the unrounded fp64 r_i, block partials folded in a fixed order: two runs agree bit for bit in map
 *              and summary
 *   form       NLE_RESID_ROWS   explicit fp64 affinity rows chunk by chunk (NLE_STREAM64_CHUNK_MB), any option, p <= 2048;
 *                               the result does not depend on the chunk size
 *              NLE_RESID_FUSED  the affinities are generated in fp64 inside the fp64-MFMA kernel, nothing N x p is stored:
 *                               patch radius 0, no chroma planes, NLE_SAMPLER_GRID, p <= 256
 *              NLE_RESID_AUTO   FUSED where it applies, else ROWS
 * NLE_ERR_INVALID with a message, nothing enqueued and the ctx left usable: world > 1 (before any collective), a NULL plane or
 * summary, thresh not finite, an unknown form, p > 2048, NLE_RESID_FUSED where it does not apply, hx or hy not > 0, and
 * whatever nle_compute_kernel64 refuses. */
#define NLE_RESID_AUTO 0
#define NLE_RESID_ROWS 1
#define NLE_RESID_FUSED 2
int nle_nystrom_residual(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, double hx,
                         double hy, int form, double thresh, float* d_r, double* h_summary);
int nle_ts_gemm64(nle_ctx* ctx, const double* d_A, long long M, int lda, int kd, const double* h_B, int nc, double* d_C);
int nle_sinkhorn_scalings64(nle_ctx* ctx, const double* d_phi, long long M, int ld, int r, const double* h_eigvals,
                            int max_iter, double* h_u_c, double* h_u_r);
int nle_gram64(nle_ctx* ctx, const double* d_phi, long long M, int ld, int r, const double* h_u, double* h_G);
int nle_row_scalings64(nle_ctx* ctx, const double* d_phi, long long M, int ld, int r, const double* h_u, double* d_out);
/* The sample-space stages (csrc/fused.hip), each alone: the launchers NLE_MODE_PHI_FREE_EXP, the table formulation's Sinkhorn
 * update and V on demand call, with nothing around them.  d_lum: the FULL H x W plane (fp32); the sample grid and hx, hy as
 * in nle_compute_kernel (the plain fp32 affinity: none of the ctx's affinity options).  Rows [row0, row1) are the local slab,
 * 0 <= row0 < row1 <= H: M = (row1 - row0) W pixels from pixel row0 W on; coordinates stay global, the indices of d_y, d_c
 * and d_V are local.  Every call returns with the stream drained.  NLE_ERR_INVALID with nle_last_error set for what a
 * launcher has no kernel for: more than 256 samples (pass, Gram), K > 128 or more than 32 x 36 samples (projection).
 *
 * nle_sample_pass: one Sinkhorn half-iteration, z[s] = sum over the NON-sample local pixels of k_i[s] y_i with y_i = 1
 *   (recip == 0) or recip(k_i . h_w) (k_sink_pass + k_reduce_partials, the slices added in order).  h_w: p doubles (NULL:
 *   zeros), d_y: M doubles or NULL (y_i, 0 at the sample pixels), h_z: p doubles.
 * nle_sample_gram: h_G (p x p, symmetric) = sum over the non-sample local pixels of d_c[i]^2 k_i k_i^T (k_gram64 +
 *   k_gram64_reduce); d_c at a sample pixel is not read.
 * nle_sample_project: d_V (M x ldv fp32, K <= ldv <= 16 ceil(K / 16)) = diag(d_c) K_rows h_D, h_D p x K ROW-major, for every
 *   local pixel, the sample pixels included (k_project64 / k_project64_res; no exact sample rows are scattered).  Columns
 *   [K, ldv) come out zero.
 * nle_sample_update: the p-sized update between two passes (k_sink_update_a/b, eps = NLE_EPS) on host operands: h_X1 2p x r
 *   column-major, h_X2 2p x r row-major, h_lam r, h_z zrows x zld (zld >= p) slices of z, h_sA the p sample row sums the
 *   pass used (recip != 0; ignored and may be NULL for the column sum).  Out: h_v = [z; y_A] (2p), h_u (r), h_sA_next (p),
 *   h_w_next (p). */
int nle_sample_pass(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, double hx, double hy,
                    int row0, int row1, int recip, const double* h_w, double* d_y, double* h_z);
int nle_sample_gram(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, double hx, double hy,
                    int row0, int row1, const double* d_c, double* h_G);
int nle_sample_project(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, double hx,
                       double hy, int row0, int row1, const double* h_D, int K, const double* d_c, float* d_V, int ldv);
int nle_sample_update(nle_ctx* ctx, int p, int r, int chol, int recip, const double* h_X1, const double* h_X2,
                      const double* h_lam, const double* h_z, int zrows, int zld, const double* h_sA, double* h_v, double* h_u,
                      double* h_sA_next, double* h_w_next);
/* The table path's stages (csrc/tables.hip), each alone: the launchers the default train and apply call (check_levels,
 * hist_tables, sink_hist_tiled, apply_hist_layers, gram_hist, apply_small, scatter_samples), with nothing around them and no
 * launch geometry of their own.  d_lum: the FULL H x W plane (fp32, integer valued in [0, 255]); rows [row0, row1) are the local
 * slab, 0 <= row0 < row1 <= H, nrows = row1 - row0: coordinates stay global, d_cvec, d_y and the outputs are indexed locally.
 * nR x nC = the realised sample grid (nle_sample_grid), p = nR nC, ldp = 64 ceil(p / 64).  The tables come one of two ways:
 *   supplied  d_er (nrows x nR), d_ecT (nC x W) and d_Ep (256 x p) are the caller's, on the device (hx, hy are not read): the
 *             pixel kernels are the LDS-atomic ones and all 16 level tiles are made -- what the library runs on planes wider than
 *             its level-sorted rows take
 *   built     d_er = d_ecT = d_Ep = NULL: the tables, the level-sorted rows, the range of level tiles that occur and the kernel
 *             forms the bandwidth allows, made from the plane, hx and hy exactly as training makes them
 * d_cvec: nrows W row scalings, may be NULL where no kernel reads them (the column-sum and reciprocal passes).  Whatever it
 * holds at a sample pixel, a NaN included, is never used.  The expand half writes 0 at the sample pixels of d_out on a
 * supplied view; on a built view with level-sorted rows it leaves them to nle_table_scatter (their content is unspecified).
 * Before the launch every workspace and every output is filled with NaN (all bytes 0xff): an element no kernel wrote still
 * holds it.  Every call returns with the stream drained.
 * NLE_ERR_INVALID with nle_last_error set, before any launch, for what the launchers have no kernel for: nR > 32, nC > 36,
 * K > 128, more layers than one launch takes; and for a plane that is not integer valued in [0, 255] (a built view: the whole
 * plane; a supplied view: the local rows, checked with check_levels first).
 *
 * nle_table_workspace: doubles of workspace of nle_table_pass (gram == 0) or nle_table_gram (gram != 0) for nrows local rows;
 *   -1 for a grid beyond 32 x 36.  Host only.
 * nle_table_levels: check_levels over n floats at d_x (any 4-byte alignment): *h_bad != 0 when a value is not an integer in
 *   [0, 255] (NaN included), bit t of *h_mask set when a valid level in [16 t, 16 t + 16) occurs.
 * nle_table_build: what the view is.  h_info (5 ints): level-sorted rows made, first level tile, number of level tiles, the Gram
 *   runs on index sums, layers one expand launch takes.  d_er_out, d_ecT_out, d_Ep_out (optional): copies of the tables.
 * nle_table_pass: one half-iteration (sink_hist_tiled).  mode 0: y = 1; 1: y = recip(d), d_i = sum_b ec[c_i][b] g[r_i][x_i][b],
 *   g from d_w (p doubles); 2: y_i = d_cvec[i] d_xvec[i], d_xvec the full plane.  y = 0 at sample pixels.  d_y (optional):
 *   nrows W.  d_ws: ws_elems >= nle_table_workspace doubles, laid out g (nrows x nC x 256, mode 1 only), h (the same shape),
 *   then the (slab, level tile) partial rows of ldp doubles; d_z: ldp doubles, [p, ldp) come out zero.
 * nle_table_expand: the expand half of apply for nl layers (apply_hist_layers): the g tables of the weight vectors d_wl (nl
 *   vectors of stride ldw >= p) into d_gws (nl x nrows x nC x 256), then d_out[l ostride + i] = (float)(c_i sum_b ec g), with
 *   round8 != 0 clamped to [0, 255] and rounded half to even in fp64.  d_out: nl ostride floats.
 * nle_table_gram: d_Gk (p x p, symmetric) = sum over the non-sample local pixels of c_i^2 k_i k_i^T (gram_hist).  d_ws: pair
 *   form A (nrows x NP x 256, NP = nC (nC + 1) / 2), EE (nrows x ldm), C (splits x ldm x NP x 256); index sums (built views
 *   where the bandwidth allows) S (nrows x (2 nC - 1) x 256), F (nrows x ldm2), T (splits x ldm2 x (2 nC - 1) x 256).
 *   h_split (2 ints): the image rows per split and the number of splits of the GEMM, in the form the view takes.
 * nle_table_apply_small: the p- and K-sized middle of apply (k_apply_small), all operands on the device: t = D^T m + Vrows^T xA
 *   (K), W'[l] = D (resp_l o t) (stride ldw, [p, ldw) zero), YA[l] = Vrows (resp_l o t) (stride p).  D, Vrows: p x ldk
 *   row-major.  d_differs (optional): a device int; where it is 0, d_m_same and d_xA_same stand in for d_m and d_xA.
 * nle_table_scatter: d_Y[l ystride + d_loc[a]] = (float)YA[l][a] where d_loc[a] >= 0 (round8 as above); d_Y is otherwise kept. */
long long nle_table_workspace(int n_sel_rows, int n_sel_cols, int nrows, int gram);
int nle_table_levels(nle_ctx* ctx, const float* d_x, long long n, int* h_bad, unsigned* h_mask);
int nle_table_build(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, int row0, int row1,
                    double hx, double hy, const double* d_er, const double* d_ecT, const double* d_Ep, const double* d_cvec,
                    double* d_er_out, double* d_ecT_out, double* d_Ep_out, int* h_info);
int nle_table_pass(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, int row0, int row1,
                   double hx, double hy, const double* d_er, const double* d_ecT, const double* d_Ep, const double* d_cvec,
                   int mode, const double* d_w, const float* d_xvec, double* d_y, double* d_ws, long long ws_elems, double* d_z);
int nle_table_expand(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, int row0, int row1,
                     double hx, double hy, const double* d_er, const double* d_ecT, const double* d_Ep, const double* d_cvec,
                     const double* d_wl, int ldw, int nl, int round8, double* d_gws, float* d_out, long long ostride);
int nle_table_gram(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, int row0, int row1,
                   double hx, double hy, const double* d_er, const double* d_ecT, const double* d_Ep, const double* d_cvec,
                   double* d_ws, long long ws_elems, double* d_Gk, int* h_split);
int nle_table_apply_small(nle_ctx* ctx, int p, int K, int ldk, int L, int ldw, const double* d_m, const double* d_D,
                          const double* d_Vrows, const double* d_xA, const double* d_resp, double* d_t, double* d_Wp,
                          double* d_YA, const int* d_differs, const double* d_m_same, const double* d_xA_same);
int nle_table_scatter(nle_ctx* ctx, int p, int L, const long long* d_loc, const double* d_YA, float* d_Y, long long ystride,
                      int round8);
/* The small dense fp64 product of the p- and q-sized algebra (one launch, fp64 MFMA), all operands on the device:
 * C(i,j) = dl[i] (sum_k A(i,k) dk[k] B(k,j)) dr[j] + add(i,j) for i < m, j < n, k < kk, every matrix given by its pointer
 * and its (row stride, column stride) in doubles, so that transposes, sub-blocks and padded row- or column-major outputs
 * need no copy; d_dl (m), d_dk (kk), d_dr (n) and d_add (strides rs_add, cs_add) may each be NULL.  Only the m x n entries
 * of C are written.  d_add may be d_C with C's strides; C must not overlap A or B.  Sums run over k ascending in one
 * chain per entry, A(i,k) dk[k] rounded first.  nle_gemm64s_window() is the number of k whose operands one wave loads
 * in one go. */
int nle_gemm64s(nle_ctx* ctx, int m, int n, int kk, const double* d_A, long long rs_a, long long cs_a, const double* d_B,
                long long rs_b, long long cs_b, double* d_C, long long rs_c, long long cs_c, const double* d_dl,
                const double* d_dk, const double* d_dr, const double* d_add, long long rs_add, long long cs_add);
int nle_gemm64s_window(void);
/* The hot path of NLE_MODE_EXACT_F64: d_Y = K d_X with K the exact N x N affinity of the plane d_lum (definition above;
 * integer valued in [0, 255], N = H W <= NLE_EXACT_MAX_PIXELS), regenerated on the fly.  d_X, d_Y: N x ld fp64, row per
 * pixel, ld a multiple of 4, ncols <= ld logical columns; d_Y must not alias d_X; its columns >= ncols come out zero.
 * Deterministic (fixed summation order). */
int nle_affinity_product64(nle_ctx* ctx, const float* d_lum, int H, int W, double hx, double hy, const double* d_X, int ld,
                           int ncols, double* d_Y);

/* ---- the fused path ---------------------------------------------------------------- */
/* NLEFilter::trainFilter, src/filter.cpp:480-502.  d_lum: FULL H x W fp32 luminance on the
 * device.  The filter keeps V (n_local x ld(K') fp32, pixel order) and eigvals on the
 * device/host: the reference's m_eigvecs / m_eigvals (include/filter.hpp:52-53).
 * Errors: n_row_samples > H or n_col_samples > W -> NLE_ERR_INVALID with the reference's
 * message (:117-119). */
int nle_train(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples,
              int n_col_samples, double hx, double hy, int n_sinkhorn_iter,
              int n_eigen_vectors, nle_filter** out);
/* same, luminance plane in HOST memory (what NLEFilter::trainFilter is handed) */
int nle_train_host(nle_ctx* ctx, const float* h_lum, int H, int W, int n_row_samples,
                   int n_col_samples, double hx, double hy, int n_sinkhorn_iter,
                   int n_eigen_vectors, nle_filter** out);
/* same, from the 8-bit plane itself: what getLuminanceChannel (src/filter.cpp:460-469) hands trainFilter is the L channel of
 * an 8-bit Lab image converted to double -- h_lum8 holds those bytes (H x W, this rank's rows in slab-input mode), one byte
 * per pixel crosses PCIe instead of four and the device widens them.  The filter is the one nle_train_host builds from the
 * same levels as floats (bit-identical), and it keeps the plane likewise for nle_apply*_host(h_x == NULL). */
int nle_train_host_u8(nle_ctx* ctx, const unsigned char* h_lum8, int H, int W, int n_row_samples,
                      int n_col_samples, double hx, double hy, int n_sinkhorn_iter,
                      int n_eigen_vectors, nle_filter** out);
void nle_filter_destroy(nle_filter* f);
/* any out pointer may be NULL.  n_local = pixels of this rank's slab, K = kept eigenpairs
 * (K' of src/filter.cpp:314), r = retained rank of Ka, p = realised sample count. */
int nle_filter_info(const nle_filter* f, long long* n_local, int* K, int* r, int* p,
                    int* row0, int* row1);
/* What the last train decided, h_info[8]:
 *   [0] formulation of the N-sized passes that was taken (NLE_MODE_MATERIALISED, NLE_MODE_PHI_FREE = look-up
 *       tables, NLE_MODE_PHI_FREE_EXP) -- auto mode resolves to one of these per image;
 *   [1] p realised sample count;  [2] eigenvalues of Ka kept by the cut at 1e-10 (src/filter.cpp:214,262-271);
 *   [3] eigenvalues of Wa kept (:287);  [4] eigenvalues of Q kept (:313);  [5] K' = min(nEigenVectors, [4]) (:314);
 *   [6] 1 if Ka was factored by Cholesky (certified full rank at the cut), 0 if by the eigensolver;
 *   [7] the same for Wa's inverse root. */
int nle_filter_diag(const nle_filter* f, int* h_info);
int nle_filter_eigvals(const nle_filter* f, double* h_eigvals /* K */);
/* the filter's sample set: *p row-major pixel indices, ascending, in h_idx (may be NULL to learn *p) */
int nle_filter_sample_pixels(const nle_filter* f, long long* h_idx, int* p);
/* min / max coefficient of the first `ncols` eigenvectors over this rank's slab (what the reference
 * prints at src/filter.cpp:506): h_min[ncols], h_max[ncols].  A filter whose V is implicit projects just
 * these columns into a temporary; it does not materialise the N x K matrix. */
int nle_filter_eigvec_range(const nle_filter* f, int ncols, double* h_min, double* h_max);
/* device pointer + leading dimension of V (n_local x ld), for inspection.  In the table formulation
 * the filter keeps V implicit (V = diag(c) K D) and applies it on its p-sized side; the first call of
 * this / nle_filter_copy_eigvecs / nle_filter_eigvec_range materialises the matrix (one projection GEMM). */
int nle_filter_eigvecs(const nle_filter* f, const float** d_V, int* ld);
/* copy V (n_local x ld floats) into a caller-owned DEVICE buffer */
int nle_filter_copy_eigvecs(const nle_filter* f, float* d_out);
/* per-stage milliseconds of the last train: sample fetch + Ka eigensolve, sinkhorn (incl. building
 * Phi in the materialised mode), gram, project (HIP events); host algebra; wall total.  h_ms[6] */
int nle_filter_timings(const nle_filter* f, double* h_ms);

/* NLEFilter::apply, src/filter.cpp:445-458: y = V diag(fS) V^T x for this rank's slab.
 * d_x: FULL H x W fp32 channel on the device; d_y: n_local fp32.  Size mismatch with the
 * training image -> NLE_ERR_INVALID (:447-449). */
int nle_apply(nle_filter* f, const float* d_x, int H, int W, const double* h_fS, float* d_y);
/* the L per-layer outputs y_l = V ((lambda^l - lambda^(l+1)) o V^T x), base layer
 * lambda^(L-1) (src/filter.cpp:334-347); d_y: L x n_local fp32 (layer-major).  1 <= L <= 64 whatever K' is: L x K' is
 * not bounded (the layers go out a group per launch when their tables do not fit on chip together). */
int nle_apply_layers(nle_filter* f, const float* d_x, int H, int W, int L, float* d_y);
/* host-buffer forms.  h_x == NULL: filter the plane the filter was trained on (kept on the device by
 * nle_train_host), which is what `enhance` does (src/enhance.cpp:43-44) -- one upload for train + apply.  Finished
 * layers are copied back on a second stream while the next one is computed. */
int nle_apply_host(nle_filter* f, const float* h_x, int H, int W, const double* h_fS,
                   float* h_y);
int nle_apply_layers_host(nle_filter* f, const float* h_x, int H, int W, int L, float* h_y);
/* The L plane NLEFilter::enhance merges back (src/filter.cpp:428-436): y = apply(x, fS), cv::max(y, 0), cv::min(y, 255),
 * convertTo(CV_8U) (round half to even, saturate) -- n_local BYTES instead of L fp32 planes: what `enhance` needs back from
 * the device (16 MB instead of 268 MB at 4096^2, four weights).  Device and host-buffer forms; h_x == NULL as above. */
int nle_apply_u8(nle_filter* f, const float* d_x, int H, int W, const double* h_fS, unsigned char* d_out);
/* the same plane as fp32 holding the 8-bit levels (the replacement-channel argument of nle_lab2bgr8 / _planes).  On the
 * default path the clamp and the round-half-even act on the fp64 value of the filtered plane, before anything is rounded
 * to fp32: `enhance` then rounds as the reference's fp64 pipeline does, not an fp32 plane's ties. */
int nle_apply_rounded8(nle_filter* f, const float* d_x, int H, int W, const double* h_fS, float* d_y);
int nle_apply_u8_host(nle_filter* f, const float* h_x, int H, int W, const double* h_fS, unsigned char* h_out);

/* ---- region edits (new in this build: the reference edits with one global weight vector, src/filter.cpp:412-443) ---- */
/* Scribble on a few regions and give each its own layer weights.  A trained filter f has K' pairs (V, lambda) over N = H W
 * pixels.  Inputs: L layers, 1 <= L <= NLE_REGION_LAYERS_MAX; M regions, 1 <= M <= NLE_REGION_MAX; stroke planes s_1 .. s_M
 * (fp32, any finite values; the CLI gives 0 / 1); scales c_m (NULL: 1); the spread t > 0; the floor phi > 0; the weights
 * Wt[(M + 1)][L], fp64, row-major, row 0 the background and row m region m.
 *   Spread   q_m = nle_apply(f, s_m, fS) with fS[k] = c_m pow(lambda_k, t): label propagation V lambda^t V^T s_m on the
 *            affinity the filter was trained on, exactly the apply path of whatever formulation f was trained in; an fp32
 *            plane.  The scale rides in fS (no extra pass).
 *   Layers   Y_0 .. Y_{L-1} = nle_apply_layers(f, x, L), fp32 planes.
 *   Combine  pointwise, per pixel i, in fp64, every operation rounded on its own (no fma), sums in ascending m and l:
 *              u_m     = Q_m[i] > 0 ? (double)Q_m[i] : 0                       (a NaN q counts as 0)
 *              sigma   = u_1 + u_2 + .. + u_M ;   d = sigma > phi ? sigma : phi
 *              alpha_m = u_m / d ;   alpha_0 = 1 - sigma / d
 *              w_l     = alpha_0 Wt[0][l] + alpha_1 Wt[1][l] + .. + alpha_M Wt[M][l]
 *              y       = w_0 (double)Y_0[i] + .. + w_{L-1} (double)Y_{L-1}[i]
 *            The rule is continuous in q: where the strokes have little influence (sigma < phi) the pixel blends to the
 *            background row, elsewhere the memberships sum to 1.
 * Output kinds: NLE_REGION_OUT_F32 stores (float)y; NLE_REGION_OUT_ROUNDED8 stores rintf((float)y) saturated to [0, 255] as
 * fp32 (the rule of nle_apply_u8's last step; what nle_lab2bgr8 takes from nle_apply_rounded8); NLE_REGION_OUT_U8 stores
 * the same value as a byte.
 * The C++ surface and the CLI set c_m = N / sum_i s_m(i) (summed on the host in fp64): a spread stroke then has mean ~ 1
 * whatever its size and phi is dimensionless; their defaults are t = 4 and phi = 0.05. */
#define NLE_REGION_MAX 8
#define NLE_REGION_LAYERS_MAX 16
#define NLE_REGION_OUT_F32 0
#define NLE_REGION_OUT_ROUNDED8 1
#define NLE_REGION_OUT_U8 2
/* the stage call, the rule alone: d_layers L planes and d_q M planes of n fp32 values each, plane l at d_layers +
 * l layer_stride and plane m at d_q + m q_stride (strides in floats, >= n); h_weights (M + 1) x L; d_out n floats, or n
 * bytes for NLE_REGION_OUT_U8.  No alignment is required of pointers or strides. */
int nle_region_combine(nle_ctx* ctx, const float* d_layers, int L, const float* d_q, int M, long long n,
                       long long layer_stride, long long q_stride, const double* h_weights, double floor, int out_kind,
                       void* d_out);
/* the spreads: d_strokes M planes of H W fp32 values, plane-major; h_scale M doubles or NULL; d_q M planes likewise */
int nle_region_spread(nle_filter* f, const float* d_strokes, int M, int H, int W, const double* h_scale, double spread,
                      float* d_q);
/* nle_apply_layers + nle_region_spread + nle_region_combine with the L + M work planes in the ctx's workspace: bitwise what
 * the three calls give.  Works for every formulation nle_apply works for (it only composes them).  NLE_ERR_INVALID, with a
 * message and the ctx left usable, for M or L out of range, a spread or floor that is not finite and > 0, a scale that is not
 * finite, H W that is not the filter's, a NULL pointer (h_scale apart), an unknown out kind, and world > 1 (the combine is pixel-local, but slabs
 * and device groups are not built: refused before any collective). */
int nle_apply_regions(nle_filter* f, const float* d_x, int H, int W, int L, const float* d_strokes, int M,
                      const double* h_scale, double spread, double floor, const double* h_weights, int out_kind,
                      void* d_out);

/* ---- the out-of-span detail layer and the detail curve (new in this build: no reference, so this text and DESIGN.md
 * section 3.15 are the definition) ---- */
/* The layers of nle_apply_layers sum to V V^T x, not to x: what of the plane lies outside the span of the K' trained
 * eigenvectors belongs to no layer, and no layer weight brings it back.  Here that residual is one more weighted layer, and
 * the detail layers may pass a monotone gain curve that boosts (or cores) small amplitudes and leaves edges their size.
 * Per pixel i, in fp64, every operation rounded on its own (no fma), in the order written.  Inputs: the plane x; the layers
 * Y_0 .. Y_{L-1}, fp32, 1 <= L <= NLE_REGION_LAYERS_MAX; the weights w_0 .. w_{L-1}; the residual weight w_rho; the gain a;
 * the amplitude sigma.
 *   S    = ((Y_0 + Y_1) + ..) + Y_{L-1}
 *   rho  = x - S
 *   g(d) = d                                    if sigma == 0 or a == 1 (no exp is evaluated)
 *   g(d) = d (1 + (a - 1) exp(-(t t))),  t = d / sigma, otherwise      (a - 1 is formed once on the host)
 *   y    = w_rho g(rho) + w_0 g(Y_0) + .. + w_{L-2} g(Y_{L-2}) + w_{L-1} Y_{L-1}
 * The sum for y runs left to right.  The base layer Y_{L-1} is never remapped; for L = 1 the rule is y = w_rho g(rho) +
 * w_0 Y_0.
 * g has slope a at 0 and tends to d for |d| >> sigma: small amplitudes are boosted (a > 1) or cored (a < 1), edges keep their
 * size, so nothing clips and no halo appears.  g' = 1 + (a - 1) e^(-t^2) (1 - 2 t^2), whose second factor lies in [-0.4463, 1]
 * (minimum at t^2 = 3/2): g is strictly increasing for 0 < a < 3.24, non-decreasing at a = 0, and Lipschitz with the constant
 * max(a, 1.4463 - 0.4463 a).
 * Accepted: a finite in [0, 3]; sigma finite and >= 0, 0 meaning the curve is off; w_rho and the weights finite.
 * Output kinds: the three of nle_region_combine with its store rule ((float)y, then the saturating round for _ROUNDED8 / _U8).
 * Identity: with every weight 1, w_rho = 1 and the curve off, y = x up to a few fp64 ulp of sum |Y_l|; for an integer plane
 * (float)y == x exactly (at x = 0 that residue has no integer to round to: NLE_REGION_OUT_F32 stores it as it is, the other
 * two kinds store 0).  The sign of a zero level is not specified.
 * nle_detail_combine is the stage call, the rule alone, on any planes: d_x n floats, layer l at d_layers + l layer_stride
 * (stride in floats, >= n), h_weights L doubles, d_out n floats, or n bytes for NLE_REGION_OUT_U8.  No alignment is required
 * of pointers or strides; x and the layers are read once.
 * nle_apply_detail runs nle_apply_layers into the ctx's workspace and then the combine: bitwise what the two calls give, for
 * every formulation nle_apply_layers works for.
 * Both return NLE_ERR_INVALID with a message, enqueue nothing and leave the ctx usable for: L out of range, a NULL pointer,
 * a weight (w_rho included) that is not finite, a gain outside [0, 3] or not finite, a sigma that is negative or not finite,
 * an unknown out kind, d_out overlapping an input, n < 1 or a layer stride smaller than n (the stage call), H W that is not
 * the filter's and world > 1 (nle_apply_detail: slabs and device groups are not built for it, as for regions). */
#define NLE_DETAIL_GAIN_MAX 3
int nle_detail_combine(nle_ctx* ctx, const float* d_x, const float* d_layers, int L, long long n, long long layer_stride,
                       const double* h_weights, double w_rho, double gain, double sigma, int out_kind, void* d_out);
int nle_apply_detail(nle_filter* f, const float* d_x, int H, int W, int L, const double* h_weights, double w_rho, double gain,
                     double sigma, int out_kind, void* d_out);

/* ---- the base tone curve: shadows, highlights, auto levels, equalise (new in this build: no reference, so this text and
 * DESIGN.md section 3.18 are the definition) ---- */
/* The detail rule above never remaps the base layer.  Here its weighted value Bw = w_{L-1} Y_{L-1} passes a monotone curve,
 * piecewise linear through NLE_TONE_KNOTS = N + 1 knots over a range [lo, hi]; everything else of the detail rule stays.  All
 * arithmetic is fp64, every operation rounded on its own (no fma), in the order written.
 * nle_plane_histogram: the histogram of a scaled plane, n >= 1 floats at d_x.  Per pixel
 *   v = (double)x scale;  b = floor((v + 256) 4)
 *   a NaN v -> counts[4097];  b < 0 -> counts[0];  b >= 4096 -> counts[4097];  otherwise counts[1 + b]
 * NLE_TONE_BINS = 4096 bins of a quarter level over [-256, 768) between an underflow and an overflow counter.  h_counts is
 * long long[NLE_TONE_BINS + 2]; the counts are integers, so the result is exact and independent of the order of the pixels
 * and of the merges.  The call returns with the counts on the host.  No alignment is required of d_x.
 * nle_tone_curve (host only, no ctx; its message is nle_last_error(NULL)): h_curve is double[NLE_TONE_KNOTS + 2] and
 * receives [lo, hi, T_0 .. T_N].  s = shadows and h = highlights in [-1, 1], P = clip_percent, A = equalise in [0, 1].
 * h_counts may be NULL when P < 0 and A == 0.  n = the sum of all counts.
 *   levels  P < 0: lo = 0, hi = 255.  P in [0, 25]: need = P / 100 n; klo = the first bin k in 0 .. 4095 with
 *           counts[0] + sum_{j <= k} counts[1 + j] > need; khi = the last bin k with counts[4097] + sum_{j >= k} counts[1 + j]
 *           > need; lo = -256 + 0.25 klo, hi = -256 + 0.25 (khi + 1); where a bin does not exist or hi - lo < 1: lo = 0, hi = 255
 *   F(v)    the share of pixels below v, linear inside a bin: q = (v + 256) 4, k = min(floor(q), 4095), phi = q - k,
 *           F = ((counts[0] + sum_{j < k} counts[1 + j]) + phi counts[1 + k]) / n      (the integer sum is exact)
 *   E_k     = (F(lo + t_k (hi - lo)) - F(lo)) / (F(hi) - F(lo)),  t_k = k / N;  E_k = t_k where the denominator is 0
 *   m_k     = (1 - A) t_k + A E_k                     (A == 0: m_k = t_k, the counts are not read)
 *   C(t)    = (t + (s t)(u u)) - (h (t t)) u,  u = 1 - t
 *   T_k     = 255 C(m_k)
 * C(0) = 0, C(1) = 1, C is C1 with slope 1 + s at 0 and 1 + h at 1, and non-decreasing for every (s, h) of the square (the
 * slope reaches 0 only at its corners): T is non-decreasing.  |C - t| <= (4 / 27)(|s| + |h|): 0.1482, which is 37.8 levels,
 * for one of the two at +-1 and the other at 0.
 * nle_tone_combine: the stage call, nle_detail_combine with the base term replaced.  With S, rho and g exactly as stated
 * there and h_curve = [lo, hi, T_0 .. T_N]:
 *   Bw = w_{L-1} Y_{L-1}
 *   u  = (Bw - lo) ks,   ks = N / (hi - lo), formed once on the host
 *   j  = min(max((int)floor(u), 0), N - 1);   f = u - (double)j
 *   B' = T_j + f (T_{j+1} - T_j)              (f < 0 or f > 1 continues the end segments linearly)
 *   y  = w_rho g(rho) + w_0 g(Y_0) + .. + w_{L-2} g(Y_{L-2}) + B'
 * The sums run left to right; for L = 1 the rule is y = w_rho g(rho) + B'.  Output kinds and store rule: the three of
 * nle_region_combine.  A NaN Bw gives a NaN y: NaN in NLE_REGION_OUT_F32, 0 in the other two kinds.  The stage call always
 * applies the curve it is given, any finite knots over any finite lo < hi.
 * nle_apply_tone: nle_apply_layers into the ctx's workspace; the histogram of layer L - 1 with scale = w_{L-1}, only when
 * P >= 0 or A > 0; the curve; the combine -- bitwise what the four calls give.  The curve is INACTIVE when s == 0, h == 0,
 * P < 0 and A == 0: the call then is nle_apply_detail, bit for bit.  h_curve_out (may be NULL) receives the curve either way.
 * NLE_ERR_INVALID with a message, nothing enqueued and the ctx left usable: what nle_detail_combine / nle_apply_detail
 * refuse; n < 1, a NULL pointer or a scale that is not finite (the histogram); s, h, P or A out of range or not finite, P > 25,
 * NULL counts where they are needed, a negative count, counts that sum to 0 (the curve); lo, hi or a knot that is not finite,
 * hi - lo that is not > 0 (the stage combine). */
#define NLE_TONE_KNOTS 1025
#define NLE_TONE_BINS 4096
int nle_plane_histogram(nle_ctx* ctx, const float* d_x, long long n, double scale, long long* h_counts);
int nle_tone_curve(const long long* h_counts, double shadows, double highlights, double clip_percent, double equalise,
                   double* h_curve);
int nle_tone_combine(nle_ctx* ctx, const float* d_x, const float* d_layers, int L, long long n, long long layer_stride,
                     const double* h_weights, double w_rho, double gain, double sigma, const double* h_curve, int out_kind,
                     void* d_out);
int nle_apply_tone(nle_filter* f, const float* d_x, int H, int W, int L, const double* h_weights, double w_rho, double gain,
                   double sigma, double shadows, double highlights, double clip_percent, double equalise, int out_kind,
                   void* d_out, double* h_curve_out);

/* ---- automatic regions: kernel k-means on the trained affinity (new in this build: no reference, so this text and
 * DESIGN.md section 3.19 are the definition) ---- */
/* Proposes the regions a region edit needs, instead of hand-drawn stroke masks.  The eigenpairs (V, lambda) of a trained
 * filter define the diffusion affinity G = V lambda^t V^T that nle_region_spread spreads strokes with; clustering the pixels
 * by G is spectral segmentation.  V is never materialised on the default path, and kernel k-means does not need it: one
 * iteration needs G applied to the C indicator planes of the current labels, which is one nle_region_spread.
 * Inputs: a trained filter f over N = H W pixels; C clusters, 1 <= C <= NLE_REGION_MAX; labels l_i in 0 .. C - 1, one byte
 * per pixel; the spread t > 0; a cap on the iterations, 1 .. NLE_SEGMENT_ITERATIONS_MAX.
 * One iteration, from labels l:
 *   Counts     n_c = #{i : l_i = c}.  A cluster with n_c = 0 is INACTIVE and stays empty for good.
 *   Spread     s_c = the 0 / 1 fp32 indicator plane of cluster c;  q = nle_region_spread(f, s, C, scale, t) with
 *              scale_c = N / n_c, and 0 for an inactive cluster -- bit for bit that call (the CLI's own stroke scaling: the
 *              spreads have mean ~ 1 and everything below is O(1)).
 *   Means      m_c = (sum_{i : l_i = c} (double)q_c[i]) / n_c in fp64, +inf for an inactive cluster.
 *   Reassign   per pixel, in fp64, every operation rounded on its own:  score_c = m_c - 2 (double)q_c[i];  a NaN score and
 *              an inactive cluster count as +inf;  l'_i = the smallest c with the smallest score;  where every score is
 *              +inf the pixel keeps l_i.  This is kernel k-means on G: N |psi_i - mu_c|^2 = score_c + a term that does not
 *              depend on c, with psi = V lambda^(t/2) and mu_c the mean of cluster c.
 *   Objective  J = ((n_0 m_0 + n_1 m_1) + ..) / N over the active clusters in ascending c, reported for the labels that
 *              ENTERED the iteration.  In exact arithmetic it never decreases.
 * Stop when an iteration changes no label, or after the cap.  Nothing is random anywhere.
 * Start (nle_segment_init): equal-population cuts of a plane x on the counts of nle_plane_histogram(x, scale = 1):
 *   cum(k) = counts[0] + sum_{j <= k} counts[1 + j];  b_c = the first bin k in 0 .. 4095 with cum(k) >= floor(N c / C) + 1,
 *   for c = 1 .. C - 1, 4096 where none exists;  l_i = #{c : bin(x_i) >= b_c} with bin(x) = floor((x + 256) 4) clamped to
 *   [-1, 4096] and a NaN taken as 4096.  Equal cuts give empty clusters: that is allowed and reported.
 * The stage calls, each the rule alone on any planes.  Plane c of d_q lies at d_q + c q_stride (stride in floats, >= n); no
 * alignment is required of any pointer or stride; each returns with its results on the host.
 *   nle_segment_init    h_cuts (may be NULL) receives b_1 .. b_{C-1}; d_labels n bytes.
 *   nle_segment_stats   h_counts[c] = n_c and h_sums[c] = the fp64 sum of q_c over the members of c, every pixel reading
 *                       the one value q_{l_i}[i].  The sums go through per-workgroup partials on a grid that depends on n
 *                       alone and are folded in a fixed order: two calls on the same buffers give the same bits.  The
 *                       order inside a workgroup depends on the placement: with d_q 16-byte aligned, q_stride a multiple
 *                       of 4 and d_labels 4-byte aligned, four aligned pixels that share a label enter as ((a + b) + c) + d,
 *                       added once; otherwise pixel by pixel -- the sums of two placements may differ in their last bits
 *                       (both within n_c 2^-52 sum |q| of the exact sum).  q_stride = 0 is legal: all
 *                       planes are then one plane and the sums are its per-cluster sums.  A label >= C is refused after
 *                       the pass (counted with an integer atomic, never used as an index).
 *   nle_segment_assign  h_m: the C values m_c, +inf for an inactive cluster.  d_labels is read and rewritten;
 *                       d_indicators (may be NULL) receives the C indicator planes of the new labels, plane c at
 *                       d_indicators + c ind_stride; h_counts the new n_c; h_changed the number of labels that changed
 *                       (integer atomics: exact, independent of the order).  A label >= C is refused after the pass:
 *                       such a pixel is left as it is and belongs to no indicator plane.  The planes, the labels and the
 *                       indicator planes must not overlap.
 * nle_filter_segment runs the loop from the labels at d_labels with the work planes in the ctx's workspace: bit for bit
 * the composition of nle_region_spread, nle_segment_stats, the division m_c = sum_c / n_c and nle_segment_assign on planes
 * placed as its own are -- 16-byte aligned, n floats apart -- and on the caller's d_labels (see nle_segment_stats on
 * placements), with one small download per iteration.  d_labels receives the result, h_counts its C counts, h_objective[0 .. iters) the
 * objective of every iteration made (the rest is not written), *h_iters their number, *h_converged 1 when the last one
 * changed no label.  d_q (may be NULL) receives the C spreads of the RETURNED labels, plane c at d_q + c q_stride: the last
 * iteration's when it changed nothing, otherwise one more spread is made.  They are the membership planes
 * nle_region_combine takes.  Works for every formulation nle_apply_planes works for.
 * NLE_ERR_INVALID with a message, nothing enqueued and the ctx left usable: C out of range, n < 1, a stride smaller than n
 * (q_stride = 0 apart, in the two stage calls), a NULL pointer (h_cuts, d_indicators and d_q apart), overlapping buffers; for
 * nle_filter_segment also a spread that is not finite and > 0, max_iter out of range, H W that is not the filter's and
 * world > 1 (slabs and device groups are not built; refused before any collective). */
#define NLE_SEGMENT_ITERATIONS_MAX 200
int nle_segment_init(nle_ctx* ctx, const float* d_x, long long n, int C, unsigned char* d_labels, int* h_cuts);
int nle_segment_stats(nle_ctx* ctx, const float* d_q, int C, long long n, long long q_stride, const unsigned char* d_labels,
                      long long* h_counts, double* h_sums);
int nle_segment_assign(nle_ctx* ctx, const float* d_q, int C, long long n, long long q_stride, const double* h_m,
                       unsigned char* d_labels, float* d_indicators, long long ind_stride, long long* h_counts,
                       long long* h_changed);
int nle_filter_segment(nle_filter* f, int H, int W, int C, double spread, int max_iter, unsigned char* d_labels, float* d_q,
                       long long q_stride, long long* h_counts, double* h_objective, int* h_iters, int* h_converged);

/* ---- local adjustments: per-region detail, tone and saturation (new in this build: no reference, so this text and
 * DESIGN.md section 3.20 are the definition) ---- */
/* Every region gets the whole edit of its own -- layer weights, residual weight, detail curve, base tone curve, saturation --
 * and the memberships of the region edits blend the results.  All arithmetic is per pixel i, in fp64, every operation rounded
 * on its own (no fma), sums left to right in ascending m and l.
 * Inputs: the plane x; the layers Y_0 .. Y_{L-1}, 1 <= L <= NLE_REGION_LAYERS_MAX; the memberships' source planes q_1 .. q_M,
 * 1 <= M <= NLE_REGION_MAX (spread strokes, or the spreads of nle_filter_segment); the floor phi > 0; and for every row
 * m = 0 .. M (row 0 the background): the weights W[m][0 .. L-1]; w_rho[m], the gain a_m in [0, NLE_DETAIL_GAIN_MAX] and
 * sigma_m >= 0; a flag for a base curve; where it is on, a curve [lo_m, hi_m, T^m_0 .. T^m_N] in nle_tone_curve's layout.
 *   Memberships  exactly nle_region_combine's:  u_m = q_m[i] > 0 ? (double)q_m[i] : 0 (a NaN q counts as 0);
 *                sigma = u_1 + .. + u_M;  d = sigma > phi ? sigma : phi;  alpha_m = u_m / d;  alpha_0 = 1 - sigma / d
 *   S, rho, g_m  exactly nle_detail_combine's, with row m's a_m and sigma_m; the curve of row m is off when sigma_m == 0 or
 *                a_m == 1, and no exp is evaluated for it then
 *   Row results  y_m = w_rho[m] g_m(rho) + W[m][0] g_m(Y_0) + .. + W[m][L-2] g_m(Y_{L-2}) + B_m, left to right, with
 *                B_m = W[m][L-1] Y_{L-1} where row m has no base curve and nle_tone_combine's B' on row m's curve otherwise
 *                (Bw = W[m][L-1] Y_{L-1}; ks_m = N / (hi_m - lo_m) formed once on the host)
 *   Blend        c_m = alpha_m > 0 ? alpha_m y_m : 0;   y = ((c_0 + c_1) + ..) + c_M
 *                A row without influence on a pixel contributes nothing, not even its NaN: the kernel does not evaluate it.
 *   Output       the three NLE_REGION_OUT_* kinds with nle_region_combine's store rule; a NaN y is NaN in _F32, 0 in the others
 *   Chroma       a saturation s_m in [0, 4] per row; planes a, b on the project's scale (128 is neutral, 8-bit and deep alike):
 *                cm_m = alpha_m > 0 ? alpha_m s_m : 0;  c = ((cm_0 + cm_1) + ..) + cm_M
 *                a' = 128 + c (a - 128);  b' = 128 + c (b - 128), each rounded once to fp32
 * Consequences:
 *   (a) where every q <= 0 (or NaN): alpha_0 = 1 and the output is bit for bit nle_detail_combine / nle_tone_combine with
 *       row 0's parameters.  The sign of a zero is left open.
 *   (b) M = 1 and q_1 >= phi everywhere: alpha_1 = 1, alpha_0 = 0, the output is bit for bit the same calls with row 1's.
 *   (c) all rows equal: the alpha_m sum to 1 up to rounding, and y differs from the single-row result by at most (2 M + 4)
 *       fp64 roundings of y; a _F32 output by at most one spacing; the 8-bit kinds are equal wherever the single-row value is
 *       not within 1e-9 of a tie.
 *   (d) every curve off, w_rho = 0 and no base curve: y is nle_region_combine's value up to the different association (the
 *       rows are blended after the layers are summed, not before): not bitwise.
 *   (e) all s_m = 1: c is 1 up to rounding (|c - 1| <= (2 M + 4) 2^-53, as in (c)), a' = a up to one fp32 spacing.  The C++ surface and the
 *       CLI do not launch the chroma kernel then: the bytes are the plain command's.
 * nle_local_combine is the stage call, the rule alone, on any planes: d_x n floats; layer l at d_layers + l layer_stride and
 * plane m at d_q + (m - 1) q_stride (strides in floats, >= n); h_weights (M + 1) x L row-major; h_detail (M + 1) x 3 =
 * (w_rho, gain, sigma) per row; h_curve_on M + 1 ints (NULL: no row has a base curve); h_curves (M + 1) x
 * (NLE_TONE_KNOTS + 2), of which only the rows that are on are read (NULL exactly when none is on); d_out n floats, or n
 * bytes for NLE_REGION_OUT_U8.  No alignment is required of pointers or strides; every plane is read once.  Only the curves
 * that are on go to the device (8200 B of LDS each).
 * nle_local_chroma: d_a, d_b n floats; d_q as above; h_saturation M + 1 doubles; d_a_out, d_b_out n floats each.  In place
 * (d_a_out == d_a, d_b_out == d_b) is allowed; any other overlap of an output with an input or the other output is refused.
 * nle_apply_local is nle_apply_layers + nle_region_spread + nle_local_combine with the L + M work planes in the ctx's workspace:
 * bitwise what the three calls give, for every formulation nle_apply works for.  Strokes, scales, spread and floor as for
 * nle_apply_regions.  d_q_out (may be NULL) receives the M spreads, plane m at d_q_out + (m - 1) H W: the membership planes
 * nle_local_chroma takes, so that the chroma call does not spread twice.
 * All three return NLE_ERR_INVALID with a message that starts with the function's name, enqueue nothing and leave the ctx
 * usable for: M or L out of range; a NULL pointer (h_curve_on, h_scale and d_q_out apart; h_curves NULL while a flag is on);
 * a weight, w_rho or saturation that is not finite, a saturation outside [0, 4]; a gain outside [0, 3] or not finite; a sigma
 * that is negative or not finite; a floor or spread that is not finite and > 0; a scale that is not finite; a curve that is on
 * with lo, hi or a knot not finite or hi - lo not > 0; an unknown out kind; an output overlapping an input (chroma's in-place
 * case apart); n < 1 or a stride smaller than n (the stage calls); H W that is not the filter's and world > 1
 * (nle_apply_local: slabs and device groups are not built for it, as for regions). */
#define NLE_LOCAL_SATURATION_MAX 4
int nle_local_combine(nle_ctx* ctx, const float* d_x, const float* d_layers, int L, const float* d_q, int M, long long n,
                      long long layer_stride, long long q_stride, const double* h_weights, const double* h_detail,
                      const int* h_curve_on, const double* h_curves, double floor, int out_kind, void* d_out);
int nle_local_chroma(nle_ctx* ctx, const float* d_a, const float* d_b, const float* d_q, int M, long long n, long long q_stride,
                     const double* h_saturation, double floor, float* d_a_out, float* d_b_out);
int nle_apply_local(nle_filter* f, const float* d_x, int H, int W, int L, const float* d_strokes, int M, const double* h_scale,
                    double spread, double floor, const double* h_weights, const double* h_detail, const int* h_curve_on,
                    const double* h_curves, int out_kind, void* d_out, float* d_q_out);

/* ---- per-region histograms: auto levels and equalise for a region of its own (new in this build: no reference, so this
 * text and DESIGN.md section 3.21 are the definition) ---- */
/* The local adjustments above give a row a base curve of two slopes only; the levels and the equalisation of nle_tone_curve
 * need a histogram, and a region's histogram is the plane's with every pixel counted by its membership.
 * Per pixel i, in fp64, every operation rounded on its own (no fma), in the order written.  Inputs: the plane y (the base
 * layer); the memberships' source planes q_1 .. q_M, 1 <= M <= NLE_REGION_MAX; the floor phi > 0; a scale per row m = 0 .. M.
 *   Memberships  exactly nle_region_combine's:  u_m = q_m[i] > 0 ? (double)q_m[i] : 0 (a NaN q counts as 0);
 *                sigma = u_1 + .. + u_M;  d = sigma > phi ? sigma : phi;  alpha_m = u_m / d;  alpha_0 = 1 - sigma / d
 *   Weight       omega_m = (long long)(alpha_m 65536.0 + 0.5), a truncation (alpha_m >= 0): 0 .. NLE_REGION_WEIGHT_ONE.
 *                An alpha_m that is not > 0 (0, or the NaN an infinite q makes) has omega_m = 0.
 *   Bin          per row m nle_plane_histogram's rule on v = (double)y[i] scale_m: a NaN v -> counts[4097]; b < 0 -> counts[0];
 *                b >= 4096 -> counts[4097]; otherwise counts[1 + b].  Every row has a scale of its own; the callers pass
 *                W[m][L-1], the row's weight of the base layer.
 *   Count        counts[m][bin_m] += omega_m, for the rows that are switched on and where omega_m > 0
 * The counts are integers: the result is exact, independent of the order of the pixels and of the merges, and bit-equal from
 * run to run.  nle_tone_curve takes a row as it is: its counts are long long, and every step of it (need, the comparisons,
 * the shares F) is invariant under a common factor 2^16 of all counts.
 * Consequences:
 *   (a) where every q <= 0 (or NaN): row 0 is 65536 x nle_plane_histogram(y, scale_0) and every other row is zero.
 *   (b) hard memberships (every pixel has one q >= phi and the others <= 0): row m is 65536 x the histogram of region m's
 *       pixels alone, and the curve nle_tone_curve makes from row m is bit for bit the curve it makes from
 *       nle_plane_histogram over those pixels.
 *   (c) |sum_m omega_m - 65536| <= (M + 1) / 2 + 1 per pixel: a pixel's mass is one up to the roundings.
 *   (d) a tie rounds up: M = 1, phi = 0.5 and q = (2 k + 1) / 262144 give alpha 65536 = k + 0.5 exactly and omega = k + 1.
 * nle_region_histograms is the stage call: d_y n floats; plane m at d_q + (m - 1) q_stride (stride in floats, >= n); h_scale
 * M + 1 doubles; h_row_on M + 1 ints (NULL: every row is on), rows that are off come back as zeros; h_counts (M + 1) x
 * (NLE_TONE_BINS + 2) long long, row-major.  No alignment is required of pointers or strides; every plane is read once; the
 * call returns with the counts on the host.  NLE_ERR_INVALID with a message that starts with the function's name, nothing
 * enqueued and the ctx left usable, for: M out of range; n < 1; a stride below n; a NULL pointer (h_row_on apart); a scale or
 * floor that is not finite; a floor that is not > 0.
 * nle_apply_local_auto is nle_apply_local with the rows' curves made here.  h_tone is (M + 1) x 4 = (shadows, highlights,
 * clip_percent P, equalise A) per row, in nle_tone_curve's ranges.  It is these calls in this order, and bitwise what they
 * give: nle_apply_layers; nle_region_spread; nle_region_histograms on layer L - 1 with scale_m = W[m][L-1], only the rows
 * with P >= 0 or A > 0 switched on, skipped when no row is; one nle_tone_curve per row whose four numbers are not all
 * inactive (s == 0, h == 0, P < 0, A == 0: the row then has no base curve); nle_local_combine.  A row whose counts sum to
 * less than NLE_REGION_WEIGHT_ONE holds less than one pixel's mass: it takes nle_tone_curve(NULL, s, h, -1, 0) instead of
 * being refused.  When no row has P >= 0 or A > 0 the call is nle_apply_local with the (s, h) curves, bit for bit.
 * h_curves_out (may be NULL) receives (M + 1) x (NLE_TONE_KNOTS + 2) doubles: the curve of every row that has one, zeros for
 * the others.  Refusals: those of the calls it composes, and nle_tone_curve's ranges per row; world > 1 as for nle_apply_local. */
#define NLE_REGION_WEIGHT_ONE 65536
int nle_region_histograms(nle_ctx* ctx, const float* d_y, const float* d_q, int M, long long n, long long q_stride,
                          const double* h_scale, const int* h_row_on, double floor, long long* h_counts);
int nle_apply_local_auto(nle_filter* f, const float* d_x, int H, int W, int L, const float* d_strokes, int M,
                         const double* h_scale, double spread, double floor, const double* h_weights, const double* h_detail,
                         const double* h_tone, int out_kind, void* d_out, float* d_q_out, double* h_curves_out);

/* ---- several planes through one filter (new in this build) ---- */
/* Applies f to P planes in one call, each plane with its own set of responses: the channels of a colour image, several guide
 * planes, the stroke planes of the region edits, the a / b pair of the denoiser.  nle_apply (P = 1, one response) and
 * nle_apply_layers (P = 1, the layer responses of nle_layer_responses) are its special cases in meaning.
 *   d_x       plane m at d_x + m x_stride (stride in floats), a full H x W fp32 plane as nle_apply takes it; 1 <= P <= NLE_PLANES_MAX
 *   h_nresp   P counts, each 1 .. 64: the response vectors of plane m; NULL: one for every plane.  R = their sum <= 128
 *   h_resp    R x K' fp64, row-major, the rows of plane 0 first
 *   d_y       output j (the order of h_resp) at d_y + j y_stride, n_local floats each
 *   out_kind  NLE_REGION_OUT_F32: what nle_apply gives; NLE_REGION_OUT_ROUNDED8: what nle_apply_rounded8 gives, its rule
 *             included that table filters round the fp64 value and the other formulations their fp32 plane
 * Contract: for every formulation nle_apply works for, the outputs of plane m are BIT FOR BIT what nle_apply / nle_apply_layers
 * / nle_apply_rounded8 give for that plane and those responses alone.  What is shared between the planes is only what does
 * not depend on them: on the default (table) path with level-sorted rows, on one device, the reduce half makes one pass over
 * the sorted rows per group of four planes (two beyond 12 sample columns) and the expand half takes the R weight vectors in
 * its usual groups; every other formulation, filters without sorted rows (W > 8192, NLE_NO_SORTED_ROWS) and world > 1 run
 * the planes one by one.
 * NLE_ERR_INVALID, with a message, before anything is enqueued and with the ctx left usable: P out of range; a count out of
 * range or R > 128; a NULL pointer (h_nresp apart); an unknown out kind; a stride smaller than the plane when P (x_stride) or
 * R (y_stride) exceeds 1; H W that is not the filter's; any output plane overlapping any input plane. */
#define NLE_PLANES_MAX 16
int nle_apply_planes(nle_filter* f, const float* d_x, int P, long long x_stride, int H, int W, const int* h_nresp,
                     const double* h_resp, int out_kind, float* d_y, long long y_stride);

/* ---- colour wrapper on the device (the code either side of the path) ------------------------------- */
/* cv::cvtColor(COLOR_BGR2Lab) on an 8-bit image as the reference uses it (src/filter.cpp:423,463) and
 * the split / convertTo(CV_64F) of the L channel (:424-426,465-467): d_bgr n x 3 bytes -> d_lab n x 3
 * bytes (may be NULL) and d_L n floats = L in 0..255 (may be NULL).  OpenCV's 8-bit path is not the float formula of its
 * documentation but a fixed-point table algorithm (imgproc `RGB2Lab_b`); that algorithm is what runs here -- with it the
 * reference's README outputs are reproduced to 0.003 .. 0.5 grey levels (tests/test_oracle_readme_pairs.py). */
int nle_bgr2lab8(nle_ctx* ctx, const unsigned char* d_bgr, long long n, unsigned char* d_lab, float* d_L);
/* the tables of that conversion (host only): h_gamma[256] = sRGB decode scaled by 255 * 8, h_cbrt[3072] = f(t) of L*a*b*
 * scaled by 2^15 (t = i / 2040; made in single precision with OpenCV's truncating rational cube root, csrc/lab8_tables.cpp),
 * h_coeffs[9] = the XYZ matrix over the D65 white point in 12-bit fixed point, row major (R, G, B columns).  L = (296 fY - 1336934 + 2^14) >> 15, a = (500 (fX - fY) + 128 * 2^15 + 2^14) >> 15, b alike with
 * 200 (fY - fZ); f* = h_cbrt[(R c0 + G c1 + B c2 + 2^11) >> 12]. */
int nle_lab8_tables(unsigned short* h_gamma, unsigned short* h_cbrt, int* h_coeffs);
/* the tables of the inverse conversion (host only), everything in units of 2^-14: h_yf[256][2] = (y, fy) for an 8-bit L,
 * h_ab_to_xz[36864] = the inverse of f(t) for t = index - 8145 (t <= 3390 ? t 108 / 841 - 290 : t t / 2^14 t / 2^14, C
 * integer division), h_inv_gamma[4096] = round(255 sRGB_encode(i / 4096)), h_coeffs[9] = round(2^12 XYZ -> sRGB times the
 * D65 white point), rows R, G, B.  fx = fy + ((5 a 53687 + 2^7) >> 13) - 4194, fz = fy - (((b 41943 + 2^4) >> 9) - 10484);
 * channel = h_inv_gamma[clamp((c0 x + c1 y + c2 z + 2^13) >> 14, 0, 4095)]. */
int nle_lab8_inverse_tables(unsigned short* h_yf, int* h_ab_to_xz, unsigned short* h_inv_gamma, int* h_coeffs);
/* max(0) / min(255) / convertTo(CV_8U) / merge / cvtColor(COLOR_Lab2BGR) (src/filter.cpp:434-440): the L
 * channel is taken from d_L (clamped, rounded half to even) when given, else from d_lab.  The conversion is OpenCV's
 * integer 8-bit path (imgproc `Lab2RGBinteger`, tables below): with it `enhance` writes the author's README output files
 * byte for byte wherever the filtered L plane has no rounding tie (tests/test_readme_pairs_gpu.py). */
int nle_lab2bgr8(nle_ctx* ctx, const unsigned char* d_lab, const float* d_L, long long n, unsigned char* d_bgr);
/* the same with any of the three channels replaced by an fp32 plane (NULL = keep d_lab's), each clamped and
 * rounded like :391-399 -- the tail of NLEFilter::denoise (src/filter.cpp:391-409) */
int nle_lab2bgr8_planes(nle_ctx* ctx, const unsigned char* d_lab, const float* d_L, const float* d_a, const float* d_b,
                        long long n, unsigned char* d_bgr);
/* cv::split + convertTo of one channel (0, 1, 2) of an interleaved 8-bit 3-channel image (:363,376-378) */
int nle_lab8_channel(nle_ctx* ctx, const unsigned char* d_lab, long long n, int channel, float* d_out);

/* ---- deep colour (new in this build: the reference is 8-bit only, so this text and DESIGN.md section 3.13 are the definition) ---- */
/* 16-bit sRGB <-> float Lab, fp64 per pixel, every operation rounded on its own (no fma) and in the order written.
 * Tables (host only, no ctx): h_lin[c], c = 0 .. 65535: with v = c / 65535, v <= 0.04045 ? v / 12.92 : pow((v + 0.055) / 1.055,
 * 2.4).  h_thr[0] = -inf, h_thr[c] = the same curve at (c - 0.5) / 65535: strictly increasing; the encoding is DEFINED through
 * it, code(v) = (number of c with h_thr[c] <= v) - 1, a NaN gives 0 -- no pow on the device, no rounding ties.  h_coeffs[0 .. 9):
 * OpenCV's sRGB -> XYZ (D65) matrix, rows X, Y, Z and columns R, G, B, each row divided by its sum (m0 + m1) + m2 (white goes
 * to X = Y = Z = 1); h_coeffs[9 .. 18): the fp64 inverse of that matrix, rows R, G, B and columns X, Y, Z.
 * nle_bgr16_to_lab: d_bgr n x 3 uint16 (B, G, R interleaved) -> fp32 planes on the 8-bit path's scales, so that hy, the
 * chroma bandwidth and the layer weights mean what they mean there:
 *   t_X = (m0 lin[R] + m1 lin[G]) + m2 lin[B] with row X of the matrix, t_Y and t_Z alike
 *   f(t) = t > 216 / 24389 ? cbrt(t) : ((24389 / 27) t + 16) / 116
 *   L = ((116 f_Y - 16) 255) / 100,  a = 500 (f_X - f_Y) + 128,  b = 200 (f_Y - f_Z) + 128, each rounded once to fp32
 *   guide = round-half-even of the fp64 L, clamped to [0, 255]: the integer plane a train takes (the table path)
 * d_a, d_b and d_guide may each be NULL.
 * nle_lab_to_bgr16: L' = L > 0 ? (L < 255 ? L : 255) : 0 (a NaN counts as 0); a and b are not clamped;
 *   f_Y = ((L' 100) / 255 + 16) / 116,  f_X = f_Y + (a - 128) / 500,  f_Z = f_Y - (b - 128) / 200
 *   t = f > 6 / 29 ? (f f) f : ((116 f - 16) 27) / 24389
 *   channel = code((i0 t_X + i1 t_Y) + i2 t_Z) with its row of the inverse matrix: out-of-gamut values saturate at 0 and 65535.
 * The forward direction followed by fp32 storage and the inverse is the identity on every grey and on millions of random
 * triples (tests/test_deep_colour.py): fp32 planes lose nothing of a 16-bit image.
 * NLE_ERR_INVALID with a message, nothing enqueued and the ctx left usable: NULL d_bgr or d_L (either direction; the inverse
 * needs d_a and d_b too), n <= 0.  The tables go to the device once per ctx, on first use. */
int nle_srgb16_tables(double* h_lin /*65536*/, double* h_thr /*65536*/, double* h_coeffs /*18*/);
int nle_bgr16_to_lab(nle_ctx* ctx, const unsigned short* d_bgr, long long n, float* d_L, float* d_a, float* d_b, float* d_guide);
int nle_lab_to_bgr16(nle_ctx* ctx, const float* d_L, const float* d_a, const float* d_b, long long n, unsigned short* d_bgr);

/* ---- HDR tone mapping (new in this build: no reference, so this text and DESIGN.md section 3.14 are the definition) ---- */
/* Linear-light float images through the filter: log-luminance on the scale of an 8-bit L plane in, 16-bit sRGB out.  fp64
 * per pixel on the device, every operation rounded on its own (no fma) and in the order written; planes are stored as fp32.
 * d_bgr: n x 3 fp32 (B, G, R interleaved, linear light).  Y = (0.212671 R + 0.715160 G) + 0.072169 B (the Y row of the matrix
 * above, not renormalised).
 * nle_hdr_range: Ymax = the largest finite Y, Ymin+ = the smallest finite Y > 0 over the n pixels (two kernels, per-block
 *   pairs read in a fixed order, no atomics); on the host l_hi = log2(Ymax), l_lo = max(log2(Ymin+), l_hi - 24),
 *   *h_range = R = l_hi - l_lo, and R = 1 when R < 2^-20 (a flat image).  No pixel with a finite positive Y: NLE_ERR_INVALID.
 * nle_hdr_to_loglum: x = 255 ((log2(Y) - l_hi) / R) + 255, then clamped into [0, 255]: the clamp of Y into
 *   [2^(l_hi - R), 2^l_hi], taken after the logarithm where it is exact.  Y <= 0, -inf and NaN give 0 (the floor), +inf gives
 *   255 (the ceiling).  x is stored as fp32; guide = round-half-even of the fp64 x, the integer plane a train takes (table
 *   path).  With these scales hy means what it means for L planes.  d_x or d_guide may be NULL, not both.  Near x = 0 the sum
 *   cancels: there x carries the absolute error of the other values, a few 1e-14 / R.
 * nle_loglum_to_bgr16: from the filtered plane d_y (y = V f(Lambda) V^T x by nle_apply on the unrounded x) and the original
 *   colours: Yout = exp2(((y - 255 c) R) / 255) with c = base_weight = f(1), the last layer weight -- a constant plane 255
 *   comes out of the filter as 255 c, which anchors white; a NaN y gives Yout = 0.  Yin = Y clamped into [exp2(l_hi - R),
 *   exp2(l_hi)] (both ends evaluated on the host; a NaN Y, -inf and Y <= 0 count as the floor, +inf as the ceiling).  Per
 *   channel C of B, G, R: r = max(C, 0) / Yin (a NaN C counts as 0), Cout = (s == 1 ? r : pow(r, s)) Yout with s =
 *   saturation, and the 16-bit code of Cout is code(Cout) through h_thr exactly as nle_lab_to_bgr16 encodes: values out of
 *   range saturate at 0 and 65535, a NaN Cout (0 times inf) gives 0.  No gamut mapping beyond that.
 * NLE_ERR_INVALID with a message, nothing enqueued and the ctx left usable: a NULL input or output (both of d_x and d_guide),
 * n < 0, a non-finite l_hi or base_weight, a range or saturation that is not finite or not > 0, a saturation above 2.  No
 * pointer needs more than its type's alignment (the kernels take two pixels per thread where 8 bytes are given). */
int nle_hdr_range(nle_ctx* ctx, const float* d_bgr, long long n, double* h_l_hi, double* h_range);
int nle_hdr_to_loglum(nle_ctx* ctx, const float* d_bgr, long long n, double l_hi, double range, float* d_x, float* d_guide);
int nle_loglum_to_bgr16(nle_ctx* ctx, const float* d_y, const float* d_bgr, long long n, double l_hi, double range,
                        double base_weight, double saturation, unsigned short* d_bgr16);

/* ---- denoise wrapper (src/denoise.cpp, src/filter.cpp:349-410,521-538): the bilateral prefilter ------------- */
/* cv::bilateralFilter(src, dst, -1, sigmaColor, sigmaSpace, BORDER_DEFAULT) on a single-channel 8-bit plane, as
 * OpenCV documents it for CV_8UC1: radius = round(1.5 sigmaSpace) >= 1, circular window, fp32 weights
 * space[dy,dx] * colour[|v - v0|], fp32 sums in row-major window order, round-half-even of sum / wsum,
 * BORDER_REFLECT_101.  Planes are fp32 holding integers 0..255 (what nle_bgr2lab8 / nle_lab8_channel produce and
 * nle_train consumes); d_dst must not alias d_src.  OpenCV's own build (SIMD summation order, version) is not
 * available here, so agreement with it is unpinned beyond the documented formula. */
int nle_bilateral8(nle_ctx* ctx, const float* d_src, int H, int W, double sigma_color, double sigma_space, float* d_dst);
/* the two weight tables of that filter (host): *radius always; h_space_w (2 radius + 1)^2 floats with 0 outside
 * the circle and h_colour_w 256 floats when both are non-NULL */
int nle_bilateral_tables(double sigma_color, double sigma_space, int* radius, float* h_space_w, float* h_colour_w);

/* ---- MSE-guided denoise (new in this build: the reference's denoise stops short of Talebi & Milanfar, "Global Image
 * Denoising", IEEE TIP 23(2), 2014, which it set out to implement; this text and DESIGN.md section 3.16 are the definition) ---- */
/* nle_nlm8: non-local means on a single-channel 8-bit plane, the pre-filter of that method.  Planes are fp32 holding integers
 * 0..255, H x W.  P = patch_radius in [1, NLE_NLM_PATCH_RADIUS_MAX], S = search_radius in [1, NLE_NLM_SEARCH_RADIUS_MAX],
 * n = (2P + 1)^2, rho = reflect-101 (BORDER_REFLECT_101) applied to every coordinate the patch and search windows touch:
 *   SSD(p, q) = sum_{delta in [-P, P]^2} (u(rho(p + delta)) - u(rho(q + delta)))^2     (an exact integer, <= 49 255^2 < 2^24)
 *   Tf = (float)(2 sigma^2 n),  cf = (float)(1 / (n h^2))                              (fp64 on the host, rounded once)
 *   w(p, q) = exp(-max((float)SSD - Tf, 0) cf)   in fp32, for every q in the (2S + 1)^2 window around p; w(p, p) = 1
 *   raw(p) = sum_q w u(rho(q)) / sum_q w        fp32 sums, row by row of the window and then over the rows, a fixed order
 *   dst(p) = rintf(raw(p))                       an integer plane again: a train takes it on the table path
 * d_raw (may be NULL) receives raw.  The weight sum is >= 1, no division can fail.  sigma >= 0 is the noise level the
 * threshold 2 sigma^2 per pixel forgives, h > 0 the filtering strength; both finite, and so must Tf and cf be.
 * NLE_ERR_INVALID with a message, nothing enqueued and the ctx left usable: a parameter out of range, a NULL d_src or d_dst,
 * d_dst or d_raw aliasing d_src (or each other), a plane that is not integer valued in [0, 255], H or W < 1. */
#define NLE_NLM_PATCH_RADIUS_MAX 3
#define NLE_NLM_SEARCH_RADIUS_MAX 10
int nle_nlm8(nle_ctx* ctx, const float* d_src, int H, int W, int patch_radius, int search_radius, double sigma, double h,
             float* d_dst, float* d_raw);
/* nle_plane_noise: Immerkaer's noise estimate of an 8-bit plane (fp32 holding integers 0..255), H, W >= 3.  With the mask
 * M = [1 -2 1; -2 4 -2; 1 -2 1]:  S = sum over the (H - 2)(W - 2) interior pixels of |(x * M)(i, j)| -- every term an integer
 * <= 2040, summed in 64-bit integers (per-block partials, a second kernel adds them in a fixed order, no atomics): exact and
 * bitwise reproducible -- and sigma = sqrt(pi / 2) S / (6 (H - 2)(W - 2)), fp64 on the host.  *h_abs_sum = S (may be NULL),
 * *h_sigma = sigma.  The mask removes what is locally linear, not texture: texture counts as noise, so this is an UPPER
 * estimate -- the safe side for a denoiser.  NLE_ERR_INVALID as above for H or W < 3, NULL d_x or h_sigma and a plane that is
 * not integer valued in [0, 255]. */
int nle_plane_noise(nle_ctx* ctx, const float* d_x, int H, int W, long long* h_abs_sum, double* h_sigma);
/* nle_filter_coefficients: t = V^T x of P planes (plane m at d_x + m x_stride, a full H x W fp32 plane as nle_apply takes it;
 * 1 <= P <= NLE_PLANES_MAX): h_t is P x K' fp64, row-major.  For every formulation nle_apply works for, row m holds bit for bit
 * the K'-vector nle_apply on that plane forms internally (the table path: the reduce half, the sample rows' term and, where
 * apply takes them, training's own reduce half; the materialised forms and the exact filter: their row pass) -- so P planes
 * in one call equal P calls.  On the table path with level-sorted rows the planes share the reduce pass as in
 * nle_apply_planes.  NLE_ERR_INVALID with a message, nothing enqueued: P out of range, a NULL pointer, a stride smaller than
 * the plane when P > 1, H W that is not the filter's, and world > 1 (a sharded ctx: not built, refused before any collective). */
int nle_filter_coefficients(nle_filter* f, const float* d_x, int P, long long x_stride, int H, int W, double* h_t);
/* nle_mse_shrink (host only, no ctx): the power k of the shrinkage mu^k that minimises the estimated mean squared error when
 * the coefficients h_b (K values; those of a pre-filtered plane stand in for the clean signal's) meet noise of level sigma:
 *   mu_j = min(max(lambda_j, 0), 1);   k_i = k_max i / n_grid,  i = 0 .. n_grid
 *   MSE_i = sum_j [(1 - mu_j^k_i)^2 b_j^2 + sigma^2 mu_j^(2 k_i)]      fp64, std::pow (pow(0, 0) = 1), summed in index order
 * *h_k = k_i of the smallest i that attains the minimum; h_mse (n_grid + 1 values, may be NULL) receives every MSE_i.  k = 0
 * leaves the span untouched, a large k keeps only the modes with lambda = 1.  NLE_ERR_INVALID: K < 1, n_grid < 1 or > 65536,
 * sigma or k_max negative or not finite, NULL h_eigvals, h_b or h_k. */
int nle_mse_shrink(const double* h_eigvals, const double* h_b, int K, double sigma, double k_max, int n_grid, double* h_k,
                   double* h_mse);
/* the pre-filters of the denoise wrapper (nle::DenoiseOptions, `denoise --prefilter`) */
#define NLE_PREFILTER_BILATERAL 0
#define NLE_PREFILTER_NLM 1

/* leading dimension used for a logical width n: (n + 3) & ~3 */
int nle_ld(int n);

/* ---- measurement hooks (bench.py) --------------------------------------------------- */
/* Kernel ids for the per-kernel HIP-event timing below. */
enum {
    NLE_K_AFFINITY = 0,      /* materialising affinity pass (stage API: computeKernel)   */
    NLE_K_NYSTROM = 1,       /* affinity-fused Nystrom extension GEMM (Phi)              */
    NLE_K_SINKHORN_PASS = 2, /* one Sinkhorn half-iteration over all local pixels        */
    NLE_K_REDUCE = 3,        /* second-stage fp64 reduction of block partials            */
    NLE_K_GRAM = 4,          /* Gram contraction                                         */
    NLE_K_PROJECT = 5,       /* projection GEMM  V = diag(c) Phi C                       */
    NLE_K_APPLY_REDUCE = 6,  /* t = V^T x                                                */
    NLE_K_APPLY_EXPAND = 7,  /* y_l = V (g_l o t)                                        */
    NLE_K_SMALL = 8,         /* everything p/r/K-sized on the device                     */
    NLE_K_SINK_TABLES = 9,   /* table pass: per-row g tables (k_hist_g)                  */
    NLE_K_GRAM_ROWS = 10,    /* table Gram: per-row histograms (k_ghist_rows)            */
    NLE_K_GRAM_GEMM = 11,    /* table Gram: fp64 MFMA GEMM (k_ghist_gemm)                */
    NLE_KERNEL_COUNT = 12,   /* the ids of the train / apply path end here (kept: callers size their tables by it) */
    NLE_K_NLM8 = 12,         /* non-local-means pre-filter (k_nlm8)                      */
    NLE_K_PLANE_NOISE = 13,  /* Immerkaer noise sum: per-block partials + their fold     */
    NLE_K_PLANE_HIST = 14,   /* histogram of a scaled plane (k_plane_hist)                */
    NLE_K_TONE_COMBINE = 15, /* detail combine with the base tone curve (k_tone_combine) */
    NLE_KERNEL_COUNT_ALL = 16 /* every id nle_kernel_name and nle_ctx_kernel_stats take  */
};
const char* nle_kernel_name(int kid);
/* enable != 0: bracket kernel launches of the ctx with HIP events recorded on the ctx's stream and
 * accumulate per-kernel launch counts and durations (resolved whenever the pipeline synchronises the
 * stream).  enable == 1: the N-sized kernels only; enable == 2: also the p-sized / second-stage
 * kernels (every timed launch opens a ~10 us gap on the stream).  Resets the counters. */
int nle_ctx_profile(nle_ctx* ctx, int enable);
int nle_ctx_kernel_stats(nle_ctx* ctx, int kid, long long* launches, double* total_ms);
/* Run `reps` launches of the materialising affinity kernel (the HBM-roofline pass of
 * computeKernel) and return the average launch duration in ms, measured with HIP events on
 * the ctx's stream. */
int nle_bench_affinity(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples,
                       int n_col_samples, double hx, double hy, float* d_kab, int reps,
                       double* h_avg_ms);
/* the same for the fp64 affinity rows of NLE_MODE_STREAMED_F64 / nle_compute_kernel64 (libm exp, 8 bytes per entry) on the
 * first `rows` image rows of this rank's slab: d_kab holds rows * W * nle_ld(p) doubles */
int nle_bench_affinity64(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, double hx,
                         double hy, long long rows, double* d_kab, int reps, double* h_avg_ms);
/* the range of 16-level tiles [first, first + n) that occur in the plane the filter was trained on: the columns of the
 * look-up-table formulation's g / h tables that its kernels make, store and contract (the others are skipped); (0, 16)
 * for a filter that does not run on level-sorted rows.  For byte models of those kernels. */
int nle_filter_level_tiles(const nle_filter* f, int* first_tile, int* n_tiles);
/* same for one Sinkhorn half-iteration pass over a device-resident phi */
int nle_bench_sinkhorn_pass(nle_ctx* ctx, const float* d_phi, long long M, int ld, int r,
                            int reps, double* h_avg_ms);

#ifdef __cplusplus
}
#endif
#endif /* NLE_H */
