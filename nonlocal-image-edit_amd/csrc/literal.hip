// The literal decomposition (reference src/filter.cpp:480-502 as written) with Phi = K_AB^T B materialised, in fp32
// (NLE_MODE_MATERIALISED) and in fp64 (generic64.hip: auto mode's fallback), its stages, the stage entry points that expose
// exactly these, the four that expose fused.hip's launchers (nle_sample_*), those that expose the table path's (nle_table_*),
// and the micro-benchmarks of two of its kernels.
#include "train.h"

using namespace nlep;

namespace {
// B = V_A diag(1/lambda) as fp32 row-major p x ldr
std::vector<float> build_B(const Nystrom& n, int p) {
    std::vector<float> B((size_t)p * n.ldr, 0.f);
    for (int k = 0; k < n.r; ++k) {
        const double inv = recip0(n.lam[k]);
        for (int s = 0; s < p; ++s) B[(size_t)s * n.ldr + k] = (float)(n.VA[(size_t)k * p + s] * inv);
    }
    return B;
}

// Phi for the local slab: fused affinity + Nystrom extension, then exact V_A sample rows
void build_phi(nle_ctx* c, const float* d_lum, const SampleSet& ss, const Nystrom& ny, double hx,
               double hy, long long pix0, long long M, float* d_phi) {
    const int p = ss.p;
    DevBuf<float4> d_samples = upload_samples(c, ss);
    std::vector<float> B = build_B(ny, p);
    DevBuf<float> d_B(B.size());
    HIP_OK(hipMemcpyAsync(d_B.p, B.data(), B.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    const float sw = nsw_of(hx), pw = nsw_of(hy);
    if (c->nystrom_bf16x3 || c->sw.nystrom_bf16x3) {  // split-bf16 operands on the bf16 matrix cores (tsgemm_bf16x3.hip)
        DevBuf<unsigned short> d_Bs(nlek::ts_gemm_bf16x3_bsplit_elems(p, ny.ldr));
        HIP_OK(nlek::ts_gemm_bf16x3_split(c->stream, d_B.p, p, ny.ldr, d_Bs.p));
        PROFILED(c, NLE_K_NYSTROM, nlek::ts_gemm_bf16x3(c->stream, d_lum, ss.gs, d_samples.p, sw, pw, pix0, d_Bs.p, ny.ldr, p,
                                                        d_phi, ny.ldr, M));
    } else {
        PROFILED(c, NLE_K_NYSTROM, nlek::ts_gemm(c->stream, true, nullptr, 0, d_lum, ss.gs, d_samples.p, sw, pw, pix0,
                                                 d_B.p, ny.ldr, p, d_phi, ny.ldr, M, nullptr, NLE_EPS));
    }
    // sample pixels carry their exact V_A row (top block of phi, reference :275); drains the stream before B goes
    scatter_sample_rows(c, ss.pix, p, ny.VA, ny.r, ny.ldr, pix0, M, d_phi);
}

// Sinkhorn (reference :238-245) as 2T passes: t0 = Phi^T 1, then alternately
// t <- Phi^T recip(Phi (lam o t)).  Returns u_c, u_r (host) and leaves lam o t_c_in on d_u_c.
template <typename T_>
void sinkhorn_passes(nle_ctx* c, const T_* d_phi, long long M, int ld_phi, int r, const std::vector<double>& lam, int T,
                     std::vector<double>* u_c, std::vector<double>* u_r, double* d_u_c_out /* ld4(r) doubles or null */) {
    if (T < 1) throw Fail{NLE_ERR_INVALID, "nSinkhornIter must be >= 1"};
    if (std::is_same<T_, double>::value && r > 2048)
        throw Fail{NLE_ERR_INVALID, "the fp64 Sinkhorn pass takes a logical width of at most 2048"};
    // length of lam, t and of a row of partials (== ld_phi on the train paths)
    const int ld = std::is_same<T_, float>::value ? ld_phi : ld4(r);
    std::vector<double> lam_pad(ld, 0.0);
    std::copy(lam.begin(), lam.begin() + r, lam_pad.begin());
    DevBuf<double> d_lam(ld), d_t[3], d_partial((size_t)nlek::kRowpassMaxBlocks * ld);
    for (auto& b : d_t) b.alloc(ld);
    HIP_OK(hipMemcpyAsync(d_lam.p, lam_pad.data(), ld * sizeof(double), hipMemcpyHostToDevice, c->stream));
    // one pass: t_out = Phi^T 1 (COLSUM), or Phi^T recip(Phi (lam o t_in)), summed over the ranks
    auto pass = [&](int mode, const double* t_in, double* t_out) {
        int nb = 0;
        PROFILED(c, NLE_K_SINKHORN_PASS, rowpass_any(c->stream, mode, d_phi, M, ld_phi, r, t_in, t_in ? d_lam.p : nullptr,
                                                       nullptr, NLE_EPS, d_partial.p, &nb));
        PROFILED(c, NLE_K_REDUCE, nlek::reduce_partials(c->stream, d_partial.p, nb, ld, t_out));
        all_reduce(c, t_out, ld);
    };
    pass(nlek::ROWPASS_COLSUM, nullptr, d_t[0].p);  // t_r(0) = Phi^T 1
    // cur = index of the t feeding the next pass
    int cur = 0;
    int idx_c_in = 0, idx_r_in = 0;
    for (int it = 0; it < T; ++it) {
        // c = recip(Phi (lam o t_r));  t_c = Phi^T c
        idx_c_in = cur;
        int nxt = (cur + 1) % 3;
        pass(nlek::ROWPASS_RECIP, d_t[cur].p, d_t[nxt].p);
        cur = nxt;
        idx_r_in = cur;
        if (it + 1 < T) {
            // r = recip(Phi (lam o t_c));  t_r = Phi^T r  (not needed after the last iteration:
            // only u_r = lam o t_c enters the W blocks)
            nxt = (cur + 1) % 3;
            if (nxt == idx_c_in) nxt = (nxt + 1) % 3;
            pass(nlek::ROWPASS_RECIP, d_t[cur].p, d_t[nxt].p);
            cur = nxt;
        }
    }
    std::vector<double> tc(ld), tr(ld);
    HIP_OK(hipMemcpyAsync(tc.data(), d_t[idx_c_in].p, ld * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(tr.data(), d_t[idx_r_in].p, ld * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (d_u_c_out) PROFILED(c, NLE_K_SMALL, nlek::scale_vec(c->stream, d_lam.p, d_t[idx_c_in].p, ld, d_u_c_out));
    HIP_OK(hipStreamSynchronize(c->stream));
    u_c->assign(r, 0.0);
    u_r->assign(r, 0.0);
    for (int k = 0; k < r; ++k) {
        (*u_c)[k] = lam[k] * tc[k];
        (*u_r)[k] = lam[k] * tr[k];
    }
}

// G (r x r col-major) = sum_i c_i^2 phi_i phi_i^T over ALL rows of every rank
std::vector<double> gram_all(nle_ctx* c, const float* d_phi, long long M, int ld, int r, const double* d_u) {
    const int ntiles = nlek::gram_num_tiles(ld);
    DevBuf<double> d_partial(std::max<size_t>(nlek::gram_partial_elems(std::max<long long>(M, 1), ld), 1));
    DevBuf<double> d_tiles((size_t)ntiles * 1024);
    if (M > 0) {
        PROFILED(c, NLE_K_GRAM, nlek::gram(c->stream, d_phi, M, ld, d_u, NLE_EPS, d_partial.p, d_tiles.p));
    } else {
        HIP_OK(hipMemsetAsync(d_tiles.p, 0, (size_t)ntiles * 1024 * sizeof(double), c->stream));
    }
    all_reduce(c, d_tiles.p, (size_t)ntiles * 1024);
    std::vector<double> tiles((size_t)ntiles * 1024);
    HIP_OK(hipMemcpyAsync(tiles.data(), d_tiles.p, tiles.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return unpack_tiles(tiles, ld, r, 32);
}

void build_phi64(nle_ctx* c, const float* d_lum, const SampleSet& ss, const Nystrom& ny, double hx, double hy, long long pix0,
                 long long M, double* d_phi) {
    const int p = ss.p, ldp = ld4(p), r = ny.r, ldr = ny.ldr;
    const AffinityRows64 kab(c, d_lum, ss, hx, hy, /*want_mask=*/false);
    DevBuf<double> d_B(ny.B.size());  // p x r column-major = what ts_gemm64 takes
    HIP_OK(hipMemcpyAsync(d_B.p, ny.B.data(), ny.B.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemsetAsync(d_phi, 0, (size_t)std::max<long long>(M, 1) * ldr * sizeof(double), c->stream));
    const long long chunk = 1ll << 20;  // affinity rows of 1 Mi pixels at a time (K_AB is never held whole)
    DevBuf<double> d_kab((size_t)std::min<long long>(std::max<long long>(M, 1), chunk) * ldp);
    for (long long i0 = 0; i0 < M; i0 += chunk) {
        const long long m = std::min(chunk, M - i0);
        PROFILED(c, NLE_K_AFFINITY, kab.rows(pix0 + i0, m, d_kab.p));
        PROFILED(c, NLE_K_NYSTROM, nlek::ts_gemm64(c->stream, d_kab.p, m, ldp, p, d_B.p, r, nullptr, d_phi + (size_t)i0 * ldr, ldr));
    }
    scatter_sample_rows(c, ss.pix, p, ny.VA, r, ldr, pix0, M, d_phi);  // exact V_A rows (top block of phi, reference :275)
}

// G (r x r col-major) = sum over ALL rows of every rank of c_i^2 phi_i phi_i^T, c_i = recip(phi_i . u) (d_u null: 1)
std::vector<double> gram_all(nle_ctx* c, const double* d_phi, long long M, int ld, int r, const double* d_u) {
    DevBuf<double> d_cs, d_part(std::max<size_t>(nlek::gram64d_partial_elems(std::max<long long>(M, 1), r), 1)), d_G((size_t)r * r);
    if (d_u && M > 0) {
        d_cs.alloc((size_t)M);
        PROFILED(c, NLE_K_SMALL, nlek::row_scalings64(c->stream, d_phi, M, ld, r, d_u, NLE_EPS, d_cs.p));
    }
    PROFILED(c, NLE_K_GRAM, nlek::gram64d(c->stream, d_phi, M, ld, r, d_cs.p, d_part.p, d_G.p));
    all_reduce(c, d_G.p, (size_t)r * r);
    std::vector<double> G((size_t)r * r);
    HIP_OK(hipMemcpyAsync(G.data(), d_G.p, G.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return G;
}

// the bodies of the stage entry points that come as an fp32 / fp64 pair and differ in their argument check only
template <typename T>
void sinkhorn_scalings_impl(nle_ctx* ctx, const T* d_phi, long long M, int ld, int r, const double* h_eigvals, int max_iter,
                            double* h_u_c, double* h_u_r) {
    HIP_OK(hipSetDevice(ctx->device));
    std::vector<double> lam(h_eigvals, h_eigvals + r), uc, ur;
    sinkhorn_passes(ctx, d_phi, M, ld, r, lam, max_iter, &uc, &ur, nullptr);
    std::copy(uc.begin(), uc.end(), h_u_c);
    std::copy(ur.begin(), ur.end(), h_u_r);
}
// h_u as the kernels of T read it: ld entries, zero padded, for fp32; the r entries themselves for fp64
template <typename T>
std::vector<double> padded_u(const double* h_u, int ld, int r) {
    std::vector<double> u(std::is_same<T, float>::value ? ld : r, 0.0);
    std::copy(h_u, h_u + r, u.begin());
    return u;
}
template <typename T>
void gram_impl(nle_ctx* ctx, const T* d_phi, long long M, int ld, int r, const double* h_u, double* h_G) {
    HIP_OK(hipSetDevice(ctx->device));
    DevBuf<double> d_u;
    if (h_u) {
        const std::vector<double> u = padded_u<T>(h_u, ld, r);
        d_u.alloc(u.size());
        HIP_OK(hipMemcpy(d_u.p, u.data(), u.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    const std::vector<double> G = gram_all(ctx, d_phi, M, ld, r, d_u.p);
    std::copy(G.begin(), G.end(), h_G);
}
template <typename T>
void row_scalings_impl(nle_ctx* ctx, const T* d_phi, long long M, int ld, int r, const double* h_u, double* d_out) {
    HIP_OK(hipSetDevice(ctx->device));
    const std::vector<double> u = padded_u<T>(h_u, ld, r);
    DevBuf<double> d_u(u.size());
    HIP_OK(hipMemcpyAsync(d_u.p, u.data(), u.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if constexpr (std::is_same<T, float>::value) HIP_OK(nlek::row_scalings(ctx->stream, d_phi, M, ld, d_u.p, NLE_EPS, d_out));
    else HIP_OK(nlek::row_scalings64(ctx->stream, d_phi, M, ld, r, d_u.p, NLE_EPS, d_out));
    HIP_OK(hipStreamSynchronize(ctx->stream));
}

// nle_compute_kernel[64]: Ka on the host and this rank's affinity rows (T = float: the plain fp32 kernel, which takes none of
// the ctx's affinity options; T = double: under those options)
template <typename T>
void compute_kernel_impl(nle_ctx* ctx, const float* d_lum, int H, int W, int nRow, int nCol, double hx, double hy, double* h_Ka,
                         T* d_kab) {
    constexpr bool f64 = std::is_same<T, double>::value;
    const GridSpec gs = checked_grid(H, W, nRow, nCol);
    const AffinityOpts opts = affinity_opts(ctx);
    check_affinity_opts(ctx, opts, gs, H, W, hx, hy, f64 ? Caller::KERNEL64 : Caller::KERNEL32);
    HIP_OK(hipSetDevice(ctx->device));
    std::vector<long long> list;
    FetchSpec spec;
    if (f64 && opts.listed()) list = sampler_list(ctx, d_lum, gs, hx, hy), spec.list = &list;
    const SampleSet ss = fetch_samples(ctx, d_lum, gs, f64 ? opts : AffinityOpts{}, spec);
    if (f64) require_integer_planes(ctx, ss, /*agree_over_ranks=*/false);
    if (h_Ka) {
        const std::vector<double> Ka = build_Ka(ss, hx, hy);
        std::copy(Ka.begin(), Ka.end(), h_Ka);
    }
    if (!d_kab) return;
    int row0, row1;
    slab(H, ctx->rank, ctx->world, &row0, &row1);
    const long long pix0 = (long long)row0 * W, M = (long long)(row1 - row0) * W;
    if constexpr (f64) {
        const AffinityRows64 kab(ctx, d_lum, ss, hx, hy, /*want_mask=*/false);
        PROFILED(ctx, NLE_K_AFFINITY, kab.rows(pix0, M, d_kab));
    } else {
        DevBuf<float4> d_samples = upload_samples(ctx, ss);
        PROFILED(ctx, NLE_K_AFFINITY, nlek::affinity(ctx->stream, d_lum, gs, d_samples.p, ss.p, ld4(ss.p), nsw_of(hx), nsw_of(hy),
                                                     pix0, M, d_kab));
    }
    HIP_OK(hipStreamSynchronize(ctx->stream));
    prof_flush(ctx);
}

// nle_nystrom_residual: r_i = 1 - || F^T k_i ||^2 for every pixel, F = B diag(sqrt(lambda)) of solve_Ka (F F^T = pinv(K_A) at
// the reference's cut; L^-T on the Cholesky route), and its summary.  FUSED (resid.hip: k_nystrom_resid64) generates the fp64
// affinities inside the MFMA kernel; ROWS runs AffinityRows64 -> ts_gemm64 -> k_resid_rows chunk by chunk, the chunks cut at
// multiples of the summary tile so that the partials -- and the summary's bits -- do not depend on the chunk size.
void nystrom_residual_impl(nle_ctx* ctx, const float* d_lum, int H, int W, int nRow, int nCol, double hx, double hy, int form,
                           double thresh, float* d_r, double* h_summary) {
    if (ctx->world > 1) throw Fail{NLE_ERR_INVALID, "nle_nystrom_residual: world > 1 is not supported (no slabs)"};
    if (!d_lum || !h_summary) throw Fail{NLE_ERR_INVALID, "nle_nystrom_residual: the plane and the summary must not be NULL"};
    if (!std::isfinite(thresh)) throw Fail{NLE_ERR_INVALID, "nle_nystrom_residual: thresh must be finite"};
    if (form != NLE_RESID_AUTO && form != NLE_RESID_ROWS && form != NLE_RESID_FUSED)
        throw Fail{NLE_ERR_INVALID, "nle_nystrom_residual: unknown form " + std::to_string(form)};
    const GridSpec gs = checked_grid(H, W, nRow, nCol);
    if (!(hx > 0) || !(hy > 0)) throw Fail{NLE_ERR_INVALID, "hx and hy must be > 0"};
    const int p = gs.p(), ldp = ld4(p);
    if (p > 2048) throw Fail{NLE_ERR_INVALID, "more than 2048 samples is not supported"};
    const AffinityOpts opts = affinity_opts(ctx);
    check_affinity_opts(ctx, opts, gs, H, W, hx, hy, Caller::KERNEL64);
    const bool fused_ok = !opts.any() && nlek::resid_fused_applies(p);
    if (form == NLE_RESID_FUSED && !fused_ok)
        throw Fail{NLE_ERR_INVALID, "NLE_RESID_FUSED takes single-value luminance affinities (patch radius 0, no chroma planes), "
                                    "the grid sampler and at most 256 samples: use NLE_RESID_ROWS or NLE_RESID_AUTO"};
    const bool fused = form == NLE_RESID_FUSED || (form == NLE_RESID_AUTO && fused_ok);
    HIP_OK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::vector<long long> list;
    FetchSpec spec;
    if (opts.listed()) list = sampler_list(ctx, d_lum, gs, hx, hy), spec.list = &list;
    const SampleSet ss = fetch_samples(ctx, d_lum, gs, opts, spec);
    require_integer_planes(ctx, ss, /*agree_over_ranks=*/false);
    const std::vector<double> Ka = build_Ka(ss, hx, hy);
    const Nystrom ny = solve_Ka(ctx, ctx->sw, Ka, p, /*allow_chol=*/true);  // as the default train factors Ka
    const int m = ny.r;
    // F on the device: column-major p x m (ts_gemm64's B) for ROWS, row-major p x ldf (zero padded) for FUSED
    const int ldf = fused ? nlek::resid_fused_ld(m) : m;
    DevBuf<double> d_F((size_t)p * ldf);
    std::vector<double> F;  // host staging: alive until the stream is drained below
    // device Cholesky (from NLE_DEV_SOLVER_MIN = 288 samples on: the fused form only when that switch is lowered): L^-1 is
    // p x p column-major there, i.e. F = L^-T row-major
    if (ny.dev) {
        if (fused) {
            HIP_OK(hipMemsetAsync(d_F.p, 0, d_F.n * sizeof(double), st));
            HIP_OK(hipMemcpy2DAsync(d_F.p, (size_t)ldf * sizeof(double), ny.dev->ch.Linv.p, (size_t)p * sizeof(double),
                                    (size_t)p * sizeof(double), p, hipMemcpyDeviceToDevice, st));
        } else {
            PROFILED(ctx, NLE_K_SMALL, nlek::transpose64(st, p, ny.dev->ch.Linv.p, d_F.p));
        }
    } else {
        F.assign((size_t)p * ldf, 0.0);
        for (int k = 0; k < m; ++k) {
            const double s = std::sqrt(ny.lam[k]);
            for (int a = 0; a < p; ++a) F[fused ? (size_t)a * ldf + k : (size_t)k * p + a] = ny.B[(size_t)k * p + a] * s;
        }
        HIP_OK(hipMemcpyAsync(d_F.p, F.data(), F.size() * sizeof(double), hipMemcpyHostToDevice, st));
    }
    const long long N = (long long)H * W, nparts = nlek::resid_num_parts(N);
    DevBuf<double> d_part((size_t)nparts * 4), d_sum(4);
    if (fused) {
        DevBuf<float4> d_samples = upload_samples(ctx, ss);
        PROFILED(ctx, NLE_K_NYSTROM, nlek::nystrom_resid64(st, d_lum, gs, d_samples.p, p, 1.0 / (hx * hx), 1.0 / (hy * hy), N,
                                                           d_F.p, m, thresh, d_r, d_part.p));
        PROFILED(ctx, NLE_K_SMALL, nlek::resid_finish(st, d_part.p, nparts, d_sum.p));
        HIP_OK(hipMemcpyAsync(h_summary, d_sum.p, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
    } else {
        const int ldt = ld4(m);
        // train_stream64's chunk (NLE_STREAM64_CHUNK_MB of affinity rows), cut down to a multiple of the summary tile
        const long long rows_fit = (long long)(((size_t)ctx->sw.stream64_chunk_mb << 20) / ((size_t)ldp * sizeof(double)));
        long long CH = std::max<long long>(256, std::min<long long>(N, rows_fit));
        if (CH < N) CH -= CH % nlek::kResidTile;
        const AffinityRows64 kab(ctx, d_lum, ss, hx, hy, /*want_mask=*/false);
        DevBuf<double> d_K((size_t)CH * ldp), d_T((size_t)CH * ldt);
        for (long long i0 = 0; i0 < N; i0 += CH) {
            const long long mc = std::min(CH, N - i0);
            PROFILED(ctx, NLE_K_AFFINITY, kab.rows(i0, mc, d_K.p));
            PROFILED(ctx, NLE_K_NYSTROM, nlek::ts_gemm64(st, d_K.p, mc, ldp, p, d_F.p, m, nullptr, d_T.p, ldt));
            PROFILED(ctx, NLE_K_SMALL, nlek::resid_rows64(st, d_T.p, mc, ldt, m, i0, thresh, d_r, d_part.p));
        }
        PROFILED(ctx, NLE_K_SMALL, nlek::resid_finish(st, d_part.p, nparts, d_sum.p));
        HIP_OK(hipMemcpyAsync(h_summary, d_sum.p, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
    }
    prof_flush(ctx);
}

// the micro-benchmarks: one untimed launch, then the average of `reps` timed ones
template <typename Launch>
double bench_ms(nle_ctx* ctx, int reps, Launch&& launch) {
    HIP_OK(launch());
    Timer tm(ctx->stream);
    tm.start();
    for (int i = 0; i < reps; ++i) HIP_OK(launch());
    tm.stop();
    return tm.ms() / reps;
}
// the checks and the sample set of the two affinity benchmarks (the plain kernels, whatever the ctx's options are); this
// rank's rows are [*row0, *row1)
SampleSet bench_samples(nle_ctx* ctx, const float* d_lum, int H, int W, int nRow, int nCol, int* row0, int* row1) {
    check_image_size(H, W);
    GridSpec gs;
    if (!make_grid(H, W, nRow, nCol, &gs)) throw Fail{NLE_ERR_INVALID, "invalid sample counts"};
    HIP_OK(hipSetDevice(ctx->device));
    slab(H, ctx->rank, ctx->world, row0, row1);
    return fetch_samples(ctx, d_lum, gs, AffinityOpts{});
}

// nle_sample_pass / _gram / _project: the plane's sample set on the device and the slab [row0, row1), as train_phi_free_exp
// hands them to fused.hip's launchers (the plain fp32 affinity: none of the ctx's affinity options)
struct SampleStage {
    SampleSet ss;
    DevBuf<float4> d_samples;
    float nsw, npw;
    long long pix0, M;
};
SampleStage sample_stage(nle_ctx* ctx, const float* d_lum, int H, int W, int nRow, int nCol, double hx, double hy, int row0,
                         int row1, int max_p, const char* refusal) {
    const GridSpec gs = checked_grid(H, W, nRow, nCol);
    if (!(hx > 0) || !(hy > 0)) throw Fail{NLE_ERR_INVALID, "hx and hy must be > 0"};
    if (row0 < 0 || row1 <= row0 || row1 > H) throw Fail{NLE_ERR_INVALID, "need 0 <= row0 < row1 <= H"};
    if (gs.p() > max_p) throw Fail{NLE_ERR_INVALID, refusal};
    HIP_OK(hipSetDevice(ctx->device));
    SampleStage st;
    st.ss = fetch_samples(ctx, d_lum, gs, AffinityOpts{});
    st.d_samples = upload_samples(ctx, st.ss, nlek::sink_pass_ld(st.ss.p));
    st.nsw = nsw_of(hx), st.npw = nsw_of(hy);
    st.pix0 = (long long)row0 * W, st.M = (long long)(row1 - row0) * W;
    return st;
}
template <typename T>
DevBuf<T> uploaded(nle_ctx* ctx, const T* h, size_t n) {
    DevBuf<T> d(n);
    HIP_OK(hipMemcpyAsync(d.p, h, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return d;
}
}  // namespace

namespace nlep {

std::vector<double> unpack_tiles(const std::vector<double>& tiles, int ld, int n, int ts) {
    std::vector<double> G((size_t)n * n, 0.0);
    const int nt = (ld + ts - 1) / ts;
    int t = 0;
    for (int ti = 0; ti < nt; ++ti)
        for (int tj = ti; tj < nt; ++tj, ++t) {
            const double* tl = tiles.data() + (size_t)t * ts * ts;
            for (int a = 0; a < ts; ++a)
                for (int b = 0; b < ts; ++b) {
                    const int i = ti * ts + a, j = tj * ts + b;
                    if (i >= n || j >= n) continue;
                    if (ti == tj && j < i) continue;  // diagonal tiles: take the upper half
                    const double v = tl[a * ts + b];
                    G[(size_t)j * n + i] = v;
                    G[(size_t)i * n + j] = v;
                }
        }
    return G;
}

// (1) materialised Phi: Phi = K_AB^T B written once (N x r fp32), streamed by every later pass
void TrainPath::train_materialised(const Nystrom& ny) {
    tm_s.start();
    DevBuf<float> d_phi((size_t)std::max<long long>(M, 1) * ny.ldr);
    build_phi(c, d_lum, ss, ny, hx, hy, pix0, M, d_phi.p);
    std::vector<double> u_c, u_r;
    DevBuf<double> d_u_c(ny.ldr);
    sinkhorn_passes(c, d_phi.p, M, ny.ldr, ny.r, ny.lam, T, &u_c, &u_r, d_u_c.p);
    tm_s.stop();
    tm_g.start();
    std::vector<double> G = gram_all(c, d_phi.p, M, ny.ldr, ny.r, d_u_c.p);
    tm_g.stop();
    double h0 = now_ms();
    Ortho o = orthogonalize_host(ny, ss.p, u_c, u_r, std::move(G), n_eig, /*device_f32=*/true, c->topk_solver, c->sw.trace);
    *host_ms += now_ms() - h0;
    adopt_ortho(f, o);
    f->formulation = NLE_MODE_MATERIALISED;
    tm_p.start();
    std::vector<float> Cp((size_t)ny.r * f->ldv, 0.f);
    for (int k = 0; k < o.K; ++k)
        for (int j = 0; j < ny.r; ++j) Cp[(size_t)j * f->ldv + k] = (float)o.Cproj[(size_t)k * ny.r + j];
    DevBuf<float> d_Cp(Cp.size());
    HIP_OK(hipMemcpyAsync(d_Cp.p, Cp.data(), Cp.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    DevBuf<float> d_V((size_t)std::max<long long>(M, 1) * f->ldv);
    PROFILED(c, NLE_K_PROJECT, nlek::ts_gemm(c->stream, false, d_phi.p, ny.ldr, nullptr, ss.gs, nullptr, 0.f, 0.f, 0,
                                             d_Cp.p, f->ldv, ny.r, d_V.p, f->ldv, M, d_u_c.p, NLE_EPS));
    scatter_sample_rows(c, ss.pix, o.q, o.VArows, o.K, f->ldv, pix0, M, d_V.p);
    tm_p.stop();
    HIP_OK(hipStreamSynchronize(c->stream));
    f->V = std::move(d_V);
}

// (1b) the same literal decomposition with Phi and V in fp64 (generic64.hip): what auto mode falls back to when the
// table form does not apply, and what the 1e-4 bar needs on inputs whose detail layers are small differences
void TrainPath::train_generic64(const Nystrom& ny) {
    tm_s.start();
    const size_t phi_elems = (size_t)std::max<long long>(M, 1) * ny.ldr;
    size_t free_b = 0, total_b = 0;
    const bool no_fit = hipMemGetInfo(&free_b, &total_b) == hipSuccess && phi_elems * sizeof(double) > free_b + c->arena_bytes;
    if (ranks_where(c, no_fit) > 0)  // refused on every rank if it does not fit on one (nobody is left in a collective)
        throw Fail{NLE_ERR_INVALID, "fp64 formulation: Phi (N x r doubles) does not fit in device memory; use an integer-valued "
                                    "luminance plane with a sample grid of at most 32 x 36 (table formulation) or NLE_MODE_MATERIALISED"};
    DevBuf<double> d_phi(phi_elems);
    build_phi64(c, d_lum, ss, ny, hx, hy, pix0, M, d_phi.p);
    std::vector<double> u_c, u_r;
    DevBuf<double> d_u_c(ny.ldr);
    sinkhorn_passes(c, d_phi.p, M, ny.ldr, ny.r, ny.lam, T, &u_c, &u_r, d_u_c.p);
    tm_s.stop();
    tm_g.start();
    std::vector<double> G = gram_all(c, d_phi.p, M, ny.ldr, ny.r, d_u_c.p);
    tm_g.stop();
    double h0 = now_ms();
    Ortho o = orthogonalize_host(ny, ss.p, u_c, u_r, std::move(G), n_eig, /*device_f32=*/false, c->topk_solver, c->sw.trace);
    *host_ms += now_ms() - h0;
    adopt_ortho(f, o);
    f->formulation = NLE_MODE_MATERIALISED_F64;
    tm_p.start();
    DevBuf<double> d_Cp(o.Cproj.size()), d_cs((size_t)std::max<long long>(M, 1));  // Cproj: r x K column-major
    HIP_OK(hipMemcpyAsync(d_Cp.p, o.Cproj.data(), o.Cproj.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    PROFILED(c, NLE_K_SMALL, nlek::row_scalings64(c->stream, d_phi.p, M, ny.ldr, ny.r, d_u_c.p, NLE_EPS, d_cs.p));
    DevBuf<double> d_V((size_t)std::max<long long>(M, 1) * f->ldv);
    HIP_OK(hipMemsetAsync(d_V.p, 0, d_V.n * sizeof(double), c->stream));
    PROFILED(c, NLE_K_PROJECT, nlek::ts_gemm64(c->stream, d_phi.p, M, ny.ldr, ny.r, d_Cp.p, o.K, d_cs.p, d_V.p, f->ldv));
    scatter_sample_rows(c, ss.pix, o.q, o.VArows, o.K, f->ldv, pix0, M, d_V.p);  // exact rows of the A block (top of :327)
    tm_p.stop();
    HIP_OK(hipStreamSynchronize(c->stream));
    f->V64 = std::move(d_V);
}

}  // namespace nlep

namespace {
// nle_table_*: the TableView the table path's launchers take (tables.hip), made one of two ways.  Supplied: the caller's
// tables on the device, no sorted rows, all 16 level tiles -- what the library runs beyond sorted_max_width() columns.
// Built: a TableFilter constructed as train_tables constructs it (fetch_samples with the level check, hist_tables, sorted
// rows, level-tile range, bandwidth predicates); the caller's row scalings, where given, are copied into it.
struct TableArgs {
    const float* d_lum;
    int H, W, nRow, nCol, row0, row1;
    double hx, hy;
    const double *d_er, *d_ecT, *d_Ep, *d_cvec;
};
struct TableStage {
    std::unique_ptr<TableFilter> built;
    nlek::TableView view{};
};
TableStage table_stage(nle_ctx* ctx, const TableArgs& a) {
    const GridSpec gs = checked_grid(a.H, a.W, a.nRow, a.nCol);
    if (a.row0 < 0 || a.row1 <= a.row0 || a.row1 > a.H) throw Fail{NLE_ERR_INVALID, "need 0 <= row0 < row1 <= H"};
    if (gs.nSelRows > 32) throw Fail{NLE_ERR_INVALID, "the table kernels take at most 32 sample rows, got " + std::to_string(gs.nSelRows)};
    if (gs.nSelCols > 36) throw Fail{NLE_ERR_INVALID, "the table kernels take at most 36 sample columns, got " + std::to_string(gs.nSelCols)};
    HIP_OK(hipSetDevice(ctx->device));
    TableStage st;
    const int nrows = a.row1 - a.row0;
    if (a.d_er || a.d_ecT || a.d_Ep) {
        if (!a.d_er || !a.d_ecT || !a.d_Ep) throw Fail{NLE_ERR_INVALID, "supplied tables: er, ecT and Ep go together"};
        // the pixel kernels index their LDS tables with the level: the local rows must hold levels, as a built view's do
        DevBuf<int> d_flag(2);
        int fl[2] = {1, 0};
        PROFILED(ctx, NLE_K_SMALL, nlek::check_levels(ctx->stream, a.d_lum + (size_t)a.row0 * a.W, (long long)nrows * a.W, d_flag.p));
        HIP_OK(hipMemcpyAsync(fl, d_flag.p, sizeof fl, hipMemcpyDeviceToHost, ctx->stream));
        HIP_OK(hipStreamSynchronize(ctx->stream));
        if (fl[0] != 0) throw Fail{NLE_ERR_INVALID, "the table kernels need local rows that are integer valued in [0, 255]"};
        st.view = nlek::TableView{a.d_lum, gs,     gs.p(),  nlek::sink_pass_ld(gs.p()), a.row0, nrows,
                                  a.d_er,  a.d_ecT, a.d_Ep, a.d_cvec,                   nullptr};
        return st;
    }
    if (!(a.hx > 0) || !(a.hy > 0)) throw Fail{NLE_ERR_INVALID, "hx and hy must be > 0"};
    FetchSpec spec;
    spec.check_levels = true;
    const SampleSet ss = fetch_samples(ctx, a.d_lum, gs, AffinityOpts{}, spec);
    if (!ss.quantised) throw Fail{NLE_ERR_INVALID, "the table formulation needs a plane that is integer valued in [0, 255]"};
    st.built = std::make_unique<TableFilter>(ctx, a.d_lum, ss, a.hx, a.hy, a.row0, nrows);
    if (a.d_cvec)
        HIP_OK(hipMemcpyAsync(st.built->c.p, a.d_cvec, st.built->c.n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    st.view = st.built->view();
    return st;
}
// the sentinel of the nle_table_* entry points: every byte 0xff is a NaN in fp64 and in fp32
template <typename T>
void fill_nan(nle_ctx* ctx, T* d, size_t n) {
    if (d && n) HIP_OK(hipMemsetAsync(d, 0xff, n * sizeof(T), ctx->stream));
}
void drain(nle_ctx* ctx) {
    HIP_OK(hipStreamSynchronize(ctx->stream));
    prof_flush(ctx);
}
}  // namespace

// ------------------------------------------------------------------------------ C ABI
extern "C" {

int nle_compute_kernel(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples,
                       double hx, double hy, double* h_Ka, float* d_kab) {
    if (!ctx || !d_lum) return NLE_ERR_INVALID;
    return guard(ctx, [&] { compute_kernel_impl(ctx, d_lum, H, W, n_row_samples, n_col_samples, hx, hy, h_Ka, d_kab); });
}

int nle_nystrom(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, double hx,
                double hy, double* h_eigvals, int* r, float* d_phi) {
    if (!ctx || !d_lum || !d_phi || !r) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        const GridSpec gs = checked_grid(H, W, n_row_samples, n_col_samples);
        check_affinity_opts(ctx, affinity_opts(ctx), gs, H, W, hx, hy, Caller::NYSTROM32);
        HIP_OK(hipSetDevice(ctx->device));
        SampleSet ss = fetch_samples(ctx, d_lum, gs, AffinityOpts{});
        std::vector<double> Ka = build_Ka(ss, hx, hy);
        Nystrom ny = solve_Ka(nullptr, ctx->sw, Ka, ss.p, false);
        int row0, row1;
        slab(H, ctx->rank, ctx->world, &row0, &row1);
        build_phi(ctx, d_lum, ss, ny, hx, hy, (long long)row0 * W, (long long)(row1 - row0) * W, d_phi);
        *r = ny.r;
        if (h_eigvals) std::copy(ny.lam.begin(), ny.lam.end(), h_eigvals);
    });
}

int nle_ts_gemm(nle_ctx* ctx, const float* d_A, long long M, int lda, int kd, const double* h_B, int nc, float* d_C) {
    if (!ctx || !d_A || !h_B || !d_C || M < 0 || kd < 1 || nc < 1 || lda < kd || (lda & 3)) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        HIP_OK(hipSetDevice(ctx->device));
        const int ldc = ld4(nc);
        std::vector<float> B((size_t)kd * ldc, 0.f);
        for (int j = 0; j < nc; ++j)
            for (int k = 0; k < kd; ++k) B[(size_t)k * ldc + j] = (float)h_B[(size_t)j * kd + k];
        DevBuf<float> d_B(B.size());
        HIP_OK(hipMemcpyAsync(d_B.p, B.data(), B.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        GridSpec gs{};
        HIP_OK(nlek::ts_gemm(ctx->stream, false, d_A, lda, nullptr, gs, nullptr, 0.f, 0.f, 0, d_B.p, ldc, kd, d_C, ldc,
                             M, nullptr, NLE_EPS));
        HIP_OK(hipStreamSynchronize(ctx->stream));
    });
}

int nle_sinkhorn_scalings(nle_ctx* ctx, const float* d_phi, long long M, int ld, int r, const double* h_eigvals,
                          int max_iter, double* h_u_c, double* h_u_r) {
    if (!ctx || !d_phi || !h_eigvals || !h_u_c || !h_u_r || M < 0 || r < 1 || ld < r || (ld & 3)) return NLE_ERR_INVALID;
    return guard(ctx, [&] { sinkhorn_scalings_impl(ctx, d_phi, M, ld, r, h_eigvals, max_iter, h_u_c, h_u_r); });
}

int nle_gram(nle_ctx* ctx, const float* d_phi, long long M, int ld, int r, const double* h_u, double* h_G) {
    if (!ctx || !d_phi || !h_G || M < 0 || r < 1 || ld < r || (ld & 3)) return NLE_ERR_INVALID;
    return guard(ctx, [&] { gram_impl(ctx, d_phi, M, ld, r, h_u, h_G); });
}

int nle_row_scalings(nle_ctx* ctx, const float* d_phi, long long M, int ld, int r, const double* h_u, double* d_out) {
    if (!ctx || !d_phi || !h_u || !d_out || M < 0 || r < 1 || ld < r || (ld & 3)) return NLE_ERR_INVALID;
    return guard(ctx, [&] { row_scalings_impl(ctx, d_phi, M, ld, r, h_u, d_out); });
}

// ---- the same five stage entry points on fp64 device matrices (generic64.hip) ----
int nle_compute_kernel64(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, double hx,
                         double hy, double* h_Ka, double* d_kab) {
    if (!ctx || !d_lum) return NLE_ERR_INVALID;
    return guard(ctx, [&] { compute_kernel_impl(ctx, d_lum, H, W, n_row_samples, n_col_samples, hx, hy, h_Ka, d_kab); });
}

int nle_nystrom_residual(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, double hx, double hy,
                         int form, double thresh, float* d_r, double* h_summary) {
    if (!ctx) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        nystrom_residual_impl(ctx, d_lum, H, W, n_row_samples, n_col_samples, hx, hy, form, thresh, d_r, h_summary);
    });
}

int nle_ts_gemm64(nle_ctx* ctx, const double* d_A, long long M, int lda, int kd, const double* h_B, int nc, double* d_C) {
    if (!ctx || !d_A || !h_B || !d_C || M < 0 || kd < 1 || nc < 1 || lda < kd) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        HIP_OK(hipSetDevice(ctx->device));
        const int ldc = ld4(nc);
        DevBuf<double> d_B((size_t)kd * nc);
        HIP_OK(hipMemcpyAsync(d_B.p, h_B, (size_t)kd * nc * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIP_OK(hipMemsetAsync(d_C, 0, (size_t)std::max<long long>(M, 0) * ldc * sizeof(double), ctx->stream));
        HIP_OK(nlek::ts_gemm64(ctx->stream, d_A, M, lda, kd, d_B.p, nc, nullptr, d_C, ldc));
        HIP_OK(hipStreamSynchronize(ctx->stream));
    });
}

int nle_sinkhorn_scalings64(nle_ctx* ctx, const double* d_phi, long long M, int ld, int r, const double* h_eigvals,
                            int max_iter, double* h_u_c, double* h_u_r) {
    if (!ctx || !d_phi || !h_eigvals || !h_u_c || !h_u_r || M < 0 || r < 1 || ld < r) return NLE_ERR_INVALID;
    return guard(ctx, [&] { sinkhorn_scalings_impl(ctx, d_phi, M, ld, r, h_eigvals, max_iter, h_u_c, h_u_r); });
}

int nle_gram64(nle_ctx* ctx, const double* d_phi, long long M, int ld, int r, const double* h_u, double* h_G) {
    if (!ctx || !d_phi || !h_G || M < 0 || r < 1 || ld < r) return NLE_ERR_INVALID;
    return guard(ctx, [&] { gram_impl(ctx, d_phi, M, ld, r, h_u, h_G); });
}

int nle_row_scalings64(nle_ctx* ctx, const double* d_phi, long long M, int ld, int r, const double* h_u, double* d_out) {
    if (!ctx || !d_phi || !h_u || !d_out || M < 0 || r < 1 || ld < r) return NLE_ERR_INVALID;
    return guard(ctx, [&] { row_scalings_impl(ctx, d_phi, M, ld, r, h_u, d_out); });
}

// ---- the sample-space stages (fused.hip), each alone: the launchers of train_phi_free_exp, SampleSinkhorn and ensure_V ----
int nle_sample_pass(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, double hx, double hy,
                    int row0, int row1, int recip, const double* h_w, double* d_y, double* h_z) {
    if (!ctx || !d_lum || !h_z) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        const SampleStage st = sample_stage(ctx, d_lum, H, W, n_row_samples, n_col_samples, hx, hy, row0, row1,
                                            nlek::sink_pass_max_p(), "nle_sample_pass: the pass kernel takes at most 256 samples");
        const int p = st.ss.p, P64 = nlek::sink_pass_ld(p);
        constexpr int kZS = 8;  // as train_phi_free_exp: slices of the block partials, added in order (k_sink_update_a's loop)
        const int npart = nlek::sink_pass_rows(st.M);
        std::vector<double> w(P64, 0.0), z((size_t)kZS * P64);
        if (h_w) std::copy(h_w, h_w + p, w.begin());
        DevBuf<double> d_w = uploaded(ctx, w.data(), w.size()), d_z(z.size()), d_partial((size_t)npart * P64);
        PROFILED(ctx, NLE_K_SINKHORN_PASS,
                 nlek::sink_pass(ctx->stream, recip ? nlek::ROWPASS_RECIP : nlek::ROWPASS_COLSUM, d_lum, st.ss.gs, st.d_samples.p, p,
                                 d_w.p, st.nsw, st.npw, st.pix0, st.M, NLE_EPS, d_y, d_partial.p));
        PROFILED(ctx, NLE_K_REDUCE, nlek::reduce_partials(ctx->stream, d_partial.p, npart, P64, d_z.p, kZS));
        HIP_OK(hipMemcpyAsync(z.data(), d_z.p, z.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_OK(hipStreamSynchronize(ctx->stream));
        prof_flush(ctx);
        for (int a = 0; a < p; ++a) {
            double t = 0.0;
            for (int q = 0; q < kZS; ++q) t += z[(size_t)q * P64 + a];
            h_z[a] = t;
        }
    });
}

int nle_sample_gram(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, double hx, double hy,
                    int row0, int row1, const double* d_c, double* h_G) {
    if (!ctx || !d_lum || !d_c || !h_G) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        const SampleStage st = sample_stage(ctx, d_lum, H, W, n_row_samples, n_col_samples, hx, hy, row0, row1,
                                            nlek::sink_pass_max_p(), "nle_sample_gram: the Gram kernel takes at most 256 samples");
        const int p = st.ss.p;
        std::vector<double> tiles((size_t)nlek::gram64_num_tiles(p) * 256);
        DevBuf<double> d_gpart(nlek::gram64_partial_elems(st.M, p)), d_tiles(tiles.size());
        PROFILED(ctx, NLE_K_GRAM, nlek::gram64(ctx->stream, d_lum, st.ss.gs, st.d_samples.p, p, st.nsw, st.npw, st.pix0, st.M, d_c,
                                               d_gpart.p, d_tiles.p));
        HIP_OK(hipMemcpyAsync(tiles.data(), d_tiles.p, tiles.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_OK(hipStreamSynchronize(ctx->stream));
        prof_flush(ctx);
        const std::vector<double> G = unpack_tiles(tiles, nlek::gram64_ld(p), p, 16);
        std::copy(G.begin(), G.end(), h_G);
    });
}

int nle_sample_project(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, double hx,
                       double hy, int row0, int row1, const double* h_D, int K, const double* d_c, float* d_V, int ldv) {
    if (!ctx || !d_lum || !h_D || !d_c || !d_V || K < 1) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        if (K > 128) throw Fail{NLE_ERR_INVALID, "nle_sample_project: the projection kernel takes at most 128 columns"};
        if (ldv < K || ldv > nlek::project64_ld(K)) throw Fail{NLE_ERR_INVALID, "nle_sample_project: need K <= ldv <= 16 ceil(K / 16)"};
        const SampleStage st = sample_stage(ctx, d_lum, H, W, n_row_samples, n_col_samples, hx, hy, row0, row1, 32 * 36,
                                            "nle_sample_project: at most 32 x 36 samples");
        const int p = st.ss.p;
        std::vector<double> X((size_t)p * K);  // column-major, as the orthogonalisation leaves D
        for (int k = 0; k < K; ++k)
            for (int a = 0; a < p; ++a) X[(size_t)k * p + a] = h_D[(size_t)a * K + k];
        const std::vector<double> Dp = padded_rows(X, p, K, nlek::project64_ld(K));
        DevBuf<double> d_D = uploaded(ctx, Dp.data(), Dp.size());
        PROFILED(ctx, NLE_K_PROJECT, nlek::project64(ctx->stream, d_lum, st.ss.gs, st.d_samples.p, p, st.nsw, st.npw, st.pix0, st.M,
                                                     d_D.p, K, d_c, d_V, ldv));
        HIP_OK(hipStreamSynchronize(ctx->stream));
        prof_flush(ctx);
    });
}

int nle_sample_update(nle_ctx* ctx, int p, int r, int chol, int recip, const double* h_X1, const double* h_X2,
                      const double* h_lam, const double* h_z, int zrows, int zld, const double* h_sA, double* h_v, double* h_u,
                      double* h_sA_next, double* h_w_next) {
    if (!ctx || !h_X1 || !h_X2 || !h_lam || !h_z || !h_v || !h_u || !h_sA_next || !h_w_next || p < 1 || r < 1 || zrows < 1 ||
        zld < p || (recip && !h_sA) || (chol && r != p))
        return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        HIP_OK(hipSetDevice(ctx->device));
        const size_t n2 = (size_t)2 * p;
        DevBuf<double> d_X1 = uploaded(ctx, h_X1, n2 * r), d_X2 = uploaded(ctx, h_X2, n2 * r), d_lam = uploaded(ctx, h_lam, (size_t)r),
                       d_z = uploaded(ctx, h_z, (size_t)zrows * zld), d_sA, d_uv(n2 + r), d_out(n2);
        if (recip) d_sA = uploaded(ctx, h_sA, (size_t)p);
        PROFILED(ctx, NLE_K_SMALL,
                 nlek::sink_update(ctx->stream, recip ? nlek::ROWPASS_RECIP : nlek::ROWPASS_COLSUM, p, r, chol != 0, d_X1.p, d_X2.p,
                                   d_lam.p, d_z.p, zrows, zld, d_sA.p, NLE_EPS, d_uv.p, d_uv.p + n2, d_out.p, d_out.p + p));
        HIP_OK(hipMemcpyAsync(h_v, d_uv.p, n2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_OK(hipMemcpyAsync(h_u, d_uv.p + n2, r * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_OK(hipMemcpyAsync(h_sA_next, d_out.p, p * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_OK(hipMemcpyAsync(h_w_next, d_out.p + p, p * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_OK(hipStreamSynchronize(ctx->stream));
        prof_flush(ctx);
    });
}

// ---- the table path's stages (tables.hip), each alone: the launchers train_tables and apply_sample_space call.  Every
// workspace and output is filled with the NaN sentinel before the launch ----
#define NLE_TABLE_PARAMS                                                                                                    \
    nle_ctx *ctx, const float *d_lum, int H, int W, int n_row_samples, int n_col_samples, int row0, int row1, double hx,   \
        double hy, const double *d_er, const double *d_ecT, const double *d_Ep, const double *d_cvec
#define NLE_TABLE_ARGS TableArgs{d_lum, H, W, n_row_samples, n_col_samples, row0, row1, hx, hy, d_er, d_ecT, d_Ep, d_cvec}

long long nle_table_workspace(int n_sel_rows, int n_sel_cols, int nrows, int gram) {
    if (n_sel_rows < 1 || n_sel_rows > 32 || n_sel_cols < 1 || n_sel_cols > 36 || nrows < 1) return -1;
    GridSpec gs{};
    gs.nSelRows = n_sel_rows, gs.nSelCols = n_sel_cols;
    return (long long)(gram ? nlek::ghist_workspace_elems(gs, nrows) : nlek::hist_tiled_workspace_elems(gs, nrows));
}

int nle_table_levels(nle_ctx* ctx, const float* d_x, long long n, int* h_bad, unsigned* h_mask) {
    if (!ctx || !d_x || n < 1 || !h_bad || !h_mask) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        HIP_OK(hipSetDevice(ctx->device));
        DevBuf<int> d_flag(2);
        int fl[2] = {0, 0};
        PROFILED(ctx, NLE_K_SMALL, nlek::check_levels(ctx->stream, d_x, n, d_flag.p));
        HIP_OK(hipMemcpyAsync(fl, d_flag.p, sizeof fl, hipMemcpyDeviceToHost, ctx->stream));
        drain(ctx);
        *h_bad = fl[0], *h_mask = (unsigned)fl[1];
    });
}

int nle_table_build(NLE_TABLE_PARAMS, double* d_er_out, double* d_ecT_out, double* d_Ep_out, int* h_info) {
    if (!ctx || !d_lum || !h_info) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        const TableStage st = table_stage(ctx, NLE_TABLE_ARGS);
        const nlek::TableView& v = st.view;
        h_info[0] = v.sorted ? 1 : 0;
        h_info[1] = v.sorted ? v.sorted->lev_t0 : 0;
        h_info[2] = v.sorted ? v.sorted->lev_nt : 16;
        h_info[3] = (v.sorted && v.sorted->E2) ? 1 : 0;
        h_info[4] = nlek::apply_layers_per_launch(v);
        const size_t n_er = (size_t)v.nrows * v.gs.nSelRows, n_ec = (size_t)v.gs.nSelCols * v.gs.W, n_ep = (size_t)256 * v.p;
        if (d_er_out) HIP_OK(hipMemcpyAsync(d_er_out, v.er, n_er * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        if (d_ecT_out) HIP_OK(hipMemcpyAsync(d_ecT_out, v.ecT, n_ec * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        if (d_Ep_out) HIP_OK(hipMemcpyAsync(d_Ep_out, v.Ep, n_ep * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        drain(ctx);
    });
}

int nle_table_pass(NLE_TABLE_PARAMS, int mode, const double* d_w, const float* d_xvec, double* d_y, double* d_ws,
                   long long ws_elems, double* d_z) {
    if (!ctx || !d_lum || !d_ws || !d_z) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        if (mode != nlek::ROWPASS_COLSUM && mode != nlek::ROWPASS_RECIP && mode != nlek::ROWPASS_XVEC)
            throw Fail{NLE_ERR_INVALID, "nle_table_pass: mode is 0 (column sum), 1 (reciprocal) or 2 (x vector)"};
        if (mode == nlek::ROWPASS_RECIP && !d_w) throw Fail{NLE_ERR_INVALID, "nle_table_pass: the reciprocal pass needs w"};
        if (mode == nlek::ROWPASS_XVEC && (!d_xvec || !d_cvec)) throw Fail{NLE_ERR_INVALID, "nle_table_pass: the x-vector pass needs x and c"};
        const TableStage st = table_stage(ctx, NLE_TABLE_ARGS);
        const nlek::TableView& v = st.view;
        const size_t need = nlek::hist_tiled_workspace_elems(v.gs, v.nrows);
        if (ws_elems < (long long)need) throw Fail{NLE_ERR_INVALID, "nle_table_pass: the workspace is smaller than nle_table_workspace says"};
        fill_nan(ctx, d_ws, need);
        fill_nan(ctx, d_z, (size_t)v.ldp);
        fill_nan(ctx, d_y, (size_t)v.nrows * v.gs.W);
        ProfObserver obs(ctx, kProfTablePass);
        HIP_OK(nlek::sink_hist_tiled(ctx->stream, mode, v, d_w, NLE_EPS, d_y, d_ws, d_z, &obs, d_xvec));
        drain(ctx);
    });
}

int nle_table_expand(NLE_TABLE_PARAMS, const double* d_wl, int ldw, int nl, int round8, double* d_gws, float* d_out,
                     long long ostride) {
    if (!ctx || !d_lum || !d_wl || !d_gws || !d_out || !d_cvec) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        const TableStage st = table_stage(ctx, NLE_TABLE_ARGS);
        const nlek::TableView& v = st.view;
        const int lmax = nlek::apply_layers_per_launch(v);
        if (nl < 1 || nl > lmax)
            throw Fail{NLE_ERR_INVALID, "nle_table_expand: one launch takes 1 .. " + std::to_string(lmax) + " layers on this grid, got " + std::to_string(nl)};
        if (ldw < v.p || ostride < (long long)v.nrows * v.gs.W) throw Fail{NLE_ERR_INVALID, "nle_table_expand: need ldw >= p and ostride >= nrows W"};
        fill_nan(ctx, d_gws, (size_t)nl * v.nrows * 256 * v.gs.nSelCols);
        fill_nan(ctx, d_out, (size_t)nl * ostride);
        ProfObserver obs(ctx, kProfTableExpand);
        HIP_OK(nlek::apply_hist_layers(ctx->stream, v, d_wl, ldw, nl, d_gws, d_out, ostride, &obs, round8 != 0));
        drain(ctx);
    });
}

int nle_table_gram(NLE_TABLE_PARAMS, double* d_ws, long long ws_elems, double* d_Gk, int* h_split) {
    if (!ctx || !d_lum || !d_cvec || !d_ws || !d_Gk || !h_split) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        const TableStage st = table_stage(ctx, NLE_TABLE_ARGS);
        const nlek::TableView& v = st.view;
        const size_t need = nlek::ghist_workspace_elems(v.gs, v.nrows);
        if (ws_elems < (long long)need) throw Fail{NLE_ERR_INVALID, "nle_table_gram: the workspace is smaller than nle_table_workspace says"};
        fill_nan(ctx, d_ws, need);
        fill_nan(ctx, d_Gk, (size_t)v.p * v.p);
        nlek::gram_hist_split(v, &h_split[0], &h_split[1]);
        ProfObserver obs(ctx, kProfTableGram);
        HIP_OK(nlek::gram_hist(ctx->stream, v, d_ws, d_Gk, &obs));
        drain(ctx);
    });
}
#undef NLE_TABLE_PARAMS
#undef NLE_TABLE_ARGS

int nle_table_apply_small(nle_ctx* ctx, int p, int K, int ldk, int L, int ldw, const double* d_m, const double* d_D,
                          const double* d_Vrows, const double* d_xA, const double* d_resp, double* d_t, double* d_Wp, double* d_YA,
                          const int* d_differs, const double* d_m_same, const double* d_xA_same) {
    if (!ctx || !d_m || !d_D || !d_Vrows || !d_xA || !d_resp || !d_t || !d_Wp || !d_YA) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        if (K > 128) throw Fail{NLE_ERR_INVALID, "nle_table_apply_small: at most 128 eigenvectors, got " + std::to_string(K)};
        if (p < 1 || p > 32 * 36 || K < 1 || L < 1 || ldk < K || ldw < p)
            throw Fail{NLE_ERR_INVALID, "nle_table_apply_small: need 1 <= p <= 32 x 36, 1 <= K <= ldk, L >= 1, ldw >= p"};
        if (d_differs && (!d_m_same || !d_xA_same)) throw Fail{NLE_ERR_INVALID, "nle_table_apply_small: the flag needs the vectors it selects"};
        HIP_OK(hipSetDevice(ctx->device));
        fill_nan(ctx, d_t, (size_t)K);
        fill_nan(ctx, d_Wp, (size_t)L * ldw);
        fill_nan(ctx, d_YA, (size_t)L * p);
        PROFILED(ctx, NLE_K_SMALL, nlek::apply_small(ctx->stream, p, K, ldk, L, ldw, d_m, d_D, d_Vrows, d_xA, d_resp, d_t, d_Wp, d_YA,
                                                     d_differs, d_m_same, d_xA_same));
        drain(ctx);
    });
}

int nle_table_scatter(nle_ctx* ctx, int p, int L, const long long* d_loc, const double* d_YA, float* d_Y, long long ystride,
                      int round8) {
    if (!ctx || !d_loc || !d_YA || !d_Y || p < 1 || L < 1 || ystride < 1) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        HIP_OK(hipSetDevice(ctx->device));
        PROFILED(ctx, NLE_K_SMALL, nlek::scatter_samples(ctx->stream, p, L, d_loc, d_YA, d_Y, ystride, round8 != 0));
        drain(ctx);
    });
}

int nle_gemm64s(nle_ctx* ctx, int m, int n, int kk, const double* d_A, long long rs_a, long long cs_a, const double* d_B,
                long long rs_b, long long cs_b, double* d_C, long long rs_c, long long cs_c, const double* d_dl,
                const double* d_dk, const double* d_dr, const double* d_add, long long rs_add, long long cs_add) {
    if (!ctx || !d_A || !d_B || !d_C || m < 0 || n < 0 || kk < 0) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        HIP_OK(hipSetDevice(ctx->device));
        HIP_OK(nlek::gemm64s(ctx->stream, m, n, kk, d_A, rs_a, cs_a, d_B, rs_b, cs_b, d_C, rs_c, cs_c, d_dl, d_dk, d_dr, d_add,
                             rs_add, cs_add));
        HIP_OK(hipStreamSynchronize(ctx->stream));
    });
}

int nle_gemm64s_window(void) { return nlek::gemm64s_window(); }

int nle_bench_affinity(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, double hx,
                       double hy, float* d_kab, int reps, double* h_avg_ms) {
    if (!ctx || !d_lum || !d_kab || reps < 1 || !h_avg_ms) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        int row0, row1;
        const SampleSet ss = bench_samples(ctx, d_lum, H, W, n_row_samples, n_col_samples, &row0, &row1);
        DevBuf<float4> d_samples = upload_samples(ctx, ss);
        const float sw = nsw_of(hx), pw = nsw_of(hy);
        const long long pix0 = (long long)row0 * W, M = (long long)(row1 - row0) * W;
        *h_avg_ms = bench_ms(ctx, reps, [&] {
            return nlek::affinity(ctx->stream, d_lum, ss.gs, d_samples.p, ss.p, ld4(ss.p), sw, pw, pix0, M, d_kab);
        });
    });
}

int nle_bench_affinity64(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, double hx,
                         double hy, long long rows, double* d_kab, int reps, double* h_avg_ms) {
    if (!ctx || !d_lum || !d_kab || reps < 1 || !h_avg_ms || rows < 1) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        int row0, row1;
        const SampleSet ss = bench_samples(ctx, d_lum, H, W, n_row_samples, n_col_samples, &row0, &row1);  // k_affinity64<false>
        const AffinityRows64 kab(ctx, d_lum, ss, hx, hy, /*want_mask=*/false);
        const long long pix0 = (long long)row0 * W, M = std::min<long long>(rows, row1 - row0) * W;
        *h_avg_ms = bench_ms(ctx, reps, [&] { return kab.rows(pix0, M, d_kab, true); });
    });
}

int nle_bench_sinkhorn_pass(nle_ctx* ctx, const float* d_phi, long long M, int ld, int r, int reps, double* h_avg_ms) {
    if (!ctx || !d_phi || reps < 1 || !h_avg_ms || M < 1 || r < 1 || ld < r || (ld & 3)) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        HIP_OK(hipSetDevice(ctx->device));
        std::vector<double> ones(ld, 1.0);
        DevBuf<double> d_lam(ld), d_t(ld), d_partial((size_t)nlek::kRowpassMaxBlocks * ld);
        HIP_OK(hipMemcpyAsync(d_lam.p, ones.data(), ld * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIP_OK(hipMemcpyAsync(d_t.p, ones.data(), ld * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        int nb = 0;
        *h_avg_ms = bench_ms(ctx, reps, [&] {
            return nlek::rowpass(ctx->stream, nlek::ROWPASS_RECIP, d_phi, M, ld, d_t.p, d_lam.p, nullptr, NLE_EPS, d_partial.p, &nb);
        });
    });
}

}  // extern "C"
