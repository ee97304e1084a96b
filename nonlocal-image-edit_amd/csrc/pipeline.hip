// Host orchestration of the hot path behind the C ABI (include/nle.h): the Nystrom solve, the checks and the dispatch of
// train (NLEFilter::trainFilter, reference src/filter.cpp:480-502), apply (:445-458) and the train, filter, apply, host-buffer
// and region entry points.  The train paths themselves are literal.hip's, sample_space.hip's and exact_train.hip's (train.h).
// Small (p x p, r x r) algebra and the three symmetric eigensolves run on the host in fp64; everything N-sized is a HIP
// kernel.  The sample set, Ka and the fp64 affinity rows -- the patch, chroma and sampler options -- are samples.hip's.
#include <numeric>

#include "train.h"

using namespace nlep;

namespace nlep {

GridSpec checked_grid(int H, int W, int nRow, int nCol) {
    check_image_size(H, W);
    if (nRow > H || nCol > W)  // reference src/filter.cpp:117-119
        throw Fail{NLE_ERR_INVALID, "Number of samples per row and col must be <= that of image."};
    GridSpec gs;
    if (!make_grid(H, W, nRow, nCol, &gs)) throw Fail{NLE_ERR_INVALID, "invalid sample counts"};
    return gs;
}

// What the later stages need of Ka.  The literal form is the reference's: Ka's eigenpairs with the
// cut at 1e-10 (VA = V_r, lam, B = V_r / lam).  The Phi-free path uses them only through
//   VA diag(lam) VA^T (= Ka restricted to its range),  B diag(lam) VA^T (= the projector P on that range)
//   and B diag(lam) B^T (= pinv(Ka)),
// so when Ka is provably full rank at the reference's threshold (every eigenvalue >= 1e-10, certified
// by 1 / trace(Ka^-1)) the Cholesky factor serves as well: VA = L, lam = 1, B = L^-T (P = I) -- a
// p^3/3 factorisation instead of a p x p eigensolve.  The materialised path keeps the eigenpairs.
Nystrom solve_Ka(nle_ctx* c, const nlesw::Switches& sw, const std::vector<double>& Ka, int p, bool allow_chol) {
    Nystrom n;
    if (allow_chol && !sw.force_eig) {
        if (c && use_dev_solver(sw, p) && !sw.host_ka) {  // blocked factorisation + inverse on the device (dense64.hip)
            const size_t pp = (size_t)p * p;
            auto kd = std::make_shared<KaDevice>();
            kd->Ka.alloc(pp);
            upload_staged(c, kd->Ka.p, Ka.data(), pp, c->stream);
            kd->ch.factor(c, p, kd->Ka.p);
            if (kd->ch.finish(c) && kd->ch.inv_trace <= kCholMaxInvTrace) {
                // the factors stay on the device: the table path builds the Sinkhorn update's operands from them there
                // (22 ms of host factorisation and ~28 ms of host transposes and uploads at p = 900 become ~6 ms)
                n.chol = true;
                n.r = p;
                n.ldr = ld4(p);
                n.lam.assign(p, 1.0);
                n.Ka = Ka;
                n.dev = std::move(kd);
                return n;
            }
        } else {
            std::vector<double> L((size_t)p * p), Li((size_t)p * p);
            double inv_trace = 0.0;
            if (nleh::cholesky_with_inverse(Ka.data(), p, L.data(), Li.data(), &inv_trace, kCholMaxInvTrace) &&
                inv_trace <= kCholMaxInvTrace) {
                n.chol = true;
                n.r = p;
                n.ldr = ld4(p);
                n.VA = std::move(L);
                n.lam.assign(p, 1.0);
                n.B.resize((size_t)p * p);
                for (int k = 0; k < p; ++k)
                    for (int a = 0; a < p; ++a) n.B[(size_t)k * p + a] = Li[(size_t)a * p + k];  // L^-T
                n.Ka = Ka;
                return n;
            }
        }
    }
    // nystromApproximation, reference src/filter.cpp:262-271
    std::vector<double> U((size_t)p * p), D(p);
    int r = 0;
    if (!nleh::eigen_decomposition(Ka.data(), p, NLE_EPS, U.data(), D.data(), &r))
        throw Fail{NLE_ERR_NUMERIC, "eigensolver did not converge on Ka"};
    int nnz = 0;
    for (int k = 0; k < r; ++k)
        if (std::fabs(D[k]) >= NLE_EPS) ++nnz;  // inplaceReciprocal count (:266)
    r = std::min(r, nnz);
    if (r <= 0) throw Fail{NLE_ERR_NUMERIC, "Ka has no eigenvalue >= 1e-10"};
    n.r = r;
    n.ldr = ld4(r);
    n.VA.assign(U.begin(), U.begin() + (size_t)p * r);
    n.lam.assign(D.begin(), D.begin() + r);
    n.B.resize((size_t)p * r);
    for (int k = 0; k < r; ++k) {
        const double inv = recip0(n.lam[k]);  // :265-268
        for (int a = 0; a < p; ++a) n.B[(size_t)k * p + a] = n.VA[(size_t)k * p + a] * inv;
    }
    return n;
}

std::unique_ptr<nle_filter> begin_train(nle_ctx* c, int H, int W, double* t_begin) {
    auto f = std::make_unique<nle_filter>();
    f->ctx = c, f->H = H, f->W = W;
    slab(H, c->rank, c->world, &f->row0, &f->row1);
    f->n_local = (long long)(f->row1 - f->row0) * W;
    if (f->n_local <= 0) throw Fail{NLE_ERR_INVALID, "a rank without image rows"};  // (world <= H: cannot happen; the paths rely on it)
    *t_begin = now_ms();
    pinned_reset(c);
    return f;
}

nle_filter* end_train(std::unique_ptr<nle_filter> f, double t_begin) {
    prof_flush(f->ctx);
    f->ms[5] = now_ms() - t_begin;
    f->ctx->filters.insert(f.get());
    return f.release();
}

}  // namespace nlep

namespace {

// The refusal of a plane that does not have the training image's size, with the reference's text (src/filter.cpp:447-449).
// each_positive: H and W are looked at one by one as well (the entry points that take them from the caller)
void check_plane_size(const nle_filter* f, int H, int W, bool each_positive) {
    if ((each_positive && (H <= 0 || W <= 0)) || (long long)H * W != (long long)f->H * f->W)
        throw Fail{NLE_ERR_INVALID, "Number of values in channel must match that of training image."};
}

// The refusal of an output kind that is no NLE_REGION_OUT_* (with_u8: NLE_REGION_OUT_U8 is one the caller takes).
// before: the caller's text up to the number
void check_out_kind(const std::string& before, int out_kind, bool with_u8) {
    if (out_kind == NLE_REGION_OUT_F32 || out_kind == NLE_REGION_OUT_ROUNDED8 || (with_u8 && out_kind == NLE_REGION_OUT_U8)) return;
    throw Fail{NLE_ERR_INVALID, before + std::to_string(out_kind) +
                                    (with_u8 ? " (NLE_REGION_OUT_*)" : " (NLE_REGION_OUT_F32 or NLE_REGION_OUT_ROUNDED8)")};
}

// d_lum_in: the full H x W plane, or -- ctx in slab-input mode -- this rank's rows [row0, row1) only
nle_filter* train_impl(nle_ctx* c, const float* d_lum_in, int H, int W, int nRow, int nCol, double hx,
                       double hy, int T, int n_eig) {
    const GridSpec gs = checked_grid(H, W, nRow, nCol);
    const float* d_lum = d_lum_in;
    if (c->slab_input && c->world > 1) {  // virtual base of the full image: only this rank's rows are ever dereferenced
        int r0, r1;
        slab(H, c->rank, c->world, &r0, &r1);
        d_lum = d_lum_in - (size_t)r0 * W;
    }
    if (T < 1) throw Fail{NLE_ERR_INVALID, "nSinkhornIter must be >= 1"};
    if (n_eig < 1) throw Fail{NLE_ERR_INVALID, "nEigenVectors must be >= 1"};
    if (!(hx > 0) || !(hy > 0)) throw Fail{NLE_ERR_INVALID, "hx and hy must be > 0"};
    // the exact filter takes no samples: nRow and nCol are only checked (above, as the reference checks them)
    if (c->mode == NLE_MODE_EXACT_F64) return train_exact_impl(c, d_lum_in, H, W, hx, hy, T, n_eig);
    if (gs.p() > 2048) throw Fail{NLE_ERR_INVALID, "more than 2048 samples is not supported"};
    // every rank owns at least one image row: the formulation, the collective sizes and their order are then the
    // same on all ranks (an empty slab used to take a different path and mismatch the all-reduces)
    if (c->world > H) throw Fail{NLE_ERR_INVALID, "more ranks than image rows"};
    // Phi-free needs <= 128 eigenvectors; its generic kernels need <= 256 samples, its table kernels
    // (quantised luminance, checked on the device below) a sample grid of at most 32 x 36: nlek::tables_apply
    const bool generic_ok = gs.p() <= nlek::sink_pass_max_p() && n_eig <= 128;
    const bool tables_ok = nlek::tables_apply(gs, n_eig) && c->mode != NLE_MODE_PHI_FREE_EXP;
    if (c->mode == NLE_MODE_PHI_FREE_EXP && !generic_ok)
        throw Fail{NLE_ERR_INVALID, "Phi-free path without tables supports at most 256 samples and 128 eigenvectors"};
    if (c->mode == NLE_MODE_PHI_FREE && !generic_ok && !tables_ok)
        throw Fail{NLE_ERR_INVALID, "Phi-free path supports at most 128 eigenvectors and a 32 x 36 sample grid"};
    // patch affinities, chroma affinities, the farthest sampler: every check here is decided the same way on every rank
    const AffinityOpts opts = affinity_opts(c);
    check_affinity_opts(c, opts, gs, H, W, hx, hy, Caller::TRAIN);
    // auto: the table form (all fp64) whenever it applies, else the literal decomposition in fp64 (generic64.hip).  The
    // fp32 formulations (materialised Phi, Phi-free with fp32 affinities) run only when asked for by mode: they miss
    // the 1e-4 bar on some well-posed inputs (DESIGN.md "Numerics").
    const bool want_fuse = !opts.any() && (c->mode == NLE_MODE_PHI_FREE || c->mode == NLE_MODE_PHI_FREE_EXP ||
                                           (c->mode == NLE_MODE_AUTO && tables_ok));
    HIP_OK(hipSetDevice(c->device));

    double t_begin;
    std::unique_ptr<nle_filter> owner = begin_train(c, H, W, &t_begin);
    nle_filter* f = owner.get();
    Trace tr(c->sw.trace);
    const long long pix0 = (long long)f->row0 * W, M = f->n_local;
    double host_ms = 0;
    // --- sample set, Ka and its eigenpairs (:486-491, host fp64)
    Timer tm_a(c->stream);
    tm_a.start();
    std::vector<long long> list;
    if (opts.listed()) list = sampler_list(c, d_lum, gs, hx, hy);
    FetchSpec spec;
    spec.check_levels = want_fuse && tables_ok;
    spec.slab_plane = c->slab_input && c->world > 1;
    spec.list = opts.listed() ? &list : nullptr;
    SampleSet ss = fetch_samples(c, d_lum, gs, opts, spec);
    require_integer_planes(c, ss, /*agree_over_ranks=*/true);
    f->chroma_hc = opts.chroma() ? opts.hc : 0.0;
    const bool fuse = c->mode == NLE_MODE_AUTO ? (want_fuse && tables_ok && ss.quantised)
                                               : (want_fuse && (generic_ok || (tables_ok && ss.quantised)));
    if (c->mode == NLE_MODE_PHI_FREE && !fuse)
        throw Fail{NLE_ERR_INVALID, "Phi-free path: more than 256 samples needs an integer-valued luminance plane"};
    tr.mark("fetch_samples");
    f->p = ss.p;
    f->h_sample_pix = ss.pix;
    double h0 = now_ms();
    std::vector<double> Ka = build_Ka(ss, hx, hy);
    tr.mark("build_Ka");
    host_ms += now_ms() - h0;
    auto solve = [&](bool allow_chol) {
        const double t0 = now_ms();
        Nystrom ny = solve_Ka(c, c->sw, Ka, ss.p, allow_chol);
        tr.mark(ny.chol ? "chol(Ka)" : "eig(Ka)");
        host_ms += now_ms() - t0;
        return ny;
    };
    tm_a.stop();
    // auto mode's fp64 fallback holds Phi (N x r doubles) when that fits comfortably (a pass reads it once); otherwise
    // -- and when asked for -- the streamed form, which holds nothing N x r (the ranks agree on it: ranks_where)
    bool stream64 = c->mode == NLE_MODE_STREAMED_F64;
    if (!fuse && c->mode == NLE_MODE_AUTO) {
        size_t free_b = 0, total_b = 0;
        const size_t need = (size_t)std::max<long long>(M, 1) * ld4(ss.p) * sizeof(double);
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > (free_b + c->arena_bytes) / 2) stream64 = true;
        if (c->sw.auto_stream64) stream64 = true;
        if (c->world > 1) stream64 = ranks_where(c, stream64) > 0;  // one rank short of memory: everybody streams
    }
    TrainPath path{c, f, d_lum, ss, hx, hy, T, n_eig, pix0, M, &host_ms, tr};
    if (fuse && tables_ok && ss.quantised) {
        path.train_tables([&] { return solve(true); });
    } else if (fuse) {
        path.train_phi_free_exp([&] { return solve(true); });
    } else if (stream64) {
        path.train_stream64([&] { return solve(true); });
    } else {
        const Nystrom ny = solve(false);
        f->r = ny.r;
        c->mode == NLE_MODE_MATERIALISED ? path.train_materialised(ny) : path.train_generic64(ny);
    }
    const double ms[5] = {tm_a.ms(), path.tm_s.ms(), path.tm_g.ms(), path.tm_p.ms(), host_ms};
    std::copy(ms, ms + 5, f->ms);
    tr.mark("train path");
    return end_train(std::move(owner), t_begin);
}

// t = V^T x (all ranks), then Y[l] = V (g_l o t), on a materialised V (fp32 or fp64)
template <typename T>
void apply_dense(nle_filter* f, const T* d_V, const float* d_x, const double* h_g /* L x K */, int L, float* d_y,
                 const LayersDone& done, long long ystride) {
    nle_ctx* c = f->ctx;
    const int ld = f->ldv;
    const long long M = f->n_local;
    const long long pix0 = (long long)f->row0 * f->W;
    DevBuf<double> d_partial((size_t)nlek::kRowpassMaxBlocks * ld), d_t(ld), d_resp((size_t)L * ld),
        d_g((size_t)L * ld);
    std::vector<double> resp((size_t)L * ld, 0.0);
    for (int l = 0; l < L; ++l)
        for (int k = 0; k < f->K; ++k) resp[(size_t)l * ld + k] = h_g[(size_t)l * f->K + k];
    HIP_OK(hipMemcpyAsync(d_resp.p, resp.data(), resp.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    int nb = 0;
    PROFILED(c, NLE_K_APPLY_REDUCE, rowpass_any(c->stream, nlek::ROWPASS_XVEC, d_V, M, ld, ld, nullptr, nullptr, d_x + pix0,
                                                NLE_EPS, d_partial.p, &nb));
    PROFILED(c, NLE_K_REDUCE, nlek::reduce_partials(c->stream, d_partial.p, nb, ld, d_t.p));
    all_reduce(c, d_t.p, ld);
    for (int l = 0; l < L; ++l)
        PROFILED(c, NLE_K_SMALL, nlek::scale_vec(c->stream, d_resp.p + (size_t)l * ld, d_t.p, ld, d_g.p + (size_t)l * ld));
    PROFILED(c, NLE_K_APPLY_EXPAND, apply_expand_any(c->stream, d_V, M, ld, f->K, d_g.p, L, d_y, ystride > 0 ? ystride : M));
    if (done) done(0, L);
    HIP_OK(hipStreamSynchronize(c->stream));
    prof_flush(c);
}

// round8: the planes come out clamped to [0, 255] and rounded half to even (src/filter.cpp:434-436) -- on the default path from
// the fp64 value, before anything is rounded to fp32 (other formulations: their fp32 planes, rounded by the caller)
// ystride: floats between the output layers (0: n_local)
void apply_impl(nle_filter* f, const float* d_x_in, int H, int W, const double* h_g /* L x K */, int L,
                float* d_y, const LayersDone& done = nullptr, int group = 0, bool round8 = false, long long ystride = 0) {
    nle_ctx* c = f->ctx;
    // slab-input mode: d_x_in holds this rank's rows only; index it through the virtual base of the full image
    const float* d_x = (c->slab_input && c->world > 1) ? d_x_in - (size_t)f->row0 * f->W : d_x_in;
    check_plane_size(f, H, W, false);
    if (L < 1 || L > 64) throw Fail{NLE_ERR_INVALID, "number of layers must be in [1, 64]"};
    HIP_OK(hipSetDevice(c->device));
    if (f->tables) {
        apply_sample_space(f, d_x, h_g, L, d_y, done, group, round8, ystride);
    } else if (f->V64.p) {
        apply_dense(f, f->V64.p, d_x, h_g, L, d_y, done, ystride);
    } else {
        ensure_V(f);
        apply_dense(f, f->V.p, d_x, h_g, L, d_y, done, ystride);
    }
}

// the fp32 planes of the formulations that keep V: clamp to [0, 255] and round half to even (nle_apply_rounded8's rule for them)
void round8_planes(nle_filter* f, float* d_y, int L, long long ystride) {
    DevBuf<unsigned char> d_o((size_t)std::max<long long>(f->n_local, 1));
    for (int l = 0; l < L; ++l) {
        HIP_OK(nlek::plane_to_u8(f->ctx->stream, d_y + (size_t)l * ystride, f->n_local, d_o.p));
        HIP_OK(nlek::channel8_plane(f->ctx->stream, d_o.p, f->n_local, d_y + (size_t)l * ystride));
    }
    HIP_OK(hipStreamSynchronize(f->ctx->stream));
}

// P planes, plane m with nresp[m] of the R rows of h_resp (R x K, plane 0's first), output j at d_y + j * ystride: bit for
// bit apply_impl(f, d_x[m], H, W, resp_m, nresp[m], .., round8) plane by plane (include/nle.h: nle_apply_planes).  A table
// filter with level-sorted rows on one device takes the batched path (sample_space.hip); everything else goes one by one.
void apply_planes_impl(nle_filter* f, const float* const* d_x, int P, int H, int W, const int* nresp, const double* h_resp,
                       float* d_y, long long ystride, bool round8) {
    nle_ctx* c = f->ctx;
    check_plane_size(f, H, W, false);
    int R = 0;
    for (int m = 0; m < P; ++m) R += nresp[m];
    if (P > 1 && f->tables && f->tables->sorted_rows() && c->world == 1) {
        HIP_OK(hipSetDevice(c->device));
        apply_sample_space_planes(f, d_x, P, nresp, h_resp, R, d_y, ystride, round8);
        return;
    }
    for (int m = 0, j = 0; m < P; j += nresp[m], ++m) {
        float* y = d_y + (size_t)j * ystride;
        apply_impl(f, d_x[m], H, W, h_resp + (size_t)j * f->K, nresp[m], y, nullptr, 0, round8, ystride);
        if (round8 && !f->tables) round8_planes(f, y, nresp[m], ystride);
    }
}

// t = V^T x on a materialised V (fp32 or fp64): apply_dense's row pass and fold, the first K of the ld sums handed out
template <typename T>
void coefficients_dense(nle_filter* f, const T* d_V, const float* d_x, double* h_t) {
    nle_ctx* c = f->ctx;
    const int ld = f->ldv;
    const long long M = f->n_local;
    DevBuf<double> d_partial((size_t)nlek::kRowpassMaxBlocks * ld), d_t(ld);
    int nb = 0;
    PROFILED(c, NLE_K_APPLY_REDUCE, rowpass_any(c->stream, nlek::ROWPASS_XVEC, d_V, M, ld, ld, nullptr, nullptr, d_x, NLE_EPS,
                                                d_partial.p, &nb));
    PROFILED(c, NLE_K_REDUCE, nlek::reduce_partials(c->stream, d_partial.p, nb, ld, d_t.p));
    HIP_OK(hipMemcpyAsync(h_t, d_t.p, (size_t)f->K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    prof_flush(c);
}

// nle_filter_coefficients on one device: the t of apply_impl, formulation by formulation
void coefficients_impl(nle_filter* f, const float* const* d_x, int P, double* h_t) {
    HIP_OK(hipSetDevice(f->ctx->device));
    if (f->tables) return coefficients_sample_space(f, d_x, P, h_t);
    if (!f->V64.p) ensure_V(f);
    for (int m = 0; m < P; ++m) {
        if (f->V64.p) coefficients_dense(f, f->V64.p, d_x[m], h_t + (size_t)m * f->K);
        else coefficients_dense(f, f->V.p, d_x[m], h_t + (size_t)m * f->K);
    }
}

void layer_resp(const double* ev, int K, int L, double* out) {
    // detail layer j <-> lambda^j - lambda^(j+1); base <-> lambda^(L-1)  (reference :334-347)
    for (int j = 0; j < L; ++j)
        for (int k = 0; k < K; ++k) {
            const double a = std::pow(ev[k], (double)j);
            out[(size_t)j * K + k] = (j < L - 1) ? a - std::pow(ev[k], (double)(j + 1)) : a;
        }
}

// The host plane of a train call on the device: H x W elements, or -- slab-input mode -- this rank's rows only (*npx of them)
template <typename T>
DevBuf<T> upload_train_plane(nle_ctx* ctx, const T* h_plane, int H, int W, size_t* npx) {
    check_image_size(H, W);
    HIP_OK(hipSetDevice(ctx->device));
    *npx = (size_t)H * W;
    if (ctx->slab_input && ctx->world > 1) {
        int r0, r1;
        slab(H, ctx->rank, ctx->world, &r0, &r1);
        *npx = (size_t)(r1 - r0) * W;
    }
    DevBuf<T> d_plane(std::max<size_t>(*npx, 1));
    HIP_OK(hipMemcpyAsync(d_plane.p, h_plane, *npx * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return d_plane;
}

// What the host-buffer apply entry points share before apply_impl: their two refusals, and x on the device -- h_x uploaded
// into d_xbuf, or the training plane the filter kept
const float* host_apply_input(nle_filter* f, const float* h_x, int H, int W, DevBuf<float>& d_xbuf) {
    nle_ctx* c = f->ctx;
    check_plane_size(f, H, W, false);
    if (!h_x && !f->plane.p)
        throw Fail{NLE_ERR_INVALID, "h_x == NULL needs a filter trained by nle_train_host (it keeps the training plane)"};
    HIP_OK(hipSetDevice(c->device));
    if (!h_x) return f->plane.p;
    const size_t npx = (c->slab_input && c->world > 1) ? (size_t)f->n_local : (size_t)H * W;
    d_xbuf.alloc(std::max<size_t>(npx, 1));
    HIP_OK(hipMemcpyAsync(d_xbuf.p, h_x, npx * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return d_xbuf.p;
}

// Whatever happens in a host-buffer apply (an exception out of apply_impl or of a later callback), no copy may still be
// reading a device buffer or writing the caller's when the entry point is left: the buffers go back to the ctx's cache
struct Drain {
    nle_ctx* c;
    ~Drain() {
        if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
        (void)hipStreamSynchronize(c->stream);
    }
};

void apply_host_common(nle_filter* f, const float* h_x, int H, int W, const double* g, int L, float* h_y) {
    nle_ctx* c = f->ctx;
    DevBuf<float> d_xbuf;
    const float* d_x = host_apply_input(f, h_x, H, W, d_xbuf);
    DevBuf<float> d_y((size_t)L * std::max<long long>(f->n_local, 1));
    // each finished group of layers goes home on the copy stream while the next one is computed (the copies are only
    // asynchronous when h_y is pinned: nle_host_alloc)
    if (!c->copy_stream) {
        HIP_OK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        for (auto& e : c->copy_ev) HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    int flip = 0;
    const size_t n = (size_t)f->n_local;
    Drain drain{c};
    apply_impl(f, d_x, H, W, g, L, d_y.p, [&](int l0, int nl) {
        hipEvent_t ev = c->copy_ev[flip ^= 1];
        HIP_OK(hipEventRecord(ev, c->stream));
        HIP_OK(hipStreamWaitEvent(c->copy_stream, ev, 0));
        HIP_OK(hipMemcpyAsync(h_y + (size_t)l0 * n, d_y.p + (size_t)l0 * n, (size_t)nl * n * sizeof(float),
                              hipMemcpyDeviceToHost, c->copy_stream));
    }, 1);
    HIP_OK(hipStreamSynchronize(c->copy_stream));
    // d_y returns to the ctx's cache: order its next use on the main stream behind the copies
    HIP_OK(hipStreamSynchronize(c->stream));
}

// ---- region edits (include/nle.h "region edits"; the kernel is region.hip) ----
// every refusal of the three entry points, before anything is enqueued (and so before any collective)
void region_check_combine(int L, int M, double floor, int out_kind) {
    if (L < 1 || L > NLE_REGION_LAYERS_MAX)
        throw Fail{NLE_ERR_INVALID, "region edits take 1 to " + std::to_string(NLE_REGION_LAYERS_MAX) + " layers, got " +
                                        std::to_string(L)};
    if (M < 1 || M > NLE_REGION_MAX)
        throw Fail{NLE_ERR_INVALID, "region edits take 1 to " + std::to_string(NLE_REGION_MAX) + " regions, got " +
                                        std::to_string(M)};
    if (!std::isfinite(floor) || !(floor > 0))
        throw Fail{NLE_ERR_INVALID, "the region floor must be finite and > 0, got " + std::to_string(floor)};
    check_out_kind("unknown region output kind ", out_kind, true);
}

void region_check_spread(const nle_filter* f, int M, int H, int W, const double* h_scale, double spread) {
    if (M < 1 || M > NLE_REGION_MAX)
        throw Fail{NLE_ERR_INVALID, "region edits take 1 to " + std::to_string(NLE_REGION_MAX) + " regions, got " +
                                        std::to_string(M)};
    if (!std::isfinite(spread) || !(spread > 0))
        throw Fail{NLE_ERR_INVALID, "the region spread must be finite and > 0, got " + std::to_string(spread)};
    for (int m = 0; h_scale && m < M; ++m)
        if (!std::isfinite(h_scale[m]))
            throw Fail{NLE_ERR_INVALID, "the scale of region " + std::to_string(m + 1) + " is not finite"};
    if (f->ctx->world > 1)
        throw Fail{NLE_ERR_INVALID, "region edits run on one device only (world == 1): slabs and device groups are not built"};
    check_plane_size(f, H, W, true);
}

void region_combine_impl(nle_ctx* c, const float* d_layers, int L, const float* d_q, int M, long long n, long long layer_stride,
                         long long q_stride, const double* h_weights, double floor, int out_kind, void* d_out) {
    nlek::RegionWeights wt{};
    std::copy(h_weights, h_weights + (size_t)(M + 1) * L, wt.wt);
    HIP_OK(hipSetDevice(c->device));
    HIP_OK(nlek::region_combine(c->stream, d_layers, layer_stride, L, d_q, q_stride, M, n, wt, floor, out_kind, d_out));
    HIP_OK(hipStreamSynchronize(c->stream));
}

// the responses of the spreads, fS_m[k] = c_m lambda_k^t: M rows of K at `out`
void spread_resp(const nle_filter* f, int M, const double* h_scale, double spread, double* out) {
    for (int m = 0; m < M; ++m) {
        const double cm = h_scale ? h_scale[m] : 1.0;
        for (int k = 0; k < f->K; ++k) out[(size_t)m * f->K + k] = cm * std::pow(f->eigvals[k], spread);
    }
}

// q_m = apply(s_m, c_m lambda^t): one batch over the M stroke planes, bitwise one nle_apply per plane
void region_spread_impl(nle_filter* f, const float* d_strokes, int M, int H, int W, const double* h_scale, double spread,
                        float* d_q) {
    std::vector<double> fS((size_t)M * f->K);
    spread_resp(f, M, h_scale, spread, fS.data());
    const float* planes[NLE_REGION_MAX];
    int ones[NLE_REGION_MAX];
    for (int m = 0; m < M; ++m) planes[m] = d_strokes + (size_t)m * H * W, ones[m] = 1;
    apply_planes_impl(f, planes, M, H, W, ones, fS.data(), d_q, f->n_local, false);
}

// ---- the out-of-span detail layer and the detail curve (include/nle.h at nle_detail_combine; the kernel is detail.hip) ----
// every refusal the two entry points share, before anything is enqueued
void detail_check(const char* who, int L, const double* h_weights, double w_rho, double gain, double sigma, int out_kind) {
    const std::string name(who);
    if (L < 1 || L > NLE_REGION_LAYERS_MAX)
        throw Fail{NLE_ERR_INVALID, name + " takes 1 to " + std::to_string(NLE_REGION_LAYERS_MAX) + " layers, got " +
                                        std::to_string(L)};
    if (!h_weights) throw Fail{NLE_ERR_INVALID, name + ": NULL pointer"};
    for (int l = 0; l < L; ++l)
        if (!std::isfinite(h_weights[l])) throw Fail{NLE_ERR_INVALID, name + ": weight " + std::to_string(l) + " is not finite"};
    if (!std::isfinite(w_rho)) throw Fail{NLE_ERR_INVALID, name + ": the residual weight is not finite"};
    if (!std::isfinite(gain) || gain < 0 || gain > NLE_DETAIL_GAIN_MAX)
        throw Fail{NLE_ERR_INVALID, name + ": the detail gain must be finite and in [0, " + std::to_string(NLE_DETAIL_GAIN_MAX) +
                                        "], got " + std::to_string(gain)};
    if (!std::isfinite(sigma) || sigma < 0)
        throw Fail{NLE_ERR_INVALID, name + ": the detail sigma must be finite and >= 0, got " + std::to_string(sigma)};
    check_out_kind(name + ": unknown output kind ", out_kind, true);
}

// d_out (n floats, or n bytes for NLE_REGION_OUT_U8) must not overlap the n floats at d_in
void detail_check_overlap(const char* who, const float* d_in, const void* d_out, long long n, int out_kind, const char* what) {
    const uintptr_t i0 = reinterpret_cast<uintptr_t>(d_in), i1 = i0 + (uintptr_t)n * sizeof(float);
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_out), o1 = o0 + (uintptr_t)n * (out_kind == NLE_REGION_OUT_U8 ? 1 : 4);
    if (i0 < o1 && o0 < i1) throw Fail{NLE_ERR_INVALID, std::string(who) + ": d_out overlaps " + what};
}

void detail_combine_impl(nle_ctx* c, const float* d_x, const float* d_layers, int L, long long n, long long layer_stride,
                         const double* h_weights, double w_rho, double gain, double sigma, int out_kind, void* d_out) {
    nlek::DetailWeights w{};
    std::copy(h_weights, h_weights + L, w.w);
    HIP_OK(hipSetDevice(c->device));
    HIP_OK(nlek::detail_combine(c->stream, d_x, d_layers, layer_stride, L, n, w, w_rho, gain, sigma, out_kind, d_out));
    HIP_OK(hipStreamSynchronize(c->stream));
}

// ---- the base tone curve (include/nle.h at nle_tone_combine; the kernels are tone.hip and detail.hip) ----
void tone_curve_impl(const long long* h_counts, double shadows, double highlights, double clip_percent, double equalise,
                     double* h_curve) {
    if (const char* refused = nlek::tone_curve(h_counts, shadows, highlights, clip_percent, equalise, h_curve))
        throw Fail{NLE_ERR_INVALID, refused};
}

void plane_histogram_impl(nle_ctx* c, const float* d_x, long long n, double scale, long long* h_counts) {
    HIP_OK(hipSetDevice(c->device));
    DevBuf<unsigned long long> d_counts(nlek::kToneCounts);
    PROFILED(c, NLE_K_PLANE_HIST, nlek::plane_hist(c->stream, d_x, n, scale, d_counts.p));
    HIP_OK(hipMemcpyAsync(h_counts, d_counts.p, sizeof(long long) * nlek::kToneCounts, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    prof_flush(c);
}

// what the stage combine asks of the curve it is given, before anything is enqueued
void tone_check_curve(const char* who, const double* h_curve) {
    const std::string name(who);
    if (!h_curve) throw Fail{NLE_ERR_INVALID, name + ": NULL pointer"};
    const double lo = h_curve[0], hi = h_curve[1];
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(hi - lo > 0) || !std::isfinite((double)(NLE_TONE_KNOTS - 1) / (hi - lo)))
        throw Fail{NLE_ERR_INVALID, name + ": the curve's range needs finite lo < hi, got " + std::to_string(lo) + " and " +
                                        std::to_string(hi)};
    for (int k = 0; k < NLE_TONE_KNOTS; ++k)
        if (!std::isfinite(h_curve[2 + k])) throw Fail{NLE_ERR_INVALID, name + ": knot " + std::to_string(k) + " is not finite"};
}

// the knots go to a buffer of the ctx's workspace; the call returns with the stream drained, so h_curve outlives the copy
void tone_combine_impl(nle_ctx* c, const float* d_x, const float* d_layers, int L, long long n, long long layer_stride,
                       const double* h_weights, double w_rho, double gain, double sigma, const double* h_curve, int out_kind,
                       void* d_out) {
    nlek::DetailWeights w{};
    std::copy(h_weights, h_weights + L, w.w);
    HIP_OK(hipSetDevice(c->device));
    DevBuf<double> d_knots(NLE_TONE_KNOTS);
    HIP_OK(hipMemcpyAsync(d_knots.p, h_curve + 2, sizeof(double) * NLE_TONE_KNOTS, hipMemcpyHostToDevice, c->stream));
    const double lo = h_curve[0], ks = (double)(NLE_TONE_KNOTS - 1) / (h_curve[1] - lo);
    PROFILED(c, NLE_K_TONE_COMBINE, nlek::tone_combine(c->stream, d_x, d_layers, layer_stride, L, n, w, w_rho, gain, sigma,
                                                        d_knots.p, lo, ks, out_kind, d_out));
    HIP_OK(hipStreamSynchronize(c->stream));
    prof_flush(c);
}

// ---- local adjustments (include/nle.h "local adjustments"; the kernels are local.hip) ----
// every refusal the stage combine and nle_apply_local share, before anything is enqueued: per row what nle_region_combine,
// nle_detail_combine and nle_tone_combine refuse
void local_check(const char* who, int L, int M, const double* h_weights, const double* h_detail, const int* h_curve_on,
                 const double* h_curves, double floor, int out_kind) {
    const std::string name(who);
    if (L < 1 || L > NLE_REGION_LAYERS_MAX)
        throw Fail{NLE_ERR_INVALID, name + " takes 1 to " + std::to_string(NLE_REGION_LAYERS_MAX) + " layers, got " + std::to_string(L)};
    if (M < 1 || M > NLE_REGION_MAX)
        throw Fail{NLE_ERR_INVALID, name + " takes 1 to " + std::to_string(NLE_REGION_MAX) + " regions, got " + std::to_string(M)};
    if (!h_weights || !h_detail) throw Fail{NLE_ERR_INVALID, name + ": NULL pointer"};
    if (!std::isfinite(floor) || !(floor > 0))
        throw Fail{NLE_ERR_INVALID, name + ": the region floor must be finite and > 0, got " + std::to_string(floor)};
    for (int m = 0; m <= M; ++m) {
        const std::string row = name + ": row " + std::to_string(m) + ": ";
        for (int l = 0; l < L; ++l)
            if (!std::isfinite(h_weights[(size_t)m * L + l])) throw Fail{NLE_ERR_INVALID, row + "weight " + std::to_string(l) + " is not finite"};
        const double w_rho = h_detail[3 * m], gain = h_detail[3 * m + 1], sigma = h_detail[3 * m + 2];
        if (!std::isfinite(w_rho)) throw Fail{NLE_ERR_INVALID, row + "the residual weight is not finite"};
        if (!std::isfinite(gain) || gain < 0 || gain > NLE_DETAIL_GAIN_MAX)
            throw Fail{NLE_ERR_INVALID, row + "the detail gain must be finite and in [0, " + std::to_string(NLE_DETAIL_GAIN_MAX) +
                                            "], got " + std::to_string(gain)};
        if (!std::isfinite(sigma) || sigma < 0)
            throw Fail{NLE_ERR_INVALID, row + "the detail sigma must be finite and >= 0, got " + std::to_string(sigma)};
        if (h_curve_on && h_curve_on[m]) {
            if (!h_curves) throw Fail{NLE_ERR_INVALID, name + ": NULL curves while the base curve of row " + std::to_string(m) + " is on"};
            tone_check_curve((name + ": row " + std::to_string(m)).c_str(), h_curves + (size_t)m * (NLE_TONE_KNOTS + 2));
        }
    }
    check_out_kind(name + ": unknown output kind ", out_kind, true);
}

// the curves that are on go to a buffer of the ctx's workspace, one after the other; the call returns with the stream
// drained, so the host copy outlives the upload
void local_combine_impl(nle_ctx* c, const float* d_x, const float* d_layers, int L, const float* d_q, int M, long long n,
                        long long layer_stride, long long q_stride, const double* h_weights, const double* h_detail,
                        const int* h_curve_on, const double* h_curves, double floor, int out_kind, void* d_out) {
    nlek::LocalRows rows{};
    std::copy(h_weights, h_weights + (size_t)(M + 1) * L, rows.wt);
    std::vector<double> knots;
    int ncurves = 0;
    for (int m = 0; m <= M; ++m) {
        nlek::LocalRow& r = rows.row[m];
        const double gain = h_detail[3 * m + 1];
        r.w_rho = h_detail[3 * m];
        r.gain_m1 = gain - 1.0;
        r.sigma = h_detail[3 * m + 2];
        r.curve = r.sigma != 0.0 && gain != 1.0;
        r.slot = -1;
        r.lo = 0.0, r.ks = 0.0;
        if (h_curve_on && h_curve_on[m]) {
            const double* cv = h_curves + (size_t)m * (NLE_TONE_KNOTS + 2);
            r.lo = cv[0];
            r.ks = (double)(NLE_TONE_KNOTS - 1) / (cv[1] - cv[0]);
            r.slot = ncurves++;
            knots.insert(knots.end(), cv + 2, cv + 2 + NLE_TONE_KNOTS);
        }
    }
    HIP_OK(hipSetDevice(c->device));
    DevBuf<double> d_knots(std::max<size_t>(knots.size(), 1));
    if (ncurves) HIP_OK(hipMemcpyAsync(d_knots.p, knots.data(), sizeof(double) * knots.size(), hipMemcpyHostToDevice, c->stream));
    HIP_OK(nlek::local_combine(c->stream, d_x, d_layers, layer_stride, L, d_q, q_stride, M, n, rows, d_knots.p, ncurves, floor,
                               out_kind, d_out));
    HIP_OK(hipStreamSynchronize(c->stream));
}

// what nle_apply_local does between its argument checks and its combine, for it and nle_apply_local_auto: the checks that
// need the filter, then the L layers of x and the M spreads into one work buffer, layers first
DevBuf<float> local_apply_planes(const char* who, nle_filter* f, const float* d_x, int H, int W, int L, const float* d_strokes, int M,
                                 const double* h_scale, double spread, int out_kind, void* d_out, float* d_q_out) {
    nle_ctx* c = f->ctx;
    try {
        region_check_spread(f, M, H, W, h_scale, spread);
    } catch (const Fail& e) {
        throw Fail{e.code, std::string(who) + ": " + e.msg};
    }
    const long long n = f->n_local;  // == H W: world == 1
    detail_check_overlap(who, d_x, d_out, n, out_kind, "the plane");
    for (int m = 0; m < M; ++m) detail_check_overlap(who, d_strokes + (size_t)m * n, d_out, n, out_kind, "a stroke plane");
    if (d_q_out)
        for (int m = 0; m < M; ++m) detail_check_overlap(who, d_q_out + (size_t)m * n, d_out, n, out_kind, "d_q_out");
    DevBuf<float> d_work((size_t)(L + M) * n);
    // one batch over [x; s_1 .. s_M], as nle_apply_regions makes it: the L layers of x and one spread per stroke
    std::vector<double> resp((size_t)(L + M) * f->K);
    layer_resp(f->eigvals.data(), f->K, L, resp.data());
    spread_resp(f, M, h_scale, spread, resp.data() + (size_t)L * f->K);
    const float* planes[1 + NLE_REGION_MAX];
    int nresp[1 + NLE_REGION_MAX];
    planes[0] = d_x, nresp[0] = L;
    for (int m = 0; m < M; ++m) planes[1 + m] = d_strokes + (size_t)m * H * W, nresp[1 + m] = 1;
    apply_planes_impl(f, planes, 1 + M, H, W, nresp, resp.data(), d_work.p, n, false);
    if (d_q_out)
        HIP_OK(hipMemcpyAsync(d_q_out, d_work.p + (size_t)L * n, (size_t)M * n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    return d_work;
}

// ---- per-region histograms (include/nle.h "per-region histograms"; the kernel is region_hist.hip) ----
void region_hist_check(const char* who, int M, const double* h_scale, double floor) {
    const std::string name(who);
    if (M < 1 || M > NLE_REGION_MAX)
        throw Fail{NLE_ERR_INVALID, name + " takes 1 to " + std::to_string(NLE_REGION_MAX) + " regions, got " + std::to_string(M)};
    if (!h_scale) throw Fail{NLE_ERR_INVALID, name + ": NULL pointer"};
    for (int m = 0; m <= M; ++m)
        if (!std::isfinite(h_scale[m])) throw Fail{NLE_ERR_INVALID, name + ": the scale of row " + std::to_string(m) + " is not finite"};
    if (!std::isfinite(floor) || !(floor > 0))
        throw Fail{NLE_ERR_INVALID, name + ": the region floor must be finite and > 0, got " + std::to_string(floor)};
}

// only the rows that are on have counters on the device; h_counts receives every row, zeros for those that are off
void region_histograms_impl(nle_ctx* c, const float* d_y, const float* d_q, int M, long long n, long long q_stride,
                            const double* h_scale, const int* h_row_on, double floor, long long* h_counts) {
    int slot[NLE_REGION_MAX + 1], nslots = 0;
    for (int m = 0; m <= M; ++m) slot[m] = !h_row_on || h_row_on[m] ? nslots++ : -1;
    std::fill(h_counts, h_counts + (size_t)(M + 1) * nlek::kToneCounts, 0ll);
    if (!nslots) return;
    HIP_OK(hipSetDevice(c->device));
    DevBuf<unsigned long long> d_counts((size_t)nslots * nlek::kToneCounts);
    HIP_OK(nlek::region_hist(c->stream, d_y, d_q, q_stride, M, n, h_scale, slot, nslots, floor, d_counts.p));
    std::vector<long long> got((size_t)nslots * nlek::kToneCounts);
    HIP_OK(hipMemcpyAsync(got.data(), d_counts.p, sizeof(long long) * got.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    for (int m = 0; m <= M; ++m)
        if (slot[m] >= 0)
            std::copy(got.begin() + (size_t)slot[m] * nlek::kToneCounts, got.begin() + (size_t)(slot[m] + 1) * nlek::kToneCounts,
                      h_counts + (size_t)m * nlek::kToneCounts);
}

// ---- automatic regions (include/nle.h "automatic regions"; the kernels are segment.hip) ----
void segment_check_count(const char* who, int C) {
    if (C < 1 || C > NLE_REGION_MAX)
        throw Fail{NLE_ERR_INVALID, std::string(who) + " takes 1 to " + std::to_string(NLE_REGION_MAX) + " segments, got " +
                                        std::to_string(C)};
}

// the C planes of n floats `stride` apart must not meet the `bytes` bytes at p
bool segment_overlaps(const float* planes, int C, long long n, long long stride, const void* p, size_t bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(planes), a1 = a0 + ((size_t)(C - 1) * stride + n) * sizeof(float);
    const uintptr_t b0 = reinterpret_cast<uintptr_t>(p), b1 = b0 + bytes;
    return a0 < b1 && b0 < a1;
}

// the step's results on the device and their copy on the host; one download per fetch()
struct SegmentStep {
    nle_ctx* c;
    DevBuf<nlek::SegmentResult> d_r;
    DevBuf<double> d_partial;
    nlek::SegmentResult r{};
    SegmentStep(nle_ctx* ctx, long long n) : c(ctx), d_r(1), d_partial((size_t)nlek::segment_stats_blocks(n) * nlek::kRegionMax) {
        HIP_OK(hipMemsetAsync(d_r.p, 0, sizeof(nlek::SegmentResult), c->stream));
    }
    void stats(const float* d_q, long long q_stride, int C, long long n, const unsigned char* d_labels) {
        HIP_OK(nlek::segment_stats(c->stream, d_q, q_stride, C, n, d_labels, d_partial.p, d_r.p));
    }
    void means(const double* h_m, int C) {
        HIP_OK(hipMemcpyAsync(&d_r.p->mean[0], h_m, sizeof(double) * C, hipMemcpyHostToDevice, c->stream));
    }
    void assign(const float* d_q, long long q_stride, int C, long long n, unsigned char* d_labels, float* d_ind, long long ind_stride) {
        HIP_OK(nlek::segment_assign(c->stream, d_q, q_stride, C, n, d_labels, d_ind, ind_stride, d_r.p));
    }
    void fetch() {
        HIP_OK(hipMemcpyAsync(&r, d_r.p, sizeof r, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
    }
};

// b_1 .. b_{C-1} of the start from the counts of nle_plane_histogram(x, 1)
void segment_cuts(const long long* counts, long long n, int C, int* cuts) {
    for (int k = 1; k < C; ++k) {
        const long long need = (long long)((__int128)n * k / C) + 1;
        long long cum = counts[0];
        int b = NLE_TONE_BINS;
        for (int j = 0; j < NLE_TONE_BINS; ++j) {
            cum += counts[1 + j];
            if (cum >= need) {
                b = j;
                break;
            }
        }
        cuts[k - 1] = b;
    }
}

void segment_init_impl(nle_ctx* c, const float* d_x, long long n, int C, unsigned char* d_labels, int* h_cuts) {
    std::vector<long long> counts(nlek::kToneCounts);
    plane_histogram_impl(c, d_x, n, 1.0, counts.data());
    nlek::SegmentCuts cuts{};
    segment_cuts(counts.data(), n, C, cuts.b);
    if (h_cuts) std::copy(cuts.b, cuts.b + (C - 1), h_cuts);
    HIP_OK(nlek::segment_init(c->stream, d_x, n, C, cuts, d_labels));
    HIP_OK(hipStreamSynchronize(c->stream));
}

[[noreturn]] void segment_bad_label(const char* who, unsigned long long bad, int C) {
    throw Fail{NLE_ERR_INVALID, std::string(who) + ": " + std::to_string(bad) + " labels are not below C = " + std::to_string(C)};
}

}  // namespace

// ------------------------------------------------------------------------------ C ABI
extern "C" {

int nle_layer_responses(const double* h_eigvals, int K, int L, double* h_resp) {
    if (!h_eigvals || !h_resp || K < 0 || L < 1) return NLE_ERR_INVALID;
    layer_resp(h_eigvals, K, L, h_resp);
    return NLE_OK;
}

int nle_train(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, double hx,
              double hy, int n_sinkhorn_iter, int n_eigen_vectors, nle_filter** out) {
    if (!ctx || !d_lum || !out) return NLE_ERR_INVALID;
    *out = nullptr;
    return guard(ctx, [&] {
        *out = train_impl(ctx, d_lum, H, W, n_row_samples, n_col_samples, hx, hy, n_sinkhorn_iter, n_eigen_vectors);
    });
}

int nle_train_host(nle_ctx* ctx, const float* h_lum, int H, int W, int n_row_samples, int n_col_samples, double hx,
                   double hy, int n_sinkhorn_iter, int n_eigen_vectors, nle_filter** out) {
    if (!ctx || !h_lum || !out) return NLE_ERR_INVALID;
    *out = nullptr;
    return guard(ctx, [&] {
        size_t npx;
        DevBuf<float> d_lum = upload_train_plane(ctx, h_lum, H, W, &npx);
        *out = train_impl(ctx, d_lum.p, H, W, n_row_samples, n_col_samples, hx, hy, n_sinkhorn_iter, n_eigen_vectors);
        (*out)->plane = std::move(d_lum);  // kept: nle_apply*_host(h_x == NULL) filters the training plane
    });
}

int nle_train_host_u8(nle_ctx* ctx, const unsigned char* h_lum8, int H, int W, int n_row_samples, int n_col_samples, double hx,
                      double hy, int n_sinkhorn_iter, int n_eigen_vectors, nle_filter** out) {
    if (!ctx || !h_lum8 || !out) return NLE_ERR_INVALID;
    *out = nullptr;
    return guard(ctx, [&] {
        size_t npx;
        // (d_u8 is released after train_impl, which has drained the stream by then)
        DevBuf<unsigned char> d_u8 = upload_train_plane(ctx, h_lum8, H, W, &npx);
        DevBuf<float> d_lum(d_u8.n);
        HIP_OK(nlek::channel8_plane(ctx->stream, d_u8.p, (long long)npx, d_lum.p));
        *out = train_impl(ctx, d_lum.p, H, W, n_row_samples, n_col_samples, hx, hy, n_sinkhorn_iter, n_eigen_vectors);
        (*out)->plane = std::move(d_lum);
    });
}

void nle_filter_destroy(nle_filter* f) {
    if (!f) return;
    if (f->ctx) f->ctx->filters.erase(f);
    delete f;  // its buffers go back to the ctx's workspace cache (or, the ctx gone, to hipFree)
}

int nle_filter_info(const nle_filter* f, long long* n_local, int* K, int* r, int* p, int* row0, int* row1) {
    if (!f) return NLE_ERR_INVALID;
    if (n_local) *n_local = f->n_local;
    if (K) *K = f->K;
    if (r) *r = f->r;
    if (p) *p = f->p;
    if (row0) *row0 = f->row0;
    if (row1) *row1 = f->row1;
    return NLE_OK;
}

int nle_filter_diag(const nle_filter* f, int* h_info) {
    if (!f || !h_info) return NLE_ERR_INVALID;
    const int v[8] = {f->formulation, f->p, f->r, f->r_wa, f->r_q, f->K, f->chol_ka, f->chol_wa};
    std::copy(v, v + 8, h_info);
    return NLE_OK;
}

int nle_filter_eigvals(const nle_filter* f, double* h_eigvals) {
    if (!f || !h_eigvals) return NLE_ERR_INVALID;
    std::copy(f->eigvals.begin(), f->eigvals.end(), h_eigvals);
    return NLE_OK;
}

int nle_filter_sample_pixels(const nle_filter* f, long long* h_idx, int* p) {
    if (!f || !p) return NLE_ERR_INVALID;
    *p = (int)f->h_sample_pix.size();
    if (h_idx) std::copy(f->h_sample_pix.begin(), f->h_sample_pix.end(), h_idx);
    return NLE_OK;
}

int nle_sample_pixels(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, double hx,
                      double hy, long long* h_idx, int* p) {
    if (!ctx || !p) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        const GridSpec gs = checked_grid(H, W, n_row_samples, n_col_samples);
        if (gs.p() > 2048) throw Fail{NLE_ERR_INVALID, "more than 2048 samples is not supported"};
        std::vector<long long> list((size_t)gs.p());
        const AffinityOpts opts = affinity_opts(ctx);
        if (opts.listed()) {
            if (!d_lum) throw Fail{NLE_ERR_INVALID, std::string(opts.sampler_name()) + " needs the luminance plane"};
            check_affinity_opts(ctx, opts, gs, H, W, hx, hy, Caller::SAMPLE_PIXELS);
            HIP_OK(hipSetDevice(ctx->device));
            list = sampler_list(ctx, d_lum, gs, hx, hy);
            prof_flush(ctx);
        } else {
            for (int k = 0; k < gs.p(); ++k)
                list[k] = (long long)(gs.rowOff + (k / gs.nSelCols) * gs.rowStep) * W + gs.colOff + (k % gs.nSelCols) * gs.colStep;
        }
        *p = gs.p();
        if (h_idx) std::copy(list.begin(), list.end(), h_idx);
    });
}

long long nle_residual_sampler_bytes(int H, int W, int n_row_samples, int n_col_samples) {
    GridSpec gs;
    if (!make_grid(H, W, n_row_samples, n_col_samples, &gs)) return -1;
    return nlek::residual_ld((long long)H * W) * gs.p() * (long long)sizeof(double);
}

int nle_sample_pixels_order(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, double hx,
                            double hy, long long* h_order, double* h_pivot, int* p, int* n_residual, double* h_stats) {
    if (!ctx || !p || !n_residual) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        const AffinityOpts opts = affinity_opts(ctx);
        if (opts.sampler != NLE_SAMPLER_RESIDUAL)
            throw Fail{NLE_ERR_INVALID, "nle_sample_pixels_order: the order and the pivots are the residual sampler's "
                                        "(nle_ctx_set_sampler(NLE_SAMPLER_RESIDUAL))"};
        if (ctx->world > 1) throw Fail{NLE_ERR_INVALID, "nle_sample_pixels_order: world > 1 is not supported"};
        const GridSpec gs = checked_grid(H, W, n_row_samples, n_col_samples);
        if (gs.p() > 2048) throw Fail{NLE_ERR_INVALID, "more than 2048 samples is not supported"};
        if (!d_lum) throw Fail{NLE_ERR_INVALID, "the residual sampler needs the luminance plane"};
        check_affinity_opts(ctx, opts, gs, H, W, hx, hy, Caller::SAMPLE_PIXELS);
        HIP_OK(hipSetDevice(ctx->device));
        SamplerOrder o;
        sampler_list(ctx, d_lum, gs, hx, hy, &o);
        prof_flush(ctx);
        *p = gs.p();
        *n_residual = o.n_residual;
        if (h_order) std::copy(o.order.begin(), o.order.end(), h_order);
        if (h_pivot) std::copy(o.pivot.begin(), o.pivot.end(), h_pivot);
        if (h_stats) std::copy(o.stats, o.stats + 3, h_stats);
    });
}

int nle_filter_eigvec_range(const nle_filter* f, int ncols, double* h_min, double* h_max) {
    if (!f || !f->ctx || ncols < 1 || ncols > f->K || !h_min || !h_max) return NLE_ERR_INVALID;
    return guard(f->ctx, [&] {
        nle_ctx* c = f->ctx;
        HIP_OK(hipSetDevice(c->device));
        // an implicit V is not materialised for this: only the requested leading columns are projected, into a
        // temporary (the CLI prints the range of 5 of K columns, src/filter.cpp:506)
        const float* d_cols = f->V.p;
        int ldc = f->ldv;
        DevBuf<float> d_tmp;
        if (!f->V.p && f->tables) {
            const TableFilter& t = *f->tables;
            DevBuf<float> d_plane;  // the filter stays as it is: a plane it does not hold is rebuilt into this temporary
            const float* lum = t.plane_into(c, d_plane);
            const long long M = f->n_local, pix0 = (long long)f->row0 * f->W;
            const int ldd_full = t.ldd, ldd = nlek::project64_ld(ncols);
            std::vector<double> Dfull((size_t)f->p * ldd_full), Dk((size_t)f->p * ldd, 0.0);
            HIP_OK(hipMemcpyAsync(Dfull.data(), t.D.p, Dfull.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIP_OK(hipStreamSynchronize(c->stream));
            for (int a = 0; a < f->p; ++a)
                for (int k = 0; k < ncols; ++k) Dk[(size_t)a * ldd + k] = Dfull[(size_t)a * ldd_full + k];
            DevBuf<double> d_Dk(Dk.size());
            HIP_OK(hipMemcpyAsync(d_Dk.p, Dk.data(), Dk.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
            ldc = ld4(ncols);
            d_tmp.alloc((size_t)std::max<long long>(M, 1) * ldc);
            PROFILED(c, NLE_K_PROJECT, nlek::project64(c->stream, lum, t.gs, t.samples.p, t.p, t.nsw, t.npw, pix0, M, d_Dk.p,
                                                       ncols, t.c.p, d_tmp.p, ldc));
            scatter_sample_rows(c, f->h_sample_pix, f->p, host_Vrows(f), ncols, ldc, pix0, M, d_tmp.p);
            HIP_OK(hipStreamSynchronize(c->stream));  // Dk (host) is consumed
            d_cols = d_tmp.p;
        } else {
            ensure_V(const_cast<nle_filter*>(f));
            d_cols = f->V.p;
        }
        const int nb = 256;
        DevBuf<float> d_out((size_t)nb * 2 * ncols);
        HIP_OK(nlek::col_range(c->stream, d_cols, f->n_local, ldc, ncols, d_out.p, nb));
        std::vector<float> out((size_t)nb * 2 * ncols);
        HIP_OK(hipMemcpyAsync(out.data(), d_out.p, out.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        for (int k = 0; k < ncols; ++k) {
            double mn = out[2 * k], mx = out[2 * k + 1];
            for (int b = 1; b < nb; ++b) {
                mn = std::min(mn, (double)out[(size_t)b * 2 * ncols + 2 * k]);
                mx = std::max(mx, (double)out[(size_t)b * 2 * ncols + 2 * k + 1]);
            }
            h_min[k] = mn;
            h_max[k] = mx;
        }
    });
}

int nle_filter_eigvecs(const nle_filter* f, const float** d_V, int* ld) {
    if (!f || !f->ctx || !d_V || !ld) return NLE_ERR_INVALID;
    const int st = guard(f->ctx, [&] {
        HIP_OK(hipSetDevice(f->ctx->device));
        ensure_V(const_cast<nle_filter*>(f));
    });
    if (st != NLE_OK) return st;
    *d_V = f->V.p;
    *ld = f->ldv;
    return NLE_OK;
}

int nle_filter_copy_eigvecs(const nle_filter* f, float* d_out) {
    if (!f || !f->ctx || !d_out) return NLE_ERR_INVALID;
    return guard(f->ctx, [&] {
        HIP_OK(hipSetDevice(f->ctx->device));
        ensure_V(const_cast<nle_filter*>(f));
        HIP_OK(hipMemcpyAsync(d_out, f->V.p, (size_t)f->n_local * f->ldv * sizeof(float), hipMemcpyDeviceToDevice,
                              f->ctx->stream));
        HIP_OK(hipStreamSynchronize(f->ctx->stream));
    });
}

int nle_filter_timings(const nle_filter* f, double* h_ms) {
    if (!f || !h_ms) return NLE_ERR_INVALID;
    std::copy(f->ms, f->ms + 6, h_ms);
    return NLE_OK;
}

int nle_apply(nle_filter* f, const float* d_x, int H, int W, const double* h_fS, float* d_y) {
    if (!f || !f->ctx || !d_x || !h_fS || !d_y) return NLE_ERR_INVALID;
    return guard(f->ctx, [&] { apply_impl(f, d_x, H, W, h_fS, 1, d_y); });
}

int nle_apply_layers(nle_filter* f, const float* d_x, int H, int W, int L, float* d_y) {
    if (!f || !f->ctx || !d_x || !d_y || L < 1) return NLE_ERR_INVALID;
    return guard(f->ctx, [&] {
        std::vector<double> resp((size_t)L * f->K);
        layer_resp(f->eigvals.data(), f->K, L, resp.data());
        apply_impl(f, d_x, H, W, resp.data(), L, d_y);
    });
}

int nle_apply_host(nle_filter* f, const float* h_x, int H, int W, const double* h_fS, float* h_y) {
    if (!f || !f->ctx || !h_fS || !h_y) return NLE_ERR_INVALID;
    return guard(f->ctx, [&] { apply_host_common(f, h_x, H, W, h_fS, 1, h_y); });
}

int nle_apply_layers_host(nle_filter* f, const float* h_x, int H, int W, int L, float* h_y) {
    if (!f || !f->ctx || !h_y || L < 1) return NLE_ERR_INVALID;
    return guard(f->ctx, [&] {
        std::vector<double> resp((size_t)L * f->K);
        layer_resp(f->eigvals.data(), f->K, L, resp.data());
        apply_host_common(f, h_x, H, W, resp.data(), L, h_y);
    });
}

// the same plane kept as fp32 levels (what nle_lab2bgr8 / nle_lab2bgr8_planes take for a replaced channel)
int nle_apply_rounded8(nle_filter* f, const float* d_x, int H, int W, const double* h_fS, float* d_y) {
    if (!f || !f->ctx || !d_x || !h_fS || !d_y) return NLE_ERR_INVALID;
    return guard(f->ctx, [&] {
        apply_impl(f, d_x, H, W, h_fS, 1, d_y, nullptr, 0, /*round8=*/true);
        if (!f->tables) round8_planes(f, d_y, 1, f->n_local);  // formulations with fp32 planes: round those
    });
}

// NLEFilter::enhance's L plane (src/filter.cpp:428-436): apply, clamp, convertTo(CV_8U) -- one byte per pixel leaves the device
int nle_apply_u8(nle_filter* f, const float* d_x, int H, int W, const double* h_fS, unsigned char* d_out) {
    if (!f || !f->ctx || !d_x || !h_fS || !d_out) return NLE_ERR_INVALID;
    return guard(f->ctx, [&] {
        nle_ctx* c = f->ctx;
        DevBuf<float> d_y((size_t)std::max<long long>(f->n_local, 1));
        apply_impl(f, d_x, H, W, h_fS, 1, d_y.p, nullptr, 0, /*round8=*/true);
        HIP_OK(nlek::plane_to_u8(c->stream, d_y.p, f->n_local, d_out));
        HIP_OK(hipStreamSynchronize(c->stream));   // d_y returns to the ctx's cache
    });
}

int nle_apply_u8_host(nle_filter* f, const float* h_x, int H, int W, const double* h_fS, unsigned char* h_out) {
    if (!f || !f->ctx || !h_fS || !h_out) return NLE_ERR_INVALID;
    return guard(f->ctx, [&] {
        nle_ctx* c = f->ctx;
        DevBuf<float> d_xbuf;
        const float* d_x = host_apply_input(f, h_x, H, W, d_xbuf);
        const size_t n = (size_t)std::max<long long>(f->n_local, 1);
        DevBuf<float> d_y(n);
        DevBuf<unsigned char> d_o(n);
        Drain drain{c};
        apply_impl(f, d_x, H, W, h_fS, 1, d_y.p, nullptr, 0, /*round8=*/true);
        HIP_OK(nlek::plane_to_u8(c->stream, d_y.p, f->n_local, d_o.p));
        HIP_OK(hipMemcpyAsync(h_out, d_o.p, (size_t)f->n_local, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
    });
}

int nle_apply_planes(nle_filter* f, const float* d_x, int P, long long x_stride, int H, int W, const int* h_nresp,
                     const double* h_resp, int out_kind, float* d_y, long long y_stride) {
    if (!f || !f->ctx) return NLE_ERR_INVALID;
    return guard(f->ctx, [&] {
        // every refusal before anything is enqueued
        if (P < 1 || P > NLE_PLANES_MAX)
            throw Fail{NLE_ERR_INVALID, "nle_apply_planes takes 1 to " + std::to_string(NLE_PLANES_MAX) + " planes, got " +
                                            std::to_string(P)};
        if (!d_x || !h_resp || !d_y) throw Fail{NLE_ERR_INVALID, "nle_apply_planes: NULL pointer"};
        check_out_kind("nle_apply_planes: unknown output kind ", out_kind, false);
        int nresp[NLE_PLANES_MAX], R = 0;
        for (int m = 0; m < P; ++m) {
            nresp[m] = h_nresp ? h_nresp[m] : 1;
            if (nresp[m] < 1 || nresp[m] > 64)
                throw Fail{NLE_ERR_INVALID, "nle_apply_planes: plane " + std::to_string(m) + " has " + std::to_string(nresp[m]) +
                                                " responses, 1 to 64 are taken"};
            R += nresp[m];
        }
        if (R > 128)
            throw Fail{NLE_ERR_INVALID, "nle_apply_planes: " + std::to_string(R) + " responses in all, at most 128 are taken"};
        check_plane_size(f, H, W, true);
        const nle_ctx* c = f->ctx;
        const long long nin = (c->slab_input && c->world > 1) ? f->n_local : (long long)H * W, nout = f->n_local;
        if ((P > 1 && x_stride < nin) || (R > 1 && y_stride < nout) || x_stride < 0 || y_stride < 0)
            throw Fail{NLE_ERR_INVALID, "nle_apply_planes: a plane stride is smaller than the plane"};
        // inputs of later planes are read after the outputs of earlier ones are written on the one-by-one route: no output
        // plane may overlap any input plane
        for (int m = 0; m < P; ++m)
            for (int j = 0; j < R; ++j) {
                const float *x0 = d_x + (size_t)m * x_stride, *y0 = d_y + (size_t)j * y_stride;
                if (reinterpret_cast<uintptr_t>(x0) < reinterpret_cast<uintptr_t>(y0 + nout) &&
                    reinterpret_cast<uintptr_t>(y0) < reinterpret_cast<uintptr_t>(x0 + nin))
                    throw Fail{NLE_ERR_INVALID, "nle_apply_planes: output plane " + std::to_string(j) + " overlaps input plane " +
                                                    std::to_string(m)};
            }
        const float* planes[NLE_PLANES_MAX];
        for (int m = 0; m < P; ++m) planes[m] = d_x + (size_t)m * x_stride;
        apply_planes_impl(f, planes, P, H, W, nresp, h_resp, d_y, R > 1 ? y_stride : nout, out_kind == NLE_REGION_OUT_ROUNDED8);
    });
}

int nle_region_combine(nle_ctx* ctx, const float* d_layers, int L, const float* d_q, int M, long long n, long long layer_stride,
                       long long q_stride, const double* h_weights, double floor, int out_kind, void* d_out) {
    if (!ctx) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        if (!d_layers || !d_q || !h_weights || !d_out) throw Fail{NLE_ERR_INVALID, "nle_region_combine: NULL pointer"};
        region_check_combine(L, M, floor, out_kind);
        if (n < 1) throw Fail{NLE_ERR_INVALID, "nle_region_combine: n must be >= 1"};
        if ((L > 1 && layer_stride < n) || (M > 1 && q_stride < n) || layer_stride < 0 || q_stride < 0)
            throw Fail{NLE_ERR_INVALID, "nle_region_combine: a plane stride is smaller than n"};
        region_combine_impl(ctx, d_layers, L, d_q, M, n, layer_stride, q_stride, h_weights, floor, out_kind, d_out);
    });
}

int nle_region_spread(nle_filter* f, const float* d_strokes, int M, int H, int W, const double* h_scale, double spread,
                      float* d_q) {
    if (!f || !f->ctx) return NLE_ERR_INVALID;
    return guard(f->ctx, [&] {
        if (!d_strokes || !d_q) throw Fail{NLE_ERR_INVALID, "nle_region_spread: NULL pointer"};
        region_check_spread(f, M, H, W, h_scale, spread);
        region_spread_impl(f, d_strokes, M, H, W, h_scale, spread, d_q);
    });
}

int nle_filter_coefficients(nle_filter* f, const float* d_x, int P, long long x_stride, int H, int W, double* h_t) {
    if (!f || !f->ctx) return NLE_ERR_INVALID;
    return guard(f->ctx, [&] {
        if (f->ctx->world > 1)
            throw Fail{NLE_ERR_INVALID, "nle_filter_coefficients runs on one device: a sharded ctx (world > 1) is not built"};
        if (P < 1 || P > NLE_PLANES_MAX)
            throw Fail{NLE_ERR_INVALID, "nle_filter_coefficients takes 1 to " + std::to_string(NLE_PLANES_MAX) + " planes, got " +
                                            std::to_string(P)};
        if (!d_x || !h_t) throw Fail{NLE_ERR_INVALID, "nle_filter_coefficients: NULL pointer"};
        check_plane_size(f, H, W, true);
        if (P > 1 && x_stride < (long long)H * W)
            throw Fail{NLE_ERR_INVALID, "nle_filter_coefficients: the plane stride is smaller than the plane"};
        const float* planes[NLE_PLANES_MAX];
        for (int m = 0; m < P; ++m) planes[m] = d_x + (size_t)m * (size_t)(P > 1 ? x_stride : 0);
        coefficients_impl(f, planes, P, h_t);
    });
}

int nle_apply_regions(nle_filter* f, const float* d_x, int H, int W, int L, const float* d_strokes, int M,
                      const double* h_scale, double spread, double floor, const double* h_weights, int out_kind, void* d_out) {
    if (!f || !f->ctx) return NLE_ERR_INVALID;
    return guard(f->ctx, [&] {
        nle_ctx* c = f->ctx;
        if (!d_x || !d_strokes || !h_weights || !d_out) throw Fail{NLE_ERR_INVALID, "nle_apply_regions: NULL pointer"};
        region_check_combine(L, M, floor, out_kind);
        region_check_spread(f, M, H, W, h_scale, spread);
        const long long n = f->n_local;  // == H W: world == 1
        DevBuf<float> d_work((size_t)(L + M) * n);
        // one batch over [x; s_1 .. s_M]: the L layers of x (nle_apply_layers) and one spread per stroke (nle_region_spread)
        std::vector<double> resp((size_t)(L + M) * f->K);
        layer_resp(f->eigvals.data(), f->K, L, resp.data());
        spread_resp(f, M, h_scale, spread, resp.data() + (size_t)L * f->K);
        const float* planes[1 + NLE_REGION_MAX];
        int nresp[1 + NLE_REGION_MAX];
        planes[0] = d_x, nresp[0] = L;
        for (int m = 0; m < M; ++m) planes[1 + m] = d_strokes + (size_t)m * H * W, nresp[1 + m] = 1;
        apply_planes_impl(f, planes, 1 + M, H, W, nresp, resp.data(), d_work.p, n, false);
        region_combine_impl(c, d_work.p, L, d_work.p + (size_t)L * n, M, n, n, n, h_weights, floor, out_kind, d_out);
    });
}

int nle_detail_combine(nle_ctx* ctx, const float* d_x, const float* d_layers, int L, long long n, long long layer_stride,
                       const double* h_weights, double w_rho, double gain, double sigma, int out_kind, void* d_out) {
    if (!ctx) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        if (!d_x || !d_layers || !h_weights || !d_out) throw Fail{NLE_ERR_INVALID, "nle_detail_combine: NULL pointer"};
        detail_check("nle_detail_combine", L, h_weights, w_rho, gain, sigma, out_kind);
        if (n < 1) throw Fail{NLE_ERR_INVALID, "nle_detail_combine: n must be >= 1"};
        if ((L > 1 && layer_stride < n) || layer_stride < 0)
            throw Fail{NLE_ERR_INVALID, "nle_detail_combine: the layer stride is smaller than n"};
        detail_check_overlap("nle_detail_combine", d_x, d_out, n, out_kind, "the plane");
        for (int l = 0; l < L; ++l)
            detail_check_overlap("nle_detail_combine", d_layers + (size_t)l * layer_stride, d_out, n, out_kind, "a layer");
        detail_combine_impl(ctx, d_x, d_layers, L, n, layer_stride, h_weights, w_rho, gain, sigma, out_kind, d_out);
    });
}

int nle_apply_detail(nle_filter* f, const float* d_x, int H, int W, int L, const double* h_weights, double w_rho, double gain,
                     double sigma, int out_kind, void* d_out) {
    if (!f || !f->ctx) return NLE_ERR_INVALID;
    return guard(f->ctx, [&] {
        nle_ctx* c = f->ctx;
        if (!d_x || !h_weights || !d_out) throw Fail{NLE_ERR_INVALID, "nle_apply_detail: NULL pointer"};
        detail_check("nle_apply_detail", L, h_weights, w_rho, gain, sigma, out_kind);
        if (c->world > 1)
            throw Fail{NLE_ERR_INVALID, "nle_apply_detail runs on one device only (world == 1): slabs and device groups are not built"};
        check_plane_size(f, H, W, true);
        const long long n = f->n_local;  // == H W: world == 1
        detail_check_overlap("nle_apply_detail", d_x, d_out, n, out_kind, "the plane");
        DevBuf<float> d_work((size_t)L * n);
        std::vector<double> resp((size_t)L * f->K);
        layer_resp(f->eigvals.data(), f->K, L, resp.data());
        apply_impl(f, d_x, H, W, resp.data(), L, d_work.p);  // nle_apply_layers
        detail_combine_impl(c, d_x, d_work.p, L, n, n, h_weights, w_rho, gain, sigma, out_kind, d_out);
    });
}

int nle_plane_histogram(nle_ctx* ctx, const float* d_x, long long n, double scale, long long* h_counts) {
    if (!ctx) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        if (!d_x || !h_counts) throw Fail{NLE_ERR_INVALID, "nle_plane_histogram: NULL pointer"};
        if (n < 1) throw Fail{NLE_ERR_INVALID, "nle_plane_histogram: n must be >= 1"};
        if (!std::isfinite(scale)) throw Fail{NLE_ERR_INVALID, "nle_plane_histogram: the scale is not finite"};
        plane_histogram_impl(ctx, d_x, n, scale, h_counts);
    });
}

int nle_segment_init(nle_ctx* ctx, const float* d_x, long long n, int C, unsigned char* d_labels, int* h_cuts) {
    if (!ctx) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        if (!d_x || !d_labels) throw Fail{NLE_ERR_INVALID, "nle_segment_init: NULL pointer"};
        segment_check_count("nle_segment_init", C);
        if (n < 1) throw Fail{NLE_ERR_INVALID, "nle_segment_init: n must be >= 1"};
        segment_init_impl(ctx, d_x, n, C, d_labels, h_cuts);
    });
}

int nle_segment_stats(nle_ctx* ctx, const float* d_q, int C, long long n, long long q_stride, const unsigned char* d_labels,
                      long long* h_counts, double* h_sums) {
    if (!ctx) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        if (!d_q || !d_labels || !h_counts || !h_sums) throw Fail{NLE_ERR_INVALID, "nle_segment_stats: NULL pointer"};
        segment_check_count("nle_segment_stats", C);
        if (n < 1) throw Fail{NLE_ERR_INVALID, "nle_segment_stats: n must be >= 1"};
        if (q_stride != 0 && q_stride < n) throw Fail{NLE_ERR_INVALID, "nle_segment_stats: the plane stride is neither 0 nor >= n"};
        HIP_OK(hipSetDevice(ctx->device));
        SegmentStep step(ctx, n);
        step.stats(d_q, q_stride, C, n, d_labels);
        step.fetch();
        if (step.r.bad) segment_bad_label("nle_segment_stats", step.r.bad, C);
        for (int c = 0; c < C; ++c) h_counts[c] = (long long)step.r.count[c], h_sums[c] = step.r.sum[c];
    });
}

int nle_segment_assign(nle_ctx* ctx, const float* d_q, int C, long long n, long long q_stride, const double* h_m,
                       unsigned char* d_labels, float* d_indicators, long long ind_stride, long long* h_counts,
                       long long* h_changed) {
    if (!ctx) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        if (!d_q || !h_m || !d_labels || !h_counts || !h_changed) throw Fail{NLE_ERR_INVALID, "nle_segment_assign: NULL pointer"};
        segment_check_count("nle_segment_assign", C);
        if (n < 1) throw Fail{NLE_ERR_INVALID, "nle_segment_assign: n must be >= 1"};
        if (q_stride != 0 && q_stride < n) throw Fail{NLE_ERR_INVALID, "nle_segment_assign: the plane stride is neither 0 nor >= n"};
        if (d_indicators && C > 1 && ind_stride < n)
            throw Fail{NLE_ERR_INVALID, "nle_segment_assign: the indicator stride is smaller than n"};
        if (segment_overlaps(d_q, C, n, q_stride, d_labels, (size_t)n))
            throw Fail{NLE_ERR_INVALID, "nle_segment_assign: the labels overlap the planes"};
        if (d_indicators && (segment_overlaps(d_indicators, C, n, C > 1 ? ind_stride : n, d_labels, (size_t)n) ||
                             segment_overlaps(d_indicators, C, n, C > 1 ? ind_stride : n, d_q,
                                              ((size_t)(C - 1) * q_stride + n) * sizeof(float))))
            throw Fail{NLE_ERR_INVALID, "nle_segment_assign: the indicator planes overlap an input"};
        HIP_OK(hipSetDevice(ctx->device));
        SegmentStep step(ctx, n);
        step.means(h_m, C);
        step.assign(d_q, q_stride, C, n, d_labels, d_indicators, C > 1 ? ind_stride : n);
        step.fetch();
        if (step.r.bad_new) segment_bad_label("nle_segment_assign", step.r.bad_new, C);
        for (int c = 0; c < C; ++c) h_counts[c] = (long long)step.r.new_count[c];
        *h_changed = (long long)step.r.changed;
    });
}

int nle_filter_segment(nle_filter* f, int H, int W, int C, double spread, int max_iter, unsigned char* d_labels, float* d_q,
                       long long q_stride, long long* h_counts, double* h_objective, int* h_iters, int* h_converged) {
    if (!f || !f->ctx) return NLE_ERR_INVALID;
    return guard(f->ctx, [&] {
        nle_ctx* c = f->ctx;
        if (!d_labels || !h_counts || !h_objective || !h_iters || !h_converged)
            throw Fail{NLE_ERR_INVALID, "nle_filter_segment: NULL pointer"};
        segment_check_count("nle_filter_segment", C);
        if (!std::isfinite(spread) || !(spread > 0))
            throw Fail{NLE_ERR_INVALID, "the segment spread must be finite and > 0, got " + std::to_string(spread)};
        if (max_iter < 1 || max_iter > NLE_SEGMENT_ITERATIONS_MAX)
            throw Fail{NLE_ERR_INVALID, "nle_filter_segment takes 1 to " + std::to_string(NLE_SEGMENT_ITERATIONS_MAX) +
                                            " iterations, got " + std::to_string(max_iter)};
        if (c->world > 1)
            throw Fail{NLE_ERR_INVALID, "nle_filter_segment runs on one device only (world == 1): slabs and device groups are not built"};
        check_plane_size(f, H, W, true);
        const long long n = f->n_local;  // == H W: world == 1
        if (d_q && C > 1 && q_stride < n) throw Fail{NLE_ERR_INVALID, "nle_filter_segment: the plane stride is smaller than n"};
        if (d_q && segment_overlaps(d_q, C, n, C > 1 ? q_stride : n, d_labels, (size_t)n))
            throw Fail{NLE_ERR_INVALID, "nle_filter_segment: the labels overlap the planes"};
        HIP_OK(hipSetDevice(c->device));
        DevBuf<float> d_ind((size_t)C * n), d_work((size_t)C * n);
        SegmentStep step(c, n);
        double scale[NLE_REGION_MAX];
        long long counts[NLE_REGION_MAX];
        auto spread_now = [&] {
            for (int k = 0; k < C; ++k) scale[k] = counts[k] ? (double)n / (double)counts[k] : 0.0;
            region_spread_impl(f, d_ind.p, C, H, W, scale, spread, d_work.p);
        };
        // the indicator planes and the counts of the start: the assignment kernel without planes, which keeps every label
        step.assign(nullptr, 0, C, n, d_labels, d_ind.p, n);
        step.fetch();
        if (step.r.bad_new) segment_bad_label("nle_filter_segment", step.r.bad_new, C);
        for (int k = 0; k < C; ++k) counts[k] = (long long)step.r.new_count[k];
        int iters = 0;
        bool converged = false;
        while (iters < max_iter && !converged) {
            spread_now();
            step.stats(d_work.p, n, C, n, d_labels);
            step.assign(d_work.p, n, C, n, d_labels, d_ind.p, n);
            step.fetch();  // the iteration's one download
            double J = 0.0;
            for (int k = 0; k < C; ++k)
                if (step.r.count[k]) J += (double)step.r.count[k] * step.r.mean[k];
            h_objective[iters++] = J / (double)n;
            for (int k = 0; k < C; ++k) counts[k] = (long long)step.r.new_count[k];
            converged = step.r.changed == 0;
        }
        if (d_q) {
            if (!converged) spread_now();  // the last assignment moved labels: the spreads of what is returned
            for (int k = 0; k < C; ++k)
                HIP_OK(hipMemcpyAsync(d_q + (size_t)k * (C > 1 ? q_stride : n), d_work.p + (size_t)k * n, (size_t)n * sizeof(float),
                                      hipMemcpyDeviceToDevice, c->stream));
            HIP_OK(hipStreamSynchronize(c->stream));
        }
        std::copy(counts, counts + C, h_counts);
        *h_iters = iters;
        *h_converged = converged ? 1 : 0;
    });
}

int nle_tone_curve(const long long* h_counts, double shadows, double highlights, double clip_percent, double equalise,
                   double* h_curve) {
    return guard(nullptr, [&] { tone_curve_impl(h_counts, shadows, highlights, clip_percent, equalise, h_curve); });
}

int nle_tone_combine(nle_ctx* ctx, const float* d_x, const float* d_layers, int L, long long n, long long layer_stride,
                     const double* h_weights, double w_rho, double gain, double sigma, const double* h_curve, int out_kind,
                     void* d_out) {
    if (!ctx) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        if (!d_x || !d_layers || !h_weights || !h_curve || !d_out) throw Fail{NLE_ERR_INVALID, "nle_tone_combine: NULL pointer"};
        detail_check("nle_tone_combine", L, h_weights, w_rho, gain, sigma, out_kind);
        tone_check_curve("nle_tone_combine", h_curve);
        if (n < 1) throw Fail{NLE_ERR_INVALID, "nle_tone_combine: n must be >= 1"};
        if ((L > 1 && layer_stride < n) || layer_stride < 0)
            throw Fail{NLE_ERR_INVALID, "nle_tone_combine: the layer stride is smaller than n"};
        detail_check_overlap("nle_tone_combine", d_x, d_out, n, out_kind, "the plane");
        for (int l = 0; l < L; ++l)
            detail_check_overlap("nle_tone_combine", d_layers + (size_t)l * layer_stride, d_out, n, out_kind, "a layer");
        tone_combine_impl(ctx, d_x, d_layers, L, n, layer_stride, h_weights, w_rho, gain, sigma, h_curve, out_kind, d_out);
    });
}

int nle_apply_tone(nle_filter* f, const float* d_x, int H, int W, int L, const double* h_weights, double w_rho, double gain,
                   double sigma, double shadows, double highlights, double clip_percent, double equalise, int out_kind,
                   void* d_out, double* h_curve_out) {
    if (!f || !f->ctx) return NLE_ERR_INVALID;
    return guard(f->ctx, [&] {
        nle_ctx* c = f->ctx;
        if (!d_x || !h_weights || !d_out) throw Fail{NLE_ERR_INVALID, "nle_apply_tone: NULL pointer"};
        detail_check("nle_apply_tone", L, h_weights, w_rho, gain, sigma, out_kind);
        // the curve's own refusals, on the parameters alone (the counts that come later are this call's own: n >= 1 of them)
        if (const char* refused = nlek::tone_check(shadows, highlights, clip_percent, equalise)) throw Fail{NLE_ERR_INVALID, refused};
        std::vector<double> curve(NLE_TONE_KNOTS + 2);
        const bool stats = clip_percent >= 0 || equalise > 0;
        std::vector<long long> counts(stats ? nlek::kToneCounts : 0);
        if (c->world > 1)
            throw Fail{NLE_ERR_INVALID, "nle_apply_tone runs on one device only (world == 1): slabs and device groups are not built"};
        check_plane_size(f, H, W, true);
        const long long n = f->n_local;  // == H W: world == 1
        detail_check_overlap("nle_apply_tone", d_x, d_out, n, out_kind, "the plane");
        DevBuf<float> d_work((size_t)L * n);
        std::vector<double> resp((size_t)L * f->K);
        layer_resp(f->eigvals.data(), f->K, L, resp.data());
        apply_impl(f, d_x, H, W, resp.data(), L, d_work.p);  // nle_apply_layers
        if (stats) plane_histogram_impl(c, d_work.p + (size_t)(L - 1) * n, n, h_weights[L - 1], counts.data());
        tone_curve_impl(stats ? counts.data() : nullptr, shadows, highlights, clip_percent, equalise, curve.data());
        if (h_curve_out) std::copy(curve.begin(), curve.end(), h_curve_out);
        if (shadows == 0 && highlights == 0 && clip_percent < 0 && equalise == 0)  // inactive: nle_apply_detail
            detail_combine_impl(c, d_x, d_work.p, L, n, n, h_weights, w_rho, gain, sigma, out_kind, d_out);
        else tone_combine_impl(c, d_x, d_work.p, L, n, n, h_weights, w_rho, gain, sigma, curve.data(), out_kind, d_out);
    });
}

int nle_local_combine(nle_ctx* ctx, const float* d_x, const float* d_layers, int L, const float* d_q, int M, long long n,
                      long long layer_stride, long long q_stride, const double* h_weights, const double* h_detail,
                      const int* h_curve_on, const double* h_curves, double floor, int out_kind, void* d_out) {
    if (!ctx) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        if (!d_x || !d_layers || !d_q || !d_out) throw Fail{NLE_ERR_INVALID, "nle_local_combine: NULL pointer"};
        local_check("nle_local_combine", L, M, h_weights, h_detail, h_curve_on, h_curves, floor, out_kind);
        if (n < 1) throw Fail{NLE_ERR_INVALID, "nle_local_combine: n must be >= 1"};
        if ((L > 1 && layer_stride < n) || (M > 1 && q_stride < n) || layer_stride < 0 || q_stride < 0)
            throw Fail{NLE_ERR_INVALID, "nle_local_combine: a plane stride is smaller than n"};
        detail_check_overlap("nle_local_combine", d_x, d_out, n, out_kind, "the plane");
        for (int l = 0; l < L; ++l)
            detail_check_overlap("nle_local_combine", d_layers + (size_t)l * layer_stride, d_out, n, out_kind, "a layer");
        for (int m = 0; m < M; ++m)
            detail_check_overlap("nle_local_combine", d_q + (size_t)m * q_stride, d_out, n, out_kind, "a membership plane");
        local_combine_impl(ctx, d_x, d_layers, L, d_q, M, n, layer_stride, q_stride, h_weights, h_detail, h_curve_on, h_curves,
                           floor, out_kind, d_out);
    });
}

int nle_local_chroma(nle_ctx* ctx, const float* d_a, const float* d_b, const float* d_q, int M, long long n, long long q_stride,
                     const double* h_saturation, double floor, float* d_a_out, float* d_b_out) {
    if (!ctx) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        if (!d_a || !d_b || !d_q || !h_saturation || !d_a_out || !d_b_out) throw Fail{NLE_ERR_INVALID, "nle_local_chroma: NULL pointer"};
        if (M < 1 || M > NLE_REGION_MAX)
            throw Fail{NLE_ERR_INVALID, "nle_local_chroma takes 1 to " + std::to_string(NLE_REGION_MAX) + " regions, got " +
                                            std::to_string(M)};
        for (int m = 0; m <= M; ++m)
            if (!std::isfinite(h_saturation[m]) || h_saturation[m] < 0 || h_saturation[m] > NLE_LOCAL_SATURATION_MAX)
                throw Fail{NLE_ERR_INVALID, "nle_local_chroma: row " + std::to_string(m) + ": the saturation must be finite and in [0, " +
                                                std::to_string(NLE_LOCAL_SATURATION_MAX) + "], got " + std::to_string(h_saturation[m])};
        if (!std::isfinite(floor) || !(floor > 0))
            throw Fail{NLE_ERR_INVALID, "nle_local_chroma: the region floor must be finite and > 0, got " + std::to_string(floor)};
        if (n < 1) throw Fail{NLE_ERR_INVALID, "nle_local_chroma: n must be >= 1"};
        if ((M > 1 && q_stride < n) || q_stride < 0) throw Fail{NLE_ERR_INVALID, "nle_local_chroma: a plane stride is smaller than n"};
        // in place is each output on its own input, exactly; everything else must lie apart
        const auto apart = [&](const float* p, const float* out, const char* out_name, const char* what) {
            const uintptr_t i0 = reinterpret_cast<uintptr_t>(p), o0 = reinterpret_cast<uintptr_t>(out), len = (uintptr_t)n * sizeof(float);
            if (i0 < o0 + len && o0 < i0 + len)
                throw Fail{NLE_ERR_INVALID, std::string("nle_local_chroma: ") + out_name + " overlaps " + what};
        };
        if (d_a_out != d_a) apart(d_a, d_a_out, "d_a_out", "d_a");
        if (d_b_out != d_b) apart(d_b, d_b_out, "d_b_out", "d_b");
        apart(d_b, d_a_out, "d_a_out", "d_b");
        apart(d_a, d_b_out, "d_b_out", "d_a");
        apart(d_a_out, d_b_out, "d_b_out", "d_a_out");
        for (int m = 0; m < M; ++m) {
            apart(d_q + (size_t)m * q_stride, d_a_out, "d_a_out", "a membership plane");
            apart(d_q + (size_t)m * q_stride, d_b_out, "d_b_out", "a membership plane");
        }
        HIP_OK(hipSetDevice(ctx->device));
        HIP_OK(nlek::local_chroma(ctx->stream, d_a, d_b, d_q, q_stride, M, n, h_saturation, floor, d_a_out, d_b_out));
        HIP_OK(hipStreamSynchronize(ctx->stream));
    });
}

int nle_apply_local(nle_filter* f, const float* d_x, int H, int W, int L, const float* d_strokes, int M, const double* h_scale,
                    double spread, double floor, const double* h_weights, const double* h_detail, const int* h_curve_on,
                    const double* h_curves, int out_kind, void* d_out, float* d_q_out) {
    if (!f || !f->ctx) return NLE_ERR_INVALID;
    return guard(f->ctx, [&] {
        nle_ctx* c = f->ctx;
        if (!d_x || !d_strokes || !d_out) throw Fail{NLE_ERR_INVALID, "nle_apply_local: NULL pointer"};
        local_check("nle_apply_local", L, M, h_weights, h_detail, h_curve_on, h_curves, floor, out_kind);
        const DevBuf<float> d_work = local_apply_planes("nle_apply_local", f, d_x, H, W, L, d_strokes, M, h_scale, spread, out_kind, d_out, d_q_out);
        const long long n = f->n_local;  // == H W: world == 1
        local_combine_impl(c, d_x, d_work.p, L, d_work.p + (size_t)L * n, M, n, n, n, h_weights, h_detail, h_curve_on, h_curves,
                           floor, out_kind, d_out);
    });
}

int nle_region_histograms(nle_ctx* ctx, const float* d_y, const float* d_q, int M, long long n, long long q_stride,
                          const double* h_scale, const int* h_row_on, double floor, long long* h_counts) {
    if (!ctx) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        if (!d_y || !d_q || !h_counts) throw Fail{NLE_ERR_INVALID, "nle_region_histograms: NULL pointer"};
        region_hist_check("nle_region_histograms", M, h_scale, floor);
        if (n < 1) throw Fail{NLE_ERR_INVALID, "nle_region_histograms: n must be >= 1"};
        if (q_stride < n) throw Fail{NLE_ERR_INVALID, "nle_region_histograms: the plane stride is smaller than n"};
        region_histograms_impl(ctx, d_y, d_q, M, n, q_stride, h_scale, h_row_on, floor, h_counts);
    });
}

int nle_apply_local_auto(nle_filter* f, const float* d_x, int H, int W, int L, const float* d_strokes, int M,
                         const double* h_scale, double spread, double floor, const double* h_weights, const double* h_detail,
                         const double* h_tone, int out_kind, void* d_out, float* d_q_out, double* h_curves_out) {
    if (!f || !f->ctx) return NLE_ERR_INVALID;
    return guard(f->ctx, [&] {
        nle_ctx* c = f->ctx;
        if (!d_x || !d_strokes || !d_out || !h_tone) throw Fail{NLE_ERR_INVALID, "nle_apply_local_auto: NULL pointer"};
        local_check("nle_apply_local_auto", L, M, h_weights, h_detail, nullptr, nullptr, floor, out_kind);
        int curve_on[NLE_REGION_MAX + 1], hist_on[NLE_REGION_MAX + 1];
        double hist_scale[NLE_REGION_MAX + 1];
        bool any_curve = false, any_hist = false;
        for (int m = 0; m <= M; ++m) {
            const double s = h_tone[4 * m], h = h_tone[4 * m + 1], P = h_tone[4 * m + 2], A = h_tone[4 * m + 3];
            if (const char* refused = nlek::tone_check(s, h, P, A))
                throw Fail{NLE_ERR_INVALID, "nle_apply_local_auto: row " + std::to_string(m) + ": " + refused};
            hist_on[m] = P >= 0 || A > 0;
            curve_on[m] = !(s == 0 && h == 0 && P < 0 && A == 0);
            hist_scale[m] = h_weights[(size_t)m * L + (L - 1)];
            any_curve = any_curve || curve_on[m];
            any_hist = any_hist || hist_on[m];
        }
        const DevBuf<float> d_work = local_apply_planes("nle_apply_local_auto", f, d_x, H, W, L, d_strokes, M, h_scale, spread, out_kind, d_out, d_q_out);
        const long long n = f->n_local;  // == H W: world == 1
        const float* d_q = d_work.p + (size_t)L * n;
        std::vector<long long> counts(any_hist ? (size_t)(M + 1) * nlek::kToneCounts : 0);
        if (any_hist) region_histograms_impl(c, d_work.p + (size_t)(L - 1) * n, d_q, M, n, n, hist_scale, hist_on, floor, counts.data());
        std::vector<double> curves((size_t)(M + 1) * (NLE_TONE_KNOTS + 2), 0.0);
        for (int m = 0; m <= M; ++m) {
            if (!curve_on[m]) continue;
            const double s = h_tone[4 * m], h = h_tone[4 * m + 1];
            const long long* row = hist_on[m] ? counts.data() + (size_t)m * nlek::kToneCounts : nullptr;
            long long mass = 0;
            if (row) mass = std::accumulate(row, row + nlek::kToneCounts, 0ll);
            double* cv = curves.data() + (size_t)m * (NLE_TONE_KNOTS + 2);
            // less than one pixel's mass: the levels and the equalisation have nothing to stand on, the slopes stay
            if (row && mass >= NLE_REGION_WEIGHT_ONE) tone_curve_impl(row, s, h, h_tone[4 * m + 2], h_tone[4 * m + 3], cv);
            else tone_curve_impl(nullptr, s, h, -1, 0, cv);
        }
        if (h_curves_out) std::copy(curves.begin(), curves.end(), h_curves_out);
        local_combine_impl(c, d_x, d_work.p, L, d_q, M, n, n, n, h_weights, h_detail, any_curve ? curve_on : nullptr,
                           any_curve ? curves.data() : nullptr, floor, out_kind, d_out);
    });
}

}  // extern "C"
