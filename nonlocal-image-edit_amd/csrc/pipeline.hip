// Host orchestration of the hot path behind the C ABI (include/nle.h): the Nystrom solve, the train paths
// (NLEFilter::trainFilter, reference src/filter.cpp:480-502), apply (:445-458) and the bodies of the stage entry points.
// Small (p x p, r x r) algebra and the three symmetric eigensolves run on the host in fp64; everything N-sized is a HIP
// kernel.  The sample set, Ka and the fp64 affinity rows -- the patch, chroma and sampler options -- are samples.hip's.
#include "ortho.h"
#include "samples.h"

using nlek::GridSpec;
using namespace nlep;

namespace {
// The image and sample-grid checks of every entry point that takes a plane and sample counts
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


// (c null: everything on the host; the switches come as an argument either way)
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

// B = V_A diag(1/lambda) as fp32 row-major p x ldr
std::vector<float> build_B(const Nystrom& n, int p) {
    std::vector<float> B((size_t)p * n.ldr, 0.f);
    for (int k = 0; k < n.r; ++k) {
        const double inv = recip0(n.lam[k]);
        for (int s = 0; s < p; ++s) B[(size_t)s * n.ldr + k] = (float)(n.VA[(size_t)k * p + s] * inv);
    }
    return B;
}

inline hipError_t scatter_rows_any(hipStream_t s, const float* rows, const long long* idx, int n, int ld, float* d_X,
                                   long long M) {
    return nlek::scatter_rows(s, rows, idx, n, ld, d_X, M);
}
inline hipError_t scatter_rows_any(hipStream_t s, const double* rows, const long long* idx, int n, int ld, double* d_X,
                                   long long M) {
    return nlek::scatter_rows64(s, rows, idx, n, ld, d_X, M);
}

// Exact sample rows: row a of the column-major host matrix src (nrows x K) is written, zero padded to ld, over the row of
// sample a's pixel in the device matrix d_X (this rank's slab [pix0, pix0 + M), ld columns); samples of other slabs are
// skipped.  Returns with the stream drained (the host staging vectors go out of scope).
template <typename T>
void scatter_sample_rows(nle_ctx* c, const std::vector<long long>& pix, int nrows, const std::vector<double>& src, int K,
                         int ld, long long pix0, long long M, T* d_X) {
    std::vector<T> rows;
    std::vector<long long> idx;
    for (int a = 0; a < nrows; ++a) {
        const long long loc = pix[a] - pix0;
        if (loc < 0 || loc >= M) continue;
        idx.push_back(loc);
        const size_t off = rows.size();
        rows.resize(off + ld, T(0));
        for (int k = 0; k < K; ++k) rows[off + k] = (T)src[(size_t)k * nrows + a];
    }
    DevBuf<T> d_rows(rows.size());
    DevBuf<long long> d_idx(idx.size());
    if (!idx.empty()) {
        HIP_OK(hipMemcpyAsync(d_rows.p, rows.data(), rows.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipMemcpyAsync(d_idx.p, idx.data(), idx.size() * sizeof(long long), hipMemcpyHostToDevice, c->stream));
        PROFILED(c, NLE_K_SMALL, scatter_rows_any(c->stream, d_rows.p, d_idx.p, (int)idx.size(), ld, d_X, M));
    }
    HIP_OK(hipStreamSynchronize(c->stream));
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
// The fp64 pass takes the logical width: it never loads a column >= r (nle.h: "leading dimension any value >= the logical
// width"), and its vectors have ld4(r) entries.  The fp32 pass reads whole rows of ld (a multiple of 4, padding zero).
inline hipError_t rowpass_any(hipStream_t s, int mode, const float* X, long long M, int ld, int /*r*/, const double* t,
                              const double* lam, const float* xv, double eps, double* partial, int* nb) {
    return nlek::rowpass(s, mode, X, M, ld, t, lam, xv, eps, partial, nb);
}
inline hipError_t rowpass_any(hipStream_t s, int mode, const double* X, long long M, int ld, int r, const double* t,
                              const double* lam, const float* xv, double eps, double* partial, int* nb) {
    return nlek::rowpass64(s, mode, X, M, ld, r, t, lam, xv, eps, partial, nb);
}
inline int pass_width(const float*, int ld, int /*r*/) { return ld; }
inline int pass_width(const double*, int /*ld*/, int r) { return ld4(r); }

template <typename T_>
void sinkhorn_passes(nle_ctx* c, const T_* d_phi, long long M, int ld_phi, int r,
                     const std::vector<double>& lam, int T, std::vector<double>* u_c,
                     std::vector<double>* u_r, double* d_u_c_out /* pass_width doubles or null */) {
    if (T < 1) throw Fail{NLE_ERR_INVALID, "nSinkhornIter must be >= 1"};
    if (std::is_same<T_, double>::value && r > 2048)
        throw Fail{NLE_ERR_INVALID, "the fp64 Sinkhorn pass takes a logical width of at most 2048"};
    const int ld = pass_width(d_phi, ld_phi, r);  // length of lam, t and of a row of partials (== ld_phi on the train paths)
    std::vector<double> lam_pad(ld, 0.0);
    std::copy(lam.begin(), lam.begin() + r, lam_pad.begin());
    DevBuf<double> d_lam(ld), d_t[3], d_partial((size_t)nlek::kRowpassMaxBlocks * ld);
    for (auto& b : d_t) b.alloc(ld);
    HIP_OK(hipMemcpyAsync(d_lam.p, lam_pad.data(), ld * sizeof(double), hipMemcpyHostToDevice, c->stream));
    int nb = 0;
    // t_r(0) = Phi^T 1
    PROFILED(c, NLE_K_SINKHORN_PASS, rowpass_any(c->stream, nlek::ROWPASS_COLSUM, d_phi, M, ld_phi, r, nullptr, nullptr,
                                                   nullptr, NLE_EPS, d_partial.p, &nb));
    PROFILED(c, NLE_K_REDUCE, nlek::reduce_partials(c->stream, d_partial.p, nb, ld, d_t[0].p));
    all_reduce(c, d_t[0].p, ld);
    // cur = index of the t feeding the next pass
    int cur = 0;
    int idx_c_in = 0, idx_r_in = 0;
    for (int it = 0; it < T; ++it) {
        // c = recip(Phi (lam o t_r));  t_c = Phi^T c
        idx_c_in = cur;
        int nxt = (cur + 1) % 3;
        PROFILED(c, NLE_K_SINKHORN_PASS, rowpass_any(c->stream, nlek::ROWPASS_RECIP, d_phi, M, ld_phi, r, d_t[cur].p,
                                                       d_lam.p, nullptr, NLE_EPS, d_partial.p, &nb));
        PROFILED(c, NLE_K_REDUCE, nlek::reduce_partials(c->stream, d_partial.p, nb, ld, d_t[nxt].p));
        all_reduce(c, d_t[nxt].p, ld);
        cur = nxt;
        idx_r_in = cur;
        if (it + 1 < T) {
            // r = recip(Phi (lam o t_c));  t_r = Phi^T r  (not needed after the last iteration:
            // only u_r = lam o t_c enters the W blocks)
            nxt = (cur + 1) % 3;
            if (nxt == idx_c_in) nxt = (nxt + 1) % 3;
            PROFILED(c, NLE_K_SINKHORN_PASS, rowpass_any(c->stream, nlek::ROWPASS_RECIP, d_phi, M, ld_phi, r, d_t[cur].p,
                                                           d_lam.p, nullptr, NLE_EPS, d_partial.p, &nb));
            PROFILED(c, NLE_K_REDUCE, nlek::reduce_partials(c->stream, d_partial.p, nb, ld, d_t[nxt].p));
            all_reduce(c, d_t[nxt].p, ld);
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

// unpack the upper-triangular ts x ts tile list of gram() / gram64() into a symmetric n x n matrix
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

// ---- the train paths; each fills f->K, ldv, eigvals and d_V or d_V64 (or the table form, f->tables) ----
struct StageMs {
    double sinkhorn = 0, gram = 0, project = 0, host = 0, host_overlapped = 0;
    void take(Timer& s, Timer& g, Timer& p) {
        sinkhorn = s.ms();
        gram = g.ms();
        project = p.ms();
    }
};

// what the filter keeps of the orthogonalisation (Ortho or OrthoSS)
template <typename O>
void adopt_ortho(nle_filter* f, const O& o) {
    f->K = o.K;
    f->ldv = ld4(o.K);
    f->eigvals = o.Sq;
    f->r_wa = o.r_wa;
    f->r_q = o.r_q;
    f->chol_wa = o.chol_wa ? 1 : 0;
}

// (1) materialised Phi: Phi = K_AB^T B written once (N x r fp32), streamed by every later pass
void train_materialised(nle_ctx* c, nle_filter* f, const float* d_lum, const SampleSet& ss, const Nystrom& ny,
                        double hx, double hy, int T, int n_eig, long long pix0, long long M, StageMs* ms) {
    Timer tm_s(c->stream), tm_g(c->stream), tm_p(c->stream);
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
    ms->host += now_ms() - h0;
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
    f->v_bytes = d_V.n * sizeof(float);
    f->d_V = d_V.take();
    ms->take(tm_s, tm_g, tm_p);
}

// (1b) the same literal decomposition with Phi and V in fp64 (generic64.hip): what auto mode falls back to when the
// table form does not apply, and what the 1e-4 bar needs on inputs whose detail layers are small differences
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
std::vector<double> gram_all64(nle_ctx* c, const double* d_phi, long long M, int ld, int r, const double* d_u) {
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

void train_generic64(nle_ctx* c, nle_filter* f, const float* d_lum, const SampleSet& ss, const Nystrom& ny, double hx,
                     double hy, int T, int n_eig, long long pix0, long long M, StageMs* ms) {
    Timer tm_s(c->stream), tm_g(c->stream), tm_p(c->stream);
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
    std::vector<double> G = gram_all64(c, d_phi.p, M, ny.ldr, ny.r, d_u_c.p);
    tm_g.stop();
    double h0 = now_ms();
    Ortho o = orthogonalize_host(ny, ss.p, u_c, u_r, std::move(G), n_eig, /*device_f32=*/false, c->topk_solver, c->sw.trace);
    ms->host += now_ms() - h0;
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
    f->v64_bytes = d_V.n * sizeof(double);
    f->d_V64 = d_V.take();
    ms->take(tm_s, tm_g, tm_p);
}

// Operands of the factored Sinkhorn update (fused.hip: k_sink_update_a/b) from what solve_Ka left: X1 (2p x r column-major)
// and X2 (2p x r row-major) = [B; V_A], lambda.
void build_update_operands(nle_ctx* c, const Nystrom& ny, int p, DevBuf<double>& d_X1, DevBuf<double>& d_X2,
                           DevBuf<double>& d_lam) {
    const int r = ny.r;
    if (ny.dev) {
        // Cholesky form with the factors on the device: X1 = [L^-T; 0] (2p x p column-major), X2 = [L^-T; Ka] row-major --
        // row a of L^-T is column a of L^-1 and Ka is symmetric, so X2 is two plain copies and X1 one transpose
        const size_t n2 = (size_t)2 * p, pp = (size_t)p * p;
        d_X1.alloc(n2 * p);
        d_X2.alloc(n2 * p);
        d_lam.alloc(p);
        HIP_OK(hipMemsetAsync(d_X1.p, 0, n2 * p * sizeof(double), c->stream));
        HIP_OK(nlek::transpose64(c->stream, p, ny.dev->ch.Linv.p, d_X1.p, p, 2 * p));
        HIP_OK(hipMemcpyAsync(d_X2.p, ny.dev->ch.Linv.p, pp * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        HIP_OK(hipMemcpyAsync(d_X2.p + pp, ny.dev->Ka.p, pp * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        HIP_OK(nlek::fill64(c->stream, d_lam.p, p, 1.0));
    } else {
        // X1 (2p x r column-major) and X2 (2p x r row-major) = [B; V_A]; Cholesky form: X1 = [L^-T; 0], the lower
        // half of X2 = the rows of Ka itself (exact projector / exact V_A diag(lambda) V_A^T, see k_sink_update_b)
        const size_t n2 = (size_t)2 * p;
        std::vector<double> X1(n2 * r, 0.0), X2(n2 * r);
        for (int k = 0; k < r; ++k)
            for (int a = 0; a < p; ++a) {
                const double b = ny.B[(size_t)k * p + a];
                const double va = ny.chol ? ny.Ka[(size_t)k * p + a] : ny.VA[(size_t)k * p + a];  // Ka symmetric
                X1[(size_t)k * n2 + a] = b;
                if (!ny.chol) X1[(size_t)k * n2 + p + a] = va;
                X2[(size_t)a * r + k] = b;
                X2[(size_t)(p + a) * r + k] = va;
            }
        d_X1.alloc(X1.size());
        d_X2.alloc(X2.size());
        d_lam.alloc(r);
        HIP_OK(hipMemcpyAsync(d_X1.p, X1.data(), X1.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipMemcpyAsync(d_X2.p, X2.data(), X2.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipMemcpyAsync(d_lam.p, ny.lam.data(), r * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));  // the staging vectors go out of scope (the column-sum pass is done by now)
    }
}

// The Sinkhorn iterations in sample space (reference :238-245 as 2T passes), shared by the table / Phi-free and the
// streamed fp64 formulations.  Each pass has an N-sized half, the caller's pass_pixels(mode, last) -- z = the column sums
// over this rank's pixels under the scaling whose sample-side vector is d_w; the last pass also stores its row scalings c
// -- and a p-sized half here: the all-reduce of z (zrows slices of stride zld), then the factored update (fused.hip).
// Pass n uses the scaling whose sample row sums are sAh[n-1] (and w) and produces sAh[n]; pass 0 is the column sum
// Phi^T 1 (:234,239).  The constructor makes d_w (zero: the pass kernels read its padding up to zld), so it goes where
// the caller's launch order wants that memset.
struct SampleSinkhorn {
    nle_ctx* c;
    int p, T, zld;
    DevBuf<double> d_w, d_sAh, d_X1, d_X2, d_lam, d_uv;
    // sample row sums V_A u of the scaling that defines the final c (input of the last pass) and of the output of the
    // last pass (the r scaling): complete once the stream is drained after run()
    std::vector<double> sA_c, sA_r;

    SampleSinkhorn(nle_ctx* c_, int p_, int zld_, int T_)
        : c(c_), p(p_), T(T_), zld(zld_), d_w(zld_), d_sAh((size_t)2 * T_ * p_), d_uv((size_t)3 * p_) {
        HIP_OK(hipMemsetAsync(d_w.p, 0, zld * sizeof(double), c->stream));
    }

    // `solve` factors Ka on the host (solve_Ka); it is called only after the first pass -- the column sum, which needs
    // nothing of it -- is on the stream, so the factorisation runs under that pass.
    Nystrom run(const std::function<Nystrom()>& solve, const std::function<void(int, bool)>& pass_pixels, double* d_z,
                int zrows) {
        pass_pixels(nlek::ROWPASS_COLSUM, false);
        Nystrom ny = solve();
        build_update_operands(c, ny, p, d_X1, d_X2, d_lam);
        auto update = [&](int n, int mode) {
            all_reduce(c, d_z, (size_t)zrows * zld);
            PROFILED(c, NLE_K_SMALL,
                     nlek::sink_update(c->stream, mode, p, ny.r, ny.chol, d_X1.p, d_X2.p, d_lam.p, d_z, zrows, zld,
                                       n > 0 ? d_sAh.p + (size_t)(n - 1) * p : nullptr, NLE_EPS, d_uv.p, d_uv.p + 2 * p,
                                       d_sAh.p + (size_t)n * p, d_w.p));
        };
        update(0, nlek::ROWPASS_COLSUM);
        for (int n = 1; n < 2 * T; ++n) {
            pass_pixels(nlek::ROWPASS_RECIP, n == 2 * T - 1);
            update(n, nlek::ROWPASS_RECIP);
        }
        // (Fetching these on a second stream, so that the Gram kernels could be queued first, saved ~50 us but made two
        // processes sharing one GPU stall for tens of milliseconds per all-reduce: one stream per ctx it stays.)
        sA_c.resize(p);
        sA_r.resize(p);
        HIP_OK(hipMemcpyAsync(sA_c.data(), d_sAh.p + (size_t)(2 * T - 2) * p, p * sizeof(double), hipMemcpyDeviceToHost,
                              c->stream));
        HIP_OK(hipMemcpyAsync(sA_r.data(), d_sAh.p + (size_t)(2 * T - 1) * p, p * sizeof(double), hipMemcpyDeviceToHost,
                              c->stream));
        return ny;
    }
};

// The host route of the sample-space orthogonalisation, the part that does not need the Gram under the Gram kernels.  The
// fp32 Phi-free form always takes it, the table form with the opt-in Lanczos solver: that one works on the LITERAL q x q
// matrix Q = Wa + S (Wab Wab^T) S with Wa as computed, not mirrored from its lower triangle -- what Spectra's
// DenseGenMatProd multiplies by in a USE_SPECTRA build, src/filter.cpp:174, 311 -- which the host forms exactly; the device
// route diagonalises a symmetric similar matrix.  d_G: what enqueue_gram fills, 16 x 16 upper tiles (gram64) or p x p.
OrthoSS ortho_ss_host(nle_ctx* c, const Nystrom& ny, int p, const SampleSinkhorn& sk, const std::function<void()>& enqueue_gram,
                      double* d_G, size_t g_elems, bool tile16, int n_eig, Timer& tm_g, StageMs* ms, Trace& tr) {
    OrthoSS o;
    enqueue_gram();
    double h0 = now_ms();
    ortho_ss_prepare(o, ny, p, sk.sA_c, sk.sA_r, /*literal_q=*/c->topk_solver != 0, c->sw.force_eig, tr.on);  // host, while the Gram kernel runs
    const double h_overlapped = now_ms() - h0;
    tr.mark("ss: ortho prepare (host)");
    // (a device-to-host copy into pageable memory blocks the host until the stream reaches it, so it
    // is issued only now)
    all_reduce(c, d_G, g_elems);
    std::vector<double> tiles(g_elems);
    HIP_OK(hipMemcpyAsync(tiles.data(), d_G, tiles.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    tm_g.stop();
    HIP_OK(hipStreamSynchronize(c->stream));
    tr.mark("ss: gram sync");
    h0 = now_ms();
    ortho_ss_finish(o, tile16 ? unpack_tiles(tiles, nlek::gram64_ld(p), p, 16) : std::move(tiles), n_eig, c->topk_solver, tr.on);
    ms->host += now_ms() - h0;
    tr.mark("ss: ortho finish (host)");
    ms->host_overlapped += h_overlapped;
    return o;
}

// X (p x K column-major on the host) as the p x ldd row-major, zero-padded operand of project64 / k_apply_small
std::vector<double> padded_rows(const std::vector<double>& X, int p, int K, int ldd) {
    std::vector<double> R((size_t)p * ldd, 0.0);
    for (int k = 0; k < K; ++k)
        for (int a = 0; a < p; ++a) R[(size_t)a * ldd + k] = X[(size_t)k * p + a];
    return R;
}

}  // namespace

// quantised luminance + Cartesian sample grid: table look-ups replace the exponentials (tables.hip), and the pixel halves of
// every table pass run on level-sorted rows, without LDS atomics (sorted.hip; sorted once here).  d_lum: virtual full base.
// Which form each sorted kernel takes is decided here and nowhere else: sorted.hip's bounds on the bandwidth, and the
// switches of the call's snapshot that force a plain form.
nlep::TableFilter::TableFilter(nle_ctx* ctx, const float* d_lum, const SampleSet& ss, double hx, double hy, int row0_, int nrows_)
    : gs(ss.gs), p(ss.p), P64(nlek::sink_pass_ld(ss.p)), row0(row0_), nrows(nrows_), nsw(nsw_of(hx)), npw(nsw_of(hy)),
      lum(d_lum), samples(upload_samples(ctx, ss, nlek::sink_pass_ld(ss.p))), c((size_t)nrows_ * ss.gs.W),
      er((size_t)nrows_ * ss.gs.nSelRows), ecT((size_t)ss.gs.nSelCols * ss.gs.W), Ep((size_t)256 * ss.p),
      sample_loc((size_t)ss.p) {
    {  // the samples' pixel index within this rank's rows (-1: another rank's): known before the first kernel
        const long long pix0 = (long long)row0_ * ss.gs.W, M = (long long)nrows_ * ss.gs.W;
        h_sample_loc.resize(p);
        for (int a = 0; a < p; ++a) {
            const long long loc = ss.pix[a] - pix0;
            h_sample_loc[a] = (loc >= 0 && loc < M) ? loc : -1;
        }
        HIP_OK(hipMemcpyAsync(sample_loc.p, h_sample_loc.data(), p * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    }
    PROFILED(ctx, NLE_K_SMALL, nlek::hist_tables(ctx->stream, gs, samples.p, p, hx, hy, row0, nrows, er.p, ecT.p, Ep.p));
    const nlesw::Switches& sw = ctx->sw;
    if (gs.W > nlek::sorted_max_width() || sw.no_sorted_rows) return;
    scol.alloc(nlek::sorted_scol_elems(gs.W, nrows));  // k_sort_rows writes every entry a pass reads
    first.alloc((size_t)nrows * 258);
    desc.alloc((size_t)nrows * nlek::kSortedThreads);
    E.alloc((size_t)gs.W + 1);
    PROFILED(ctx, NLE_K_SMALL, nlek::dist_table(ctx->stream, gs.W, hx, E.p));
    PROFILED(ctx, NLE_K_SMALL, nlek::sort_rows(ctx->stream, d_lum, gs, row0, nrows, scol.p, desc.p, first.p));
    HIP_OK(hipMemsetAsync(c.p, 0, c.n * sizeof(double), ctx->stream));  // sample pixels are never visited
    sorted = nlek::SortedRows{scol.p, desc.p, first.p, E.p, false, 0.0};
    sorted.rec = nlek::sorted_recurrence(gs, hx, &sorted.kappa) && !sw.sorted_table;  // (kappa is set either way)
    sorted.mom = nlek::sorted_moments_ok(gs, hx) && !sw.sorted_table && !sw.sorted_no_moments;
    sorted.wgs_per_cu = sw.sorted_wgs_per_cu;
    if (!sw.all_level_tiles) {  // the tables' columns of level tiles that do not occur are skipped
        int t0 = 0, t1 = 16;
        while (t0 < 15 && !((ss.level_tiles >> t0) & 1u)) ++t0;
        while (t1 > t0 + 1 && !((ss.level_tiles >> (t1 - 1)) & 1u)) --t1;
        sorted.lev_t0 = t0;
        sorted.lev_nt = t1 - t0;
    }
    if (nlek::sorted_gsum_ok(gs, hx) && !sw.gram_pairs) {  // the Gram on index sums: one more distance table, exp(-2 d^2 / hx^2)
        E2.alloc((size_t)gs.W + 1);
        PROFILED(ctx, NLE_K_SMALL, nlek::dist_table(ctx->stream, gs.W, hx / std::sqrt(2.0), E2.p));
        sorted.E2 = E2.p;
        sorted.hx = hx;
    }
}

// The training plane for the consumers that read it after training (V on demand).  On the level-sorted path it was not
// kept: plane_into rebuilds this rank's rows from the sorted rows and the sample values into `dst` -- exact, the plane is
// integer valued -- and returns the virtual base of the full image; where the plane is held it returns that and leaves
// `dst` alone.  ensure_plane keeps the rebuilt rows in `slab` (V is being materialised: 4 bytes per pixel beside 4 K).
const float* nlep::TableFilter::plane_into(nle_ctx* ctx, DevBuf<float>& dst) const {
    if (lum || !sorted_rows() || nrows <= 0) return lum;
    dst.alloc((size_t)nrows * gs.W);
    PROFILED(ctx, NLE_K_SMALL, nlek::rows_from_sorted(ctx->stream, gs, row0, nrows, sorted, samples.p, p, dst.p));
    return dst.p - (long long)row0 * gs.W;
}
void nlep::TableFilter::ensure_plane(nle_ctx* ctx) { lum = plane_into(ctx, slab); }

namespace {

// (2) the table formulation: every N-sized pass works on look-up tables of the quantised plane; V
// stays implicit (TableFilter)
void train_tables(nle_ctx* c, nle_filter* f, const float* d_lum, const SampleSet& ss, const std::function<Nystrom()>& solve,
                  double hx, double hy, int T, int n_eig, long long pix0, long long M, StageMs* ms) {
    const int p = ss.p;
    Trace tr(c->sw.trace);
    Timer tm_s(c->stream), tm_g(c->stream), tm_p(c->stream);
    tm_s.start();
    auto t = std::make_unique<TableFilter>(c, d_lum, ss, hx, hy, (int)(pix0 / ss.gs.W), (int)(M / ss.gs.W));
    const nlek::TableView view = t->view();
    DevBuf<double> d_z(t->P64), d_hws(nlek::hist_tiled_workspace_elems(ss.gs, t->nrows));
    SampleSinkhorn sk(c, p, t->P64, T);
    tr.mark("ss: alloc+upload");
    auto pass_pixels = [&](int mode, bool last) {  // the N-sized half: the local column sums, straight into d_z
        static const int kmap[4] = {NLE_K_SINK_TABLES, NLE_K_SINKHORN_PASS, NLE_K_REDUCE, NLE_K_REDUCE};
        ProfObserver obs(c, kmap);
        HIP_OK(nlek::sink_hist_tiled(c->stream, mode, view, sk.d_w.p, NLE_EPS, last ? t->c.p : nullptr, d_hws.p, d_z.p, &obs));
    };
    const Nystrom ny = sk.run(solve, pass_pixels, d_z.p, 1);
    f->r = ny.r;
    f->chol_ka = ny.chol ? 1 : 0;
    f->formulation = NLE_MODE_PHI_FREE;
    tm_s.stop();
    tr.mark("ss: passes enqueued");
    HIP_OK(hipStreamSynchronize(c->stream));
    tr.mark("ss: sinkhorn sync");

    // Gram in sample space: histogram + fp64 GEMM over the look-up tables (k_ghist_*), enqueued; the host half that does
    // not need it runs meanwhile
    tm_g.start();
    const size_t g_elems = (size_t)p * p;
    DevBuf<double> d_gpart, d_G(g_elems);
    auto enqueue_gram = [&] {
        d_gpart.alloc(nlek::ghist_workspace_elems(ss.gs, t->nrows));
        static const int gmap[4] = {NLE_K_GRAM_ROWS, NLE_K_SMALL, NLE_K_GRAM_GEMM, NLE_K_SMALL};
        ProfObserver obs(c, gmap);
        HIP_OK(nlek::gram_hist(c->stream, view, d_gpart.p, d_G.p, &obs));
    };
    // what defines V = diag(c) K_AB^T D implicitly (K' <= 128: tables_apply) stays on the device: D and the exact rows of V
    // at the sample pixels, p x ldd row-major, zero padded -- the operands of k_apply_small and project64
    auto place = [&](int K) {
        t->ldd = nlek::project64_ld(K);
        const size_t n = (size_t)p * t->ldd;
        t->D.alloc(n);
        t->Vrows.alloc(n);
        HIP_OK(hipMemsetAsync(t->D.p, 0, n * sizeof(double), c->stream));
        HIP_OK(hipMemsetAsync(t->Vrows.p, 0, n * sizeof(double), c->stream));
        return DeviceDV{t->D.p, t->Vrows.p, t->ldd};
    };
    OrthoSS o;  // (outlives the last synchronisation below: o.staged)
    if (c->topk_solver == 0) {
        // the q-sized products run on the device, the eigensolves on the host; D and Vrows are written where apply reads
        // them and never visit the host
        ortho_ss_device(c, o, ny, p, sk.sA_c, sk.sA_r, d_G.p, n_eig, enqueue_gram, [&] { all_reduce(c, d_G.p, g_elems); },
                        &ms->host, &ms->host_overlapped, tr, place);
        tm_g.stop();
    } else {
        o = ortho_ss_host(c, ny, p, sk, enqueue_gram, d_G.p, g_elems, /*tile16=*/false, n_eig, tm_g, ms, tr);
    }
    adopt_ortho(f, o);

    tm_p.start();
    std::vector<double> Dp, Vr;  // host route only: staged until the synchronisation below
    if (c->topk_solver != 0) {
        const DeviceDV dst = place(o.K);
        Dp = padded_rows(o.D, p, o.K, dst.ldd), Vr = padded_rows(o.Vrows, p, o.K, dst.ldd);
        HIP_OK(hipMemcpyAsync(dst.D, Dp.data(), Dp.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipMemcpyAsync(dst.Vrows, Vr.data(), Vr.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    // the caller's plane is not ours to keep.  With level-sorted rows nothing on the apply path reads the plane, and the
    // rows hold it exactly: it is rebuilt if V is ever asked for (TableFilter::ensure_plane).  Without them the unsorted
    // kernels read it in every apply: keep a copy of this rank's rows.
    if (t->sorted_rows()) {
        t->lum = nullptr;
    } else {
        t->slab.alloc((size_t)M);
        HIP_OK(hipMemcpyAsync(t->slab.p, d_lum + pix0, (size_t)M * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        t->lum = t->slab.p - pix0;
    }
    t->drop_gram_only();
    f->tables = std::move(t);
    tm_p.stop();
    // the one synchronisation after eig(Q): the filter is valid from here, and o.staged / Dp / Vr may go.  (On the stream and
    // not left to the timers' hipEventSynchronize: with that wait alone the gap from the last product to apply's first copy
    // was 176 us, with this one 101 us: profiles/r10_handover.txt, section 2)
    HIP_OK(hipStreamSynchronize(c->stream));
    ms->take(tm_s, tm_g, tm_p);
}

// (2b) Phi-free with fp32 affinities (NLE_MODE_PHI_FREE on a plane that is not integer valued, NLE_MODE_PHI_FREE_EXP): every
// N-sized pass regenerates its affinity rows (fused.hip)
void train_phi_free_exp(nle_ctx* c, nle_filter* f, const float* d_lum, const SampleSet& ss,
                        const std::function<Nystrom()>& solve, double hx, double hy, int T, int n_eig, long long pix0,
                        long long M, StageMs* ms) {
    const int p = ss.p;
    if (p > nlek::sink_pass_max_p()) throw Fail{NLE_ERR_INVALID, "Phi-free path: too many samples for the generic kernels"};
    const int P64 = nlek::sink_pass_ld(p);
    const float nsw = nsw_of(hx), npw = nsw_of(hy);
    Trace tr(c->sw.trace);
    Timer tm_s(c->stream), tm_g(c->stream), tm_p(c->stream);
    tm_s.start();
    // the pass kernel reads the sample table up to the next multiple of 16: pad with zeros (their
    // w entries are zero, so they only have to be finite)
    DevBuf<float4> d_samples = upload_samples(c, ss, P64);
    constexpr int kZS = 8;  // slices of the block partials, summed by k_sink_update
    const int npart = nlek::sink_pass_rows(M);  // M > 0: every rank owns an image row (train_impl)
    DevBuf<double> d_z((size_t)kZS * P64), d_partial((size_t)npart * P64), d_cbuf((size_t)M);
    SampleSinkhorn sk(c, p, P64, T);
    tr.mark("ss: alloc+upload");
    auto pass_pixels = [&](int mode, bool last) {  // the N-sized half: z = sum over this rank's pixels
        PROFILED(c, NLE_K_SINKHORN_PASS, nlek::sink_pass(c->stream, mode, d_lum, ss.gs, d_samples.p, p, sk.d_w.p, nsw, npw, pix0,
                                                         M, NLE_EPS, last ? d_cbuf.p : nullptr, d_partial.p));
        PROFILED(c, NLE_K_REDUCE, nlek::reduce_partials(c->stream, d_partial.p, npart, P64, d_z.p, kZS));
    };
    const Nystrom ny = sk.run(solve, pass_pixels, d_z.p, kZS);
    f->r = ny.r;
    f->chol_ka = ny.chol ? 1 : 0;
    f->formulation = NLE_MODE_PHI_FREE_EXP;
    tm_s.stop();
    tr.mark("ss: passes enqueued");
    HIP_OK(hipStreamSynchronize(c->stream));
    tr.mark("ss: sinkhorn sync");

    // Gram in sample space on regenerated affinity rows (k_gram64, fp64 MFMA), enqueued; the host half that does not need
    // it runs meanwhile
    tm_g.start();
    const size_t g_elems = (size_t)nlek::gram64_num_tiles(p) * 256;
    DevBuf<double> d_gpart(nlek::gram64_partial_elems(M, p)), d_tiles(g_elems);
    const OrthoSS o = ortho_ss_host(
        c, ny, p, sk,
        [&] {
            PROFILED(c, NLE_K_GRAM, nlek::gram64(c->stream, d_lum, ss.gs, d_samples.p, p, nsw, npw, pix0, M, d_cbuf.p, d_gpart.p,
                                                 d_tiles.p));
        },
        d_tiles.p, g_elems, /*tile16=*/true, n_eig, tm_g, ms, tr);
    adopt_ortho(f, o);

    // V = diag(c) K_AB^T D: the Nystrom extension of the K' <= 128 (train_impl) retained eigenvectors, affinity fused
    tm_p.start();
    const std::vector<double> Dp = padded_rows(o.D, p, o.K, nlek::project64_ld(o.K));
    DevBuf<double> d_D(Dp.size());
    HIP_OK(hipMemcpyAsync(d_D.p, Dp.data(), Dp.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    DevBuf<float> d_V((size_t)M * f->ldv);
    PROFILED(c, NLE_K_PROJECT, nlek::project64(c->stream, d_lum, ss.gs, d_samples.p, p, nsw, npw, pix0, M, d_D.p, o.K,
                                               d_cbuf.p, d_V.p, f->ldv));
    tr.mark("ss: project enqueued");
    scatter_sample_rows(c, ss.pix, p, o.Vrows, o.K, f->ldv, pix0, M, d_V.p);
    tm_p.stop();
    HIP_OK(hipStreamSynchronize(c->stream));
    tr.mark("ss: project sync");
    f->v_bytes = d_V.n * sizeof(float);
    f->d_V = d_V.take();
    ms->take(tm_s, tm_g, tm_p);
}

// (3) The same sample-space algebra on fp64 affinity rows (k_affinity64: libm exp of the reference's own argument, :104-112),
// regenerated CHUNK BY CHUNK in every pass: no N x r matrix, a bounded workspace, any luminance plane, any grid up to 2048
// samples, any K.  Every N-sized step is a generic64.hip kernel on the chunk (k_i = row i of the chunk):
//   Sinkhorn half-iteration   y_i = recip(k_i . w), z += k_i y_i                 k_rowpass64 (u := w)
//   Gram                      Gk += sum c_i^2 k_i k_i^T                          k_gram64d
//   eigenvectors              V_i = c_i k_i^T D                                  k_tsgemm64      (V: N x K' fp64, as mode 4)
// and the p-sized side is train_tables' (SampleSinkhorn, ortho_ss_device).  Costs a pass 2 x N p 8 bytes of HBM
// traffic (write + read of the chunk) where the materialised form reads N r 8 once -- the price of not holding it.
void train_stream64(nle_ctx* c, nle_filter* f, const float* d_lum, const SampleSet& ss, const std::function<Nystrom()>& solve,
                    double hx, double hy, int T, int n_eig, long long pix0, long long M, StageMs* ms) {
    const int p = ss.p, ld = ld4(p);
    hipStream_t st = c->stream;
    Trace tr(c->sw.trace);
    Timer tm_s(st), tm_g(st), tm_p(st);
    tm_s.start();
    const size_t budget_mb = (size_t)c->sw.stream64_chunk_mb;
    const long long rows_fit = (long long)((budget_mb << 20) / ((size_t)ld * sizeof(double)));
    const long long CH = std::max<long long>(256, std::min<long long>(std::max<long long>(M, 1), rows_fit));
    const AffinityRows64 kab(c, d_lum, ss, hx, hy, /*want_mask=*/true);
    DevBuf<double> d_K((size_t)CH * ld), d_partial((size_t)nlek::kRowpassMaxBlocks * ld), d_zc(ld), d_z(ld), d_ones(ld),
        d_cbuf((size_t)std::max<long long>(M, 1));
    SampleSinkhorn sk(c, p, ld, T);
    HIP_OK(nlek::fill64(st, d_ones.p, ld, 1.0));
    tr.mark("s64: alloc+upload");
    auto chunk_rows = [&](long long i0) { return std::min<long long>(CH, M - i0); };
    auto gen = [&](long long i0, long long mc) { PROFILED(c, NLE_K_AFFINITY, kab.rows(pix0 + i0, mc, d_K.p, true)); };
    auto pass_pixels = [&](int mode, bool last) {
        HIP_OK(hipMemsetAsync(d_z.p, 0, ld * sizeof(double), st));
        for (long long i0 = 0; i0 < M; i0 += CH) {
            const long long mc = chunk_rows(i0);
            gen(i0, mc);
            int nb = 0;
            PROFILED(c, NLE_K_SINKHORN_PASS, nlek::rowpass64(st, mode, d_K.p, mc, ld, ld, sk.d_w.p, d_ones.p, nullptr, NLE_EPS, d_partial.p, &nb));
            PROFILED(c, NLE_K_REDUCE, nlek::reduce_partials(st, d_partial.p, nb, ld, d_zc.p));
            HIP_OK(nlek::add64(st, d_z.p, d_zc.p, ld));
            if (last) PROFILED(c, NLE_K_SMALL, nlek::row_scalings64(st, d_K.p, mc, ld, p, sk.d_w.p, NLE_EPS, d_cbuf.p + i0));
        }
    };
    const Nystrom ny = sk.run(solve, pass_pixels, d_z.p, 1);
    f->r = ny.r;
    f->chol_ka = ny.chol ? 1 : 0;
    f->formulation = NLE_MODE_STREAMED_F64;
    tm_s.stop();
    HIP_OK(hipStreamSynchronize(st));
    tr.mark("s64: sinkhorn");
    // Gram: Gk = sum over the non-sample pixels of c_i^2 k_i k_i^T, chunk by chunk
    tm_g.start();
    const size_t pp = (size_t)p * p;
    DevBuf<double> d_G(pp), d_Gc(pp), d_gpart(std::max<size_t>(nlek::gram64d_partial_elems(CH, p), 1));
    auto enqueue_gram = [&] {
        HIP_OK(hipMemsetAsync(d_G.p, 0, pp * sizeof(double), st));
        for (long long i0 = 0; i0 < M; i0 += CH) {
            const long long mc = chunk_rows(i0);
            gen(i0, mc);
            PROFILED(c, NLE_K_GRAM, nlek::gram64d(st, d_K.p, mc, ld, p, d_cbuf.p + i0, d_gpart.p, d_Gc.p));
            HIP_OK(nlek::add64(st, d_G.p, d_Gc.p, pp));
        }
    };
    OrthoSS o;
    ortho_ss_device(c, o, ny, p, sk.sA_c, sk.sA_r, d_G.p, n_eig, enqueue_gram, [&] { all_reduce(c, d_G.p, pp); }, &ms->host,
                    &ms->host_overlapped, tr);
    tm_g.stop();
    adopt_ortho(f, o);
    // V = diag(c) K D (the Nystrom extension of the K' kept eigenvectors, :324-327) + the exact sample rows
    tm_p.start();
    DevBuf<double> d_D((size_t)p * o.K), d_V((size_t)std::max<long long>(M, 1) * f->ldv);
    HIP_OK(hipMemcpyAsync(d_D.p, o.D.data(), o.D.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(d_V.p, 0, d_V.n * sizeof(double), st));
    for (long long i0 = 0; i0 < M; i0 += CH) {
        const long long mc = chunk_rows(i0);
        gen(i0, mc);
        PROFILED(c, NLE_K_PROJECT, nlek::ts_gemm64(st, d_K.p, mc, ld, p, d_D.p, o.K, d_cbuf.p + i0, d_V.p + (size_t)i0 * f->ldv, f->ldv));
    }
    scatter_sample_rows(c, ss.pix, p, o.Vrows, o.K, f->ldv, pix0, M, d_V.p);
    tm_p.stop();
    HIP_OK(hipStreamSynchronize(st));
    tr.mark("s64: project");
    f->v64_bytes = d_V.n * sizeof(double);
    f->d_V64 = d_V.take();
    ms->take(tm_s, tm_g, tm_p);
}

// the exact sample rows of V of a table filter on the host, p x K column-major (scatter_sample_rows' operand), fetched from
// the device: only V on demand reads them
std::vector<double> host_Vrows(const nle_filter* f) {
    nle_ctx* c = f->ctx;
    const TableFilter& t = *f->tables;
    std::vector<double> rows((size_t)t.p * t.ldd), out((size_t)t.p * f->K);
    HIP_OK(hipMemcpyAsync(rows.data(), t.Vrows.p, rows.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < f->K; ++k)
        for (int a = 0; a < t.p; ++a) out[(size_t)k * t.p + a] = rows[(size_t)a * t.ldd + k];
    return out;
}

// materialise V = diag(c) K D of a table filter (projection kernel + exact sample rows)
void ensure_V(nle_filter* f) {
    if (f->d_V) return;
    nle_ctx* c = f->ctx;
    if (f->d_V64) {  // fp64 formulation: an fp32 copy for the accessors that hand out float pointers
        DevBuf<float> d_V((size_t)std::max<long long>(f->n_local, 1) * f->ldv);
        HIP_OK(nlek::to_f32(c->stream, f->d_V64, f->n_local * f->ldv, d_V.p));
        HIP_OK(hipStreamSynchronize(c->stream));
        f->v_bytes = d_V.n * sizeof(float);
        f->d_V = d_V.take();
        return;
    }
    if (!f->tables) return;
    f->tables->ensure_plane(c);
    const TableFilter& t = *f->tables;
    const long long M = f->n_local, pix0 = (long long)f->row0 * f->W;
    DevBuf<float> d_V((size_t)std::max<long long>(M, 1) * f->ldv);
    PROFILED(c, NLE_K_PROJECT, nlek::project64(c->stream, t.lum, t.gs, t.samples.p, t.p, t.nsw, t.npw, pix0, M, t.D.p, f->K,
                                               t.c.p, d_V.p, f->ldv));
    scatter_sample_rows(c, f->h_sample_pix, f->p, host_Vrows(f), f->K, f->ldv, pix0, M, d_V.p);
    HIP_OK(hipStreamSynchronize(c->stream));
    f->v_bytes = d_V.n * sizeof(float);
    f->d_V = d_V.take();
}

// apply on the p-sized side of a table filter: reduce half (column sums m = sum_i k_i c_i x_i through the
// tables), the p/K-sized middle (k_apply_small), and one table pass per output layer
// `done(l0, nl)`, when given, is called after layers [l0, l0 + nl) are complete on the stream (the host-buffer entry
// points start their download there); `group` caps the layers per launch (0: as many as fit)
using LayersDone = std::function<void(int, int)>;
void apply_sample_space(nle_filter* f, const float* d_x, const double* h_g /* L x K */, int L, float* d_y,
                        const LayersDone& done = nullptr, int group = 0, bool round8 = false) {
    nle_ctx* c = f->ctx;
    const TableFilter& t = *f->tables;
    const nlek::TableView view = t.view();
    const long long M = f->n_local;
    const int p = t.p, K = f->K, P64 = t.P64;
    DevBuf<double> d_ws(nlek::hist_tiled_workspace_elems(t.gs, t.nrows)), d_m(P64), d_resp((size_t)L * K), d_t(K),
        d_Wp((size_t)L * P64), d_YA((size_t)L * p);
    HIP_OK(hipMemcpyAsync(d_resp.p, h_g, (size_t)L * K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    {
        static const int rmap[4] = {NLE_K_SINK_TABLES, NLE_K_APPLY_REDUCE, NLE_K_REDUCE, NLE_K_REDUCE};
        ProfObserver obs(c, rmap);
        HIP_OK(nlek::sink_hist_tiled(c->stream, nlek::ROWPASS_XVEC, view, nullptr, NLE_EPS, nullptr, d_ws.p, d_m.p, &obs, d_x));
    }
    all_reduce(c, d_m.p, P64);
    // x at the p sample pixels: every rank's own rows, completed by the all-reduce when the planes are slabs
    DevBuf<double> d_xA(p);
    {
        const bool slabs = c->slab_input && c->world > 1;
        PROFILED(c, NLE_K_SMALL, nlek::gather_samples_slab(c->stream, d_x, t.gs, slabs ? f->row0 : 0, slabs ? f->row1 : f->H, d_xA.p));
        if (slabs) all_reduce(c, d_xA.p, p);
    }
    PROFILED(c, NLE_K_SMALL, nlek::apply_small(c->stream, p, K, t.ldd, L, P64, d_m.p, t.D.p, t.Vrows.p, d_xA.p, d_resp.p,
                                               d_t.p, d_Wp.p, d_YA.p));
    static const int emap[4] = {NLE_K_SINK_TABLES, NLE_K_APPLY_EXPAND, NLE_K_REDUCE, NLE_K_REDUCE};
    int lb = std::min(L, nlek::apply_layers_per_launch(view));
    if (group > 0) lb = std::min(lb, group);
    DevBuf<double> d_gws((size_t)lb * t.nrows * 256 * t.gs.nSelCols);
    for (int l = 0; l < L; l += lb) {
        const int nl = std::min(lb, L - l);
        {
            ProfObserver obs(c, emap);
            HIP_OK(nlek::apply_hist_layers(c->stream, view, d_Wp.p + (size_t)l * P64, P64, nl, d_gws.p, d_y + (size_t)l * M, M,
                                           &obs, round8));
        }
        PROFILED(c, NLE_K_SMALL, nlek::scatter_samples(c->stream, p, nl, t.sample_loc.p, d_YA.p + (size_t)l * p,
                                                       d_y + (size_t)l * M, M, round8));
        if (done) done(l, nl);
    }
    HIP_OK(hipStreamSynchronize(c->stream));
    prof_flush(c);
}

// ---- the exact filter (NLE_MODE_EXACT_F64): the reference algorithm with the full N x N affinity in
// place of K_A / K_AB and Phi D Phi^T.  Sinkhorn on the one-column product of exact.hip, then the top-K eigenpairs of
// Ws = (W + W^T) / 2 by thick-restart block Lanczos with full re-orthogonalisation (CGS2 + CholQR2) and explicit
// Rayleigh-Ritz; every product with Ws is one product with K on [c o X | r o X].
constexpr long long kExactMaxBlockProducts = 400;  // block operator applications before NLE_ERR_NUMERIC
constexpr double kExactTol = 1e-10;                // ||Ws v - lambda v||_2 of every kept pair

// the refusals that need no device, the same on every rank (none of them needs a collective)
void check_exact(const nle_ctx* c, int H, int W, int n_eig) {
    if (c->world > 1) throw Fail{NLE_ERR_INVALID, "NLE_MODE_EXACT_F64 runs on one device only (world == 1)"};
    if ((long long)H * W > NLE_EXACT_MAX_PIXELS)
        throw Fail{NLE_ERR_INVALID, "NLE_MODE_EXACT_F64 takes at most NLE_EXACT_MAX_PIXELS (2^20) pixels"};
    if (n_eig > 256) throw Fail{NLE_ERR_INVALID, "NLE_MODE_EXACT_F64 takes at most 256 eigenvectors"};
    const AffinityOpts opts = affinity_opts(c);
    if (opts.patch()) throw Fail{NLE_ERR_INVALID, "NLE_MODE_EXACT_F64 does not take patch affinities (radius must be 0)"};
    if (opts.chroma()) throw Fail{NLE_ERR_INVALID, "NLE_MODE_EXACT_F64 does not take chroma affinities (nle_ctx_set_chroma)"};
    if (opts.listed())
        throw Fail{NLE_ERR_INVALID, "NLE_MODE_EXACT_F64 takes no samples: the sampler must be NLE_SAMPLER_GRID"};
}

void check_exact_plane(nle_ctx* c, const float* d_lum, long long N) {
    DevBuf<int> d_flag(2);
    int fl[2] = {0, 0};
    PROFILED(c, NLE_K_SMALL, nlek::check_levels(c->stream, d_lum, N, d_flag.p));
    HIP_OK(hipMemcpyAsync(fl, d_flag.p, sizeof fl, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    if (fl[0] != 0)
        throw Fail{NLE_ERR_INVALID, "NLE_MODE_EXACT_F64 needs an integer-valued luminance plane in [0, 255] (the L channel of "
                                    "8-bit Lab)"};
}

// Y = K X (exact.hip) with the tables of one plane
struct ExactOperator {
    nle_ctx* c;
    long long N;
    DevBuf<double> es, el, part;
    nlek::ExactPlane pl{};
    ExactOperator(nle_ctx* c_, const float* d_lum, int H, int W, double hx, double hy) : c(c_), N((long long)H * W) {
        std::vector<double> hes, hel;
        nlek::exact_tables(H, W, hx, hy, &hes, &hel);
        es.alloc(hes.size());
        el.alloc(hel.size());
        part.alloc(nlek::exact_part_elems(N));
        HIP_OK(hipMemcpyAsync(es.p, hes.data(), hes.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipMemcpyAsync(el.p, hel.data(), hel.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));  // the host tables go out of scope
        pl = nlek::ExactPlane{d_lum, H, W, es.p, (int)hes.size(), el.p, part.p};
    }
    void product(const double* X, int ldx, int ncols, double* Y, int ldy) {
        HIP_OK(nlek::affinity_product64(c->stream, pl, X, ldx, ncols, Y, ldy));
    }
};

// The device algebra of the eigensolver on N-row matrices (row per pixel)
struct ExactSolver {
    nle_ctx* c;
    ExactOperator& op;
    long long N;
    const double *d_c, *d_r;
    int bmax;
    DevBuf<double> Z, Y;  // N x 2 bmax: [c o X | r o X] and K of it
    double ms_prod = 0, ms_host = 0;
    long long products = 0;  // block operator applications
    ExactSolver(nle_ctx* c_, ExactOperator& op_, const double* dc, const double* dr, int b)
        : c(c_), op(op_), N(op_.N), d_c(dc), d_r(dr), bmax(b), Z((size_t)op_.N * 2 * b), Y((size_t)op_.N * 2 * b) {}
    // A (N x n, ld lda) = Ws X (N x n, ld ldx), bmax columns at a time: Ws X = (r o K(c o X) + c o K(r o X)) / 2
    void apply(const double* X, int ldx, int n, double* A, int lda) {
        const double t0 = now_ms();
        for (int k0 = 0; k0 < n; k0 += bmax) {
            const int b = std::min(bmax, n - k0);
            HIP_OK(nlek::exact_scale2(c->stream, X + k0, ldx, N, b, d_c, d_r, Z.p));
            op.product(Z.p, 2 * b, 2 * b, Y.p, 2 * b);
            HIP_OK(nlek::exact_combine(c->stream, Y.p, N, b, d_c, d_r, A + k0, lda));
            ++products;
        }
        HIP_OK(hipStreamSynchronize(c->stream));
        ms_prod += now_ms() - t0;
    }
    // X^T X (r x r, column-major) over the N rows
    std::vector<double> gram(const double* X, int ld, int r) {
        DevBuf<double> part(nlek::gram64d_partial_elems(N, r)), G((size_t)r * r);
        HIP_OK(nlek::gram64d(c->stream, X, N, ld, r, nullptr, part.p, G.p));
        std::vector<double> h((size_t)r * r);
        HIP_OK(hipMemcpyAsync(h.data(), G.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        return h;
    }
    // C (N x nc, ld ldc) = A (N x kd, ld lda) B (kd x nc column-major, host)
    void gemm(const double* A, int lda, int kd, const std::vector<double>& B, int nc, double* Cp, int ldc) {
        DevBuf<double> d_B(B.size());
        HIP_OK(hipMemcpyAsync(d_B.p, B.data(), B.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_OK(nlek::ts_gemm64(c->stream, A, N, lda, kd, d_B.p, nc, nullptr, Cp, ldc));
        HIP_OK(hipStreamSynchronize(c->stream));  // B (host) is consumed
    }
    // ||A_k - theta_k B_k||_2 of the first n columns, partials summed in block order on the host
    std::vector<double> resid(const double* A, int lda, const double* B, int ldb, const std::vector<double>& theta, int n) {
        const int nb = nlek::exact_col_blocks(N);
        DevBuf<double> d_th(std::max(n, 1)), d_part((size_t)nb * std::max(n, 1));
        HIP_OK(hipMemcpyAsync(d_th.p, theta.data(), n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_OK(nlek::exact_colnorm2(c->stream, A, lda, B, ldb, d_th.p, N, n, d_part.p));
        std::vector<double> h((size_t)nb * n), out(n, 0.0);
        HIP_OK(hipMemcpyAsync(h.data(), d_part.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        for (int k = 0; k < n; ++k) {
            double s = 0.0;
            for (int b = 0; b < nb; ++b) s += h[(size_t)b * n + k];
            out[k] = std::sqrt(s);
        }
        return out;
    }
    // Block W = Q[:, m : m+b] against Q[:, :m] (CGS2; the coefficients are the off-diagonal block of the Gram matrix of
    // Q[:, :m+b], so gram64d serves as the cross product) and within itself (CholQR2).  C1 (m x b, column-major): the
    // first pass's coefficients Q[:, :m]^T W.  false: W is numerically rank deficient.
    bool orth(double* Q, int ldq, int m, int b, double* T, std::vector<double>* C1) {
        double* Wp = Q + m;
        const int n = m + b;
        for (int pass = 0; pass < 2 && m > 0; ++pass) {
            const std::vector<double> G = gram(Q, ldq, n);
            std::vector<double> Cm((size_t)m * b);
            for (int j = 0; j < b; ++j)
                for (int i = 0; i < m; ++i) Cm[(size_t)j * m + i] = G[(size_t)(m + j) * n + i];
            if (pass == 0 && C1) *C1 = Cm;
            gemm(Q, ldq, m, Cm, b, T, b);
            HIP_OK(nlek::exact_axpby(c->stream, Wp, ldq, 1.0, T, b, -1.0, Wp, ldq, N, b, b));
        }
        for (int pass = 0; pass < 2; ++pass) {
            const std::vector<double> G = gram(Wp, ldq, b);
            const double h0 = now_ms();
            std::vector<double> L((size_t)b * b), Li((size_t)b * b), B((size_t)b * b);
            double tr = 0.0, gmax = 0.0;
            for (int k = 0; k < b; ++k) gmax = std::max(gmax, G[(size_t)k * b + k]);
            const bool ok = gmax > 0.0 && nleh::cholesky_with_inverse(G.data(), b, L.data(), Li.data(), &tr) && tr * gmax < 1e12;
            for (int j = 0; j < b; ++j)
                for (int k = 0; k < b; ++k) B[(size_t)j * b + k] = Li[(size_t)k * b + j];  // L^-T
            ms_host += now_ms() - h0;
            if (!ok) return false;
            gemm(Wp, ldq, b, B, b, T, b);
            HIP_OK(nlek::exact_axpby(c->stream, T, b, 1.0, nullptr, 0, 0.0, Wp, ldq, N, b, b));
        }
        return true;
    }
};

// Sinkhorn and the eigensolver of the exact filter; fills f's V (fp64), eigvals, K and timings [1] .. [4]
void train_exact64(nle_ctx* c, nle_filter* f, const float* d_lum, int H, int W, double hx, double hy, int T, int n_eig,
                   Trace& tr) {
    const long long N = (long long)H * W;
    hipStream_t st = c->stream;
    check_exact_plane(c, d_lum, N);
    ExactOperator op(c, d_lum, H, W, hx, hy);
    // Sinkhorn (src/filter.cpp:238-245 on the full K): r = 1; T times c = recip(K r), r = recip(K c)
    const double t_sink = now_ms();
    DevBuf<double> d_r(N), d_c(N);
    {
        const std::vector<double> ones((size_t)N, 1.0);
        HIP_OK(hipMemcpyAsync(d_r.p, ones.data(), N * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_OK(hipStreamSynchronize(st));
    }
    for (int t = 0; t < T; ++t) {
        op.product(d_r.p, 1, 1, d_c.p, 1);
        HIP_OK(nlek::exact_recip(st, d_c.p, N, NLE_EPS));
        op.product(d_c.p, 1, 1, d_r.p, 1);
        HIP_OK(nlek::exact_recip(st, d_r.p, N, NLE_EPS));
    }
    HIP_OK(hipStreamSynchronize(st));
    f->ms[1] = now_ms() - t_sink;
    tr.mark("exact sinkhorn");
    const double t_solve = now_ms();

    const int nev = (int)std::min<long long>(n_eig, N);
    const int b = std::min(64, std::max(16, (nev + 15) / 16 * 16));  // block size
    const int nkeep = nev + std::max(8, b / 2);                          // Ritz pairs kept across a restart
    const int ldq = nkeep + 5 * b;                                       // basis: kept + 4 blocks + the pending one
    const bool dense = N <= ldq;                                         // small plane: the basis is the identity
    ExactSolver sv(c, op, d_c.p, d_r.p, b);
    const int ldt = ld4(dense ? (int)N : nkeep);
    DevBuf<double> V((size_t)N * ldt), AV((size_t)N * ldt);
    std::vector<double> theta;  // Ritz values, descending
    int nk = 0;
    // pairs to certify: the leading nev, up to and including the first Ritz value below the cut
    auto n_need = [&] {
        int need = 0;
        while (need < std::min(nev, nk)) {
            ++need;
            if (theta[need - 1] < NLE_EPS) break;
        }
        return need;
    };
    // Rayleigh-Ritz on the m multiplied columns, Tm = Q^T Ws Q (m x m, symmetric): theta, V = Q S, AV = AQ S
    auto ritz = [&](const double* Q, const double* AQ, int ld, int m, std::vector<double> Tm, int nk_want,
                    std::vector<double>* S_out) -> bool {
        const double h0 = now_ms();
        for (int j = 0; j < m; ++j)
            for (int i = 0; i < j; ++i) {
                const double s = 0.5 * (Tm[(size_t)j * m + i] + Tm[(size_t)i * m + j]);
                Tm[(size_t)j * m + i] = Tm[(size_t)i * m + j] = s;
            }
        std::vector<double> U((size_t)m * m), D(m);
        if (!nleh::sym_eigen(Tm.data(), m, U.data(), D.data()))
            throw Fail{NLE_ERR_NUMERIC, "exact filter: the Rayleigh-Ritz eigensolve did not converge"};
        nk = std::min(nk_want, m);
        theta.assign(nk, 0.0);
        std::vector<double> S((size_t)m * nk);
        for (int k = 0; k < nk; ++k) {
            theta[k] = D[m - 1 - k];
            std::copy(U.begin() + (size_t)(m - 1 - k) * m, U.begin() + (size_t)(m - k) * m, S.begin() + (size_t)k * m);
        }
        sv.ms_host += now_ms() - h0;
        sv.gemm(Q, ld, m, S, nk, V.p, ldt);
        sv.gemm(AQ, ld, m, S, nk, AV.p, ldt);
        if (S_out) *S_out = std::move(S);
        const int need = n_need();
        const std::vector<double> res = sv.resid(AV.p, ldt, V.p, ldt, theta, need);
        for (int k = 0; k < need; ++k)
            if (!(res[k] <= kExactTol)) return false;
        return true;
    };
    // the rule, with an explicit operator application on the Ritz vectors
    auto certify = [&]() -> bool {
        const int need = n_need();
        DevBuf<double> AVe((size_t)N * ldt);
        sv.apply(V.p, ldt, need, AVe.p, ldt);
        const std::vector<double> res = sv.resid(AVe.p, ldt, V.p, ldt, theta, need);
        for (int k = 0; k < need; ++k)
            if (!(res[k] <= kExactTol)) return false;
        return true;
    };
    int restarts = 0;
    if (dense) {
        const int n = (int)N, ldn = ld4(n);
        DevBuf<double> Q((size_t)N * ldn), AQ((size_t)N * ldn);
        std::vector<double> I((size_t)N * ldn, 0.0);
        for (int i = 0; i < n; ++i) I[(size_t)i * ldn + i] = 1.0;
        HIP_OK(hipMemcpyAsync(Q.p, I.data(), I.size() * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_OK(hipStreamSynchronize(st));
        sv.apply(Q.p, ldn, n, AQ.p, ldn);
        std::vector<double> Tm((size_t)n * n), A((size_t)N * ldn);
        HIP_OK(hipMemcpyAsync(A.data(), AQ.p, A.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < n; ++i) Tm[(size_t)j * n + i] = A[(size_t)i * ldn + j];  // Q = I: Q^T AQ = AQ
        if (!ritz(Q.p, AQ.p, ldn, n, std::move(Tm), nev, nullptr) || !certify())
            throw Fail{NLE_ERR_NUMERIC, "exact filter: the dense eigenpairs miss ||Ws v - lambda v|| <= 1e-10"};
    } else {
        DevBuf<double> Q((size_t)N * ldq), AQ((size_t)N * ldq), Tb((size_t)N * b);
        std::vector<double> Tm((size_t)ldq * ldq, 0.0);  // Q^T Ws Q over the multiplied columns, leading dimension ldq
        unsigned seed = 0;
        auto fresh = [&](int m) {  // start vectors in Q[:, m : m+b], a fixed function of (pixel, column, seed)
            for (int tries = 0; tries < 3; ++tries) {
                HIP_OK(nlek::exact_start(st, Q.p, N, ldq, m, b, seed++));
                if (sv.orth(Q.p, ldq, m, b, Tb.p, nullptr)) return;
            }
            throw Fail{NLE_ERR_NUMERIC, "exact filter: cannot extend the Krylov basis"};
        };
        fresh(0);
        int m = 0, qn = b;
        for (;;) {
            if (sv.products >= kExactMaxBlockProducts)
                throw Fail{NLE_ERR_NUMERIC, "exact filter: ||Ws v - lambda v|| <= 1e-10 not reached within " +
                                                std::to_string(kExactMaxBlockProducts) + " block operator applications"};
            sv.apply(Q.p + m, ldq, qn - m, AQ.p + m, ldq);
            // the next block: Ws of this one against the basis; the first CGS pass's coefficients are T's new columns
            HIP_OK(nlek::exact_axpby(st, AQ.p + m, ldq, 1.0, nullptr, 0, 0.0, Q.p + qn, ldq, N, b, b));
            std::vector<double> C1;
            const bool ok = sv.orth(Q.p, ldq, qn, b, Tb.p, &C1);
            for (int j = 0; j < b; ++j)
                for (int i = 0; i < qn; ++i) {
                    Tm[(size_t)(m + j) * ldq + i] = C1[(size_t)j * qn + i];
                    Tm[(size_t)i * ldq + m + j] = C1[(size_t)j * qn + i];
                }
            if (!ok) fresh(qn);
            m = qn;
            qn = m + b;
            if (qn + b <= ldq) continue;
            std::vector<double> Tmm((size_t)m * m), S;
            for (int j = 0; j < m; ++j)
                for (int i = 0; i < m; ++i) Tmm[(size_t)j * m + i] = Tm[(size_t)j * ldq + i];
            if (ritz(Q.p, AQ.p, ldq, m, Tmm, nkeep, &S) && certify()) break;
            // thick restart: the kept Ritz pairs, then the pending block (orthogonal to the whole old basis)
            ++restarts;
            HIP_OK(nlek::exact_axpby(st, V.p, ldt, 1.0, nullptr, 0, 0.0, Q.p, ldq, N, nk, nk));
            HIP_OK(nlek::exact_axpby(st, AV.p, ldt, 1.0, nullptr, 0, 0.0, AQ.p, ldq, N, nk, nk));
            HIP_OK(nlek::exact_axpby(st, Q.p + m, ldq, 1.0, nullptr, 0, 0.0, Q.p + nk, ldq, N, b, b));
            // T of the kept pairs: S^T T S (the Ritz values up to rounding)
            const double h0 = now_ms();
            std::vector<double> TS((size_t)m * nk, 0.0);
            nleh::gemm_nn_cols(Tmm.data(), S.data(), TS.data(), m, m, nk, 0, nk);
            std::vector<double> Tk((size_t)nk * nk, 0.0);
            nleh::gemm_tn_cols(S.data(), TS.data(), Tk.data(), m, nk, nk, 0, nk);
            std::fill(Tm.begin(), Tm.end(), 0.0);
            for (int j = 0; j < nk; ++j)
                for (int i = 0; i < nk; ++i) Tm[(size_t)j * ldq + i] = Tk[(size_t)j * nk + i];
            sv.ms_host += now_ms() - h0;
            m = nk;
            qn = nk + b;
            HIP_OK(hipStreamSynchronize(st));
        }
    }
    tr.mark("exact eigensolver");
    if (tr.on)
        std::fprintf(stderr, "[nle trace] exact: N %lld, %lld block products of up to %d columns (x2), %d restarts\n", N,
                     sv.products, b, restarts);
    int Kp = 0;
    while (Kp < std::min(nev, nk) && theta[Kp] >= NLE_EPS) ++Kp;
    if (Kp == 0) throw Fail{NLE_ERR_NUMERIC, "exact filter: no eigenvalue >= 1e-10"};
    const int ldv = ld4(Kp);
    DevBuf<double> d_V((size_t)N * ldv);
    HIP_OK(nlek::exact_axpby(st, V.p, ldt, 1.0, nullptr, 0, 0.0, d_V.p, ldv, N, Kp, ldv));
    // signs: each column's entry of largest magnitude positive, ties to the lowest index
    const int nb = nlek::exact_col_blocks(N);
    DevBuf<double> d_pv((size_t)nb * Kp), d_s(Kp);
    HIP_OK(nlek::exact_colmaxabs(st, d_V.p, ldv, N, Kp, d_pv.p));
    std::vector<double> pv((size_t)nb * Kp), sgn(Kp, 1.0);
    HIP_OK(hipMemcpyAsync(pv.data(), d_pv.p, pv.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    for (int k = 0; k < Kp; ++k) {
        double best = 0.0;
        for (int blk = 0; blk < nb; ++blk)
            if (std::fabs(pv[(size_t)blk * Kp + k]) > std::fabs(best)) best = pv[(size_t)blk * Kp + k];
        sgn[k] = best < 0.0 ? -1.0 : 1.0;
    }
    HIP_OK(hipMemcpyAsync(d_s.p, sgn.data(), Kp * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_OK(nlek::exact_scale_cols(st, d_V.p, ldv, N, Kp, d_s.p));
    HIP_OK(hipStreamSynchronize(st));
    f->K = Kp;
    f->ldv = ldv;
    f->eigvals.assign(theta.begin(), theta.begin() + Kp);
    f->formulation = NLE_MODE_EXACT_F64;
    f->p = f->r = 0;
    f->r_wa = 0;
    f->r_q = Kp;
    f->v64_bytes = d_V.n * sizeof(double);
    f->d_V64 = d_V.take();
    f->ms[0] = 0.0;
    f->ms[2] = sv.ms_prod;
    f->ms[4] = sv.ms_host;
    f->ms[3] = std::max(0.0, now_ms() - t_solve - sv.ms_prod - sv.ms_host);
}

nle_filter* train_exact_impl(nle_ctx* c, const float* d_lum, int H, int W, double hx, double hy, int T, int n_eig) {
    check_exact(c, H, W, n_eig);
    HIP_OK(hipSetDevice(c->device));
    auto f = new nle_filter();
    try {
        f->ctx = c;
        f->H = H;
        f->W = W;
        f->row0 = 0;
        f->row1 = H;
        f->n_local = (long long)H * W;
        const double t_begin = now_ms();
        pinned_reset(c);
        Trace tr(c->sw.trace);
        train_exact64(c, f, d_lum, H, W, hx, hy, T, n_eig, tr);
        prof_flush(c);
        f->ms[5] = now_ms() - t_begin;
        c->filters.insert(f);
    } catch (...) {
        if (f->d_V64) arena_release(c, f->d_V64, f->v64_bytes);
        delete f;
        throw;
    }
    return f;
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

    auto f = new nle_filter();
    try {
        f->ctx = c;
        f->H = H;
        f->W = W;
        slab(H, c->rank, c->world, &f->row0, &f->row1);
        const long long pix0 = (long long)f->row0 * W;
        const long long M = (long long)(f->row1 - f->row0) * W;
        f->n_local = M;
        if (M <= 0) throw Fail{NLE_ERR_INVALID, "a rank without image rows"};  // (world <= H: cannot happen; the train paths rely on it)
        const double t_begin = now_ms();
        pinned_reset(c);
        Trace tr(c->sw.trace);
        StageMs sm;
        // --- sample set, Ka and its eigenpairs (:486-491, host fp64)
        Timer tm_a(c->stream);
        tm_a.start();
        std::vector<long long> list;
        if (opts.listed()) list = farthest_list(c, d_lum, gs, hx, hy);
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
        sm.host += now_ms() - h0;
        auto solve = [&](bool allow_chol) {
            const double t0 = now_ms();
            Nystrom ny = solve_Ka(c, c->sw, Ka, ss.p, allow_chol);
            tr.mark(ny.chol ? "chol(Ka)" : "eig(Ka)");
            sm.host += now_ms() - t0;
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
        if (fuse && tables_ok && ss.quantised) {
            train_tables(c, f, d_lum, ss, [&] { return solve(true); }, hx, hy, T, n_eig, pix0, M, &sm);
        } else if (fuse) {
            train_phi_free_exp(c, f, d_lum, ss, [&] { return solve(true); }, hx, hy, T, n_eig, pix0, M, &sm);
        } else if (stream64) {
            train_stream64(c, f, d_lum, ss, [&] { return solve(true); }, hx, hy, T, n_eig, pix0, M, &sm);
        } else {
            const Nystrom ny = solve(false);
            f->r = ny.r;
            if (c->mode == NLE_MODE_MATERIALISED)
                train_materialised(c, f, d_lum, ss, ny, hx, hy, T, n_eig, pix0, M, &sm);
            else
                train_generic64(c, f, d_lum, ss, ny, hx, hy, T, n_eig, pix0, M, &sm);
        }
        tr.mark("train path");
        prof_flush(c);
        f->ms[0] = tm_a.ms();
        f->ms[1] = sm.sinkhorn;
        f->ms[2] = sm.gram;
        f->ms[3] = sm.project;
        f->ms[4] = sm.host;
        f->ms[5] = now_ms() - t_begin;
        c->filters.insert(f);
    } catch (...) {
        delete f;
        throw;
    }
    return f;
}

// t = V^T x (all ranks), then Y[l] = V (g_l o t)
// round8: the planes come out clamped to [0, 255] and rounded half to even (src/filter.cpp:434-436) -- on the default path from
// the fp64 value, before anything is rounded to fp32 (other formulations: their fp32 planes, rounded by the caller)
void apply_impl(nle_filter* f, const float* d_x_in, int H, int W, const double* h_g /* L x K */, int L,
                float* d_y, const LayersDone& done = nullptr, int group = 0, bool round8 = false) {
    nle_ctx* c = f->ctx;
    // slab-input mode: d_x_in holds this rank's rows only; index it through the virtual base of the full image
    const float* d_x = (c->slab_input && c->world > 1) ? d_x_in - (size_t)f->row0 * f->W : d_x_in;
    if ((long long)H * W != (long long)f->H * f->W)  // reference src/filter.cpp:447-449
        throw Fail{NLE_ERR_INVALID, "Number of values in channel must match that of training image."};
    if (L < 1 || L > 64) throw Fail{NLE_ERR_INVALID, "number of layers must be in [1, 64]"};
    HIP_OK(hipSetDevice(c->device));
    if (f->tables) {
        apply_sample_space(f, d_x, h_g, L, d_y, done, group, round8);
        return;
    }
    if (!f->d_V64) ensure_V(f);
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
    if (f->d_V64)
        PROFILED(c, NLE_K_APPLY_REDUCE, nlek::rowpass64(c->stream, nlek::ROWPASS_XVEC, f->d_V64, M, ld, ld, nullptr, nullptr,
                                                        d_x + pix0, NLE_EPS, d_partial.p, &nb));
    else
    PROFILED(c, NLE_K_APPLY_REDUCE, nlek::rowpass(c->stream, nlek::ROWPASS_XVEC, f->d_V, M, ld, nullptr, nullptr,
                                                  d_x + pix0, NLE_EPS, d_partial.p, &nb));
    PROFILED(c, NLE_K_REDUCE, nlek::reduce_partials(c->stream, d_partial.p, nb, ld, d_t.p));
    all_reduce(c, d_t.p, ld);
    for (int l = 0; l < L; ++l)
        PROFILED(c, NLE_K_SMALL, nlek::scale_vec(c->stream, d_resp.p + (size_t)l * ld, d_t.p, ld, d_g.p + (size_t)l * ld));
    if (f->d_V64)
        PROFILED(c, NLE_K_APPLY_EXPAND, nlek::apply_expand64(c->stream, f->d_V64, M, ld, f->K, d_g.p, L, d_y, M));
    else
    PROFILED(c, NLE_K_APPLY_EXPAND, nlek::apply_expand(c->stream, f->d_V, M, ld, d_g.p, L, d_y, M));
    if (done) done(0, L);
    HIP_OK(hipStreamSynchronize(c->stream));
    prof_flush(c);
}

void layer_resp(const double* ev, int K, int L, double* out) {
    // detail layer j <-> lambda^j - lambda^(j+1); base <-> lambda^(L-1)  (reference :334-347)
    for (int j = 0; j < L; ++j)
        for (int k = 0; k < K; ++k) {
            const double a = std::pow(ev[k], (double)j);
            out[(size_t)j * K + k] = (j < L - 1) ? a - std::pow(ev[k], (double)(j + 1)) : a;
        }
}

}  // namespace

// ------------------------------------------------------------------------------ C ABI
extern "C" {

int nle_layer_responses(const double* h_eigvals, int K, int L, double* h_resp) {
    if (!h_eigvals || !h_resp || K < 0 || L < 1) return NLE_ERR_INVALID;
    layer_resp(h_eigvals, K, L, h_resp);
    return NLE_OK;
}

int nle_compute_kernel(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples,
                       double hx, double hy, double* h_Ka, float* d_kab) {
    if (!ctx || !d_lum) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        const GridSpec gs = checked_grid(H, W, n_row_samples, n_col_samples);
        check_affinity_opts(ctx, affinity_opts(ctx), gs, H, W, hx, hy, Caller::KERNEL32);
        HIP_OK(hipSetDevice(ctx->device));
        SampleSet ss = fetch_samples(ctx, d_lum, gs, AffinityOpts{});
        if (h_Ka) {
            std::vector<double> Ka = build_Ka(ss, hx, hy);
            std::copy(Ka.begin(), Ka.end(), h_Ka);
        }
        if (d_kab) {
            int row0, row1;
            slab(H, ctx->rank, ctx->world, &row0, &row1);
            DevBuf<float4> d_samples = upload_samples(ctx, ss);
            PROFILED(ctx, NLE_K_AFFINITY,
                     nlek::affinity(ctx->stream, d_lum, gs, d_samples.p, ss.p, ld4(ss.p), nsw_of(hx), nsw_of(hy),
                                    (long long)row0 * W, (long long)(row1 - row0) * W, d_kab));
            HIP_OK(hipStreamSynchronize(ctx->stream));
            prof_flush(ctx);
        }
    });
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
    return guard(ctx, [&] {
        HIP_OK(hipSetDevice(ctx->device));
        std::vector<double> lam(h_eigvals, h_eigvals + r), uc, ur;
        sinkhorn_passes(ctx, d_phi, M, ld, r, lam, max_iter, &uc, &ur, nullptr);
        std::copy(uc.begin(), uc.end(), h_u_c);
        std::copy(ur.begin(), ur.end(), h_u_r);
    });
}

int nle_gram(nle_ctx* ctx, const float* d_phi, long long M, int ld, int r, const double* h_u, double* h_G) {
    if (!ctx || !d_phi || !h_G || M < 0 || r < 1 || ld < r || (ld & 3)) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        HIP_OK(hipSetDevice(ctx->device));
        DevBuf<double> d_u;
        if (h_u) {
            std::vector<double> u(ld, 0.0);
            std::copy(h_u, h_u + r, u.begin());
            d_u.alloc(ld);
            HIP_OK(hipMemcpy(d_u.p, u.data(), ld * sizeof(double), hipMemcpyHostToDevice));
        }
        std::vector<double> G = gram_all(ctx, d_phi, M, ld, r, d_u.p);
        std::copy(G.begin(), G.end(), h_G);
    });
}

int nle_row_scalings(nle_ctx* ctx, const float* d_phi, long long M, int ld, int r, const double* h_u, double* d_out) {
    if (!ctx || !d_phi || !h_u || !d_out || M < 0 || r < 1 || ld < r || (ld & 3)) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        HIP_OK(hipSetDevice(ctx->device));
        std::vector<double> u(ld, 0.0);
        std::copy(h_u, h_u + r, u.begin());
        DevBuf<double> d_u(ld);
        HIP_OK(hipMemcpyAsync(d_u.p, u.data(), ld * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIP_OK(nlek::row_scalings(ctx->stream, d_phi, M, ld, d_u.p, NLE_EPS, d_out));
        HIP_OK(hipStreamSynchronize(ctx->stream));
    });
}

// ---- the same five stage entry points on fp64 device matrices (generic64.hip) ----
int nle_compute_kernel64(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, double hx,
                         double hy, double* h_Ka, double* d_kab) {
    if (!ctx || !d_lum) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        const GridSpec gs = checked_grid(H, W, n_row_samples, n_col_samples);
        const AffinityOpts opts = affinity_opts(ctx);
        check_affinity_opts(ctx, opts, gs, H, W, hx, hy, Caller::KERNEL64);
        HIP_OK(hipSetDevice(ctx->device));
        std::vector<long long> list;
        if (opts.listed()) list = farthest_list(ctx, d_lum, gs, hx, hy);
        FetchSpec spec;
        spec.list = opts.listed() ? &list : nullptr;
        SampleSet ss = fetch_samples(ctx, d_lum, gs, opts, spec);
        require_integer_planes(ctx, ss, /*agree_over_ranks=*/false);
        if (h_Ka) {
            std::vector<double> Ka = build_Ka(ss, hx, hy);
            std::copy(Ka.begin(), Ka.end(), h_Ka);
        }
        if (d_kab) {
            int row0, row1;
            slab(H, ctx->rank, ctx->world, &row0, &row1);
            const AffinityRows64 kab(ctx, d_lum, ss, hx, hy, /*want_mask=*/false);
            PROFILED(ctx, NLE_K_AFFINITY, kab.rows((long long)row0 * W, (long long)(row1 - row0) * W, d_kab));
            HIP_OK(hipStreamSynchronize(ctx->stream));
            prof_flush(ctx);
        }
    });
}

int nle_affinity_product64(nle_ctx* ctx, const float* d_lum, int H, int W, double hx, double hy, const double* d_X, int ld,
                           int ncols, double* d_Y) {
    if (!ctx || !d_lum || !d_X || !d_Y) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        check_image_size(H, W);
        const long long N = (long long)H * W;
        if (N > NLE_EXACT_MAX_PIXELS) throw Fail{NLE_ERR_INVALID, "nle_affinity_product64: more than NLE_EXACT_MAX_PIXELS pixels"};
        if (ncols < 1 || ld < ncols || (ld & 3))
            throw Fail{NLE_ERR_INVALID, "nle_affinity_product64: need 1 <= ncols <= ld, ld a multiple of 4"};
        if (!(hx > 0) || !(hy > 0)) throw Fail{NLE_ERR_INVALID, "hx and hy must be > 0"};
        HIP_OK(hipSetDevice(ctx->device));
        check_exact_plane(ctx, d_lum, N);
        ExactOperator op(ctx, d_lum, H, W, hx, hy);
        HIP_OK(hipMemsetAsync(d_Y, 0, (size_t)N * ld * sizeof(double), ctx->stream));
        op.product(d_X, ld, ncols, d_Y, ld);
        HIP_OK(hipStreamSynchronize(ctx->stream));
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
    return guard(ctx, [&] {
        HIP_OK(hipSetDevice(ctx->device));
        std::vector<double> lam(h_eigvals, h_eigvals + r), uc, ur;
        sinkhorn_passes(ctx, d_phi, M, ld, r, lam, max_iter, &uc, &ur, nullptr);
        std::copy(uc.begin(), uc.end(), h_u_c);
        std::copy(ur.begin(), ur.end(), h_u_r);
    });
}

int nle_gram64(nle_ctx* ctx, const double* d_phi, long long M, int ld, int r, const double* h_u, double* h_G) {
    if (!ctx || !d_phi || !h_G || M < 0 || r < 1 || ld < r) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        HIP_OK(hipSetDevice(ctx->device));
        DevBuf<double> d_u;
        if (h_u) {
            d_u.alloc(r);
            HIP_OK(hipMemcpy(d_u.p, h_u, r * sizeof(double), hipMemcpyHostToDevice));
        }
        std::vector<double> G = gram_all64(ctx, d_phi, M, ld, r, d_u.p);
        std::copy(G.begin(), G.end(), h_G);
    });
}

int nle_row_scalings64(nle_ctx* ctx, const double* d_phi, long long M, int ld, int r, const double* h_u, double* d_out) {
    if (!ctx || !d_phi || !h_u || !d_out || M < 0 || r < 1 || ld < r) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        HIP_OK(hipSetDevice(ctx->device));
        DevBuf<double> d_u(r);
        HIP_OK(hipMemcpyAsync(d_u.p, h_u, r * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIP_OK(nlek::row_scalings64(ctx->stream, d_phi, M, ld, r, d_u.p, NLE_EPS, d_out));
        HIP_OK(hipStreamSynchronize(ctx->stream));
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
        check_image_size(H, W);
        HIP_OK(hipSetDevice(ctx->device));
        size_t npx = (size_t)H * W;  // slab-input mode: h_lum holds this rank's rows only
        if (ctx->slab_input && ctx->world > 1) {
            int r0, r1;
            slab(H, ctx->rank, ctx->world, &r0, &r1);
            npx = (size_t)(r1 - r0) * W;
        }
        DevBuf<float> d_lum(std::max<size_t>(npx, 1));
        HIP_OK(hipMemcpyAsync(d_lum.p, h_lum, npx * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        nle_filter* f = train_impl(ctx, d_lum.p, H, W, n_row_samples, n_col_samples, hx, hy, n_sinkhorn_iter, n_eigen_vectors);
        f->plane_bytes = d_lum.n * sizeof(float);  // kept: nle_apply*_host(h_x == NULL) filters the training plane
        f->d_plane = d_lum.take();
        *out = f;
    });
}

int nle_train_host_u8(nle_ctx* ctx, const unsigned char* h_lum8, int H, int W, int n_row_samples, int n_col_samples, double hx,
                      double hy, int n_sinkhorn_iter, int n_eigen_vectors, nle_filter** out) {
    if (!ctx || !h_lum8 || !out) return NLE_ERR_INVALID;
    *out = nullptr;
    return guard(ctx, [&] {
        check_image_size(H, W);
        HIP_OK(hipSetDevice(ctx->device));
        size_t npx = (size_t)H * W;  // slab-input mode: h_lum8 holds this rank's rows only
        if (ctx->slab_input && ctx->world > 1) {
            int r0, r1;
            slab(H, ctx->rank, ctx->world, &r0, &r1);
            npx = (size_t)(r1 - r0) * W;
        }
        DevBuf<float> d_lum(std::max<size_t>(npx, 1));
        DevBuf<unsigned char> d_u8(std::max<size_t>(npx, 1));  // released after train_impl, which has drained the stream by then
        HIP_OK(hipMemcpyAsync(d_u8.p, h_lum8, npx, hipMemcpyHostToDevice, ctx->stream));
        HIP_OK(nlek::channel8_plane(ctx->stream, d_u8.p, (long long)npx, d_lum.p));
        nle_filter* f = train_impl(ctx, d_lum.p, H, W, n_row_samples, n_col_samples, hx, hy, n_sinkhorn_iter, n_eigen_vectors);
        f->plane_bytes = d_lum.n * sizeof(float);
        f->d_plane = d_lum.take();
        *out = f;
    });
}

void nle_filter_destroy(nle_filter* f) {
    if (!f) return;
    if (f->ctx) f->ctx->filters.erase(f);
    if (f->d_V) arena_release(f->ctx, f->d_V, f->v_bytes);  // back to the ctx's workspace cache (or hipFree)
    if (f->d_plane) arena_release(f->ctx, f->d_plane, f->plane_bytes);
    if (f->d_V64) arena_release(f->ctx, f->d_V64, f->v64_bytes);
    delete f;
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
            if (!d_lum) throw Fail{NLE_ERR_INVALID, "the farthest sampler needs the luminance plane"};
            check_affinity_opts(ctx, opts, gs, H, W, hx, hy, Caller::SAMPLE_PIXELS);
            HIP_OK(hipSetDevice(ctx->device));
            list = farthest_list(ctx, d_lum, gs, hx, hy);
            prof_flush(ctx);
        } else {
            for (int k = 0; k < gs.p(); ++k)
                list[k] = (long long)(gs.rowOff + (k / gs.nSelCols) * gs.rowStep) * W + gs.colOff + (k % gs.nSelCols) * gs.colStep;
        }
        *p = gs.p();
        if (h_idx) std::copy(list.begin(), list.end(), h_idx);
    });
}

int nle_filter_eigvec_range(const nle_filter* f, int ncols, double* h_min, double* h_max) {
    if (!f || !f->ctx || ncols < 1 || ncols > f->K || !h_min || !h_max) return NLE_ERR_INVALID;
    return guard(f->ctx, [&] {
        nle_ctx* c = f->ctx;
        HIP_OK(hipSetDevice(c->device));
        // an implicit V is not materialised for this: only the requested leading columns are projected, into a
        // temporary (the CLI prints the range of 5 of K columns, src/filter.cpp:506)
        const float* d_cols = f->d_V;
        int ldc = f->ldv;
        DevBuf<float> d_tmp;
        if (!f->d_V && f->tables) {
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
            d_cols = f->d_V;
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
    *d_V = f->d_V;
    *ld = f->ldv;
    return NLE_OK;
}

int nle_filter_copy_eigvecs(const nle_filter* f, float* d_out) {
    if (!f || !f->ctx || !d_out) return NLE_ERR_INVALID;
    return guard(f->ctx, [&] {
        HIP_OK(hipSetDevice(f->ctx->device));
        ensure_V(const_cast<nle_filter*>(f));
        HIP_OK(hipMemcpyAsync(d_out, f->d_V, (size_t)f->n_local * f->ldv * sizeof(float), hipMemcpyDeviceToDevice,
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

static void apply_host_common(nle_filter* f, const float* h_x, int H, int W, const double* g, int L, float* h_y) {
    nle_ctx* c = f->ctx;
    if ((long long)H * W != (long long)f->H * f->W)
        throw Fail{NLE_ERR_INVALID, "Number of values in channel must match that of training image."};
    if (!h_x && !f->d_plane)
        throw Fail{NLE_ERR_INVALID, "h_x == NULL needs a filter trained by nle_train_host (it keeps the training plane)"};
    HIP_OK(hipSetDevice(c->device));
    DevBuf<float> d_xbuf, d_y((size_t)L * std::max<long long>(f->n_local, 1));
    const float* d_x = f->d_plane;
    if (h_x) {
        const size_t npx = (c->slab_input && c->world > 1) ? (size_t)f->n_local : (size_t)H * W;
        d_xbuf.alloc(std::max<size_t>(npx, 1));
        HIP_OK(hipMemcpyAsync(d_xbuf.p, h_x, npx * sizeof(float), hipMemcpyHostToDevice, c->stream));
        d_x = d_xbuf.p;
    }
    // each finished group of layers goes home on the copy stream while the next one is computed (the copies are only
    // asynchronous when h_y is pinned: nle_host_alloc)
    if (!c->copy_stream) {
        HIP_OK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        for (auto& e : c->copy_ev) HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    int flip = 0;
    const size_t n = (size_t)f->n_local;
    // whatever happens below (an exception out of apply_impl or of a later callback), no copy may still be reading d_y or
    // writing the caller's h_y when this function is left: d_y goes back to the ctx's cache in its destructor
    struct CopyDrain {
        nle_ctx* c;
        ~CopyDrain() {
            if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
            (void)hipStreamSynchronize(c->stream);
        }
    } drain{c};
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
        if (!f->tables) {  // formulations with fp32 planes: round those
            DevBuf<unsigned char> d_o((size_t)std::max<long long>(f->n_local, 1));
            HIP_OK(nlek::plane_to_u8(f->ctx->stream, d_y, f->n_local, d_o.p));
            HIP_OK(nlek::channel8_plane(f->ctx->stream, d_o.p, f->n_local, d_y));
            HIP_OK(hipStreamSynchronize(f->ctx->stream));
        }
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
        if ((long long)H * W != (long long)f->H * f->W)
            throw Fail{NLE_ERR_INVALID, "Number of values in channel must match that of training image."};
        if (!h_x && !f->d_plane)
            throw Fail{NLE_ERR_INVALID, "h_x == NULL needs a filter trained by nle_train_host (it keeps the training plane)"};
        HIP_OK(hipSetDevice(c->device));
        const size_t n = (size_t)std::max<long long>(f->n_local, 1);
        DevBuf<float> d_xbuf, d_y(n);
        DevBuf<unsigned char> d_o(n);
        const float* d_x = f->d_plane;
        if (h_x) {
            const size_t npx = (c->slab_input && c->world > 1) ? (size_t)f->n_local : (size_t)H * W;
            d_xbuf.alloc(std::max<size_t>(npx, 1));
            HIP_OK(hipMemcpyAsync(d_xbuf.p, h_x, npx * sizeof(float), hipMemcpyHostToDevice, c->stream));
            d_x = d_xbuf.p;
        }
        struct Drain {   // no copy may still be writing the caller's buffer, nor a kernel using d_y, when this is left
            nle_ctx* c;
            ~Drain() { (void)hipStreamSynchronize(c->stream); }
        } drain{c};
        apply_impl(f, d_x, H, W, h_fS, 1, d_y.p, nullptr, 0, /*round8=*/true);
        HIP_OK(nlek::plane_to_u8(c->stream, d_y.p, f->n_local, d_o.p));
        HIP_OK(hipMemcpyAsync(h_out, d_o.p, (size_t)f->n_local, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
    });
}

// ---- region edits (include/nle.h "region edits"; the kernel is region.hip) ----
}  // extern "C"

namespace {

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
    if (out_kind != NLE_REGION_OUT_F32 && out_kind != NLE_REGION_OUT_ROUNDED8 && out_kind != NLE_REGION_OUT_U8)
        throw Fail{NLE_ERR_INVALID, "unknown region output kind " + std::to_string(out_kind) + " (NLE_REGION_OUT_*)"};
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
    if (H <= 0 || W <= 0 || (long long)H * W != (long long)f->H * f->W)  // the text of nle_apply's refusal (:447-449)
        throw Fail{NLE_ERR_INVALID, "Number of values in channel must match that of training image."};
}

void region_combine_impl(nle_ctx* c, const float* d_layers, int L, const float* d_q, int M, long long n, long long layer_stride,
                         long long q_stride, const double* h_weights, double floor, int out_kind, void* d_out) {
    nlek::RegionWeights wt{};
    std::copy(h_weights, h_weights + (size_t)(M + 1) * L, wt.wt);
    HIP_OK(hipSetDevice(c->device));
    HIP_OK(nlek::region_combine(c->stream, d_layers, layer_stride, L, d_q, q_stride, M, n, wt, floor, out_kind, d_out));
    HIP_OK(hipStreamSynchronize(c->stream));
}

// q_m = apply(s_m, c_m lambda^t), one nle_apply per stroke plane
void region_spread_impl(nle_filter* f, const float* d_strokes, int M, int H, int W, const double* h_scale, double spread,
                        float* d_q) {
    std::vector<double> fS((size_t)f->K);
    for (int m = 0; m < M; ++m) {
        const double cm = h_scale ? h_scale[m] : 1.0;
        for (int k = 0; k < f->K; ++k) fS[k] = cm * std::pow(f->eigvals[k], spread);
        apply_impl(f, d_strokes + (size_t)m * H * W, H, W, fS.data(), 1, d_q + (size_t)m * f->n_local);
    }
}

}  // namespace

extern "C" {

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
        std::vector<double> resp((size_t)L * f->K);
        layer_resp(f->eigvals.data(), f->K, L, resp.data());
        apply_impl(f, d_x, H, W, resp.data(), L, d_work.p);  // nle_apply_layers
        region_spread_impl(f, d_strokes, M, H, W, h_scale, spread, d_work.p + (size_t)L * n);
        region_combine_impl(c, d_work.p, L, d_work.p + (size_t)L * n, M, n, n, n, h_weights, floor, out_kind, d_out);
    });
}

int nle_bench_affinity(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, double hx,
                       double hy, float* d_kab, int reps, double* h_avg_ms) {
    if (!ctx || !d_lum || !d_kab || reps < 1 || !h_avg_ms) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        check_image_size(H, W);
        GridSpec gs;
        if (!make_grid(H, W, n_row_samples, n_col_samples, &gs)) throw Fail{NLE_ERR_INVALID, "invalid sample counts"};
        HIP_OK(hipSetDevice(ctx->device));
        SampleSet ss = fetch_samples(ctx, d_lum, gs, AffinityOpts{});
        int row0, row1;
        slab(H, ctx->rank, ctx->world, &row0, &row1);
        DevBuf<float4> d_samples = upload_samples(ctx, ss);
        const float sw = nsw_of(hx), pw = nsw_of(hy);
        const long long pix0 = (long long)row0 * W, M = (long long)(row1 - row0) * W;
        HIP_OK(nlek::affinity(ctx->stream, d_lum, gs, d_samples.p, ss.p, ld4(ss.p), sw, pw, pix0, M, d_kab));
        Timer tm(ctx->stream);
        tm.start();
        for (int i = 0; i < reps; ++i)
            HIP_OK(nlek::affinity(ctx->stream, d_lum, gs, d_samples.p, ss.p, ld4(ss.p), sw, pw, pix0, M, d_kab));
        tm.stop();
        *h_avg_ms = tm.ms() / reps;
    });
}

int nle_bench_affinity64(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples, double hx,
                         double hy, long long rows, double* d_kab, int reps, double* h_avg_ms) {
    if (!ctx || !d_lum || !d_kab || reps < 1 || !h_avg_ms || rows < 1) return NLE_ERR_INVALID;
    return guard(ctx, [&] {
        check_image_size(H, W);
        GridSpec gs;
        if (!make_grid(H, W, n_row_samples, n_col_samples, &gs)) throw Fail{NLE_ERR_INVALID, "invalid sample counts"};
        HIP_OK(hipSetDevice(ctx->device));
        // the plain k_affinity64<false>, whatever the ctx's options are
        SampleSet ss = fetch_samples(ctx, d_lum, gs, AffinityOpts{});
        int row0, row1;
        slab(H, ctx->rank, ctx->world, &row0, &row1);
        const AffinityRows64 kab(ctx, d_lum, ss, hx, hy, /*want_mask=*/false);
        const long long pix0 = (long long)row0 * W, M = std::min<long long>(rows, row1 - row0) * W;
        HIP_OK(kab.rows(pix0, M, d_kab, true));
        Timer tm(ctx->stream);
        tm.start();
        for (int i = 0; i < reps; ++i)
            HIP_OK(kab.rows(pix0, M, d_kab, true));
        tm.stop();
        *h_avg_ms = tm.ms() / reps;
    });
}

int nle_filter_level_tiles(const nle_filter* f, int* first_tile, int* n_tiles) {
    if (!f || !first_tile || !n_tiles) return NLE_ERR_INVALID;
    const nlek::SortedRows* sr = f->tables ? f->tables->sorted_rows() : nullptr;
    *first_tile = sr ? sr->lev_t0 : 0;
    *n_tiles = sr ? sr->lev_nt : 16;
    return NLE_OK;
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
        HIP_OK(nlek::rowpass(ctx->stream, nlek::ROWPASS_RECIP, d_phi, M, ld, d_t.p, d_lam.p, nullptr, NLE_EPS, d_partial.p, &nb));
        Timer tm(ctx->stream);
        tm.start();
        for (int i = 0; i < reps; ++i)
            HIP_OK(nlek::rowpass(ctx->stream, nlek::ROWPASS_RECIP, d_phi, M, ld, d_t.p, d_lam.p, nullptr, NLE_EPS, d_partial.p, &nb));
        tm.stop();
        *h_avg_ms = tm.ms() / reps;
    });
}

}  // extern "C"
