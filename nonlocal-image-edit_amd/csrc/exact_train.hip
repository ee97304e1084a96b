// The exact filter (NLE_MODE_EXACT_F64) on the host side: the reference algorithm with the full N x N
// affinity in place of K_A / K_AB and Phi D Phi^T.  Sinkhorn on the one-column product of exact.hip, then the top-K eigenpairs
// of Ws = (W + W^T) / 2 by thick-restart block Lanczos with full re-orthogonalisation (CGS2 + CholQR2) and explicit
// Rayleigh-Ritz; every product with Ws is one product with K on [c o X | r o X].  nle_affinity_product64 exposes the operator.
#include "train.h"

using namespace nlep;

namespace {

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
    // first pass's coefficients Q[:, :m]^T W; w2 (m > 0): the largest squared column norm of W as it came.  false: W is
    // numerically rank deficient.  The first CholQR pass refuses such a block and leaves it as the projection made it; a
    // first pass that went through (condition below 1e12) leaves a block the second pass cannot refuse but for rounding,
    // and then W is rescaled already: `deflate` takes either.
    bool orth(double* Q, int ldq, int m, int b, double* T, std::vector<double>* C1, double* w2 = nullptr) {
        double* Wp = Q + m;
        const int n = m + b;
        for (int pass = 0; pass < 2 && m > 0; ++pass) {
            const std::vector<double> G = gram(Q, ldq, n);
            std::vector<double> Cm((size_t)m * b);
            for (int j = 0; j < b; ++j)
                for (int i = 0; i < m; ++i) Cm[(size_t)j * m + i] = G[(size_t)(m + j) * n + i];
            if (pass == 0 && C1) *C1 = Cm;
            if (pass == 0 && w2) {
                *w2 = 0.0;
                for (int j = 0; j < b; ++j) *w2 = std::max(*w2, G[(size_t)(m + j) * n + m + j]);
            }
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

// The top nev eigenpairs of Ws by Rayleigh-Ritz: on the identity basis when the plane is small (dense), else by thick-restart
// block Lanczos.  After run(): theta[0 .. nk) descending, V the Ritz vectors (N x ldt), every needed pair certified.
struct ExactLanczos {
    nle_ctx* c;
    const long long N;
    // b: block size; nkeep: Ritz pairs kept across a restart; ldq: basis = kept + 4 blocks + the pending one; dense: basis = I
    const int nev, b, nkeep, ldq;
    const bool dense;
    const int ldt;
    ExactSolver sv;
    DevBuf<double> V, AV;
    std::vector<double> theta;  // Ritz values, descending
    int nk = 0, restarts = 0;
    // the Krylov basis Q[:, :qn], Ws of its first m columns, and Tm = Q^T Ws Q over those (leading dimension ldq)
    DevBuf<double> Q, AQ, Tb;
    std::vector<double> Tm;
    int m = 0, qn = 0;
    unsigned seed = 0;

    ExactLanczos(nle_ctx* c_, ExactOperator& op, const double* d_c, const double* d_r, int n_eig)
        : c(c_), N(op.N), nev((int)std::min<long long>(n_eig, N)), b(std::min(64, std::max(16, (nev + 15) / 16 * 16))),
          nkeep(nev + std::max(8, b / 2)), ldq(nkeep + 5 * b), dense(N <= ldq), ldt(ld4(dense ? (int)N : nkeep)),
          sv(c_, op, d_c, d_r, b), V((size_t)N * ldt), AV((size_t)N * ldt) {}

    // pairs to certify: the leading nev, up to and including the first Ritz value below the cut
    int n_need() const {
        int need = 0;
        while (need < std::min(nev, nk)) {
            ++need;
            if (theta[need - 1] < NLE_EPS) break;
        }
        return need;
    }
    // ||AVp_k - theta_k V_k|| <= kExactTol for every needed pair
    bool converged(const double* AVp) {
        const int need = n_need();
        const std::vector<double> res = sv.resid(AVp, ldt, V.p, ldt, theta, need);
        for (int k = 0; k < need; ++k)
            if (!(res[k] <= kExactTol)) return false;
        return true;
    }
    // Rayleigh-Ritz on the mm multiplied columns of Qp, T = Qp^T Ws Qp (mm x mm, symmetric): theta, V = Qp S, AV = AQp S
    bool ritz(const double* Qp, const double* AQp, int ld, int mm, std::vector<double> T, int nk_want, std::vector<double>* S_out) {
        const double h0 = now_ms();
        for (int j = 0; j < mm; ++j)
            for (int i = 0; i < j; ++i) {
                const double s = 0.5 * (T[(size_t)j * mm + i] + T[(size_t)i * mm + j]);
                T[(size_t)j * mm + i] = T[(size_t)i * mm + j] = s;
            }
        std::vector<double> U((size_t)mm * mm), D(mm);
        if (!nleh::sym_eigen(T.data(), mm, U.data(), D.data()))
            throw Fail{NLE_ERR_NUMERIC, "exact filter: the Rayleigh-Ritz eigensolve did not converge"};
        nk = std::min(nk_want, mm);
        theta.assign(nk, 0.0);
        std::vector<double> S((size_t)mm * nk);
        for (int k = 0; k < nk; ++k) {
            theta[k] = D[mm - 1 - k];
            std::copy(U.begin() + (size_t)(mm - 1 - k) * mm, U.begin() + (size_t)(mm - k) * mm, S.begin() + (size_t)k * mm);
        }
        sv.ms_host += now_ms() - h0;
        sv.gemm(Qp, ld, mm, S, nk, V.p, ldt);
        sv.gemm(AQp, ld, mm, S, nk, AV.p, ldt);
        if (S_out) *S_out = std::move(S);
        return converged(AV.p);
    }
    // the rule, with an explicit operator application on the Ritz vectors
    bool certify() {
        DevBuf<double> AVe((size_t)N * ldt);
        sv.apply(V.p, ldt, n_need(), AVe.p, ldt);
        return converged(AVe.p);
    }
    void solve_dense() {
        hipStream_t st = c->stream;
        const int n = (int)N, ldn = ld4(n);
        Q.alloc((size_t)N * ldn), AQ.alloc((size_t)N * ldn);
        std::vector<double> I((size_t)N * ldn, 0.0);
        for (int i = 0; i < n; ++i) I[(size_t)i * ldn + i] = 1.0;
        HIP_OK(hipMemcpyAsync(Q.p, I.data(), I.size() * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_OK(hipStreamSynchronize(st));
        sv.apply(Q.p, ldn, n, AQ.p, ldn);
        std::vector<double> T((size_t)n * n), A((size_t)N * ldn);
        HIP_OK(hipMemcpyAsync(A.data(), AQ.p, A.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < n; ++i) T[(size_t)j * n + i] = A[(size_t)i * ldn + j];  // Q = I: Q^T AQ = AQ
        if (!ritz(Q.p, AQ.p, ldn, n, std::move(T), nev, nullptr) || !certify())
            throw Fail{NLE_ERR_NUMERIC, "exact filter: the dense eigenpairs miss ||Ws v - lambda v|| <= 1e-10"};
    }
    // start vectors in Q[:, at : at+b], a fixed function of (pixel, column, seed)
    void fresh(int at) {
        for (int tries = 0; tries < 3; ++tries) {
            HIP_OK(nlek::exact_start(c->stream, Q.p, N, ldq, at, b, seed++));
            if (sv.orth(Q.p, ldq, at, b, Tb.p, nullptr)) return;
        }
        throw Fail{NLE_ERR_NUMERIC, "exact filter: cannot extend the Krylov basis"};
    }
    // The block Q[:, at : at+b] is orthogonal to the basis but numerically rank deficient (Ws of rank below the basis, as
    // for a plane of few levels under a wide spatial bandwidth).  Its independent directions stay: without them a range
    // whose dimension is no multiple of b never enters the basis whole, and no Ritz pair converges.  Kept: the singular
    // directions within 1e-6 of the block's largest and above 1e-10 of the block as it came (w2: its largest squared
    // column norm), so what the projection left is signal and not its rounding; start vectors fill the other columns.
    // D holds eigenvalues of the Gram matrix, squared singular values: the two thresholds stand squared in the code,
    // 1e-12 and 1e-20.  (After a refusal in orth's second pass the block is near orthonormal and w2 no longer its scale:
    // the second test then passes for every direction and the first one decides.)
    void deflate(int at, double w2) {
        const std::vector<double> G = sv.gram(Q.p + at, ldq, b);
        const double h0 = now_ms();
        std::vector<double> U((size_t)b * b), D(b), B((size_t)b * b, 0.0);
        if (!nleh::sym_eigen(G.data(), b, U.data(), D.data()))
            throw Fail{NLE_ERR_NUMERIC, "exact filter: cannot extend the Krylov basis"};
        int r = 0;  // D ascending
        while (r < b && D[b - 1 - r] > 0.0 && D[b - 1 - r] >= 1e-12 * D[b - 1] && D[b - 1 - r] >= 1e-20 * w2) ++r;
        for (int k = 0; k < r; ++k) {
            const double s = 1.0 / std::sqrt(D[b - 1 - k]);
            for (int i = 0; i < b; ++i) B[(size_t)k * b + i] = s * U[(size_t)(b - 1 - k) * b + i];
        }
        sv.ms_host += now_ms() - h0;
        if (r == 0) return fresh(at);
        sv.gemm(Q.p + at, ldq, b, B, b, Tb.p, b);
        HIP_OK(nlek::exact_axpby(c->stream, Tb.p, b, 1.0, nullptr, 0, 0.0, Q.p + at, ldq, N, b, b));
        for (int tries = 0; tries < 3; ++tries) {
            if (r < b) HIP_OK(nlek::exact_start(c->stream, Q.p, N, ldq, at + r, b - r, seed++));
            if (sv.orth(Q.p, ldq, at, b, Tb.p, nullptr)) return;
        }
        fresh(at);
    }
    // one block step: Ws of the unmultiplied columns, then the next block
    void extend() {
        if (sv.products >= kExactMaxBlockProducts)
            throw Fail{NLE_ERR_NUMERIC, "exact filter: ||Ws v - lambda v|| <= 1e-10 not reached within " +
                                            std::to_string(kExactMaxBlockProducts) + " block operator applications"};
        sv.apply(Q.p + m, ldq, qn - m, AQ.p + m, ldq);
        // the next block: Ws of this one against the basis; the first CGS pass's coefficients are T's new columns
        HIP_OK(nlek::exact_axpby(c->stream, AQ.p + m, ldq, 1.0, nullptr, 0, 0.0, Q.p + qn, ldq, N, b, b));
        std::vector<double> C1;
        double w2 = 0.0;
        const bool ok = sv.orth(Q.p, ldq, qn, b, Tb.p, &C1, &w2);
        for (int j = 0; j < b; ++j)
            for (int i = 0; i < qn; ++i) {
                Tm[(size_t)(m + j) * ldq + i] = C1[(size_t)j * qn + i];
                Tm[(size_t)i * ldq + m + j] = C1[(size_t)j * qn + i];
            }
        if (!ok) deflate(qn, w2);
        m = qn;
        qn = m + b;
    }
    // thick restart: the kept Ritz pairs (S: their coordinates in the old basis, Tmm: its T), then the pending block
    // (orthogonal to the whole old basis)
    void restart(const std::vector<double>& S, const std::vector<double>& Tmm) {
        hipStream_t st = c->stream;
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
    void solve_lanczos() {
        Q.alloc((size_t)N * ldq), AQ.alloc((size_t)N * ldq), Tb.alloc((size_t)N * b);
        Tm.assign((size_t)ldq * ldq, 0.0);
        fresh(0);
        m = 0, qn = b;
        for (;;) {
            extend();
            if (qn + b <= ldq) continue;
            std::vector<double> Tmm((size_t)m * m), S;
            for (int j = 0; j < m; ++j)
                for (int i = 0; i < m; ++i) Tmm[(size_t)j * m + i] = Tm[(size_t)j * ldq + i];
            if (ritz(Q.p, AQ.p, ldq, m, Tmm, nkeep, &S) && certify()) break;
            restart(S, Tmm);
        }
    }
    void run() {
        dense ? solve_dense() : solve_lanczos();
        Tb.release(), AQ.release(), Q.release();  // only V, AV and theta are read from here
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
    ExactLanczos eig(c, op, d_c.p, d_r.p, n_eig);
    eig.run();
    const ExactSolver& sv = eig.sv;
    tr.mark("exact eigensolver");
    if (tr.on)
        std::fprintf(stderr, "[nle trace] exact: N %lld, %lld block products of up to %d columns (x2), %d restarts\n", N,
                     sv.products, eig.b, eig.restarts);
    int Kp = 0;
    while (Kp < std::min(eig.nev, eig.nk) && eig.theta[Kp] >= NLE_EPS) ++Kp;
    if (Kp == 0) throw Fail{NLE_ERR_NUMERIC, "exact filter: no eigenvalue >= 1e-10"};
    const int ldv = ld4(Kp);
    DevBuf<double> d_V((size_t)N * ldv);
    HIP_OK(nlek::exact_axpby(st, eig.V.p, eig.ldt, 1.0, nullptr, 0, 0.0, d_V.p, ldv, N, Kp, ldv));
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
    f->K = Kp, f->ldv = ldv;
    f->eigvals.assign(eig.theta.begin(), eig.theta.begin() + Kp);
    f->formulation = NLE_MODE_EXACT_F64;
    f->r_q = Kp;  // (p, r, r_wa and ms[0] stay 0)
    f->V64 = std::move(d_V);
    f->ms[2] = sv.ms_prod;
    f->ms[4] = sv.ms_host;
    f->ms[3] = std::max(0.0, now_ms() - t_solve - sv.ms_prod - sv.ms_host);
}

}  // namespace

nle_filter* nlep::train_exact_impl(nle_ctx* c, const float* d_lum, int H, int W, double hx, double hy, int T, int n_eig) {
    check_exact(c, H, W, n_eig);
    HIP_OK(hipSetDevice(c->device));
    double t_begin;
    std::unique_ptr<nle_filter> f = begin_train(c, H, W, &t_begin);
    Trace tr(c->sw.trace);
    train_exact64(c, f.get(), d_lum, H, W, hx, hy, T, n_eig, tr);
    return end_train(std::move(f), t_begin);
}

extern "C" int nle_affinity_product64(nle_ctx* ctx, const float* d_lum, int H, int W, double hx, double hy, const double* d_X,
                                      int ld, int ncols, double* d_Y) {
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
