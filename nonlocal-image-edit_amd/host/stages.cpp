// The reference's stage functions over the C ABI (include/nle/filter.hpp: computeKernel, eigenDecomposition,
// nystromApproximation, sinkhorn, orthogonalize, transformEigenValues) and the small host glue beside them (operator*,
// eigen2opencv, opencv2eigen).  Mirrors the reference's src/filter.cpp function by function; every N-sized product runs
// in libnle_hip.so on the GPU on fp64 device matrices (nle_*64), the p x p algebra stays here in fp64.
#include <algorithm>
#include <cmath>

#include "surface_internal.hpp"

namespace nle {

using namespace surface;

Mat operator*(const Mat& a, const Mat& b) {
    if (a.cols() != b.rows()) throw std::runtime_error("matrix product: shape mismatch");
    Mat c(a.rows(), b.cols());
    for (int j = 0; j < b.cols(); ++j)
        for (int k = 0; k < a.cols(); ++k) {
            const double bv = b(k, j);
            for (int i = 0; i < a.rows(); ++i) c(i, j) += a(i, k) * bv;
        }
    return c;
}

Image eigen2opencv(const Vec& v, int nrows, int ncols) {  // include/utils.hpp:21-26 (clone)
    Image m(nrows, ncols, NLE_64F, 1);
    std::copy(v.data(), v.data() + (size_t)nrows * ncols, m.ptr<double>());
    return m;
}

Vec opencv2eigen(const Image& mat) {  // include/utils.hpp:28-41, row-major flatten
    Vec lv((int)mat.total());
    int k = 0;
    for (int i = 0; i < mat.rows; i++)
        for (int j = 0; j < mat.cols; j++) lv(k++) = mat.at<double>(i, j);
    return lv;
}

// ------------------------------------------------------------------ computeKernel, :114-167
std::tuple<Permutation, Mat, Mat> computeKernel(const Image& mat, int nRowSamples, int nColSamples, DType hx,
                                                DType hy) {
    if (nRowSamples > mat.rows || nColSamples > mat.cols)
        throw std::runtime_error("Number of samples per row and col must be <= that of image.");
    nle_ctx* c = shared_ctx();
    const int H = mat.rows, W = mat.cols;
    const long long N = (long long)H * W;
    int rs, ro, nr, cs, co, nc;
    if (nle_sample_grid(H, W, nRowSamples, nColSamples, &rs, &ro, &nr, &cs, &co, &nc) != NLE_OK)
        throw std::runtime_error("Number of samples per row and col must be <= that of image.");
    const int p = nr * nc, ld = nle_ld(p);
    std::vector<float> lum = plane_f32(mat);
    Dev d_lum(c, (size_t)N * 4), d_kab(c, (size_t)N * ld * 8);
    check(nle_dev_upload(c, d_lum.p, lum.data(), (size_t)N * 4), c);
    Mat Ka(p, p);
    check(nle_compute_kernel64(c, d_lum.f(), H, W, nRowSamples, nColSamples, hx, hy, Ka.data(), d_kab.d()), c);
    std::vector<double> kab((size_t)N * ld);
    check(nle_dev_download(c, kab.data(), d_kab.p, kab.size() * 8), c);
    // [selected; rest] order, both in row-major scan order (:56-80, :156-164)
    Permutation P;
    P.idx.resize((size_t)N);
    std::vector<char> sel((size_t)N, 0);
    int k = 0;
    for (int i = 0; i < nr; ++i)
        for (int j = 0; j < nc; ++j) {
            const int pix = to1DIndex(ro + i * rs, co + j * cs, W);
            P.idx[(size_t)k++] = pix;
            sel[(size_t)pix] = 1;
        }
    Mat Kab(p, (int)(N - p));
    int jrest = 0;
    for (long long pix = 0; pix < N; ++pix) {
        if (sel[(size_t)pix]) continue;
        P.idx[(size_t)(p + jrest)] = (int)pix;
        const double* row = kab.data() + (size_t)pix * ld;
        for (int i = 0; i < p; ++i) Kab(i, jrest) = row[i];
        ++jrest;
    }
    return std::make_tuple(P, Ka, Kab);
}

// ------------------------------------------------------------------ eigenDecomposition, :204-228
std::pair<Mat, Vec> eigenDecomposition(const Mat& M, DType eps) {
    const int n = M.rows();
    if (n == 0 || M.cols() != n) throw std::runtime_error("eigenDecomposition: square matrix expected");
    Mat U(n, n);
    Vec D(n);
    int r = 0;
    if (nle_eigen_decomposition(M.data(), n, eps, U.data(), D.data(), &r) != NLE_OK)
        throw std::runtime_error("eigenDecomposition: no convergence");
    return std::make_pair(U.leftCols(r), D.head(r));
}

// ------------------------------------------------------------------ nystromApproximation, :257-280
std::pair<Vec, Mat> nystromApproximation(const Mat& Ka, const Mat& Kab) {
    nle_ctx* c = shared_ctx();
    Mat eigvecs;
    Vec eigvals;
    std::tie(eigvecs, eigvals) = eigenDecomposition(Ka);
    int nnz = 0;
    for (int i = 0; i < eigvals.size(); ++i)
        if (std::fabs(eigvals(i)) >= EPS) ++nnz;  // :265-266
    eigvecs = eigvecs.leftCols(nnz);
    eigvals = eigvals.head(nnz);
    const int p = Ka.rows(), r = nnz, n_rest = Kab.cols(), n = p + n_rest;
    Mat B(p, r);  // eigvecs * invEigVals
    for (int k = 0; k < r; ++k)
        for (int s = 0; s < p; ++s) B(s, k) = eigvecs(s, k) * recip0(eigvals(k));
    Mat phi(n, r);
    for (int k = 0; k < r; ++k)
        for (int s = 0; s < p; ++s) phi(s, k) = eigvecs(s, k);
    if (n_rest > 0 && r > 0) {
        const int lda = nle_ld(p), ldc = nle_ld(r);
        std::vector<double> rows = cols_as_rows_f64(Kab, lda);
        Dev d_A(c, rows.size() * 8), d_C(c, (size_t)n_rest * ldc * 8);
        check(nle_dev_upload(c, d_A.p, rows.data(), rows.size() * 8), c);
        check(nle_ts_gemm64(c, d_A.d(), n_rest, lda, p, B.data(), r, d_C.d()), c);  // Kab^T * B, :275
        std::vector<double> out((size_t)n_rest * ldc);
        check(nle_dev_download(c, out.data(), d_C.p, out.size() * 8), c);
        for (int j = 0; j < n_rest; ++j)
            for (int k = 0; k < r; ++k) phi(p + j, k) = out[(size_t)j * ldc + k];
    }
    return std::make_pair(eigvals, phi);
}

// ------------------------------------------------------------------ sinkhorn, :230-254
std::pair<Mat, Mat> sinkhorn(const Mat& phi, const Vec& eigvals, int maxIter) {
    nle_ctx* c = shared_ctx();
    const int n = phi.rows(), r = phi.cols();
    if (r == 0 || n == 0) throw std::runtime_error("sinkhorn: empty phi");
    if (maxIter < 1) throw std::runtime_error("sinkhorn: maxIter must be >= 1");
    const int ld = nle_ld(r);
    std::vector<double> rows((size_t)n * ld, 0.0);
    for (int k = 0; k < r; ++k)
        for (int i = 0; i < n; ++i) rows[(size_t)i * ld + k] = phi(i, k);
    Dev d_phi(c, rows.size() * 8), d_c(c, (size_t)n * 8);
    check(nle_dev_upload(c, d_phi.p, rows.data(), rows.size() * 8), c);
    std::vector<double> u_c(r), u_r(r);
    check(nle_sinkhorn_scalings64(c, d_phi.d(), n, ld, r, eigvals.data(), maxIter, u_c.data(), u_r.data()), c);
    check(nle_row_scalings64(c, d_phi.d(), n, ld, r, u_c.data(), d_c.d()), c);
    std::vector<double> cv((size_t)n);
    check(nle_dev_download(c, cv.data(), d_c.p, cv.size() * 8), c);
    const int q = r;  // :247  p = phi.cols()
    if (q > n) throw std::runtime_error("sinkhorn: phi has more columns than rows");
    // left = R * (phi_top * D)
    Mat left(q, r), right(q, r);
    for (int a = 0; a < q; ++a) {
        double sr = 0.0;
        for (int k = 0; k < r; ++k) sr += rows[(size_t)a * ld + k] * u_r[k];
        const double ra = recip0(sr);
        for (int k = 0; k < r; ++k) {
            const double v = rows[(size_t)a * ld + k];
            left(a, k) = ra * v * eigvals(k);
            right(a, k) = cv[(size_t)a] * v;
        }
    }
    Mat Wa = left * right.transpose();  // :249
    Mat Wab(q, n - q);
    if (n > q) {
        const int ldq = nle_ld(q);
        Mat lt = left.transpose();  // r x q
        Dev d_out(c, (size_t)(n - q) * ldq * 8);
        check(nle_ts_gemm64(c, d_phi.d() + (size_t)q * ld, n - q, ld, r, lt.data(), q, d_out.d()), c);
        std::vector<double> out((size_t)(n - q) * ldq);
        check(nle_dev_download(c, out.data(), d_out.p, out.size() * 8), c);
        for (int j = 0; j < n - q; ++j)
            for (int a = 0; a < q; ++a) Wab(a, j) = out[(size_t)j * ldq + a] * cv[(size_t)(q + j)];  // :250
    }
    return std::make_pair(Wa, Wab);
}

// ------------------------------------------------------------------ orthogonalize, :282-331
std::pair<Mat, Vec> orthogonalize(const Mat& Wa, const Mat& Wab, int nEigVectors, DType eps) {
    nle_ctx* c = shared_ctx();
    const int q = Wa.rows(), nb = Wab.cols();
    Mat eigvecs;
    Vec eigvals;
    std::tie(eigvecs, eigvals) = eigenDecomposition(Wa, eps);
    const int r2 = eigvals.size();
    Mat Us(q, r2);
    for (int k = 0; k < r2; ++k) {
        const double s = std::sqrt(recip0(eigvals(k), eps));
        for (int i = 0; i < q; ++i) Us(i, k) = eigvecs(i, k) * s;
    }
    Mat invRootWa = Us * eigvecs.transpose();  // :292
    Mat G(q, q);
    const int ldq = nle_ld(q);
    std::vector<double> rows = cols_as_rows_f64(Wab, ldq);  // Wab^T, one row per pixel
    Dev d_X(c, std::max<size_t>(rows.size(), 1) * 8);
    if (nb > 0) {
        check(nle_dev_upload(c, d_X.p, rows.data(), rows.size() * 8), c);
        check(nle_gram64(c, d_X.d(), nb, ldq, q, nullptr, G.data()), c);  // Wab * Wab^T, :296
    }
    Mat Q = invRootWa * G * invRootWa;
    for (int j = 0; j < q; ++j)
        for (int i = 0; i < q; ++i) Q(i, j) += Wa(i, j);
    Mat Vq;
    Vec Sq;
    std::tie(Vq, Sq) = eigenDecomposition(Q, eps);  // :313
    const int k = std::min(nEigVectors, Vq.cols());
    Vq = Vq.leftCols(k);
    Sq = Sq.head(k);
    Mat C = invRootWa * Vq;  // q x k
    for (int j = 0; j < k; ++j) {
        const double s = std::sqrt(recip0(Sq(j), eps));  // :319-321
        for (int i = 0; i < q; ++i) C(i, j) *= s;
    }
    Mat V(q + nb, k);
    Mat top = Wa * C;
    for (int j = 0; j < k; ++j)
        for (int i = 0; i < q; ++i) V(i, j) = top(i, j);
    if (nb > 0 && k > 0) {
        const int ldk = nle_ld(k);
        Dev d_out(c, (size_t)nb * ldk * 8);
        check(nle_ts_gemm64(c, d_X.d(), nb, ldq, q, C.data(), k, d_out.d()), c);  // Wab^T * C, :327
        std::vector<double> out((size_t)nb * ldk);
        check(nle_dev_download(c, out.data(), d_out.p, out.size() * 8), c);
        for (int i = 0; i < nb; ++i)
            for (int j = 0; j < k; ++j) V(q + i, j) = out[(size_t)i * ldk + j];
    }
    return std::make_pair(V, Sq);
}

// ------------------------------------------------------------------ transformEigenValues, :334-347
Vec transformEigenValues(const Vec& eigvals, const std::vector<DType>& weights) {
    if (weights.empty()) throw std::runtime_error("transformEigenValues: at least one weight is required");
    Vec fS(eigvals.size());
    if (nle_transform_eigenvalues(eigvals.data(), eigvals.size(), weights.data(), (int)weights.size(), fS.data()) !=
        NLE_OK)
        throw std::runtime_error("transformEigenValues: bad arguments");
    return fS;
}

}  // namespace nle
