// Host fp64 dense algebra on small column-major matrices and the thread splitter (host_dense.cpp).  Internal to
// libnle_hip.so.
#pragma once

#include <algorithm>
#include <functional>
#include <thread>
#include <vector>

namespace nleh {

// Cholesky factor of a symmetric positive definite matrix (lower triangle of M read): L is n x n column-major lower
// triangular (zeros above the diagonal), Linv = L^-1 likewise.  Returns false if a pivot is not positive.  *inv_trace =
// trace(M^-1) = ||Linv||_F^2, so every eigenvalue of M is at least 1 / *inv_trace: the caller's proof that the
// reference's eigenvalue cut at eps removes nothing.  max_inv_trace > 0: the caller will reject the factor if trace(M^-1) exceeds it -- the factorisation then stops at the
// first pivot that already proves that (returns false)
bool cholesky_with_inverse(const double* M, int n, double* L, double* Linv, double* inv_trace, double max_inv_trace = 0.0);
// its unblocked halves, in place on the lower triangle / X = L^-1 (what the Cholesky-QR of eigen_tridiag.cpp runs)
bool cholesky_lower(int n, double* A, double min_pivot);
void lower_inverse(int n, const double* L, double* X);

// Column ranges [j0, j1) of small column-major products (the caller splits columns over threads):
//   nn: C (m x n) = A (m x k) B (k x n);  nt: C (m x n) = A (m x k) B^T (B n x k);  tn: C (k x n) = A^T B (A m x k, B m x n)
void gemm_nn_cols(const double* A, const double* B, double* C, int m, int k, int n, int j0, int j1);
void gemm_nt_cols(const double* A, const double* B, double* C, int m, int k, int n, int j0, int j1);
void gemm_tn_cols(const double* A, const double* B, double* C, int m, int k, int n, int j0, int j1);

// body(part) for part in [0, nparts) on up to nthreads threads (the caller's plus short-lived helpers); parts are dealt
// round-robin.  run_parts is the same behind a std::function, for callers outside the host algebra.
template <typename F>
void run_split(int nparts, int nthreads, F&& body) {
    nthreads = std::max(1, std::min(nthreads, nparts));
    if (nthreads == 1) {
        for (int q = 0; q < nparts; ++q) body(q);
        return;
    }
    std::vector<std::thread> th;
    auto work = [&](int t) {
        for (int q = t; q < nparts; q += nthreads) body(q);
    };
    for (int t = 1; t < nthreads; ++t) th.emplace_back(work, t);
    work(0);
    for (auto& x : th) x.join();
}
void run_parts(int nparts, int nthreads, const std::function<void(int)>& body);

// threads for the eigensolver's two parallel phases at order n (1 below n = 512, else 8: see host_dense.cpp)
int default_threads(int n, int ncols);

}  // namespace nleh
