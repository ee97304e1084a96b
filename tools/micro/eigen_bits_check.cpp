// Every output of the host fp64 algebra (csrc/eigen_sym.h, csrc/host_dense.h) on a fixed set of matrices, written raw to a
// file: build it once against the sources of two commits and compare the two files byte for byte.  The bits depend on the
// CPU (which target_clones version runs) and on the compiler, so the files are compared with each other, never stored.
//   build: g++ -O3 -fopenmp-simd -std=c++17 -pthread -Wno-psabi -I <csrc> eigen_bits_check.cpp <csrc>/{eigen_sym,eigen_reduce,
//          eigen_tridiag,host_dense,lanczos}.cpp -o check_new       (an older commit: its eigen_sym.cpp alone, -I its csrc)
//   run:   ./check_new out_new.bin [x8|bisect]      (x8 / bisect: with NLE_EIG_NO_X8 / NLE_EIG_NO_BISECT set);  cmp the outputs
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "eigen_sym.h"
#if __has_include("host_dense.h")
#include "host_dense.h"
#endif

static FILE* out;
static long ncases = 0;
static void put(const std::vector<double>& v) { fwrite(v.data(), sizeof(double), v.size(), out); }
static void put(long long v) { fwrite(&v, sizeof(v), 1, out); ++ncases; }  // one return value = one case
static void putd(double v) { fwrite(&v, sizeof(v), 1, out); }

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static double rnd() {  // uniform in [-0.5, 0.5)
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return (double)(rng_state >> 11) * (1.0 / 9007199254740992.0) - 0.5;
}
// A (n x n) = sum_{k < rank} w^k b_k b_k^T / n + shift I
static std::vector<double> gram(int n, int rank, double w, double shift) {
    std::vector<double> B((size_t)n * rank), A((size_t)n * n, 0.0);
    for (auto& v : B) v = rnd();
    double wk = 1.0;
    for (int k = 0; k < rank; ++k, wk *= w)
        for (int j = 0; j < n; ++j) {
            const double s = wk * B[(size_t)k * n + j] / n;
            for (int i = 0; i < n; ++i) A[(size_t)j * n + i] += B[(size_t)k * n + i] * s;
        }
    for (int i = 0; i < n; ++i) A[(size_t)i * n + i] += shift;
    return A;
}

static const double kFill = -7.0;  // what an output array holds where the library does not write

static void eigen_cases(int n, const std::vector<double>& A) {
    using namespace nleh;
    const double eps = 1e-10;
    std::vector<double> U, D;
    auto fresh = [&](size_t cols) { U.assign((size_t)n * std::max<size_t>(cols, 1), kFill), D.assign(n, kFill); };
    auto done = [&](long long ret) { put(ret), put(U), put(D); };
    fresh(n), done(sym_eigen(A.data(), n, U.data(), D.data()));
    fresh(n), done(sym_eigen_blocked(A.data(), n, U.data(), D.data()));
    int r = -1;
    fresh(n), done(eigen_decomposition(A.data(), n, eps, U.data(), D.data(), &r)), put(r);
    // a matrix "already reduced": T from A's diagonal and sub-diagonal, random reflectors u_i (column i, rows < i) with
    // hs[i] = |u_i|^2 / 2, the scale that makes I - u u^T / hs orthogonal
    std::vector<double> V((size_t)n * n, 0.0), d(n), e(n, 0.0), hs(n, 0.0);
    for (int i = 0; i < n; ++i) {
        d[i] = A[(size_t)i * n + i];
        if (i > 0) e[i] = 0.5 * A[(size_t)(i - 1) * n + i];
        double s = 0.0;
        for (int k = 0; k < i; ++k) V[(size_t)i * n + k] = rnd(), s += V[(size_t)i * n + k] * V[(size_t)i * n + k];
        hs[i] = 0.5 * s;
    }
    std::vector<double> lam(n, kFill), none(1);
    if (n > 1) put(sym_eigen_top_reduced(n, V.data(), d.data(), e.data(), hs.data(), 0, 0, none.data(), lam.data())), put(lam);
    const std::set<int> counts{0, 1, n / 8, n / 2, std::min(n, n / 2 + 1), n};
    for (int k : counts) {
        for (int threads : {0, 3}) fresh(k), done(sym_eigen_top(A.data(), n, k, threads, U.data(), D.data()));
        r = -1, fresh(k), done(eigen_decomposition_top(A.data(), n, eps, k, U.data(), D.data(), &r)), put(r);
        r = -1, fresh(k), done(eigen_decomposition_topk(A.data(), n, eps, k, U.data(), D.data(), &r)), put(r);
        if (n > 1) {  // (the reduced forms are entered with n >= 2 only)
            for (int threads : {0, 3})
                fresh(k), done(sym_eigen_top_reduced(n, V.data(), d.data(), e.data(), hs.data(), k, threads, U.data(), D.data()));
            r = -1, fresh(k), done(eigen_decomposition_top_reduced(n, eps, k, V.data(), d.data(), e.data(), hs.data(), U.data(), D.data(), &r)), put(r);
            for (int first : {0, n / 8})
                if (first + k <= n) fresh(k), done(tridiag_eigenvectors(n, d.data(), e.data(), lam.data(), first, k, U.data()));
        }
        int restarts = -1;
        fresh(k), done(lanczos_topk(A.data(), n, k, 1e-10, 30, U.data(), D.data(), &restarts)), put(restarts);
    }
    for (int max_below : {0, n / 8}) {
        int kept = -1;
        double lmax = kFill, lmin = kFill;
        fresh(max_below);
        done(sym_eigen_below(A.data(), n, eps, max_below, &kept, &lmax, &lmin, D.data(), U.data())), put(kept), putd(lmax), putd(lmin);
    }
}

static void dense_cases(int n, const std::vector<double>& A) {
    using namespace nleh;
    for (double max_tr : {0.0, 1e3}) {
        std::vector<double> L((size_t)n * n, kFill), Li((size_t)n * n, kFill);
        double tr = kFill;
        put(cholesky_with_inverse(A.data(), n, L.data(), Li.data(), &tr, max_tr)), put(L), put(Li), putd(tr);
    }
}

int main(int argc, char** argv) {
    if (argc < 2 || !(out = fopen(argv[1], "wb"))) return 2;
    if (argc > 2 && !strcmp(argv[2], "x8")) setenv("NLE_EIG_NO_X8", "1", 1);
    if (argc > 2 && !strcmp(argv[2], "bisect")) setenv("NLE_EIG_NO_BISECT", "1", 1);
    for (int n : {1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 64, 95, 96, 130, 200, 224, 400, 512, 530}) {
        std::vector<std::vector<double>> mats;
        mats.push_back(gram(n, n, 1.0, 0.05));                   // random SPD
        mats.push_back(gram(n, std::max(1, n - 3), 1.0, 0.0));  // rank n - 3: a cluster below the 1e-10 cut
        mats.push_back(gram(n, n, 0.8, 0.0));                    // geometrically decaying spectrum
        mats.push_back(gram(n, 0, 1.0, 1.0));                    // identity
        mats.push_back(gram(n, 0, 1.0, 0.0));                    // zero
        mats.push_back(mats[0]);                                  // only the lower triangle valid
        for (int c = 0; c < n; ++c)
            for (int rr = 0; rr < c; ++rr) mats.back()[(size_t)c * n + rr] = 12345.678 + rr - c;
        for (const auto& A : mats) eigen_cases(n, A), dense_cases(n, A);
        fprintf(stderr, "n=%d done, %ld cases so far\n", n, ncases);
    }
    {   // indefinite: refused
        std::vector<double> A = {1, 2, 2, 1}, L(4, kFill), Li(4, kFill);
        double tr = kFill;
        put(nleh::cholesky_with_inverse(A.data(), 2, L.data(), Li.data(), &tr)), put(L), put(Li), putd(tr);
    }
    for (auto mkn : {std::vector<int>{37, 19, 23}, std::vector<int>{131, 67, 45}, std::vector<int>{7, 1, 3}}) {
        const int m = mkn[0], k = mkn[1], n = mkn[2];  // odd sizes, two column ranges
        std::vector<double> A((size_t)m * k), Bnn((size_t)k * n), Bnt((size_t)n * k), Btn((size_t)m * n);
        for (auto* v : {&A, &Bnn, &Bnt, &Btn})
            for (auto& x : *v) x = rnd();
        std::vector<double> C1((size_t)m * n, kFill), C2((size_t)m * n, kFill), C3((size_t)k * n, kFill);
        for (int j0 : {0, n / 3}) {
            const int j1 = j0 ? n : n / 3;
            nleh::gemm_nn_cols(A.data(), Bnn.data(), C1.data(), m, k, n, j0, j1);
            nleh::gemm_nt_cols(A.data(), Bnt.data(), C2.data(), m, k, n, j0, j1);
            nleh::gemm_tn_cols(A.data(), Btn.data(), C3.data(), m, k, n, j0, j1);
        }
        put(3), put(C1), put(C2), put(C3);
    }
    for (int threads : {1, 3, 64}) {
        std::vector<double> hit(37, kFill);
        nleh::run_parts(37, threads, [&](int q) { hit[q] = 2.0 * q + 1.0; });
        put(threads), put(hit);
    }
    fclose(out);
    printf("%ld cases written\n", ncases);
    return 0;
}
