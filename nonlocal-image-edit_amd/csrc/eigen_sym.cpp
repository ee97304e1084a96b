// Host fp64 symmetric eigensolver, the front ends: which stages (eigen_stages.h) a caller's question needs, the order of
// the results and the reference's rank cut.  The stages live in eigen_reduce.cpp (dense <-> tridiagonal) and
// eigen_tridiag.cpp (everything on (d, e)); Cholesky, the small products and the thread splitter in host_dense.cpp.
//
// Replaces Eigen::SelfAdjointEigenSolver at the reference's call site src/filter.cpp:207-210 (Eigen3 is a system
// dependency of the reference, version floor 3.3, not vendored).  Same contract: symmetric input, LOWER triangle
// referenced, orthonormal eigenvectors; `eigen_decomposition` adds the reference's post-processing (:209-216).
#include "eigen_sym.h"
#include "eigen_stages.h"
#include "host_dense.h"
#include "switches.h"

#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

namespace nleh {

namespace {

EigOpts read_opts() {  // every public function: once, on entry; what it calls is handed the result
    const nlesw::Switches sw = nlesw::read_switches();
    return EigOpts{sw.eig_no_bisect, sw.eig_no_x8};
}

// the order that sorts d: ascending and stable, reversed as a whole for descending (every front end breaks ties alike)
std::vector<int> sorted_order(const double* d, int n, bool descending) {
    std::vector<int> idx(n);
    std::iota(idx.begin(), idx.end(), 0);
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return d[a] < d[b]; });
    if (descending) std::reverse(idx.begin(), idx.end());
    return idx;
}

// reference src/filter.cpp:209-216: D is descending, keep the leading run >= eps
int leading_run(const double* D, int n, double eps) {
    int r = 0;
    while (r < n && D[r] >= eps) ++r;
    return r;
}

struct Rotations {
    std::vector<Sweep> sweeps;
    std::vector<double> cs, sn;
};
bool record_rotations(int n, double* d, double* e, Rotations& r) {
    r.cs.reserve((size_t)n * n);
    r.sn.reserve((size_t)n * n);
    return ql_record(n, d, e, r.sweeps, r.cs, r.sn);
}

// U (n x ncols) = columns idx[0 .. ncols) of Z0 R, R the product of the recorded rotations, Z0 n x n (null: the identity).
// The rotations run over 64-row blocks of a padded copy, one block per part: cache resident and free of barriers.
void rotated_columns(int n, const double* Z0, const Rotations& r, const int* idx, int ncols, int nthreads, double* U) {
    const int ldz = (n + 7) & ~7;  // rows padded to whole 8-row vectors (the padding stays zero)
    // (64-byte aligned: the 64-row blocks of different threads then never share a cache line)
    std::vector<double> Zbuf((size_t)ldz * n + 8, 0.0);
    double* Z = Zbuf.data();
    while (reinterpret_cast<uintptr_t>(Z) & 63) ++Z;
    for (int j = 0; j < n; ++j) {
        if (Z0) std::copy(Z0 + (size_t)j * n, Z0 + (size_t)j * n + n, Z + (size_t)j * ldz);
        else Z[(size_t)j * ldz + j] = 1.0;
    }
    const int nvec = ldz / 8, nblocks = (nvec + 7) / 8;
    run_split(nblocks, nthreads, [&](int b) {
        apply_rotations_rows(ldz, Z, b * 64, std::min(8, nvec - b * 8), r.sweeps.data(), r.sweeps.size(), r.cs.data(), r.sn.data());
    });
    for (int j = 0; j < ncols; ++j) std::copy(Z + (size_t)idx[j] * ldz, Z + (size_t)idx[j] * ldz + n, U + (size_t)j * n);
}

// the reduction of M and what bisection needs of its tridiagonal form (the result points into red.d: keep red alive)
SturmT reduce_for_bisection(const double* M, int n, Reduced& red) {
    red = reduce_lower(M, n);
    return sturm_setup(n, red.d.data(), red.e.data());
}

// The part of sym_eigen_top after the reduction: V (n x n, u_i in column i rows 0..i-1), hs, and the tridiagonal (d, e) as
// tridiag_reduce -- or the device kernel k_tridiag (tridiag.hip), same conventions -- leaves them.
bool top_reduced(int n, const double* V, const double* d_in, const double* e_in, const double* hs, int ncols, int nthreads,
                 double* U, double* D, const EigOpts& o) {
    if (nthreads <= 0) nthreads = default_threads(n, ncols);
    std::vector<double> d(d_in, d_in + n), e(e_in, e_in + n);
    const std::vector<double> d0(d), e0(e);  // T itself (the QL iteration overwrites d and e)
    Rotations rot;
    // a leading part of the spectrum: the eigenvectors come from inverse iteration, the rotations are not needed (should
    // the inverse iteration give up, the iteration is repeated with recording below)
    const bool invit = ncols > 0 && 2 * ncols <= n;
    if (invit || ncols == 0) {
        if (!ql_values(n, d.data(), e.data())) return false;
    } else if (!record_rotations(n, d.data(), e.data(), rot)) {
        return false;
    }
    const std::vector<int> idx = sorted_order(d.data(), n, true);
    for (int j = 0; j < n; ++j) D[j] = d[idx[j]];
    if (ncols == 0) return true;
    auto back_transform = [&] {
        const int cparts = std::max(1, std::min(nthreads, (ncols + 3) / 4));
        run_split(cparts, nthreads, [&](int q) {
            const int j0 = (int)((long long)ncols * q / cparts), j1 = (int)((long long)ncols * (q + 1) / cparts);
            back_transform_cols(n, V, hs, U, j0, j1);
        });
    };
    if (invit) {
        if (tridiag_inverse_iteration(n, d0.data(), e0.data(), D, ncols, U, o)) {
            back_transform();
            return true;
        }
        // inverse iteration gave up: the rotations after all
        d = d0, e = e0;
        if (!record_rotations(n, d.data(), e.data(), rot)) return false;
    }
    rotated_columns(n, nullptr, rot, idx.data(), ncols, nthreads, U);
    back_transform();
    return true;
}

bool top(const double* M, int n, int ncols, int nthreads, double* U, double* D, const EigOpts& o) {
    if (n <= 0) return true;
    ncols = std::max(0, std::min(ncols, n));
    if (n == 1) {
        D[0] = M[0];
        if (ncols) U[0] = 1.0;
        return true;
    }
    const Reduced t = reduce_lower(M, n);
    return top_reduced(n, t.V.data(), t.d.data(), t.e.data(), t.hs.data(), ncols, nthreads, U, D, o);
}

bool decomposition_top(const double* M, int n, double eps, int kmax, double* U, double* D, int* r_out, const EigOpts& o) {
    kmax = std::max(0, std::min(kmax, n));
    if (2 * kmax > n && default_threads(n, kmax) == 1) {
        // most eigenvectors wanted, one thread: accumulating the orthogonal factor (classic form) is cheaper
        // than back-transforming them one by one (n = 200: 1.65 ms against 1.9 ms; n = 900: 116 against 124 ms,
        // but ~70 ms once the two phases are threaded)
        std::vector<double> Ua((size_t)n * n), Da(n);
        if (!sym_eigen_blocked(M, n, Ua.data(), Da.data())) return false;
        for (int j = 0; j < n; ++j) {  // ascending -> descending
            const int src = n - 1 - j;
            D[j] = Da[src];
            if (j < kmax) std::copy(Ua.begin() + (size_t)src * n, Ua.begin() + (size_t)src * n + n, U + (size_t)j * n);
        }
    } else if (!top(M, n, kmax, 0, U, D, o)) {
        return false;
    }
    *r_out = leading_run(D, n, eps);
    return true;
}

// sym_eigen_below without bisection: all eigenvalues DESCENDING in D by the QL iteration, *kept_out = the leading run
// >= eps; if at most max_below follow it, their eigenvectors in U by inverse iteration and back-transformation.
// (n == 1 returns before *kept_out is written, as it always has: the caller's value stands.)
bool below_by_ql(const double* M, int n, double eps, int max_below, int* kept_out, double* D, double* U, const EigOpts& o) {
    if (n == 1) D[0] = M[0];
    if (n <= 1) return true;
    Reduced t = reduce_lower(M, n);
    const std::vector<double> d0(t.d), e0(t.e);
    if (!ql_values(n, t.d.data(), t.e.data())) return false;
    std::sort(t.d.begin(), t.d.end(), [](double a, double b) { return a > b; });
    std::copy(t.d.begin(), t.d.end(), D);
    const int kept = *kept_out = leading_run(D, n, eps);
    const int count = (n - kept <= max_below) ? n - kept : 0;
    if (count == 0) return true;
    if (!tridiag_inverse_iteration(n, d0.data(), e0.data(), D + kept, count, U, o)) return false;
    back_transform_cols(n, t.V.data(), t.hs.data(), U, 0, count);
    return true;
}

}  // namespace

bool sym_eigen(const double* M, int n, double* U, double* D) {
    if (n <= 0) return true;
    mirror_lower(M, n, U);
    std::vector<double> e(n);
    if (n == 1) {
        D[0] = U[0];
        U[0] = 1.0;
        return true;
    }
    tridiagonalize(n, U, D, e.data());
    if (!ql_implicit(n, U, D, e.data())) return false;
    const std::vector<int> idx = sorted_order(D, n, false);
    std::vector<double> Ds(n), Us((size_t)n * n);
    for (int j = 0; j < n; ++j) {
        Ds[j] = D[idx[j]];
        std::copy(U + (size_t)idx[j] * n, U + (size_t)idx[j] * n + n, Us.begin() + (size_t)j * n);
    }
    std::copy(Ds.begin(), Ds.end(), D);
    std::copy(Us.begin(), Us.end(), U);
    return true;
}

// All eigenvectors on one thread: the classic reduction WITH accumulation of the orthogonal factor (cheaper than
// back-transforming n vectors one reflector at a time), then the recorded rotations applied to it by cache-resident
// row blocks instead of column pair by column pair.
bool sym_eigen_blocked(const double* M, int n, double* U, double* D) {
    if (n <= 2) return sym_eigen(M, n, U, D);
    std::vector<double> V((size_t)n * n), d(n), e(n);
    mirror_lower(M, n, V.data());
    tridiagonalize(n, V.data(), d.data(), e.data());
    Rotations rot;
    if (!record_rotations(n, d.data(), e.data(), rot)) return false;
    const std::vector<int> idx = sorted_order(d.data(), n, false);
    for (int j = 0; j < n; ++j) D[j] = d[idx[j]];
    rotated_columns(n, V.data(), rot, idx.data(), n, 1, U);
    return true;
}

bool sym_eigen_top(const double* M, int n, int ncols, int nthreads, double* U, double* D) {
    return top(M, n, ncols, nthreads, U, D, read_opts());
}

bool sym_eigen_top_reduced(int n, const double* V, const double* d, const double* e, const double* hs, int ncols, int nthreads,
                           double* U, double* D) {
    return top_reduced(n, V, d, e, hs, ncols, nthreads, U, D, read_opts());
}

bool eigen_decomposition_top_reduced(int n, double eps, int kmax, const double* V, const double* d, const double* e,
                                     const double* hs, double* U, double* D, int* r_out) {
    kmax = std::max(0, std::min(kmax, n));
    if (!top_reduced(n, V, d, e, hs, kmax, 0, U, D, read_opts())) return false;
    *r_out = leading_run(D, n, eps);
    return true;
}

bool eigen_decomposition_top(const double* M, int n, double eps, int kmax, double* U, double* D, int* r_out) {
    return decomposition_top(M, n, eps, kmax, U, D, r_out, read_opts());
}

bool eigen_decomposition(const double* M, int n, double eps, double* U, double* D, int* r_out) {
    return decomposition_top(M, n, eps, n, U, D, r_out, read_opts());
}

// Householder reduction, eigenvalues by bisection (a count is a chain of n - 1 divisions, eight shifts a vector: the K
// leading eigenvalues cost ~55 sweeps of T, not an implicit QL run for all n), eigenvectors by inverse iteration and
// back-transformation.  For 2 kmax <= n; otherwise, and should the inverse iteration give up: decomposition_top.
bool eigen_decomposition_topk(const double* M, int n, double eps, int kmax, double* U, double* Dk, int* r_out) {
    const EigOpts o = read_opts();
    kmax = std::max(0, std::min(kmax, n));
    auto by_ql = [&] {
        std::vector<double> D(n);
        if (!decomposition_top(M, n, eps, kmax, U, D.data(), r_out, o)) return false;
        std::copy(D.begin(), D.begin() + kmax, Dk);
        return true;
    };
    if (n < 8 || 2 * kmax > n || o.no_bisect) return by_ql();
    Reduced red;
    const SturmT t = reduce_for_bisection(M, n, red);
    *r_out = n - sturm_count1(t, eps);  // descending order: the leading run >= eps IS the count of eigenvalues >= eps
    sturm_eigenvalues_desc(t, 0, kmax, Dk);
    if (kmax == 0) return true;
    if (!tridiag_inverse_iteration(n, red.d.data(), red.e.data(), Dk, kmax, U, o)) return by_ql();
    back_transform_cols(n, red.V.data(), red.hs.data(), U, 0, kmax);
    return true;
}

// One Sturm count for the cut; lambda_max, the smallest kept eigenvalue and (if few) the ones below the cut are one or
// two vectors of shifts.  Below n = 8, or with NLE_EIG_NO_BISECT, the QL form above answers the same question.
bool sym_eigen_below(const double* M, int n, double eps, int max_below, int* kept_out, double* lam_max, double* lam_min_kept,
                     double* Dbelow, double* U) {
    const EigOpts o = read_opts();
    if (n < 8 || o.no_bisect) {
        std::vector<double> D(n);
        if (!below_by_ql(M, n, eps, max_below, kept_out, D.data(), U, o)) return false;
        const int kept = *kept_out;
        *lam_max = D[0];
        *lam_min_kept = kept > 0 ? D[kept - 1] : 0.0;
        if (n - kept <= max_below) std::copy(D.begin() + kept, D.end(), Dbelow);
        return true;
    }
    Reduced red;
    const SturmT t = reduce_for_bisection(M, n, red);
    const int kept = n - sturm_count1(t, eps);
    *kept_out = kept;
    const int nb = n - kept;
    std::vector<int> k{n - 1, kept > 0 ? n - kept : n - 1};
    if (nb <= max_below)
        for (int j = 0; j < nb; ++j) k.push_back(nb - 1 - j);
    std::vector<double> out(k.size());
    for (size_t j0 = 0; j0 < k.size(); j0 += 64) sturm_bisect(t, k.data() + j0, (int)std::min<size_t>(64, k.size() - j0), out.data() + j0);
    *lam_max = out[0];
    *lam_min_kept = kept > 0 ? out[1] : 0.0;
    if (nb <= max_below) std::copy(out.begin() + 2, out.end(), Dbelow);
    if (nb == 0 || nb > max_below) return true;
    if (!tridiag_inverse_iteration(n, red.d.data(), red.e.data(), Dbelow, nb, U, o)) return false;
    back_transform_cols(n, red.V.data(), red.hs.data(), U, 0, nb);
    return true;
}

bool tridiag_eigenvectors(int n, const double* d, const double* e, const double* lam_all, int first, int count, double* Z) {
    if (count <= 0) return true;
    if (tridiag_inverse_iteration(n, d, e, lam_all + first, count, Z, read_opts())) return true;
    // the classic iteration on T itself: rotations accumulated from the identity
    std::vector<double> V((size_t)n * n, 0.0), dd(d, d + n), ee(e, e + n);
    for (int i = 0; i < n; ++i) V[(size_t)i * n + i] = 1.0;
    if (!ql_implicit(n, V.data(), dd.data(), ee.data())) return false;
    const std::vector<int> idx = sorted_order(dd.data(), n, true);
    for (int j = 0; j < count; ++j)
        std::copy(V.begin() + (size_t)idx[first + j] * n, V.begin() + (size_t)idx[first + j] * n + n, Z + (size_t)j * n);
    return true;
}

}  // namespace nleh
