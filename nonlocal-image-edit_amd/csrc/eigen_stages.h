// The stages of the host fp64 symmetric eigensolver, for its front ends (eigen_sym.cpp) and for tools that time a stage
// (tools/micro/eig_phase_bench.cpp).  Internal to the host algebra: nothing outside it includes this.
//
// Two solvers are built from them.  The classic one (sym_eigen): `tridiagonalize` with the orthogonal factor accumulated,
// then `ql_implicit` rotating its columns.  The one in three barrier-free phases (sym_eigen_top and what sits on it):
//   1. tridiag_reduce: the reduction alone; the Householder vectors u_i stay in column i (rows 0..i-1), scales in hs.
//   2. (d, e) alone: ql_values or bisection for eigenvalues; ql_record RECORDS the plane rotations of every sweep.
//   3. eigenvectors of T, by inverse iteration for a few, else the rotations applied to Z = I by independent row blocks
//      (apply_rotations_rows); then only the wanted columns are back-transformed, by independent column blocks.
// Phase 3 splits over threads without any synchronisation, which the per-sweep update of the classic loop does not allow.
#pragma once
#include <cstddef>
#include <vector>

#include "host_simd.h"

namespace nleh {

// the two measurement switches of the solver (switches.h), read once at each public entry point and handed down
struct EigOpts {
    bool no_bisect, no_x8;
};

// ---- eigen_reduce.cpp: dense symmetric <-> tridiagonal
// M's lower triangle mirrored into V (n x n; SelfAdjointEigenSolver reads only the lower one)
void mirror_lower(const double* M, int n, double* V);
// V: the mirrored matrix in, the orthogonal Q with Q^T A Q = T out (d diagonal, e[1..n) sub-diagonal; e[i] couples i-1 and i)
void tridiagonalize(int n, double* V, double* d, double* e);
// the same T without forming Q: column i of V, rows < i, holds u_i with H_i = I - u_i u_i^T / hs[i]
void tridiag_reduce(int n, double* V, double* d, double* e, double* hs);
// the mirrored M after tridiag_reduce: Householder vectors in V, their scales in hs, T in (d, e)
struct Reduced {
    std::vector<double> V, d, e, hs;
};
Reduced reduce_lower(const double* M, int n);
// columns [j0, j1) of Y (n rows) <- Q Y, Q as tridiag_reduce left it in (V, hs)
void back_transform_cols(int n, const double* V, const double* hs, double* Y, int j0, int j1);

// ---- eigen_tridiag.cpp: everything on (d, e).  The QL forms return false when an eigenvalue does not converge.
struct Sweep {
    int l, m;      // rotations act on columns (i, i+1) for i = m-1 .. l
    size_t first;  // index of the i = m-1 rotation in the (c, s) lists
};
bool ql_implicit(int n, double* V, double* d, double* e);  // rotations accumulated into V's columns; d unsorted
bool ql_record(int n, double* d, double* e, std::vector<Sweep>& sweeps, std::vector<double>& cs, std::vector<double>& sn);
bool ql_values(int n, double* d, double* e);  // eigenvalues only (square-root free), d unsorted, e destroyed
// rows [k0, k0 + 8 nvec) of Z (leading dimension ldz, a multiple of 8) times every recorded rotation, in order
void apply_rotations_rows(int ldz, double* Z, int k0, int nvec, const Sweep* sweeps, size_t nsweeps, const double* cs,
                          const double* sn);
// eigenvectors (Z: n x k) of T for lam[0..k), DESCENDING and accurate to rounding; false: a vector did not converge
bool tridiag_inverse_iteration(int n, const double* d, const double* e, const double* lam, int k, double* Z, const EigOpts& o);

// bisection on Sturm counts; t.d points into the caller's diagonal, which must outlive t
struct SturmT {
    int n;
    const double* d;
    std::vector<double> e2;  // e2[i] = e[i]^2 couples i - 1 and i (e2[0] = 0)
    double pivmin, lo, hi;   // Gershgorin bounds, widened
};
SturmT sturm_setup(int n, const double* d, const double* e);
int sturm_count1(const SturmT& t, double s);  // the number of eigenvalues smaller than s
// the eigenvalues number k[0 .. m) of T counted from the SMALLEST (k = 0), m <= 64
void sturm_bisect(const SturmT& t, const int* k, int m, double* out);
// eigenvalues with DESCENDING numbers [first, first + count) (number 0 = the largest) into out[0 .. count)
void sturm_eigenvalues_desc(const SturmT& t, int first, int count, double* out);

}  // namespace nleh
