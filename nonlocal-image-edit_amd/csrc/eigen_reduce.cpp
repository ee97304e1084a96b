// Host fp64 eigensolver, the dense side: the two Householder reductions to tridiagonal form (the classic row-oriented one
// that accumulates the orthogonal factor, and the column-oriented one that keeps the reflectors) and the
// back-transformation of eigenvectors through the kept reflectors.  Column-major, every inner loop unit stride.
#include "eigen_stages.h"

#include <algorithm>
#include <cmath>

namespace nleh {

// V: n x n col-major, in: symmetric matrix (lower triangle valid, mirrored by caller);
// out: orthogonal Q with Q^T A Q tridiagonal (d diag, e[1..n-1] sub-diagonal).  The EISPACK tred2 recurrence.
NLE_SIMD_CLONES void tridiagonalize(int n, double* V, double* d, double* e) {
    for (int j = 0; j < n; ++j) d[j] = at(V, n, n - 1, j);
    for (int i = n - 1; i > 0; --i) {
        double scale = 0.0, h = 0.0;
        for (int k = 0; k < i; ++k) scale += std::fabs(d[k]);
        if (scale == 0.0) {
            e[i] = d[i - 1];
            for (int j = 0; j < i; ++j) {
                d[j] = at(V, n, i - 1, j);
                at(V, n, i, j) = 0.0;
                at(V, n, j, i) = 0.0;
            }
        } else {
            for (int k = 0; k < i; ++k) {
                d[k] /= scale;
                h += d[k] * d[k];
            }
            double f = d[i - 1];
            double g = std::sqrt(h);
            if (f > 0) g = -g;
            e[i] = scale * g;
            h -= f * g;
            d[i - 1] = f - g;
            for (int j = 0; j < i; ++j) e[j] = 0.0;
            for (int j = 0; j < i; ++j) {
                f = d[j];
                at(V, n, j, i) = f;
                g = e[j] + at(V, n, j, j) * f;
                const double* col = &at(V, n, 0, j);
                double gs = 0.0;
#pragma omp simd reduction(+ : gs)
                for (int k = j + 1; k <= i - 1; ++k) {
                    gs += col[k] * d[k];
                    e[k] += col[k] * f;
                }
                e[j] = g + gs;
            }
            f = 0.0;
            for (int j = 0; j < i; ++j) {
                e[j] /= h;
                f += e[j] * d[j];
            }
            const double hh = f / (h + h);
            for (int j = 0; j < i; ++j) e[j] -= hh * d[j];
            for (int j = 0; j < i; ++j) {
                f = d[j];
                g = e[j];
                double* col = &at(V, n, 0, j);
#pragma omp simd
                for (int k = j; k <= i - 1; ++k) col[k] -= (f * e[k] + g * d[k]);
                d[j] = at(V, n, i - 1, j);
                at(V, n, i, j) = 0.0;
            }
        }
        d[i] = h;
    }
    // accumulate transformations
    for (int i = 0; i < n - 1; ++i) {
        at(V, n, n - 1, i) = at(V, n, i, i);
        at(V, n, i, i) = 1.0;
        const double h = d[i + 1];
        if (h != 0.0) {
            const double* ci1 = &at(V, n, 0, i + 1);
            for (int k = 0; k <= i; ++k) d[k] = ci1[k] / h;
            for (int j = 0; j <= i; ++j) {
                double* cj = &at(V, n, 0, j);
                double g = 0.0;
#pragma omp simd reduction(+ : g)
                for (int k = 0; k <= i; ++k) g += ci1[k] * cj[k];
#pragma omp simd
                for (int k = 0; k <= i; ++k) cj[k] -= g * d[k];
            }
        }
        for (int k = 0; k <= i; ++k) at(V, n, k, i + 1) = 0.0;
    }
    for (int j = 0; j < n; ++j) {
        d[j] = at(V, n, n - 1, j);
        at(V, n, n - 1, j) = 0.0;
    }
    at(V, n, n - 1, n - 1) = 1.0;
    e[0] = 0.0;
}

// Householder reduction on the UPPER triangle, column-major, eight columns per sweep.  Step i annihilates column i above the
// sub-diagonal entry: the vector x = A(0..i-1, i), the columns' active parts A(0..j, j) and the stored reflector u_i (column
// i, rows < i) are all CONTIGUOUS -- the row-oriented classic (tred2) gathers and scatters a strided row every step.  The two
// O(i^2) loops of a step, p = A u and A -= u q^T + q u^T, take eight columns at a time over full vectors of eight rows; where
// a block of columns crosses the diagonal the 8 x 8 triangle is one more vector per column under a 0/1 mask, and the
// work vectors are zero beyond i: no scalar remainder loops anywhere (they, the strided copies and the scalar O(i) loops
// were two thirds of the four-column form's 0.33 ms at n = 200).  Reads the whole of V (both triangles mirrored by the
// caller); on return column i, rows < i, holds u_i with H_i = I - u_i u_i^T / hs[i], d and e the tridiagonal matrix
// (e[i] couples i - 1 and i): the layout back_transform_cols and the tridiagonal routines take.
NLE_SIMD_CLONES static void tridiag_reduce_impl(int n, double* V, double* d, double* e, double* hs, const double (*kLe)[8], const double (*kLt)[8]) {
    // The rank-2 update of step i+1 and the product A u of step i are ONE sweep over the block: an entry is loaded, updated,
    // stored and multiplied while it is in a register (the two-sweep form loaded it twice; same operations on the same operands
    // in the same order, bit for bit the same T).  Column i itself is brought up to date first (O(i)): its reflector must be
    // known before the sweep starts.
    std::vector<double> work((size_t)4 * (n + 16), 0.0);
    double* u = work.data();       // the pending update's vectors (step i+1), zero from i+1 on; zero at the start
    double* q = u + (n + 16);
    double* un = q + (n + 16);     // this step's reflector and product
    double* qn = un + (n + 16);
    for (int i = n - 1; i >= 0; --i) {
        double* x = V + (size_t)i * n;
        const int i8 = (i + 7) & ~7;
        if (i < n - 1) {  // column i and its diagonal entry after the pending update (u, q are zero beyond row i: the rows below
                          // the diagonal, and the entries of the next column a last vector reaches, are rewritten unchanged)
            const double ui = u[i], qi = q[i];
            for (int k = 0; k <= i; k += 8) st8(x + k, ld8(x + k) - (ld8(u + k) * qi + ld8(q + k) * ui));
        }
        if (i == 0) break;
        double scale = 0.0, h = 0.0;
#pragma omp simd reduction(+ : scale)
        for (int k = 0; k < i; ++k) scale += std::fabs(x[k]);
        for (int k = 0; k < i8 + 8; ++k) un[k] = 0.0;
        for (int k = 0; k < i8 + 8; ++k) qn[k] = 0.0;
        if (scale == 0.0) {
            e[i] = x[i - 1];
            for (int k = 0; k < i; ++k) x[k] = 0.0;
        } else {
            const double rscale = 1.0 / scale;
#pragma omp simd reduction(+ : h)
            for (int k = 0; k < i; ++k) {
                const double t = x[k] * rscale;
                un[k] = t;
                h += t * t;
            }
            const double f0 = un[i - 1];
            double g = std::sqrt(h);
            if (f0 > 0) g = -g;
            e[i] = scale * g;
            h -= f0 * g;
            un[i - 1] = f0 - g;
#pragma omp simd
            for (int k = 0; k < i; ++k) x[k] = un[k];
        }
        // the block's upper triangle: A -= u q^T + q u^T (pending), then qn = A un on what was just stored
        for (int j0 = 0; j0 < i; j0 += 8) {
            const int nc = std::min(8, i - j0);
            double* col[8];
            double uj[8], qj[8], unj[8];
            for (int c = 0; c < 8; ++c) {
                col[c] = V + (size_t)(j0 + (c < nc ? c : 0)) * n;
                uj[c] = c < nc ? u[j0 + c] : 0.0;
                qj[c] = c < nc ? q[j0 + c] : 0.0;
                unj[c] = c < nc ? un[j0 + c] : 0.0;
            }
            v8d acc[8];
            for (int c = 0; c < 8; ++c) acc[c] = v8d{0, 0, 0, 0, 0, 0, 0, 0};
            for (int k = 0; k < j0; k += 8) {
                const v8d uv = ld8(u + k), qv = ld8(q + k), nv = ld8(un + k);
                v8d pv = ld8(qn + k);
                for (int c = 0; c < 8; ++c) {
                    const v8d cv = ld8(col[c] + k) - (uv * qj[c] + qv * uj[c]);
                    if (c < nc) st8(col[c] + k, cv);
                    acc[c] += cv * nv;
                    pv += cv * unj[c];
                }
                st8(qn + k, pv);
            }
            {
                const v8d uv = ld8(u + j0), qv = ld8(q + j0), nv = ld8(un + j0);
                v8d pv = ld8(qn + j0);
                for (int c = 0; c < 8; ++c) {
                    const v8d cv = ld8(col[c] + j0) - ld8(kLe[c]) * (uv * qj[c] + qv * uj[c]);
                    if (c < nc) st8(col[c] + j0, cv);
                    acc[c] += (cv * ld8(kLe[c])) * nv;
                    pv += (cv * ld8(kLt[c])) * unj[c];
                }
                st8(qn + j0, pv);
            }
            for (int c = 0; c < nc; ++c) qn[j0 + c] += hsum8(acc[c]);
        }
        if (scale != 0.0) {
            const double rh = 1.0 / h;
            double f = 0.0;
#pragma omp simd reduction(+ : f)
            for (int k = 0; k < i; ++k) {
                qn[k] *= rh;
                f += qn[k] * un[k];
            }
            const double hh = f / (h + h);
#pragma omp simd
            for (int k = 0; k < i; ++k) qn[k] -= hh * un[k];
            for (int k = i; k < i8 + 8; ++k) qn[k] = 0.0;
        } else {
            for (int k = 0; k < i8 + 8; ++k) qn[k] = 0.0;  // no reflector: nothing pending for the next step
        }
        hs[i] = h;
        std::swap(u, un);
        std::swap(q, qn);
    }
    hs[0] = 0.0;
    for (int j = 0; j < n; ++j) d[j] = at(V, n, j, j);  // the diagonal of T
    e[0] = 0.0;
}

void tridiag_reduce(int n, double* V, double* d, double* e, double* hs) {
    static const double kLe[8][8] = {{1, 0, 0, 0, 0, 0, 0, 0}, {1, 1, 0, 0, 0, 0, 0, 0}, {1, 1, 1, 0, 0, 0, 0, 0}, {1, 1, 1, 1, 0, 0, 0, 0},
                                     {1, 1, 1, 1, 1, 0, 0, 0}, {1, 1, 1, 1, 1, 1, 0, 0}, {1, 1, 1, 1, 1, 1, 1, 0}, {1, 1, 1, 1, 1, 1, 1, 1}};
    static const double kLt[8][8] = {{0, 0, 0, 0, 0, 0, 0, 0}, {1, 0, 0, 0, 0, 0, 0, 0}, {1, 1, 0, 0, 0, 0, 0, 0}, {1, 1, 1, 0, 0, 0, 0, 0},
                                     {1, 1, 1, 1, 0, 0, 0, 0}, {1, 1, 1, 1, 1, 0, 0, 0}, {1, 1, 1, 1, 1, 1, 0, 0}, {1, 1, 1, 1, 1, 1, 1, 0}};
    if (n < 16) {  // the sweeps read (and rewrite unchanged) up to seven entries past a column's end: give a tiny matrix room
        std::vector<double> Vp((size_t)n * n + 16, 0.0);
        std::copy(V, V + (size_t)n * n, Vp.begin());
        tridiag_reduce_impl(n, Vp.data(), d, e, hs, kLe, kLt);
        std::copy(Vp.begin(), Vp.begin() + (size_t)n * n, V);
        return;
    }
    tridiag_reduce_impl(n, V, d, e, hs, kLe, kLt);
}

// M's lower triangle mirrored into V (n x n; SelfAdjointEigenSolver reads only the lower one)
void mirror_lower(const double* M, int n, double* V) {
    for (int c = 0; c < n; ++c)
        for (int r = 0; r < n; ++r) V[(size_t)c * n + r] = (r >= c) ? M[(size_t)c * n + r] : M[(size_t)r * n + c];
}

Reduced reduce_lower(const double* M, int n) {
    Reduced t{std::vector<double>((size_t)n * n), std::vector<double>(n), std::vector<double>(n), std::vector<double>(n)};
    mirror_lower(M, n, t.V.data());
    tridiag_reduce(n, t.V.data(), t.d.data(), t.e.data(), t.hs.data());
    return t;
}

// Y (n x ncols, column-major, ld n) <- Q Y with Q = P_{n-1} ... P_1, P_i = I - u_i u_i^T / h_i on rows 0..i-1
// (u_i = column i of V, rows 0..i-1): the product `tridiagonalize` accumulates, applied to a few columns.
// Eight columns share every load of a reflector (their eight dot products are independent chains; vector by vector the
// loop waited on one horizontal sum and one division per reflector and column): 0.20 -> 0.0x ms for 50 vectors at n = 200.
template <int NB>
static inline __attribute__((always_inline)) void back_transform_block(int n, const double* V, const double* hs, double* Y0, int nb) {
    double* y[NB];
    for (int jj = 0; jj < NB; ++jj) y[jj] = Y0 + (size_t)(jj < nb ? jj : nb - 1) * n;  // (columns >= nb: recomputed, not stored)
    for (int i = 1; i < n; ++i) {
        const double h = hs[i];
        if (h == 0.0) continue;
        const double* u = V + (size_t)i * n;
        const int i8 = i & ~7;
        v8d acc[NB];
        for (int jj = 0; jj < NB; ++jj) acc[jj] = v8d{0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < i8; k += 8) {
            const v8d uv = ld8(u + k);
            for (int jj = 0; jj < NB; ++jj) acc[jj] += uv * ld8(y[jj] + k);
        }
        double g[NB];
        for (int jj = 0; jj < NB; ++jj) g[jj] = hsum8(acc[jj]);
        for (int k = i8; k < i; ++k)
            for (int jj = 0; jj < NB; ++jj) g[jj] += u[k] * y[jj][k];
        const double rh = 1.0 / h;
        for (int jj = 0; jj < NB; ++jj) g[jj] *= rh;
        for (int k = 0; k < i8; k += 8) {
            const v8d uv = ld8(u + k);
            for (int jj = 0; jj < NB; ++jj)
                if (jj < nb) st8(y[jj] + k, ld8(y[jj] + k) - g[jj] * uv);
        }
        for (int k = i8; k < i; ++k)
            for (int jj = 0; jj < nb; ++jj) y[jj][k] -= g[jj] * u[k];
    }
}
NLE_SIMD_CLONES void back_transform_cols(int n, const double* V, const double* hs, double* Y, int j0, int j1) {
    constexpr int CB = 8;
    for (int jb = j0; jb < j1; jb += CB) back_transform_block<CB>(n, V, hs, Y + (size_t)jb * n, std::min(CB, j1 - jb));
}

}  // namespace nleh
