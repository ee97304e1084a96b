// Host fp64 eigensolver, everything that works on the tridiagonal form (d, e): the three QL iterations, the blocked
// application of recorded rotations, bisection on Sturm counts, and inverse iteration (scalar, eight lanes at once, and
// the Cholesky-QR form for large clusters).  Where AVX-512 is used it is asked for at run time; no -march.
#include "eigen_stages.h"
#include "host_dense.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace nleh {

// Implicit-shift QL on (d, e) (tql2), written once for its two uses: ACCUMULATE applies every plane rotation to V's
// columns at once (ql_implicit), otherwise the rotations of each sweep are recorded for later (ql_record).  The
// iteration itself, and so d, is the same either way.  false: an eigenvalue needs more than 60 sweeps.
template <bool ACCUMULATE>
static inline __attribute__((always_inline)) bool tql2(int n, double* V, double* d, double* e, std::vector<Sweep>* sweeps,
                                                       std::vector<double>* cs, std::vector<double>* sn) {
    for (int i = 1; i < n; ++i) e[i - 1] = e[i];
    e[n - 1] = 0.0;
    double f = 0.0, tst1 = 0.0;
    const double eps = std::ldexp(1.0, -52);
    for (int l = 0; l < n; ++l) {
        tst1 = std::max(tst1, std::fabs(d[l]) + std::fabs(e[l]));
        int m = l;
        while (m < n) {
            if (std::fabs(e[m]) <= eps * tst1) break;
            ++m;
        }
        if (m > l) {
            int iter = 0;
            do {
                if (++iter > 60) return false;
                double g = d[l];
                double p = (d[l + 1] - g) / (2.0 * e[l]);
                double r = hyp(p, 1.0);
                if (p < 0) r = -r;
                d[l] = e[l] / (p + r);
                d[l + 1] = e[l] * (p + r);
                const double dl1 = d[l + 1];
                double h = g - d[l];
                for (int i = l + 2; i < n; ++i) d[i] -= h;
                f += h;
                p = d[m];
                double c = 1.0, c2 = c, c3 = c;
                const double el1 = e[l + 1];
                double s = 0.0, s2 = 0.0;
                if (!ACCUMULATE) sweeps->push_back(Sweep{l, m, cs->size()});
                for (int i = m - 1; i >= l; --i) {
                    c3 = c2;
                    c2 = c;
                    s2 = s;
                    g = c * e[i];
                    h = c * p;
                    r = hyp(p, e[i]);
                    e[i + 1] = s * r;
                    s = e[i] / r;
                    c = p / r;
                    p = c * d[i] - s * g;
                    d[i + 1] = h + s * (c * g + s * d[i]);
                    if (ACCUMULATE) {
                        double* vi = &at(V, n, 0, i);
                        double* vi1 = &at(V, n, 0, i + 1);
#pragma omp simd
                        for (int k = 0; k < n; ++k) {
                            const double hk = vi1[k];
                            vi1[k] = s * vi[k] + c * hk;
                            vi[k] = c * vi[k] - s * hk;
                        }
                    } else {
                        cs->push_back(c);
                        sn->push_back(s);
                    }
                }
                p = -s * s2 * c3 * el1 * e[l] / dl1;
                e[l] = s * p;
                d[l] = c * p;
            } while (std::fabs(e[l]) > eps * tst1);
        }
        d[l] += f;
        e[l] = 0.0;
    }
    return true;
}

// implicit QL on (d, e) accumulating rotations into V's columns
NLE_SIMD_CLONES bool ql_implicit(int n, double* V, double* d, double* e) { return tql2<true>(n, V, d, e, nullptr, nullptr, nullptr); }

// the same iteration recording the rotations of every sweep (phase 2 of eigen_stages.h)
bool ql_record(int n, double* d, double* e, std::vector<Sweep>& sweeps, std::vector<double>& cs, std::vector<double>& sn) {
    return tql2<false>(n, nullptr, d, e, &sweeps, &cs, &sn);
}

// Eigenvalues only, by the square-root-free QL variant of Pal, Walker and Kahan as LAPACK's dsterf organises it (implicit
// Wilkinson shift; deflation where e_m^2 <= eps^2 |d_m d_{m+1}|; 2 x 2 blocks in closed form, dlae2): one reciprocal
// and a handful of multiplications per rotation instead of tql2's two hypot calls -- 0.22 -> ~0.1 ms at n = 196.
// d: diagonal, e[1..n): sub-diagonal (e[i] couples i-1 and i) on entry; d holds the eigenvalues (unsorted) on return.
bool ql_values(int n, double* d, double* e2) {
    if (n <= 1) return true;
    const double eps = std::ldexp(1.0, -53), eps2 = eps * eps, safmin = 2.2250738585072014e-308;
    double anorm = 0.0;
    for (int i = 0; i < n; ++i) anorm = std::max(anorm, std::fabs(d[i]) + (i + 1 < n ? std::fabs(e2[i + 1]) : 0.0) + std::fabs(e2[i]));
    if (anorm == 0.0) return true;
    // scale to norm 1 (squares of tiny off-diagonals must not underflow), e2[i] := (e[i+1] / anorm)^2 couples i and i+1
    const double scl = 1.0 / anorm;
    for (int i = 0; i < n; ++i) d[i] *= scl;
    for (int i = 0; i + 1 < n; ++i) {
        const double t = e2[i + 1] * scl;
        e2[i] = t * t;
    }
    e2[n - 1] = 0.0;
    int iter_left = 60 * n;
    for (int l = 0; l < n; ++l) {
        for (;;) {
            int m = l;
            while (m + 1 < n) {
                if (e2[m] <= eps2 * std::fabs(d[m] * d[m + 1]) + safmin) break;
                ++m;
            }
            if (m + 1 < n) e2[m] = 0.0;  // the block [l, m] is decoupled from the rest
            if (m == l) break;           // d[l] is an eigenvalue
            if (m == l + 1) {   // 2 x 2 block [[a, b], [b, c]]: dlae2
                const double a = d[l], c = d[l + 1], b = std::sqrt(e2[l]);
                const double sm = a + c, df = a - c, adf = std::fabs(df), tb = b + b, ab = std::fabs(tb);
                const double acmx = std::fabs(a) > std::fabs(c) ? a : c, acmn = std::fabs(a) > std::fabs(c) ? c : a;
                double rt;
                if (adf > ab) rt = adf * std::sqrt(1.0 + (ab / adf) * (ab / adf));
                else if (adf < ab) rt = ab * std::sqrt(1.0 + (adf / ab) * (adf / ab));
                else rt = ab * std::sqrt(2.0);
                double rt1, rt2;
                if (sm < 0.0) {
                    rt1 = 0.5 * (sm - rt);
                    rt2 = (acmx / rt1) * acmn - (b / rt1) * b;
                } else if (sm > 0.0) {
                    rt1 = 0.5 * (sm + rt);
                    rt2 = (acmx / rt1) * acmn - (b / rt1) * b;
                } else {
                    rt1 = 0.5 * rt;
                    rt2 = -0.5 * rt;
                }
                d[l] = rt1;
                d[l + 1] = rt2;
                e2[l] = 0.0;
                ++l;  // both are done
                break;
            }
            if (--iter_left < 0) return false;
            // Wilkinson shift from the leading 2 x 2 block of [l, m]
            const double rte = std::sqrt(e2[l]);
            const double p0 = d[l];
            double sigma = (d[l + 1] - p0) / (2.0 * rte);
            const double r0 = hyp(sigma, 1.0);
            sigma = p0 - rte / (sigma + (sigma >= 0.0 ? r0 : -r0));
            double c = 1.0, sn = 0.0, gamma = d[m] - sigma, p = gamma * gamma;
            for (int i = m - 1; i >= l; --i) {
                const double bb = e2[i], r = p + bb;
                if (i != m - 1) e2[i + 1] = sn * r;
                const double oldc = c, rinv = 1.0 / r;
                c = p * rinv;
                sn = bb * rinv;
                const double oldgam = gamma, alpha = d[i];
                gamma = c * (alpha - sigma) - sn * oldgam;
                d[i + 1] = oldgam + (alpha - gamma);
                p = (c != 0.0) ? (gamma * gamma) / c : oldc * bb;
            }
            e2[l] = sn * p;
            d[l] = sigma + gamma;
        }
    }
    for (int i = 0; i < n; ++i) d[i] *= anorm;
    return true;
}

// Rows [k0, k0 + 8 NV) of Z (column-major, leading dimension ldz, a multiple of 8): every sweep's rotations,
// in order.  Consecutive rotations share a column; its running value stays in NV vector registers, so each
// column is loaded and stored once per sweep, and NV independent dependency chains hide the FMA latency.

template <int NV>
static inline __attribute__((always_inline)) void rotate_rows(int ldz, double* Z, int k0, const Sweep* sweeps,
                                                              size_t nsweeps, const double* cs, const double* sn) {
    for (size_t q = 0; q < nsweeps; ++q) {
        const Sweep sw = sweeps[q];
        const double* c = cs + sw.first;
        const double* s = sn + sw.first;
        v8d carry[NV];
        const double* top = Z + (size_t)sw.m * ldz + k0;
#pragma GCC unroll 8
        for (int v = 0; v < NV; ++v) carry[v] = ld8(top + 8 * v);
        for (int i = sw.m - 1, t = 0; i >= sw.l; --i, ++t) {
            const double ci = c[t], si = s[t];
            double* vi = Z + (size_t)i * ldz + k0;
            double* vi1 = vi + ldz;
#pragma GCC unroll 8
            for (int v = 0; v < NV; ++v) {
                const v8d hk = carry[v], vk = ld8(vi + 8 * v);
                st8(vi1 + 8 * v, si * vk + ci * hk);
                carry[v] = ci * vk - si * hk;
            }
        }
        double* bot = Z + (size_t)sw.l * ldz + k0;
#pragma GCC unroll 8
        for (int v = 0; v < NV; ++v) st8(bot + 8 * v, carry[v]);
    }
}

// Z starts as the identity, so entries far from the diagonal are products of many sines and pass through the
// denormal range on their way to zero; denormal operands cost ~100 cycles each on x86.  They are flushed
// to zero for the duration of the phase (a change below 1e-307 in an orthogonal matrix).
struct FlushDenormals {
#if defined(__x86_64__)
    unsigned saved = _mm_getcsr();
    FlushDenormals() { _mm_setcsr(saved | 0x8040); }  // FTZ | DAZ
    ~FlushDenormals() { _mm_setcsr(saved); }
#endif
};

NLE_SIMD_CLONES void apply_rotations_rows(int ldz, double* Z, int k0, int nvec, const Sweep* sweeps, size_t nsweeps,
                                          const double* cs, const double* sn) {
    FlushDenormals ftz;
    while (nvec > 0) {  // 8, 4, 2, 1 vectors of 8 rows
        if (nvec >= 8) {
            rotate_rows<8>(ldz, Z, k0, sweeps, nsweeps, cs, sn);
            nvec -= 8, k0 += 64;
        } else if (nvec >= 4) {
            rotate_rows<4>(ldz, Z, k0, sweeps, nsweeps, cs, sn);
            nvec -= 4, k0 += 32;
        } else if (nvec >= 2) {
            rotate_rows<2>(ldz, Z, k0, sweeps, nsweeps, cs, sn);
            nvec -= 2, k0 += 16;
        } else {
            rotate_rows<1>(ldz, Z, k0, sweeps, nsweeps, cs, sn);
            nvec -= 1, k0 += 8;
        }
    }
}

// x <- x minus its components along the m orthonormal vectors z_0 .. z_{m-1} (stride n), two passes.  Four vectors at a
// time: their four dot products in ONE sweep over x (independent accumulators), their combined update in one more -- half the
// sweeps of vector-by-vector modified Gram-Schmidt and vectorisable; inside a block the projection is classical, across
// blocks sequential, and the second pass makes either form orthogonal to rounding ("twice is enough").  With the ~100
// eigenvalues the 1e-10 cut drops from a 900 x 900 Wa in ONE cluster this loop was 10 of the 10.8 ms of inverse iteration.
NLE_SIMD_CLONES static void orth_against_cluster(int n, const double* Zc, int m, double* x) {
    for (int pass = 0; pass < 2; ++pass) {
        int q = 0;
        for (; q + 4 <= m; q += 4) {
            const double *z0 = Zc + (size_t)q * n, *z1 = z0 + n, *z2 = z1 + n, *z3 = z2 + n;
            double h0 = 0.0, h1 = 0.0, h2 = 0.0, h3 = 0.0;
#pragma omp simd reduction(+ : h0, h1, h2, h3)
            for (int i = 0; i < n; ++i) {
                const double xi = x[i];
                h0 += z0[i] * xi;
                h1 += z1[i] * xi;
                h2 += z2[i] * xi;
                h3 += z3[i] * xi;
            }
#pragma omp simd
            for (int i = 0; i < n; ++i) x[i] -= (h0 * z0[i] + h1 * z1[i]) + (h2 * z2[i] + h3 * z3[i]);
        }
        for (; q < m; ++q) {
            const double* zq = Zc + (size_t)q * n;
            double h = 0.0;
#pragma omp simd reduction(+ : h)
            for (int i = 0; i < n; ++i) h += zq[i] * x[i];
#pragma omp simd
            for (int i = 0; i < n; ++i) x[i] -= h * zq[i];
        }
    }
}

// Inverse iteration (the scheme of tridiag_inverse_iteration below, operation for operation) for EIGHT isolated eigenvalues
// at once, one per AVX-512 lane: the LU factorisation with partial pivoting and the two substitutions are chains of n
// dependent steps, so eight shifts cost what one does.  Pivot choices differ per lane: both branches are formed and
// blended.  Same operations in the same order as the scalar code (whose compiler may contract or reorder a sum or two: the
// vectors agree to a few ulp, tools/micro/bisect_check.py).  lam8: the shifts (m <= 8 used, the rest repeat the last), idx8: their vector numbers (seeds), Zcols: where the
// vectors go.  false: a lane did not converge (the caller falls back exactly as for the scalar path).
#if defined(__x86_64__)
__attribute__((target("avx512f"))) static inline __m512d x8_fix_tiny(__m512d v, __m512d vtiny) {  // |v| < tiny: copysign(tiny, v == 0 ? 1 : v)
    const __m512d zero = _mm512_setzero_pd();
    const __m512i signbit = _mm512_set1_epi64((long long)0x8000000000000000ull);
    const __mmask8 small = _mm512_cmp_pd_mask(_mm512_abs_pd(v), vtiny, _CMP_LT_OQ);
    const __mmask8 iszero = _mm512_cmp_pd_mask(v, zero, _CMP_EQ_OQ);
    __m512i sg = _mm512_and_epi64(_mm512_castpd_si512(v), signbit);
    sg = _mm512_mask_mov_epi64(sg, iszero, _mm512_setzero_si512());
    const __m512d t = _mm512_castsi512_pd(_mm512_or_epi64(_mm512_castpd_si512(vtiny), sg));
    return _mm512_mask_mov_pd(v, small, t);
}
struct X8Arr {  // n vectors of eight doubles in 64-byte aligned storage (std::vector<__m512d> drops the alignment)
    double* p;
    __attribute__((target("avx512f"))) inline __m512d operator()(int i) const { return _mm512_load_pd(p + (size_t)8 * i); }
    __attribute__((target("avx512f"))) inline void set(int i, __m512d v) const { _mm512_store_pd(p + (size_t)8 * i, v); }
};
__attribute__((target("avx512f"))) static bool inverse_iteration_x8(int n, const double* d, const double* e, const double* lam8,
                                                                   const int* idx8, int m, double onenrm, double* const* Zcols) {
    const double eps = std::ldexp(1.0, -52), tiny = eps * onenrm;
    std::vector<double> store((size_t)7 * n * 8 + 8);
    double* base = store.data();
    while (reinterpret_cast<uintptr_t>(base) & 63) ++base;
    X8Arr a{base}, ra{base + (size_t)8 * n}, b{base + (size_t)16 * n}, c{base + (size_t)24 * n}, dd{base + (size_t)32 * n},
        x{base + (size_t)40 * n}, y{base + (size_t)48 * n};
    std::vector<__mmask8> piv(n);
    const __m512d vtiny = _mm512_set1_pd(tiny), zero = _mm512_setzero_pd();
    double lamv[8];
    for (int l = 0; l < 8; ++l) lamv[l] = lam8[l < m ? l : m - 1];
    const __m512d xj = _mm512_loadu_pd(lamv);
    for (int i = 0; i < n; ++i) {
        a.set(i, _mm512_sub_pd(_mm512_set1_pd(d[i]), xj));
        {
            const __m512d ev = _mm512_set1_pd(i + 1 < n ? e[i + 1] : 0.0);
            b.set(i, ev);
            c.set(i, ev);
        }
        dd.set(i, zero);
    }
    for (int i = 0; i + 1 < n; ++i) {
        const __m512d ai = a(i), ci = c(i), an = a(i + 1), bi = b(i);
        const __mmask8 ge = _mm512_cmp_pd_mask(_mm512_abs_pd(ai), _mm512_abs_pd(ci), _CMP_GE_OQ);
        const __m512d af = x8_fix_tiny(ai, vtiny);
        const __m512d num = _mm512_mask_blend_pd(ge, ai, ci), den = _mm512_mask_blend_pd(ge, ci, af);
        const __m512d mult = _mm512_div_pd(num, den);
        const __m512d X = _mm512_mask_blend_pd(ge, bi, an), Yv = _mm512_mask_blend_pd(ge, an, bi);
        a.set(i + 1, _mm512_sub_pd(X, _mm512_mul_pd(mult, Yv)));
        a.set(i, _mm512_mask_blend_pd(ge, ci, af));
        if (i + 2 < n) {
            const __m512d bn = b(i + 1);
            dd.set(i, _mm512_mask_blend_pd(ge, bn, zero));
            b.set(i + 1, _mm512_mask_blend_pd(ge, _mm512_mul_pd(_mm512_sub_pd(zero, mult), bn), bn));
        }
        b.set(i, _mm512_mask_blend_pd(ge, an, bi));
        c.set(i, mult);
        piv[i] = (__mmask8)~ge;
    }
    a.set(n - 1, x8_fix_tiny(a(n - 1), vtiny));
    const __m512d one = _mm512_set1_pd(1.0);
    for (int i = 0; i < n; ++i) ra.set(i, _mm512_div_pd(one, a(i)));
    {
        unsigned long long seed[8];
        for (int l = 0; l < 8; ++l) seed[l] = 0x2545F4914F6CDD1Dull ^ (0x9E3779B97F4A7C15ull * (unsigned long long)(idx8[l < m ? l : m - 1] + 1));
        double xs[8];
        for (int i = 0; i < n; ++i) {
            for (int l = 0; l < 8; ++l) {
                seed[l] ^= seed[l] << 13, seed[l] ^= seed[l] >> 7, seed[l] ^= seed[l] << 17;
                xs[l] = (double)(seed[l] >> 11) * (1.0 / 9007199254740992.0) - 0.5;
            }
            x.set(i, _mm512_loadu_pd(xs));
        }
    }
    const __m512d veps = _mm512_set1_pd(eps), vfloor = _mm512_set1_pd(1e-300), vn = _mm512_set1_pd((double)n * onenrm);
    const __m512d an1 = _mm512_max_pd(veps, _mm512_abs_pd(a(n - 1)));
    __mmask8 done = 0;
    const __mmask8 want = (__mmask8)((1u << m) - 1u);
    for (int it = 0; it < 8 && (done & want) != want; ++it) {
        __m512d s1 = zero;
        for (int i = 0; i < n; ++i) s1 = _mm512_add_pd(s1, _mm512_abs_pd(x(i)));
        const __m512d scl = _mm512_div_pd(_mm512_mul_pd(vn, an1), _mm512_max_pd(s1, vfloor));
        __m512d yi = _mm512_mul_pd(x(0), scl);
        for (int i = 0; i + 1 < n; ++i) {  // forward: row interchanges and multipliers
            const __m512d yn = _mm512_mul_pd(x(i + 1), scl);
            const __m512d p0 = _mm512_mask_blend_pd(piv[i], yi, yn), p1 = _mm512_mask_blend_pd(piv[i], yn, yi);
            y.set(i, p0);
            yi = _mm512_sub_pd(p1, _mm512_mul_pd(c(i), p0));
        }
        y.set(n - 1, yi);
        for (int i = n - 1; i >= 0; --i) {  // back substitution with the three upper diagonals
            __m512d t = y(i);
            if (i + 1 < n) t = _mm512_sub_pd(t, _mm512_mul_pd(b(i), x(i + 1)));
            if (i + 2 < n) t = _mm512_sub_pd(t, _mm512_mul_pd(dd(i), x(i + 2)));
            x.set(i, _mm512_mul_pd(t, ra(i)));
        }
        __m512d nrm = zero;
        for (int i = 0; i < n; ++i) nrm = _mm512_add_pd(nrm, _mm512_mul_pd(x(i), x(i)));
        nrm = _mm512_sqrt_pd(nrm);
        {
            double nv[8];
            _mm512_storeu_pd(nv, nrm);
            for (int l = 0; l < m; ++l)
                if (!(nv[l] > 0.0) || !std::isfinite(nv[l])) return false;
        }
        for (int i = 0; i < n; ++i) x.set(i, _mm512_div_pd(x(i), nrm));
        if (it >= 1) {  // residual ||(T - lam I) x||_2 against the ORIGINAL eigenvalue
            __m512d res = zero;
            for (int i = 0; i < n; ++i) {
                __m512d t = _mm512_mul_pd(_mm512_sub_pd(_mm512_set1_pd(d[i]), xj), x(i));
                if (i > 0) t = _mm512_add_pd(t, _mm512_mul_pd(_mm512_set1_pd(e[i]), x(i - 1)));
                if (i + 1 < n) t = _mm512_add_pd(t, _mm512_mul_pd(_mm512_set1_pd(e[i + 1]), x(i + 1)));
                res = _mm512_add_pd(res, _mm512_mul_pd(t, t));
            }
            const __mmask8 ok = _mm512_cmp_pd_mask(_mm512_sqrt_pd(res), _mm512_set1_pd(1e3 * eps * onenrm), _CMP_LE_OQ);
            const __mmask8 fresh = (__mmask8)(ok & ~done & want);
            if (fresh) {
                double xs[8];
                for (int i = 0; i < n; ++i) {
                    _mm512_storeu_pd(xs, x(i));
                    for (int l = 0; l < m; ++l)
                        if (fresh & (1u << l)) Zcols[l][i] = xs[l];
                }
                done |= fresh;
            }
        }
    }
    return (done & want) == want;
}
#endif

// What the one-vector-at-a-time forms of inverse iteration share: the LU factorisation of T - xj I with partial pivoting
// (row i holds (a, b, dd), multipliers in c; tiny pivots perturbed), the iterate x started pseudo-randomly from the
// vector's number j (so the result does not depend on who computes it), one solve, the normalisation, the residual.
namespace {
struct InverseIteration {
    const int n;
    const double *d, *e, onenrm;
    const double eps = std::ldexp(1.0, -52), tiny = eps * onenrm;
    std::vector<double> a, ra, b, c, dd, x, y;
    std::vector<char> piv;
    InverseIteration(int n, const double* d, const double* e, double onenrm)
        : n(n), d(d), e(e), onenrm(onenrm), a(n), ra(n), b(n), c(n), dd(n), x(n), y(n), piv(n) {}
    void start(double xj, int j) {
        for (int i = 0; i < n; ++i) {
            a[i] = d[i] - xj;
            b[i] = (i + 1 < n) ? e[i + 1] : 0.0;
            c[i] = (i + 1 < n) ? e[i + 1] : 0.0;
            dd[i] = 0.0;
        }
        for (int i = 0; i + 1 < n; ++i) {
            if (std::fabs(a[i]) >= std::fabs(c[i])) {
                if (std::fabs(a[i]) < tiny) a[i] = std::copysign(tiny, a[i] == 0.0 ? 1.0 : a[i]);
                const double mult = c[i] / a[i];
                a[i + 1] -= mult * b[i];
                c[i] = mult;
                piv[i] = 0;
            } else {
                const double mult = a[i] / c[i];
                a[i] = c[i];
                const double t = a[i + 1];
                a[i + 1] = b[i] - mult * t;
                if (i + 2 < n) {
                    dd[i] = b[i + 1];
                    b[i + 1] = -mult * dd[i];
                }
                b[i] = t;
                c[i] = mult;
                piv[i] = 1;
            }
        }
        if (std::fabs(a[n - 1]) < tiny) a[n - 1] = std::copysign(tiny, a[n - 1] == 0.0 ? 1.0 : a[n - 1]);
        for (int i = 0; i < n; ++i) ra[i] = 1.0 / a[i];  // the back substitution is a dependent chain: multiply, not divide
        unsigned long long seed = 0x2545F4914F6CDD1Dull ^ (0x9E3779B97F4A7C15ull * (unsigned long long)(j + 1));
        for (int i = 0; i < n; ++i) {
            seed ^= seed << 13, seed ^= seed >> 7, seed ^= seed << 17;
            x[i] = (double)(seed >> 11) * (1.0 / 9007199254740992.0) - 0.5;
        }
    }
    void solve() {  // x <- (T - xj I)^-1 x up to scale
        // scale the right-hand side so that the solve cannot overflow (dstein: ||x||_1 = n ||T|| max(eps, |u_nn|))
        double s1 = 0.0;
        for (int i = 0; i < n; ++i) s1 += std::fabs(x[i]);
        const double scl = n * onenrm * std::max(eps, std::fabs(a[n - 1])) / std::max(s1, 1e-300);
        for (int i = 0; i < n; ++i) y[i] = x[i] * scl;
        for (int i = 0; i + 1 < n; ++i) {  // forward: apply the row interchanges and multipliers
            if (piv[i]) std::swap(y[i], y[i + 1]);
            y[i + 1] -= c[i] * y[i];
        }
        for (int i = n - 1; i >= 0; --i) {  // back substitution with the three upper diagonals
            double t = y[i];
            if (i + 1 < n) t -= b[i] * x[i + 1];
            if (i + 2 < n) t -= dd[i] * x[i + 2];
            x[i] = t * ra[i];
        }
    }
    bool normalise() {
        double nrm = 0.0;
        for (int i = 0; i < n; ++i) nrm += x[i] * x[i];
        nrm = std::sqrt(nrm);
        if (!(nrm > 0.0) || !std::isfinite(nrm)) return false;
        for (int i = 0; i < n; ++i) x[i] /= nrm;
        return true;
    }
};
// the residual ||(T - lam I) v||_2, against the ORIGINAL eigenvalue, is within 1e3 eps ||T||
bool converged(int n, const double* d, const double* e, double onenrm, const double* v, double lam) {
    double res = 0.0;
    for (int i = 0; i < n; ++i) {
        double t = (d[i] - lam) * v[i];
        if (i > 0) t += e[i] * v[i - 1];
        if (i + 1 < n) t += e[i + 1] * v[i + 1];
        res += t * t;
    }
    return std::sqrt(res) <= 1e3 * std::ldexp(1.0, -52) * onenrm;
}
}  // namespace

// Eigenvectors of the symmetric tridiagonal T (diagonal d[0..n), sub-diagonal e[1..n)) for k of its eigenvalues
// lam[0..k), given in DESCENDING order and accurate to rounding, by inverse iteration -- the scheme of LAPACK's dstein:
// LU of T - lam I with partial pivoting (tiny pivots perturbed), a few solves from a pseudo-random start, vectors of
// eigenvalues closer than 1e-3 ||T|| re-orthogonalised against each other (modified Gram-Schmidt, twice).  O(n k)
// instead of the O(n^2 k)-ish rotation sweeps: what sym_eigen_top uses when only the leading part of the spectrum is
// wanted (orthogonalize keeps K of q eigenvectors, src/filter.cpp:314).  Z: n x k column-major.  false: a vector did not
// reach a residual of 1e3 eps ||T|| (the caller falls back to the rotation form).
bool tridiag_inverse_iteration(int n, const double* d, const double* e, const double* lam, int k, double* Z, const EigOpts& o) {
    const double eps = std::ldexp(1.0, -52);
    double onenrm = 0.0;
    for (int i = 0; i < n; ++i)
        onenrm = std::max(onenrm, std::fabs(d[i]) + (i > 0 ? std::fabs(e[i]) : 0.0) + (i + 1 < n ? std::fabs(e[i + 1]) : 0.0));
    if (onenrm == 0.0) onenrm = 1.0;
    const double ortol = 1e-3 * onenrm, tiny = eps * onenrm;
    // Clusters (eigenvalues closer than ortol to their neighbour; their vectors are re-orthogonalised against each other)
    // are independent of one another: the shift perturbation below never reaches across a gap > ortol, and every vector
    // starts from its own pseudo-random vector (seeded by its index, so the result does not depend on who computes it).
    // With many vectors the clusters are dealt to a few threads.
    std::vector<int> starts;
    for (int j = 0; j < k; ++j)
        if (j == 0 || std::fabs(lam[j] - lam[j - 1]) > ortol) starts.push_back(j);
    starts.push_back(k);
    const int ngroups = (int)starts.size() - 1;
    // the shifts: the eigenvalues, kept distinct inside a cluster (descending order)
    std::vector<double> shift(lam, lam + k);
    for (int g = 0; g < ngroups; ++g)
        for (int j = starts[g] + 1; j < starts[g + 1]; ++j) {
            const double pertol = 10.0 * eps * std::max(std::fabs(shift[j]), tiny);
            if (shift[j - 1] - shift[j] < pertol) shift[j] = shift[j - 1] - pertol;
        }
    auto do_group = [&](int gp, int gend) -> bool {
        InverseIteration s(n, d, e, onenrm);
        for (int j = gp; j < gend; ++j) {
            s.start(shift[j], j);
            bool ok = false;
            for (int it = 0; it < 8 && !ok; ++it) {
                s.solve();
                orth_against_cluster(n, Z + (size_t)gp * n, j - gp, s.x.data());  // the cluster's earlier vectors, twice
                if (!s.normalise()) return false;
                if (it >= 1) ok = converged(n, d, e, onenrm, s.x.data(), lam[j]);
            }
            if (!ok) return false;
            std::copy(s.x.begin(), s.x.end(), Z + (size_t)j * n);
        }
        return true;
    };
    // A LARGE cluster (the ~100 eigenvalues the 1e-10 cut drops from a 900 x 900 Wa, all within ortol of each other) spends
    // its time in the vector-by-vector re-orthogonalisation, a chain nothing can be overlapped with.  Its eigenvalues are
    // known to ~eps ||T|| while they differ by far more, so plain inverse iteration (no orthogonalisation, every vector
    // independent of the others: threads) already isolates each vector to ~eps ||T|| / gap; ONE Cholesky-QR of the block
    // (two level-3 products) then makes it orthonormal to rounding, moving every vector by that same small amount inside
    // the cluster's invariant subspace.  Numerically repeated eigenvalues give (random, independent) vectors of their
    // eigenspace -- a worse conditioned block: then a second Cholesky-QR, and if the Gram matrix does not factor at all the
    // cluster goes through the sequential path.  Residuals are checked against the same bound as there.
    constexpr int kBlockMin = 24;
    auto do_group_block = [&](int gp, int gend) -> bool {
        const int mc = gend - gp;
        double* Zg = Z + (size_t)gp * n;
        const int nt = std::min(4, std::max(1, mc / 8));
        std::vector<char> okv(nt, 1);
        run_split(nt, nt, [&](int t) {
            InverseIteration s(n, d, e, onenrm);
            for (int jj = (int)((long long)mc * t / nt); jj < (int)((long long)mc * (t + 1) / nt); ++jj) {
                s.start(shift[gp + jj], gp + jj);
                for (int it = 0; it < 3; ++it) {
                    s.solve();
                    if (!s.normalise()) {
                        okv[t] = 0;
                        return;
                    }
                }
                std::copy(s.x.begin(), s.x.end(), Zg + (size_t)jj * n);
            }
        });
        if (std::count(okv.begin(), okv.end(), 0)) return false;
        // Cholesky-QR: G = Z^T Z = L L^T, Z <- Z L^-T; again if the block was far from orthonormal
        std::vector<double> Zt((size_t)mc * n), G((size_t)mc * mc), Li((size_t)mc * mc), Zn((size_t)n * mc);
        for (int pass = 0; pass < 2; ++pass) {
            for (int j = 0; j < mc; ++j)
                for (int i = 0; i < n; ++i) Zt[(size_t)i * mc + j] = Zg[(size_t)j * n + i];
            gemm_nn_cols(Zt.data(), Zg, G.data(), mc, n, mc, 0, mc);  // (mc x n) (n x mc)
            double off = 0.0;
            for (int j = 0; j < mc; ++j)
                for (int i = 0; i < mc; ++i)
                    if (i != j) off = std::max(off, std::fabs(G[(size_t)j * mc + i]));
            if (pass == 1 && off < 1e-13) break;  // already orthonormal to rounding
            for (int j = 0; j < mc; ++j)
                for (int i = 0; i < j; ++i) G[(size_t)j * mc + i] = 0.0;  // lower triangle only
            if (!cholesky_lower(mc, G.data(), 1e-10)) return false;  // (nearly) dependent vectors: the sequential path
            lower_inverse(mc, G.data(), Li.data());
            gemm_nt_cols(Zg, Li.data(), Zn.data(), n, mc, mc, 0, mc);  // Z L^-T
            std::copy(Zn.begin(), Zn.end(), Zg);
            if (pass == 0 && off < 1e-5) break;  // one pass leaves an error ~ eps (1 + off^2 ...): enough
        }
        for (int jj = 0; jj < mc; ++jj)
            if (!converged(n, d, e, onenrm, Zg + (size_t)jj * n, lam[gp + jj])) return false;
        return true;
    };
    std::vector<char> done_group(ngroups, 0);
    for (int g = 0; g < ngroups; ++g)
        if (starts[g + 1] - starts[g] >= kBlockMin) {
            if (!do_group_block(starts[g], starts[g + 1]) && !do_group(starts[g], starts[g + 1])) return false;
            done_group[g] = 1;
        }
#if defined(__x86_64__)
    {   // isolated eigenvalues (clusters of one: nothing to orthogonalise against), eight per sweep
        const bool x8 = __builtin_cpu_supports("avx512f") && !o.no_x8;
        std::vector<int> single;
        if (x8 && n >= 16)
            for (int g = 0; g < ngroups; ++g)
                if (!done_group[g] && starts[g + 1] - starts[g] == 1) single.push_back(g);
        if (single.size() >= 3)
            for (size_t s0 = 0; s0 < single.size(); s0 += 8) {
                const int m8 = (int)std::min<size_t>(8, single.size() - s0);
                double lam8[8];
                int idx8[8];
                double* zc[8];
                for (int l = 0; l < m8; ++l) {
                    const int j = starts[single[s0 + l]];
                    lam8[l] = lam[j];
                    idx8[l] = j;
                    zc[l] = Z + (size_t)j * n;
                }
                if (!inverse_iteration_x8(n, d, e, lam8, idx8, m8, onenrm, zc)) return false;
                for (int l = 0; l < m8; ++l) done_group[single[s0 + l]] = 1;
            }
    }
#endif
    // work of a cluster of m vectors ~ m n (8 + m) (solves + re-orthogonalisation), ~2.6 ns per unit on the GPU box's cores;
    // threads (~0.1 ms to start and join) pay off from ~0.8 ms of it
    double work = 0.0;
    for (int g = 0; g < ngroups; ++g) {
        const double m = done_group[g] ? 0.0 : starts[g + 1] - starts[g];
        work += m * n * (8.0 + m);
    }
    const int nthreads = (ngroups >= 2 && work > 3e5) ? std::min(4, ngroups) : 1;
    // contiguous runs of clusters of about equal work per thread (one thread: all of them, in the caller)
    std::vector<int> cut(nthreads + 1, ngroups);
    cut[0] = 0;
    {
        double acc = 0.0;
        int t = 1;
        for (int g = 0; g < ngroups && t < nthreads; ++g) {
            const double m = done_group[g] ? 0.0 : starts[g + 1] - starts[g];
            acc += m * n * (8.0 + m);
            if (acc >= work * t / nthreads) cut[t++] = g + 1;
        }
    }
    std::vector<char> okv(nthreads, 1);
    run_split(nthreads, nthreads, [&](int t) {
        for (int g = cut[t]; g < cut[t + 1]; ++g)
            if (!done_group[g] && !do_group(starts[g], starts[g + 1])) {
                okv[t] = 0;
                return;
            }
    });
    return std::count(okv.begin(), okv.end(), 0) == 0;
}

// ---- a FEW eigenvalues of the tridiagonal form by bisection on Sturm counts, up to 64 shifts per sweep of T.
// What the train path needs of Q is its K leading eigenpairs and the NUMBER of eigenvalues >= 1e-10 (src/filter.cpp:313-316), of
// Wa the number below 1e-10, those few eigenvalues, and the largest (the deflated root): an implicit QL run for all n
// eigenvalues (0.31 ms at n = 200 on the GPU box's host, a chain of dependent rotations) is replaced by counts.  A count is
// a chain of n - 1 dependent divisions (~20 cycles each): eight shifts ride in one AVX-512 vector and up to eight vectors are
// interleaved so the divider stays busy -- 50 eigenvalues are ONE sweep of T per halving, ~55 halvings.  Accuracy: the
// count is exact for a tridiagonal matrix within a few ulp ||T|| of T (dstebz's recurrence with its pivmin guard), the same
// backward error the QL iteration has; the rank cut at eps is one more count.
typedef long long v8l __attribute__((vector_size(64)));
SturmT sturm_setup(int n, const double* d, const double* e) {
    SturmT t{n, d, std::vector<double>(n, 0.0), 0.0, 0.0, 0.0};
    double emax2 = 0.0, lo = d[0], hi = d[0];
    for (int i = 1; i < n; ++i) {
        t.e2[i] = e[i] * e[i];
        emax2 = std::max(emax2, t.e2[i]);
    }
    for (int i = 0; i < n; ++i) {
        const double r = (i > 0 ? std::fabs(e[i]) : 0.0) + (i + 1 < n ? std::fabs(e[i + 1]) : 0.0);
        lo = std::min(lo, d[i] - r);
        hi = std::max(hi, d[i] + r);
    }
    const double nrm = std::max(std::fabs(lo), std::fabs(hi));
    t.pivmin = 2.2250738585072014e-308 * std::max(1.0, emax2);
    t.lo = lo - 2.0 * 2.220446049250313e-16 * nrm * n - 2.0 * t.pivmin;
    t.hi = hi + 2.0 * 2.220446049250313e-16 * nrm * n + 2.0 * t.pivmin;
    return t;
}
// cnt[v] = number of eigenvalues of T smaller than each of the shifts s[v] (NV vectors of eight).  Intrinsics, not vector
// extensions: GCC scalarises 512-bit vector comparisons inside target_clones (measured: 48 cycles per vector step).
template <int NV>
__attribute__((target("avx512f"))) static void sturm_counts_avx512(int n, const double* d, const double* e2, double pivmin,
                                                                    const v8d* s, v8l* cnt) {
    const __m512d pm = _mm512_set1_pd(pivmin), npm = _mm512_set1_pd(-pivmin), zero = _mm512_setzero_pd();
    const __m512i one = _mm512_set1_epi64(1);
    __m512d q[NV], sv[NV];
    __m512i c[NV];
    for (int v = 0; v < NV; ++v) {
        sv[v] = _mm512_loadu_pd(&s[v]);
        q[v] = _mm512_sub_pd(_mm512_set1_pd(d[0]), sv[v]);
        q[v] = _mm512_mask_mov_pd(q[v], _mm512_cmp_pd_mask(_mm512_abs_pd(q[v]), pm, _CMP_LT_OQ), npm);
        c[v] = _mm512_maskz_mov_epi64(_mm512_cmp_pd_mask(q[v], zero, _CMP_LT_OQ), one);
    }
    for (int i = 1; i < n; ++i) {
        const __m512d di = _mm512_set1_pd(d[i]), ei = _mm512_set1_pd(e2[i]);
        for (int v = 0; v < NV; ++v) {
            q[v] = _mm512_sub_pd(_mm512_sub_pd(di, sv[v]), _mm512_div_pd(ei, q[v]));
            q[v] = _mm512_mask_mov_pd(q[v], _mm512_cmp_pd_mask(_mm512_abs_pd(q[v]), pm, _CMP_LT_OQ), npm);
            c[v] = _mm512_mask_add_epi64(c[v], _mm512_cmp_pd_mask(q[v], zero, _CMP_LT_OQ), c[v], one);
        }
    }
    for (int v = 0; v < NV; ++v) _mm512_storeu_si512(&cnt[v], c[v]);
}
static void sturm_counts_scalar(int n, const double* d, const double* e2, double pivmin, const v8d* s, int nv, v8l* cnt) {
    for (int v = 0; v < nv; ++v) {
        double q[8], sh[8];
        long long c[8];
        for (int l = 0; l < 8; ++l) {
            sh[l] = s[v][l];
            q[l] = d[0] - sh[l];
            if (std::fabs(q[l]) < pivmin) q[l] = -pivmin;
            c[l] = q[l] < 0.0;
        }
        for (int i = 1; i < n; ++i)
            for (int l = 0; l < 8; ++l) {
                q[l] = (d[i] - sh[l]) - e2[i] / q[l];
                if (std::fabs(q[l]) < pivmin) q[l] = -pivmin;
                c[l] += q[l] < 0.0;
            }
        for (int l = 0; l < 8; ++l) cnt[v][l] = c[l];
    }
}
static void sturm_counts(const SturmT& t, const v8d* s, int nv, v8l* cnt) {
    static const bool avx512 = __builtin_cpu_supports("avx512f");
    if (!avx512) return sturm_counts_scalar(t.n, t.d, t.e2.data(), t.pivmin, s, nv, cnt);
    switch (nv) {  // (direct calls: through a table of pointers the kernels lose what they know about s's alignment)
        case 1: sturm_counts_avx512<1>(t.n, t.d, t.e2.data(), t.pivmin, s, cnt); break;
        case 2: sturm_counts_avx512<2>(t.n, t.d, t.e2.data(), t.pivmin, s, cnt); break;
        case 3: sturm_counts_avx512<3>(t.n, t.d, t.e2.data(), t.pivmin, s, cnt); break;
        case 4: sturm_counts_avx512<4>(t.n, t.d, t.e2.data(), t.pivmin, s, cnt); break;
        case 5: sturm_counts_avx512<5>(t.n, t.d, t.e2.data(), t.pivmin, s, cnt); break;
        case 6: sturm_counts_avx512<6>(t.n, t.d, t.e2.data(), t.pivmin, s, cnt); break;
        case 7: sturm_counts_avx512<7>(t.n, t.d, t.e2.data(), t.pivmin, s, cnt); break;
        default: sturm_counts_avx512<8>(t.n, t.d, t.e2.data(), t.pivmin, s, cnt); break;
    }
}
int sturm_count1(const SturmT& t, double s) {
    const v8d sv = {s, s, s, s, s, s, s, s};
    v8l c;
    sturm_counts(t, &sv, 1, &c);
    return (int)c[0];
}
// the eigenvalues number k[0 .. m) of T counted from the SMALLEST (k = 0), m <= 64, to the last bit the counts resolve
void sturm_bisect(const SturmT& t, const int* k, int m, double* out) {
    const int nv = (m + 7) / 8;
    v8d lo[8], hi[8], mid[8];
    v8l kk[8], c[8];
    for (int l = 0; l < 8 * nv; ++l) {
        lo[l / 8][l % 8] = t.lo;
        hi[l / 8][l % 8] = t.hi;
        kk[l / 8][l % 8] = k[l < m ? l : m - 1];
    }
    // to one ulp of ||T|| (what any eigenvalue of T is defined to; a relative criterion would spend 40 more halvings on the
    // eigenvalues near the 1e-10 cut for digits the reduction never had)
    const double tol = 2.220446049250313e-16 * std::max(std::fabs(t.lo), std::fabs(t.hi)) + 2.0 * t.pivmin;
    for (int it = 0; it < 1100; ++it) {  // a double has 2098 binades at most; ~55 halvings when lambda is O(||T||)
        for (int v = 0; v < nv; ++v) mid[v] = 0.5 * (lo[v] + hi[v]);
        sturm_counts(t, mid, nv, c);
        bool done = true;
        for (int v = 0; v < nv; ++v) {
            const v8l up = c[v] > kk[v];  // more than k eigenvalues below mid: lambda_k < mid
            hi[v] = up ? mid[v] : hi[v];
            lo[v] = up ? lo[v] : mid[v];
            for (int l = 0; l < 8; ++l) {
                const double m2 = 0.5 * (lo[v][l] + hi[v][l]);
                if (hi[v][l] - lo[v][l] > tol && m2 > lo[v][l] && m2 < hi[v][l]) done = false;
            }
        }
        if (done) break;
    }
    for (int l = 0; l < m; ++l) out[l] = 0.5 * (lo[l / 8][l % 8] + hi[l / 8][l % 8]);
}
// eigenvalues with DESCENDING numbers [first, first + count) (number 0 = the largest) into out[0 .. count)
void sturm_eigenvalues_desc(const SturmT& t, int first, int count, double* out) {
    for (int j0 = 0; j0 < count; j0 += 64) {
        const int m = std::min(64, count - j0);
        int k[64];
        for (int l = 0; l < m; ++l) k[l] = t.n - 1 - (first + j0 + l);
        sturm_bisect(t, k, m, out + j0);
    }
}

}  // namespace nleh
