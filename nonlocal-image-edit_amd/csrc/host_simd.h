// What the host fp64 sources (host_dense.cpp, eigen_reduce.cpp, eigen_tridiag.cpp) write their inner loops on.  Everything
// here must inline into its caller, hence `static inline`: a copy per translation unit, the same code in each.
#pragma once
#include <cmath>
#include <cstddef>

// The O(n^3) loops are unit-stride; the library is built without -march (it has to run on whatever host the GPU box has),
// so they are multiversioned and resolved at load time.
#define NLE_SIMD_CLONES __attribute__((target_clones("default", "avx2", "avx512f")))

namespace nleh {

static inline double& at(double* v, int n, int row, int col) { return v[(size_t)col * n + row]; }

// hypot without the libm call on the common path (no overflow/underflow of the squares)
static inline double hyp(double a, double b) {
    const double s = a * a + b * b;
    return (s > 1e-280 && s < 1e280) ? std::sqrt(s) : std::hypot(a, b);
}

typedef double v8d __attribute__((vector_size(64)));  // eight doubles
static inline __attribute__((always_inline)) v8d ld8(const double* p) {
    v8d v;
    __builtin_memcpy(&v, p, sizeof(v));
    return v;
}
static inline __attribute__((always_inline)) void st8(double* p, v8d v) { __builtin_memcpy(p, &v, sizeof(v)); }
static inline __attribute__((always_inline)) double hsum8(v8d v) {
    return ((v[0] + v[4]) + (v[2] + v[6])) + ((v[1] + v[5]) + (v[3] + v[7]));
}

}  // namespace nleh
