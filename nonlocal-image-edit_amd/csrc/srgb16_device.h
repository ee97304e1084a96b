// The device side of the 16-bit sRGB encoding (srgb16.h): the threshold search both 16-bit writers use -- the deep-colour
// inverse (colour16.hip) and the tone mapper's (tonemap.hip).  Include after <hip/hip_runtime.h> and after the file's
// `#pragma clang fp contract(off)`: the first guess is fp32 arithmetic rounded operation by operation, like the rest.
#pragma once

namespace nlek {

// code = (number of c with thr[c] <= v) - 1, a NaN gives 0.  An fp32 evaluation of the encoding gives a first guess (a
// small fraction of a code off), the thresholds decide: pairs[g] = (thr[g], thr[g + 1]) in one aligned 16-byte gather
// (thr[0] = -inf, thr[65536] = +inf), and the loop ends at thr[g] <= v < thr[g + 1] whatever the guess was, one step and
// one gather per round -- a single round for nearly every pixel.
__device__ __forceinline__ int code_of(double v, const double2* __restrict__ pairs) {
    if (!(v == v)) return 0;
    const float vf = (float)v;
    const float e = vf <= 0.0031308f ? 12.92f * vf : 1.055f * exp2f(log2f(vf) * (1.f / 2.4f)) - 0.055f;
    int g = (int)fminf(65535.f, fmaxf(0.f, rintf(65535.f * e)));  // a NaN e (vf < 0 cannot reach the log) would give 0
    for (;;) {
        double2 t = pairs[g];
        asm volatile("" : "+v"(t.x), "+v"(t.y));  // both halves are used here: keeps the pair one 16-byte load
        if (v < t.x) --g;  // never at g = 0: thr[0] = -inf
        else if (v >= t.y && g < 65535) ++g;  // v = +inf meets the last pair's +inf: the index stays inside the table
        else return g;
    }
}

}  // namespace nlek
