// Tables of the 16-bit sRGB <-> float Lab conversion (srgb16.h; the definition is DESIGN.md section 3.13).  The tables are
// fp64; the matrices are made in fp64, every operation rounded on its own (this file is compiled with -ffp-contract=off):
// a test restates the device arithmetic from these numbers.
#include <cmath>
#include <limits>

#include "srgb16.h"

namespace nlesrgb16 {
namespace {

// the sRGB decoding curve at code / 65535.  Evaluated in long double and rounded once: in fp64 the rounding of the base
// alone, amplified by the exponent, costs up to 6 ulp of the result (measured), and thr must separate neighbouring codes
// of lin by construction, not by luck.  The constants are the decimal ones at that precision, so that white decodes to 1.
double decode(long double code) {
    const long double v = code / 65535.0L;
    if (v <= 0.04045L) return (double)(v / 12.92L);
    return (double)std::pow((v + 0.055L) / 1.055L, 2.4L);
}

}  // namespace

void tables(double* lin, double* thr, double* coeffs) {
    for (int c = 0; c < kCodes; ++c) lin[c] = decode((long double)c);
    // code = (number of c with thr[c] <= v) - 1: the encoding's steps lie half a code below every code
    thr[0] = -std::numeric_limits<double>::infinity();
    for (int c = 1; c < kCodes; ++c) thr[c] = decode((long double)c - 0.5L);
    // OpenCV's sRGB -> XYZ (D65), each row over its own sum: white (1, 1, 1) goes to X = Y = Z = 1
    const double M[3][3] = {{0.412453, 0.357580, 0.180423}, {0.212671, 0.715160, 0.072169}, {0.019334, 0.119193, 0.950227}};
    double* F = coeffs;      // rows X, Y, Z; columns R, G, B
    double* I = coeffs + 9;  // rows R, G, B; columns X, Y, Z
    for (int r = 0; r < 3; ++r) {
        const double s = (M[r][0] + M[r][1]) + M[r][2];
        for (int c = 0; c < 3; ++c) F[3 * r + c] = M[r][c] / s;
    }
    // the inverse by cofactors
    const double c00 = F[4] * F[8] - F[5] * F[7], c01 = F[5] * F[6] - F[3] * F[8], c02 = F[3] * F[7] - F[4] * F[6];
    const double det = (F[0] * c00 + F[1] * c01) + F[2] * c02;
    I[0] = c00 / det;
    I[1] = (F[2] * F[7] - F[1] * F[8]) / det;
    I[2] = (F[1] * F[5] - F[2] * F[4]) / det;
    I[3] = c01 / det;
    I[4] = (F[0] * F[8] - F[2] * F[6]) / det;
    I[5] = (F[2] * F[3] - F[0] * F[5]) / det;
    I[6] = c02 / det;
    I[7] = (F[1] * F[6] - F[0] * F[7]) / det;
    I[8] = (F[0] * F[4] - F[1] * F[3]) / det;
}

}  // namespace nlesrgb16
