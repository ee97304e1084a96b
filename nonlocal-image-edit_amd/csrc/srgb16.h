// 16-bit sRGB <-> float Lab (the deep-colour wrapper): the host tables and the layout of the blob
// a ctx uploads on first use.  lin[c] decodes code c, thr[c] is the linear value where the encoding steps from c - 1 to c
// (thr[0] = -inf), coeffs = the white-normalised sRGB -> XYZ matrix (rows X, Y, Z) and its inverse (rows R, G, B).
#pragma once

namespace nlesrgb16 {

constexpr int kCodes = 65536;
constexpr int kCoeffs = 18;
// the device blob, in doubles: lin | coeffs | pairs -- what the kernels read.  pairs[c] = (thr[c], thr[c + 1]) with
// thr[65536] = +inf: the threshold search takes one aligned 16-byte gather per step (kOffPairs is even and the blob's base is
// 16-byte aligned).  The host keeps thr itself behind the blob, for nle_srgb16_tables; it is not uploaded.
constexpr int kOffLin = 0, kOffCoeffs = kCodes, kOffPairs = kCodes + kCoeffs, kBlobDoubles = kOffPairs + 2 * kCodes;
constexpr int kOffThrHost = kBlobDoubles, kHostDoubles = kBlobDoubles + kCodes;
static_assert(kOffPairs % 2 == 0, "the pairs must be 16-byte aligned");

void tables(double* lin, double* thr, double* coeffs);  // srgb16_tables.cpp (built without contraction)

}  // namespace nlesrgb16
