"""The fp32 stage kernels, each ALONE and entry by entry: k_affinity (nle_compute_kernel), k_tsgemm<NT, false> (nle_ts_gemm),
k_rowpass<G, QPL> (nle_sinkhorn_scalings), k_row_scalings<G, QPL> (nle_row_scalings), k_gram + k_gram_reduce (nle_gram) of
csrc/kernels.hip, and the two fused Nystrom GEMMs behind nle_nystrom: k_tsgemm<NT, true> and, with
Context.set_nystrom_bf16x3, k_tsgemm_bf16x3<NT> of csrc/tsgemm_bf16x3.hip.  What tests/test_stage64.py is for the fp64 family.

1. EXACT ARITHMETIC: no tolerance.  Small non-negative integers make every product and every partial sum an integer below
2^24 (fp32) or 2^53 (fp64): any summation order, any rounding mode, fused or not, gives the same bits, so the device must
EQUAL the integer product.  A wrong index cannot hide in a norm.
    ts_gemm        A in {0..7} with the row pattern (i 7 + k) % 8 added (rows differ), B in {-3..3} (integers survive h_B's
                   fp64 -> fp32 conversion), kd <= 300: |sum| <= 300 * 21.  C[:, :nc] == A B, C[:, nc:] == 0
    gram, u NULL   X in {0..3}: G == X^T X (<= 9 M; M = 300 000: the fp32 sum stays inside a chunk of gram_chunk_rows(M) = 320
                   rows, 9 * 320 < 2^24, the chunks are summed in fp64), G == G^T
    row_scalings   X in {1..7}, u in {1..5}: s = X u is an exact integer, recip_or_zero is the plain fp64 division 1.0 / s
                   (csrc/kernels.hip: `(fabs(s) >= eps) ? 1.0 / s : 0.0`, no fast-math in the build), IEEE-correctly rounded on
                   both sides: out == 1.0 / s bit for bit
    sinkhorn_scalings, max_iter = 1: one COLSUM pass and one RECIP pass of k_rowpass (u_c = lam o X^T 1, u_r = lam o X^T
                   recip(X u_c)).  Sums of reciprocals are not exact: the project's figure for this stage, relative L2 <= 1e-10
                   on u_c and u_r against the longdouble loop (tests/test_stage64.py: sinkhorn_reference)
    ld = 2052      (r = 2049..2052) has no (G, QPL): nle_row_scalings and nle_sinkhorn_scalings return an error and leave
                   nle_last_error set.  (nle_gram does not go through pick_gq; its LDS bound is another limit, not tested here.)

Widths.  pick_gq (csrc/kernels.hip) maps the row stride ld to G lanes per row and QPL float4 per lane; `pick_gq` below is
its mirror, test_width_table_covers_every_instantiation holds the table to it.  Every pair it can return, at a width r with
r % 4 == 0 and at one with r % 4 != 0 (nq = ld / 4; the switches nq = 32 | 33, 64 | 65, 128 | 129, 256 | 257 and the last
width that dispatches, ld = 2048, are in it):
    (G, QPL)   r (nq)               (G, QPL)   r (nq)               (G, QPL)   r (nq)
    ( 4, 1)    4 (1), 13 (4)        ( 8, 6)    132 (33), 190 (48)   (32, 6)    516 (129), 766 (192)
    ( 4, 2)    32 (8), 17 (5)       ( 8, 7)    196 (49), 222 (56)   (32, 7)    772 (193), 894 (224)
    ( 4, 4)    36 (9), 61 (16)      ( 8, 8)    256 (64), 229 (58)   (32, 8)    1024 (256), 901 (226)
    ( 4, 6)    68 (17), 95 (24)     (16, 6)    260 (65), 383 (96)   (64, 6)    1028 (257), 1535 (384)
    ( 4, 7)    100 (25), 110 (28)   (16, 7)    388 (97), 446 (112)  (64, 7)    1540 (385), 1790 (448)
    ( 4, 8)    128 (32), 113 (29)   (16, 8)    512 (128), 453 (114) (64, 8)    2048 (512), 1797 (450)
Rows: 1, 4 (64 / G) - 1 and + 1 (one workgroup's rows, short and over by one), 1000; the Sinkhorn pass once with
kRowpassMaxBlocks (csrc/kernels.h) * 64 + 65 rows at r = 4: past one grid-stride round.

2. REAL DATA: derived elementwise bounds.  Data as in test_stage64.py, (|N(0,1)| + 0.1) / sqrt(width) rounded to fp32: every
dot product has condition number 1.  u32 = 2^-24, u64 = 2^-53, g_t(k) = k u_t / (1 - k u_t): a sum of k terms each carrying at
most k roundings (1 + d), |d| <= u_t, in any order, fused or not, is within g_t(k) sum |terms| (Higham, Accuracy and Stability
of Numerical Algorithms, section 3.1).  References are formed in np.longdouble (64-bit significand).  The model: the matrix
core's fp32 accumulation rounds to nearest -- the largest err / bound per kernel is printed by every case and recorded in
profiles/r18_stage32_edges.txt; none passes 0.61 (the matrix-core kernels: 0.33), so the chopping model (unit 2^-23) was
never needed.
    ts_gemm   v_mfma_f32_32x32x2_f32 is a chain of fp32 fmas over k (zero-padded k terms add exactly): kd roundings
              |C - A B32| <= g32(kd + 2) (|A| |B32|),  B32 = fp32(h_B)
    gram, u given   per row s_i = x_i . u in fp64 (<= r roundings per term: g64(r)), c_i = 1 / s_i (one more), cf = (float)c_i
              (u32), z_ij = fp32(x_ij cf) (u32): z_ia z_ib = c_i^2 x_ia x_ib (1 + d)^(4 of u32, 2 (r + 1) of u64).  The MFMA adds
              the rows of one chunk in fp32, one rounding per row: R = min(M, gram_chunk_rows(M)) more of u32.  The chunk sums
              are exact doubles added in fp64 by k_gram_reduce: nchunks more of u64.  With Z = diag(c) X, c from the longdouble
              reference:   |G - Z^T Z| <= [(1 + g32(R + 4)) (1 + g64(2 (r + 1) + nchunks)) - 1] (|Z|^T |Z|),   G == G^T
    affinity  affinity_value (csrc/kernels.h): arg = nsw d2 + npw dv^2, k = v_exp_f32(arg).  d2 = dr^2 + dc^2 is an exact
              integer (H W < 2^24).  nsw = fp32(-log2(e) / hx^2): one rounding, the product nsw d2 one, the sum one: the spatial
              term carries 3.  npw one, dv = fp32(px - sz) one but squared (2), dv dv one, the product with npw one, the sum
              one: the range term carries 6.  Both terms are <= 0, so |d arg| <= g32(6) |arg| (contraction to fma only removes
              roundings).  v_exp_f32: "1 ULP accuracy" (AMD GCN3 / CDNA instruction set guides, V_EXP_F32), i.e. relative
              2^-23 = 2 u32.  The fp64 roundings of the host's nsw, npw and of the oracle are below 2^-45.  So
                  |k - k_ref| <= [(1 + expm1(g32(6) |arg| ln 2)) (1 + 2 u32) - 1 + 2^-45] k_ref  =: e_aff k_ref
              -- to first order (a |arg| ln 2 + b) u32 k_ref with a = 6, b = 2 -- for |arg| <= 60 (no flushed result; held on
              the CPU for every case).  Padding columns exactly 0.
    nystrom   Phi = K B, B = V_A / lambda.  build_phi scatters fp32(V_A) into Phi's sample rows and nle_nystrom returns lambda,
              so the test rebuilds B from the result itself: the kernel's B32 = fp32(V_A fl64(1 / lambda)) is within 2 u32 of
              fp32(V_A) / lambda.  k_tsgemm<NT, true> accumulates p terms as above.  Every NON-sample row:
                  |Phi - K_ref B| <= sum_s [g32(p + 2) + e_aff(i, s) + 2 u32 (+ e_split)] K_ref(i, s) |B(s, j)| + 2^-125 sum_s |B(s, j)|
              (the last term: where K_ref < 2^-126 the fp32 affinity may be flushed; the planes are many bandwidths wide).
              e_split, k_tsgemm_bf16x3: x = h + m + l exactly (x has 24 bits, h = bf16(x) takes 8, r1 = x - h fits 16, m 8, r2 =
              r1 - m fits 8 = l), |m| <= 2^-8 |x|, |l| <= 2^-16 |x|.  Of the nine products the kernel drops am bl, al bm, al bl:
              e_split = (2^-24 + 2^-24 + 2^-32) = (2 + 2^-8) u32 <= 3 u32, the figure of the kernel's header.  The two kernels
              see the same affinities and the same B: their difference is held to the bound with both terms.
              Grids: hx = the sample spacing, so K_A has full numerical rank: r == p is a condition of every case, held on the
              CPU from the oracle alone (test_nystrom_cases_have_full_rank) and asserted again on the device's r.  p % 16 in {0,
              1, 7, 8, 9, 15} around the bf16 kernel's 16-deep step and 8-deep k blocks; p <= 32 | 33..64 (NT 1 | 2), 96, 100, 160,
              192 (NT 3..6), 224 | 228 (bf16: 7 tiles in one panel | 4 + 4; fp32: NT 7 | 8), 256 | 260 (fp32: 8 tiles | 5 + 5, the last
              tile wholly beyond ldc); H W % 128 in {0, 1, 127}.

3. The checkers are plain functions of (result, inputs).  test_checkers_* (no GPU) feed them numpy's own fp32 results, which
must pass, and what a wrong tile, tail or lane map would produce -- one row repeated, one 32-column tile shifted by 4 rows,
the last k term dropped from one tile, one chunk left out of the Gram, two rows of the MFMA element map swapped -- each of which
must fail.

4. Leading dimension (include/nle.h, above nle_ts_gemm): the fp32 entry points read whole float4 quads, so ld % 4 == 0 and
zero padding are the caller's duty; ld % 4 != 0 is NLE_ERR_INVALID before anything is launched (test_fp32_ld_contract).
"""
import functools
import os
import re

import numpy as np
import pytest

from test_stage64 import LD, check_sinkhorn, positive, recip_ld, sinkhorn_reference  # (skips without a 64-bit longdouble)

U32 = 2.0 ** -24
U64 = 2.0 ** -53
LN2 = float(np.log(2.0))
E_SPLIT = (2.0 + 2.0 ** -8) * U32
ARG_MAX = 60.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def g32(k):
    return k * U32 / (1.0 - k * U32)


def g64(k):
    return k * U64 / (1.0 - k * U64)


def nle_ld(n):
    return (n + 3) & ~3


# ------------------------------------------------------------------ mirrors of the dispatch in csrc/kernels.hip
def pick_gq(ld):
    nq = ld // 4
    for G in (4, 8, 16, 32, 64):
        if G * 8 >= nq:
            q = max((nq + G - 1) // G, 1)
            return G, {3: 4, 5: 6}.get(q, q)
    return None


def tsgemm_nt(ldc, per_panel=8):
    """(column tiles per workgroup, panels) of launch_tsgemm (8) and of ts_gemm_bf16x3 (7)"""
    ntiles = (ldc + 31) // 32
    panels = (ntiles + per_panel - 1) // per_panel
    return (ntiles + panels - 1) // panels, panels


def gram_chunk_rows(M):
    fl = (M + 1023) // 1024
    return min(max((fl + 31) // 32 * 32, 256), 8192)


def rowpass_max_blocks():
    with open(os.path.join(ROOT, "nonlocal-image-edit_amd", "csrc", "kernels.h")) as f:
        return int(re.search(r"constexpr int kRowpassMaxBlocks = (\d+);", f.read()).group(1))


# r -> (G, QPL): the table of the module docstring
WIDTHS = {4: (4, 1), 13: (4, 1), 32: (4, 2), 17: (4, 2), 36: (4, 4), 61: (4, 4), 68: (4, 6), 95: (4, 6), 100: (4, 7), 110: (4, 7),
          128: (4, 8), 113: (4, 8), 132: (8, 6), 190: (8, 6), 196: (8, 7), 222: (8, 7), 256: (8, 8), 229: (8, 8),
          260: (16, 6), 383: (16, 6), 388: (16, 7), 446: (16, 7), 512: (16, 8), 453: (16, 8),
          516: (32, 6), 766: (32, 6), 772: (32, 7), 894: (32, 7), 1024: (32, 8), 901: (32, 8),
          1028: (64, 6), 1535: (64, 6), 1540: (64, 7), 1790: (64, 7), 2048: (64, 8), 1797: (64, 8)}
ALL_GQ = [(4, q) for q in (1, 2, 4, 6, 7, 8)] + [(G, q) for G in (8, 16, 32, 64) for q in (6, 7, 8)]


def rows_for(G):
    return [1, 4 * (64 // G) - 1, 4 * (64 // G) + 1, 1000]


# ------------------------------------------------------------------ inputs
def padded32(X, ld=None):
    M, w = X.shape
    out = np.zeros((M, nle_ld(w) if ld is None else ld), dtype=np.float32)
    out[:, :w] = X
    return out


def int_gemm_inputs(M, kd, nc):
    rng = np.random.default_rng(100003 * M + 1009 * kd + nc)
    A = (rng.integers(0, 8, (M, kd)) + np.arange(M)[:, None] * 7 + np.arange(kd)[None, :]) % 8
    return A.astype(np.int64), rng.integers(-3, 4, (kd, nc)).astype(np.int64)


def positive32(rng, M, width):
    return positive(rng, M, width).astype(np.float32)


# ------------------------------------------------------------------ checkers
def _worst(err, bound):
    """(largest err / bound, position of the first entry beyond the bound or None)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))
    bad = np.argwhere(err > bound)
    return float(ratio.max()) if ratio.size else 0.0, (bad[0].tolist() if bad.size else None)


def check_ts_gemm_exact(C, A, B):
    """C: M x nle_ld(nc) device result for integer A (M x kd), B (kd x nc)"""
    C = np.asarray(C)
    (M, kd), nc = A.shape, B.shape[1]
    assert C.shape == (M, nle_ld(nc)), (C.shape, M, nc)
    assert np.all(C[:, nc:] == 0), "padding columns of the output must be exactly zero"
    ref = A @ B
    assert np.abs(ref).max() < 2 ** 24
    bad = np.argwhere(C[:, :nc] != ref)
    assert bad.size == 0, (f"{len(bad)} entries differ from the integer product; first (row, col) {bad[0].tolist()}: tile "
                           f"{bad[0][1] // 32}, row in block {bad[0][0] % 128}, got {C[tuple(bad[0])]} want {ref[tuple(bad[0])]}")


def check_ts_gemm(C, A, B):
    """C: M x nle_ld(nc) result for fp32 A (M x kd) and fp64 B (kd x nc) as nle_ts_gemm takes them; returns max err / bound"""
    C, A = np.asarray(C), np.asarray(A)
    B32 = np.asarray(B).astype(np.float32)
    (M, kd), nc = A.shape, B32.shape[1]
    assert C.shape == (M, nle_ld(nc)), (C.shape, M, nc)
    assert np.all(C[:, nc:] == 0), "padding columns of the output must be exactly zero"
    assert np.isfinite(C).all()
    ref = A.astype(LD) @ B32.astype(LD)
    bound = g32(kd + 2) * (np.abs(A).astype(LD) @ np.abs(B32).astype(LD))
    worst, first = _worst(np.abs(C[:, :nc].astype(LD) - ref), bound)
    assert first is None, f"entries beyond g32({kd + 2}) |A||B|; first at {first}, max err/bound {worst:.3g}"
    return worst


def check_gram_exact(G, X):
    G = np.asarray(G)
    M, r = X.shape
    assert G.shape == (r, r)
    assert np.array_equal(G, G.T), "G must be exactly symmetric"
    ref = X.T @ X
    bad = np.argwhere(G != ref)
    assert bad.size == 0, (f"{len(bad)} entries differ from the integer X^T X; first {bad[0].tolist()} (tile "
                           f"{(bad[0] // 32).tolist()}): got {G[tuple(bad[0])]} want {ref[tuple(bad[0])]}")


def check_gram(G, X, u):
    """G: r x r result for sum_i c_i^2 x_i x_i^T, c = recip(X u), X fp32; returns max err / bound"""
    G, X = np.asarray(G), np.asarray(X)
    M, r = X.shape
    assert G.shape == (r, r) and np.isfinite(G).all()
    assert np.array_equal(G, G.T), "G must be exactly symmetric"
    rows = gram_chunk_rows(M)
    nchunks = (M + rows - 1) // rows
    Xl = X.astype(LD)
    Z = Xl * recip_ld(Xl @ np.asarray(u).astype(LD))[:, None]
    factor = (1 + g32(min(M, rows) + 4)) * (1 + g64(2 * (r + 1) + nchunks)) - 1
    worst, first = _worst(np.abs(G.astype(LD) - Z.T @ Z), factor * (np.abs(Z).T @ np.abs(Z)))
    assert first is None, f"entries beyond {factor:.3g} |Z|^T|Z|; first at {first}, max err/bound {worst:.3g}"
    return worst


def check_row_scalings_exact(out, X, u):
    out = np.asarray(out)
    s = X.astype(np.int64) @ u.astype(np.int64)
    assert (s > 0).all() and s.max() < 2 ** 53
    ref = 1.0 / s.astype(np.float64)
    bad = np.argwhere(out != ref)
    assert out.shape == ref.shape and bad.size == 0, f"{len(bad)} rows differ from 1.0 / s; first row {bad[0].tolist()}"


class Plane:
    """a sample grid on a plane of fp32 luminances and the fp64 oracle's view of it (nothing here needs a GPU)"""

    def __init__(self, oracle, H, W, nr, nc, hx, hy):
        self.H, self.W, self.nr, self.nc, self.hx, self.hy = H, W, nr, nc, hx, hy
        rng = np.random.default_rng(H * 1000 + W * 7 + nr)
        self.x = rng.uniform(20.0, 235.0, (H, W)).astype(np.float32)
        self.perm, self.Ka, Kab = oracle.compute_kernel(self.x.astype(np.float64), nr, nc, hx, hy)
        self.p = self.Ka.shape[0]
        self.sel, self.rest = self.perm[:self.p], self.perm[self.p:]
        self.K = np.empty((H * W, self.p))       # affinity rows of every pixel, natural order
        self.K[self.perm] = np.vstack([self.Ka, Kab.T])
        with np.errstate(divide="ignore"):
            self.L = -np.log(self.K)              # |arg| ln 2


def e_aff(L):
    """relative bound of one fp32 affinity with |arg| ln 2 = L (module docstring)"""
    return (1.0 + np.expm1(g32(6) * L)) * (1.0 + 2 * U32) - 1.0 + 2.0 ** -45


def check_affinity(kab, pl):
    """kab: N x nle_ld(p) device affinities of Plane pl; returns max err / bound"""
    kab = np.asarray(kab)
    assert kab.shape == (pl.H * pl.W, nle_ld(pl.p)), kab.shape
    assert np.all(kab[:, pl.p:] == 0), "padding columns of d_kab must be exactly zero"
    assert pl.L.max() <= ARG_MAX * LN2, "the case must keep |arg| <= 60"
    worst, first = _worst(np.abs(kab[:, :pl.p].astype(np.float64) - pl.K), e_aff(pl.L) * pl.K)
    assert first is None, f"affinities beyond (6 |arg| ln 2 + 2) u32 k_ref; first (pixel, sample) {first}, max err/bound {worst:.3g}"
    return worst


def nystrom_parts(phi, lam, pl):
    """over the non-sample rows, with B rebuilt from Phi's own sample rows: K_ref B, and bound(split), the elementwise bound"""
    p = pl.p
    B = phi[pl.sel, :p].astype(LD) / np.asarray(lam).astype(LD)[None, :]
    Bm, K = np.abs(B), pl.K[pl.rest]
    flat = K.astype(LD) @ Bm                                                      # |K_ref| |B|
    aff = (K * e_aff(np.minimum(pl.L[pl.rest], 1100.0))).astype(LD) @ Bm + 2.0 ** -125 * Bm.sum(axis=0)[None, :]

    def bound(split):
        return (g32(p + 2) + 2 * U32 + (E_SPLIT if split else 0.0)) * flat + aff
    return K.astype(LD) @ B, bound


def check_nystrom(phi, lam, r, pl, split, parts=None):
    """phi: N x nle_ld(p) device Phi, lam: its eigenvalues, r: its rank; returns max err / bound"""
    phi = np.asarray(phi)
    p = pl.p
    assert r == p == len(lam), f"K_A must have full numerical rank: r = {r}, p = {p}"
    assert phi.shape == (pl.H * pl.W, nle_ld(p)), phi.shape
    assert np.all(phi[:, p:] == 0), "padding columns of Phi must be exactly zero"
    assert np.isfinite(phi).all()
    ref, bound = parts if parts is not None else nystrom_parts(phi, lam, pl)
    worst, first = _worst(np.abs(phi[pl.rest, :p].astype(LD) - ref), bound(split))
    assert first is None, (f"Phi beyond the bound; first (non-sample row, column) {first} = pixel {pl.rest[first[0]]}, "
                           f"max err/bound {worst:.3g}")
    return worst


def check_nystrom_pair(phi0, phi3, lam, pl, bound):
    """the fp32 and the split-bf16 kernel against each other: the bound with both error terms"""
    phi0, phi3 = np.asarray(phi0), np.asarray(phi3)
    assert np.array_equal(phi0[pl.sel], phi3[pl.sel]), "the sample rows are the same exact V_A rows"
    worst, first = _worst(np.abs(phi3[pl.rest, :pl.p].astype(LD) - phi0[pl.rest, :pl.p].astype(LD)), bound)
    assert first is None, f"the two kernels differ beyond the bound; first {first}, max err/bound {worst:.3g}"
    return worst


# ------------------------------------------------------------------ case lists (from the switches in the two .hip files)
GEMM_M = [1, 127, 128, 129, 257]
GEMM_KD = [1, 31, 32, 33, 65, 300]                      # around the 32-deep KB step
GEMM_NC = [4, 32, 33, 65, 97, 129, 161, 193, 225, 256, 257, 260]   # NT 1, 1, 2, 3, 4, 5, 6, 7, 8, 8, 5 + 5, 5 + 5
GEMM_CASES = [c for i, nc in enumerate(GEMM_NC)
              for c in ((GEMM_M[i % 5], GEMM_KD[i % 6], nc), (GEMM_M[(i + 2) % 5], GEMM_KD[(i + 3) % 6], nc))]
GEMM_REAL = GEMM_CASES[1::2] + [(257, 300, 256), (129, 33, 257)]

GRAM_R = [1, 31, 32, 33, 193, 224, 225, 257]            # nt 1 -> 2; 28 tiles: one full group; 36: the second partly empty
GRAM_M = [1, 31, 32, 33, 256, 257, 769, 1025, 1281]     # the 32-row stage; 1 | 2 chunks; 3, 5, 6: the reduce's unroll and tail
GRAM_BIG = (300000, 4)                                  # gram_chunk_rows leaves its 256-row floor
GRAM_CASES = [c for i, M in enumerate(GRAM_M) for c in ((M, GRAM_R[i % 8]), (M, GRAM_R[(i + 3) % 8]))] + [GRAM_BIG]
GRAM_REAL = [(33, 33), (31, 31), (256, 32), (257, 193), (769, 224), (1025, 225), (1281, 257), (1, 1), GRAM_BIG]

AFFINITY_CASES = [  # H, W, nr, nc, hx, hy: H W % 128 = 0, 1, 127; p % 4 = 0, 1, 3 (p = 8, 16; 5, 21; 7, 11)
    (16, 8, 2, 4, 3.0, 40.0), (16, 8, 4, 4, 3.5, 50.0), (3, 43, 1, 5, 8.0, 45.0), (3, 43, 3, 7, 8.0, 45.0),
    (127, 1, 7, 1, 22.0, 50.0), (127, 1, 11, 1, 25.0, 45.0)]      # max |arg| 51, 44, 47, 50, 56, 45

NYSTROM_CASES = [  # H, W, nr, nc, hx (the sample spacing), hy
    (24, 32, 6, 8, 4.0, 100.0), (31, 33, 7, 7, 4.0, 100.0), (19, 27, 5, 11, 2.5, 100.0), (23, 39, 7, 8, 3.5, 100.0),
    (9, 71, 3, 19, 3.0, 100.0), (24, 32, 7, 9, 3.0, 100.0),                                  # p = 48 .. 63: NT 2
    (15, 17, 5, 5, 3.0, 100.0), (19, 27, 4, 8, 3.5, 100.0), (16, 24, 3, 5, 4.5, 100.0), (3, 43, 1, 17, 2.5, 100.0),  # NT 1
    (16, 24, 8, 12, 2.0, 100.0), (20, 32, 10, 10, 2.5, 100.0), (23, 39, 10, 16, 2.0, 100.0), (31, 33, 12, 16, 2.0, 100.0),
    (31, 33, 14, 16, 2.0, 100.0), (25, 41, 12, 19, 2.0, 100.0), (32, 32, 16, 16, 2.0, 100.0), (29, 53, 13, 20, 2.0, 100.0)]


def _ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


@functools.lru_cache(maxsize=None)
def _plane(case):
    from conftest import load_oracle
    return Plane(load_oracle(), *case)


# ------------------------------------------------------------------ CPU: the case lists reach what they claim
def test_width_table_covers_every_instantiation():
    hit = {}
    for r, gq in WIDTHS.items():
        assert pick_gq(nle_ld(r)) == gq, (r, pick_gq(nle_ld(r)), gq)
        hit.setdefault(gq, set()).add(r % 4 == 0)
    assert sorted(hit) == sorted(ALL_GQ) and all(v == {True, False} for v in hit.values())
    nqs = {nle_ld(r) // 4 for r in WIDTHS}
    assert {32, 33, 64, 65, 128, 129, 256, 257, 512} <= nqs
    assert all(pick_gq(nle_ld(r)) is None for r in (2049, 2050, 2051, 2052)) and pick_gq(2048) == (64, 8)
    # every pair pick_gq returns anywhere is in the table
    assert {pick_gq(ld) for ld in range(4, 2049, 4)} == set(ALL_GQ)


def test_case_lists_cover_the_switches():
    for axis, col in ((GEMM_M, 0), (GEMM_KD, 1), (GEMM_NC, 2)):
        for v in axis:
            assert sum(c[col] == v for c in GEMM_CASES) >= 2, (col, v)
    for cases in (GEMM_CASES, GEMM_REAL):
        for nt in range(1, 9):   # every NT with an M tail and a kd tail in the same case
            assert any(tsgemm_nt(nle_ld(nc))[0] == nt and M % 128 and kd % 32 for M, kd, nc in cases), nt
        assert any(tsgemm_nt(nle_ld(nc)) == (5, 2) for _, _, nc in cases)
    for v in GRAM_R:
        assert sum(c[1] == v for c in GRAM_CASES) >= 2, v
    for v in GRAM_M:
        assert sum(c[0] == v for c in GRAM_CASES) >= 2, v
    assert gram_chunk_rows(GRAM_BIG[0]) == 320 and 9 * 320 < 2 ** 24 and gram_chunk_rows(1281) == 256
    assert rowpass_max_blocks() == 1024
    got32 = {tsgemm_nt(nle_ld(c[2] * c[3])) for c in NYSTROM_CASES}
    got16 = {tsgemm_nt(nle_ld(c[2] * c[3]), 7) for c in NYSTROM_CASES}
    assert got32 == {(n, 1) for n in range(1, 9)} | {(5, 2)} and got16 == {(n, 1) for n in range(1, 8)} | {(4, 2), (5, 2)}
    assert {(c[2] * c[3]) % 16 for c in NYSTROM_CASES} >= {0, 1, 7, 8, 9, 15}
    assert {(c[0] * c[1]) % 128 for c in NYSTROM_CASES} == {0, 1, 127} == {(c[0] * c[1]) % 128 for c in AFFINITY_CASES}
    assert {(c[2] * c[3]) % 4 for c in AFFINITY_CASES} == {0, 1, 3}


@pytest.mark.parametrize("case", NYSTROM_CASES, ids=_ids(NYSTROM_CASES))
def test_nystrom_cases_have_full_rank(oracle, case):
    pl = _plane(case)
    assert pl.p == case[2] * case[3], "the grid must select exactly nr x nc samples"
    lam, _ = oracle.nystrom_approximation(pl.Ka, pl.K[pl.rest].T)
    assert lam.size == pl.p, f"K_A is cut at rank {lam.size} < p = {pl.p}"
    assert lam[-1] > 1e-3, "far above the 1e-10 cut: the device's fp64 solver must keep every eigenvalue too"
    assert abs(case[4] - 0.5 * (case[0] // case[2] + case[1] // case[3])) <= 0.5, "hx is the sample spacing"


@pytest.mark.parametrize("case", AFFINITY_CASES, ids=_ids(AFFINITY_CASES))
def test_affinity_cases_keep_the_exponent_in_range(case):
    pl = _plane(case)
    assert pl.p == case[2] * case[3]
    assert pl.L.max() <= ARG_MAX * LN2, f"|arg| reaches {pl.L.max() / LN2:.1f}"
    assert pl.L.max() >= 20 * LN2, "and is not trivially small either"


# ------------------------------------------------------------------ CPU: the checkers have teeth
def _rejects(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return True
    return False


def _swap_lane_rows(C):
    """rows 1 and 8 of the first 32-row block: accumulator elements e = 1 and e = 4 of the MFMA map swapped"""
    m = C.copy()
    m[[1, 8]] = m[[8, 1]]
    return m


@pytest.mark.parametrize("M,kd,nc", [(129, 33, 65), (257, 300, 260), (40, 65, 33)])
def test_checkers_ts_gemm(M, kd, nc):
    def pad(Cm):
        return padded32(Cm.astype(np.float32))
    A, B = int_gemm_inputs(M, kd, nc)
    rng = np.random.default_rng(M + kd + nc)
    Ar, Br = positive32(rng, M, kd), positive(rng, kd, nc)
    good_i = pad((A.astype(np.float32) @ B.astype(np.float32)))          # numpy's own fp32 products pass
    good_r = pad(Ar @ Br.astype(np.float32))
    check_ts_gemm_exact(good_i, A, B)
    assert check_ts_gemm(good_r, Ar, Br) < 1.0
    for check, good, a, b in ((check_ts_gemm_exact, good_i, A, B), (check_ts_gemm, good_r, Ar, Br)):
        af, bf = a.astype(np.float64), np.asarray(b).astype(np.float32).astype(np.float64)
        m = good.copy()                                                  # one row repeated
        m[M // 2] = m[M // 2 - 1]
        assert _rejects(check, m, a, b)
        m = good.copy()                                                  # one 32-column tile shifted by 4 rows
        m[4:, 32:64] = good[:-4, 32:64]
        m[:, nc:] = 0
        assert _rejects(check, m, a, b)
        m = good.copy()                                                  # the last k term dropped from one tile
        m[0:32, 32:min(64, nc)] = (af[0:32, :kd - 1] @ bf[:kd - 1, 32:min(64, nc)]).astype(np.float32)
        assert _rejects(check, m, a, b)
        m = good.copy()                                                  # ... from one entry only
        m[M - 1, nc - 1] = np.float32(af[M - 1, :kd - 1] @ bf[:kd - 1, nc - 1])
        assert _rejects(check, m, a, b) or af[M - 1, kd - 1] * bf[kd - 1, nc - 1] == 0
        assert _rejects(check, _swap_lane_rows(good), a, b)              # two rows of the MFMA element map swapped
        m = good.copy()                                                  # the last (partial) row block not written
        m[(M - 1) // 128 * 128:] = 0
        assert _rejects(check, m, a, b)
        if nle_ld(nc) > nc:                                              # a padding column of the output non-zero
            m = good.copy()
            m[M // 3, nc] = 1e-30
            assert _rejects(check, m, a, b)


@pytest.mark.parametrize("M,r", [(600, 65), (1281, 33), (257, 40)])
def test_checkers_gram(M, r):
    rng = np.random.default_rng(M * 7 + r)
    rows = gram_chunk_rows(M)

    def chunked(Z32, skip=None):                                        # fp32 inside a chunk, fp64 across, as the device
        G = np.zeros((r, r))
        for ci, c0 in enumerate(range(0, M, rows)):
            if ci != skip:
                G += (Z32[c0:c0 + rows].T @ Z32[c0:c0 + rows]).astype(np.float64)
        return np.triu(G) + np.triu(G, 1).T

    Xi = rng.integers(0, 4, (M, r)).astype(np.int64)
    Xr, u = positive32(rng, M, r), rng.uniform(0.5, 2.0, r)
    Zr = Xr * (1.0 / (Xr.astype(np.float64) @ u)).astype(np.float32)[:, None]
    check_gram_exact(chunked(Xi.astype(np.float32)), Xi)                  # numpy's own fp32 products pass
    assert check_gram(chunked(Zr), Xr, u) < 1.0
    for check, Z, args in ((check_gram_exact, Xi.astype(np.float32), (Xi,)), (check_gram, Zr, (Xr, u))):
        good = chunked(Z)
        assert _rejects(check, chunked(Z, skip=(M - 1) // rows), *args)   # one chunk left out (the last, short one)
        assert _rejects(check, chunked(Z, skip=0), *args)
        assert _rejects(check, good - np.outer(Z[M // 2], Z[M // 2]).astype(np.float64), *args)   # one row dropped
        m = good.copy()                                                  # one off-diagonal tile shifted by 4 rows
        m[4:32, 32:r] = good[0:28, 32:r]
        m[32:r, 0:32] = m[0:32, 32:r].T
        assert _rejects(check, m, *args)
        m = good.copy()                                                  # two rows of the element map swapped in one tile
        m[[1, 8], 32:r] = good[[8, 1], 32:r]
        m[32:r, 0:32] = m[0:32, 32:r].T
        assert _rejects(check, m, *args)
        m = good.copy()                                                  # asymmetric by one ulp
        m[0, r - 1] = np.nextafter(m[0, r - 1], np.inf)
        assert _rejects(check, m, *args)
    assert _rejects(check_gram, chunked(Xr * np.sqrt(1.0 / (Xr.astype(np.float64) @ u)).astype(np.float32)[:, None]), Xr, u)


def test_checkers_row_scalings():
    rng = np.random.default_rng(5)
    X, u = rng.integers(1, 8, (300, 133)), rng.integers(1, 6, 133)
    good = 1.0 / (X @ u).astype(np.float64)
    check_row_scalings_exact(good, X, u)
    assert _rejects(check_row_scalings_exact, 1.0 / (X[:, :-1] @ u[:-1]).astype(np.float64), X, u)    # the last column dropped
    assert _rejects(check_row_scalings_exact, 1.0 / (X[:, 4:] @ u[4:]).astype(np.float64), X, u)      # the first quad dropped
    assert _rejects(check_row_scalings_exact, np.nextafter(good, 0.0), X, u)                          # one ulp off
    m = good.copy()
    m[[10, 11]] = m[[11, 10]]                                                                         # two rows swapped
    assert _rejects(check_row_scalings_exact, m, X, u)
    m = good.copy()
    m[-1] = 0.0                                                                                       # the last row not written
    assert _rejects(check_row_scalings_exact, m, X, u)


def _affinity_f32(pl):
    """affinity_value's arithmetic in numpy fp32: every operation rounded on its own"""
    f = np.float32
    nsw, npw = f(-np.log2(np.e) / (pl.hx * pl.hx)), f(-np.log2(np.e) / (pl.hy * pl.hy))
    i = np.arange(pl.H * pl.W)
    dr = (i // pl.W)[:, None].astype(f) - (pl.sel // pl.W)[None, :].astype(f)
    dc = (i % pl.W)[:, None].astype(f) - (pl.sel % pl.W)[None, :].astype(f)
    dv = pl.x.ravel()[:, None] - pl.x.ravel()[pl.sel][None, :]
    return np.exp2(nsw * (dr * dr + dc * dc) + npw * (dv * dv)).astype(f)


@pytest.mark.parametrize("case", AFFINITY_CASES[1::2], ids=_ids(AFFINITY_CASES[1::2]))
def test_checkers_affinity(case):
    pl = _plane(case)
    good = padded32(_affinity_f32(pl))
    assert check_affinity(good, pl) < 1.0                               # numpy's own fp32 evaluation passes
    assert _rejects(check_affinity, _swap_lane_rows(good), pl)          # two pixels swapped
    m = good.copy()
    m[:, [0, 1]] = m[:, [1, 0]]                                         # two samples swapped
    assert _rejects(check_affinity, m, pl)
    m = good.copy()
    m[-1] = 0.0                                                         # the last pixel not written
    assert _rejects(check_affinity, m, pl)
    m = good.copy()                                                     # one entry off by twice its bound
    m[5, 2] = np.float32(pl.K[5, 2] * (1 + 2 * e_aff(pl.L[5, 2])))
    assert _rejects(check_affinity, m, pl)
    if nle_ld(pl.p) > pl.p:
        m = good.copy()
        m[7, pl.p] = 1e-30
        assert _rejects(check_affinity, m, pl)
    H, W, nr, nc, hx, hy = case                                         # the spatial weight taken for the range weight
    assert _rejects(check_affinity, padded32(_affinity_f32(_plane((H, W, nr, nc, hy, hx)))), pl)


_CHECKED = [NYSTROM_CASES[2], NYSTROM_CASES[9], NYSTROM_CASES[14]]


@pytest.mark.parametrize("case", _CHECKED, ids=_ids(_CHECKED))
def test_checkers_nystrom(oracle, case):
    pl = _plane(case)
    p, N = pl.p, pl.H * pl.W
    lam, phi_o = oracle.nystrom_approximation(pl.Ka, pl.K[pl.rest].T)
    VA = phi_o[:p].astype(np.float32)
    B32 = (phi_o[:p] * (1.0 / lam)[None, :]).astype(np.float32)
    K32 = _affinity_f32(pl)
    good = np.zeros((N, nle_ld(p)), dtype=np.float32)
    good[pl.rest, :p] = K32[pl.rest] @ B32                              # numpy's own fp32 product of its fp32 affinities
    good[pl.sel, :p] = VA
    for split in (False, True):
        assert check_nystrom(good, lam, p, pl, split) < 1.0
    K64, B64 = K32.astype(np.float64), B32.astype(np.float64)
    i, j = pl.rest[len(pl.rest) // 2], p // 2
    s = int(np.argmax(K64[i] * np.abs(B64[:, j])))                      # the term that weighs most in entry (i, j)
    dropped = good.copy()                                               # one sample's term dropped from one entry
    dropped[i, j] = np.float32(K64[i] @ B64[:, j] - K64[i, s] * B64[s, j])
    assert _rejects(check_nystrom, dropped, lam, p, pl, True)
    m = good.copy()                                                     # the last k term dropped from a 32-row block of one tile
    rows = pl.rest[np.argsort(-K64[pl.rest, p - 1])[:32]]               # (the rows next to that sample)
    m[rows, :min(32, p)] = K32[rows, :p - 1] @ B32[:p - 1, :min(32, p)]
    assert _rejects(check_nystrom, m, lam, p, pl, True)
    m = good.copy()                                                     # two rows of the element map swapped
    m[pl.rest[[1, 8]]] = good[pl.rest[[8, 1]]]
    assert _rejects(check_nystrom, m, lam, p, pl, True)
    m = good.copy()                                                     # one row repeated
    m[pl.rest[40]] = good[pl.rest[39]]
    assert _rejects(check_nystrom, m, lam, p, pl, True)
    if p <= 64:                                                         # the mid x mid product left out: 2^-16 relative
        m = good.copy()
        m[i, j] = np.float32(np.float64(m[i, j]) + 2.0 ** -16 * (K64[i] @ np.abs(B64[:, j])))
        assert _rejects(check_nystrom, m, lam, p, pl, True)
    assert _rejects(check_nystrom, good, lam[:-1], p - 1, pl, True)     # a rank cut is refused, not compared
    _, bound = nystrom_parts(good, lam, pl)
    assert check_nystrom_pair(good, good, lam, pl, bound(True)) == 0.0
    assert _rejects(check_nystrom_pair, good, dropped, lam, pl, bound(True))


# ------------------------------------------------------------------ GPU: exact arithmetic
def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("M,kd,nc", GEMM_CASES, ids=_ids(GEMM_CASES))
def test_ts_gemm_exact(nle, ctx, M, kd, nc):
    A, B = int_gemm_inputs(M, kd, nc)
    C = ctx.ts_gemm(_dev(padded32(A)), kd, B.astype(np.float64)).cpu().numpy()
    print(f"stage32 ts_gemm exact M={M} kd={kd} nc={nc}: k_tsgemm<{tsgemm_nt(nle_ld(nc))[0]}, false> x {tsgemm_nt(nle_ld(nc))[1]} panel(s)")
    check_ts_gemm_exact(C, A, B)


@pytest.mark.gpu
@pytest.mark.parametrize("M,r", GRAM_CASES, ids=_ids(GRAM_CASES))
def test_gram_exact(nle, ctx, M, r):
    X = np.random.default_rng(31 * r + M).integers(0, 4, (M, r)).astype(np.int64)
    G = ctx.gram(_dev(padded32(X)), r, None)
    rows = gram_chunk_rows(M)
    print(f"stage32 gram exact M={M} r={r}: {(nle_ld(r) + 31) // 32} column tiles, {(M + rows - 1) // rows} chunk(s) of {rows} rows")
    check_gram_exact(G, X)


@pytest.mark.gpu
@pytest.mark.parametrize("r", sorted(WIDTHS), ids=[f"r{r}-G{WIDTHS[r][0]}-Q{WIDTHS[r][1]}" for r in sorted(WIDTHS)])
def test_row_scalings_exact(nle, ctx, r):
    G, Q = WIDTHS[r]
    rng = np.random.default_rng(r)
    X, u = rng.integers(1, 8, (1000, r)), rng.integers(1, 6, r)
    d_X = _dev(padded32(X))
    print(f"stage32 row_scalings exact r={r} ld={nle_ld(r)}: k_row_scalings<{G}, {Q}>, M in {rows_for(G)}")
    for M in rows_for(G):
        check_row_scalings_exact(ctx.row_scalings(d_X[:M], r, u.astype(np.float64)).cpu().numpy(), X[:M], u)


def _sinkhorn_rows():
    out = []
    for i, r in enumerate(sorted(WIDTHS)):
        out.append((rows_for(WIDTHS[r][0])[1:][i % 3], r))
    return out + [(rowpass_max_blocks() * 64 + 65, 4)]   # G = 4: 64 rows per workgroup; past one grid-stride round


@pytest.mark.gpu
@pytest.mark.parametrize("M,r", _sinkhorn_rows(), ids=_ids(_sinkhorn_rows()))
def test_sinkhorn_scalings_one_iteration(nle, ctx, M, r):
    G, Q = WIDTHS[r]
    rng = np.random.default_rng(13 * r + M)
    X = positive32(rng, M, r)
    lam = np.sort(rng.uniform(0.5, 2.0, r))[::-1].copy()
    uc, ur = ctx.sinkhorn_scalings(_dev(padded32(X)), r, lam, 1)
    ec, er = check_sinkhorn(uc, ur, X.astype(np.float64), lam, 1)
    print(f"stage32 sinkhorn M={M} r={r} ld={nle_ld(r)}: k_rowpass<{G}, {Q}> COLSUM + RECIP, rel L2 u_c {ec:.2e} u_r {er:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("r", [2049, 2050, 2051, 2052])
def test_widths_without_an_instantiation_are_refused(nle, ctx, r):
    import torch
    X = torch.zeros((8, nle_ld(r)), dtype=torch.float32, device="cuda")
    for call in (lambda: ctx.row_scalings(X, r, np.ones(r)), lambda: ctx.sinkhorn_scalings(X, r, np.ones(r), 1)):
        with pytest.raises(nle.NLEError) as e:
            call()
        assert e.value.code != 0
        assert (nle.lib().nle_last_error(ctx._h) or b"").decode().strip(), "nle_last_error must say what was refused"


@pytest.mark.gpu
def test_fp32_ld_contract(nle, ctx):
    """include/nle.h above nle_ts_gemm: a row stride that is no multiple of 4 is NLE_ERR_INVALID (a float4 would straddle rows)"""
    import torch
    for ldx in (5, 6, 7, 9):
        X = torch.ones((8, ldx), dtype=torch.float32, device="cuda")
        for call in (lambda: ctx.ts_gemm(X, 5, np.ones((5, 3))), lambda: ctx.row_scalings(X, 5, np.ones(5)),
                     lambda: ctx.gram(X, 5, np.ones(5)), lambda: ctx.gram(X, 5, None),
                     lambda: ctx.sinkhorn_scalings(X, 5, np.ones(5), 1)):
            with pytest.raises(nle.NLEError) as e:
                call()
            assert e.value.code == nle.NLE_ERR_INVALID
    # ld % 4 == 0 with zero padding is the contract: the same calls go through
    X = _dev(padded32(np.ones((8, 5)), 8))
    assert np.array_equal(ctx.row_scalings(X, 5, np.ones(5)).cpu().numpy(), np.full(8, 0.2))
    assert np.array_equal(ctx.gram(X, 5, None), np.full((5, 5), 8.0))


# ------------------------------------------------------------------ GPU: real data, derived bounds
@pytest.mark.gpu
@pytest.mark.parametrize("M,kd,nc", GEMM_REAL, ids=_ids(GEMM_REAL))
def test_ts_gemm_elementwise(nle, ctx, M, kd, nc):
    rng = np.random.default_rng(1000 * kd + nc + M)
    A, B = positive32(rng, M, kd), positive(rng, kd, nc)
    worst = check_ts_gemm(ctx.ts_gemm(_dev(padded32(A)), kd, B).cpu().numpy(), A, B)
    print(f"stage32 ts_gemm M={M} kd={kd} nc={nc}: k_tsgemm<{tsgemm_nt(nle_ld(nc))[0]}, false>, max err/bound {worst:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("M,r", GRAM_REAL, ids=_ids(GRAM_REAL))
def test_gram_elementwise(nle, ctx, M, r):
    rng = np.random.default_rng(31 * r + M)
    X, u = positive32(rng, M, r), rng.uniform(0.5, 2.0, r)
    worst = check_gram(ctx.gram(_dev(padded32(X)), r, u), X, u)
    print(f"stage32 gram M={M} r={r}: chunks of {gram_chunk_rows(M)} rows, max err/bound {worst:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", AFFINITY_CASES, ids=_ids(AFFINITY_CASES))
def test_affinity_elementwise(nle, ctx, case):
    pl = _plane(case)
    Ka, kab = ctx.compute_kernel(pl.x, pl.nr, pl.nc, pl.hx, pl.hy)
    worst = check_affinity(kab.cpu().numpy(), pl)
    print(f"stage32 affinity {pl.H}x{pl.W} p={pl.p} |arg| <= {pl.L.max() / LN2:.1f}: k_affinity, max err/bound {worst:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", NYSTROM_CASES, ids=_ids(NYSTROM_CASES))
def test_nystrom_gemms_elementwise(nle, ctx, case):
    pl = _plane(case)
    lam0, phi0, r0 = ctx.nystrom(pl.x, pl.nr, pl.nc, pl.hx, pl.hy)
    ctx.set_nystrom_bf16x3(True)
    try:
        lam3, phi3, r3 = ctx.nystrom(pl.x, pl.nr, pl.nc, pl.hx, pl.hy)
    finally:
        ctx.set_nystrom_bf16x3(False)
    phi0, phi3 = phi0.cpu().numpy(), phi3.cpu().numpy()
    assert r0 == r3 == pl.p and np.array_equal(lam0, lam3)
    parts = nystrom_parts(phi0, lam0, pl)
    w0 = check_nystrom(phi0, lam0, r0, pl, False, parts)
    wp = check_nystrom_pair(phi0, phi3, lam0, pl, parts[1](True))      # (phi3's sample rows, hence its B, are phi0's)
    w3 = check_nystrom(phi3, lam3, r3, pl, True, parts)
    ld = nle_ld(pl.p)
    print(f"stage32 nystrom {pl.H}x{pl.W} (N % 128 = {pl.H * pl.W % 128}) p={pl.p} (p % 16 = {pl.p % 16}): "
          f"k_tsgemm<{tsgemm_nt(ld)[0]}, true> x {tsgemm_nt(ld)[1]} max err/bound {w0:.3g}; "
          f"k_tsgemm_bf16x3<{tsgemm_nt(ld, 7)[0]}> x {tsgemm_nt(ld, 7)[1]} max err/bound {w3:.3g}; between them {wp:.3g}")
