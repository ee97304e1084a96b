"""The sample-space kernels of csrc/fused.hip, each ALONE and entry by entry: k_sink_pass<PP> + k_reduce_partials
(nle_sample_pass), k_gram64<TPW> + k_gram64_reduce (nle_sample_gram), k_project64<NT> and k_project64_res<NT, 16, REM>
(nle_sample_project), k_sink_update_a/b (nle_sample_update).  What tests/test_stage32.py is for csrc/kernels.hip.  Every entry
point calls only the launcher the trains call (sink_pass, gram64, project64, sink_update).

1. EXACT ARITHMETIC: no tolerance.  hx = 1e30: nsw = fp32(-log2(e) / hx^2) is -0, the spatial term is exactly -0.  hy = 0.05 on
an integer plane: npw = -577.08, the argument is -0 for equal levels and <= -577 otherwise, v_exp_f32 returns exactly 1 or
exactly 0 (2^-577 is far below the smallest fp32 denormal): k(i, s) = [lum_i == lum_s].  The sample pixels carry chosen levels
(`Levels`): distinct 0 .. p - 1 for the pass and the projection; s % ceil(p / 3) for the Gram, so that two or three samples
-- in different 16 x 16 tiles once p > 48 -- share a level and the off-diagonal tiles are not all zero.  The other pixels:
a skewed draw over those levels and three levels beyond them that match no sample.  With small integers the device must EQUAL
    projection  V[i, k] = c_i sum_{s: lev_s = lev_i} D[s, k], c in 1..7, D in -3..3: |V| <= 63 < 2^24; columns K .. ldv - 1
                exactly 0; the output is pre-filled with NaN, so an element that is never written shows
    Gram        G[a, b] = sum_{i not a sample} c_i^2 [lev_i = lev_a] [lev_i = lev_b] (<= 49 M < 2^53), G == G^T; c is NaN at
                the sample pixels: never read
    pass        column sum: z_s = number of non-sample pixels at the level of sample s (every fp32 partial sum is an integer
                <= 64), y = 1 at non-sample pixels and 0 at sample pixels.  Reciprocal: w_s a power of two (a level class
                is one sample, its sum w_s): d_i = w_s exactly, y_i = 1 / w_s, (float)y_i and k y_i exact, the fold adds <= 64
                equal powers of two: z_s = count_s / w_s exactly; y_i = 0 at the unmatched levels (d = 0 < eps) and at
                sample pixels.  w = 0: y = 0 and z = 0 everywhere
    update      X1, X2, z, lam small integers, s_A in {0.5, 1, 2, 4} and the entries 0 and 1e-20, whose y_A must be 0: v, u,
                s_A' and w' are multiples of 1/4 far below 2^53, exact in any order.  chol = 0 and chol = 1 (r = p, the lower
                half of X1 zero), column sum and reciprocal

2. REAL DATA: derived elementwise bounds.  Planes as test_stage32.py's affinity cases (uniform fp32 luminances, |arg| <= 60
held on the CPU for every plane); c, w, D = (|N(0,1)| + 0.1) / sqrt(width), D signed.  References in np.longdouble from the
oracle's fp64 affinity K_ref.  u32 = 2^-24, u64 = 2^-53, g_t(k) = k u_t / (1 - k u_t) (Higham, section 3.1).  One fp32
affinity (test_stage32.py: 6 roundings of the argument, v_exp_f32 at 1 ULP): |k - K_ref| <= e_aff K_ref, plus stage32's flush
term 2^-125 where K_ref < 2^-126 =: dK;  Kp = K_ref + dK.
    projection  (double)k is exact; the fp64 MFMA adds the p terms of an entry in a chain (one rounding per term; the REM
                columns: four chains and two shuffles), the product with c_i is one more: <= p + 2 roundings per term.  The
                result is rounded to fp32 once:
                    b0 = |c_i| sum_s [dK + g64(p + 2) Kp](i, s) |D(s, k)|,   |V - ref| <= b0 + u32 (|ref| + b0)
    Gram        z_ia = c_i (double)k_ia: one fp64 rounding each; the MFMA adds the rows of a chunk (chunk_rows roundings), the
                chunk sums are added in fp64 by k_gram64_reduce (<= nchunks): <= chunk_rows + nchunks + 4 per term:
                    |G - ref| <= (1 + g64(chunk_rows + nchunks + 4)) Kp^T diag(c^2) Kp - K_ref^T diag(c^2) K_ref
                (per term (1 + e_aff(i, a)) (1 + e_aff(i, b)) (1 + g64) - 1 on c_i^2 K_ia K_ib, written for absolute dK)
    pass        d_i = sum_s (double)k_is w_s in fp64, four chains: <= p + 3 roundings per term, all terms positive:
                |d - d_ref| <= (1 + g64(p + 3)) (Kp w) - K_ref w =: dd, rho = dd / d_ref, y = fl(1 / d):
                    |y - y_ref| <= ey y_ref,   ey = (1 + rho / (1 - rho)) (1 + u64) - 1     (column sum: y = 1, ey = 0)
                then yf = (float)y (u32), k yf in fp32 (u32), the six-level fp32 fold (g32(6)), then fp64: the tiles of a
                wave, the 4 waves of a block, the blocks of a slice (k_reduce_partials: 8 chains and their sum), 8 slices:
                n64 = tiles per wave + 2 + ceil(blocks per slice / 8) + 8 + 8 roundings:
                    |z - z_ref| <= (1 + u32)^2 (1 + g32(6)) (1 + g64(n64)) Kp^T (y_ref (1 + ey)) - K_ref^T y_ref
    update      plain fp64 dots.  v = [sum of the zrows slices; y_A]: g64(zrows) |z| and u64 |y_A|.  u_k = lam_k X1[:, k] . v:
                du = g64(2 p + zrows + 2) |lam_k| |X1[:, k]| . |v|.  w' and s_A' are dots of length r with u (or y_A, exact
                K_A form): |X2| du + g64(r + 2) |X2| (|u| + du)   (adding a zero is exact: a term meets at most r - 1
                inexact additions, its product, and the y_A or z term of the Cholesky form)
Every case prints its largest err / bound; the printed values are recorded in profiles/r20_sample_space_edges.txt.

3. DISPATCH.  sink_pp, gram64_form, gram64_chunk_rows, project64_form below mirror fused.hip; test_mirrors_* hold them to the
source text and test_case_tables_* hold the case tables to them: every one of the 16 + 6 (+ the two-group launch) + 28
instantiations is named by a case.  "The realised p (nle.sample_grid) is the intended p" is a condition of every plane
(test_planes_realise_the_intended_p).  The 513 x 512, 363 x 362, 128 x 128 and 129 x 128 planes (a second grid-stride round of
the pass, a second round of the projection's persistent loop, gram64_chunk_rows 32 | 64) run in exact arithmetic only: |arg| <= 60
cannot be held on a plane that wide, and an index error shows in exact arithmetic.

4. The checkers are plain functions of (result, inputs).  test_checkers_* (no GPU) feed them numpy's own evaluation in the
kernel's precision, which must pass, and what a wrong map would produce, each of which must fail: one 16-column tile of V
taken from the pixel 16 rows on, a remainder column left at the sentinel, the last sample dropped from one tile's contraction,
one 64-pixel tile left out of z, z[s] and z[s ^ 32] exchanged (a wrong fold level), a Gram tile of the second group replaced by
tile 0, one Gram chunk left out, y_A taken from the wrong half of v in the update.
"""
import functools
import os
import re

import numpy as np
import pytest

from test_stage32 import LD, U32, U64, LN2, ARG_MAX, Plane, _affinity_f32, _rejects, _worst, e_aff, g32, g64, nle_ld, positive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-10   # NLE_EPS
HX_EXACT, HY_EXACT = 1e30, 0.05


def fused_source():
    with open(os.path.join(ROOT, "nonlocal-image-edit_amd", "csrc", "fused.hip")) as f:
        return f.read()


# ------------------------------------------------------------------ mirrors of the dispatch in csrc/fused.hip
def sink_pp(p):
    return (p + 15) & ~15


def sink_nj(p):
    return (p + 63) // 64


def sink_pass_ld(p):
    return (p + 63) & ~63


def sink_grid(M):
    return min(max(((M + 63) // 64 + 3) // 4, 1), 1024)


def sink_n64(M):
    """fp64 roundings a term of z can meet after the fp32 fold (module docstring)"""
    grid = sink_grid(M)
    tiles_per_wave = -(-((M + 63) // 64) // (grid * 4))
    return tiles_per_wave + 2 + -(-(-(-grid // 8)) // 8) + 8 + 8


GRAM_TPW = (4, 8, 12, 16, 20, 23)


def gram64_form(p):
    """(TPW, groups, ldz, ntiles) of gram64"""
    ld16 = (p + 15) & ~15
    nt = ld16 // 16
    ntiles = nt * (nt + 1) // 2
    tpw = next((t for t in GRAM_TPW if 4 * t >= ntiles), GRAM_TPW[-1])
    return tpw, -(-ntiles // (4 * tpw)), ld16 + (0 if ld16 % 32 == 16 else 16), ntiles


def gram64_chunk_rows(M):
    return max(-(-(-(-M // 512)) // 32) * 32, 32)


def gram64_chunks(M):
    return -(-M // gram64_chunk_rows(M))


def project64_res_ldb(nt, rem):
    ldb = (nt * 16 + rem + 15) // 16 * 16
    return ldb + 16 if ldb % 32 == 0 else ldb


def project64_form(K, p):
    """(resident?, NT, REM, LDB) of project64"""
    nt_r, rem = K // 16, K % 16
    if rem > 4 or nt_r == 0:
        nt_r, rem = (K + 15) // 16, 0
    p4 = (p + 3) & ~3
    if nt_r <= 4 and p4 * project64_res_ldb(nt_r, rem) * 8 + p4 * 16 <= 150 * 1024:
        return True, nt_r, rem, project64_res_ldb(nt_r, rem)
    nt = (K + 15) // 16
    return False, nt, 0, nt * 16 + (0 if nt & 1 else 16)


ALL_PP = list(range(16, 257, 16))
ALL_PROJECT = [(True, nt, rem) for nt in range(1, 5) for rem in range(5)] + [(False, nt, 0) for nt in range(1, 9)]

# ------------------------------------------------------------------ case tables: a plane is (H, W, nr, nc), realised p = the key
PASS_PLANES = {15: (9, 15, 3, 5), 16: (8, 8, 4, 4), 17: (5, 51, 1, 17), 48: (13, 25, 6, 8), 64: (16, 17, 8, 8), 65: (11, 41, 5, 13),
               80: (17, 31, 8, 10), 96: (17, 25, 8, 12), 112: (17, 29, 8, 14), 128: (17, 49, 8, 16), 129: (9, 43, 3, 43),
               144: (24, 25, 12, 12), 160: (21, 33, 10, 16), 176: (23, 33, 11, 16), 192: (25, 33, 12, 16), 193: (3, 193, 1, 193),
               208: (27, 33, 13, 16), 224: (29, 33, 14, 16), 240: (31, 33, 15, 16), 255: (31, 35, 15, 17), 256: (33, 33, 16, 16)}
# (plane, rows or None): M < 64, every pixel a sample (M = 16), M % 64 = 1 on a slab from row 0, a slab with row0 > 0
PASS_M = [((9, 4, 4, 4), None), ((4, 4, 4, 4), None), ((12, 13, 4, 4), (0, 5)), ((12, 13, 4, 4), (3, 9))]
PASS_BIG = ((513, 512, 4, 4), None)       # 262 656 pixels > 1024 * 4 * 64: a second grid-stride round
PASS_CASES = [(pl, None) for pl in PASS_PLANES.values()] + PASS_M
PASS_REFUSED = (32, 34, 16, 17)           # p = 272

GRAM_PLANES = {16: (9, 9, 4, 4), 80: (17, 31, 8, 10), 81: (19, 27, 9, 9), 112: (17, 29, 8, 14), 113: (3, 113, 1, 113),
               144: (24, 25, 12, 12), 145: (11, 59, 5, 29), 160: (21, 33, 10, 16), 161: (15, 47, 7, 23), 192: (25, 33, 12, 16),
               193: (3, 193, 1, 193), 208: (27, 33, 13, 16), 209: (23, 39, 11, 19), 256: (33, 33, 16, 16)}
GRAM_M = [((9, 9, 4, 4), (2, 5)), ((24, 25, 12, 12), (5, 20))]       # M = 27 < 32 with row0 > 0; M = 375, row0 > 0
GRAM_BIG = [((128, 128, 4, 4), None), ((129, 128, 4, 4), None)]       # chunk_rows 32 | 64
GRAM_CASES = [(pl, None) for pl in GRAM_PLANES.values()] + GRAM_M

# moderate p, N = 512, 513, 511: N % 512 and N % 128 are both 0, 1 and -1
MODERATE = [(16, 32, 5, 6), (27, 19, 5, 6), (7, 73, 7, 4)]             # p = 30, 30, 28
PROJECT_K = [1, 16, 17, 18, 19, 20, 21, 32, 33, 34, 35, 36, 37, 48, 49, 50, 51, 52, 53, 64, 65, 66, 67, 68, 69, 80, 96, 112, 128]
P232, P233, P400, P1152 = (17, 29, 8, 29), (3, 233, 1, 233), (41, 20, 20, 20), (65, 36, 32, 36)
# (K, plane, rows or None)
PROJECT_CASES = [(K, MODERATE[i % 3], None) for i, K in enumerate(PROJECT_K)] + [
    (18, MODERATE[2], None), (19, MODERATE[0], None), (80, MODERATE[0], None), (96, MODERATE[1], None),
    (64, P232, None), (64, P233, None), (48, P400, None), (32, P400, None), (16, P1152, None),
    (17, (9, 15, 3, 5), (4, 5)), (50, MODERATE[0], (3, 11)), (69, MODERATE[1], (20, 27))]      # M = 15 < 16; slabs with row0 > 0
PROJECT_BIG = (17, (363, 362, 4, 4), None)   # 131 406 pixels > 256 * 512: a second round of the persistent loop
PROJECT_REFUSED_K = 129

# (p, r, chol, zrows)
UPDATE_CASES = [(1, 1, 0, 1), (1, 1, 1, 8), (31, 3, 0, 8), (31, 31, 1, 1), (32, 4, 0, 1), (32, 32, 1, 8), (33, 5, 0, 8), (33, 33, 1, 1), (33, 33, 0, 8),
                (63, 1, 0, 8), (63, 63, 1, 1), (64, 63, 0, 1), (64, 64, 1, 8), (65, 64, 0, 8), (65, 65, 1, 1), (576, 128, 0, 1),
                (576, 129, 0, 8), (576, 576, 1, 1), (1152, 65, 0, 8), (1152, 1152, 1, 1)]


def zld_of(p):
    return sink_pass_ld(p + 1)   # sink_pass_ld(p) where that is > p, one more 64 where p % 64 == 0


def _id(case):
    return "-".join("x".join(str(v) for v in c) if isinstance(c, tuple) else str(c) for c in case)


def _ids(cases):
    return [_id(c) for c in cases]


# ------------------------------------------------------------------ planes
class Levels:
    """an integer plane whose samples carry chosen levels: k(i, s) = [x_i == lev_s] under HX_EXACT, HY_EXACT"""

    def __init__(self, oracle, H, W, nr, nc, shared):
        self.H, self.W, self.nr, self.nc = H, W, nr, nc
        self.sel, _ = oracle.sample_pixels(H, W, nr, nc)
        p = self.p = self.sel.size
        rng = np.random.default_rng(7919 * H + 31 * W + nr + 2 * int(shared))
        self.lev = np.arange(p) % max(1, (p + 2) // 3) if shared else np.arange(p)
        nlev = int(self.lev.max()) + 1
        x = np.minimum((rng.random(H * W) ** 2 * (nlev + 3)).astype(np.int64), nlev + 2)   # skewed; nlev .. nlev + 2 match no sample
        x[self.sel] = self.lev
        ns = np.ones(H * W, dtype=bool)
        ns[self.sel] = False
        x[np.flatnonzero(ns)[1:7:2]] = nlev + np.arange(len(np.flatnonzero(ns)[1:7:2]))                  # ... and do occur
        self.xi = x
        self.x = x.reshape(H, W).astype(np.float32)
        self.ns = np.ones(H * W, dtype=bool)
        self.ns[self.sel] = False
        self.hx, self.hy = HX_EXACT, HY_EXACT

    def slab(self, rows):
        """(K, dK, ns) of the local pixels: the exact affinities as float64 and no error"""
        r0, r1 = rows or (0, self.H)
        sl = slice(r0 * self.W, r1 * self.W)
        return (self.xi[sl, None] == self.lev[None, :]).astype(np.float64), None, self.ns[sl]


class Real(Plane):
    """test_stage32.py's plane with bandwidths that keep |arg| <= 60: the spatial term <= 14, the range term <= 23"""

    def __init__(self, oracle, H, W, nr, nc):
        hx = max(np.sqrt(((H - 1) ** 2 + (W - 1) ** 2) / 14.0), 1.0)
        super().__init__(oracle, H, W, nr, nc, float(hx), 45.0)
        self.ns = np.ones(H * W, dtype=bool)
        self.ns[self.sel] = False

    def slab(self, rows):
        r0, r1 = rows or (0, self.H)
        sl = slice(r0 * self.W, r1 * self.W)
        K, L = self.K[sl], self.L[sl]
        return K, K * e_aff(np.minimum(L, 1100.0)) + np.where(K < 2.0 ** -126, 2.0 ** -125, 0.0), self.ns[sl]


@functools.lru_cache(maxsize=None)
def _levels(plane, shared=False):
    from conftest import load_oracle
    return Levels(load_oracle(), *plane, shared)


@functools.lru_cache(maxsize=8)
def _real(plane):
    from conftest import load_oracle
    return Real(load_oracle(), *plane)


def _M(plane, rows):
    return ((rows[1] - rows[0]) if rows else plane[0]) * plane[1]


def pass_inputs(pl, exact):
    if exact:
        return 2.0 ** ((np.arange(pl.p) * 5 % 7) - 3)            # powers of two 1/8 .. 8
    return positive(np.random.default_rng(pl.p), 1, pl.p)[0]


def pixel_scalings(pl, rows, exact, nan_at_samples=False):
    M = _M((pl.H, pl.W), rows)
    rng = np.random.default_rng(M + 3 * pl.p)
    c = rng.integers(1, 8, M).astype(np.float64) if exact else positive(rng, M, 1)[:, 0]
    if nan_at_samples:
        c[~pl.slab(rows)[2]] = np.nan
    return c


def project_inputs(pl, K, exact):
    rng = np.random.default_rng(1000 * K + pl.p)
    if exact:
        return rng.integers(-3, 4, (pl.p, K)).astype(np.float64)
    return positive(rng, pl.p, K) * rng.choice([-1.0, 1.0], (pl.p, K))


def update_inputs(p, r, chol, zrows, exact, recip):
    rng = np.random.default_rng(100003 * p + 101 * r + 7 * zrows + chol)
    zld = zld_of(p)
    if exact:
        X1, X2 = (rng.integers(-3, 4, (2 * p, r)).astype(np.float64) for _ in range(2))
        lam, z = rng.integers(1, 4, r).astype(np.float64), rng.integers(0, 6, (zrows, zld)).astype(np.float64)
        sA = rng.choice([0.5, 1.0, 2.0, 4.0], p)
        sA[::7], sA[3::11] = 0.0, 1e-20                            # below eps: y_A = 0
    else:
        X1, X2 = (positive(rng, 2 * p, r) * rng.choice([-1.0, 1.0], (2 * p, r)) for _ in range(2))
        lam, z, sA = rng.uniform(0.5, 2.0, r), positive(rng, zrows, zld), rng.uniform(0.5, 2.0, p)
    if chol:
        X1[p:] = 0.0
    return X1, X2, lam, z, (sA if recip else None)


# ------------------------------------------------------------------ checkers
def _first(bad, what, extra=lambda b: ""):
    assert bad.size == 0, f"{len(bad)} {what}; first at {bad[0].tolist()}{extra(bad[0])}"


def check_project(V, K, dK, c, D):
    """V: M x nle_ld(Kc) device result of diag(c) K D; dK None: exact arithmetic.  Returns max err / bound"""
    V, (M, p), Kc = np.asarray(V), K.shape, D.shape[1]
    form = project64_form(Kc, p)
    assert V.shape == (M, nle_ld(Kc)), (V.shape, M, Kc)
    _first(np.argwhere(~(V[:, Kc:] == 0)), f"padding entries of V (columns {Kc} .. {nle_ld(Kc) - 1}) are not exactly zero {form}",
           lambda b: f": {V[:, Kc:][tuple(b)]}")
    _first(np.argwhere(~np.isfinite(V)), f"entries of V are not finite (never written?) {form}")
    if dK is None:
        ref = c[:, None] * (K @ D)
        assert np.abs(ref).max() < 2 ** 24
        _first(np.argwhere(V[:, :Kc] != ref), f"entries differ from c_i sum_s [lev] D {form}",
               lambda b: f": column tile {b[1] // 16}, row in 512-block {b[0] % 512}, got {V[tuple(b)]} want {ref[tuple(b)]}")
        return 0.0
    Kl, Dl, cl = K.astype(LD), D.astype(LD), c.astype(LD)
    ref = cl[:, None] * (Kl @ Dl)
    b0 = np.abs(cl)[:, None] * ((dK.astype(LD) + g64(p + 2) * (Kl + dK)) @ np.abs(Dl))
    worst, first = _worst(np.abs(V[:, :Kc].astype(LD) - ref), b0 + U32 * (np.abs(ref) + b0))
    assert first is None, f"V beyond the bound {form}; first (pixel, column) {first}, max err/bound {worst:.3g}"
    return worst


def check_gram(G, K, dK, c, ns):
    """G: p x p device result of sum over ns of c_i^2 k_i k_i^T (c may be NaN where ~ns).  Returns max err / bound"""
    G, (M, p) = np.asarray(G), K.shape
    assert G.shape == (p, p) and np.isfinite(G).all(), "G must be finite: c at a sample pixel must not be read"
    assert np.array_equal(G, G.T), "G must be exactly symmetric"
    c2 = np.where(ns, c, 0.0) ** 2
    if dK is None:
        ref = K.T @ (c2[:, None] * K)
        _first(np.argwhere(G != ref), f"entries differ from the integer Gram {gram64_form(p)}",
               lambda b: f" (tile {(b // 16).tolist()}): got {G[tuple(b)]} want {ref[tuple(b)]}")
        return 0.0
    Kl, Kp, cl = K.astype(LD), K.astype(LD) + dK, c2.astype(LD)
    ref = Kl.T @ (cl[:, None] * Kl)
    n = gram64_chunk_rows(M) + gram64_chunks(M) + 4
    worst, first = _worst(np.abs(G.astype(LD) - ref), (1 + g64(n)) * (Kp.T @ (cl[:, None] * Kp)) - ref)
    assert first is None, f"G beyond the bound {gram64_form(p)}; first {first}, max err/bound {worst:.3g}"
    return worst


def pass_reference(K, w, ns, recip, dtype=np.float64):
    Kl = K.astype(dtype)
    d = Kl @ w.astype(dtype)
    y = np.ones(K.shape[0], dtype=dtype)
    if recip:
        y = np.where(np.abs(d) >= EPS, 1 / np.where(d != 0, d, 1), 0)
    y = np.where(ns, y, 0)
    return d, y, Kl.T @ y


def check_pass(z, y, K, dK, w, ns, recip):
    """z (p), y (M): device result of one half-iteration with the sample-side vector w.  Returns max err / bound of (z, y)"""
    z, y, (M, p) = np.asarray(z), np.asarray(y), K.shape
    assert z.shape == (p,) and y.shape == (M,) and np.isfinite(z).all() and np.isfinite(y).all()
    assert np.all(y[~ns] == 0), "y must be exactly 0 at the sample pixels"
    if dK is None:
        _, yref, zref = pass_reference(K, w, ns, recip)
        _first(np.argwhere(y != yref), "entries of y differ", lambda b: f" (lane {b[0] % 64} of tile {b[0] // 64})")
        _first(np.argwhere(z != zref), f"entries of z differ (PP = {sink_pp(p)})", lambda b: f": got {z[tuple(b)]} want {zref[tuple(b)]}")
        return 0.0, 0.0
    d, yref, zref = pass_reference(K, w, ns, recip, LD)
    Kp, ey = K.astype(LD) + dK, np.zeros(M, dtype=LD)
    if recip:
        assert (d[ns] > 100 * EPS).all(), "the test data keep d above eps"
        rho = ((1 + g64(p + 3)) * (Kp @ w.astype(LD)) - d) / d
        ey = (1 + rho / (1 - rho)) * (1 + U64) - 1
    wy, first = _worst(np.abs(y.astype(LD) - yref), ey * yref)
    assert first is None, f"y beyond the bound; first pixel {first}, max err/bound {wy:.3g}"
    F = (1 + U32) ** 2 * (1 + g32(6)) * (1 + g64(sink_n64(M)))
    wz, first = _worst(np.abs(z.astype(LD) - zref), F * (Kp.T @ (yref * (1 + ey))) - zref)
    assert first is None, f"z beyond the bound (PP = {sink_pp(p)}); first sample {first}, max err/bound {wz:.3g}"
    return wz, wy


def update_reference(X1, X2, lam, z, sA, chol, dtype=np.float64, wrong_half=False):
    p = X1.shape[0] // 2
    X1, X2, lam, z = (a.astype(dtype) for a in (X1, X2, lam, z))
    t = np.zeros(p, dtype=dtype)
    for q in range(z.shape[0]):
        t = t + z[q, :p]
    ya = np.ones(p, dtype=dtype)
    if sA is not None:
        s = sA.astype(dtype)
        ya = np.where(np.abs(s) >= EPS, 1 / np.where(s != 0, s, 1), 0)
    v = np.concatenate([t, ya])
    u = lam * (X1.T @ v)
    yb = t if wrong_half else ya                               # (the mutation of test_checkers_update)
    if chol:
        return v, u, t + X2[p:] @ yb, X2[:p] @ u + yb
    return v, u, X2[p:] @ u, X2[:p] @ u


def check_update(res, X1, X2, lam, z, sA, chol, exact):
    """res = (v, u, sA_next, w_next) of the device.  Returns max err / bound of (v; u, sA_next and w_next): y_A is one correctly
    rounded division, whose error can be all of its bound u64 |y_A|"""
    p, r = X1.shape[0] // 2, X1.shape[1]
    names = ("v", "u", "sA_next", "w_next")
    assert [np.asarray(a).shape for a in res] == [(2 * p,), (r,), (p,), (p,)] and all(np.isfinite(a).all() for a in res)
    if exact:
        for name, got, want in zip(names, res, update_reference(X1, X2, lam, z, sA, chol)):
            _first(np.argwhere(got != want), f"entries of {name} differ (p = {p}, r = {r}, chol = {chol})")
        if sA is not None:
            assert np.all(res[0][p:][np.abs(sA) < EPS] == 0), "y_A must be 0 where |s_A| < eps"
        return 0.0, 0.0
    ref = update_reference(X1, X2, lam, z, sA, chol, LD)
    A1, A2, zrows = np.abs(X1).astype(LD), np.abs(X2).astype(LD), z.shape[0]
    vmag = np.concatenate([np.abs(z[:, :p]).sum(axis=0), np.abs(ref[0][p:])]).astype(LD)
    dv = np.concatenate([g64(zrows) * vmag[:p], U64 * vmag[p:]])
    du = g64(2 * p + zrows + 2) * np.abs(lam) * (A1.T @ (vmag + dv)) + np.abs(lam) * (A1.T @ dv)
    umag = np.abs(ref[1]) + du
    if chol:
        ymag = vmag[p:] + dv[p:]
        ds = dv[:p] + A2[p:] @ dv[p:] + g64(r + 2) * (vmag[:p] + dv[:p] + A2[p:] @ ymag)
        dw = A2[:p] @ du + dv[p:] + g64(r + 2) * (A2[:p] @ umag + ymag)
    else:
        ds, dw = A2[p:] @ du + g64(r + 2) * (A2[p:] @ umag), A2[:p] @ du + g64(r + 2) * (A2[:p] @ umag)
    worst = []
    for name, got, want, bound in zip(names, res, ref, (dv, du, ds, dw)):
        wst, first = _worst(np.abs(np.asarray(got).astype(LD) - want), bound)
        assert first is None, f"{name} beyond the bound (p = {p}, r = {r}, chol = {chol}); first {first}, max err/bound {wst:.3g}"
        worst.append(wst)
    return worst[0], max(worst[1:])


# ------------------------------------------------------------------ CPU: the mirrors are the source's, the tables reach every instantiation
def test_mirrors_match_the_source():
    src = fused_source()
    def listed(pattern):
        """the values of the one dispatch_values<...> / dispatch_columns<LO, HI> of the source that selects on `pattern`"""
        (form, args), = re.findall(r"dispatch_(values|columns)<([^<>]*)>\(%s," % pattern, src)
        vals = [a.strip() for a in args.split(",")]
        return vals if form == "values" else [str(v) for v in range(int(vals[0]), int(vals[1]) + 1)]
    assert [int(v) for v in listed("pp")] == ALL_PP
    assert "const int pp = (p + 15) & ~15;" in src and "constexpr int P64 = (PP + 63) & ~63;" in src and "constexpr int NJ = P64 / 64;" in src
    assert "int sink_pass_ld(int p) { return (p + 63) & ~63; }" in src and "if (g > 1024) g = 1024;" in src
    assert all(sink_nj(p) == ((sink_pp(p) + 63) & ~63) // 64 for p in range(1, 257))
    assert "static const int kTpw[6] = {4, 8, 12, 16, 20, kG64TilesPerWave};" in src
    with open(os.path.join(ROOT, "nonlocal-image-edit_amd", "csrc", "kernels.h")) as f:
        assert "constexpr int kG64TilesPerWave = 23;" in f.read()
    assert listed("tpw") == [str(v) for v in GRAM_TPW[:-1]] + ["kG64TilesPerWave"] and "k_gram64<decltype(t)::value>" in src
    assert "const int ldz = ld16 + ((ld16 % 32 == 16) ? 0 : 16);" in src and "constexpr int kG64Rows = 32;" in src
    assert "long long fl = (M + 511) / 512;" in src and "if (p > 256) return hipErrorInvalidValue;" in src
    assert [(True, int(a), int(b)) for a in listed("nt_r") for b in listed("rem")] == ALL_PROJECT[:20]
    assert [(False, int(a), 0) for a in listed("nt")] == ALL_PROJECT[20:] and "k_project64<decltype(ntv)::value>" in src
    assert "if (nt_r <= 4 && shm <= 150 * 1024) {" in src and "if (rem > 4 || nt_r == 0) {" in src
    assert "const unsigned grid = (unsigned)std::min<long long>(ntiles, 256);" in src
    assert "k_project64_res<decltype(ntv)::value, NW, decltype(remv)::value>" in src and "constexpr int NW = 16;" in src and \
        "const long long ntiles = (M + NW * 32 - 1) / (NW * 32);" in src and \
"constexpr int LDB = NT * 16 + ((NT & 1) ? 0 : 16);" in src
    for nt, rem in ((1, 0), (2, 0), (2, 3), (3, 4), (4, 0), (4, 4)):   # == 16 (mod 32) doubles, the smallest that holds the row
        ldb = project64_res_ldb(nt, rem)
        assert ldb % 32 == 16 and ldb >= nt * 16 + rem and ldb - 32 < nt * 16 + rem


def test_case_tables_cover_every_instantiation():
    assert {sink_pp(p) for p in PASS_PLANES} == set(ALL_PP), "every k_sink_pass<PP> is named by a case"
    assert {15, 16, 17, 64, 65, 80, 112, 128, 129, 144, 160, 176, 192, 193, 224, 240, 255, 256} <= set(PASS_PLANES)
    assert {(sink_nj(a), sink_nj(a + 1)) for a in (64, 128, 192)} == {(1, 2), (2, 3), (3, 4)} and {p % 16 for p in PASS_PLANES} >= {0, 1, 15}
    Ms = [_M(pl, rows) for pl, rows in PASS_CASES]
    assert {0, 1, 63} <= {M % 64 for M in Ms if M >= 64} and any(M < 64 for M in Ms) and any(rows and rows[0] > 0 for _, rows in PASS_M)
    assert _M(*PASS_BIG) > 1024 * 4 * 64 and sink_grid(_M(*PASS_BIG)) == 1024
    forms = {p: gram64_form(p) for p in GRAM_PLANES}
    assert [forms[p][0] for p in (16, 80, 81, 112, 113, 144, 145, 160, 161, 192, 193, 208, 209, 256)] == [4, 4, 8, 8, 12, 12, 16, 16, 20, 20, 23, 23, 23, 23]
    assert [forms[p][1] for p in (208, 209, 256)] == [1, 2, 2] and {f[0] for f in forms.values()} == set(GRAM_TPW)
    assert {forms[p][2] - ((p + 15) & ~15) for p in GRAM_PLANES} == {0, 16}, "both parities of ld16 / 16"
    gm = [_M(pl, rows) for pl, rows in GRAM_CASES]
    assert any(M < 32 for M in gm) and any(M % 32 for M in gm) and any(rows and rows[0] > 0 for _, rows in GRAM_M)
    assert [gram64_chunk_rows(_M(*c)) for c in GRAM_BIG] == [32, 64] and [gram64_chunks(_M(*c)) for c in GRAM_BIG] == [512, 258]
    hit = {}
    for K, plane, rows in PROJECT_CASES:
        res, nt, rem, _ = project64_form(K, _levels(plane).p)
        hit.setdefault((res, nt, rem), set()).add(_M(plane, rows) % 512 if res else _M(plane, rows) % 128)
        assert nle_ld(K) <= (K + 15) // 16 * 16
    assert sorted(hit) == sorted(ALL_PROJECT), "every one of the 28 projection kernels is named by a case"
    assert all(hit[(True, nt, rem)] & {0, 1, 511} for nt in range(1, 5) for rem in range(5))
    assert all(hit[(False, nt, 0)] & {0, 1, 127} for nt in range(5, 9))
    assert set().union(*(hit[f] for f in ALL_PROJECT[:20])) >= {0, 1, 511} and set().union(*(hit[f] for f in ALL_PROJECT[20:])) >= {0, 1, 127}
    assert {K % 4 for K, _, _ in PROJECT_CASES if project64_form(K, 30)[2]} == {0, 1, 2, 3}, "the REM forms with and without padding columns"
    assert project64_form(64, 232)[:2] == (True, 4) and project64_form(64, 233)[:2] == (False, 4)
    assert [project64_form(K, _levels(pl).p)[:3] for K, pl in ((48, P400), (32, P400), (16, P1152))] == [(False, 3, 0), (False, 2, 0), (False, 1, 0)]
    assert any(_M(pl, rows) < 16 for _, pl, rows in PROJECT_CASES) and any(rows and rows[0] > 0 for _, _, rows in PROJECT_CASES)
    assert _M(*PROJECT_BIG[1:]) > 256 * 512 and project64_form(PROJECT_BIG[0], 16)[:3] == (True, 1, 1)
    ps, rs = {c[0] for c in UPDATE_CASES}, {c[1] for c in UPDATE_CASES}
    assert ps == {1, 31, 32, 33, 63, 64, 65, 576, 1152} and rs >= {1, 3, 4, 5, 63, 64, 65, 128, 129}
    assert all(any(c[0] == p and c[1] == p and c[2] for c in UPDATE_CASES) for p in ps), "r = p with chol at every p"
    assert any(c[1] < c[0] for c in UPDATE_CASES) and {c[3] for c in UPDATE_CASES} == {1, 8} and all(zld_of(p) > p for p in ps)
    assert {(2 * p > 64, 2 * p > 128) for p in ps} == {(False, False), (True, False), (True, True)}


def _all_planes():
    out = {}
    for table in (PASS_PLANES, GRAM_PLANES):
        out.update({pl: p for p, pl in table.items()})
    out.update({MODERATE[0]: 30, MODERATE[1]: 30, MODERATE[2]: 28, P232: 232, P233: 233, P400: 400, P1152: 1152, PASS_REFUSED: 272})
    for pl in [c[0] for c in PASS_M + GRAM_M + GRAM_BIG] + [PASS_BIG[0], PROJECT_BIG[1]]:
        out.setdefault(pl, 16)
    return out


def test_planes_realise_the_intended_p(nle, oracle):
    for (H, W, nr, nc), p in _all_planes().items():
        g = nle.sample_grid(H, W, nr, nc)
        assert g["n_sel_rows"] * g["n_sel_cols"] == p, ((H, W, nr, nc), p)
        assert oracle.sample_pixels(H, W, nr, nc)[0].size == p
    assert PASS_PLANES[16][:2] != (4, 4) and _levels((4, 4, 4, 4)).ns.sum() == 0, "an image whose every pixel is a sample"


def test_exact_inputs_are_exact():
    for p, plane in list(PASS_PLANES.items())[::5] + [(16, PASS_BIG[0])]:
        pl, w = _levels(plane), pass_inputs(_levels(plane), True)
        assert len(set(pl.lev)) == p and (pl.xi[pl.ns] >= p).any() and pl.xi.max() <= p + 2 and (np.bincount(pl.xi)[:p] > 1).any()
        cls = np.bincount(pl.lev, weights=w)
        assert np.all(np.frexp(cls)[0] == 0.5), "every level class sums to a power of two"
        assert np.bincount(pl.xi).max() < 2 ** 24
    for p, plane in GRAM_PLANES.items():
        pl = _levels(plane, True)
        counts = np.bincount(pl.lev)
        assert set(counts) <= {2, 3}, "levels shared by two or three samples"
        if p > 48:
            a = np.flatnonzero(pl.lev == 0)
            assert len({s // 16 for s in a}) == len(a), "... of different 16 x 16 tiles"
    npw = np.float32(-np.log2(np.e) / HY_EXACT ** 2)
    assert np.float32(-np.log2(np.e) / HX_EXACT ** 2) == 0 and np.signbit(np.float32(-np.log2(np.e) / HX_EXACT ** 2)) and npw <= -577


REAL_PLANES = sorted(set(PASS_PLANES.values()) | set(GRAM_PLANES.values()) | set(MODERATE) | {P232, P233, P400, P1152, (12, 13, 4, 4), (9, 4, 4, 4)})


@pytest.mark.parametrize("plane", REAL_PLANES, ids=_ids(REAL_PLANES))
def test_real_planes_keep_the_exponent_in_range(plane):
    pl = _real(plane)
    assert pl.p == _all_planes().get(plane, pl.p)
    assert pl.L.max() <= ARG_MAX * LN2, f"|arg| reaches {pl.L.max() / LN2:.1f}"
    assert pl.L.max() >= 20 * LN2, "and is not trivially small either"


# ------------------------------------------------------------------ CPU: the checkers have teeth
def _k32(pl):
    """the kernels' fp32 affinities in numpy: the exact indicator, or affinity_value's arithmetic rounded step by step"""
    return pl.slab(None)[0] if isinstance(pl, Levels) else _affinity_f32(pl).astype(np.float64)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])
@pytest.mark.parametrize("Kc", [50, 35])
def test_checkers_project(exact, Kc):
    pl = _levels(MODERATE[0]) if exact else _real(MODERATE[0])
    K, dK, _ = pl.slab(None)
    c, D = pixel_scalings(pl, None, exact), project_inputs(pl, Kc, exact)
    k32, p = _k32(pl), pl.p
    good = np.zeros((K.shape[0], nle_ld(Kc)), dtype=np.float32)
    good[:, :Kc] = c[:, None] * (k32 @ D)
    assert check_project(good, K, dK, c, D) < 1.0
    m = good.copy()                                                 # one 16-column tile taken from the pixel 16 rows on
    m[:-16, 16:32] = good[16:, 16:32]
    assert _rejects(check_project, m, K, dK, c, D)
    m = good.copy()                                                 # a remainder column left at the sentinel
    m[K.shape[0] // 2, Kc // 16 * 16] = np.nan
    assert _rejects(check_project, m, K, dK, c, D)
    m = good.copy()                                                 # a padding column left at the sentinel, or at anything
    m[7, Kc] = np.nan
    assert _rejects(check_project, m, K, dK, c, D)
    m[7, Kc] = 1e-30
    assert _rejects(check_project, m, K, dK, c, D)
    rows = np.argsort(-k32[:, p - 1])[:16]                          # the last sample dropped from one tile's contraction
    m = good.copy()
    m[rows, :16] = c[rows, None] * (k32[rows, :p - 1] @ D[:p - 1, :16])
    assert _rejects(check_project, m, K, dK, c, D) or not np.any(D[p - 1, :16])
    m = good.copy()                                                 # the last pixel not written
    m[-1] = 0
    assert _rejects(check_project, m, K, dK, c, D)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])
def test_checkers_pass(exact):
    plane = PASS_PLANES[80]
    pl = _levels(plane) if exact else _real(plane)
    K, dK, ns = pl.slab(None)
    w, k32 = pass_inputs(pl, exact), _k32(pl).astype(np.float32)
    for recip in (False, True):
        d = k32.astype(np.float64) @ w
        y = np.where(ns, np.where(d >= EPS, 1 / np.where(d != 0, d, 1), 0) if recip else 1.0, 0.0)
        terms = (k32 * y.astype(np.float32)[:, None]).astype(np.float64)     # k (float)y in fp32, summed in fp64
        good = terms.sum(axis=0)
        assert max(check_pass(good, y, K, dK, w, ns, recip)) < 1.0
        assert _rejects(check_pass, good - terms[64:128].sum(axis=0), y, K, dK, w, ns, recip)     # one 64-pixel tile left out of z
        m = good.copy()                                                                             # z[s] and z[s ^ 32] exchanged
        m[[3, 35]] = m[[35, 3]]
        assert _rejects(check_pass, m, y, K, dK, w, ns, recip)
        m = y.copy()                                                                                # y written at a sample pixel
        m[pl.sel[0]] = 1.0
        assert _rejects(check_pass, good, m, K, dK, w, ns, recip)
        if recip:                                                                                   # the last sample left out of d
            yb = np.where(ns, 1 / (k32[:, :-1].astype(np.float64) @ w[:-1] + 1e-300), 0.0)
            share = np.where(ns, k32[:, -1] * w[-1] / np.maximum(d, 1e-300), 0)
            near = int(np.argmax(share))
            m = y.copy()
            m[near] = min(yb[near], 1e300)
            assert _rejects(check_pass, good, m, K, dK, w, ns, recip) or share[near] < 1e-3


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])
def test_checkers_gram(exact):
    plane = GRAM_PLANES[209]
    pl = _levels(plane, True) if exact else _real(plane)
    K, dK, ns = pl.slab(None)
    c, k32, p, M = pixel_scalings(pl, None, exact, nan_at_samples=True), _k32(pl), pl.p, K.shape[0]
    Z = np.where(ns, c, 0.0)[:, None] * k32                        # z = c (double)k in fp64
    rows = gram64_chunk_rows(M)

    def chunked(skip=None):
        G = np.zeros((p, p))
        for ci, c0 in enumerate(range(0, M, rows)):
            if ci != skip:
                G += Z[c0:c0 + rows].T @ Z[c0:c0 + rows]
        return np.triu(G) + np.triu(G, 1).T

    good = chunked()
    assert check_gram(good, K, dK, c, ns) < 1.0
    big = int(np.argmax([np.abs(Z[c0:c0 + rows]).sum() for c0 in range(0, M, rows)]))
    assert _rejects(check_gram, chunked(skip=big), K, dK, c, ns)                                    # one chunk left out
    tpw, groups, _, ntiles = gram64_form(p)
    assert groups == 2
    nt, t = (p + 15) // 16, 4 * tpw                               # the first tile of the second group: (ti, tj) of list index t
    ti = 0
    while t >= nt - ti:
        t, ti = t - (nt - ti), ti + 1
    tj = ti + t
    m = good.copy()                                                                                 # ... replaced by tile 0
    hi, wj = min(16, p - ti * 16), min(16, p - tj * 16)
    m[ti * 16:ti * 16 + hi, tj * 16:tj * 16 + wj] = good[:hi, :wj]
    m[tj * 16:tj * 16 + wj, ti * 16:ti * 16 + hi] = good[:hi, :wj].T
    assert _rejects(check_gram, m, K, dK, c, ns)
    m = good.copy()                                                                                 # asymmetric by one ulp
    m[0, p - 1] = np.nextafter(m[0, p - 1], np.inf)
    assert _rejects(check_gram, m, K, dK, c, ns)
    Zs = np.where(np.isnan(c), 1.0, c)[:, None] * k32                                               # the sample pixels not skipped
    assert _rejects(check_gram, Zs.T @ Zs, K, dK, c, ns)
    assert _rejects(check_gram, np.full((p, p), np.nan), K, dK, c, ns)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])
@pytest.mark.parametrize("p,r,chol,zrows", [(33, 5, 0, 8), (65, 65, 1, 1)])
def test_checkers_update(exact, p, r, chol, zrows):
    for recip in (False, True):
        X1, X2, lam, z, sA = update_inputs(p, r, chol, zrows, exact, recip)
        good = update_reference(X1, X2, lam, z, sA, chol)           # numpy's own fp64 evaluation
        assert max(check_update(good, X1, X2, lam, z, sA, chol, exact)) < 1.0
        if chol:                                                     # y_A taken from the wrong half of v
            assert _rejects(check_update, update_reference(X1, X2, lam, z, sA, chol, wrong_half=True), X1, X2, lam, z, sA, chol, exact)
        if zrows > 1:                                                # the last slice of z left out
            assert _rejects(check_update, update_reference(X1, X2, lam, z[:-1], sA, chol), X1, X2, lam, z, sA, chol, exact)
        bad = [a.copy() for a in good]                               # the last entry of v dropped from u
        bad[1][:] = lam * (X1[:-1].T @ good[0][:-1])
        assert _rejects(check_update, bad, X1, X2, lam, z, sA, chol, exact) or np.abs(X1[-1]).max() == 0
        bad = [a.copy() for a in good]                               # two entries of w' swapped
        if p > 1:
            bad[3][[0, p - 1]] = bad[3][[p - 1, 0]]
            assert _rejects(check_update, bad, X1, X2, lam, z, sA, chol, exact)


# ------------------------------------------------------------------ GPU
def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _plane_for(plane, exact, shared=False):
    return _levels(plane, shared) if exact else _real(plane)


def _run_pass(ctx, plane, rows, exact, tag):
    pl = _plane_for(plane, exact)
    K, dK, ns = pl.slab(rows)
    w = pass_inputs(pl, exact)
    out = []
    for recip, wv in ((False, None), (True, w)) + (((True, np.zeros(pl.p)),) if exact else ()):
        z, y = ctx.sample_pass(pl.x, pl.nr, pl.nc, pl.hx, pl.hy, wv, recip, rows)
        out += list(check_pass(z, y.cpu().numpy(), K, dK, wv if wv is not None else np.zeros(pl.p), ns, recip))
    print(f"sample_space pass {tag} {_id((plane, rows))} p={pl.p} M={K.shape[0]}: k_sink_pass<{sink_pp(pl.p)}> NJ={sink_nj(pl.p)} "
          f"grid={sink_grid(K.shape[0])}, max err/bound colsum z {out[0]:.3g}; recip z {out[2]:.3g} y {out[3]:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("plane,rows", PASS_CASES + [PASS_BIG], ids=_ids(PASS_CASES + [PASS_BIG]))
def test_pass_exact(nle, ctx, plane, rows):
    _run_pass(ctx, plane, rows, True, "exact")


PASS_REAL = [c for c in PASS_CASES if c[0] != (4, 4, 4, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("plane,rows", PASS_REAL, ids=_ids(PASS_REAL))
def test_pass_elementwise(nle, ctx, plane, rows):
    _run_pass(ctx, plane, rows, False, "real")


def _run_gram(ctx, plane, rows, exact, tag):
    pl = _plane_for(plane, exact, shared=True)
    K, dK, ns = pl.slab(rows)
    c = pixel_scalings(pl, rows, exact, nan_at_samples=True)
    worst = check_gram(ctx.sample_gram(pl.x, pl.nr, pl.nc, pl.hx, pl.hy, _dev(c), rows), K, dK, c, ns)
    M = K.shape[0]
    print(f"sample_space gram {tag} {_id((plane, rows))} p={pl.p} M={M}: k_gram64<{gram64_form(pl.p)[0]}> x {gram64_form(pl.p)[1]} group(s), "
          f"{gram64_chunks(M)} chunk(s) of {gram64_chunk_rows(M)} rows, max err/bound {worst:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("plane,rows", GRAM_CASES + GRAM_BIG, ids=_ids(GRAM_CASES + GRAM_BIG))
def test_gram_exact(nle, ctx, plane, rows):
    _run_gram(ctx, plane, rows, True, "exact")


@pytest.mark.gpu
@pytest.mark.parametrize("plane,rows", GRAM_CASES, ids=_ids(GRAM_CASES))
def test_gram_elementwise(nle, ctx, plane, rows):
    _run_gram(ctx, plane, rows, False, "real")


def _run_project(ctx, Kc, plane, rows, exact, tag):
    import torch
    pl = _plane_for(plane, exact)
    K, dK, _ = pl.slab(rows)
    c, D = pixel_scalings(pl, rows, exact), project_inputs(pl, Kc, exact)
    out = torch.full((K.shape[0], nle_ld(Kc)), float("nan"), dtype=torch.float32, device="cuda")   # an unwritten element shows
    V = ctx.sample_project(pl.x, pl.nr, pl.nc, pl.hx, pl.hy, D, _dev(c), rows, out=out).cpu().numpy()
    res, nt, rem, ldb = project64_form(Kc, pl.p)
    print(f"sample_space project {tag} K={Kc} {_id((plane, rows))} p={pl.p} M={K.shape[0]} ldv={nle_ld(Kc)}: "
          f"{'k_project64_res<%d, 16, %d>' % (nt, rem) if res else 'k_project64<%d>' % nt}", end="")
    worst = check_project(V, K, dK, c, D)
    print(f", max err/bound {worst:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("Kc,plane,rows", PROJECT_CASES + [PROJECT_BIG], ids=_ids(PROJECT_CASES + [PROJECT_BIG]))
def test_project_exact(nle, ctx, Kc, plane, rows):
    _run_project(ctx, Kc, plane, rows, True, "exact")


@pytest.mark.gpu
@pytest.mark.parametrize("Kc,plane,rows", PROJECT_CASES, ids=_ids(PROJECT_CASES))
def test_project_elementwise(nle, ctx, Kc, plane, rows):
    _run_project(ctx, Kc, plane, rows, False, "real")


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])
@pytest.mark.parametrize("p,r,chol,zrows", UPDATE_CASES, ids=_ids(UPDATE_CASES))
def test_update(nle, ctx, p, r, chol, zrows, exact):
    worst = (0.0, 0.0)
    for recip in (False, True):
        X1, X2, lam, z, sA = update_inputs(p, r, chol, zrows, exact, recip)
        got = check_update(ctx.sample_update(X1, X2, lam, z, sA, bool(chol)), X1, X2, lam, z, sA, chol, exact)
        worst = tuple(max(a, b) for a, b in zip(worst, got))
    print(f"sample_space update {'exact' if exact else 'real'} p={p} r={r} chol={chol} zrows={zrows} zld={zld_of(p)}: "
          f"k_sink_update_a x {(r + 3) // 4} + k_sink_update_b x {(2 * p + 3) // 4} workgroups, max err/bound v {worst[0]:.3g}; u, s_A', w' {worst[1]:.3g}")


def _refused(nle, ctx, call):
    with pytest.raises(nle.NLEError) as e:
        call()
    assert e.value.code == nle.NLE_ERR_INVALID
    assert (nle.lib().nle_last_error(ctx._h) or b"").decode().strip(), "nle_last_error must say what was refused"


@pytest.mark.gpu
def test_pass_refuses_more_than_256_samples(nle, ctx):
    pl = _levels(PASS_REFUSED)
    _refused(nle, ctx, lambda: ctx.sample_pass(pl.x, pl.nr, pl.nc, pl.hx, pl.hy, np.ones(pl.p), True))


@pytest.mark.gpu
def test_gram_refuses_more_than_256_samples(nle, ctx):
    pl = _levels(PASS_REFUSED)
    _refused(nle, ctx, lambda: ctx.sample_gram(pl.x, pl.nr, pl.nc, pl.hx, pl.hy, _dev(np.ones(pl.H * pl.W))))


@pytest.mark.gpu
def test_project_refuses_more_than_128_columns(nle, ctx):
    pl = _levels(MODERATE[0])
    _refused(nle, ctx, lambda: ctx.sample_project(pl.x, pl.nr, pl.nc, pl.hx, pl.hy, np.ones((pl.p, PROJECT_REFUSED_K)),
                                                  _dev(np.ones(pl.H * pl.W))))
