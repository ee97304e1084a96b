"""The kernels of csrc/tables.hip, each ALONE and entry by entry, through the nle_table_* stage entry points: k_check_levels
(table_levels); k_hist_tables (table_build); k_hist_g, k_hist_pix<NC>, k_hist_hh, k_z_reduce (table_pass); k_hist_g, k_hist_dot<NC>
(table_expand); k_apply_small, k_scatter_samples; k_ghist_rows, k_ghist_rows_chunk, k_ghist_ee, k_ghist_gemm<14>, k_ghist_final and
k_gsum_rowf, k_ghist_gemm<4>, k_gsum_final (table_gram).  What tests/test_sample_space.py is for csrc/fused.hip.  The entry
points call only the launchers the trains call, fill every workspace and output with NaN first, and hand the workspace back.

PRINCIPLE.  Every kernel is held to a reference formed from the DEVICE's own upstream intermediate, downloaded: g from the
tables, y from the device's g, h from the device's y, the (slab, level tile) partial rows from the device's h, z from the device's
partial rows; EE from er, C (or T) from the device's EE (or F) and A (or S), Gk from the device's C (or T).  No bound covers another
kernel's error.  A view is SUPPLIED (the test uploads er, ecT, Ep: no sorted rows, all 16 level tiles, the LDS-atomic pixel
kernels) or BUILT (made from a plane, hx, hy as training makes it: sorted rows -- inputs here, not subjects --, the level-tile
range, the Gram on index sums).

1. EXACT ARITHMETIC (supplied views): er, ec in {1, 2, 3}, Ep in {0, 1, 2}, w in {1, 2, 3}, c in 1 .. 7, levels and x in 0 .. 255, D,
Vrows, resp in -3 .. 3, all drawn at random so that they differ along every index.  Every product and sum is an integer below 2^53
(`magnitude_cap`, checked per case), exact in any order, LDS atomics included: g, y, h, the partial rows and z of the column-sum and
x-vector passes, the planes with round8 on and off (weights in halves: ties, and clamps at 0 and 255), t, W', YA, A, EE, C, Gk must
EQUAL the integer reference, Gk == Gk^T, and the padding z[p, ldp), W'[p, ldw), EE[NM, ldm) is exactly 0.  In the reciprocal pass d
is exact and y must be the correctly rounded quotient, |y - 1/d| <= u64 / d, and exactly 0 below eps: Ep is 0 at the levels 7 mod 16
(d = 0 exactly) and, in the reciprocal pass, scaled by 2^-60 at the levels 9 mod 16 (0 < d < eps); both kinds of pixel occur in every
case, and h and z must take nothing from them.  h and z are then sums of positive terms held to g64(n) (below).  c is NaN at the sample pixels in every case: no kernel may use it there (kernels.h, TableView::cvec).

2. REAL DATA: positive tables, Higham's g64(k) = k u / (1 - k u), u = 2^-53, k counted from the code; all terms are positive, so a
bound is g64(k) times the reference.
    k_hist_g      w Ep is one product, the MFMA chain adds 4 ksteps terms: k = 4 ceil(nR / 4) + 1
    k_hist_pix    d: nC products, two chains and their sum: k = nC + 2 =: kd; y = fl(1 / d):  |y - yref| <= ((1 + r / (1 - r)) (1 + u) - 1) yref,
                  r = g64(kd).  h[x][b] adds e y (one product) for the <= W pixels of the row in any order, a wave sum first (6 adds):
                  k = W + 7
    k_hist_hh     slab_rows MFMA terms, the product with Ep, a four-step shuffle tree: k = slab_rows + 5
    k_z_reduce    ceil(nparts / 32) terms per thread, then 32: k = ceil(nparts / 32) + 32
    k_hist_dot    nC products in two chains, their sum, the product with c: k = nC + 3; then one rounding to fp32 (u32 = 2^-24)
    k_apply_small t: two chains of ceil(p / G) products, their sum, G partials: k = ceil(p / G) + G + 2 on |D|^T |m| + |Vrows|^T |xA|;
                  W', YA from the device's t: resp t, the product, a chain of K: k = K + 2
    k_ghist_ee    one product: k = 1.   k_ghist_gemm: ksplit chain terms: k = ksplit + 1 (inputs are used as stored)
    k_ghist_final nsplit - 1 adds, two products, 4 chain terms per lane, a six-step tree: k = nsplit + 12; k_gsum_final: one more
                  for kappa, plus kappa's own error
Three outputs go through libm exp: k_hist_tables, k_gsum_rowf, kappa in k_gsum_final.  Their fp64 argument is restated bit for
bit (d d is an exact integer, one rounding in the product with 1 / hx^2; kappa's argument with and without a fused multiply-add,
either is accepted) and the result held to the longdouble exp of it at rtol 1e-14, the project's figure for an fp64 libm affinity
(tests/test_patch_affinity.py).

3. DISPATCH.  hist_g_launch, hist_slab_rows, ghist_split, chunk_cut, layers_per_launch mirror tables.hip; test_mirrors_* hold them to
the source text, test_case_tables_* hold the case tables to them and name every switch.  test_checkers_* (no GPU) feed the
checkers numpy's own fp64 evaluation, which must pass, and seven wrong maps, each of which must fail.
Every case prints its largest err / bound; the printed values are recorded in profiles/r21_table_kernel_edges.txt.
"""
import fractions
import functools
import os
import re

import numpy as np
import pytest

from test_stage32 import U32, _rejects, _worst, g64
from test_stage64 import LD, positive

U64 = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-10   # NLE_EPS
EXP_RTOL = 1e-14
COLSUM, RECIP, XVEC = 0, 1, 2


def tables_source():
    with open(os.path.join(ROOT, "nonlocal-image-edit_amd", "csrc", "tables.hip")) as f:
        return f.read()


# ------------------------------------------------------------------ mirrors of csrc/tables.hip and of make_grid
def make_grid(H, W, nr, nc):
    rs, cs = H // nr, W // nc
    ro, co = (rs - 1 + (H - rs * nr)) // 2, (cs - 1 + (W - cs * nc)) // 2

    def count(n, off, step):
        hi = min(n - 1, n - off)
        return 0 if hi < off else (hi - off) // step + 1
    return dict(row_step=rs, row_off=ro, n_sel_rows=count(H, ro, rs), col_step=cs, col_off=co, n_sel_cols=count(W, co, cs))


def hist_g_launch(nR, nC, nrows, lev_nt=16):
    ntiles, gx = (nrows + 15) // 16, (nC * lev_nt + 3) // 4
    cap = 8 if nR > 24 else 16
    chunks = max(1, min(ntiles, max((640 + gx - 1) // gx, (ntiles + cap - 1) // cap)))
    tpw = (ntiles + chunks - 1) // chunks
    return dict(gx=gx, gy=(ntiles + tpw - 1) // tpw, tpw=tpw, ksteps=(nR + 3) // 4, cap=cap, shm=tpw * 16 * nR * 8,
                idle_waves=gx * 4 - nC * lev_nt, ragged=nrows % 16 != 0)


def hist_slab_rows(nR, nC, nrows):
    ncoltiles = 256 * nC // 16
    want = max(1, (4096 + ncoltiles - 1) // ncoltiles)
    rows = (nrows + want - 1) // want
    rows = max(64, ((rows + 31) // 32) * 32)
    lds_rows = ((8192 // max(nR, 1)) // 32) * 32
    return min(rows, max(64, lds_rows))


def ghist_ldm(nR):
    return ((nR * (nR + 1) // 2) + 15) & ~15


def gsum_ldm(nR):
    return ((2 * nR - 1) + 15) & ~15


def ghist_split(N, ldm, nrows, mt=14):
    """(ksplit, nsplit) -- the split of the workspace is always made with kGhistMT, also for k_ghist_gemm<4>"""
    base = ((N // 16 + 3) // 4) * ((ldm // 16 + 14 - 1) // 14)
    ns = min(16, max(1, (1024 + base - 1) // base))
    ks = max((((nrows + ns - 1) // ns) + 15) & ~15, 16)
    return ks, max(1, (nrows + ks - 1) // ks)


def chunk_cut(nC):
    """the launches of k_ghist_rows_chunk: (b0, b1, pair offset, pairs)"""
    out, b0, off = [], 0, 0
    while b0 < nC:
        b1, n = b0, 0
        while b1 < nC and n + (nC - b1) <= 72:
            n += nC - b1
            b1 += 1
        out.append((b0, b1, off, n))
        off, b0 = off + n, b1
    return out


def layers_per_launch(nC):
    return max(1, min(4, (144 * 1024) // (256 * (nC | 1) * 8)))


def apply_small_form(K):
    KP = 64 if K <= 64 else 128
    return KP, 256 // KP


def tri_pairs(n):
    return [(i, j) for i in range(n) for j in range(i, n)]


# ------------------------------------------------------------------ cases
class Case:
    """a plane H x W whose realised grid is nR x nC, and the local rows [row0, row0 + nrows)"""

    def __init__(self, nR, nC, nrows, row0=0, W=None, H=0):
        self.nR, self.nC, self.nrows, self.row0 = nR, nC, nrows, row0
        W = max(W or 0, nC)
        while make_grid(8, W, 1, nC)["n_sel_cols"] != nC:
            W += 1
        H = max(row0 + nrows, nR, H)
        while make_grid(H, W, nR, nC)["n_sel_rows"] != nR:
            H += 1
        self.H, self.W = H, W
        self.g = make_grid(H, W, nR, nC)
        self.p, self.ldp = nR * nC, (nR * nC + 63) & ~63
        self.rows = (row0, row0 + nrows)
        self.id = f"nR{nR}-nC{nC}-rows{row0}+{nrows}-W{W}"

    def not_sample(self):
        """(nrows, W) bool: the local pixels that are no sample pixels"""
        g = self.g
        r, c = np.arange(self.row0, self.row0 + self.nrows), np.arange(self.W)
        sr = (r >= g["row_off"]) & ((r - g["row_off"]) % g["row_step"] == 0) & ((r - g["row_off"]) // g["row_step"] < self.nR)
        sc = (c >= g["col_off"]) & ((c - g["col_off"]) % g["col_step"] == 0) & ((c - g["col_off"]) // g["col_step"] < self.nC)
        return ~(sr[:, None] & sc[None, :])

    def seed(self):
        return 1009 * self.nR + 37 * self.nC + 7 * self.nrows + self.row0 + 3 * self.W


_NROWS = (1, 15, 16, 17)
# k_hist_g: ksteps 1 .. 8, the LDS cap at nR = 24 | 25, the second accumulator of k_hist_hh from nR = 17; nrows 1, 15, 16, 17; row0 > 0
G_CASES = [Case(nR, 3, _NROWS[i % 4], row0=(0, 2)[i % 2], W=13) for i, nR in enumerate((1, 3, 4, 5, 16, 17, 24, 25, 32))] + [
    Case(9, 3, 15, row0=1, W=13), Case(13, 3, 17, row0=0, W=13), Case(21, 3, 16, W=13), Case(29, 3, 1, row0=5, W=13)]
# tiles_per_wave = 2: 100 rows at nC = 36 (4 row chunks, ragged last tile), 330 rows at nC = 8
TPW_CASES = [Case(3, 36, 100, W=37), Case(32, 36, 100, W=37), Case(5, 8, 330, W=17), Case(32, 8, 330, W=17)]
# k_hist_hh / k_z_reduce: a second slab of one row, a partial slab, p % 8 != 0, a slab without a sample row (rows 1 + 2 of step 5)
HH_CASES = [Case(3, 3, 65, W=13), Case(3, 5, 100, row0=3, W=21), Case(2, 2, 2, row0=1, W=9, H=16)]
HH_BIG = Case(4, 36, 600, W=37)      # slab_rows 96, 7 slabs, the last of 24 rows: the pass only, in exact arithmetic
PASS_CASES = G_CASES + TPW_CASES + HH_CASES
PASS_REAL = G_CASES[:9] + [TPW_CASES[0], TPW_CASES[2]] + HH_CASES

# k_hist_pix<NC> and k_hist_dot<NC>, all 36: five rows (flat; four levels of 16 lanes; runs of 3 .. 11; noise; noise), one of them
# a sample row; W cycles through NC-sized, 511, 512, 513, 1025
def _nc_width(NC):
    return (NC + 2, 511, 512, 513, 1025)[NC % 5] if NC not in (1, 36) else (NC + 2 if NC == 1 else 1025)


NC_CASES = [Case(2, NC, 5, row0=1, W=_nc_width(NC)) for NC in range(1, 37)]
EXPAND_BELOW = [17, 23, 35]          # also one layer below the limit

# (K, p, L, differs)
SMALL_CASES = [(1, 1, 1, None), (63, 7, 5, 0), (64, 200, 1, 1), (65, 200, 5, None), (128, 1152, 1, 0), (128, 7, 5, 1), (65, 1, 1, 1),
               (64, 1152, 5, None)]
# Gram, pair form (nR, nC, nrows): k_ghist_rows to nC = 11, the chunk cut from 12 (12 fills one launch, 36 takes 11), gridDim.y
# 1, 2, 3 at nR 20, 21, 32, seven splits of 16 rows with a last of 4
GRAM_CASES = [Case(2, 1, 20, W=9), Case(2, 11, 20, row0=2, W=23), Case(2, 12, 20, W=25), Case(2, 13, 20, W=27), Case(2, 36, 40, W=37),
              Case(20, 2, 20, W=9), Case(21, 2, 20, row0=3, W=9), Case(32, 2, 33, W=9), Case(4, 1, 100, W=9), Case(3, 2, 2, row0=3, W=9, H=16)]
GRAM_REAL = [GRAM_CASES[i] for i in (1, 3, 5, 6, 8)]
# built views (nR, nC, nrows, row0, W; levels lo .. hi)
BUILT_CASES = [(Case(4, 5, 40, W=61), (40, 79)), (Case(3, 36, 100, W=75), (0, 255)), (Case(2, 1, 100, W=31), (16, 47)),
               (Case(3, 5, 7, row0=9, W=61), (40, 79)), (Case(3, 4, 2, row0=3, W=41, H=16), (100, 140))]
REFUSED_ROWS, REFUSED_COLS = (67, 8, 33, 2), (8, 75, 2, 37)      # planes realising nR = 33 and nC = 37


def _ids(cases):
    return [c.id if isinstance(c, Case) else "-".join(str(v) for v in c) for c in cases]


def magnitude_cap(c):
    """the largest integer an exact-arithmetic case can form: a Gram entry (module docstring)"""
    return 256 * 4 * c.nrows * 9 * c.W * 441


# ------------------------------------------------------------------ inputs
ZERO_LEVELS = np.arange(7, 256, 16)     # Ep = 0 for every sample: d = 0 exactly, y must be 0 (exact inputs)
TINY_LEVELS = np.arange(9, 256, 16)     # Ep scaled by 2^-60 in the reciprocal pass: 0 < d <= 2^-60 62208 < eps, y must be 0


def plane_patterns(rng, nrows, W):
    """integer levels: row 0 flat, row 1 four levels of 16 lanes per wave, row 2 runs of 3 .. 11 lanes, the rest noise"""
    x = rng.integers(0, 256, (nrows, W))
    x[0] = 200
    if nrows > 1:
        x[1] = (np.arange(W) // 16 * 37 + 5) % 256
    if nrows > 2:
        runs = np.repeat(rng.integers(0, 256, W), rng.integers(3, 12, W))[:W]
        x[2] = runs
    return x


@functools.lru_cache(maxsize=None)
def inputs(case, exact, lo=0, hi=255):
    c = case
    rng = np.random.default_rng(c.seed() + (0 if exact else 500000))
    full = rng.integers(lo, hi + 1, (c.H, c.W))
    loc = plane_patterns(rng, c.nrows, c.W)
    full[c.row0:c.row0 + c.nrows] = lo + loc % (hi - lo + 1)
    ns = c.not_sample()
    d = dict(lum=full.astype(np.float32), xi=full[c.row0:c.row0 + c.nrows].copy(), ns=ns,
             xvec=rng.integers(0, 256, (c.H, c.W)).astype(np.float32))
    if exact:
        d.update(er=rng.integers(1, 4, (c.nrows, c.nR)).astype(np.float64), ecT=rng.integers(1, 4, (c.nC, c.W)).astype(np.float64),
                 Ep=rng.integers(0, 3, (256, c.p)).astype(np.float64), w=rng.integers(1, 4, c.p).astype(np.float64),
                 c=rng.integers(1, 8, (c.nrows, c.W)).astype(np.float64))
        d["er"][:, 0], d["Ep"][:, 0] = (np.arange(c.nrows) % 3) + 1, 1 + np.arange(256) % 2     # d > 0 at every level ...
        d["Ep"][ZERO_LEVELS] = 0                                       # ... but these: g = 0 and d = 0 exactly
        d["Ep_recip"] = d["Ep"].copy()                                 # the reciprocal pass: and 0 < d < eps at these levels
        d["Ep_recip"][TINY_LEVELS] *= 2.0 ** -60
        spare = np.argwhere(ns)[-2:]                                   # both kinds occur in every case that has two free pixels
        for (r, cc), lev in zip(spare, (ZERO_LEVELS[0], TINY_LEVELS[0])):
            if lo == 0 and hi == 255:
                d["xi"][r, cc] = lev
                d["lum"][c.row0 + r, cc] = lev
    else:
        d.update(er=positive(rng, c.nrows, c.nR), ecT=positive(rng, c.nC, c.W), Ep=positive(rng, 256, c.p),
                 w=positive(rng, 1, c.p)[0], c=positive(rng, c.nrows, c.W))
    return d


def c_with(d, at_samples):
    c = d["c"].copy()
    c[~d["ns"]] = at_samples
    return c


# ------------------------------------------------------------------ references and checkers (plain functions; dt = np.float64 or LD)
def _first(bad, what, extra=lambda b: ""):
    assert bad.size == 0, f"{len(bad)} {what}; first at {bad[0].tolist()}{extra(bad[0])}"


def _hold(got, ref, k, what, exact, extra_rel=0.0):
    """every entry of got to the exact ref, or within (g64(k) + extra_rel) |ref| of it.  Returns max err / bound"""
    got = np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    _first(np.argwhere(~np.isfinite(got)), f"entries of {what} are not finite (never written, or a sentinel was read)")
    if exact:
        _first(np.argwhere(got != ref), f"entries of {what} differ from the integer reference", lambda b: f": got {got[tuple(b)]} want {ref[tuple(b)]}")
        return 0.0
    worst, first = _worst(np.abs(got.astype(LD) - ref), (g64(k) + extra_rel) * np.abs(ref))
    assert first is None, f"{what} beyond g64({k}); first {first}, max err/bound {worst:.3g}"
    return worst


def tiles_mask(lev):
    t0, nt = lev
    m = np.zeros(256, dtype=bool)
    m[16 * t0:16 * (t0 + nt)] = True
    return m


def g_reference(er, Ep, w, nR, nC, dt):
    WE = (w.reshape(nR, nC)[None] * Ep.reshape(256, nR, nC)).astype(dt)           # [x][a][b]
    return np.einsum("ra,xab->rbx", er.astype(dt), WE) if dt is np.float64 else (
        er.astype(dt) @ WE.transpose(1, 2, 0).reshape(nR, nC * 256)).reshape(er.shape[0], nC, 256)


def check_g(g, er, Ep, w, nR, nC, exact, lev=(0, 16)):
    """g: (nrows, nC, 256) of k_hist_g; outside the level tiles `lev` the sentinel must still be there"""
    m = tiles_mask(lev)
    assert np.isnan(g[:, :, ~m]).all(), "g outside the level tiles that occur must not be written"
    ref = g_reference(er, Ep, w, nR, nC, np.float64 if exact else LD)
    k, what = 4 * ((nR + 3) // 4) + 1, f"g {hist_g_launch(nR, nC, er.shape[0], lev[1])}"
    if exact or (w >= 0).all():
        return _hold(g[:, :, m], ref[:, :, m], k, what, exact)
    assert np.isfinite(g[:, :, m]).all(), what                     # signed weights (the expand half): the bound is on the magnitudes
    worst, first = _worst(np.abs(g[:, :, m].astype(LD) - ref[:, :, m]), g64(k) * g_reference(er, Ep, np.abs(w), nR, nC, LD)[:, :, m])
    assert first is None, f"{what} beyond g64({k}); first {first}, max err/bound {worst:.3g}"
    return worst


def d_reference(g, ecT, xi, dt):
    nrows, W = xi.shape
    gv = g[np.arange(nrows)[:, None], :, xi]                                       # (nrows, W, nC)
    return np.einsum("rcb,bc->rc", gv.astype(dt), ecT.astype(dt))


def check_y(y, mode, g, ecT, xi, ns, c, xvec_loc, exact):
    """y: (nrows, W) of k_hist_pix from the DEVICE's g.  Returns max err / bound"""
    assert y.shape == xi.shape and np.isfinite(y).all(), "y must be written (and finite) at every local pixel"
    assert np.all(y[~ns] == 0), "y must be exactly 0 at the sample pixels"
    nC = ecT.shape[0]
    if mode == COLSUM:
        _first(np.argwhere(y[ns] != 1), "entries of y differ from 1")
        return 0.0
    if mode == XVEC:
        _first(np.argwhere(y[ns] != (c * xvec_loc)[ns]), "entries of y differ from c x (one correctly rounded product)")
        return 0.0
    d = d_reference(g, ecT, xi, np.float64 if exact else LD)
    live = ns & (np.abs(d) >= EPS)                                  # recip_or_zero_d: 1 / d from eps on, 0 below
    if exact:                                                        # d is exact: the eps arm is decided without a margin
        _first(np.argwhere(ns & ~live & ~(y == 0)), "entries of y are not exactly 0 where |d| < eps",
               lambda b: f": d = {d[tuple(b)]}, y = {y[tuple(b)]}")
    else:
        assert (d[ns] > 100 * EPS).all(), "the real data keep d well above eps"
    yref = np.where(live, 1 / np.where(live, d, 1).astype(LD), 0)
    r = 0.0 if exact else g64(nC + 2)
    rel = LD(r) / (1 - LD(r))                                       # (1 + rel) (1 + u64) - 1, formed without cancellation
    worst, first = _worst(np.abs(y.astype(LD) - yref), (rel * (1 + LD(U64)) + LD(U64)) * yref)
    assert first is None, f"y beyond the bound; first pixel {first}, max err/bound {worst:.3g}"
    return worst


def h_reference(y, ecT, xi, ns, dt):
    nrows, W = xi.shape
    nC = ecT.shape[0]
    h = np.zeros((nrows, nC, 256), dtype=dt)
    rr, cc = np.nonzero(ns)
    for b in range(nC):
        np.add.at(h[:, b, :], (rr, xi[rr, cc]), ecT[b, cc].astype(dt) * y[rr, cc].astype(dt))
    return h


def check_h(h, y, ecT, xi, ns, exact, lev=(0, 16)):
    """h: (nrows, nC, 256) of k_hist_pix from the DEVICE's y"""
    m = tiles_mask(lev)
    assert np.isnan(h[:, :, ~m]).all(), "h outside the level tiles that occur must not be written"
    ref = h_reference(y, ecT, xi, ns, np.float64 if exact else LD)
    assert not ref[:, :, ~m].any(), "the plane's levels lie inside the level tiles"
    return _hold(h[:, :, m], ref[:, :, m], xi.shape[1] + 7, "h", exact)


def zpart_reference(h, er, Ep, nR, nC, slab_rows, lev, dt, drop=None, swap_acc=False):
    """the (slab, level tile) partial rows from h; drop: a (slab, tile) left out; swap_acc: the sample rows a >= 16 take the
    first accumulator's values (two of the wrong maps of test_checkers_z)"""
    nrows, (t0, nt) = h.shape[0], lev
    nslabs = (nrows + slab_rows - 1) // slab_rows
    Ex = Ep.reshape(256, nR, nC).astype(dt)
    out = np.zeros((nslabs, nt, nR * nC), dtype=dt)
    for s in range(nslabs):
        sl = slice(s * slab_rows, min(nrows, (s + 1) * slab_rows))
        hs = np.where(tiles_mask(lev), h[sl], 0).astype(dt)
        HH = (er[sl].astype(dt).T @ hs.reshape(hs.shape[0], nC * 256)).reshape(nR, nC, 256)     # [a][b][x]
        if swap_acc and nR > 16:
            HH[16:] = HH[:nR - 16]
        prod = HH * Ex.transpose(1, 2, 0)
        for t in range(nt):
            if drop != (s, t):
                out[s, t] = prod[:, :, 16 * (t0 + t):16 * (t0 + t) + 16].sum(axis=2).reshape(-1)
    return out


def check_z(zpart, z, h, er, Ep, nR, nC, slab_rows, exact, lev=(0, 16)):
    """zpart: (nslabs lev_nt, ldp) of k_hist_hh from the DEVICE's h; z: (ldp) of k_z_reduce from the DEVICE's zpart"""
    p, ldp, nparts = nR * nC, z.shape[0], zpart.shape[0]
    assert np.isnan(zpart[:, p:]).all(), "the partial rows beyond p are nobody's to write"
    ref = zpart_reference(h, er, Ep, nR, nC, slab_rows, lev, np.float64 if exact else LD).reshape(nparts, p)
    w1 = _hold(zpart[:, :p], ref, slab_rows + 5, f"zpart (slab_rows {slab_rows}, {nparts} parts)", exact)
    _first(np.argwhere(~(z[p:] == 0)), f"padding entries z[{p} .. {ldp}) are not exactly zero")
    zsum = zpart[:, :p].astype(np.float64 if exact else LD).sum(axis=0)
    return max(w1, _hold(z[:p], zsum, (nparts + 31) // 32 + 32, "z", exact))


def round8(v):
    return np.rint(np.minimum(255.0, np.maximum(0.0, v)))


def check_planes(out, gws, ecT, c, xi, ns, r8, exact):
    """out: (nl, nrows W) fp32 of k_hist_dot from the DEVICE's g tables gws (nl, nrows, nC, 256)"""
    nl, (nrows, W), nC = gws.shape[0], xi.shape, ecT.shape[0]
    worst = 0.0
    for l in range(nl):
        o = out[l, :nrows * W].reshape(nrows, W)
        _first(np.argwhere(o[~ns] != 0), "sample pixels of a plane are not 0 (c is not used there)")
        s = d_reference(gws[l], ecT, xi, np.float64 if exact else LD)
        v = np.where(ns, c, 0).astype(s.dtype) * s
        assert np.isfinite(o[ns]).all(), "every non-sample pixel of a plane is written"
        if exact:
            want = (round8(v) if r8 else v).astype(np.float32)
            assert np.abs(v).max() < 2 ** 24
            _first(np.argwhere((o != want) & ns), f"pixels of plane {l} differ (round8 {r8})", lambda b: f": got {o[tuple(b)]} want {want[tuple(b)]}")
        else:
            b0 = g64(nC + 3) * np.abs(v)
            if r8:          # the rounded value of anything within b0 of v
                lo, hi = round8((v - b0).astype(np.float64)), round8((v + b0).astype(np.float64))
                _first(np.argwhere(((o < lo) | (o > hi)) & ns), f"pixels of plane {l} are not the rounded value")
            else:
                w, first = _worst(np.where(ns, np.abs(o.astype(LD) - v), 0), b0 + U32 * (np.abs(v) + b0))
                assert first is None, f"plane {l} beyond the bound; first pixel {first}, max err/bound {w:.3g}"
                worst = max(worst, w)
    return worst


def small_reference(m, D, V, xA, resp, dt, exchanged=False):
    K = resp.shape[1]
    if exchanged:                                                    # (the wrong map of test_checkers_small)
        m, xA = xA, m
    t = D[:, :K].astype(dt).T @ m.astype(dt) + V[:, :K].astype(dt).T @ xA.astype(dt)
    return t


def check_small(res, m, D, V, xA, resp, ldw, exact):
    """res = (t (K), W' (L, ldw), YA (L, p)) of k_apply_small; W' and YA from the DEVICE's t"""
    t, Wp, YA = res
    (p, _), (L, K) = D.shape, resp.shape
    KP, G = apply_small_form(K)
    dt = np.float64 if exact else LD
    _first(np.argwhere(~(Wp[:, p:] == 0)), f"padding entries W'[{p} .. {ldw}) are not exactly zero")
    tref = small_reference(m, D, V, xA, resp, dt)
    if exact:
        w0 = _hold(t, tref, 0, f"t (KP {KP}, G {G})", True)
    else:
        mag = np.abs(D[:, :K]).astype(LD).T @ np.abs(m).astype(LD) + np.abs(V[:, :K]).astype(LD).T @ np.abs(xA).astype(LD)
        w0, first = _worst(np.abs(t.astype(LD) - tref), g64(-(-p // G) + G + 2) * mag)
        assert first is None, f"t beyond the bound (KP {KP}, G {G}); first {first}, max err/bound {w0:.3g}"
    gk = resp.astype(dt) * t.astype(dt)[None]                        # (L, K)
    worst = w0
    for name, got, M in (("W'", Wp[:, :p], D), ("YA", YA, V)):
        ref = gk @ M[:, :K].astype(dt).T
        if exact:
            _hold(got, ref, 0, name, True)
        else:
            assert np.isfinite(got).all(), f"{name} must be written"
            w, first = _worst(np.abs(got.astype(LD) - ref), g64(K + 2) * (np.abs(gk) @ np.abs(M[:, :K]).astype(LD).T))
            assert first is None, f"{name} beyond the bound; first {first}, max err/bound {w:.3g}"
            worst = max(worst, w)
    return worst


def A_reference(c, ecT, xi, ns, dt):
    """A: (nrows, NP, 256) = sum over the row's non-sample pixels of level x of c^2 ec[b] ec[b2], pairs b <= b2 row-major"""
    nrows, W = xi.shape
    nC = ecT.shape[0]
    q = np.where(ns, c, 0).astype(dt)[None] * ecT.astype(dt)[:, None, :]          # (nC, nrows, W)
    A = np.zeros((nrows, nC * (nC + 1) // 2, 256), dtype=dt)
    rr, cc = np.nonzero(ns)
    for j, (b, b2) in enumerate(tri_pairs(nC)):
        np.add.at(A[:, j, :], (rr, xi[rr, cc]), q[b, rr, cc] * q[b2, rr, cc])
    return A


def gemm_reference(EE, A2, ksplit, dt, skip=None):
    """C: (nsplit, ldm, N) from EE (nrows, ldm) and A2 (nrows, N); skip: a split left out (test_checkers_gram)"""
    nrows = EE.shape[0]
    ns = max(1, (nrows + ksplit - 1) // ksplit)
    C = np.zeros((ns, EE.shape[1], A2.shape[1]), dtype=dt)
    for z in range(ns):
        if z != skip:
            sl = slice(z * ksplit, min(nrows, (z + 1) * ksplit))
            C[z] = EE[sl].astype(dt).T @ A2[sl].astype(dt)
    return C


def final_reference(C, Ep, nR, nC, dt, cross_wrong=False):
    """Gk from C (nsplit, ldm, NP, 256); cross_wrong: the (a1,b2) x (a2,b1) entry written with the (a1,b1) x (a2,b2) value"""
    p = nR * nC
    Cs = np.zeros(C.shape[1:], dtype=dt)
    for z in range(C.shape[0]):
        Cs = Cs + C[z].astype(dt)
    E = Ep.astype(dt)
    Gk = np.full((p, p), np.nan, dtype=dt)
    for m, (a1, a2) in enumerate(tri_pairs(nR)):
        for pc, (b1, b2) in enumerate(tri_pairs(nC)):
            s11, s22, s12, s21 = a1 * nC + b1, a2 * nC + b2, a1 * nC + b2, a2 * nC + b1
            u = (E[:, s11] * E[:, s22] * Cs[m, pc]).sum()
            Gk[s11, s22] = Gk[s22, s11] = u
            if a1 != a2 and b1 != b2:
                v = u if cross_wrong else (E[:, s12] * E[:, s21] * Cs[m, pc]).sum()
                Gk[s12, s21] = Gk[s21, s12] = v
    return Gk


def check_gram_pairs(Gk, ws, c, er, ecT, Ep, xi, ns, nR, nC, exact, split=None, check_A=True):
    """Gk (p, p) and the workspace (A, EE, C) of the pair form; returns max err / bound over EE, C, Gk (and A in exact arithmetic)"""
    nrows, NP, NM, ldm, p = xi.shape[0], nC * (nC + 1) // 2, nR * (nR + 1) // 2, ghist_ldm(nR), nR * nC
    N = 256 * NP
    ksplit, nsplit = split or ghist_split(N, ldm, nrows)             # the split the entry point reports (held to the mirror by the caller)
    A = ws[:nrows * N].reshape(nrows, NP, 256)
    EE = ws[nrows * N:nrows * (N + ldm)].reshape(nrows, ldm)
    C = ws[nrows * (N + ldm):nrows * (N + ldm) + nsplit * ldm * N].reshape(nsplit, ldm, N)
    dt = np.float64 if exact else LD
    worst = 0.0
    if check_A:
        # (real data: the sums of a bin go through LDS atomics in any order, after two products and c ec: k = W + 9)
        worst = _hold(A, A_reference(c, ecT, xi, ns, dt), xi.shape[1] + 9, f"A ({'k_ghist_rows' if nC <= 11 else 'k_ghist_rows_chunk x %d' % len(chunk_cut(nC))})", exact)
    _first(np.argwhere(~(EE[:, NM:] == 0)), f"padding entries EE[{NM} .. {ldm}) are not exactly zero")
    pa = tri_pairs(nR)
    EEref = er.astype(dt)[:, [a for a, _ in pa]] * er.astype(dt)[:, [b for _, b in pa]]
    worst = max(worst, _hold(EE[:, :NM], EEref, 1, "EE", exact))
    Cref = gemm_reference(EE, A.reshape(nrows, N), ksplit, dt)
    worst = max(worst, _hold(C, Cref, ksplit + 1, f"C (ksplit {ksplit}, nsplit {nsplit}, gridDim.y {(ldm // 16 + 13) // 14})", exact))
    assert np.array_equal(Gk, Gk.T), "Gk must be exactly symmetric"
    Gref = final_reference(C.reshape(nsplit, ldm, NP, 256), Ep, nR, nC, dt)
    assert np.isfinite(Gref.astype(np.float64)).all(), "every entry of Gk is fed by one (row pair, column pair)"
    return max(worst, _hold(Gk, Gref, nsplit + 12, "Gk", exact))


def exp_of(arg):
    """the longdouble exp of fp64 arguments"""
    return np.exp(np.asarray(arg, dtype=np.float64).astype(LD))


def hold_exp(got, arg, what):
    """got = libm exp(arg) on the device, arg restated bit for bit: rtol 1e-14 against the longdouble exp"""
    ref = exp_of(arg)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    worst, first = _worst(np.abs(got.astype(LD) - ref), EXP_RTOL * ref)
    assert first is None, f"{what} beyond rtol 1e-14 of exp; first {first}, max err/bound {worst:.3g}"
    return worst


def tables_arguments(case, hx, hy, sample_levels):
    """the fp64 arguments of k_hist_tables' three exp calls, restated: -(d d) (1 / (h h))"""
    g = case.g
    ihx, ihy = 1.0 / (hx * hx), 1.0 / (hy * hy)
    dr = (case.row0 + np.arange(case.nrows))[:, None] - (g["row_off"] + np.arange(case.nR) * g["row_step"])[None]
    dc = np.arange(case.W)[None] - (g["col_off"] + np.arange(case.nC) * g["col_step"])[:, None]
    dx = np.arange(256, dtype=np.float64)[:, None] - np.asarray(sample_levels, dtype=np.float64)[None]
    return -(dr * dr).astype(np.float64) * ihx, -(dc * dc).astype(np.float64) * ihx, -(dx * dx) * ihy


def _fma(a, b, c):
    return float(fractions.Fraction(a) * fractions.Fraction(b) + fractions.Fraction(c))


def check_gram_sums(Gk, ws, case, hx, Ep, split):
    """the index-sum form of a built view: F (k_gsum_rowf), T (k_ghist_gemm<4>) from the DEVICE's F and S, Gk (k_gsum_final) from
    the DEVICE's T.  S is k_sorted_gsum's: an input.  Returns (max err/bound of T and Gk, largest ratio of the exp outputs)"""
    nR, nC, nrows, g = case.nR, case.nC, case.nrows, case.g
    p, N2, ldm2, ns_ = nR * nC, 256 * (2 * nC - 1), gsum_ldm(nR), 2 * nR - 1
    ksplit, nsplit = split
    assert split == ghist_split(N2, ldm2, nrows), "the split the entry point reports is the mirror's"
    S = ws[:nrows * N2].reshape(nrows, N2)
    F = ws[nrows * N2:nrows * (N2 + ldm2)].reshape(nrows, ldm2)
    T = ws[nrows * (N2 + ldm2):nrows * (N2 + ldm2) + nsplit * ldm2 * N2].reshape(nsplit, ldm2, N2)
    assert np.isfinite(S).all() and (S >= 0).all(), "S, the sorted kernel's output, is this test's input"
    _first(np.argwhere(~(F[:, ns_:] == 0)), f"padding entries F[{ns_} .. {ldm2}) are not exactly zero")
    ihx = 1.0 / (hx * hx)
    d = (case.row0 + np.arange(nrows) - g["row_off"]).astype(np.float64)[:, None] - 0.5 * np.arange(ns_)[None] * float(g["row_step"])
    wexp = hold_exp(F[:, :ns_], -2.0 * d * d * ihx, "F")
    worst = _hold(T, gemm_reference(F, S, ksplit, LD), ksplit + 1, f"T (ksplit {ksplit}, nsplit {nsplit})", False)
    assert np.array_equal(Gk, Gk.T), "Gk must be exactly symmetric"
    rs, cs = float(g["row_step"]), float(g["col_step"])
    kr2, kc2 = rs * rs / (2.0 * hx * hx), cs * cs / (2.0 * hx * hx)
    Ts = np.zeros(T.shape[1:], dtype=LD)
    for z in range(nsplit):
        Ts = Ts + T[z].astype(LD)
    Ts = Ts.reshape(ldm2, 2 * nC - 1, 256)
    a, b = np.divmod(np.arange(p), nC)
    core = np.einsum("xi,xj,ijx->ij", Ep.astype(LD), Ep.astype(LD), Ts[a[:, None] + a[None], b[:, None] + b[None]])
    # kappa = exp(-(da da) kr2 - (db db) kc2): the compiler may fuse either product into the subtraction
    kap_ok = {}
    for da in range(nR):
        for db in range(nC):
            fa, fb = float(da * da), float(db * db)
            kap_ok[(da, db)] = {-fa * kr2 - fb * kc2, _fma(-fb, kc2, -fa * kr2), _fma(-fa, kr2, -(fb * kc2))}
    da, db = np.abs(a[:, None] - a[None]), np.abs(b[:, None] - b[None])
    best = np.full((p, p), np.inf)
    for i in range(3):
        arg = np.array([[sorted(kap_ok[(x, y)])[min(i, len(kap_ok[(x, y)]) - 1)] for y in range(nC)] for x in range(nR)])[da, db]
        ref = exp_of(arg) * core
        best = np.minimum(best, (np.abs(Gk.astype(LD) - ref) / ((g64(nsplit + 13) + EXP_RTOL * (1 + g64(nsplit + 13))) * np.abs(ref))).astype(np.float64))
    assert np.isfinite(Gk).all(), "every entry of Gk is written"
    _first(np.argwhere(~(best <= 1)), "entries of Gk beyond g64(nsplit + 13) and kappa's rtol 1e-14", lambda b_: f": err/bound {best[tuple(b_)]:.3g}")
    return max(worst, float(best.max())), wexp


# ------------------------------------------------------------------ CPU: mirrors, case tables, conditions
def test_mirrors_match_the_source():
    src = tables_source()
    for text in ("const int ntiles = (nrows_local + 15) / 16;", "const int gx = (gs.nSelCols * lev_nt + 3) / 4;",
                 "const int cap = gs.nSelRows > 24 ? 8 : 16;",
                 "const int chunks = std::max(1, std::min(ntiles, std::max((640 + gx - 1) / gx, (ntiles + cap - 1) / cap)));",
                 "const int tpw = (ntiles + chunks - 1) / chunks;", "const int ksteps = (nR + 3) >> 2;",
                 "const int ncoltiles = kLevels * gs.nSelCols / 16;", "const int want = std::max(1, (4096 + ncoltiles - 1) / ncoltiles);",
                 "rows = std::max(64, ((rows + 31) / 32) * 32);", "const int lds_rows = ((8192 / std::max(gs.nSelRows, 1)) / 32) * 32;",
                 "return std::min(rows, std::max(64, lds_rows));", "int ghist_ldm(int nR) { return ((nR * (nR + 1) / 2) + 15) & ~15; }",
                 "static int gsum_ldm(int nR) { return ((2 * nR - 1) + 15) & ~15; }", "constexpr int kGhistMT = 14;",
                 "const long long base = ((N / 16 + 3) / 4) * ((ldm / 16 + kGhistMT - 1) / kGhistMT);",
                 "int ns = (int)std::min<long long>(16, std::max<long long>(1, (1024 + base - 1) / base));",
                 "int ks = (((nrows_local + ns - 1) / ns) + 15) & ~15;", "ks = std::max(ks, 16);", "constexpr int kGhistChunkPairs = 72;",
                 "while (b1 < nC && np + (nC - b1) <= kGhistChunkPairs) {", "} else if (nC <= 11) {", "constexpr int kDotLayers = 4;",
                 "const size_t table = (size_t)kLevels * (v.gs.nSelCols | 1) * sizeof(double);",
                 "return (int)std::max<size_t>(1, std::min<size_t>(kDotLayers, (size_t)(144 * 1024) / table));",
                 "const int KP = K <= 64 ? 64 : 128, G = 256 / KP;", "const bool two = nR > 16;", "constexpr int MT2 = 4;",
                 "dispatch_columns<1, 36>(nC, [&](auto nc) {", "constexpr int kLevels = 256;",
                 "const size_t ldp = ((size_t)gs.nSelRows * gs.nSelCols + 63) & ~(size_t)63;",
                 "return 2 * (size_t)nrows_local * n + (size_t)nslabs * std::max(n * gs.nSelRows, (size_t)(kLevels / 16) * ldp);"):
        assert text in src, text
    with open(os.path.join(ROOT, "nonlocal-image-edit_amd", "csrc", "pipeline_internal.h")) as f:
        hdr = f.read()
    for text in ("gs->rowOff = (gs->rowStep - 1 + (H - gs->rowStep * nRow)) / 2;", "const int hi = std::min(n - 1, n - off);",
                 "return (hi - off) / step + 1;"):
        assert text in hdr, text


def test_case_tables_hist_g_and_hh():
    forms = {c.nR: hist_g_launch(c.nR, c.nC, c.nrows) for c in G_CASES}
    assert {f["ksteps"] for f in forms.values()} == set(range(1, 9)), "ksteps = ceil(nR / 4) takes 1 .. 8"
    assert {1, 3, 4, 5, 16, 17, 24, 25, 32} <= set(forms) and forms[24]["cap"] == 16 and forms[25]["cap"] == 8
    assert {c.nrows for c in G_CASES} == {1, 15, 16, 17} and any(c.row0 > 0 for c in G_CASES)
    assert all(f["tpw"] == 1 for f in forms.values())
    t = [hist_g_launch(c.nR, c.nC, c.nrows) for c in TPW_CASES]
    assert [(c.nR, c.nC, c.nrows) for c in TPW_CASES] == [(3, 36, 100), (32, 36, 100), (5, 8, 330), (32, 8, 330)]
    assert all(f["tpw"] == 2 for f in t) and t[0]["gy"] == 4 and t[0]["ragged"] and t[2]["ragged"]
    # tiles_per_wave goes above 1 from 81 rows at nC = 36 and from 321 rows at nC = 8
    assert [hist_g_launch(4, 36, n)["tpw"] for n in (80, 81)] == [1, 2] and [hist_g_launch(4, 8, n)["tpw"] for n in (320, 321)] == [1, 2]
    assert max(f["shm"] for f in t + list(forms.values())) <= 48 * 1024
    assert {c.nR > 16 for c in PASS_CASES} == {True, False} and {16, 17} <= {c.nR for c in PASS_CASES}, "the second accumulator from nR = 17"
    slabs = [(hist_slab_rows(c.nR, c.nC, c.nrows), c.nrows) for c in HH_CASES + [HH_BIG]]
    assert slabs[0] == (64, 65) and slabs[1] == (64, 100), "a second slab of one row; a partial second slab"
    assert slabs[3] == (96, 600) and -(-600 // 96) == 7 and 600 - 6 * 96 == 24, "96-row slabs: the 64-row loop runs a second, partial time"
    assert any(c.p % 8 for c in HH_CASES) and any(c.ldp > c.p for c in PASS_CASES) and any(c.ldp == c.p for c in PASS_CASES)
    nparts = [-(-c.nrows // hist_slab_rows(c.nR, c.nC, c.nrows)) * 16 for c in PASS_CASES + [HH_BIG]]
    assert min(nparts) < 32 < max(nparts), "fewer than 32 parts, and more"
    c = HH_CASES[2]
    assert c.row0 > 0 and c.not_sample().all(), "a slab at row0 > 0 that holds no sample row"
    b = BUILT_CASES[0][0]
    f = hist_g_launch(b.nR, b.nC, b.nrows, 3)
    assert (b.nC, f["gx"], f["idle_waves"]) == (5, 4, 1), "15 column tiles, one idle wave (col_ok false)"


def test_case_tables_pix_dot_small_gram():
    assert sorted(c.nC for c in NC_CASES) == list(range(1, 37)), "all 36 instantiations of k_hist_pix and k_hist_dot"
    assert {c.W for c in NC_CASES} >= {511, 512, 513, 1025} and any(c.W < 64 for c in NC_CASES)
    assert all(c.row0 > 0 and not c.not_sample().all() and c.not_sample().all(axis=1).any() for c in NC_CASES), "sample and non-sample rows"
    assert [layers_per_launch(n) for n in (17, 18, 23, 24, 35, 36)] == [4, 3, 3, 2, 2, 1]
    assert [n for n in range(1, 36) if layers_per_launch(n) != layers_per_launch(n + 1)] == [17, 23, 35] == EXPAND_BELOW
    Ks, ps = {c[0] for c in SMALL_CASES}, {c[1] for c in SMALL_CASES}
    assert Ks == {1, 63, 64, 65, 128} and ps == {1, 7, 200, 1152} and {c[2] for c in SMALL_CASES} == {1, 5}
    assert {c[3] for c in SMALL_CASES} == {None, 0, 1} and apply_small_form(64) == (64, 4) and apply_small_form(65) == (128, 2)
    assert any(p % apply_small_form(K)[1] for K, p, _, _ in SMALL_CASES)
    assert [c.nC for c in GRAM_CASES[:5]] == [1, 11, 12, 13, 36] and GRAM_CASES[4].nrows <= 40
    assert [n for *_, n in chunk_cut(12)] == [72, 6] and len(chunk_cut(36)) == 11, "nC = 12 fills a launch exactly"
    assert all(sum(n for *_, n in chunk_cut(nC)) == nC * (nC + 1) // 2 and max(n for *_, n in chunk_cut(nC)) <= 72 for nC in range(12, 37))
    assert [(ghist_ldm(c.nR) // 16 + 13) // 14 for c in GRAM_CASES[5:8]] == [1, 2, 3] and [c.nR for c in GRAM_CASES[5:8]] == [20, 21, 32]
    c = GRAM_CASES[8]
    assert ghist_split(256, ghist_ldm(c.nR), c.nrows) == (16, 7) and c.nrows - 6 * 16 == 4
    assert any(c.row0 > 0 for c in GRAM_CASES) and GRAM_CASES[9].not_sample().all()
    b36, b1 = BUILT_CASES[1][0], BUILT_CASES[2][0]
    assert ghist_split(256 * 71, gsum_ldm(b36.nR), b36.nrows)[1] == 4 and ghist_split(256, gsum_ldm(b1.nR), b1.nrows)[1] == 7
    assert any(c.row0 > 0 for c, _ in BUILT_CASES) and BUILT_CASES[4][0].not_sample().all()


ALL_CASES = PASS_CASES + [HH_BIG] + NC_CASES + GRAM_CASES + [c for c, _ in BUILT_CASES]


def test_cases_realise_the_intended_grid_and_stay_exact(nle):
    for c in ALL_CASES:
        g = nle.sample_grid(c.H, c.W, c.nR, c.nC)
        assert g == c.g and (g["n_sel_rows"], g["n_sel_cols"]) == (c.nR, c.nC), c.id
        assert magnitude_cap(c) < 2 ** 53 and c.row0 + c.nrows <= c.H, c.id
    for c in PASS_CASES + [HH_BIG] + NC_CASES:                           # the reciprocal's eps arm runs in every exact pass case
        d = inputs(c, True)
        if d["ns"].sum() >= 2:
            assert (np.isin(d["xi"], ZERO_LEVELS) & d["ns"]).any() and (np.isin(d["xi"], TINY_LEVELS) & d["ns"]).any(), c.id
        assert not d["Ep"][ZERO_LEVELS].any() and 54 * c.p * 2.0 ** -60 < EPS and (d["Ep"][:, 0][TINY_LEVELS] > 0).all()
    for pl, want in ((REFUSED_ROWS, (33, 2)), (REFUSED_COLS, (2, 37))):
        g = nle.sample_grid(*pl)
        assert (g["n_sel_rows"], g["n_sel_cols"]) == want
    assert nle.table_workspace(33, 2, 8) == -1 and nle.table_workspace(2, 37, 8, True) == -1
    c = HH_BIG
    assert nle.table_workspace(c.nR, c.nC, c.nrows) == 2 * c.nrows * 256 * c.nC + 7 * max(256 * c.nC * c.nR, 16 * c.ldp)


# ------------------------------------------------------------------ CPU: the checkers have teeth
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])
def test_checkers_pass(exact):
    c = Case(19, 3, 40, row0=2, W=13)
    d = inputs(c, exact)
    nR, nC, sr = c.nR, c.nC, 32                                        # (two slabs: any slab length serves the checker)
    d = dict(d, Ep=d["Ep_recip"]) if exact else d                        # the reciprocal pass's table: levels with d = 0 and 0 < d < eps
    g = g_reference(d["er"], d["Ep"], d["w"], nR, nC, np.float64)
    assert check_g(g, d["er"], d["Ep"], d["w"], nR, nC, exact) < 1
    m = g.copy()                                                         # a g tile taken from the row tile below
    m[:16, 1, 32:48] = g[16:32, 1, 32:48]
    assert _rejects(check_g, m, d["er"], d["Ep"], d["w"], nR, nC, exact)
    m = g.copy()                                                         # an element left at the sentinel
    m[39, 2, 255] = np.nan
    assert _rejects(check_g, m, d["er"], d["Ep"], d["w"], nR, nC, exact)
    dd = d_reference(g, d["ecT"], d["xi"], np.float64)
    live = d["ns"] & (dd >= EPS)
    y = np.where(live, 1 / np.where(live, dd, 1), 0)
    assert check_y(y, RECIP, g, d["ecT"], d["xi"], d["ns"], None, None, exact) < 1
    if exact:                                                            # the eps arm of the reciprocal left out, or decided the wrong way
        zero, tiny = d["ns"] & (dd == 0), d["ns"] & (dd > 0) & (dd < EPS)
        assert zero.any() and tiny.any()
        for where, val in ((zero, np.inf), (zero, 1 / EPS), (tiny, 1 / EPS)):
            m = y.copy()
            m[where] = val
            assert _rejects(check_y, m, RECIP, g, d["ecT"], d["xi"], d["ns"], None, None, exact)
        m = y.copy()
        m[tiny] = 1 / dd[tiny]                                           # eps ignored: the quotient of a d below it
        assert _rejects(check_y, m, RECIP, g, d["ecT"], d["xi"], d["ns"], None, None, exact)
        m = np.where(d["ns"] & (dd < 1e3), 0, y)                         # the comparison the other way round somewhere above eps
        assert _rejects(check_y, m, RECIP, g, d["ecT"], d["xi"], d["ns"], None, None, exact)
        r0, c0 = np.argwhere(zero)[0]                                    # h takes a contribution from a pixel whose y is 0
        hb = h_reference(y, d["ecT"], d["xi"], d["ns"], np.float64)
        hb[r0, :, d["xi"][r0, c0]] += d["ecT"][:, c0] * 1e-3
        assert _rejects(check_h, hb, y, d["ecT"], d["xi"], d["ns"], False)
    m = y.copy()
    m[~d["ns"]] = 1.0
    assert _rejects(check_y, m, RECIP, g, d["ecT"], d["xi"], d["ns"], None, None, exact)
    m = np.roll(y, 1, axis=1)                                            # the neighbour's y
    assert _rejects(check_y, m, RECIP, g, d["ecT"], d["xi"], d["ns"], None, None, exact)
    h = h_reference(y, d["ecT"], d["xi"], d["ns"], np.float64)
    assert check_h(h, y, d["ecT"], d["xi"], d["ns"], False) < 1
    m = h.copy()                                                         # two levels of one table exchanged
    x0 = int(np.argmax(h[3, 1]))
    m[3, 1, [x0, (x0 + 1) % 256]] = m[3, 1, [(x0 + 1) % 256, x0]]
    assert _rejects(check_h, m, y, d["ecT"], d["xi"], d["ns"], False)
    zp = zpart_reference(h, d["er"], d["Ep"], nR, nC, sr, (0, 16), np.float64)
    nparts = zp.shape[0] * 16

    def full(zparts):
        out = np.full((nparts, c.ldp), np.nan)
        out[:, :c.p] = zparts.reshape(nparts, c.p)
        return out
    z = np.zeros(c.ldp)
    z[:c.p] = zp.reshape(nparts, c.p).sum(axis=0)
    assert check_z(full(zp), z, h, d["er"], d["Ep"], nR, nC, sr, False) < 1
    big = np.unravel_index(np.argmax(zp.sum(axis=2)), zp.shape[:2])
    bad = zpart_reference(h, d["er"], d["Ep"], nR, nC, sr, (0, 16), np.float64, drop=tuple(int(v) for v in big))
    assert _rejects(check_z, full(bad), z, h, d["er"], d["Ep"], nR, nC, sr, False)            # one level tile's zpart row dropped
    zb = z.copy()
    zb[:c.p] -= zp[big]
    assert _rejects(check_z, full(zp), zb, h, d["er"], d["Ep"], nR, nC, sr, False)           # ... or left out of the reduce
    bad = zpart_reference(h, d["er"], d["Ep"], nR, nC, sr, (0, 16), np.float64, swap_acc=True)
    assert _rejects(check_z, full(bad), z, h, d["er"], d["Ep"], nR, nC, sr, False)            # the second accumulator's sample rows exchanged
    zb = z.copy()
    zb[c.p] = np.nan                                                                           # a padding element left at the sentinel
    assert _rejects(check_z, full(zp), zb, h, d["er"], d["Ep"], nR, nC, sr, False)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])
def test_checkers_gram(exact):
    c = Case(3, 3, 40, row0=1, W=13)
    d = inputs(c, exact)
    nR, nC, nrows = c.nR, c.nC, c.nrows
    NP, ldm = 6, ghist_ldm(nR)
    N = 256 * NP
    ksplit, nsplit = ghist_split(N, ldm, nrows)
    assert nsplit == 3
    cv = c_with(d, 0.0)
    A = A_reference(cv, d["ecT"], d["xi"], d["ns"], np.float64)
    EE = np.zeros((nrows, ldm))
    pa = tri_pairs(nR)
    EE[:, :len(pa)] = d["er"][:, [a for a, _ in pa]] * d["er"][:, [b for _, b in pa]]

    def run(skip=None, cross_wrong=False, pad=0.0):
        E2 = EE.copy()
        E2[5, len(pa)] = pad
        C = gemm_reference(EE, A.reshape(nrows, N), ksplit, np.float64, skip=skip)
        Gk = final_reference(C.reshape(nsplit, ldm, NP, 256), d["Ep"], nR, nC, np.float64, cross_wrong)
        ws = np.concatenate([A.ravel(), E2.ravel(), C.ravel()])
        return check_gram_pairs(Gk, ws, cv, d["er"], d["ecT"], d["Ep"], d["xi"], d["ns"], nR, nC, exact)
    assert run() < 1
    assert _rejects(run, 1)                      # one GEMM split left out
    assert _rejects(run, None, True)             # the (a1,b2) x (a2,b1) entry written with the (a1,b1) x (a2,b2) value
    assert _rejects(run, None, False, np.nan)    # a padding element left at the sentinel


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])
def test_checkers_small_and_planes(exact):
    K, p, L, ldw = 65, 200, 3, 256
    m, D, V, xA, resp, _, _ = small_inputs(K, p, L, exact)

    def device(exchanged=False, pad=0.0):
        t = small_reference(m, D, V, xA, resp, np.float64, exchanged)
        gk = resp * t[None]
        Wp = np.full((L, ldw), pad)
        Wp[:, :p] = gk @ D[:, :K].T
        return t, Wp, gk @ V[:, :K].T
    assert check_small(device(), m, D, V, xA, resp, ldw, exact) < 1
    assert _rejects(check_small, device(exchanged=True), m, D, V, xA, resp, ldw, exact)       # t formed with xA and m exchanged
    assert _rejects(check_small, device(pad=np.nan), m, D, V, xA, resp, ldw, exact)           # padding left at the sentinel
    c = Case(2, 3, 5, row0=1, W=13)
    d = inputs(c, exact)
    wl = expand_weights(c, 2, exact)
    gws = np.stack([g_reference(d["er"], d["Ep"], w[:c.p], c.nR, c.nC, np.float64) for w in wl])
    cv = c_with(d, 0.0)
    for r8 in (False, True):
        v = np.stack([cv * d_reference(gws[l], d["ecT"], d["xi"], np.float64) for l in range(2)])
        out = (round8(v) if r8 else v).astype(np.float32).reshape(2, -1)
        assert check_planes(out, gws, d["ecT"], cv, d["xi"], d["ns"], r8, exact) < 1
        bad = out.copy()
        bad[1] = out[0]                                                                          # the other layer's table
        assert _rejects(check_planes, bad, gws, d["ecT"], cv, d["xi"], d["ns"], r8, exact)
        if exact and r8:
            assert (v < 0).any() and (v > 255).any() and (np.abs(v - np.floor(v) - 0.5) == 0).any(), "clamps at 0 and 255, and ties"
            bad = np.floor(np.minimum(255, np.maximum(0, v)) + 0.5).astype(np.float32).reshape(2, -1)   # ties rounded up
            assert _rejects(check_planes, bad, gws, d["ecT"], cv, d["xi"], d["ns"], r8, exact)


# ------------------------------------------------------------------ GPU
def small_inputs(K, p, L, exact):
    rng = np.random.default_rng(977 * K + 31 * p + L)
    ldk = (K + 15) // 16 * 16
    if exact:
        D, V = (rng.integers(-3, 4, (p, ldk)).astype(np.float64) for _ in range(2))
        resp = rng.integers(-3, 4, (L, K)).astype(np.float64)
        m, xA, ms, xs = (rng.integers(0, 256, p).astype(np.float64) for _ in range(4))
    else:
        D, V = (positive(rng, p, ldk) * rng.choice([-1.0, 1.0], (p, ldk)) for _ in range(2))
        resp = rng.uniform(-2.0, 2.0, (L, K))
        m, xA, ms, xs = (positive(rng, 1, p)[0] * 100 for _ in range(4))
    D[:, K:], V[:, K:] = np.nan, np.nan                                   # columns [K, ldk) are never read
    return m, D, V, xA, resp, ms, xs


def expand_weights(c, nl, exact):
    rng = np.random.default_rng(c.seed() + 77)
    if exact:                      # halves: ties; layer 0 mostly beyond 255, layer 1 mostly below 0
        wl = rng.integers(-3, 4, (nl, c.ldp)).astype(np.float64) * 0.5
        wl[0] = np.abs(wl[0]) + 0.5
        if nl > 1:
            wl[1] = -np.abs(wl[1])
        scale = 2.0 ** -np.ceil(np.log2(max(c.nR * c.nC * 7 * 3 * 3 * 2 * 3 / 512, 1)))
        wl[2:] *= scale
        wl[0, 0] *= scale
        return wl
    return positive(rng, nl, c.ldp) * rng.choice([-1.0, 1.0], (nl, c.ldp)) * 300


def _np(t):
    return t.cpu().numpy()


def _split_ws(c, res, lev_nt=16):
    n, ws = res["n"], _np(res["ws"])
    sr = hist_slab_rows(c.nR, c.nC, c.nrows)
    nparts = -(-c.nrows // sr) * lev_nt
    shape = (c.nrows, c.nC, 256)
    return ws[:n].reshape(shape), ws[n:2 * n].reshape(shape), ws[2 * n:2 * n + nparts * c.ldp].reshape(nparts, c.ldp), sr


def _run_pass(ctx, c, exact, modes=(COLSUM, XVEC, RECIP)):
    d = inputs(c, exact)
    tabs = (d["er"], d["ecT"], d["Ep"])
    cnan = c_with(d, np.nan)
    out = {}
    for mode in modes:
        Ep = d["Ep_recip"] if exact and mode == RECIP else d["Ep"]
        tabs = (d["er"], d["ecT"], Ep)
        res = ctx.table_pass(d["lum"], c.nR, c.nC, mode, rows=c.rows, tables=tabs, c=cnan if mode == XVEC else None,
                             w=d["w"] if mode == RECIP else None, x=d["xvec"] if mode == XVEC else None)
        g, h, zpart, sr = _split_ws(c, res)
        y, z = _np(res["y"]).reshape(c.nrows, c.W), _np(res["z"])
        ex = exact and mode != RECIP
        if mode == RECIP:
            out["g"] = check_g(g, d["er"], Ep, d["w"], c.nR, c.nC, exact)
            if exact:
                dd = d_reference(g, d["ecT"], d["xi"], np.float64)
                out["d=0"], out["0<d<eps"] = int((d["ns"] & (dd == 0)).sum()), int((d["ns"] & (dd > 0) & (dd < EPS)).sum())
                assert (out["d=0"] and out["0<d<eps"]) or d["ns"].sum() < 2, "the eps arm of the reciprocal runs"
        else:
            assert np.isnan(g).all(), "only the reciprocal pass makes g"
        xloc = d["xvec"][c.row0:c.row0 + c.nrows].astype(np.float64)
        out[f"y{mode}"] = check_y(y, mode, g, d["ecT"], d["xi"], d["ns"], d["c"], xloc, exact)
        out[f"h{mode}"] = check_h(h, y, d["ecT"], d["xi"], d["ns"], ex)
        out[f"z{mode}"] = check_z(zpart, z, h, d["er"], Ep, c.nR, c.nC, sr, ex)
    f = hist_g_launch(c.nR, c.nC, c.nrows)
    print(f"table_kernels pass {'exact' if exact else 'real'} {c.id}: k_hist_g ksteps {f['ksteps']} tpw {f['tpw']} grid {f['gx']}x{f['gy']}, "
          f"k_hist_pix<{c.nC}>, slab_rows {hist_slab_rows(c.nR, c.nC, c.nrows)}; max err/bound " + ", ".join(f"{k} {v:.3g}" for k, v in out.items()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", PASS_CASES, ids=_ids(PASS_CASES))
def test_pass_exact(nle, ctx, case):
    _run_pass(ctx, case, True)


@pytest.mark.gpu
def test_pass_exact_96_row_slabs(nle, ctx):
    _run_pass(ctx, HH_BIG, True, modes=(COLSUM, RECIP))


@pytest.mark.gpu
@pytest.mark.parametrize("case", PASS_REAL, ids=_ids(PASS_REAL))
def test_pass_elementwise(nle, ctx, case):
    _run_pass(ctx, case, False, modes=(RECIP, XVEC))


def _run_expand(ctx, c, nl, exact, r8):
    d = inputs(c, exact)
    cv, wl = c_with(d, np.nan), expand_weights(c, nl, exact)
    ostride = c.nrows * c.W + 3
    gws, out = ctx.table_expand(d["lum"], c.nR, c.nC, wl, cv, rows=c.rows, tables=(d["er"], d["ecT"], d["Ep"]), round8=r8, ostride=ostride)
    gws, out = _np(gws), _np(out)
    assert np.isnan(out[:, c.nrows * c.W:]).all(), "the planes end at nrows W"
    worst = max(check_g(gws[l], d["er"], d["Ep"], wl[l, :c.p], c.nR, c.nC, exact) for l in range(nl))
    return max(worst, check_planes(out, gws, d["ecT"], cv, d["xi"], d["ns"], r8, exact))


@pytest.mark.gpu
@pytest.mark.parametrize("case", NC_CASES, ids=_ids(NC_CASES))
def test_pix_and_dot_every_column_count(nle, ctx, case):
    """k_hist_pix<NC> and k_hist_dot<NC> in exact arithmetic: the three pass modes; the expand half with nl at the LDS limit (and
    one below it where the limit switches), round8 on and off"""
    _run_pass(ctx, case, True)
    lim = layers_per_launch(case.nC)
    for nl in [lim] + ([lim - 1] if case.nC in EXPAND_BELOW else []):
        for r8 in (False, True):
            _run_expand(ctx, case, nl, True, r8)
    print(f"table_kernels dot exact {case.id}: k_hist_dot<{case.nC}> nl {lim}, max err/bound 0")


EXPAND_REAL = [NC_CASES[i] for i in (0, 4, 16, 22, 35)] + [G_CASES[8]]


@pytest.mark.gpu
@pytest.mark.parametrize("case", EXPAND_REAL, ids=_ids(EXPAND_REAL))
def test_expand_elementwise(nle, ctx, case):
    nl = layers_per_launch(case.nC)
    worst = max(_run_expand(ctx, case, nl, False, r8) for r8 in (False, True))
    print(f"table_kernels dot real {case.id}: k_hist_dot<{case.nC}> nl {nl}, max err/bound {worst:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "real"])
@pytest.mark.parametrize("K,p,L,differs", SMALL_CASES, ids=_ids(SMALL_CASES))
def test_apply_small(nle, ctx, K, p, L, differs, exact):
    m, D, V, xA, resp, ms, xs = small_inputs(K, p, L, exact)
    ldw = (p + 63) & ~63
    nan = np.full(p, np.nan)
    if differs == 0:            # the stand-ins are used: the others are never read
        res = ctx.table_apply_small(nan, D, V, nan, resp, ldw, 0, m, xA)
    elif differs == 1:
        res = ctx.table_apply_small(m, D, V, xA, resp, ldw, 1, nan, nan)
    else:
        res = ctx.table_apply_small(m, D, V, xA, resp, ldw)
    worst = check_small(res, m, np.nan_to_num(D), np.nan_to_num(V), xA, resp, ldw, exact)
    print(f"table_kernels apply_small {'exact' if exact else 'real'} K={K} p={p} L={L} differs={differs}: KP, G = {apply_small_form(K)}, max err/bound {worst:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("p,L,r8", [(7, 5, False), (200, 3, True), (1, 1, True)])
def test_scatter_samples(nle, ctx, p, L, r8):
    import torch
    assert (L * p) % 256 != 0
    rng = np.random.default_rng(p + L)
    n = 4 * p + 9
    loc = rng.permutation(n)[:p].astype(np.int64)
    loc[::3] = -1
    YA = rng.integers(-40, 600, (L, p)) * 0.5
    Y = torch.full((L, n), float("nan"), dtype=torch.float32, device="cuda")
    got = _np(ctx.table_scatter(loc, YA, Y, r8))
    want = np.full((L, n), np.nan, dtype=np.float32)
    want[:, loc[loc >= 0]] = (round8(YA) if r8 else YA)[:, loc >= 0].astype(np.float32)
    assert np.array_equal(got, want, equal_nan=True)


def _run_gram(ctx, c, exact):
    d = inputs(c, exact)
    cv = c_with(d, np.nan)
    Gk, ws, split = ctx.table_gram(d["lum"], c.nR, c.nC, cv, rows=c.rows, tables=(d["er"], d["ecT"], d["Ep"]))
    NP, ldm = c.nC * (c.nC + 1) // 2, ghist_ldm(c.nR)
    ks, ns = ghist_split(256 * NP, ldm, c.nrows)
    assert split == (ks, ns), "the split the entry point reports is the mirror's"
    worst = check_gram_pairs(_np(Gk), _np(ws), cv, d["er"], d["ecT"], d["Ep"], d["xi"], d["ns"], c.nR, c.nC, exact, split)
    print(f"table_kernels gram {'exact' if exact else 'real'} {c.id}: {'k_ghist_rows' if c.nC <= 11 else 'k_ghist_rows_chunk x %d' % len(chunk_cut(c.nC))}, "
          f"k_ghist_gemm<14> grid y {(ldm // 16 + 13) // 14} z {ns} (ksplit {ks}), max err/bound {worst:.3g}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", GRAM_CASES, ids=_ids(GRAM_CASES))
def test_gram_exact(nle, ctx, case):
    _run_gram(ctx, case, True)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GRAM_REAL, ids=_ids(GRAM_REAL))
def test_gram_elementwise(nle, ctx, case):
    _run_gram(ctx, case, False)


@pytest.mark.gpu
@pytest.mark.parametrize("case,levels", BUILT_CASES, ids=_ids([c for c, _ in BUILT_CASES]))
def test_built_view(nle, ctx, oracle, case, levels):
    """a view built as training builds it: k_hist_tables against the restated exp arguments; the level-tile range (g and h outside
    it keep the sentinel, z and the planes are finite); k_hist_g, k_hist_hh, k_z_reduce on it; the Gram on index sums"""
    c, (lo, hi) = case, levels
    d = inputs(c, False, lo, hi)
    hx, hy = c.W / 4.0, 30.0
    b = ctx.table_build(d["lum"], c.nR, c.nC, hx, hy, rows=c.rows)
    lev = (lo // 16, hi // 16 - lo // 16 + 1)
    assert b["sorted"] and (b["lev_t0"], b["lev_nt"]) == lev and b["index_sums"], b
    er, ecT, Ep = (_np(b[k]) for k in ("er", "ecT", "Ep"))
    sel, _ = oracle.sample_pixels(c.H, c.W, c.nR, c.nC)
    a_er, a_ec, a_ep = tables_arguments(c, hx, hy, d["lum"].reshape(-1)[sel])
    wexp = max(hold_exp(er, a_er, "er"), hold_exp(ecT, a_ec, "ecT"), hold_exp(Ep, a_ep, "Ep"))
    cnan = c_with(d, np.nan)
    out = {}
    for mode in (RECIP, XVEC):
        res = ctx.table_pass(d["lum"], c.nR, c.nC, mode, rows=c.rows, hx=hx, hy=hy, c=cnan if mode == XVEC else None,
                             w=d["w"] if mode == RECIP else None, x=d["xvec"] if mode == XVEC else None)
        g, h, zpart, sr = _split_ws(c, res, lev[1])
        if mode == RECIP:
            out["g"] = check_g(g, er, Ep, d["w"], c.nR, c.nC, False, lev)
        m = tiles_mask(lev)
        assert np.isnan(h[:, :, ~m]).all() and np.isfinite(h[:, :, m]).all(), "h: the sorted rows write the level tiles that occur, and no other"
        out[f"z{mode}"] = check_z(zpart, _np(res["z"]), h, er, Ep, c.nR, c.nC, sr, False, lev)
        assert np.isfinite(_np(res["z"])).all()
    nl = min(2, b["layers_per_launch"])
    wl = expand_weights(c, nl, False)
    gws, planes = ctx.table_expand(d["lum"], c.nR, c.nC, wl, cnan, rows=c.rows, hx=hx, hy=hy)
    gws, planes = _np(gws), _np(planes).reshape(nl, c.nrows, c.W)
    for l in range(nl):
        out["gl"] = max(out.get("gl", 0.0), check_g(gws[l], er, Ep, wl[l, :c.p], c.nR, c.nC, False, lev))
        # (the sample pixels' slots hold whatever the sorted kernel's row buffer held: they are k_scatter_samples' to write, sorted.hip)
        assert np.isfinite(planes[l][d["ns"]]).all(), "the planes are finite off the sample pixels"
    Gk, ws, split = ctx.table_gram(d["lum"], c.nR, c.nC, cnan, rows=c.rows, hx=hx, hy=hy)
    out["gram"], w2 = check_gram_sums(_np(Gk), _np(ws), c, hx, Ep, split)
    wexp = max(wexp, w2)
    f = hist_g_launch(c.nR, c.nC, c.nrows, lev[1])
    print(f"table_kernels built {c.id} levels {lo}..{hi}: tiles {lev}, k_hist_g grid {f['gx']}x{f['gy']} idle waves {f['idle_waves']}, "
          f"k_ghist_gemm<4> nsplit {ghist_split(256 * (2 * c.nC - 1), gsum_ldm(c.nR), c.nrows)[1]}; exp outputs: largest err / (1e-14 ref) {wexp:.3g}; "
          "max err/bound " + ", ".join(f"{k} {v:.3g}" for k, v in out.items()))


LEVEL_N = (1, 2, 3, 5, 1027)


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_check_levels(nle, ctx, off):
    """k_check_levels at pointer offsets of 0 .. 3 floats: the scalar head, the 16-byte body, the scalar tail; one bad value
    (non-integer, negative, 256, NaN) in each; the tile mask bit for bit"""
    import torch
    rng = np.random.default_rng(off)
    for n in LEVEL_N:
        tiles = rng.choice(16, size=rng.integers(1, 5), replace=False)
        x = (16 * rng.choice(tiles, n) + rng.integers(0, 16, n)).astype(np.float32)
        x[0], x[-1] = 16 * tiles[0], 16 * tiles[-1] + 15
        mask = int(sum(1 << int(t) for t in set((x // 16).astype(int))))
        buf = torch.full((n + 8,), float("nan"), dtype=torch.float32, device="cuda")
        buf[off:off + n] = torch.as_tensor(x, device="cuda")
        assert ctx.table_levels(buf[off:off + n]) == (0, mask), (off, n)
        head = min((4 - off) & 3, n)                                   # the kernel's scalar head, then whole float4s, then the tail
        spots = sorted({0, max(head - 1, 0), min(head, n - 1), min(head + 4 * ((n - head) // 4), n - 1), n - 1, n // 2})
        for pos in spots:
            for bad in (7.5, -1.0, 256.0, float("nan")):
                keep = buf[off + pos].item()
                buf[off + pos] = bad
                rest = np.delete(x, pos)
                want = int(sum(1 << int(t) for t in set((rest // 16).astype(int))))
                assert ctx.table_levels(buf[off:off + n]) == (1, want), (off, n, pos, bad)
                buf[off + pos] = keep
    assert ctx.table_levels(torch.tensor([0.0, 255.0, 15.0, 16.0, 128.0], device="cuda")) == (0, 1 | 2 | 1 << 8 | 1 << 15)


def _refused(nle, ctx, call):
    with pytest.raises(nle.NLEError) as e:
        call()
    assert e.value.code == nle.NLE_ERR_INVALID
    assert (nle.lib().nle_last_error(ctx._h) or b"").decode().strip(), "nle_last_error must say what was refused"


@pytest.mark.gpu
@pytest.mark.parametrize("plane", [REFUSED_ROWS, REFUSED_COLS], ids=["33-rows", "37-columns"])
def test_refuses_a_grid_beyond_32_by_36(nle, ctx, plane):
    H, W, nr, nc = plane
    g = nle.sample_grid(H, W, nr, nc)
    nR, nC = g["n_sel_rows"], g["n_sel_cols"]
    lum = np.zeros((H, W), dtype=np.float32)
    tabs = (np.ones((H, nR)), np.ones((nC, W)), np.ones((256, nR * nC)))
    _refused(nle, ctx, lambda: ctx.table_pass(lum, nr, nc, COLSUM, tables=tabs))
    _refused(nle, ctx, lambda: ctx.table_pass(lum, nr, nc, COLSUM, hx=8.0, hy=30.0))
    _refused(nle, ctx, lambda: ctx.table_gram(lum, nr, nc, np.ones((H, W)), tables=tabs))
    _refused(nle, ctx, lambda: ctx.table_expand(lum, nr, nc, np.ones((1, nR * nC)), np.ones((H, W)), tables=tabs))
    _refused(nle, ctx, lambda: ctx.table_build(lum, nr, nc, 8.0, 30.0))


@pytest.mark.gpu
def test_refuses_more_than_128_eigenvectors(nle, ctx):
    m, D, V, xA, resp, _, _ = small_inputs(129, 7, 1, True)
    _refused(nle, ctx, lambda: ctx.table_apply_small(m, np.nan_to_num(D), np.nan_to_num(V), xA, resp, 64))


@pytest.mark.gpu
@pytest.mark.parametrize("nC", [17, 18, 24, 36])
def test_refuses_more_layers_than_a_launch_takes(nle, ctx, nC):
    c = NC_CASES[nC - 1]
    d = inputs(c, True)
    wl = expand_weights(c, layers_per_launch(nC) + 1, True)
    _refused(nle, ctx, lambda: ctx.table_expand(d["lum"], c.nR, c.nC, wl, c_with(d, np.nan), rows=c.rows, tables=(d["er"], d["ecT"], d["Ep"])))


@pytest.mark.gpu
def test_built_view_refuses_a_plane_that_is_not_integer_valued(nle, ctx):
    lum = np.full((16, 16), 7.5, dtype=np.float32)
    _refused(nle, ctx, lambda: ctx.table_build(lum, 2, 2, 8.0, 30.0))


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [7.5, -1.0, 256.0, float("nan")])
def test_supplied_view_refuses_local_rows_that_hold_no_levels(nle, ctx, bad):
    """the pixel kernels index LDS with the level: a supplied view is checked (check_levels over the local rows) before any launch;
    a bad value outside the local rows is nobody's business"""
    c = Case(2, 3, 4, row0=2, W=13, H=12)
    d = inputs(c, True)
    tabs, cv = (d["er"], d["ecT"], d["Ep"]), c_with(d, np.nan)
    lum = d["lum"].copy()
    lum[c.row0 + 1, 5] = bad
    _refused(nle, ctx, lambda: ctx.table_pass(lum, c.nR, c.nC, COLSUM, rows=c.rows, tables=tabs))
    _refused(nle, ctx, lambda: ctx.table_gram(lum, c.nR, c.nC, cv, rows=c.rows, tables=tabs))
    _refused(nle, ctx, lambda: ctx.table_expand(lum, c.nR, c.nC, expand_weights(c, 1, True), cv, rows=c.rows, tables=tabs))
    lum = d["lum"].copy()
    lum[0, 0], lum[c.row0 + c.nrows, 3] = bad, bad
    res = ctx.table_pass(lum, c.nR, c.nC, COLSUM, rows=c.rows, tables=tabs)
    assert np.isfinite(_np(res["z"])).all()
