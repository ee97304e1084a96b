"""The exact filter's operator and train beyond one launch segment (csrc/exact.hip, csrc/exact_train.hip).

tests/test_exact_filter.py stops at 64 x 64 and 1 x 3000, where every launch of exact.hip is its simplest one.  Here the
planes are the smallest at which the launchers take their other branches: a second (third, ... 36th) source segment that
adds into Y, a partial last stage, the spatial table read from global memory, fewer than 16 sub-segments of the narrow
form, and a train whose block and Sinkhorn products run through those branches on buffers that are not fresh.

`exact_plan` restates the dispatch; a CPU test holds its constants to the source and another one holds every GPU case to
the branch it is named after, so a changed budget fails there and moves no case off its branch silently.

Two references for Y = K X, neither storing K:
  (a) `kron_ref`: on a plane whose level depends on the row only (or on the column only) K = A (x) B with
      A[r, r'] = exp(-sw (r-r')^2 - pw (g_r-g_r')^2) and B[c, c'] = exp(-sw (c-c')^2) (the exponent summed before the exp,
      no table of the kernel's), so Y = A X B^T column by column: every entry of Y.
  (b) `rows_ref`: whole rows k_i = exp(-sw d^2 - pw dy^2) and k_i @ X for a fixed set of output pixels, any plane.
Per entry |Y - ref| <= (N + H + W + 16) 2^-53 S for (a) and (2 N + 16) 2^-53 S for (b), S_ic = sum_j K_ij |X_jc| from the
same reference: N for the longest addition chain of either kernel, the rest for the reference's own sums and the
three-factor table product.  A worst-case bound from the arithmetic; the measured ratios err / (2^-53 S) are printed.
On the two 45 100-pixel lines S is replaced by the smaller sum_j K_ij (every |X| is >= 1), which only tightens the bound
and spares the reference 130 columns; there the kind across the line is a constant plane, for which (a) would cost the
same again and say little more: it is held to (b).

The train is held to a closed form: with hx so large that every spatial factor is 1.0 in fp64, K = P K_l P^T for the
N x m level indicator P, and Sinkhorn, Ws and its eigenpairs collapse to m x m (`level_closed_form`)."""
import os
import re
import time

import numpy as np
import pytest

from conftest import ROOT, rel_l2
from test_exact_filter import EPS, dense_K, inplace_reciprocal, layers, restatement, sign_rule, train

U = 2.0 ** -53

# ------------------------------------------------------------------------------------------ the mirror of the dispatch
K_TAB_LDS, K_MFMA_SRC, K_NARROW_SRC, K_MAX_SUB = 4096, 32, 256, 16
K_MFMA_FLOP, K_NARROW_AFF = 1.0e12, 1.0e11
K_SUB_GROUPS = 2048              # workgroups the narrow form aims for
NT_LIMITS = ((16, 1), (32, 2), (64, 4))  # ncols <= limit -> NT; above: 8


def exact_plan(H, W, ncols):
    """product_tab / launch_mfma / launch_narrow of csrc/exact.hip"""
    N = H * W
    plan = dict(tab_lds=max(H, W) <= K_TAB_LDS)
    if ncols <= 2:
        nb = (N + 255) // 256
        nsub = min(K_MAX_SUB, max(1, K_SUB_GROUPS // nb))
        seg = max(K_NARROW_SRC, int(K_NARROW_AFF / float(N)))
        segs = [(s, min(N, s + seg)) for s in range(0, N, seg)]
        plan.update(form="narrow", nc=ncols, cblocks=1, stage=K_NARROW_SRC, segments=segs, nsub=nsub,
                    sub_len=[(s1 - s + nsub - 1) // nsub for s, s1 in segs])
        return plan
    nt = next((t for lim, t in NT_LIMITS if ncols <= lim), 8)
    cblocks = (ncols + nt * 16 - 1) // (nt * 16)
    seg = int(K_MFMA_FLOP / (2.0 * float(N) * cblocks * nt * 16))
    seg = max(K_MFMA_SRC, seg // K_MFMA_SRC * K_MFMA_SRC)
    plan.update(form="mfma", nt=nt, cblocks=cblocks, stage=K_MFMA_SRC, segments=[(s, min(N, s + seg)) for s in range(0, N, seg)])
    return plan


def _L(H, W, ncols, **claims):
    return (H, W, ncols, claims)


def _mfma(nt, cblocks, tab, nseg, seg, tail, partial):
    return dict(form="mfma", nt=nt, cblocks=cblocks, tab_lds=tab, nseg=nseg, seg=seg, tail=tail, partial=partial)


def _narrow(nc, tab, nseg, seg, tail, partial, nsub, sub_len):
    return dict(form="narrow", nc=nc, cblocks=1, tab_lds=tab, nseg=nseg, seg=seg, tail=tail, partial=partial, nsub=nsub,
                sub_len=sub_len)


_NT8X2 = _mfma(8, 2, False, 2, 43296, 1804, True)
# id -> launches (H, W, ncols, what the launch reaches: segment count, full segment, last segment, whether the last segment
# ends in a partial stage, TAB_LDS, and for the narrow form nsub and sub_len per segment)
CASES = {
    "nt8x2-tall": [_L(4100, 11, 130, **_NT8X2)],
    "nt8x2-wide": [_L(11, 4100, 130, **_NT8X2)],
    "nt8x2-line": [_L(1, 45100, 130, **_NT8X2), _L(45100, 1, 130, **_NT8X2)],
    # 300 x 296 ends on a whole stage; 300 x 297 is the same branch with a partial one
    "nt4": [_L(300, 296, 64, **_mfma(4, 1, True, 2, 87968, 832, False)), _L(300, 297, 64, **_mfma(4, 1, True, 2, 87680, 1420, True))],
    "nt2": [_L(354, 354, 17, **_mfma(2, 1, True, 2, 124672, 644, True))],
    "nt1": [_L(421, 421, nc, **_mfma(1, 1, True, 2, 176288, 953, True)) for nc in (3, 16)],
    "many": [_L(256, 512, 130, **_mfma(8, 2, True, 9, 14880, 12032, False))],
    "narrow-2seg": [_L(H, W, nc, **_narrow(nc, tab, 2, 312500, 7500, True, 1, [312500, 7500]))
                    for H, W, tab in ((800, 400, True), (5000, 64, False)) for nc in (1, 2)],
    # 3 x 7: 16 sub-segments of 2 sources, of which the last five are empty
    "nsub-16-15": [_L(128, 256, nc, **_narrow(nc, True, 1, 32768, 32768, False, 16, [2048])) for nc in (1, 2)] +
                  [_L(99, 331, nc, **_narrow(nc, True, 1, 32769, 32769, True, 15, [2185])) for nc in (1, 2)] +
                  [_L(3, 7, nc, **_narrow(nc, True, 1, 21, 21, True, 16, [2])) for nc in (1, 2)],
    "nsub-2-1": [_L(512, 512, 1, **_narrow(1, True, 1, 262144, 262144, False, 2, [131072])),
                 _L(517, 508, 1, **_narrow(1, True, 1, 262636, 262636, True, 1, [262636]))],
    "cap-narrow": [_L(1024, 1024, nc, **_narrow(nc, True, 11, 95367, 94906, True, 1, [95367] * 10 + [94906])) for nc in (1, 2)],
    "cap-mfma": [_L(1024, 1024, 3, **_mfma(1, 1, True, 36, 29792, 5856, False))],
}
DECAYING_TOO = ("many", "narrow-2seg")
REPRODUCIBLE = ("nt8x2-tall", "many", "narrow-2seg")
# (case, kind of plane): the general kind (reference (b)) everywhere but at the cap, where (a) alone is enough
# and the decaying family on two ids
OPERATOR_TESTS = [(c, k, f) for c in CASES for k in ("row", "col", "gen") if not (k == "gen" and c.startswith("cap-"))
                  for f in (("sensitive", "decaying") if c in DECAYING_TOO else ("sensitive",))]
# the trains: (H, W, T, K); the 32-column block products and the one-column Sinkhorn products
TRAINS = {"360x360": (360, 360, 3, 8), "800x400": (800, 400, 1, 4)}
TRAIN_HX, TRAIN_HY, TRAIN_LEVELS = 1.0e12, 20.0, np.arange(10.0, 241.0, 10.0)


# ------------------------------------------------------------------------------------------ inputs
def family_bandwidths(family, H, W):
    """(hx, hy): sensitive -- hx the plane's diagonal at least, so with levels 128 apart at most and hy = 80 every affinity of
    the plane is >= exp(-1) exp(-2.56) = 0.028 and one source pixel lost or doubled moves every entry; decaying -- far table
    entries 0 or denormal, levels over all of 0..255"""
    return (float(np.ceil(np.hypot(H, W))), 80.0) if family == "sensitive" else (7.0, 25.0)


def make_plane(family, kind, H, W):
    """integer levels; kind row / col: a function of the row / column only, gen: a level of its own per pixel"""
    rng = np.random.default_rng([H, W, {"row": 0, "col": 1, "gen": 2}[kind], family == "sensitive"])
    lo, hi = (64, 192) if family == "sensitive" else (0, 255)
    n = {"row": H, "col": W, "gen": H * W}[kind]
    g = rng.integers(lo, hi + 1, size=n).astype(np.float64)
    g[0], g[-1] = lo, hi  # both ends of the band are there (one of them when n == 1)
    if kind == "row":
        return np.repeat(g[:, None], W, axis=1)
    if kind == "col":
        return np.repeat(g[None, :], H, axis=0)
    return g.reshape(H, W)


def make_X(H, W, ncols):
    """+-(1 + U[0, 1)): no entry near zero"""
    rng = np.random.default_rng([H * W, ncols, 77])
    return np.where(rng.random((H * W, ncols)) < 0.5, -1.0, 1.0) * (1.0 + rng.random((H * W, ncols)))


def tables(H, W, hx, hy):
    sw, pw = 1.0 / (hx * hx), 1.0 / (hy * hy)
    d = np.arange(max(H, W), dtype=np.float64)
    l = np.arange(256, dtype=np.float64)
    return np.exp(-sw * d * d), np.exp(-pw * l * l)


# ------------------------------------------------------------------------------------------ the references
def factor_apply(g, sw, pw, Z):
    """M @ Z for M[i, j] = exp(-sw (i-j)^2 - pw (g_i-g_j)^2), made 2048 rows at a time from the summed exponent; M is symmetric,
    so only its blocks on and right of the diagonal are made"""
    import torch
    n = g.numel()
    idx = torch.arange(n, dtype=torch.float64)
    out = torch.zeros_like(Z)
    for i0 in range(0, n, 2048):
        i1 = min(n, i0 + 2048)
        E = idx[i0:i1, None] - idx[None, i0:]
        E.mul_(E).mul_(-sw)
        D = g[i0:i1, None] - g[None, i0:]
        D.mul_(D).mul_(pw)
        E.sub_(D).exp_()
        out[i0:i1] += E @ Z[i0:]
        if i1 < n:
            out[i1:] += E[:, i1 - i0:].T @ Z[i0:i1]
    return out


def kron_ref(y, hx, hy, X, s_lower=False):
    """reference (a): (K X, S) for a plane that is a function of the row only or of the column only; S = K |X|, or with
    s_lower K 1 in one column"""
    import torch
    H, W = y.shape
    assert np.array_equal(y, np.repeat(y[:, :1], W, axis=1)) or np.array_equal(y, np.repeat(y[:1], H, axis=0))
    row_kind = np.array_equal(y, np.repeat(y[:, :1], W, axis=1))
    gr = torch.from_numpy(np.ascontiguousarray(y[:, 0] if row_kind else np.zeros(H)))
    gc = torch.from_numpy(np.ascontiguousarray(np.zeros(W) if row_kind else y[0]))
    sw, pw = 1.0 / (hx * hx), 1.0 / (hy * hy)
    def both_factors(Z):
        m = Z.shape[1]
        Z = factor_apply(gr, sw, pw, Z.reshape(H, W * m))
        Z = Z.reshape(H, W, m).permute(1, 0, 2).reshape(W, H * m)
        return factor_apply(gc, sw, pw, Z).reshape(W, H, m).permute(1, 0, 2).reshape(H * W, m).numpy()
    # K X in products of its own: a host BLAS may round a column differently when the matrix it stands in has other
    # columns beside it, and K X must not depend on which S is asked for
    Xt = torch.from_numpy(X)
    KX, S = both_factors(Xt), both_factors(torch.ones(H * W, 1, dtype=torch.float64) if s_lower else Xt.abs())
    return KX, (np.repeat(S, X.shape[1], axis=1) if s_lower else S)


def rows_ref(y, hx, hy, rows, X):
    """reference (b): (K X, K |X|) at the output pixels `rows`, whole rows of K from the definition"""
    import torch
    H, W = y.shape
    N = H * W
    sw, pw = 1.0 / (hx * hx), 1.0 / (hy * hy)
    f = torch.from_numpy(y.astype(np.float64).ravel())
    r, c = torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64)
    Z = torch.cat([torch.from_numpy(X), torch.from_numpy(np.abs(X))], dim=1)
    rows = torch.as_tensor(np.asarray(rows, dtype=np.int64))
    out = []
    for k0 in range(0, rows.numel(), 64):
        i = rows[k0:k0 + 64]
        dr = (i // W).to(torch.float64)[:, None] - r[None]  # per source row and per source column: the exponent is summed
        dc = (i % W).to(torch.float64)[:, None] - c[None]   # before the exp all the same
        E = ((-sw * dr * dr)[:, :, None] + (-sw * dc * dc)[:, None, :]).reshape(i.numel(), N)
        dy = f[i, None] - f[None]
        E.add_(dy.mul_(dy), alpha=-pw).exp_()
        out.append(E @ Z)
    out = torch.cat(out).numpy()
    return out[:, :X.shape[1]], out[:, X.shape[1]:]


def seams_of(plan, N):
    """source indices at which a segment ends and the next begins, and for the narrow form the first and the last boundary
    between its 256-pixel blocks of output pixels"""
    seams = [s1 for _, s1 in plan["segments"][:-1]]
    if plan["form"] == "narrow":
        seams += [256 * k for k in sorted({1, (N - 1) // 256}) if 0 < 256 * k < N]
    return seams


def pick_rows(plan, N):
    """output pixels for reference (b): the first 64, the last (partial) workgroup (of a 256-pixel block of the narrow form
    the first 8 and the last 56), 64 across every segment seam, 64 across the narrow form's first and last block seam, 64 at
    random.  320 to 400 rows at two segments, 704 at nine (256 x 512, where they cost a second of CPU)"""
    g = 64 if plan["form"] == "mfma" else 256
    last0 = (N - 1) // g * g
    rows = set(range(min(64, N))) | set(range(last0, min(N, last0 + 8))) | set(range(max(last0, N - 56), N))
    for s in seams_of(plan, N):
        rows |= set(range(max(0, s - 32), min(N, s + 32)))
    rows |= set(np.random.default_rng(N).integers(0, N, size=64).tolist())
    return np.array(sorted(rows), dtype=np.int64)


def across(H, W, kind):
    """the kind across a one-pixel-wide line: a constant plane"""
    return (kind == "row" and H == 1) or (kind == "col" and W == 1)


def case_rows(case, H, W):
    """ncols -> the rows of reference (b) for every launch of the case on this plane, each from the launch's own plan"""
    return {nc: pick_rows(exact_plan(h, w, nc), H * W) for h, w, nc, _ in CASES[case] if (h, w) == (H, W)}


def held(Y, ref, S, c, what):
    """every entry within c 2^-53 S; returns the largest err / (2^-53 S)"""
    assert Y.shape == ref.shape == S.shape
    err = np.abs(Y - ref)
    ratio = float(np.max(err / (U * S)))
    print(f"{what}: max err / (2^-53 S) = {ratio:.2f} (bound {c})")
    bad = ~(err <= c * U * S)  # a NaN is bad
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), ratio, c)
    return ratio


# ------------------------------------------------------------------------------------------ the train's closed form
def level_plane(H, W):
    """24 levels 10, 20, ..., 240 drawn per pixel with unequal probabilities"""
    rng = np.random.default_rng([H, W, 24])
    p = 0.3 + np.arange(TRAIN_LEVELS.size) % 5
    return rng.choice(TRAIN_LEVELS, size=(H, W), p=p / p.sum())


def level_closed_form(y, hy, T, K):
    """(kept eigenvalues, their eigenvectors N x K', all m eigenvalues descending) of the exact filter on a plane whose
    spatial factors are all 1.0: K = P K_l P^T, so Sinkhorn acts on level vectors with the counts as weights,
    S = (diag(r) K_l diag(c) + its transpose) / 2, the eigenvalues are those of D^1/2 S D^1/2 with D = diag(counts) and the
    eigenvectors are P D^-1/2 w"""
    lv, inv, n = np.unique(np.asarray(y, dtype=np.float64).ravel(), return_inverse=True, return_counts=True)
    n = n.astype(np.float64)
    Kl = np.exp(-(lv[:, None] - lv[None]) ** 2 / (hy * hy))
    r = np.ones(lv.size)
    for _ in range(T):
        c = inplace_reciprocal(Kl @ (n * r))
        r = inplace_reciprocal(Kl @ (n * c))
    S = 0.5 * (r[:, None] * Kl * c[None] + c[:, None] * Kl * r[None])
    w, Wv = np.linalg.eigh(np.sqrt(n)[:, None] * S * np.sqrt(n)[None])
    order = np.argsort(w)[::-1]
    w, Wv = w[order], Wv[:, order]
    kept = 0
    while kept < min(K, w.size) and w[kept] >= EPS:
        kept += 1
    V = (Wv[:, :kept] / np.sqrt(n)[:, None])[inv.ravel()]
    return w[:kept].copy(), sign_rule(V), w


# ------------------------------------------------------------------------------------------ CPU tests
def test_mirror_constants_are_the_sources():
    with open(os.path.join(ROOT, "nonlocal-image-edit_amd", "csrc", "exact.hip")) as f:
        src = f.read()

    def const(name):
        return float(re.search(r"constexpr (?:int|double) %s = ([0-9.e+]+);" % name, src).group(1))

    assert [const(n) for n in ("kExactTabLds", "kMfmaSrc", "kNarrowSrc", "kMaxSub", "kMfmaFlopPerLaunch", "kNarrowAffPerLaunch")] == \
        [K_TAB_LDS, K_MFMA_SRC, K_NARROW_SRC, K_MAX_SUB, K_MFMA_FLOP, K_NARROW_AFF]
    assert [(int(a), int(b)) for a, b in re.findall(r"if \(ncols <= (\d+)\) return launch_mfma<(\d), TAB>", src)] == list(NT_LIMITS)
    assert "return launch_mfma<8, TAB>(st, pl, X, ldx, ncols, Y, ldy);" in src
    assert [int(a) for a in re.findall(r"if \(ncols == (\d)\) return launch_narrow<\1, TAB>", src)] == [1, 2]
    assert "return pl.es_len <= kExactTabLds ? product_tab<true>" in src
    # launch_mfma
    assert "const int cblocks = (ncols + NT * 16 - 1) / (NT * 16);" in src
    assert "const double flop_per_src = 2.0 * (double)N * cblocks * NT * 16;" in src
    assert "long long seg = (long long)(kMfmaFlopPerLaunch / flop_per_src);" in src
    assert "seg = std::max<long long>(kMfmaSrc, (seg / kMfmaSrc) * kMfmaSrc);" in src
    # launch_narrow
    assert "const int nsub = (int)std::min<long long>(kMaxSub, std::max<long long>(1, %d / nb));" % K_SUB_GROUPS in src
    assert "long long seg = (long long)(kNarrowAffPerLaunch / (double)N);" in src
    assert "seg = std::max<long long>(kNarrowSrc, seg);" in src
    assert "const long long sub = (s1 - s + nsub - 1) / nsub;" in src
    assert src.count("s > 0 ? 1 : 0") == 2  # both forms: the first segment stores, the later ones add


def test_every_case_takes_the_branch_it_is_named_after():
    for case, launches in CASES.items():
        for H, W, ncols, claims in launches:
            plan = exact_plan(H, W, ncols)
            N, segs = H * W, plan["segments"]
            assert N <= 1 << 20 and segs[0][0] == 0 and segs[-1][1] == N
            assert all(a[1] == b[0] for a, b in zip(segs, segs[1:]))  # no source pixel dropped or doubled by the mirror
            got = dict(form=plan["form"], cblocks=plan["cblocks"], tab_lds=plan["tab_lds"], nseg=len(segs),
                       seg=segs[0][1] - segs[0][0], tail=segs[-1][1] - segs[-1][0],
                       partial=(segs[-1][1] - segs[-1][0]) % plan["stage"] != 0)
            if plan["form"] == "mfma":
                got["nt"] = plan["nt"]
            else:
                got.update(nc=plan["nc"], nsub=plan["nsub"], sub_len=plan["sub_len"])
            assert got == claims, (case, H, W, ncols, got, claims)
    # what the ids say, over the whole table
    every = {c: [cl for _, _, _, cl in l] for c, l in CASES.items()}
    assert all(cl["nseg"] >= 2 for c in every if not c.startswith("nsub") for cl in every[c])
    assert all(not cl["tab_lds"] for c in ("nt8x2-tall", "nt8x2-wide", "nt8x2-line") for cl in every[c])
    assert {cl["tab_lds"] for cl in every["narrow-2seg"]} == {True, False}
    assert {cl["nt"] for c in every for cl in every[c] if cl["form"] == "mfma"} == {1, 2, 4, 8}
    assert all(any(cl["partial"] for cl in every[c]) for c in ("nt8x2-tall", "nt4", "nt2", "nt1", "narrow-2seg"))
    assert {cl["nsub"] for c in every for cl in every[c] if cl["form"] == "narrow"} == {16, 15, 2, 1}
    H, W, _, _ = CASES["nsub-16-15"][-1]  # the last sub-segments of 3 x 7 are empty, the last one of 99 x 331 is short
    assert 11 * 2 >= H * W and 14 * 2185 < 99 * 331 < 15 * 2185
    # the trains: the block products (2 b = 32 columns) and the Sinkhorn products (one column, ldx = 1)
    p = exact_plan(360, 360, 32)
    assert (p["form"], p["nt"], p["segments"]) == ("mfma", 2, [(0, 120544), (120544, 129600)])
    p = exact_plan(360, 360, 1)
    assert (p["form"], len(p["segments"]), p["nsub"]) == ("narrow", 1, 4)
    p = exact_plan(800, 400, 32)
    assert (p["form"], p["nt"], len(p["segments"])) == ("mfma", 2, 7)
    p = exact_plan(800, 400, 1)
    assert (p["form"], p["segments"], p["nsub"]) == ("narrow", [(0, 312500), (312500, 320000)], 1)
    with open(os.path.join(ROOT, "nonlocal-image-edit_amd", "csrc", "exact_train.hip")) as f:
        src = f.read()
    # K = 8 and K = 4 give b = 16: 32-column block products; Y is one un-zeroed buffer for all of them
    assert "b(std::min(64, std::max(16, (nev + 15) / 16 * 16)))" in src and "op.product(Z.p, 2 * b, 2 * b, Y.p, 2 * b);" in src
    assert "op.product(d_r.p, 1, 1, d_c.p, 1);" in src and "op.product(d_c.p, 1, 1, d_r.p, 1);" in src


def test_input_conditions_hold():
    for case, launches in CASES.items():
        for H, W, _, _ in launches:
            hx, hy = family_bandwidths("sensitive", H, W)
            es, el = tables(H, W, hx, hy)
            assert hx >= np.hypot(H - 1, W - 1)
            assert es[H - 1] * es[W - 1] * el[192 - 64] >= 0.01  # the smallest affinity of the plane
            for kind in ("row", "col", "gen"):
                y = make_plane("sensitive", kind, H, W)
                assert y.min() >= 64 and y.max() <= 192 and np.array_equal(y, np.round(y))
                assert (y.min() == y.max()) == (across(H, W, kind) or H * W == 1)
    for case in DECAYING_TOO:
        for H, W, _, _ in CASES[case]:
            hx, hy = family_bandwidths("decaying", H, W)
            es, el = tables(H, W, hx, hy)
            assert es[-1] == 0.0 and np.any((es > 0) & (es < 2.3e-308)) and 0 < el[255] < 1e-40
            for kind in ("row", "col", "gen"):
                y = make_plane("decaying", kind, H, W)
                assert y.min() == 0 and y.max() == 255  # index 255 of El is used
    X = make_X(37, 53, 5)
    assert np.abs(X).min() >= 1.0 and np.abs(X).max() < 2.0 and (X > 0).any(axis=0).all() and (X < 0).any(axis=0).all()
    for H, W, _, _ in TRAINS.values():  # every spatial factor of the trains is 1.0
        es, _ = tables(H, W, TRAIN_HX, TRAIN_HY)
        assert np.all(es == 1.0) and np.exp(-((H - 1.0) ** 2 + (W - 1.0) ** 2) / TRAIN_HX ** 2) == 1.0
        assert np.unique(level_plane(H, W)).size == 24


@pytest.mark.parametrize("family", ["sensitive", "decaying"])
def test_the_references_agree_with_each_other_and_with_dense_K(family):
    H, W, nc = 37, 53, 3
    N = H * W
    hx, hy = family_bandwidths(family, H, W)
    X = make_X(H, W, nc)
    for kind in ("row", "col"):
        y = make_plane(family, kind, H, W)
        Kd = dense_K(y, hx, hy)
        want, S = Kd @ X, Kd @ np.abs(X)
        a, Sa = kron_ref(y, hx, hy, X)
        rows = pick_rows(exact_plan(H, W, nc), N)
        b, Sb = rows_ref(y, hx, hy, rows, X)
        held(a, want, S, N + H + W + 16, f"{family} {kind}: (a) against dense K")
        held(b, want[rows], S[rows], 2 * N + 16, f"{family} {kind}: (b) against dense K")
        held(a[rows], b, Sb, 2 * N + 16, f"{family} {kind}: (a) against (b)")
        assert np.max(np.abs(Sa - S) / S) <= (N + H + W + 16) * U and np.max(np.abs(Sb - S[rows]) / S[rows]) <= (2 * N + 16) * U
        lo, Slo = kron_ref(y, hx, hy, X, s_lower=True)
        assert np.array_equal(lo, a) and np.all(Slo <= Sa * (1 + 64 * U)) and np.all(2 * Slo >= Sa * (1 - 64 * U))
    y = make_plane(family, "gen", H, W)
    Kd = dense_K(y, hx, hy)
    rows = pick_rows(exact_plan(H, W, 1), N)
    # the narrow form's last block, 1792 .. 1960: its first 8 and last 56 pixels
    assert rows[0] == 0 and rows[-1] == N - 1 and np.all(np.isin(np.r_[1792:1800, N - 56:N], rows))
    b, Sb = rows_ref(y, hx, hy, rows, X)
    held(b, (Kd @ X)[rows], (Kd @ np.abs(X))[rows], 2 * N + 16, f"{family} gen: (b) against dense K")


def test_pick_rows_covers_what_it_names():
    p = exact_plan(256, 512, 130)
    rows = set(pick_rows(p, 256 * 512).tolist())
    assert set(range(64)) <= rows and set(range(131072 - 64, 131072)) <= rows and len(rows) <= 704
    assert all(set(range(k * 14880 - 32, k * 14880 + 32)) <= rows for k in range(1, 9))
    p = exact_plan(800, 400, 2)
    rows = set(pick_rows(p, 320000).tolist())
    assert set(range(312500 - 32, 312500 + 32)) <= rows and set(range(256 - 32, 256 + 32)) <= rows
    assert set(range(1249 * 256 - 32, 1249 * 256 + 32)) <= rows and len(rows) <= 400
    p = exact_plan(4100, 11, 130)  # the last workgroup of the MFMA form is partial: 45 100 = 704 * 64 + 44
    assert set(range(704 * 64, 45100)) <= set(pick_rows(p, 45100).tolist())


def test_the_rows_of_every_case_straddle_the_seams_of_its_own_plan():
    """what the GPU cases compare against reference (b), launch by launch: `case_rows` is what they call"""
    seen = 0
    for case, kind, family in OPERATOR_TESTS:
        for H, W, ncols, claims in CASES[case]:
            if kind != "gen" and not across(H, W, kind):
                continue
            N = H * W
            plan = exact_plan(H, W, ncols)
            rows = set(case_rows(case, H, W)[ncols].tolist())
            seams = seams_of(plan, N)
            assert len([s for s in seams if s in {s1 for _, s1 in plan["segments"]}]) == claims["nseg"] - 1
            assert all(set(range(max(0, s - 32), min(N, s + 32))) <= rows for s in seams), (case, H, W, ncols)
            g = 64 if plan["form"] == "mfma" else 256
            assert set(range(min(64, N))) <= rows and {(N - 1) // g * g, N - 1} <= rows and len(rows) <= 704
            seen += claims["nseg"] - 1
    assert seen >= 2 * 8 + 8 + 9 + 2  # many, narrow-2seg (two families each), the two-segment MFMA launches, the lines across


def test_closed_form_matches_the_restatement():
    y = level_plane(20, 35)
    assert np.unique(y).size == 24
    for T, K in ((3, 8), (1, 4)):
        w, V, wall = restatement(y, TRAIN_HX, TRAIN_HY, T, 30)
        wc, Vc, wl = level_closed_form(y, TRAIN_HY, T, 30)
        assert w.size == wc.size == 24 and wl.size == 24  # rank 24: the rest of the spectrum is rounding
        assert np.max(np.abs(w - wc)) <= 1e-13 and np.max(np.abs(wall[24:])) <= 1e-13
        gaps = np.minimum(np.r_[np.inf, wl[:-1] - wl[1:]], np.r_[wl[:-1] - wl[1:], np.inf])
        sep = gaps >= 1e-3
        assert sep[:K].all() and np.max(np.abs(V[:, sep] - Vc[:, sep])) <= 1e-9
        assert np.allclose(np.sum(Vc * Vc, axis=0), 1.0, atol=1e-13)


def test_the_trains_spectra_are_separated():
    for H, W, T, K in TRAINS.values():
        w, V, wl = level_closed_form(level_plane(H, W), TRAIN_HY, T, K)
        assert w.size == K and wl.size == 24 and wl[-1] >= 1e-6
        assert np.min((wl[:K] - wl[1:K + 1]) / wl[:K]) >= 0.01, wl[:K + 1]


# ------------------------------------------------------------------------------------------ GPU tests
@pytest.fixture(scope="module")
def sctx(nle):
    """a context of this module's own"""
    c = nle.Context(0)
    yield c
    c.close()


_refs = {}


def reference(case, family, kind, H, W):
    """computed once per plane and shared by the launches on it (X as wide as the widest launch; a launch takes its leading
    columns): reference (b) for the general kind and for the constant plane across a line, else (a).  A 1 x n plane of the
    column kind is the n x 1 plane of the row kind transposed, with the same X: one reference"""
    if kind == "col" and H == 1:
        y, *rest = reference(case, family, "row", W, 1)
        return (np.ascontiguousarray(y.T), *rest)
    key = (case, family, kind, H, W)
    if key not in _refs:
        y = make_plane(family, kind, H, W)
        hx, hy = family_bandwidths(family, H, W)
        rows = case_rows(case, H, W)
        X = make_X(H, W, max(rows))
        t0 = time.perf_counter()
        if kind == "gen" or across(H, W, kind):
            allr = np.unique(np.concatenate(list(rows.values())))
            ref, S = rows_ref(y, hx, hy, allr, X)
        else:
            allr, rows = None, None
            ref, S = kron_ref(y, hx, hy, X, s_lower=max(H, W) > 8192)
        print(f"reference {key}: {time.perf_counter() - t0:.2f} s")
        _refs[key] = (y, hx, hy, X, ref, S, allr, rows)
    return _refs[key]


def product(ctx, y, X, hx, hy):
    import torch
    t0 = time.perf_counter()
    Y = ctx.affinity_product64(y.astype(np.float32), X, hx, hy)
    torch.cuda.synchronize()
    return Y.cpu().numpy(), time.perf_counter() - t0


@pytest.mark.gpu
@pytest.mark.parametrize("case,kind,family", OPERATOR_TESTS, ids=["%s-%s-%s" % ckf for ckf in OPERATOR_TESTS])
def test_affinity_product_beyond_one_segment(nle, sctx, case, kind, family):
    worst = {}
    for n, (H, W, ncols, claims) in enumerate(CASES[case]):
        N = H * W
        y, hx, hy, X, ref, S, allr, rows = reference(case, family, kind, H, W)
        Xc = np.ascontiguousarray(X[:, :ncols])
        Y, sec = product(sctx, y, Xc, hx, hy)
        what = f"{case} {family} {kind} {H}x{W} ncols {ncols} ({sec:.3f} s)"
        if rows is not None:
            r = rows[ncols]
            at = np.searchsorted(allr, r)
            ratio = held(Y[r], ref[at, :ncols], S[at, :ncols], 2 * N + 16, what)
        else:
            ratio = held(Y, ref[:, :ncols], S[:, :ncols], N + H + W + 16, what)
        worst[claims["form"]] = max(worst.get(claims["form"], 0.0), ratio)
        if case in REPRODUCIBLE and n == 0:
            assert np.array_equal(Y, product(sctx, y, Xc, hx, hy)[0])
    assert worst
    print(f"{case} {kind} {family}: largest err / (2^-53 S) per form {worst}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TRAINS))
def test_exact_train_beyond_one_segment(nle, oracle, sctx, name):
    import torch
    H, W, T, K = TRAINS[name]
    L = 4
    y = level_plane(H, W)
    w, V, wl = level_closed_form(y, TRAIN_HY, T, K)
    assert w.size == K
    # a 130-column product on the same context directly before training: what the first train allocates is not fresh by
    # luck, and the second train follows on what the first one freed
    product(sctx, y, make_X(H, W, 130), TRAIN_HX, TRAIN_HY)
    out = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f, Y = train(nle, sctx, y, TRAIN_HX, TRAIN_HY, T, K, L)
        sec = time.perf_counter() - t0
        out.append((f, Y, f.eigvals.copy(), f.eigvecs().cpu().numpy().astype(np.float64)[:, :K]))
        print(f"train {name}: {sec:.2f} s, timings {f.timings()}")
    (f, Y, ev, Vg), (f2, Y2, ev2, Vg2) = out
    assert np.array_equal(ev, ev2) and np.array_equal(Vg, Vg2) and np.array_equal(Y, Y2)
    assert f.diag() == {"formulation": 6, "p": 0, "r_Ka": 0, "r_Wa": 0, "r_Q": K, "K": K, "chol_Ka": 0, "chol_Wa": 0}
    assert ev.size == K and np.max(np.abs(ev - w)) <= 1e-9, np.max(np.abs(ev - w))
    # unit norms: the copy handed out is fp32, each entry within 2^-24 of the fp64 one, and so is the norm
    assert np.max(np.abs(np.sqrt(np.sum(Vg * Vg, axis=0)) - 1.0)) <= 2.0 ** -24 + 1e-10
    for k in range(K):  # the sign rule; every pair is separated (test_the_trains_spectra_are_separated)
        assert Vg[int(np.argmax(np.abs(Vg[:, k]))), k] > 0
        assert min(np.inf if k == 0 else wl[k - 1] - wl[k], wl[k] - wl[k + 1]) >= 1e-3
        assert np.max(np.abs(Vg[:, k] - V[:, k])) <= 1e-6, (k, np.max(np.abs(Vg[:, k] - V[:, k])))
    Y_ref = layers(oracle, w, V, y, L)
    errs = [rel_l2(Y[j], Y_ref[j]) for j in range(L)]
    assert max(errs) <= 1e-6, errs
    print(f"train {name}: eigenvalues {np.max(np.abs(ev - w)):.1e}, eigenvectors {np.max(np.abs(Vg - V)):.1e}, per-layer "
          + str(["%.1e" % e for e in errs]))
    f.close()
    f2.close()
