"""Chroma-aware (Lab) affinities: nle_ctx_set_chroma / NLEFilter::chromaBandwidth / `enhance --chroma HC`.

The restatement below is the contract of include/nle.h, in numpy.  With planes L, a, b (integer valued in [0, 255]), patch
radius R (0: single values), reflect-101 borders, sw = 1/hx^2, pw = 1/hy^2, cw = 1/hc^2:

    S_L, S_ab   the exact integer sums of squared differences of the (2R + 1)^2 patches of L, and of a and of b
    e0          R = 0: -sw d2 - pw dL^2 (oracle._neg_weighted_distance);  R > 0: -sw d2 - pwd S_L, pwd = pw / (2R + 1)^2
                (tests/test_patch_affinity.py)
    K_ij        exp(e0 - cwd S_ab), cwd = cw / (2R + 1)^2, the chroma term subtracted last, every operation rounded on its own

K_A and K_AB alike; every later stage is the oracle's own.  With chroma off (hc None) the restatement is e0: the oracle's
kernel at R = 0 and the patch restatement at R > 0, bit for bit (checked below)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, rel_l2

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_patch_affinity as tpa  # noqa: E402
import test_sampler as tsa  # noqa: E402

ENHANCE = tpa.ENHANCE
DENOISE = tpa.DENOISE
FLOWER, FLOWER_ARGS, DENOISE_ARGS = tpa.FLOWER, tpa.FLOWER_ARGS, tpa.DENOISE_ARGS
PER_LAYER_TOL = 1e-4


# ----------------------------------------------------------------------------------------------- the restatement
def _exponent(L, a, b, ia, ib, sw, pw, cw, R, Pt):
    """the exponent between pixels ia (rows) and ib (columns); Pt: the patch tables of (L, a, b) (R > 0) or None"""
    H, W = L.shape
    ra, ca, rb, cb = ia // W, ia % W, ib // W, ib % W
    d = (2 * R + 1) ** 2
    if R == 0:
        f = L.ravel()
        dr = ra[:, None].astype(np.int64) - rb[None, :].astype(np.int64)
        dc = ca[:, None].astype(np.int64) - cb[None, :].astype(np.int64)
        di = f[ia][:, None] - f[ib][None, :]
        e = -sw * (dr * dr + dc * dc).astype(np.float64) - pw * (di * di)
    else:
        e = tpa._patch_neg_dist(Pt[0][ia], ra, ca, Pt[0][ib], rb, cb, sw, pw / d)
    if cw is None:
        return e
    S = np.zeros(e.shape, dtype=np.int64)
    for k, plane in ((1, a), (2, b)):
        if R == 0:
            v = plane.ravel().astype(np.int64)
            dv = v[ia][:, None] - v[ib][None, :]
            S += dv * dv
        else:  # |x|^2 + |s|^2 - 2 x.s on exact integers in fp64 (every partial sum below 2^53)
            x, s = Pt[k][ia].astype(np.float64), Pt[k][ib].astype(np.float64)
            S += np.rint((x * x).sum(1)[:, None] + (s * s).sum(1)[None, :] - 2.0 * (x @ s.T)).astype(np.int64)
    return e - (cw / d) * S.astype(np.float64)


def compute_kernel_chroma(oracle, L, a, b, nr, nc, hx, hy, hc, R, chunk=1 << 15):
    """(perm, Ka, Kab) in the oracle's [selected; rest] order, like oracle.compute_kernel; hc None: chroma off"""
    L = np.asarray(L, dtype=np.float64)
    H, W = L.shape
    for plane in ((L,) if hc is None else (L, a, b)) if (R > 0 or hc is not None) else ():
        plane = np.asarray(plane, dtype=np.float64)
        assert plane.shape == (H, W) and np.array_equal(plane, np.rint(plane)) and plane.min() >= 0 and plane.max() <= 255
    sel, rest = oracle.sample_pixels(H, W, nr, nc)
    sw, pw = 1.0 / (hx * hx), 1.0 / (hy * hy)
    cw = None if hc is None else 1.0 / (hc * hc)
    Pt = None
    if R > 0:
        Pt = [tpa.patches(np.asarray(pl).astype(np.int64), R) if pl is not None else None
              for pl in ((L, a, b) if hc is not None else (L, None, None))]
    Ka = np.exp(_exponent(L, a, b, sel, sel, sw, pw, cw, R, Pt))
    Kab = np.empty((sel.size, rest.size))
    for s in range(0, rest.size, chunk):
        Kab[:, s:s + chunk] = np.exp(_exponent(L, a, b, sel, rest[s:s + chunk], sw, pw, cw, R, Pt))
    return np.concatenate([sel, rest]), Ka, Kab


def train_chroma(oracle, L, a, b, nr, nc, hx, hy, hc, T, K, R):
    """oracle.train_filter on the restated affinities: (V N x K' pixel order, eigvals, cut diagnostics of Ka, Wa, Q)"""
    perm, Ka, Kab = compute_kernel_chroma(oracle, L, a, b, nr, nc, hx, hy, hc, R)
    info = []
    lam, phi = oracle.nystrom_approximation(Ka, Kab, info=info)
    del Kab
    Wa, Wab, _, _ = oracle.sinkhorn_with_scalings(phi, lam, T)
    V, S = oracle.orthogonalize(Wa, Wab, K, info=info)
    out = np.empty_like(V)
    out[perm] = V
    return out, S, info


# ----------------------------------------------------------------------------------------------- inputs
_cache = {}


def _lab(oracle, name):
    """(L, a, b) fp64 planes: 8-bit Lab of a golden image, or the seeded synthetic triple `synth:H:W`"""
    if name not in _cache:
        if name.startswith("synth:"):
            H, W = (int(v) for v in name.split(":")[1:])
            _cache[name] = tuple(oracle.synthetic_luminance(H, W, seed=s) for s in (1234, 77, 4242))
        else:
            lab = oracle.bgr_to_lab8(tpa._load_bgr(name)).astype(np.float64)
            _cache[name] = tuple(np.ascontiguousarray(lab[..., k]) for k in range(3))
    return _cache[name]


def _isoluminant(H, W):
    """L = 128 everywhere; a = 100 left of the vertical edge at W / 2 and 160 right of it; b = 128"""
    L = np.full((H, W), 128.0)
    a = np.where(np.arange(W)[None, :] < W // 2, 100.0, 160.0) * np.ones((H, 1))
    return L, a, np.full((H, W), 128.0)


def _retained_step(plane, W):
    """the step that survives across the edge: mean of the 8 columns right of it minus the 8 left of it, over 60"""
    return float(plane[:, W // 2:W // 2 + 8].mean() - plane[:, W // 2 - 8:W // 2].mean()) / 60.0


# train + apply cases (item 5): plane, nr, nc, hx, hy, hc, T, K, L; chosen with the restatement on the CPU so that no
# restated spectrum sits on a 1e-10 cut (the margins are printed by the test)
TRAIN_CASES = {
    "synth": ("synth:72:96", 6, 8, 16.0, 30.0, 25.0, 10, 12, 4),
    "flower": ("flower-50.bmp", 10, 20, 100.0, 30.0, 20.0, 50, 30, 4),
    "cherries": ("readme/red-cherries-10.bmp", 8, 10, 40.0, 30.0, 15.0, 20, 20, 4),
}
# the isoluminant plane of item 7: H, W, nr, nc, hx, hy, hc, T, K, L
ISO = (48, 64, 6, 8, 10.0, 30.0, 10.0, 10, 8, 4)


# ------------------------------------------------------------------------------------------------------ CPU tests
def test_restatement_with_chroma_off_is_the_oracle_s_and_the_patch_restatement_bit_for_bit(oracle):
    for (H, W, nr, nc, hx, hy) in [(30, 44, 5, 6, 7.0, 20.0), (17, 23, 4, 3, 40.0, 9.0)]:
        y = oracle.synthetic_luminance(H, W)
        for R in (0, 1, 3):
            want = oracle.compute_kernel(y, nr, nc, hx, hy) if R == 0 else tpa.compute_kernel_patch(oracle, y, nr, nc, hx, hy, R)
            got = compute_kernel_chroma(oracle, y, None, None, nr, nc, hx, hy, None, R)
            for g, w in zip(got, want):
                assert np.array_equal(g, w), (H, W, R)


def test_restatement_chroma_term_by_hand(oracle):
    """one entry evaluated scalar by scalar, R = 0 and R = 1"""
    L, a, b = _lab(oracle, "synth:12:15")
    H, W = L.shape
    nr, nc, hx, hy, hc = 3, 4, 5.0, 20.0, 12.0
    for R in (0, 1):
        perm, Ka, Kab = compute_kernel_chroma(oracle, L, a, b, nr, nc, hx, hy, hc, R)
        p = Ka.shape[0]
        i, j = int(perm[p + 7]), int(perm[2])
        ri, ci, rj, cj = i // W, i % W, j // W, j % W
        refl = lambda t, n: -t if t < 0 else (2 * n - 2 - t if t >= n else t)  # noqa: E731
        SL = Sab = 0
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                yi, xi, yj, xj = refl(ri + dy, H), refl(ci + dx, W), refl(rj + dy, H), refl(cj + dx, W)
                SL += int(L[yi, xi] - L[yj, xj]) ** 2
                Sab += int(a[yi, xi] - a[yj, xj]) ** 2 + int(b[yi, xi] - b[yj, xj]) ** 2
        d = (2 * R + 1) ** 2
        sw, pw, cw = 1.0 / (hx * hx), 1.0 / (hy * hy), 1.0 / (hc * hc)
        e0 = -sw * float((ri - rj) ** 2 + (ci - cj) ** 2) - (pw / d if R else pw) * float(SL)
        assert Kab[2, 7] == np.exp(e0 - (cw / d) * float(Sab))


def test_chroma_is_declared_exported_and_mirrored(nle):
    hdr = open(os.path.join(ROOT, "include", "nle.h")).read()
    assert "int nle_ctx_set_chroma(nle_ctx* ctx, const float* d_a, const float* d_b, double hc);" in hdr
    assert "int nle_filter_chroma(const nle_filter* f, double* hc);" in hdr
    assert "#define NLE_CHROMA_PATCH_RADIUS_MAX 3" in hdr
    from nle_amd import _abi
    assert _abi.NLE_CHROMA_PATCH_RADIUS_MAX == 3
    for name in ("nle_ctx_set_chroma", "nle_filter_chroma"):
        assert name in _abi.SIGNATURES and name in nle.EXPORTED_SYMBOLS
        assert hasattr(nle.lib(), name)  # exported by the built library
    assert callable(getattr(nle.Context, "set_chroma", None)) and callable(getattr(nle.NLEFilter, "chroma", None))
    hpp = open(os.path.join(ROOT, "include", "nle", "filter.hpp")).read()
    assert "double chromaBandwidth = 0;" in hpp


@pytest.mark.parametrize("lead", [["--chroma", "0"], ["--chroma", "-5"], ["--chroma", "nan"], ["--chroma", "inf"],
                                  ["--chroma", "ten"], ["--chroma", "20", "--exact"], ["--exact", "--chroma", "20"],
                                  ["--patch-radius", "4", "--chroma", "20"], ["--chroma", "20", "--patch-radius", "4"]],
                         ids=lambda v: "_".join(v).replace("--", ""))
def test_cli_refuses_bad_chroma_before_any_gpu_call(lead, tmp_path):
    # HIP_VISIBLE_DEVICES=-1: no device is visible -- the refusal must not need one
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = tmp_path / "o.png"
    r = subprocess.run([ENHANCE] + lead + [os.path.join(GOLDEN, "flower-50.bmp"), str(out)] + FLOWER_ARGS,
                       capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "--chroma" in r.stderr
    assert r.stdout == "" and not out.exists()


def test_denoise_cli_refuses_chroma_before_any_gpu_call(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = tmp_path / "o.png"
    r = subprocess.run([DENOISE, "--chroma", "20", os.path.join(GOLDEN, "flower-50.bmp"), str(out)] + DENOISE_ARGS,
                       capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "--chroma" in r.stderr
    assert r.stdout == "" and not out.exists()


# ------------------------------------------------------------------------------------------------------ GPU tests
@pytest.fixture
def cctx(ctx):
    """the session ctx, handed back without chroma, with the reference's affinity, grid and auto mode"""
    yield ctx
    ctx.set_chroma(None, None, 0.0)
    ctx.set_patch_radius(0)
    ctx.set_sampler(0)
    ctx.set_mode(0)


_kernel64 = tpa._kernel64


# H, W, nr, nc, hx, hy, hc, R, sampler: non-square planes, p not a multiple of 16, R = min(H, W) - 1 (the 4-row plane)
KERNEL_CASES = [("synth:24:40", 4, 5, 8.0, 30.0, 20.0, 0, "grid"), ("synth:37:12", 5, 3, 6.0, 12.0, 9.0, 0, "farthest"),
                ("synth:24:40", 4, 5, 8.0, 30.0, 20.0, 1, "grid"), ("synth:31:45", 5, 7, 9.0, 25.0, 30.0, 1, "farthest"),
                ("synth:48:64", 6, 8, 12.0, 25.0, 15.0, 3, "grid"), ("synth:37:12", 5, 3, 6.0, 12.0, 9.0, 3, "farthest"),
                ("synth:4:21", 3, 6, 10.0, 30.0, 25.0, 3, "grid"), ("synth:3:19", 2, 5, 10.0, 30.0, 25.0, 2, "grid"),
                ("readme/red-cherries-10.bmp", 7, 9, 30.0, 30.0, 15.0, 0, "grid"),
                ("readme/red-cherries-10.bmp", 7, 9, 30.0, 30.0, 15.0, 2, "farthest"),
                ("flower-50.bmp", 10, 20, 100.0, 30.0, 20.0, 3, "grid")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: f"{c[0].split('/')[-1]}-R{c[6]}-{c[7]}")
def test_compute_kernel64_with_chroma_matches_the_restatement(nle, oracle, cctx, monkeypatch, case):
    name, nr, nc, hx, hy, hc, R, sampler = case
    L, a, b = _lab(oracle, name)
    H, W = L.shape
    cctx.set_patch_radius(R)
    cctx.set_chroma(a, b, hc)
    if sampler == "farthest":
        cctx.set_sampler(nle.SAMPLER_FARTHEST)
        S = tsa.farthest(L, tsa.grid_count(oracle, H, W, nr, nc), hx, hy)  # the luminance-only metric, also with chroma
        tsa.use_set(monkeypatch, oracle, H, W, S)
    st, Ka, kab, p = _kernel64(nle, cctx, L, nr, nc, hx, hy)
    assert st == 0, nle.lib().nle_last_error(cctx._h)
    perm, Ka_o, Kab_o = compute_kernel_chroma(oracle, L, a, b, nr, nc, hx, hy, hc, R)
    K_o = np.empty((H * W, p))  # natural pixel order, every pixel (the sample pixels' rows are rows of Ka)
    K_o[perm[:p]] = Ka_o
    K_o[perm[p:]] = Kab_o.T
    for what, got, want in (("Ka", Ka, Ka_o), ("Kab", kab[:, :p], K_o)):
        zero = want == 0.0
        assert np.all(got[zero] == 0.0)
        rel = np.abs(got[~zero] - want[~zero]) / want[~zero]
        print(f"{name} R = {R} {sampler}: {what} {H} x {W}, p = {p}, in [{want.min():.2e}, {want.max():.2e}], "
              f"largest relative difference {rel.max():.2e}")
        np.testing.assert_allclose(got[~zero], want[~zero], rtol=1e-14, atol=0)
    assert np.all(kab[:, p:] == 0.0)
    # the term is really there: the same call without chroma gives another kernel
    cctx.set_chroma(None, None, 0.0)
    st, Ka0, _, _ = _kernel64(nle, cctx, L, nr, nc, hx, hy)
    assert st == 0 and not np.array_equal(Ka0, Ka)


def _train_apply(nle, ctx, L, x, nr, nc, hx, hy, T, K, nl):
    f = nle.NLEFilter(ctx).train_filter(np.asarray(L, dtype=np.float32), nr, nc, hx, hy, T, K)
    Y = f.apply_layers(np.asarray(x, dtype=np.float32), nl).cpu().numpy().astype(np.float64)
    return f, Y


def _restated(oracle, key, *args):
    if key not in _cache:
        _cache[key] = train_chroma(oracle, *args)
    return _cache[key]


def _check_against_restatement(nle, oracle, ctx, planes, x, params, R, modes, key):
    """train + apply in `modes` against the oracle's stages on the restated kernel, at the project's standing bars; returns
    {mode: layers}, or None when the restated spectrum sits on a 1e-10 cut (not asserted then, as tests/test_patch_affinity.py)"""
    L, a, b = planes
    nr, nc, hx, hy, hc, T, K, nl = params
    V_o, S_o, info = _restated(oracle, key, L, a, b, nr, nc, hx, hy, hc, T, K, R)
    Y_o = oracle.apply_layers(V_o, S_o, x, nl).reshape(nl, -1)
    cuts = [d["kept"] for d in info]
    margin = tpa._cut_margin(info)
    print(f"{key}: restated cuts {cuts}, K' = {S_o.size}, nearest eigenvalue to the 1e-10 cut is {margin:.1f}x away")
    ctx.set_patch_radius(R)
    if hc is None:
        ctx.set_chroma(None, None, 0.0)
    else:
        ctx.set_chroma(a, b, hc)
    results = {}
    for mode in modes:
        ctx.set_mode(mode)
        f, Y = tsa._with_chunks(mode, lambda: _train_apply(nle, ctx, L, x, nr, nc, hx, hy, T, K, nl))
        d = f.diag()
        want_form = nle.MODE_MATERIALISED_F64 if mode == nle.MODE_AUTO else mode
        assert d["formulation"] == want_form  # the fp64 formulation that ran
        assert f.chroma() == (0.0 if hc is None else hc)
        ev_err = rel_l2(f.eigvals, S_o) if f.eigvals.size == S_o.size else np.inf
        errs = [rel_l2(Y[j], Y_o[j]) for j in range(nl)]
        print(f"  mode {mode}: cuts {[d['r_Ka'], d['r_Wa'], d['r_Q']]}, eigenvalues {ev_err:.1e}, per-layer",
              ["%.1e" % e for e in errs])
        f.close()
        if margin < 1.5:
            continue
        assert [d["r_Ka"], d["r_Wa"], d["r_Q"]] == cuts
        assert d["K"] == S_o.size
        assert ev_err < 1e-8
        assert max(errs) < PER_LAYER_TOL
        results[mode] = Y
    if margin < 1.5:
        return None
    return results, Y_o


_dropped = []


@pytest.mark.gpu
@pytest.mark.parametrize("R", [0, 3])
@pytest.mark.parametrize("plane", list(TRAIN_CASES))
def test_train_apply_with_chroma_meets_the_bars_in_every_fp64_form(nle, oracle, cctx, plane, R):
    name, nr, nc, hx, hy, hc, T, K, nl = TRAIN_CASES[plane]
    planes = _lab(oracle, name)
    modes = (nle.MODE_MATERIALISED_F64, nle.MODE_STREAMED_F64, nle.MODE_AUTO)
    out = _check_against_restatement(nle, oracle, cctx, planes, planes[0], (nr, nc, hx, hy, hc, T, K, nl), R, modes,
                                     ("train", plane, R))
    if out is None:  # at most one parametrised case may drop out this way
        _dropped.append((plane, R))
        assert len(_dropped) <= 1, _dropped
        return
    results, _ = out
    for j in range(nl):  # the two fp64 forms agree as tests/test_gpu_parity.py holds them
        assert rel_l2(results[nle.MODE_STREAMED_F64][j], results[nle.MODE_MATERIALISED_F64][j]) < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("plane", ["cherries", "flower"])  # the most pixels (624 x 416), the most samples (p = 200)
def test_two_runs_of_the_largest_case_are_bitwise_equal(nle, oracle, cctx, plane):
    name, nr, nc, hx, hy, hc, T, K, nl = TRAIN_CASES[plane]
    L, a, b = _lab(oracle, name)
    cctx.set_patch_radius(3)
    cctx.set_chroma(a, b, hc)
    for mode in (nle.MODE_MATERIALISED_F64, nle.MODE_STREAMED_F64):
        cctx.set_mode(mode)
        runs = []
        for _ in range(2):
            f, Y = tsa._with_chunks(mode, lambda: _train_apply(nle, cctx, L, L, nr, nc, hx, hy, T, K, nl))
            runs.append((f.eigvals.copy(), Y, f.diag()))
            f.close()
        assert runs[0][2] == runs[1][2]
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 4], ids=["auto_tables", "materialised_f64"])
def test_chroma_off_changes_nothing(nle, oracle, cctx, mode):
    H, W, nr, nc, hx, hy, T, K, nl = tpa.SYNTH
    L, a, b = _lab(oracle, f"synth:{H}:{W}")
    fresh = nle.Context(0)
    try:
        fresh.set_mode(mode)
        f0, Y0 = _train_apply(nle, fresh, L, L, nr, nc, hx, hy, T, K, nl)
        cctx.set_mode(mode)
        cctx.set_chroma(a, b, 20.0)
        cctx.set_chroma(None, None, 0.0)
        f1, Y1 = _train_apply(nle, cctx, L, L, nr, nc, hx, hy, T, K, nl)
        assert f0.diag() == f1.diag()
        assert f0.diag()["formulation"] == (nle.MODE_PHI_FREE if mode == 0 else mode)  # auto: the tables
        assert f1.chroma() == 0.0
        assert np.array_equal(f0.eigvals, f1.eigvals) and np.array_equal(Y0, Y1)
        f0.close()
        f1.close()
    finally:
        fresh.close()


@pytest.mark.gpu
def test_chroma_keeps_an_isoluminant_edge_that_luminance_cannot_see(nle, oracle, cctx):
    """L = 128 everywhere, a steps from 100 to 160 at W / 2, b = 128: no luminance information at all.  The base layer of
    the a plane keeps the step with chroma affinities and blurs it without.  Restatement (fp64, CPU), ISO = 48 x 64, 6 x 8
    grid, hx = 10, hy = 30, hc = 10, T = 10, K = 8, 4 layers: retained step 1.0000 with chroma, 0.2087 without (4.8x).  The
    product is held to both numbers at the standing bars; the factor 2 asserted below is a floor, not a measurement."""
    H, W, nr, nc, hx, hy, hc, T, K, nl = ISO
    planes = _isoluminant(H, W)
    a = planes[1]
    steps, want = {}, {}
    for label, h in (("chroma", hc), ("no chroma", None)):
        out = _check_against_restatement(nle, oracle, cctx, planes, a, (nr, nc, hx, hy, h, T, K, nl), 0,
                                         (nle.MODE_MATERIALISED_F64,), ("iso", label))
        assert out is not None, "the isoluminant configuration must not sit on a cut"
        results, Y_o = out
        steps[label] = _retained_step(results[nle.MODE_MATERIALISED_F64][nl - 1].reshape(H, W), W)
        want[label] = _retained_step(Y_o[nl - 1].reshape(H, W), W)
        print(f"{label}: retained step {steps[label]:.4f} (restatement {want[label]:.4f})")
        assert abs(steps[label] - want[label]) <= 1e-4 * max(abs(want[label]), 1.0)
    assert want["chroma"] >= 4.0 * want["no chroma"]  # the configuration itself (see the docstring)
    assert steps["chroma"] >= 2.0 * steps["no chroma"]


@pytest.mark.gpu
def test_refusals_leave_the_ctx_usable(nle, oracle, cctx):
    nr, nc, hx, hy, T, K, nl = 4, 5, 12.0, 30.0, 5, 6, 3
    L, a, b = _lab(oracle, "synth:40:56")

    def refused(fn):
        with pytest.raises(nle.NLEError) as e:
            fn()
        assert e.value.code == nle.NLE_ERR_INVALID
        print("refused:", e.value)

    def train(plane=L):
        return _train_apply(nle, cctx, plane, plane, nr, nc, hx, hy, T, K, nl)

    refused(lambda: cctx.set_chroma(a, None, 20.0))          # one plane without the other
    refused(lambda: cctx.set_chroma(None, b, 20.0))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(lambda: cctx.set_chroma(a, b, bad))
    cctx.set_chroma(a, b, 20.0)
    for mode in (nle.MODE_MATERIALISED, nle.MODE_PHI_FREE, nle.MODE_PHI_FREE_EXP, nle.MODE_EXACT_F64):
        cctx.set_mode(mode)                                  # fp32, table, Phi-free and exact forms
        refused(train)
    cctx.set_mode(0)
    refused(lambda: train(L + 0.5))                          # L not integer valued
    cctx.set_chroma(a + 0.5, b, 20.0)
    refused(train)                                           # a not integer valued
    cctx.set_chroma(a, b + 256.0, 20.0)
    refused(train)                                           # b not in [0, 255]
    cctx.set_chroma(a, b, 20.0)
    cctx.set_patch_radius(4)
    refused(train)                                           # radius above NLE_CHROMA_PATCH_RADIUS_MAX
    st, _, _, _ = _kernel64(nle, cctx, L, nr, nc, hx, hy)
    assert st == nle.NLE_ERR_INVALID
    cctx.set_patch_radius(0)
    refused(lambda: cctx.compute_kernel(L.astype(np.float32), nr, nc, hx, hy))   # fp32 stage entry points
    refused(lambda: cctx.nystrom(L.astype(np.float32), nr, nc, hx, hy))
    st, _, _, _ = _kernel64(nle, cctx, L + 0.5, nr, nc, hx, hy)
    assert st == nle.NLE_ERR_INVALID
    # still usable: the same ctx trains with chroma, and without it a plain filter that meets the bars
    f, _ = train()
    assert f.diag()["formulation"] == nle.MODE_MATERIALISED_F64 and f.chroma() == 20.0
    f.close()
    cctx.set_chroma(None, None, 0.0)
    f, Y = train()
    assert f.chroma() == 0.0
    V_o, S_o = oracle.train_filter(L, nr, nc, hx, hy, T, K)
    Y_o = oracle.apply_layers(V_o, S_o, L, nl).reshape(nl, -1)
    assert max(rel_l2(Y[j], Y_o[j]) for j in range(nl)) < PER_LAYER_TOL
    f.close()


# ------------------------------------------------------------------------------------------------------ multi-rank
MR = (64, 80, 6, 8, 14.0, 30.0, 8, 10, 4)
MR_HC, MR_R = 20.0, 3


def _mr_planes(synth):
    H, W = MR[:2]
    return tuple(synth.synthetic_luminance(H, W, seed=s) for s in (1234, 77, 4242))


def _worker(rank, world, port, outdir, slabs):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401
    import torch.distributed as dist
    import __graft_entry__ as entry
    nle = entry.load_package()
    synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        H, W, nr, nc, hx, hy, T, K, nl = MR
        x, a, b = (v.astype(np.float32) for v in _mr_planes(synth))
        ctx = nle.Context(0)
        ctx.set_patch_radius(MR_R)
        g = nle.sample_grid(H, W, nr, nc)
        ctx.set_shard(rank, world, g["n_sel_rows"] * g["n_sel_cols"], lambda t: dist.all_reduce(t))
        if slabs:
            ctx.set_slab_input(True)
            r0, r1 = nle.slab_rows(H, rank, world)
            ctx.set_chroma(np.ascontiguousarray(a[r0:r1]), np.ascontiguousarray(b[r0:r1]), MR_HC)
            try:
                nle.NLEFilter(ctx).train_filter(np.ascontiguousarray(x[r0:r1]), nr, nc, hx, hy, T, K, shape=(H, W))
                code = 0
            except nle.NLEError as e:
                code = e.code
            np.savez(os.path.join(outdir, f"rank{rank}.npz"), code=np.array([code]))
        else:
            ctx.set_chroma(a, b, MR_HC)
            f = nle.NLEFilter(ctx).train_filter(x, nr, nc, hx, hy, T, K)
            Y = f.apply_layers(x, nl).cpu().numpy()
            info = f.info()
            np.savez(os.path.join(outdir, f"rank{rank}.npz"), Y=Y, S=f.eigvals, form=np.array([f.diag()["formulation"]]),
                     hc=np.array([f.chroma()]), rows=np.array([info["row0"], info["row1"]]))
            f.close()
        ctx.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_ranks_with_chroma_match_single_rank(nle, cctx, tmp_path, world):
    import torch.multiprocessing as mp
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
    H, W, nr, nc, hx, hy, T, K, nl = MR
    x, a, b = _mr_planes(synth)
    cctx.set_patch_radius(MR_R)
    cctx.set_chroma(a, b, MR_HC)
    f1, Y1 = _train_apply(nle, cctx, x, x, nr, nc, hx, hy, T, K, nl)
    S1 = f1.eigvals
    f1.close()
    mp.spawn(_worker, args=(world, tpa._free_port(), str(tmp_path), False), nprocs=world, join=True)
    Y = np.zeros((nl, H * W))
    for r in range(world):
        d = np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))
        r0, r1 = d["rows"]
        Y[:, r0 * W:r1 * W] = d["Y"]
        assert int(d["form"][0]) == nle.MODE_MATERIALISED_F64 and float(d["hc"][0]) == MR_HC
        assert rel_l2(d["S"], S1) < 1e-9
    for j in range(nl):
        assert rel_l2(Y[j], Y1[j]) < 1e-6, j


@pytest.mark.gpu
def test_slab_input_with_chroma_is_refused_on_every_rank(nle, tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, tpa._free_port(), str(tmp_path), True), nprocs=2, join=True)
    for r in range(2):
        assert int(np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))["code"][0]) == nle.NLE_ERR_INVALID


# ------------------------------------------------------------------------------------------------------ CLI
@pytest.mark.gpu
@pytest.mark.parametrize("lead,R,sampler", [(["--chroma", "20"], 0, 0),
                                            (["--patch-radius", "2", "--chroma", "20", "--sampler", "farthest"], 2, 1)],
                         ids=["chroma", "radius_chroma_farthest"])
def test_enhance_with_chroma_matches_the_python_mirror(nle, oracle, cctx, tmp_path, lead, R, sampler):
    from PIL import Image
    import torch
    src = tpa._load_bgr("flower-50.bmp")
    out = tmp_path / "flower-chroma.png"
    r = subprocess.run([ENHANCE] + lead + [os.path.join(GOLDEN, "flower-50.bmp"), str(out)] + FLOWER_ARGS,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    got = np.asarray(Image.open(str(out)).convert("RGB"))[..., ::-1]
    # the same pipeline through the Python mirror: bgr2lab8 -> lab8_channel x 2 -> set_chroma -> train_host_u8 ->
    # apply_u8_host -> lab2bgr8
    H, W = src.shape[:2]
    lab, _ = cctx.bgr2lab8(src)
    cctx.set_patch_radius(R)
    cctx.set_sampler(sampler)
    cctx.set_chroma(cctx.lab8_channel(lab, 1), cctx.lab8_channel(lab, 2), 20.0)
    L8 = lab[..., 0].cpu().numpy().copy()
    f = nle.NLEFilter(cctx).train_filter_host_u8(L8, FLOWER["nr"], FLOWER["nc"], FLOWER["hx"], FLOWER["hy"], FLOWER["T"],
                                                 FLOWER["K"])
    assert f.chroma() == 20.0 and f.diag()["formulation"] == nle.MODE_MATERIALISED_F64
    fS = oracle.transform_eigenvalues(f.eigvals, FLOWER["weights"])
    y8 = np.empty(H * W, dtype=np.uint8)
    f.apply_u8_host(None, fS, y8)
    f.close()
    Lf = torch.as_tensor(y8.reshape(H, W).astype(np.float32), device=lab.device)
    mirror = cctx.lab2bgr8(lab, L=Lf).cpu().numpy()
    assert np.array_equal(got, mirror)
    # and it is not what enhance writes without the option
    out0 = tmp_path / "flower-plain.png"
    r = subprocess.run([ENHANCE] + [v for v in lead if v not in ("--chroma", "20")] +
                       [os.path.join(GOLDEN, "flower-50.bmp"), str(out0)] + FLOWER_ARGS, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr
    assert not np.array_equal(got, np.asarray(Image.open(str(out0)).convert("RGB"))[..., ::-1])
