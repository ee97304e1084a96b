"""Residual-greedy (pivoted-Cholesky) sample selection: NLE_SAMPLER_RESIDUAL / nle_sample_pixels_order /
nle_residual_sampler_bytes / NLEFilter::sampler = 3 / `--sampler residual`.

The restatement below is the rule of include/nle.h in numpy, fp64, plane values taken as fp32 as the product reads them:

    K(i, j) = exp(-sw (double)(dr^2 + dc^2) - pw dy^2);  d_i = 1;  s_0 = pixel (H/2, W/2)
    round k:  l_k[i] = (K(i, s_k) - sum_{j<k} l_j[i] l_j[s_k]) / sqrt(d_{s_k});  d_i -= l_k[i]^2
              s_{k+1} = argmax over the pixels not chosen of d_i, ties to the smallest row-major index

while that maximum is >= NLE_EPS; from the first round whose maximum is below it every remaining sample is the farthest-point
step of tests/test_sampler.py on m (the smallest D to ALL samples so far, -1 at a chosen pixel, kept from round 0).

Why the GPU tests do not compare indices with `residual_greedy`: exact ties between the best and the runner-up occur on real
planes, near-ties go down to 1e-13, and the device's libm exp differs from numpy's in the last place.  The device is held to
the rule along ITS OWN order (`follow`): at every residual round k

    |h_pivot[k] - d_ref[s_k]| <= tol,   d_ref[s_k] >= max over the pixels not chosen of d_ref - 2 tol,   d_ref[s_k] >= NLE_EPS - tol

at the first fallback round max d_ref < NLE_EPS + tol, and every fallback round equals the farthest-point step on numpy's m
exactly (D involves no exp).

tol = p^2 2^-53, absolute.  Round k's column carries about k roundings of size u = 2^-53 before the division; |l_k[i]| <=
sqrt(d_i) <= sqrt(d_s), so the division by sqrt(d_s) does not amplify them beyond about 2 k u per d_i and round; the sum over
the rounds is below p^2 u (4.4e-12 at p = 200), far below NLE_EPS.  fp64 against long double along the same pivots measured
1.8e-15 on flower[::2, ::2], bird[::3, ::3] and forest[::4, ::4] at p = 200."""
import os
import shutil
import subprocess
import sys
import textwrap
import time

import numpy as np
import pytest

from conftest import GOLDEN, PKG_DIR, ROOT, rel_l2

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_nystrom_residual as tnr  # noqa: E402
import test_sampler as tsa  # noqa: E402

ENHANCE, DENOISE = tsa.ENHANCE, tsa.DENOISE
FLOWER, FLOWER_ARGS, DENOISE_ARGS = tsa.FLOWER, tsa.FLOWER_ARGS, tsa.DENOISE_ARGS
NLE_EPS = 1e-10
U = 2.0 ** -53


def tol(p):
    return p * p * U


# ----------------------------------------------------------------------------------------------- the restatement
def _plane(y):
    y = np.asarray(y, dtype=np.float32).astype(np.float64)
    H, W = y.shape
    idx = np.arange(H * W, dtype=np.int64)
    return y.ravel(), idx // W, idx % W, H, W


def _D(f, rr, cc, s, sw, pw):
    dr, dc = rr - rr[s], cc - cc[s]
    dy = f - f[s]
    return sw * (dr * dr + dc * dc).astype(np.float64) + pw * (dy * dy)


def _column(f, rr, cc, s, sw, pw, cols, d):
    """l_k for the sample s: the rule's operation order, j ascending, one accumulator"""
    dr, dc = rr - rr[s], cc - cc[s]
    dy = f - f[s]
    acc = np.zeros(f.size)
    for lj in cols:
        acc = acc + lj * lj[s]
    return (np.exp(-sw * (dr * dr + dc * dc).astype(np.float64) - pw * (dy * dy)) - acc) / np.sqrt(d[s])


def residual_greedy(y, p, hx, hy):
    """(order, pivots, n_residual, d after the last residual round) of the rule on plane y"""
    f, rr, cc, H, W = _plane(y)
    N = H * W
    sw, pw = 1.0 / (hx * hx), 1.0 / (hy * hy)
    d, m, chosen, cols = np.ones(N), None, np.zeros(N, dtype=bool), []
    order, pivots = [], []
    s, piv, fallen = (H // 2) * W + W // 2, 1.0, False
    for k in range(p):
        order.append(s)
        pivots.append(piv)
        chosen[s] = True
        D = _D(f, rr, cc, s, sw, pw)
        m = D if m is None else np.minimum(m, D)
        m[s] = -1.0
        if not fallen:
            cols.append(_column(f, rr, cc, s, sw, pw, cols, d))
            d = d - cols[-1] * cols[-1]
        if k == p - 1:
            break
        if not fallen:
            dm = np.where(chosen, -np.inf, d)
            s = int(np.argmax(dm))  # first maximum: the smallest index on ties
            piv = float(dm[s])
            fallen = not piv >= NLE_EPS
        if fallen:
            s = int(np.argmax(m))
            piv = float(m[s])
    return np.array(order, dtype=np.int64), np.array(pivots), len(cols), d


def follow(y, order, hx, hy, n_residual=None):
    """the reference state along a GIVEN order: d[k] = d before round k for k <= n_residual (d[n_residual]: after the last
    residual round), m[k] = the farthest-point m before round k (m[0] is None), -1 at the pixels chosen before round k"""
    f, rr, cc, H, W = _plane(y)
    sw, pw = 1.0 / (hx * hx), 1.0 / (hy * hy)
    n_residual = len(order) if n_residual is None else n_residual
    d, m, cols = np.ones(H * W), None, []
    ds, ms = [d], [None]
    for k, s in enumerate(order):
        s = int(s)
        D = _D(f, rr, cc, s, sw, pw)
        m = D if m is None else np.minimum(m, D)
        m[s] = -1.0
        ms.append(m.copy())
        if k < n_residual:
            cols.append(_column(f, rr, cc, s, sw, pw, cols, d))
            d = d - cols[-1] * cols[-1]
            ds.append(d)
    return dict(d=ds, m=ms)


def textbook(y, p, hx, hy):
    """diagonal-pivoted Cholesky of the explicit N x N affinity, Schur complements written out; (order, pivots, smallest
    relative gap between the best and the runner-up diagonal entry over the rounds)"""
    f, rr, cc, H, W = _plane(y)
    N = H * W
    sw, pw = 1.0 / (hx * hx), 1.0 / (hy * hy)
    A = np.empty((N, N))
    for i in range(N):
        for j in range(N):
            dr, dc = int(rr[i] - rr[j]), int(cc[i] - cc[j])
            dy = float(f[i]) - float(f[j])
            A[i, j] = np.exp(-sw * float(dr * dr + dc * dc) - pw * (dy * dy))
    order, pivots, gap = [], [], np.inf
    s = (H // 2) * W + W // 2
    for k in range(p):
        order.append(s)
        pivots.append(A[s, s])
        col = A[:, s] / np.sqrt(A[s, s])
        A = A - np.outer(col, col)
        diag = np.array([A[i, i] if i not in order else -np.inf for i in range(N)])
        if k < p - 1:
            s = int(np.argmax(diag))
            top = np.sort(diag)[-2:]
            gap = min(gap, (top[1] - top[0]) / top[1])
    return np.array(order), np.array(pivots), gap


def check_farthest_step(m_before, s, pivot=None):
    assert s == int(np.argmax(m_before))  # first maximum: the smallest index on ties
    if pivot is not None:
        assert pivot == m_before[s]


def check_along_own_order(y, p, hx, hy, order, pivot, n_residual):
    """the consistency check of the module docstring; returns follow's state"""
    f, rr, cc, H, W = _plane(y)
    N, t = H * W, tol(p)
    assert order.size == p and pivot.size == p and np.unique(order).size == p and order.min() >= 0 and order.max() < N
    assert 1 <= n_residual <= p and order[0] == (H // 2) * W + W // 2 and pivot[0] == 1.0
    ref = follow(y, order, hx, hy, n_residual)
    chosen = np.zeros(N, dtype=bool)
    worst = 0.0
    for k in range(p):
        s = int(order[k])
        assert not chosen[s]
        if k < n_residual:
            d = ref["d"][k]
            worst = max(worst, abs(pivot[k] - d[s]))
            assert abs(pivot[k] - d[s]) <= t, (k, pivot[k], d[s])
            if k > 0:
                assert d[s] >= d[~chosen].max() - 2 * t, (k, d[s], d[~chosen].max())
                assert d[s] >= NLE_EPS - t, (k, d[s])
        else:
            if k == n_residual:
                assert ref["d"][n_residual][~chosen].max() < NLE_EPS + t
            check_farthest_step(ref["m"][k], s, pivot[k])
        chosen[s] = True
    print(f"p = {p}, n_residual = {n_residual}, N = {N}: largest |pivot - d_ref| = {worst:.2e} (tol {t:.2e}), "
          f"smallest residual pivot = {pivot[:n_residual].min():.3e}")
    return ref


# ------------------------------------------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("case", [(5, 7, 12, 8.0, 120.0, 2), (6, 6, 10, 5.0, 200.0, 1), (4, 9, 12, 5.0, 200.0, 3)])
def test_restatement_equals_textbook_pivoted_cholesky(case):
    H, W, p, hx, hy, seed = case
    y = np.random.default_rng(seed).uniform(0.0, 255.0, (H, W)).astype(np.float32)
    order, pivots, n_residual, _ = residual_greedy(y, p, hx, hy)
    t_order, t_pivots, gap = textbook(y, p, hx, hy)
    print(f"{H} x {W}, p = {p}: smallest best-to-runner-up gap {gap:.3e}, smallest pivot {pivots.min():.3e}")
    assert gap > 1e-9, "a near-tie: choose another seed or bandwidth for this case"
    assert n_residual == p
    assert np.array_equal(order, t_order)
    assert np.abs(pivots - t_pivots).max() <= 1e-13


@pytest.mark.parametrize("case", [(30, 44, 5, 6, 7.0, 20.0), (17, 23, 4, 3, 40.0, 9.0), (1, 50, 1, 7, 10.0, 30.0)])
def test_restatement_structure(oracle, case):
    H, W, nr, nc, hx, hy = case
    y = oracle.synthetic_luminance(H, W)
    p = tsa.grid_count(oracle, H, W, nr, nc)
    order, pivots, n_residual, d = residual_greedy(y, p, hx, hy)
    assert order.size == p and np.unique(order).size == p and order.min() >= 0 and order.max() < H * W
    assert order[0] == (H // 2) * W + W // 2 and pivots[0] == 1.0
    assert np.all(np.diff(pivots[:n_residual]) <= 0)  # the largest residual cannot grow: d only decreases
    assert np.all(d <= 1.0) and d.min() > -tol(p)


def test_final_d_is_the_nystrom_residual_of_the_chosen_set(oracle, monkeypatch):
    H, W, nr, nc, hx, hy = tnr.SMALL
    y = oracle.synthetic_luminance(H, W)
    p = tsa.grid_count(oracle, H, W, nr, nc)
    order, _, n_residual, d = residual_greedy(y, p, hx, hy)
    assert n_residual == p
    tsa.use_set(monkeypatch, oracle, H, W, np.sort(order))
    perm, Ka, Kab = oracle.compute_kernel(y, nr, nc, hx, hy)
    r, lam = tnr.residual(oracle, perm, Ka, Kab)
    assert lam.size == p
    print(f"max |d - r| = {np.abs(d - r).max():.2e}, cond2 = {lam[0] / lam[-1]:.3g}, max r = {r.max():.4f}")
    assert np.abs(d - r).max() <= 1e-10


_cache = {}


def _L(oracle, name):
    if name not in _cache:
        path = os.path.join(GOLDEN, name) if os.path.exists(os.path.join(GOLDEN, name)) else os.path.join(GOLDEN, "readme", name)
        from PIL import Image
        bgr = np.asarray(Image.open(path).convert("RGB"))[..., ::-1].copy()
        _cache[name] = oracle.bgr_to_lab8(bgr)[..., 0].astype(np.float64)
        _cache[name].setflags(write=False)
    return _cache[name]


FOREST = (20, 10, 5000.0, 30.0)  # the README pair's own arguments


def _forest(oracle):
    y = _L(oracle, "forest-10.bmp")[::4, ::4].copy()
    return y, tsa.grid_count(oracle, y.shape[0], y.shape[1], FOREST[0], FOREST[1])


def _forest_ref(oracle):
    if "forest_ref" not in _cache:
        y, p = _forest(oracle)
        _cache["forest_ref"] = residual_greedy(y, p, FOREST[2], FOREST[3])
    return _cache["forest_ref"]


def test_fallback_on_a_real_plane(oracle):
    y, p = _forest(oracle)
    order, pivots, n_residual, d = _forest_ref(oracle)
    print(f"forest [::4, ::4] {y.shape}, p = {p}: n_residual = {n_residual}, last residual pivot {pivots[n_residual - 1]:.3e}")
    assert p == 200 and 1 <= n_residual < p  # K_A runs out of rank at the 1e-10 cut
    assert np.unique(order).size == p
    ref = follow(y, order, FOREST[2], FOREST[3], n_residual)
    chosen = np.zeros(y.size, dtype=bool)
    chosen[order[:n_residual]] = True
    assert ref["d"][n_residual][~chosen].max() < NLE_EPS
    for k in range(n_residual, p):
        check_farthest_step(ref["m"][k], int(order[k]), pivots[k])


def test_residual_sampler_is_declared_exported_and_mirrored(nle):
    hdr = open(os.path.join(ROOT, "include", "nle.h")).read()
    assert "#define NLE_SAMPLER_RESIDUAL 3" in hdr and "#define NLE_SAMPLER_FARTHEST 1" in hdr and "2 is unused" in hdr
    assert "int nle_sample_pixels_order(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples" in hdr
    assert "long long nle_residual_sampler_bytes(int H, int W, int n_row_samples, int n_col_samples);" in hdr
    from nle_amd import _abi
    assert _abi.NLE_SAMPLER_RESIDUAL == 3 and nle.SAMPLER_RESIDUAL == 3
    assert {nle.SAMPLER_GRID, nle.SAMPLER_FARTHEST, nle.SAMPLER_RESIDUAL} == {0, 1, 3}  # what set_sampler accepts
    for name in ("nle_sample_pixels_order", "nle_residual_sampler_bytes"):
        assert name in _abi.SIGNATURES and name in nle.EXPORTED_SYMBOLS
        assert hasattr(nle.lib(), name)  # exported by the built library
    assert callable(getattr(nle.Context, "sample_pixels_order", None))
    hpp = open(os.path.join(ROOT, "include", "nle", "filter.hpp")).read()
    assert "NLE_SAMPLER_RESIDUAL" in hpp and "samplePixels() const;" in hpp


@pytest.mark.parametrize("case", [(267, 400, 10, 20), (37, 53, 6, 7), (3, 4, 3, 4), (4096, 4096, 20, 10), (8192, 8192, 30, 30)])
def test_residual_sampler_bytes_is_the_formula(nle, oracle, case):
    H, W, nr, nc = case
    p = tsa.grid_count(oracle, H, W, nr, nc)
    assert nle.residual_sampler_bytes(H, W, nr, nc) == ((H * W + 1) // 2 * 2) * p * 8
    assert nle.residual_sampler_bytes(H, W, H + 1, nc) == -1


def test_the_issue_s_scale_figure(nle):
    assert round(nle.residual_sampler_bytes(8192, 8192, 30, 30) / 1e9) == 483  # 8192^2 with p = 900: 483 GB


@pytest.mark.parametrize("tool", [ENHANCE, DENOISE], ids=["enhance", "denoise"])
@pytest.mark.parametrize("lead", [["--sampler", "Residual"], ["--exact", "--sampler", "residual"],
                                  ["--sampler", "residual", "--exact"]], ids=["case", "exact_first", "exact_last"])
def test_cli_refuses_before_any_gpu_call(tool, lead, tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")  # no device is visible: the refusal must not need one
    out = tmp_path / "o.png"
    args = lead + [os.path.join(GOLDEN, "flower-50.bmp"), str(out)] + (FLOWER_ARGS if tool == ENHANCE else DENOISE_ARGS)
    r = subprocess.run([tool] + args, capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "--sampler" in r.stderr and "residual" in r.stderr
    assert r.stdout == "" and not out.exists()


# ------------------------------------------------------------------------------------------------------ GPU tests
@pytest.fixture
def rsctx(ctx):
    """the session ctx, handed back with the grid, no patches and auto mode whatever the test did"""
    yield ctx
    ctx.set_sampler(0)
    ctx.set_patch_radius(0)
    ctx.set_mode(0)


def _cases(oracle):
    rng = np.random.default_rng(7)
    return {
        "synthetic": (oracle.synthetic_luminance(48, 64), 6, 8, 12.0, 30.0),
        "scalar_tail": (oracle.synthetic_luminance(37, 53), 6, 7, 12.0, 30.0),       # N % 4 = 1
        "unaligned": (oracle.synthetic_luminance(40, 44), 5, 6, 10.0, 30.0),         # a view one float into a buffer
        "tiny": (oracle.synthetic_luminance(5, 7), 3, 3, 3.0, 30.0),                 # fewer pixels than one workgroup
        "p1": (oracle.synthetic_luminance(9, 11), 1, 1, 4.0, 30.0),
        "p_equals_N": (oracle.synthetic_luminance(3, 4), 3, 4, 2.0, 30.0),
        "one_row": (oracle.synthetic_luminance(1, 300), 1, 40, 20.0, 30.0),
        "non_integer": (rng.uniform(-3.0, 300.0, (40, 52)).astype(np.float32), 5, 7, 9.0, 17.5),
        "constant": (np.full((33, 41), 128.0), 4, 6, 10.0, 30.0),                    # every luminance tie
        "large_hx": (oracle.synthetic_luminance(50, 70), 6, 7, 1e7, 25.0),           # rank limited by the levels: falls back
        "flower_half": (_L(oracle, "flower-50.bmp")[::2, ::2].copy(), 10, 20, 100.0, 30.0),  # k beyond any unroll or LDS chunk
        "forest": (_forest(oracle)[0],) + FOREST,
    }


CASE_P = {"tiny": 12, "p1": 1, "p_equals_N": 12, "one_row": 40, "flower_half": 200, "forest": 200}


def _device_plane(y, unaligned=False):
    import torch
    x = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float32), device="cuda:0")
    if not unaligned:
        return x
    buf = torch.empty(x.numel() + 1, dtype=torch.float32, device="cuda:0")
    v = buf[1:].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["synthetic", "scalar_tail", "unaligned", "tiny", "p1", "p_equals_N", "one_row", "non_integer",
                                  "constant", "large_hx", "flower_half", "forest"])
def test_device_follows_the_rule_along_its_own_order(nle, oracle, rsctx, case):
    y, nr, nc, hx, hy = _cases(oracle)[case]
    H, W = y.shape
    p = tsa.grid_count(oracle, H, W, nr, nc)
    assert p == CASE_P.get(case, p) and p <= H * W
    x = _device_plane(y, unaligned=case == "unaligned")
    rsctx.set_sampler(nle.SAMPLER_RESIDUAL)
    got = rsctx.sample_pixels_order(x, nr, nc, hx, hy)
    order, pivot, n_residual = got["order"], got["pivot"], got["n_residual"]
    assert order.dtype == np.int64
    check_along_own_order(y, p, hx, hy, order, pivot, n_residual)
    sel = rsctx.sample_pixels(x, nr, nc, hx, hy)
    assert sel.dtype == np.int64 and np.array_equal(sel, np.sort(order))
    if case in ("large_hx", "forest"):  # the restatement itself falls back here, so the device must
        n_ref = _forest_ref(oracle)[2] if case == "forest" else residual_greedy(y, p, hx, hy)[2]
        assert n_ref < p and n_residual < p


@pytest.mark.gpu
def test_two_runs_are_bitwise_equal_on_a_plane_beyond_one_sweep(nle, oracle, rsctx):
    """1024 x 1536: more pixels than 2048 workgroups cover in one sweep (the grid-stride loop), a 1.2 GB factor"""
    y = oracle.synthetic_luminance(1024, 1536)
    x = _device_plane(y)
    rsctx.set_sampler(nle.SAMPLER_RESIDUAL)
    a = rsctx.sample_pixels_order(x, 8, 12, 300.0, 30.0)
    b = rsctx.sample_pixels_order(x, 8, 12, 300.0, 30.0)
    assert a["order"].size == 96 and np.unique(a["order"]).size == 96 and 1 <= a["n_residual"] <= 96
    assert nle.residual_sampler_bytes(1024, 1536, 8, 12) == 1024 * 1536 * 96 * 8
    for key in ("order", "pivot", "stats"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert a["n_residual"] == b["n_residual"]
    assert np.all(np.diff(a["pivot"][:a["n_residual"]]) <= tol(96))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["synthetic", "scalar_tail", "non_integer", "flower_half"])
def test_statistics_are_those_of_the_set(nle, oracle, rsctx, case):
    y, nr, nc, hx, hy = _cases(oracle)[case]
    H, W = y.shape
    N, p = H * W, tsa.grid_count(oracle, H, W, nr, nc)
    rsctx.set_sampler(nle.SAMPLER_RESIDUAL)
    got = rsctx.sample_pixels_order(y, nr, nc, hx, hy)
    assert got["n_residual"] == p, "this case is meant to stay with the residual rule"
    d = follow(y, got["order"], hx, hy)["d"][p]
    rest = np.ones(N, dtype=bool)
    rest[got["order"]] = False
    dm = np.where(rest, d, -np.inf)
    t = tol(p)
    mx, arg, total = got["stats"]
    print(f"{case}: max d {mx!r} vs {dm.max()!r}, argmax {int(arg)} vs {int(np.argmax(dm))}, sum {total!r} vs "
          f"{np.maximum(d, 0).sum()!r}")
    assert abs(mx - dm.max()) <= t
    assert abs(total - np.maximum(d, 0.0).sum()) <= N * t
    top = np.sort(dm)[-2:]
    if top[1] - top[0] > 2 * t:
        assert int(arg) == int(np.argmax(dm))
    else:
        assert rest[int(arg)] and d[int(arg)] >= dm.max() - 2 * t
    # max r and sum r of the residual map under this sampler, at test_nystrom_residual's own bar
    S = np.sort(got["order"])
    f, rr, cc, _, _ = _plane(y)
    sw, pw = 1.0 / (hx * hx), 1.0 / (hy * hy)
    Ka = np.stack([np.exp(-_D(f[S], rr[S], cc[S], j, sw, pw)) for j in range(p)])
    lam = np.linalg.eigvalsh(Ka)[::-1]
    lam = lam[lam >= NLE_EPS]
    bar = tnr.bars(d, p, lam, stored=False)
    _, s = tnr.run(rsctx, y, nr, nc, hx, hy, nle.RESID_ROWS, want_map=False)
    print(f"  nle_nystrom_residual: max {s['max']!r}, sum {s['sum']!r}, bar {bar:.2e}, kept {lam.size} of {p}")
    assert abs(s["max"] - mx) <= bar + t
    assert abs(s["sum"] - total) <= N * (bar + t)


def _train_on_device_set(nle, oracle, ctx, monkeypatch, y, nr, nc, hx, hy, T, K, L, R):
    H, W = y.shape
    ctx.set_sampler(nle.SAMPLER_RESIDUAL)
    ctx.set_patch_radius(0)
    S = ctx.sample_pixels(y, nr, nc, hx, hy)  # the DEVICE's set: every later stage is the oracle's own
    tsa.use_set(monkeypatch, oracle, H, W, S)
    if R == 0:
        info = []
        V_o, S_o = oracle.train_filter(y, nr, nc, hx, hy, T, K, info=info)
    else:
        import test_patch_affinity as tpa
        V_o, S_o, info = tpa.train_patch(oracle, y, nr, nc, hx, hy, T, K, R)
    return S, S_o, oracle.apply_layers(V_o, S_o, y, L).reshape(L, -1), [d["kept"] for d in info]


@pytest.mark.gpu
@pytest.mark.parametrize("plane,R", [("synthetic", 0), ("flower", 0), ("synthetic", 3)])
def test_train_apply_with_residual_meets_the_bars(nle, oracle, rsctx, monkeypatch, plane, R):
    if plane == "synthetic":
        H, W, nr, nc, hx, hy, T, K, L = tsa.SYNTH
        y = oracle.synthetic_luminance(H, W)
    else:
        y = _L(oracle, "flower-50.bmp").copy()
        nr, nc, hx, hy, T, K, L = FLOWER["nr"], FLOWER["nc"], FLOWER["hx"], FLOWER["hy"], FLOWER["T"], FLOWER["K"], 4
    S, S_o, Y_o, cuts = _train_on_device_set(nle, oracle, rsctx, monkeypatch, y, nr, nc, hx, hy, T, K, L, R)
    rsctx.set_patch_radius(R)
    results = {}
    for mode in (nle.MODE_MATERIALISED_F64, nle.MODE_STREAMED_F64, nle.MODE_AUTO):
        rsctx.set_mode(mode)
        f, Y = tsa._with_chunks(mode, lambda: tsa._train_apply(nle, rsctx, y, nr, nc, hx, hy, T, K, L))
        d = f.diag()
        assert d["formulation"] == (nle.MODE_MATERIALISED_F64 if mode == nle.MODE_AUTO else mode)
        assert np.array_equal(f.sample_pixels(), S)
        assert [d["r_Ka"], d["r_Wa"], d["r_Q"]] == cuts
        assert d["K"] == S_o.size
        ev_err = rel_l2(f.eigvals, S_o)
        errs = [rel_l2(Y[j], Y_o[j]) for j in range(L)]
        print(f"{plane} R = {R} mode {mode}: cuts {cuts}, eigenvalues {ev_err:.1e}, per-layer", ["%.1e" % e for e in errs])
        assert ev_err < 1e-8
        assert max(errs) < tsa.PER_LAYER_TOL
        results[mode] = Y
        f.close()
    for j in range(L):
        assert rel_l2(results[nle.MODE_STREAMED_F64][j], results[nle.MODE_MATERIALISED_F64][j]) < 1e-6


def _layer_errors(nle, oracle, ctx, y, nr, nc, hx, hy, T, K, L, samplers):
    ex = tsa._exact_layers(oracle, y, hx, hy, T, K, L)
    err, max_r = {}, {}
    for name, s in samplers:
        ctx.set_sampler(s)
        f, Y = tsa._train_apply(nle, ctx, y, nr, nc, hx, hy, T, K, L)
        f.close()
        err[name] = [rel_l2(Y[j], ex[j]) for j in range(L)]
        max_r[name] = tnr.run(ctx, y, nr, nc, hx, hy, nle.RESID_AUTO, want_map=False)[1]["max"]
    print("relative error against the exact filter per layer:", {k: ["%.4f" % e for e in v] for k, v in err.items()},
          "max r:", {k: "%.3e" % v for k, v in max_r.items()})
    return err, max_r


@pytest.mark.gpu
def test_residual_is_closer_to_the_exact_filter_on_a_flower_crop(nle, oracle, rsctx):
    """CPU values: layer 1 0.317 grid / 0.0069 farthest / 0.0010 residual; max r 3.4e-2 farthest / 5.1e-3 residual"""
    y = np.load(os.path.join(GOLDEN, "flower_cfg1.npz"))["L_in"].astype(np.float64)[100:160, 150:240]
    err, max_r = _layer_errors(nle, oracle, rsctx, y, 6, 9, 100.0, 30.0, 50, 30, 4,
                               (("grid", nle.SAMPLER_GRID), ("farthest", nle.SAMPLER_FARTHEST), ("residual", nle.SAMPLER_RESIDUAL)))
    assert 4 * err["residual"][0] <= err["grid"][0]
    assert max_r["residual"] < max_r["farthest"]


@pytest.mark.gpu
def test_residual_beats_farthest_on_the_bird_crop(nle, oracle, rsctx):
    """the crop that keeps farthest opt-in (profiles/r5_sampler_quality.txt).  CPU values: layer 1 0.49 grid / 1.66 farthest /
    0.62 residual -- better than farthest, NOT better than the grid"""
    full = _L(oracle, "bird.bmp")
    H, W = full.shape
    y = full[H // 2 - 30:H // 2 + 30, W // 2 - 45:W // 2 + 45]
    err, _ = _layer_errors(nle, oracle, rsctx, y, 6, 9, 100.0, 20.0, 10, 10, 4,
                           (("farthest", nle.SAMPLER_FARTHEST), ("residual", nle.SAMPLER_RESIDUAL)))
    assert err["residual"][0] < err["farthest"][0]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 4], ids=["auto_tables", "materialised_f64"])
def test_grid_and_farthest_are_what_they_were(nle, oracle, rsctx, mode):
    H, W, nr, nc, hx, hy, T, K, L = tsa.SYNTH
    y = oracle.synthetic_luminance(H, W)
    fresh = nle.Context(0)
    try:
        fresh.set_mode(mode)
        f0, Y0 = tsa._train_apply(nle, fresh, y, nr, nc, hx, hy, T, K, L)
        if mode == 0:
            assert f0.diag()["formulation"] == nle.MODE_PHI_FREE  # the tables
        rsctx.set_mode(mode)
        rsctx.set_sampler(nle.SAMPLER_GRID)
        f1, Y1 = tsa._train_apply(nle, rsctx, y, nr, nc, hx, hy, T, K, L)
        rsctx.set_sampler(nle.SAMPLER_RESIDUAL)
        rsctx.sample_pixels_order(y, nr, nc, hx, hy)
        rsctx.set_sampler(nle.SAMPLER_GRID)
        f2, Y2 = tsa._train_apply(nle, rsctx, y, nr, nc, hx, hy, T, K, L)
        for f, Y in ((f1, Y1), (f2, Y2)):
            assert f0.diag() == f.diag()
            assert np.array_equal(f0.eigvals, f.eigvals) and np.array_equal(Y0, Y)
            assert np.array_equal(f.sample_pixels(), oracle.sample_pixels(H, W, nr, nc)[0])
        for f in (f0, f1, f2):
            f.close()
        # farthest's set: the numpy rule of tests/test_sampler.py, before and after a residual call on the same ctx
        want = tsa.farthest(y, tsa.grid_count(oracle, H, W, nr, nc), hx, hy)
        rsctx.set_sampler(nle.SAMPLER_FARTHEST)
        assert np.array_equal(rsctx.sample_pixels(y, nr, nc, hx, hy), want)
        rsctx.set_sampler(nle.SAMPLER_RESIDUAL)
        rsctx.sample_pixels(y, nr, nc, hx, hy)
        rsctx.set_sampler(nle.SAMPLER_FARTHEST)
        assert np.array_equal(rsctx.sample_pixels(y, nr, nc, hx, hy), want)
    finally:
        fresh.close()


@pytest.mark.gpu
def test_refusals_leave_the_ctx_usable(nle, oracle, rsctx):
    H, W, nr, nc, hx, hy, T, K, L = 40, 56, 4, 5, 12.0, 30.0, 5, 6, 3
    y = oracle.synthetic_luminance(H, W)
    y32 = y.astype(np.float32)

    def trains():
        rsctx.set_sampler(nle.SAMPLER_RESIDUAL)
        rsctx.set_mode(0)
        f, _ = tsa._train_apply(nle, rsctx, y, nr, nc, hx, hy, T, K, L)
        assert f.diag()["formulation"] == nle.MODE_MATERIALISED_F64
        f.close()

    def refused(fn, word=None):
        with pytest.raises(nle.NLEError) as e:
            fn()
        assert e.value.code == nle.NLE_ERR_INVALID
        print("refused:", e.value)
        if word:
            assert word in str(e.value)
        trains()  # the ctx is still usable

    rsctx.set_sampler(nle.SAMPLER_RESIDUAL)
    for mode in (nle.MODE_MATERIALISED, nle.MODE_PHI_FREE, nle.MODE_PHI_FREE_EXP, nle.MODE_EXACT_F64):
        def in_mode():
            rsctx.set_mode(mode)
            tsa._train_apply(nle, rsctx, y, nr, nc, hx, hy, T, K, L)
        refused(in_mode, "the residual sampler" if mode != nle.MODE_EXACT_F64 else None)
    refused(lambda: rsctx.compute_kernel(y32, nr, nc, hx, hy))  # the fp32 stage entry points
    refused(lambda: rsctx.nystrom(y32, nr, nc, hx, hy))
    refused(lambda: rsctx.sample_pixels(y32, nr, nc, 0.0, hy))
    refused(lambda: rsctx.sample_pixels_order(y32, nr, nc, hx, -1.0))
    refused(lambda: tsa._train_apply(nle, rsctx, y, nr, nc, 0.0, hy, T, K, L))
    for other in (nle.SAMPLER_GRID, nle.SAMPLER_FARTHEST):
        def under_other():
            rsctx.set_sampler(other)
            rsctx.sample_pixels_order(y32, nr, nc, hx, hy)
        refused(under_other, "residual")
    big = oracle.synthetic_luminance(50, 50).astype(np.float32)
    assert tsa.grid_count(oracle, 50, 50, 46, 46) > 2048
    refused(lambda: rsctx.sample_pixels_order(big, 46, 46, hx, hy), "2048")
    refused(lambda: rsctx.sample_pixels(big, 46, 46, hx, hy), "2048")
    refused(lambda: tnr.run(rsctx, y, nr, nc, hx, hy, nle.RESID_FUSED))
    refused(lambda: rsctx.set_sampler(2))  # unused
    rsctx.set_sampler(nle.SAMPLER_GRID)
    f, Y = tsa._train_apply(nle, rsctx, y, nr, nc, hx, hy, T, K, L)
    V_o, S_o = oracle.train_filter(y, nr, nc, hx, hy, T, K)
    Y_o = oracle.apply_layers(V_o, S_o, y, L).reshape(L, -1)
    assert max(rel_l2(Y[j], Y_o[j]) for j in range(L)) < tsa.PER_LAYER_TOL
    f.close()


# ------------------------------------------------------------------------------------------------------ multi-rank
def _worker(rank, world, port, args, outdir, slabs):
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
        H, W, nr, nc, hx, hy, T, K, L = args
        x = synth.synthetic_luminance(H, W).astype(np.float32)
        ctx = nle.Context(0)
        ctx.set_sampler(nle.SAMPLER_RESIDUAL)
        g = nle.sample_grid(H, W, nr, nc)
        ctx.set_shard(rank, world, g["n_sel_rows"] * g["n_sel_cols"], lambda t: dist.all_reduce(t))

        def code_of(fn):
            try:
                fn()
                return 0
            except nle.NLEError as e:
                return e.code

        if slabs:
            ctx.set_slab_input(True)
            r0, r1 = nle.slab_rows(H, rank, world)
            code = code_of(lambda: nle.NLEFilter(ctx).train_filter(np.ascontiguousarray(x[r0:r1]), nr, nc, hx, hy, T, K,
                                                                   shape=(H, W)))
            np.savez(os.path.join(outdir, f"rank{rank}.npz"), code=np.array([code]))
        else:
            order_code = code_of(lambda: ctx.sample_pixels_order(x, nr, nc, hx, hy))  # refused before any collective
            sel = ctx.sample_pixels(x, nr, nc, hx, hy)
            f = nle.NLEFilter(ctx).train_filter(x, nr, nc, hx, hy, T, K)
            Y = f.apply_layers(x, L).cpu().numpy()
            info = f.info()
            np.savez(os.path.join(outdir, f"rank{rank}.npz"), Y=Y, S=f.eigvals, sel=sel, fsel=f.sample_pixels(),
                     form=np.array([f.diag()["formulation"]]), rows=np.array([info["row0"], info["row1"]]),
                     order_code=np.array([order_code]))
            f.close()
        ctx.close()
    finally:
        dist.destroy_process_group()


def _spawn_two(tmp_path, slabs, limit=240.0):
    """two workers, each under its own time limit"""
    import torch.multiprocessing as mp
    pc = mp.spawn(_worker, args=(2, tsa._free_port(), tsa.MR, str(tmp_path), slabs), nprocs=2, join=False)
    deadline = time.monotonic() + limit
    while not pc.join(timeout=2.0):
        if time.monotonic() > deadline:
            for pr in pc.processes:
                if pr.is_alive():
                    pr.kill()
            pytest.fail("a worker ran past its time limit")


@pytest.mark.gpu
def test_two_ranks_with_residual_match_single_rank(nle, rsctx, tmp_path):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
    H, W, nr, nc, hx, hy, T, K, L = tsa.MR
    x = synth.synthetic_luminance(H, W)
    rsctx.set_sampler(nle.SAMPLER_RESIDUAL)
    f1, Y1 = tsa._train_apply(nle, rsctx, x, nr, nc, hx, hy, T, K, L)
    S1, sel1 = f1.eigvals, f1.sample_pixels()
    f1.close()
    assert np.array_equal(sel1, np.sort(rsctx.sample_pixels_order(x, nr, nc, hx, hy)["order"]))
    _spawn_two(tmp_path, False)
    Y = np.zeros((L, H * W))
    for r in range(2):
        d = np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))
        r0, r1 = d["rows"]
        Y[:, r0 * W:r1 * W] = d["Y"]
        assert np.array_equal(d["sel"], sel1) and np.array_equal(d["fsel"], sel1)
        assert int(d["form"][0]) == nle.MODE_MATERIALISED_F64
        assert int(d["order_code"][0]) == nle.NLE_ERR_INVALID
        assert rel_l2(d["S"], S1) < 1e-9
    for j in range(L):
        assert rel_l2(Y[j], Y1[j]) < 1e-6, j


@pytest.mark.gpu
def test_slab_input_with_residual_is_refused_on_every_rank(nle, tmp_path):
    _spawn_two(tmp_path, True)
    for r in range(2):
        assert int(np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))["code"][0]) == nle.NLE_ERR_INVALID


# ------------------------------------------------------------------------------------------------------ CLI and C++
@pytest.mark.gpu
def test_enhance_with_residual_matches_the_python_mirror(nle, oracle, rsctx, tmp_path):
    from PIL import Image
    import torch
    src = tsa._load_bgr("flower-50.bmp")
    out = tmp_path / "flower-res.png"
    r = subprocess.run([ENHANCE, "--sampler", "residual", os.path.join(GOLDEN, "flower-50.bmp"), str(out)] + FLOWER_ARGS,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    got = np.asarray(Image.open(str(out)).convert("RGB"))[..., ::-1]
    # the same pipeline through the Python mirror: bgr2lab8 -> train_host_u8 -> apply_u8_host -> lab2bgr8
    rsctx.set_sampler(nle.SAMPLER_RESIDUAL)
    H, W = src.shape[:2]
    lab, _ = rsctx.bgr2lab8(src)
    L8 = lab[..., 0].cpu().numpy().copy()
    f = nle.NLEFilter(rsctx).train_filter_host_u8(L8, FLOWER["nr"], FLOWER["nc"], FLOWER["hx"], FLOWER["hy"], FLOWER["T"],
                                                  FLOWER["K"])
    assert np.array_equal(f.sample_pixels(), rsctx.sample_pixels(L8.astype(np.float32), FLOWER["nr"], FLOWER["nc"], FLOWER["hx"],
                                                                 FLOWER["hy"]))
    fS = oracle.transform_eigenvalues(f.eigvals, FLOWER["weights"])
    y8 = np.empty(H * W, dtype=np.uint8)
    f.apply_u8_host(None, fS, y8)
    f.close()
    Lf = torch.as_tensor(y8.reshape(H, W).astype(np.float32), device=lab.device)
    mirror = rsctx.lab2bgr8(lab, L=Lf).cpu().numpy()
    assert np.array_equal(got, mirror)


@pytest.mark.gpu
@pytest.mark.parametrize("lead", [["--sampler", "residual"], ["--patch-radius", "2", "--sampler", "residual"]],
                         ids=["residual", "residual_after_radius"])
def test_denoise_with_residual_runs(tmp_path, lead):
    out = tmp_path / "flower-dn.png"
    r = subprocess.run([DENOISE] + lead + [os.path.join(GOLDEN, "flower-50.bmp"), str(out)] + DENOISE_ARGS,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert out.exists() and out.stat().st_size > 0


@pytest.mark.gpu
def test_enhance_report_with_residual_prints_its_line(nle, rsctx, tmp_path):
    out = tmp_path / "o.png"
    r = subprocess.run([ENHANCE, "--nystrom-report", "--sampler", "residual", "--chroma", "20", "--patch-radius", "1",
                        os.path.join(GOLDEN, "flower-50.bmp"), str(out)] + FLOWER_ARGS, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines()[-1].startswith("Nystrom residual: mean ") and out.exists()


CPP_DRIVER = textwrap.dedent(r"""
    #include <cmath>
    #include <cstdio>
    #include <vector>
    #include "nle.h"
    #include "nle/filter.hpp"
    #define REQUIRE(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); return 1; } } while (0)
    int main() {
        const int H = 37, W = 53, nr = 5, nc = 6;
        const double hx = 9.0, hy = 25.0;
        const size_t n = (size_t)H * W;
        nle::Image L(H, W, nle::NLE_64F, 1);
        std::vector<float> lum(n);
        for (int r = 0; r < H; ++r)
            for (int c = 0; c < W; ++c) {
                const double v = std::floor(128 + 60 * std::sin(0.2 * r) * std::cos(0.15 * c) + 20 * ((r * 7 + c * 13) % 5) / 5.0);
                L.at<double>(r, c) = v;
                lum[(size_t)r * W + c] = (float)v;
            }
        nle_ctx* c = nullptr;
        REQUIRE(nle_ctx_create(0, nullptr, &c) == NLE_OK);
        void* d_lum = nullptr;
        REQUIRE(nle_dev_alloc(c, n * 4, &d_lum) == NLE_OK && nle_dev_upload(c, d_lum, lum.data(), n * 4) == NLE_OK);
        int p = 0, p2 = 0, nres = 0;
        std::vector<long long> grid(n), set(n), order(n);
        std::vector<double> pivot(n);
        REQUIRE(nle_sample_pixels(c, (const float*)d_lum, H, W, nr, nc, hx, hy, grid.data(), &p) == NLE_OK && p == 30);
        REQUIRE(nle_ctx_set_sampler(c, NLE_SAMPLER_RESIDUAL) == NLE_OK);
        REQUIRE(nle_sample_pixels(c, (const float*)d_lum, H, W, nr, nc, hx, hy, set.data(), &p) == NLE_OK && p == 30);
        REQUIRE(nle_sample_pixels_order(c, (const float*)d_lum, H, W, nr, nc, hx, hy, order.data(), pivot.data(), &p2, &nres,
                                        nullptr) == NLE_OK && p2 == p && nres >= 1 && nres <= p);
        REQUIRE(order[0] == (long long)(H / 2) * W + W / 2 && pivot[0] == 1.0);
        nle::NLEFilter f;
        f.verbose = false;
        f.sampler = NLE_SAMPLER_RESIDUAL;
        REQUIRE(f.sampler == 3);
        f.trainFilter(L, nr, nc, hx, hy, 10, 8);
        const std::vector<long long> got = f.samplePixels();
        REQUIRE((int)got.size() == p);
        bool same = true, is_grid = true;
        for (int k = 0; k < p; ++k) same = same && got[k] == set[k], is_grid = is_grid && got[k] == grid[k];
        REQUIRE(same && !is_grid);
        nle::NLEFilter g;  // the shared ctx is back at the grid
        g.verbose = false;
        g.trainFilter(L, nr, nc, hx, hy, 10, 8);
        const std::vector<long long> gg = g.samplePixels();
        for (int k = 0; k < p; ++k) REQUIRE(gg[k] == grid[k]);
        nle_dev_free(c, d_lum);
        nle_ctx_destroy(c);
        std::printf("residual sampler OK\n");
        return 0;
    }
""")


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_cpp_sampler_3_trains_on_the_c_abi_s_set(tmp_path):
    host = os.path.join(PKG_DIR, "host")
    libdir = os.path.join(PKG_DIR, "lib")
    (tmp_path / "drv.cpp").write_text(CPP_DRIVER)
    b = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(tmp_path / "drv.cpp"),
                        *[os.path.join(host, s) for s in ("filter.cpp", "stages.cpp", "colour.cpp", "device_group.cpp", "image_io.cpp", "jpeg.cpp")],
                        "-L", libdir, "-lnle_hip", "-Wl,-rpath," + libdir, "-o", str(tmp_path / "drv")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "drv")], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "residual sampler OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-1000:])
