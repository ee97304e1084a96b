"""The Nystrom residual map: nle_nystrom_residual / Context.nystrom_residual / NLEFilter::nystromResidual /
`enhance --nystrom-report [--nystrom-map FILE]`.

The restatement is the definition of include/nle.h in the oracle's terms: with (perm, Ka, Kab) = oracle.compute_kernel (or the
patch / chroma / farthest restatements of the other test modules) and (eigvals, phi) = oracle.nystrom_approximation(Ka, Kab),

    r[perm] = 1 - (phi^2 . eigvals).sum(1)

the diagonal of K - K~ for the extension a train uses (K~ = phi diag(eigvals) phi^T).

The bar of the GPU tests, per pixel i, is

    bar_i = u p (8 + cond2) + 2^-24 |r_i|,    u = 2^-53, cond2 = lambda_max / lambda_min(kept) of K_A (numpy)

Derivation.  The device computes r_i = 1 - || F^T k_i ||^2 with F F^T = pinv(K_A) (F = V diag(1 / sqrt(lambda)), or L^-T on the
Cholesky route).  (a) The m <= p dot products of length p and the sum of their squares are sums of terms of magnitude at most 1
(affinities are in (0, 1], || F^T k_i ||^2 <= K_ii = 1 because K - K~ is positive semi-definite): recursive summation in fp64
errs by at most gamma_p per dot product relative to sum |terms|, which carried through the square and the second sum is bounded
by 8 u p (a generous constant for 2 gamma_p + gamma_m + the libm exp's ulp and the final subtraction).  (b) The factorisation
(eigensolver or Cholesky) is backward stable: it is the exact factorisation of K_A + E with || E ||_2 <= gamma_p || K_A ||_2, so
x^T pinv(K_A + E) x differs from x^T pinv(K_A) x by at most about || E || / lambda_min || pinv^(1/2) x ||^2 <= u p cond2 for
x = k_i (again || pinv^(1/2) k_i ||^2 <= 1).  (c) The map is stored as fp32: a relative half-ulp, 2^-24 |r_i|.  The summary
is computed from the unrounded fp64 values, so its bars leave (c) out; the argmax must equal the restatement's wherever the
runner-up is further away than the bar, and otherwise be a pixel within two bars of the maximum (both values carry an error).  Both routes and both factorisations are held to
the same bar; on the CPU the eigen and the Cholesky route differ from a longdouble evaluation by at most 0.06 of it."""
import ctypes as C
import os
import shutil
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import GOLDEN, PKG_DIR, ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_chroma_affinity as tca  # noqa: E402
import test_patch_affinity as tpa  # noqa: E402
import test_sampler as tsa  # noqa: E402

ENHANCE, DENOISE = tpa.ENHANCE, tpa.DENOISE
FLOWER, FLOWER_ARGS, DENOISE_ARGS = tpa.FLOWER, tpa.FLOWER_ARGS, tpa.DENOISE_ARGS
U = 2.0 ** -53

# H, W, nr, nc, hx, hy, p (as the issue's table states it; checked against the oracle's grid)
CASES = {
    "ragged": (37, 53, 6, 7, 12.0, 30.0, 42),       # not a multiple of 16 or 4; the last 128-pixel tile ragged
    "sq_hx16": (64, 64, 8, 8, 16.0, 30.0, 64),
    "sq_hx40": (64, 64, 8, 8, 40.0, 30.0, 64),
    "one_row": (1, 300, 1, 17, 40.0, 25.0, 17),
    "panels": (120, 160, 10, 20, 40.0, 30.0, 200),  # 13 column tiles, m not a multiple of 16; several staged chunks
    "p255": (45, 51, 15, 17, 3.0, 30.0, 255),       # FUSED: the widest instantiation (16 column tiles), the last one ragged;
                                                    # the narrowest (m <= 16) is the rank-truncated case below (m = 10)
    "p288": (120, 160, 16, 18, 30.0, 20.0, 288),    # ROWS only: FUSED must refuse (and the device Cholesky factors K_A)
}
FUSED_CASES = [k for k, c in CASES.items() if c[6] <= 256]
# a constant plane whose K_A is rank deficient at the cut with a clean gap on both sides (asserted below)
TRUNCATED = (48, 48, 6, 6, 600.0, 30.0)


# ----------------------------------------------------------------------------------------------- the restatement
def residual(oracle, perm, Ka, Kab):
    """(r in natural pixel order, eigenvalues kept): 1 - (phi^2 . eigvals).sum(1), un-permuted"""
    lam, phi = oracle.nystrom_approximation(Ka, Kab)
    r = np.empty(perm.size)
    r[perm] = 1.0 - (phi * phi * lam[None, :]).sum(1)
    return r, lam


def bars(r, p, lam, stored=True):
    return U * p * (8.0 + lam[0] / lam[-1]) + (2.0 ** -24 * np.abs(r) if stored else 0.0)


_refs = {}


def ref(oracle, key):
    """the restated map of a case, computed once and shared: (y, r, lam, p)"""
    if key not in _refs:
        H, W, nr, nc, hx, hy = (CASES[key] if key in CASES else TRUNCATED)[:6]
        y = oracle.synthetic_luminance(H, W) if key in CASES else np.full((H, W), 128.0)
        perm, Ka, Kab = oracle.compute_kernel(y, nr, nc, hx, hy)
        r, lam = residual(oracle, perm, Ka, Kab)
        r.setflags(write=False)
        _refs[key] = (y, r, lam, Ka.shape[0])
    return _refs[key]


def brute(oracle, y, nr, nc, hx, hy):
    """(K N x N, K~ = Kab_full^T pinv(Ka) Kab_full, Ka) in natural pixel order, from the full pairwise affinity"""
    H, W = y.shape
    idx = np.arange(H * W)
    f = y.ravel()
    K = np.exp(oracle._neg_weighted_distance(y, idx // W, idx % W, f, idx // W, idx % W, f, 1.0 / (hx * hx), 1.0 / (hy * hy)))
    sel = oracle.sample_pixels(H, W, nr, nc)[0]
    Ka, Kab_full = K[np.ix_(sel, sel)], K[sel, :]
    return K, Kab_full.T @ np.linalg.pinv(Ka, hermitian=True) @ Kab_full, Ka, sel


# ------------------------------------------------------------------------------------------------------ CPU tests
SMALL = (20, 24, 4, 4, 6.0, 30.0)


def _small(oracle):
    H, W, nr, nc, hx, hy = SMALL
    y = oracle.synthetic_luminance(H, W)
    perm, Ka, Kab = oracle.compute_kernel(y, nr, nc, hx, hy)
    r, lam = residual(oracle, perm, Ka, Kab)
    return y, r, lam, Ka.shape[0]


def test_restatement_equals_the_brute_force_diagonal(oracle):
    y, r, lam, p = _small(oracle)
    K, Kt, Ka, _ = brute(oracle, y, *SMALL[2:])
    assert lam.size == p  # full rank: pinv is the inverse
    np.testing.assert_allclose(r, np.diag(K - Kt), rtol=0, atol=U * p * (8.0 + lam[0] / lam[-1]))


def test_restatement_is_non_negative_and_zero_at_the_samples(oracle):
    y, r, lam, p = _small(oracle)
    assert r.min() >= -1e-12 and r.max() <= 1.0
    sel = oracle.sample_pixels(*SMALL[:4])[0]
    assert lam.size == p and np.abs(r[sel]).max() <= 1e-12
    for key in ("ragged", "one_row"):
        _, rr, ll, pp = ref(oracle, key)
        assert rr.min() >= -1e-12 and rr.max() <= 1.0
        assert np.abs(rr[oracle.sample_pixels(*CASES[key][:4])[0]]).max() <= 1e-12


def test_restatement_sums_to_the_nuclear_norm_of_the_extension_error(oracle):
    y, r, lam, p = _small(oracle)
    K, Kt, _, _ = brute(oracle, y, *SMALL[2:])
    nuc = np.abs(np.linalg.eigvalsh(K - Kt)).sum()
    assert abs(r.sum() - nuc) <= 1e-10 * nuc
    # and the entrywise bound that positive semi-definiteness gives
    assert np.all(np.abs(K - Kt) <= np.sqrt(np.maximum(np.outer(r, r), 0.0)) + 1e-12)


def test_the_issue_s_two_cpu_figures(oracle):
    _, r, _, _ = ref(oracle, "ragged")
    assert abs(r.mean() - 0.26) < 0.005 and abs(r.max() - 0.998) < 0.001
    _, r, _, _ = ref(oracle, "panels")
    assert abs(r.mean() - 0.010) < 0.001


def test_case_table_matches_the_oracle_s_grid_and_conditioning(oracle):
    want_cond = {"ragged": 76, "sq_hx16": 93, "sq_hx40": 1.9e4, "panels": 2.5e5, "p288": 2.9e4}
    for key, c in CASES.items():
        _, r, lam, p = ref(oracle, key)
        assert p == c[6] == lam.size  # full rank at the cut
        if key in want_cond:
            assert abs(lam[0] / lam[-1] / want_cond[key] - 1.0) < 0.05
        if lam[0] / lam[-1] <= 1e6:
            assert bars(r, p, lam).max() <= 2.2e-8 + 2.0 ** -24


def test_truncated_case_has_a_clean_gap_at_the_cut(oracle):
    H, W, nr, nc, hx, hy = TRUNCATED
    _, Ka, _ = oracle.compute_kernel(np.full((H, W), 128.0), nr, nc, hx, hy)
    w = np.linalg.eigvalsh(Ka)[::-1]
    k = int((w >= 1e-10).sum())
    assert 0 < k < w.size and np.all(w[:k] >= 1e-10)       # a leading run, rank deficient at the cut
    assert w[k - 1] >= 10 * 1e-10 and abs(w[k]) <= 1e-10 / 10


def test_residual_is_declared_exported_and_mirrored(nle):
    hdr = open(os.path.join(ROOT, "include", "nle.h")).read()
    for line in ("#define NLE_RESID_AUTO 0", "#define NLE_RESID_ROWS 1", "#define NLE_RESID_FUSED 2",
                 "int nle_nystrom_residual(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples, int n_col_samples,"):
        assert line in hdr
    from nle_amd import _abi
    assert (_abi.NLE_RESID_AUTO, _abi.NLE_RESID_ROWS, _abi.NLE_RESID_FUSED) == (0, 1, 2)
    assert (nle.RESID_AUTO, nle.RESID_ROWS, nle.RESID_FUSED) == (0, 1, 2)
    assert "nle_nystrom_residual" in _abi.SIGNATURES and "nle_nystrom_residual" in nle.EXPORTED_SYMBOLS
    assert hasattr(nle.lib(), "nle_nystrom_residual")  # exported by the built library
    assert callable(getattr(nle.Context, "nystrom_residual", None))
    assert "Residual nystromResidual(" in open(os.path.join(ROOT, "include", "nle", "filter.hpp")).read()
    assert nle._abi.NLE_K_NYSTROM == 1 and nle.KERNEL_COUNT == 12  # the NLE_K_* ids did not move


@pytest.mark.parametrize("tool,lead", [(ENHANCE, ["--exact", "--nystrom-report"]), (ENHANCE, ["--nystrom-report", "--exact"]),
                                       (ENHANCE, ["--nystrom-map", "m.png", "--exact", "--nystrom-report"]),
                                       (ENHANCE, ["--exact", "--nystrom-map", "m.png"]), (ENHANCE, ["--nystrom-map", "m.png"]),
                                       (ENHANCE, ["--nystrom-report=1"]),
                                       (DENOISE, ["--nystrom-report"]), (DENOISE, ["--nystrom-map", "m.png"]),
                                       (DENOISE, ["--sampler", "farthest", "--nystrom-report", "--nystrom-map", "m.png"])],
                         ids=["exact_report", "report_exact", "map_exact_report", "exact_map", "map_alone", "report_with_value", "denoise_report", "denoise_map", "denoise_both"])
def test_cli_refuses_before_any_gpu_call(tool, lead, tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")  # no device is visible: the refusal must not need one
    out = tmp_path / "o.png"
    lead = [str(tmp_path / v) if v == "m.png" else v for v in lead]
    tail = FLOWER_ARGS if tool == ENHANCE else DENOISE_ARGS
    r = subprocess.run([tool] + lead + [os.path.join(GOLDEN, "flower-50.bmp"), str(out)] + tail, capture_output=True, text=True,
                       timeout=60, env=env)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "--nystrom" in r.stderr and r.stdout == ""
    assert not out.exists() and not (tmp_path / "m.png").exists()


# ------------------------------------------------------------------------------------------------------ GPU tests
@pytest.fixture
def rctx(ctx):
    """the session ctx, handed back with the reference's affinity, the grid and auto mode whatever the test did"""
    yield ctx
    ctx.set_chroma(None, None, 0.0)
    ctx.set_patch_radius(0)
    ctx.set_sampler(0)
    ctx.set_mode(0)


def run(ctx, y, nr, nc, hx, hy, form, thresh=0.5, want_map=True):
    r, s = ctx.nystrom_residual(np.asarray(y, dtype=np.float32), nr, nc, hx, hy, form=form, thresh=thresh, want_map=want_map)
    return (r.cpu().numpy().ravel() if want_map else None), s


def check_map(what, got, want, p, lam):
    assert got.dtype == np.float32 and got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want)
    bar = bars(want, p, lam)
    i = int(np.argmax(err / bar))
    print(f"{what}: N = {want.size}, p = {p}, kept {lam.size}, cond2 = {lam[0] / lam[-1]:.3g}, mean r = {want.mean():.4g}, "
          f"max r = {want.max():.4g}; largest error / bar = {err[i]:.3e} / {bar[i]:.3e} at pixel {i}")
    assert np.all(err <= bar)


def check_summary(what, s, want, p, lam, thresh):
    bar = bars(want, p, lam, stored=False)  # a scalar: the summary comes from the unrounded values
    N = want.size
    print(f"{what}: sum {s['sum']!r} vs {want.sum()!r}, max {s['max']!r} vs {want.max()!r}, argmax {s['argmax']} vs "
          f"{int(np.argmax(want))}, count(r > {thresh}) {s['count']} vs {int((want > thresh).sum())}")
    assert abs(s["sum"] - want.sum()) <= 1e-12 * abs(want.sum()) + N * bar
    assert abs(s["max"] - want.max()) <= bar
    top = np.sort(want)[-2:]
    if top[1] - top[0] > bar:  # the runner-up is further away than the bar: the argmax is decided
        assert s["argmax"] == int(np.argmax(want))
    else:  # undecided at the bar: any pixel whose restated value is within two bars of the maximum
        assert want[s["argmax"]] >= want.max() - 2 * bar
    assert np.abs(want - thresh).min() > bar, "the test's threshold sits within a bar of some r_i: choose another"
    assert s["count"] == int((want > thresh).sum())


def pick_threshold(want, bar):
    """the first of a fixed list of thresholds that no r_i is within 4 bars of"""
    for t in (0.5, 0.25, 0.1, 0.75, 0.05, 0.9, 0.01):
        if np.abs(want - t).min() > 4 * bar:
            return t
    raise AssertionError("no threshold clear of every r_i")


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["rows", "fused", "auto"])
@pytest.mark.parametrize("key", list(CASES))
def test_map_and_summary_match_the_restatement(nle, oracle, rctx, key, form):
    H, W, nr, nc, hx, hy, p = CASES[key]
    y, want, lam, _ = ref(oracle, key)
    fid = {"rows": nle.RESID_ROWS, "fused": nle.RESID_FUSED, "auto": nle.RESID_AUTO}[form]
    t = pick_threshold(want, bars(want, p, lam, stored=False))
    if form == "fused" and key not in FUSED_CASES:
        with pytest.raises(nle.NLEError) as e:
            run(rctx, y, nr, nc, hx, hy, fid)
        assert e.value.code == nle.NLE_ERR_INVALID and "NLE_RESID_FUSED" in str(e.value)
        return
    got, s = run(rctx, y, nr, nc, hx, hy, fid, thresh=t)
    check_map(f"{key} {form}", got, want, p, lam)
    check_summary(f"{key} {form}", s, want, p, lam, t)
    # d_r = NULL gives the same summary, and a second run the same bits in map and summary
    _, s0 = run(rctx, y, nr, nc, hx, hy, fid, thresh=t, want_map=False)
    got2, s2 = run(rctx, y, nr, nc, hx, hy, fid, thresh=t)
    assert s0 == s and s2 == s and np.array_equal(got.view(np.uint32), got2.view(np.uint32))
    if form == "auto":  # AUTO is one of the two routes, bit for bit: FUSED where it applies, else ROWS
        route = nle.RESID_FUSED if key in FUSED_CASES else nle.RESID_ROWS
        got3, s3 = run(rctx, y, nr, nc, hx, hy, route, thresh=t)
        assert s3 == s and np.array_equal(got.view(np.uint32), got3.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["rows", "fused", "auto"])
def test_rank_truncated_spectrum(nle, oracle, rctx, form):
    H, W, nr, nc, hx, hy = TRUNCATED
    y, want, lam, p = ref(oracle, "truncated")
    assert p == 36 and 0 < lam.size < p and lam[-1] >= 1e-9  # (the gap itself: test_truncated_case_has_a_clean_gap_at_the_cut)
    fid = {"rows": nle.RESID_ROWS, "fused": nle.RESID_FUSED, "auto": nle.RESID_AUTO}[form]
    t = pick_threshold(want, bars(want, p, lam, stored=False))
    got, s = run(rctx, y, nr, nc, hx, hy, fid, thresh=t)
    check_map(f"truncated {form}", got, want, p, lam)
    check_summary(f"truncated {form}", s, want, p, lam, t)


def _restated_with_options(oracle, monkeypatch, opt):
    """(y, planes a and b or None, radius, sampler id, perm, Ka, Kab, args) for one option of the fp64 affinities"""
    if opt == "farthest":
        H, W, nr, nc, hx, hy = 37, 45, 5, 6, 9.0, 25.0
        y = oracle.synthetic_luminance(H, W)
        S = tsa.farthest(y, tsa.grid_count(oracle, H, W, nr, nc), hx, hy)
        tsa.use_set(monkeypatch, oracle, H, W, S)
        return y, None, None, 0, 1, oracle.compute_kernel(y, nr, nc, hx, hy), (nr, nc, hx, hy)
    if opt in ("patch1", "patch3"):
        H, W, nr, nc, hx, hy, R = 40, 52, 5, 6, 10.0, 25.0, int(opt[-1])
        y = oracle.synthetic_luminance(H, W)
        return y, None, None, R, 0, tpa.compute_kernel_patch(oracle, y, nr, nc, hx, hy, R), (nr, nc, hx, hy)
    nr, nc, hx, hy, hc = 5, 6, 9.0, 30.0, 20.0
    L, a, b = tca._lab(oracle, "synth:37:45")
    return L, a, b, 0, 0, tca.compute_kernel_chroma(oracle, L, a, b, nr, nc, hx, hy, hc, 0), (nr, nc, hx, hy, hc)


@pytest.mark.gpu
@pytest.mark.parametrize("opt", ["farthest", "patch1", "patch3", "chroma"])
def test_rows_under_the_affinity_options(nle, oracle, rctx, monkeypatch, opt):
    y, a, b, R, sampler, (perm, Ka, Kab), args = _restated_with_options(oracle, monkeypatch, opt)
    want, lam = residual(oracle, perm, Ka, Kab)
    p = Ka.shape[0]
    rctx.set_patch_radius(R)
    rctx.set_sampler(sampler)
    if a is not None:
        rctx.set_chroma(a, b, args[4])
    t = pick_threshold(want, bars(want, p, lam, stored=False))
    for form in (nle.RESID_ROWS, nle.RESID_AUTO):
        got, s = run(rctx, y, *args[:4], form, thresh=t)
        check_map(f"{opt} form {form}", got, want, p, lam)
        check_summary(f"{opt} form {form}", s, want, p, lam, t)
    with pytest.raises(nle.NLEError) as e:  # the fused form takes none of the options
        run(rctx, y, *args[:4], nle.RESID_FUSED)
    assert e.value.code == nle.NLE_ERR_INVALID
    # the option is really in the map: the plain call gives another one
    rctx.set_chroma(None, None, 0.0)
    rctx.set_patch_radius(0)
    rctx.set_sampler(0)
    plain, _ = run(rctx, y, *args[:4], nle.RESID_ROWS)
    assert not np.array_equal(plain, got)


@pytest.mark.gpu
def test_rows_in_several_chunks_equals_one_chunk_bit_for_bit(nle, oracle, rctx, monkeypatch):
    H, W, nr, nc, hx, hy, p = CASES["panels"]  # 19200 x 200 doubles of affinity rows: 30 chunks of 1 MiB
    y = ref(oracle, "panels")[0]
    names = [nle.lib().nle_kernel_name(k).decode() for k in range(nle.KERNEL_COUNT)]

    def counted(fn):
        rctx.profile(2)
        out = fn()
        st = rctx.kernel_stats()
        rctx.profile(False)
        return out, int(st[names[0]][0]), int(st[names[1]][0])  # NLE_K_AFFINITY, NLE_K_NYSTROM launches

    (one, s1), aff1, gemm1 = counted(lambda: run(rctx, y, nr, nc, hx, hy, nle.RESID_ROWS))
    monkeypatch.setenv("NLE_STREAM64_CHUNK_MB", "1")
    (many, sm), affm, gemmm = counted(lambda: run(rctx, y, nr, nc, hx, hy, nle.RESID_ROWS))
    # 1 MiB / (200 x 8 bytes) = 655 rows, cut down to 640 = 5 x 128: 30 chunks of the 19200 rows
    assert (aff1, gemm1) == (1, 1) and (affm, gemmm) == (30, 30)
    assert sm == s1 and np.array_equal(one.view(np.uint32), many.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["rows", "fused"])
def test_device_cholesky_factor_below_its_usual_order(nle, oracle, rctx, monkeypatch, form):
    """K_A's Cholesky factor comes from the device from 288 samples on, where the fused form no longer applies; the existing
    measurement switch NLE_DEV_SOLVER_MIN brings it down to p = 200, so that both routes take their F from the device's L^-1
    (FUSED: as the row-major L^-T, zero padded to 13 column tiles; ROWS: transposed)"""
    H, W, nr, nc, hx, hy, p = CASES["panels"]
    y, want, lam, _ = ref(oracle, "panels")
    fid = {"rows": nle.RESID_ROWS, "fused": nle.RESID_FUSED}[form]
    t = pick_threshold(want, bars(want, p, lam, stored=False))
    host, sh = run(rctx, y, nr, nc, hx, hy, fid, thresh=t)
    monkeypatch.setenv("NLE_DEV_SOLVER_MIN", "32")
    got, s = run(rctx, y, nr, nc, hx, hy, fid, thresh=t)
    print("bits equal to the host factor's:", np.array_equal(host.view(np.uint32), got.view(np.uint32)), sh["sum"], s["sum"])
    check_map(f"panels {form}, device factor", got, want, p, lam)
    check_summary(f"panels {form}, device factor", s, want, p, lam, t)


@pytest.mark.gpu
def test_refusals_leave_the_ctx_usable(nle, oracle, rctx):
    import torch
    H, W, nr, nc, hx, hy, p = CASES["ragged"]
    y, want, lam, _ = ref(oracle, "ragged")
    lum = torch.as_tensor(np.asarray(y, dtype=np.float32), device="cuda:0").contiguous()
    out = torch.zeros(H * W, dtype=torch.float32, device="cuda:0")
    s = np.zeros(4)
    torch.cuda.synchronize()

    def call(ctx, d_lum=lum, h=H, w=W, r=nr, c=nc, x=hx, yy=hy, form=0, thresh=0.5, summary=s):
        return nle.lib().nle_nystrom_residual(ctx._h, C.c_void_p(d_lum.data_ptr()) if d_lum is not None else None, h, w, r, c,
                                              float(x), float(yy), form, float(thresh), C.c_void_p(out.data_ptr()),
                                              summary.ctypes.data_as(C.c_void_p) if summary is not None else None)

    def refused(st, ctx=rctx):
        assert st == nle.NLE_ERR_INVALID
        print("refused:", nle.lib().nle_last_error(ctx._h).decode())

    refused(call(rctx, d_lum=None))
    refused(call(rctx, summary=None))
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused(call(rctx, thresh=bad))
    for form in (-1, 3, 99):
        refused(call(rctx, form=form))
    refused(call(rctx, r=H + 1))                       # the reference's check of the sample counts
    refused(call(rctx, x=0.0))
    big = torch.zeros((64, 64), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    refused(call(rctx, d_lum=big, h=64, w=64, r=46, c=46))            # 47 x 47 samples > 2048
    refused(call(rctx, d_lum=big, h=64, w=64, r=17, c=17, form=2))    # p = 289 > 256: the fused form does not apply
    rctx.set_patch_radius(1)
    refused(call(rctx, form=2))
    rctx.set_patch_radius(0)
    rctx.set_sampler(nle.SAMPLER_FARTHEST)
    refused(call(rctx, form=2))
    rctx.set_sampler(0)
    a = oracle.synthetic_luminance(H, W, seed=77)
    rctx.set_chroma(a, a, 20.0)
    refused(call(rctx, form=2))
    refused(call(rctx, d_lum=lum + 0.5, form=1))       # what nle_compute_kernel64 refuses: a non-integer plane with chroma
    rctx.set_chroma(None, None, 0.0)
    assert torch.count_nonzero(out).item() == 0       # nothing was written
    # world > 1: refused before any collective
    calls = []
    c2 = nle.Context(0)
    try:
        c2.set_shard(0, 2, p, lambda t: calls.append(int(t.numel())))
        refused(call(c2), c2)
        assert calls == []
    finally:
        c2.close()
    # still usable: nle_compute_kernel64 matches the oracle, and the residual its restatement
    st, Ka, kab, pp = tpa._kernel64(nle, rctx, y, nr, nc, hx, hy)
    assert st == 0 and pp == p
    perm, Ka_o, Kab_o = oracle.compute_kernel(y, nr, nc, hx, hy)
    K_o = np.empty((H * W, p))
    K_o[perm[:p]] = Ka_o
    K_o[perm[p:]] = Kab_o.T
    np.testing.assert_allclose(Ka, Ka_o, rtol=1e-14, atol=0)
    np.testing.assert_allclose(kab[:, :p], K_o, rtol=1e-14, atol=0)
    got, _ = run(rctx, y, nr, nc, hx, hy, nle.RESID_AUTO)
    check_map("after the refusals", got, want, p, lam)


@pytest.mark.gpu
def test_profile_ids_of_the_two_routes(nle, oracle, rctx):
    H, W, nr, nc, hx, hy, p = CASES["sq_hx16"]
    y = ref(oracle, "sq_hx16")[0]
    names = [nle.lib().nle_kernel_name(k).decode() for k in range(nle.KERNEL_COUNT)]
    for form, want in ((nle.RESID_FUSED, {1: 1, 8: 1}), (nle.RESID_ROWS, {0: 1, 1: 1, 8: 2})):
        rctx.profile(2)
        run(rctx, y, nr, nc, hx, hy, form)
        st = rctx.kernel_stats()
        rctx.profile(False)
        counts = {k: int(st[names[k]][0]) for k in range(nle.KERNEL_COUNT)}
        print(form, counts)
        assert counts[1] == want[1] and counts[0] == want.get(0, 0)        # NLE_K_NYSTROM, NLE_K_AFFINITY
        assert counts[8] >= want[8]                                        # NLE_K_SMALL: the reductions (and the sample fetch)
        assert all(counts[k] == 0 for k in (2, 3, 4, 5, 6, 7, 9, 10, 11))


# ------------------------------------------------------------------------------------------------------ C++ surface and CLI

CPP_DRIVER = textwrap.dedent(r"""
    #include <cmath>
    #include <cstdio>
    #include <cstring>
    #include <string>
    #include <vector>
    #include "nle.h"
    #include "nle/filter.hpp"
    #define REQUIRE(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); return 1; } } while (0)
    template <typename Fn> static bool throws(Fn&& fn) {
        try { fn(); } catch (const std::runtime_error& e) { std::printf("threw: %s\n", e.what()); return true; }
        return false;
    }
    // the map and the summary of the C++ call against the C ABI's on the same device plane: fp32 values and all four entries exactly
    static bool same(const nle::NLEFilter::Residual& res, int H, int W, const std::vector<float>& h, const double* s) {
        if (res.map.rows != H || res.map.cols != W || res.map.depth() != nle::NLE_64F || res.map.channels() != 1) return false;
        for (size_t i = 0; i < h.size(); ++i)
            if (res.map.ptr<double>()[i] != (double)h[i]) return false;
        return res.sum == s[0] && res.max == s[1] && res.argmax == (long long)s[2] && res.count == (long long)s[3];
    }
    int main() {
        const int H = 37, W = 53, nr = 5, nc = 6;
        const double hx = 9.0, hy = 25.0;
        const size_t n = (size_t)H * W;
        nle::Image L(H, W, nle::NLE_64F, 1), bgr(H, W, nle::NLE_8U, 3);
        std::vector<float> lum(n);
        for (int r = 0; r < H; ++r)
            for (int c = 0; c < W; ++c) {
                const double v = std::floor(128 + 60 * std::sin(0.2 * r) * std::cos(0.15 * c) + 20 * ((r * 7 + c * 13) % 5) / 5.0);
                L.at<double>(r, c) = v;
                lum[(size_t)r * W + c] = (float)v;
                unsigned char* px = bgr.ptr<unsigned char>(r) + 3 * c;
                px[0] = (unsigned char)((r * 5 + c * 3) % 256), px[1] = (unsigned char)v, px[2] = (unsigned char)((r * c) % 251);
            }
        // the yardstick: nle_nystrom_residual on a ctx of the driver's own
        nle_ctx* c = nullptr;
        REQUIRE(nle_ctx_create(0, nullptr, &c) == NLE_OK);
        void *d_lum = nullptr, *d_r = nullptr, *d_bgr = nullptr;
        REQUIRE(nle_dev_alloc(c, n * 4, &d_lum) == NLE_OK && nle_dev_alloc(c, n * 4, &d_r) == NLE_OK && nle_dev_alloc(c, n * 3, &d_bgr) == NLE_OK);
        REQUIRE(nle_dev_upload(c, d_lum, lum.data(), n * 4) == NLE_OK);
        std::vector<float> h(n);
        double s[4];
        long long counts[2];
        const double thr[2] = {0.3, 0.9};
        for (int form : {NLE_RESID_ROWS, NLE_RESID_FUSED, NLE_RESID_AUTO})
            for (int t = 0; t < 2; ++t) {
                REQUIRE(nle_nystrom_residual(c, (const float*)d_lum, H, W, nr, nc, hx, hy, form, thr[t], (float*)d_r, s) == NLE_OK);
                REQUIRE(nle_dev_download(c, h.data(), d_r, n * 4) == NLE_OK);
                nle::NLEFilter f;
                const nle::NLEFilter::Residual res = f.nystromResidual(L, nr, nc, hx, hy, form, thr[t]);
                REQUIRE(same(res, H, W, h, s));
                REQUIRE(res.argmax >= 0 && res.argmax < (long long)n && (double)h[(size_t)res.argmax] == (double)(float)res.max);
                counts[t] = res.count;
            }
        REQUIRE(counts[0] > counts[1] && counts[1] >= 0);  // thresh reaches the call
        {   // the defaults: AUTO and thresh 0.5
            REQUIRE(nle_nystrom_residual(c, (const float*)d_lum, H, W, nr, nc, hx, hy, NLE_RESID_AUTO, 0.5, (float*)d_r, s) == NLE_OK);
            REQUIRE(nle_dev_download(c, h.data(), d_r, n * 4) == NLE_OK);
            REQUIRE(same(nle::NLEFilter().nystromResidual(L, nr, nc, hx, hy), H, W, h, s));
        }
        {   // the 8-bit image form: its L channel (nle_bgr2lab8); under patchRadius and the farthest sampler too
            REQUIRE(nle_dev_upload(c, d_bgr, bgr.ptr<unsigned char>(), n * 3) == NLE_OK);
            REQUIRE(nle_bgr2lab8(c, (const unsigned char*)d_bgr, (long long)n, nullptr, (float*)d_lum) == NLE_OK);
            REQUIRE(nle_ctx_set_patch_radius(c, 1) == NLE_OK && nle_ctx_set_sampler(c, NLE_SAMPLER_FARTHEST) == NLE_OK);
            REQUIRE(nle_nystrom_residual(c, (const float*)d_lum, H, W, nr, nc, hx, hy, NLE_RESID_ROWS, 0.3, (float*)d_r, s) == NLE_OK);
            REQUIRE(nle_dev_download(c, h.data(), d_r, n * 4) == NLE_OK);
            nle::NLEFilter f;
            f.patchRadius = 1, f.sampler = NLE_SAMPLER_FARTHEST;
            REQUIRE(same(f.nystromResidual(bgr, nr, nc, hx, hy, NLE_RESID_ROWS, 0.3), H, W, h, s));
            REQUIRE(nle_ctx_set_patch_radius(c, 0) == NLE_OK && nle_ctx_set_sampler(c, NLE_SAMPLER_GRID) == NLE_OK);
        }
        // refusals throw, and the shared ctx is back at radius 0, the grid and no chroma afterwards: the free function
        // computeKernel runs on it with whatever options it finds, and a plain train gives the same filter
        const nle::Mat Ka0 = std::get<1>(nle::computeKernel(L, nr, nc, hx, hy));
        nle::NLEFilter t0;
        t0.verbose = false;
        t0.trainFilter(L, nr, nc, hx, hy, 10, 8);
        const nle::Vec e0 = t0.eigvals();
        auto unchanged = [&] {
            const nle::Mat Ka = std::get<1>(nle::computeKernel(L, nr, nc, hx, hy));
            nle::NLEFilter t1;
            t1.verbose = false;
            t1.trainFilter(L, nr, nc, hx, hy, 10, 8);
            const nle::Vec e1 = t1.eigvals();
            return Ka.rows() == Ka0.rows() && std::memcmp(Ka.data(), Ka0.data(), sizeof(double) * Ka.rows() * Ka.cols()) == 0 &&
                   e1.size() == e0.size() && std::memcmp(e1.data(), e0.data(), sizeof(double) * e0.size()) == 0;
        };
        nle::NLEFilter f;
        f.exact = true;
        REQUIRE(throws([&] { f.nystromResidual(L, nr, nc, hx, hy); }));                        // no extension in the exact filter
        f.exact = false;
        REQUIRE(throws([&] { f.nystromResidual(nle::Image(H, W, nle::NLE_8U, 1), nr, nc, hx, hy); }));   // neither form
        REQUIRE(throws([&] { f.nystromResidual(L, H + 1, nc, hx, hy); }));                     // the reference's sample-count check
        REQUIRE(throws([&] { f.nystromResidual(L, nr, nc, hx, hy, 7); }));                     // unknown form
        REQUIRE(unchanged());
        f.patchRadius = 1, f.sampler = NLE_SAMPLER_FARTHEST;
        REQUIRE(throws([&] { f.nystromResidual(L, nr, nc, hx, hy, NLE_RESID_FUSED); }));       // refused by the call, options set
        REQUIRE(unchanged());
        f.chromaBandwidth = -1.0;
        REQUIRE(throws([&] { f.nystromResidual(bgr, nr, nc, hx, hy); }));                      // refused by nle_ctx_set_chroma
        REQUIRE(unchanged());
        f.chromaBandwidth = 20.0;
        (void)f.nystromResidual(bgr, nr, nc, hx, hy);                                          // a call that succeeds under all three
        REQUIRE(unchanged());
        nle_dev_free(c, d_lum), nle_dev_free(c, d_r), nle_dev_free(c, d_bgr);
        nle_ctx_destroy(c);
        std::printf("nystromResidual OK\n");
        return 0;
    }
""")


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_cpp_nystrom_residual_matches_the_c_abi(tmp_path):
    """NLEFilter::nystromResidual through a compiled driver: the CV_64F plane form with ROWS, FUSED, AUTO and two thresholds,
    the defaults, and the 8-bit image form under a patch radius and the farthest sampler -- map (fp32 values) and the four
    summary entries exactly what nle_nystrom_residual returns for the same plane; every throw; the shared ctx's options and a
    later plain train unchanged after refused and successful calls"""
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
    assert r.returncode == 0 and "nystromResidual OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-1000:])


@pytest.mark.gpu
@pytest.mark.parametrize("lead,R,sampler,hc", [([], 0, 0, None),
                                               (["--sampler", "farthest", "--chroma", "20", "--patch-radius", "1"], 1, 1, 20.0)],
                         ids=["plain", "options"])
def test_enhance_report_matches_the_python_mirror(nle, oracle, rctx, tmp_path, lead, R, sampler, hc):
    """`enhance --nystrom-report --nystrom-map` runs NLEFilter::nystromResidual (the C++ surface) on the image: the map's
    bytes and the line's figures against the Python mirror, and the enhanced image and the other stdout lines unchanged"""
    from PIL import Image
    src_path = os.path.join(GOLDEN, "flower-50.bmp")
    out, out0, mp = tmp_path / "o.png", tmp_path / "o0.png", tmp_path / "map.png"
    # the options in any order with the existing ones
    argv = [ENHANCE, "--nystrom-map", str(mp)] + lead + ["--nystrom-report", src_path, str(out)] + FLOWER_ARGS
    r = subprocess.run(argv, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    r0 = subprocess.run([ENHANCE] + lead + [src_path, str(out0)] + FLOWER_ARGS, capture_output=True, text=True, timeout=600)
    assert r0.returncode == 0, r0.stderr
    assert open(out, "rb").read() == open(out0, "rb").read()       # the enhanced image: the same bytes
    lines = r.stdout.splitlines()
    assert lines[:-1] == r0.stdout.splitlines() and lines[-1].startswith("Nystrom residual: mean ")
    # the mirror: bgr2lab8 -> L (and a, b) -> nystrom_residual under the same options
    src = tpa._load_bgr("flower-50.bmp")
    H, W = src.shape[:2]
    lab, L = rctx.bgr2lab8(src)
    rctx.set_patch_radius(R)
    rctx.set_sampler(sampler)
    if hc is not None:
        rctx.set_chroma(rctx.lab8_channel(lab, 1), rctx.lab8_channel(lab, 2), hc)
    m, s = rctx.nystrom_residual(L.reshape(H, W), FLOWER["nr"], FLOWER["nc"], FLOWER["hx"], FLOWER["hy"])
    m = m.cpu().numpy().astype(np.float64)
    want8 = np.floor(255.0 * np.clip(m, 0.0, 1.0) + 0.5).astype(np.uint8)
    got = np.asarray(Image.open(str(mp)).convert("RGB"))
    assert got.shape == (H, W, 3) and all(np.array_equal(got[..., k], want8) for k in range(3))
    words = lines[-1].replace("(", " ").replace(")", " ").replace(",", " ").split()
    mean, mx, row, col, share = float(words[3]), float(words[5]), int(words[7]), int(words[8]), float(words[-1])
    assert (row, col) == divmod(s["argmax"], W)
    assert abs(mean - s["sum"] / (H * W)) <= 1e-5 * mean and abs(mx - s["max"]) <= 1e-5 * mx
    assert abs(share - s["count"] / (H * W)) <= 1e-5
