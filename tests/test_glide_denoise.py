"""The MSE-guided denoiser (include/nle.h "MSE-guided denoise"): the non-local-means pre-filter
nle_nlm8, Immerkaer's noise estimate nle_plane_noise, the coefficients t = V^T x of nle_filter_coefficients, the host-only
search nle_mse_shrink, and their wiring through NLEFilter::trainForDenoise / denoise and the `denoise` CLI
(--prefilter, --glide, --noise-sigma, --nlm-h).  The numpy restatements live here; the oracle supplies train and apply."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

BIN = os.path.join(ROOT, "nonlocal-image-edit_amd", "bin")
DENOISE = os.path.join(BIN, "denoise")
ENHANCE = os.path.join(BIN, "enhance")
U24 = 2.0 ** -24          # unit roundoff of fp32


@pytest.fixture(scope="module", autouse=True)
def built():
    if not (os.path.exists(DENOISE) and os.path.exists(ENHANCE)):
        import __graft_entry__ as entry
        entry.build()
    assert os.path.exists(DENOISE) and os.path.exists(ENHANCE)


# ------------------------------------------------------------------------------------------------ numpy restatements
def reflect101(idx, n):
    if n == 1:
        return np.zeros_like(idx)
    period = 2 * n - 2
    i = np.mod(idx, period)
    return np.where(i < n, i, period - i)


def np_mse_shrink(eigvals, b, sigma, k_max, n_grid):
    """nle_mse_shrink as the header states it: (k, mse[n_grid + 1]), every sum in index order"""
    mu = np.minimum(np.maximum(np.asarray(eigvals, dtype=np.float64), 0.0), 1.0)
    b = np.asarray(b, dtype=np.float64)
    mse = np.zeros(n_grid + 1)
    for i in range(n_grid + 1):
        k = k_max * i / n_grid
        s = 0.0
        for j in range(mu.size):
            a = math.pow(mu[j], k)                       # pow(0, 0) = 1
            s += (1.0 - a) ** 2 * b[j] ** 2 + sigma * sigma * math.pow(mu[j], 2.0 * k)
        mse[i] = s
    i = int(np.argmin(mse))                              # the smallest index attaining the minimum
    return k_max * i / n_grid, mse


def np_noise(x):
    """nle_plane_noise: (S, sigma) in int64 / fp64"""
    x = np.asarray(x, dtype=np.int64)
    H, W = x.shape
    c = (x[:-2, :-2] + x[:-2, 2:] + x[2:, :-2] + x[2:, 2:]) - 2 * (x[:-2, 1:-1] + x[1:-1, :-2] + x[1:-1, 2:] + x[2:, 1:-1]) \
        + 4 * x[1:-1, 1:-1]
    S = int(np.abs(c).sum())
    return S, math.sqrt(math.pi / 2.0) * float(S) / (6.0 * float(H - 2) * float(W - 2))


# The elementwise bound of nle_nlm8's `raw`, by counting the roundings of k_nlm8 (csrc/denoise.hip), u = 2^-24:
#   SSD is an exact integer in fp32.  d = max(SSD - Tf, 0): one rounding.  x = d cf: one rounding.  The exponential is the
#   hardware's exp2: t = -x log2e (one rounding; the fp32 constant is off by 0.22 u) and v_exp_f32, accurate to 1 ulp = 2 u
#   relative.  The argument x thus carries at most 4 u of relative error, which the exponential turns into 4 u x e^-x (<= 0.37
#   * 4 u) of absolute error, and the result 2 u w more:            dw_q <= u w_q (4 x_q + 2)      (+ 2^-120 where the
#   hardware flushes a denormal result).  w(p, p) = 1 is exact.
#   The two sums run over the 2S + 1 window rows, each a sum of 2S + 1 terms started from 0, then over the rows: 2S + 2S
#   additions deep, so each carries at most 4S u of relative error on its (non-negative) terms; the numerator one more u per
#   term for w u(q) (a fused multiply-add has fewer).  The division rounds once.
#     |raw - ref| <= [ sum dw_q v_q + (4S + 1) u sum w v  +  ref (sum dw_q + 4S u sum w) ] / sum w  +  u ref
#   first order in u; 1 % is added for the higher orders (441 u^2 and the like).  Evaluated per pixel from the reference's own
#   weights: about 1e-4 levels where many weights are large, up to ~1e-3 where the weight sum is close to 1.
@functools.lru_cache(maxsize=None)
def nlm_reference(shape, P, S, sigma, h, seed):
    """(plane int64, ref fp64 H x W, bound fp64 H x W) of nle_nlm8 on the seeded test plane"""
    plane = nlm_plane(shape, seed)
    return (plane,) + np_nlm(plane, P, S, sigma, h)


def np_nlm(plane, P, S, sigma, h):
    u = np.asarray(plane, dtype=np.int64)
    H, W = u.shape
    n = (2 * P + 1) ** 2
    Tf = float(np.float32(2.0 * sigma * sigma * n))
    cf = float(np.float32(1.0 / (n * h * h)))
    R = P + S
    pad = u[np.ix_(reflect101(np.arange(-R, H + R), H), reflect101(np.arange(-R, W + R), W))]
    A = pad[S:S + H + 2 * P, S:S + W + 2 * P]
    den = np.zeros((H, W))
    num = np.zeros((H, W))
    dw_sum = np.zeros((H, W))
    dwv_sum = np.zeros((H, W))
    for dy in range(-S, S + 1):
        for dx in range(-S, S + 1):
            B = pad[S + dy:S + dy + H + 2 * P, S + dx:S + dx + W + 2 * P]
            D = (A - B) ** 2
            c = np.zeros((D.shape[0] + 1, D.shape[1] + 1), dtype=np.int64)
            c[1:, 1:] = D.cumsum(0).cumsum(1)
            d = 2 * P + 1
            ssd = c[d:, d:] - c[:-d, d:] - c[d:, :-d] + c[:-d, :-d]          # exact integers, H x W
            x = np.maximum(ssd.astype(np.float64) - Tf, 0.0) * cf
            w = np.exp(-x)
            v = B[P:P + H, P:P + W].astype(np.float64)
            dw = 1.01 * U24 * w * (4.0 * x + 2.0) + 2.0 ** -120
            if dy == 0 and dx == 0:
                assert np.all(w == 1.0)
                dw = 0.0 * w
            den += w
            num += w * v
            dw_sum += dw
            dwv_sum += dw * v
    ref = num / den
    a = dwv_sum + 1.01 * (4 * S + 1) * U24 * num
    b = dw_sum + 1.01 * 4 * S * U24 * den
    bound = 1.01 * ((a + ref * b) / den + U24 * ref)
    return ref, bound


def nlm_plane(shape, seed):
    """an integer step edge plus a ramp plus seeded integer noise"""
    H, W = shape
    rng = np.random.default_rng(seed)
    rr, cc = np.mgrid[0:H, 0:W]
    x = 60 + 90 * (cc > 0.45 * W + 0.2 * rr) + (rr + 2 * cc) // 3 + rng.integers(-6, 7, shape)
    return np.clip(x, 0, 255).astype(np.int64)


def near_half(ref, bound):
    return np.abs(ref - (np.floor(ref) + 0.5)) <= bound


# shape, P, S, sigma, h, seed
NLM_CASES = [((7, 5), 1, 10, 4.0, 3.0, 1),       # the window is larger than the image: the reflection wraps more than once
             ((33, 47), 3, 10, 5.0, 4.0, 2),
             ((40, 65), 1, 1, 3.0, 2.0, 3),      # one column past a tile
             ((64, 96), 2, 5, 5.0, 3.0, 4)]
NLM_IDS = ["7x5-S10", "33x47-P3-S10", "40x65-P1-S1", "64x96-P2-S5"]


def colour_scene(H, W, seed, sigma=12.0):
    """(clean, noisy) uint8 BGR: piecewise constant, three colours, seeded Gaussian noise added in BGR and clipped"""
    rng = np.random.default_rng(seed)
    rr, cc = np.mgrid[0:H, 0:W]
    region = np.where(cc < 0.4 * W + 0.15 * rr, 0, np.where(rr < 0.55 * H, 1, 2))
    colours = np.array([[40, 40, 160], [200, 180, 60], [150, 230, 240]], dtype=np.float64)   # three distinct lightnesses
    clean = colours[region]
    noisy = np.clip(np.rint(clean + rng.normal(0.0, sigma, clean.shape)), 0, 255)
    return clean.astype(np.uint8), noisy.astype(np.uint8)


def psnr(a, b):
    return 10.0 * math.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def nlm_params(sigma, nlm_h=0.0):
    """DenoiseOptions' table (Buades, Coll & Morel, IPOL 2011, grey images, cut to the kernel's limits): P, S, h"""
    P = 1 if sigma <= 15 else 2 if sigma <= 30 else 3
    return P, 10, (nlm_h if nlm_h > 0 else (0.40 if sigma <= 30 else 0.35) * sigma)


QUALITY = dict(shape=(64, 96), seed=7, nr=8, nc=12, hx=12.0, hy=15.0, T=10, K=20, k_max=6.0)


# ------------------------------------------------------------------------------------------------ CPU
def spectrum(K, seed):
    rng = np.random.default_rng(seed)
    ev = np.sort(rng.uniform(0.02, 0.999, K))[::-1]
    special = [1.0, 0.0, 1.3, -0.2]            # exact 1 and 0, above 1 and below 0 (clamped)
    for i, v in enumerate(special[:K]):
        ev[(i * 7) % K] = v
    return ev, rng.normal(0.0, 40.0, K)


@pytest.mark.parametrize("K,sigma,k_max,n_grid", [(1, 7.0, 6.0, 64), (8, 7.0, 6.0, 256), (50, 12.5, 9.0, 256), (8, 0.0, 6.0, 256),
                                                  (8, 7.0, 0.0, 16), (50, 3.0, 2.5, 1000)])
def test_mse_shrink_matches_the_numpy_restatement(nle, K, sigma, k_max, n_grid):
    ev, b = spectrum(K, 100 + K)
    if K == 1:
        ev[0] = 0.7
    want_k, want = np_mse_shrink(ev, b, sigma, k_max, n_grid)
    distinct = np.unique(want)
    if distinct.size > 1:                      # the precondition: best and second-best grid values are well apart
        assert (distinct[1] - distinct[0]) > 1e-9 * distinct[0]
    got_k, got = nle.mse_shrink(ev, b, sigma, k_max, n_grid)
    assert got.shape == want.shape
    assert np.allclose(got, want, rtol=1e-12, atol=0.0)
    assert got_k == want_k
    if sigma == 0.0:
        assert got_k == 0.0                    # nothing to remove: the span stays untouched
    if k_max == 0.0:
        assert got_k == 0.0 and np.all(got == got[0])


def test_mse_shrink_prefers_more_shrinkage_under_more_noise(nle):
    ev, b = spectrum(8, 5)
    ks = [nle.mse_shrink(ev, b, s, 8.0, 256)[0] for s in (0.0, 5.0, 20.0, 80.0)]
    assert ks == sorted(ks) and ks[0] == 0.0 and ks[-1] > 0.0


@pytest.mark.parametrize("case", ["K0", "grid0", "grid_big", "sigma_neg", "sigma_nan", "sigma_inf", "kmax_neg", "kmax_nan",
                                  "null_eigvals", "null_b", "null_k"])
def test_mse_shrink_refusals(nle, case):
    import ctypes as C
    ev, b = np.array([0.9, 0.5]), np.array([3.0, 1.0])
    k = C.c_double(-1.0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    args = dict(ev=ptr(ev), b=ptr(b), K=2, sigma=1.0, k_max=4.0, n_grid=8, k=C.byref(k))
    args.update({"K0": dict(K=0), "grid0": dict(n_grid=0), "grid_big": dict(n_grid=65537), "sigma_neg": dict(sigma=-1.0),
                 "sigma_nan": dict(sigma=float("nan")), "sigma_inf": dict(sigma=float("inf")), "kmax_neg": dict(k_max=-0.5),
                 "kmax_nan": dict(k_max=float("nan")), "null_eigvals": dict(ev=None), "null_b": dict(b=None),
                 "null_k": dict(k=None)}[case])
    st = nle.lib().nle_mse_shrink(args["ev"], args["b"], args["K"], args["sigma"], args["k_max"], args["n_grid"], args["k"], None)
    assert st == nle.NLE_ERR_INVALID and k.value == -1.0
    assert nle.lib().nle_mse_shrink(ptr(ev), ptr(b), 2, 1.0, 4.0, 65536, C.byref(k), None) == nle.NLE_OK   # the limit itself


TAIL = ["in.bmp", "out.bmp", "6", "8", "12", "30", "5", "8", "10", "3", "4"]   # a denoise command line (never read: exit 2 first)


@pytest.mark.parametrize("tool,opts,word", [
    (ENHANCE, ["--glide"], "not supported here"),
    (ENHANCE, ["--prefilter", "nlm"], "not supported here"),
    (ENHANCE, ["--noise-sigma", "3"], "not supported here"),
    (ENHANCE, ["--nlm-h", "2"], "not supported here"),
    (DENOISE, ["--prefilter", "foo"], "--prefilter"),
    (DENOISE, ["--glide", "--noise-sigma", "-1"], "--noise-sigma"),
    (DENOISE, ["--noise-sigma", "3"], "--noise-sigma needs"),
    (DENOISE, ["--prefilter", "nlm", "--nlm-h", "0"], "--nlm-h"),
    (DENOISE, ["--nlm-h", "2"], "--nlm-h needs"),
    (DENOISE, ["--prefilter", "bilateral", "--nlm-h", "2"], "--nlm-h needs"),
    (DENOISE, ["--glide=1"], "takes no value"),
    (DENOISE, ["--glide", "--noise-sigma", "nan"], "--noise-sigma"),
], ids=["enhance-glide", "enhance-prefilter", "enhance-noise-sigma", "enhance-nlm-h", "prefilter-foo", "noise-sigma-negative",
        "noise-sigma-unused", "nlm-h-zero", "nlm-h-without-nlm", "nlm-h-with-bilateral", "glide-with-value", "noise-sigma-nan"])
def test_cli_refuses_bad_options_before_the_gpu(tool, opts, word):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")   # no device could be opened anyway
    r = subprocess.run([tool] + opts + TAIL + (["1"] if tool == ENHANCE else []), capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 2 and word in r.stderr and r.stdout == "", (r.returncode, r.stderr)


def test_cli_takes_the_options_in_any_order():
    """the four options parse beside --patch-radius, --sampler and --exact: the command line gets as far as the image (which
    does not exist: the reference's soft failure, exit 0)"""
    for opts in (["--glide", "--patch-radius", "1", "--prefilter", "nlm", "--sampler", "farthest", "--noise-sigma", "5", "--nlm-h", "2"],
                 ["--nlm-h", "2", "--exact", "--noise-sigma", "0", "--prefilter", "nlm", "--glide"],
                 ["--prefilter", "bilateral"], ["--noise-sigma", "5", "--glide"]):
        r = subprocess.run([DENOISE] + opts + ["/nonexistent/in.bmp"] + TAIL[1:], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "Failed to read file from" in r.stderr, (opts, r.stderr)


@pytest.mark.parametrize("case", NLM_CASES, ids=NLM_IDS)
def test_nlm_reference_rounds_unambiguously_almost_everywhere(case):
    """the precondition of the device test, on the numpy reference alone: at most 1 % of the plane lies within the bound of a
    half-integer"""
    shape, P, S, sigma, h, seed = case
    plane, ref, bound = nlm_reference(shape, P, S, sigma, h, seed)
    assert ref.min() >= plane.min() and ref.max() <= plane.max()         # a convex combination
    assert bound.max() < 5e-3
    assert near_half(ref, bound).mean() <= 0.01
    assert np.abs(np.diff(ref, axis=1)).mean() < np.abs(np.diff(plane, axis=1)).mean()   # it smooths


def numpy_glide(oracle, noisy, q, prefilter_nlm=True):
    """trainForDenoise + denoise with glide, composed from the oracle's train and apply and the restatements above"""
    lab = oracle.bgr_to_lab8(noisy)
    planes = [lab[..., ch].astype(np.int64) for ch in range(3)]

    def pre(x):
        s = np_noise(x)[1]
        P, S, h = nlm_params(s)
        return s, np.rint(np_nlm(x, P, S, s, h)[0])
    V, ev = oracle.train_filter(pre(planes[0])[1].astype(np.float64), q["nr"], q["nc"], q["hx"], q["hy"], q["T"], q["K"])
    out = lab.copy()
    ks = []
    for ch in range(3):
        s, p = pre(planes[ch])
        b = V.T @ p.ravel()
        k, _ = np_mse_shrink(ev, b, s, q["k_max"], 256)
        resp = np.minimum(np.maximum(ev, 0.0), 1.0) ** k
        y = oracle.apply_filter(V, planes[ch].astype(np.float64), resp)
        out[..., ch] = np.rint(np.clip(y, 0, 255)).astype(np.uint8)
        ks.append(k)
    return oracle.lab8_to_bgr(out), ks


def test_quality_floor_holds_for_the_oracle_composition(oracle):
    """before the GPU run: at this size and seed the method denoises when composed from the oracle's train and apply"""
    clean, noisy = colour_scene(*QUALITY["shape"], QUALITY["seed"])
    out, ks = numpy_glide(oracle, noisy, QUALITY)
    print("oracle composition: PSNR noisy %.3f -> %.3f, k = %s" % (psnr(noisy, clean), psnr(out, clean), ks))
    assert psnr(out, clean) > psnr(noisy, clean)


# ------------------------------------------------------------------------------------------------ GPU: nle_nlm8
@pytest.mark.gpu
@pytest.mark.parametrize("case", NLM_CASES, ids=NLM_IDS)
def test_nlm8_against_the_numpy_restatement(nle, ctx, case):
    shape, P, S, sigma, h, seed = case
    plane, ref, bound = nlm_reference(shape, P, S, sigma, h, seed)
    tie = near_half(ref, bound)
    assert tie.mean() <= 0.01
    dst, raw = ctx.nlm8(plane.astype(np.float32), P, S, sigma, h, want_raw=True)
    dst, raw = dst.cpu().numpy(), raw.cpu().numpy()
    err = np.abs(raw.astype(np.float64) - ref)
    print("nlm8 %s: max |raw - ref| %.3e, max bound %.3e, worst ratio %.3f, ties %d" %
          (shape, err.max(), bound.max(), (err / bound).max(), int(tie.sum())))
    assert np.all(err <= bound)
    assert np.array_equal(dst, np.rint(raw))                              # on the device's own raw
    assert np.array_equal(dst[~tie], np.rint(ref)[~tie].astype(np.float32))
    assert np.array_equal(ctx.nlm8(plane.astype(np.float32), P, S, sigma, h).cpu().numpy(), dst)   # without d_raw, the same


@pytest.mark.gpu
@pytest.mark.parametrize("P,S", [(1, 1), (2, 10), (3, 10)])
def test_nlm8_fixed_points(nle, ctx, P, S):
    flat = np.full((37, 70), 200, dtype=np.float32)
    dst, raw = ctx.nlm8(flat, P, S, 3.0, 2.0, want_raw=True)
    assert np.array_equal(dst.cpu().numpy(), flat) and np.array_equal(raw.cpu().numpy(), flat)
    # h so small that every weight but those of identical patches underflows (identical patches share their centre value)
    plane = nlm_plane((37, 70), 9).astype(np.float32)
    dst, raw = ctx.nlm8(plane, P, S, 0.0, 1e-3, want_raw=True)
    assert np.array_equal(dst.cpu().numpy(), plane) and np.array_equal(raw.cpu().numpy(), plane)


@pytest.mark.gpu
def test_nlm8_refusals_leave_the_ctx_usable(nle, ctx):
    import ctypes as C
    import torch
    x = torch.as_tensor(nlm_plane((20, 30), 1).astype(np.float32), device="cuda:0")
    y, z = torch.empty_like(x), torch.empty_like(x)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    good = dict(src=x, H=20, W=30, P=1, S=2, sigma=2.0, h=2.0, dst=y, raw=z)
    bad = [dict(P=0), dict(P=4), dict(S=0), dict(S=11), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")),
           dict(h=0.0), dict(h=-1.0), dict(h=float("inf")), dict(h=float("nan")), dict(src=None), dict(dst=None), dict(dst=x),
           dict(raw=x), dict(raw=y), dict(H=0), dict(W=0), dict(h=1e-30), dict(sigma=1e25)]
    torch.cuda.synchronize()
    for change in bad:
        a = dict(good, **change)
        st = nle.lib().nle_nlm8(ctx._h, p(a["src"]), a["H"], a["W"], a["P"], a["S"], a["sigma"], a["h"], p(a["dst"]), p(a["raw"]))
        assert st == nle.NLE_ERR_INVALID, change
        assert nle.lib().nle_last_error(ctx._h).decode().startswith("nle_nlm8") or "image" in nle.lib().nle_last_error(ctx._h).decode()
    for v in (17.5, 300.0, -1.0, float("nan")):
        q = x.clone()
        q[7, 11] = v
        with pytest.raises(nle.NLEError, match="integer valued"):
            ctx.nlm8(q, 1, 2, 2.0, 2.0)
    want = np.rint(np_nlm(x.cpu().numpy().astype(np.int64), 1, 2, 2.0, 2.0)[0])
    got = ctx.nlm8(x, 1, 2, 2.0, 2.0).cpu().numpy()
    assert np.mean(got != want) <= 0.01                                   # the ctx works afterwards


# ------------------------------------------------------------------------------------------------ GPU: nle_plane_noise
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 3), (5, 300), (67, 129), (128, 1027), (700, 900)])
def test_plane_noise_is_exact(nle, ctx, shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    x = rng.integers(0, 256, shape)
    S, sigma = ctx.plane_noise(x.astype(np.float32))
    want_S, want_sigma = np_noise(x)
    assert S == want_S and sigma == want_sigma                            # bit for bit
    assert ctx.plane_noise(x.astype(np.float32)) == (S, sigma)
    flat = np.full(shape, 131, dtype=np.float32)
    assert ctx.plane_noise(flat) == (0, 0.0)
    worst = np.zeros(shape, dtype=np.float32)
    worst[1::2, 1::2] = 255.0                                             # terms of 4 * 255 at the lit pixels
    assert ctx.plane_noise(worst) == np_noise(worst)


@pytest.mark.gpu
def test_plane_noise_estimates_gaussian_noise_and_refuses_what_it_cannot_take(nle, ctx):
    rng = np.random.default_rng(0)
    x = np.clip(np.rint(128 + rng.normal(0.0, 10.0, (256, 256))), 0, 255)
    assert abs(ctx.plane_noise(x.astype(np.float32))[1] - 10.0) < 0.5
    for shape in ((2, 40), (40, 2)):
        with pytest.raises(nle.NLEError, match="nle_plane_noise"):
            ctx.plane_noise(np.zeros(shape, dtype=np.float32))
    y = x.astype(np.float32)
    y[100, 100] = 0.5
    with pytest.raises(nle.NLEError, match="integer valued"):
        ctx.plane_noise(y)
    assert ctx.plane_noise(x.astype(np.float32))[0] == np_noise(x)[0]


# ------------------------------------------------------------------------------------------------ GPU: nle_filter_coefficients
COEFF = dict(H=48, W=64, nr=6, nc=8, hx=12.0, hy=30.0, T=5, K=8)


@pytest.fixture(scope="module")
def coeff_plane():
    rng = np.random.default_rng(21)
    rr, cc = np.mgrid[0:COEFF["H"], 0:COEFF["W"]]
    x = np.clip(np.rint(110 + 60 * np.sin(rr / 7.0) * np.cos(cc / 9.0)) + 40 * (cc > 30) + rng.integers(-8, 9, rr.shape), 0, 255)
    return x.astype(np.float32)            # integer levels: the default train takes the table path


@pytest.fixture(scope="module", params=["tables", "materialised_f64", "exact"])
def coeff_filter(request, nle, ctx, coeff_plane):
    mode = {"tables": nle.MODE_AUTO, "materialised_f64": nle.MODE_MATERIALISED_F64, "exact": nle.MODE_EXACT_F64}[request.param]
    ctx.set_mode(mode)
    try:
        f = nle.NLEFilter(ctx).train_filter(coeff_plane, COEFF["nr"], COEFF["nc"], COEFF["hx"], COEFF["hy"], COEFF["T"], COEFF["K"])
    finally:
        ctx.set_mode(nle.MODE_AUTO)
    want = {"tables": nle.MODE_PHI_FREE, "materialised_f64": nle.MODE_MATERIALISED_F64, "exact": nle.MODE_EXACT_F64}[request.param]
    assert f.diag()["formulation"] == want
    yield f
    f.close()


def coeff_inputs(plane):
    other = plane.copy()
    other[17, 23] = 255.0 - other[17, 23]
    rng = np.random.default_rng(4)
    return {"training": plane, "one_pixel": other, "non_integer": (plane + rng.uniform(-0.45, 0.45, plane.shape)).astype(np.float32)}


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["training", "one_pixel", "non_integer"])
def test_coefficients_are_the_t_of_apply(nle, ctx, coeff_filter, coeff_plane, which):
    """for every j: |t_j^2 - x^T y_j| <= 2^-23 sum_i |x_i| |y_i(j)| with y_j = nle_apply(x, e_j): sign-free, resting on the
    apply the oracle pins; the bound is the fp32 storage of y"""
    f = coeff_filter
    x = coeff_inputs(coeff_plane)[which]
    K = f.info()["K"]
    t = f.coefficients(x)
    assert t.shape == (1, K)
    x64 = x.astype(np.float64).ravel()
    for j in range(K):
        e = np.zeros(K)
        e[j] = 1.0
        y = f.apply(x, e).cpu().numpy().astype(np.float64)
        assert abs(t[0, j] ** 2 - x64 @ y) <= 2.0 ** -23 * (np.abs(x64) @ np.abs(y)), (which, j)
    assert np.array_equal(f.coefficients(x), t)                            # reproducible


@pytest.mark.gpu
def test_coefficients_of_three_planes_equal_three_calls(nle, ctx, coeff_filter, coeff_plane):
    ins = coeff_inputs(coeff_plane)
    planes = np.stack([ins["non_integer"], ins["training"], ins["one_pixel"]])
    t3 = coeff_filter.coefficients(planes)
    assert t3.shape == (3, coeff_filter.info()["K"])
    for m in range(3):
        assert np.array_equal(t3[m], coeff_filter.coefficients(planes[m])[0]), m      # bit for bit
    import torch
    wide = torch.zeros((3, COEFF["H"] + 5, COEFF["W"]), dtype=torch.float32, device="cuda:0")   # a stride larger than a plane
    wide[:, :COEFF["H"]] = torch.as_tensor(planes, device="cuda:0")
    assert np.array_equal(coeff_filter.coefficients(wide[:, :COEFF["H"]]), t3)


@pytest.mark.gpu
def test_coefficients_refusals(nle, ctx, coeff_filter, coeff_plane):
    import ctypes as C
    import torch
    f, H, W = coeff_filter, COEFF["H"], COEFF["W"]
    x = torch.as_tensor(np.stack([coeff_plane] * 17), device="cuda:0")
    out = np.zeros((17, f.info()["K"]))
    xp, op = C.c_void_p(x.data_ptr()), out.ctypes.data_as(C.c_void_p)
    torch.cuda.synchronize()
    call = nle.lib().nle_filter_coefficients
    for args in ((xp, 0, H * W, H, W, op), (xp, 17, H * W, H, W, op), (xp, 1, H * W, H + 1, W, op), (xp, 1, H * W, H, W - 1, op),
                 (None, 1, H * W, H, W, op), (xp, 1, H * W, H, W, None), (xp, 2, H * W - 1, H, W, op)):
        assert call(f._f, *args) == nle.NLE_ERR_INVALID, args[1:5]
        assert nle.lib().nle_last_error(ctx._h)
    assert call(f._f, xp, 16, H * W, H, W, op) == nle.NLE_OK
    assert np.array_equal(out[15], f.coefficients(coeff_plane)[0])


# ------------------------------------------------------------------------------------------------ GPU: wiring
WIRE = dict(nr=6, nc=8, hx=12.0, hy=30.0, T=5, K=8, sc=10, ss=3, k=4.0)


def write_bmp(path, bgr):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(path)


def read_bgr(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))[..., ::-1]


def run_denoise(tmp_path, noisy, opts, q, name):
    src, out = tmp_path / "in.bmp", tmp_path / (name + ".bmp")
    if not src.exists():
        write_bmp(str(src), noisy)
    args = [str(q[k]) for k in ("nr", "nc", "hx", "hy", "T", "K", "sc", "ss", "k")]
    r = subprocess.run([DENOISE] + opts + [str(src), str(out)] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return read_bgr(str(out)), r.stdout.splitlines()


def mirror_denoise(nle, ctx, noisy, q, glide, nlm):
    """the same steps through the Python mirror: (bgr, [(sigma, k)] * 3 or None)"""
    import torch
    H, W = noisy.shape[:2]
    lab, L = ctx.bgr2lab8(noisy)

    def pre(x):
        if not nlm:
            return None, ctx.bilateral8(x, q["sc"], q["ss"])
        s = ctx.plane_noise(x)[1]
        P, S, h = nlm_params(s)
        return s, (x.clone() if h == 0 else ctx.nlm8(x, P, S, s, h))
    f = nle.NLEFilter(ctx).train_filter(pre(L)[1], q["nr"], q["nc"], q["hx"], q["hy"], q["T"], q["K"])
    try:
        ev = f.eigvals
        planes = torch.stack([ctx.lab8_channel(lab, ch) for ch in range(3)])
        if not glide:
            resp = np.array([math.pow(min(l, 1.0), q["k"]) for l in ev])
            ab = f.apply_planes(planes[1:], [resp, resp], out_kind=nle.REGION_OUT_ROUNDED8)
            return ctx.lab2bgr8(lab, pre(planes[0])[1], ab[0].view(H, W), ab[1].view(H, W)).cpu().numpy(), None
        sig, pres = [], []
        for ch in range(3):
            s, p = pre(planes[ch])
            sig.append(s if nlm else ctx.plane_noise(planes[ch])[1])
            pres.append(p)
        b = f.coefficients(torch.stack(pres))
        ks = [nle.mse_shrink(ev, b[ch], sig[ch], q["k"], 256)[0] for ch in range(3)]
        resp = [np.array([math.pow(min(max(l, 0.0), 1.0), ks[ch]) for l in ev]) for ch in range(3)]
        y = f.apply_planes(planes, resp, out_kind=nle.REGION_OUT_ROUNDED8)
        return ctx.lab2bgr8(lab, y[0].view(H, W), y[1].view(H, W), y[2].view(H, W)).cpu().numpy(), list(zip(sig, ks))
    finally:
        f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("glide,nlm", [(True, True), (True, False), (False, True)], ids=["glide-nlm", "glide", "nlm"])
def test_denoise_cli_equals_the_mirror_composition(nle, ctx, tmp_path, glide, nlm):
    _, noisy = colour_scene(48, 64, 3)
    opts = (["--glide"] if glide else []) + (["--prefilter", "nlm"] if nlm else [])
    got, lines = run_denoise(tmp_path, noisy, opts, WIRE, "out")
    want, report = mirror_denoise(nle, ctx, noisy, WIRE, glide, nlm)
    assert np.array_equal(got, want)                                      # byte for byte
    assert lines[-1] == "Done. Press any key in result window to exit."
    glide_lines = [l for l in lines if l.startswith("glide:")]
    if glide:
        (sL, kL), (sa, ka), (sb, kb) = report
        assert glide_lines == ["glide: L sigma=%g k=%g  a sigma=%g k=%g  b sigma=%g k=%g" % (sL, kL, sa, ka, sb, kb)]
        assert lines.index(glide_lines[0]) == len(lines) - 2              # before the banner
    else:
        assert glide_lines == []


@pytest.mark.gpu
def test_prefilter_bilateral_and_given_levels(nle, ctx, tmp_path):
    """--prefilter bilateral writes what no option writes; --noise-sigma and --nlm-h reach the calls"""
    _, noisy = colour_scene(48, 64, 3)
    plain, _ = run_denoise(tmp_path, noisy, [], WIRE, "plain")
    same, _ = run_denoise(tmp_path, noisy, ["--prefilter", "bilateral"], WIRE, "bilateral")
    assert np.array_equal(plain, same)
    rep = tmp_path / "report.json"
    os.environ["NLE_REPORT"] = str(rep)
    try:
        _, lines = run_denoise(tmp_path, noisy, ["--glide", "--noise-sigma", "7.5", "--prefilter", "nlm", "--nlm-h", "3"], WIRE, "given")
    finally:
        del os.environ["NLE_REPORT"]
    line = [l for l in lines if l.startswith("glide:")][0]
    assert line.count("sigma=7.5 ") == 3
    import json
    g = json.loads(rep.read_text())["glide"]
    assert sorted(g) == ["L", "a", "b"] and all(g[c]["sigma"] == 7.5 and 0.0 <= g[c]["k"] <= WIRE["k"] and g[c]["mse"] >= 0 for c in g)
    assert "k=%g" % g["L"]["k"] in line


@pytest.mark.gpu
def test_glide_denoises(nle, tmp_path):
    """the floor: on a piecewise-constant scene with Gaussian noise of sigma 12 the output is closer to the clean image than
    the input is (test_quality_floor_holds_for_the_oracle_composition: the same on the CPU, from the oracle)"""
    q = dict(QUALITY, sc=10, ss=3, k=QUALITY["k_max"])
    clean, noisy = colour_scene(*q["shape"], q["seed"])
    out, lines = run_denoise(tmp_path, noisy, ["--glide", "--prefilter", "nlm"], q, "q")
    print("glide + nlm: PSNR noisy %.3f -> %.3f; %s" % (psnr(noisy, clean), psnr(out, clean), [l for l in lines if l.startswith("glide:")]))
    assert psnr(out, clean) > psnr(noisy, clean)
