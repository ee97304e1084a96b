"""The out-of-span detail layer and the detail curve (include/nle.h at nle_detail_combine states the
rule).  There is no reference for it, so the rule is restated here in numpy -- fp64, the yardstick with the curve off, where
the kernel has to reproduce it bit for bit, and longdouble, the yardstick with the curve on -- and the tests hold the kernel,
the two entry points, the Python mirror, the C++ surface and the `enhance` options to it.

Bounds.  Curve off: every operation of the rule is one IEEE fp64 operation, so the device result equals the fp64
restatement in every bit.  Curve on: the device's exp is within one ulp of the correctly rounded value, which moves y by a few
fp64 ulp; the stored fp32 value (or level) differs from the longdouble restatement's only where y lies within ~1e-15
relative of an fp32 rounding boundary (or of a .5 tie): at most 1 pixel in 1e5 may differ, by one fp32 ulp or one level (the
fp64 numpy restatement differs from the longdouble one in 0 of 2 000 000 pixels at the three settings below).  A fused
multiply-add, a reciprocal in place of the division or another order of the sum would exceed that by orders of magnitude.
Against the oracle: ||y_dev - y_ref||_2 <= 1e-4 Lambda(a) sum_l (|w_l| + |w_rho|) ||Y_l||_2 -- the project's 1e-4 per-layer
bar carried through a Lambda-Lipschitz map and the linear sum (rho = x - sum Y_l inherits every layer's error).

Identity.  With every weight 1, w_rho = 1 and the curve off the rule returns x up to a few fp64 ulp of sum |Y_l|; the stored
value is x exactly wherever x is an integer other than 0 (the ROUNDED8 and U8 kinds: everywhere).  At x = 0 the fp64 residue
has no integer to round to in the F32 kind: there it is held to 8 ulp of sum |Y_l|."""
import ctypes as C
import os
import re
import shutil
import subprocess
import textwrap

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT

ENHANCE = os.path.join(PKG_DIR, "bin", "enhance")
DENOISE = os.path.join(PKG_DIR, "bin", "denoise")
F32, ROUNDED8, U8 = 0, 1, 2
KINDS = [F32, ROUNDED8, U8]
GRID_CAP_N = 4096 * 256 * 4 + 1027      # past the grid cap times the block size times four pixels: the stride loop wraps
# (gain, sigma, weights, w_rho): the settings of the cap above
CURVES = [(2.5, 6.0, [3.0, 3.0, 1.0, 1.0], 3.0), (0.0, 4.0, [1.0, 1.0, 1.0, 1.0], 1.0), (3.0, 20.0, [10.0, 5.0, 2.0, 1.05], 10.0)]


# ------------------------------------------------------------------------------------------------ the restatement
def g_of(d, a, sigma, dt=np.float64):
    """the gain curve, operation by operation; a - 1 is formed once, in fp64, as the host forms it"""
    if sigma == 0 or a == 1:
        return d
    t = d / dt(sigma)
    return d * (dt(1.0) + dt(np.float64(a) - 1.0) * np.exp(-(t * t)))


def rule(x, Y, w, w_rho, a=1.0, sigma=0.0, dt=np.float64):
    """y of the rule in dtype dt: x (n,), Y (L, n) fp32 planes, w the L weights"""
    x, Y = np.asarray(x, dtype=np.float32).astype(dt), np.asarray(Y, dtype=np.float32).astype(dt)
    L = Y.shape[0]
    S = Y[0]
    for l in range(1, L):
        S = S + Y[l]
    rho = x - S
    y = dt(w_rho) * g_of(rho, a, sigma, dt)
    for l in range(L - 1):
        y = y + dt(w[l]) * g_of(Y[l], a, sigma, dt)
    return y + dt(w[L - 1]) * Y[L - 1]


def store(y, kind):
    """the store rule of the three output kinds: (float)y, then round half to even and saturate"""
    v = y.astype(np.float32)
    if kind == F32:
        return v
    r = unsigned_zero(np.clip(np.rint(v), np.float32(0), np.float32(255)))
    return r if kind == ROUNDED8 else r.astype(np.uint8)


def unsigned_zero(v):
    """-0 as +0: the sign of a zero LEVEL is not part of the store rule (the maximum of 0 and -0 may be either, in numpy's
    clip as in fmaxf); the F32 kind is compared sign and all"""
    return v + np.float32(0.0)


def lipschitz(a):
    return max(a, 1.4463 - 0.4463 * a)


def planes(n, L, seed):
    """inputs of the kind the cap was measured on: detail layers N(0, 3 | 6 | 10), a base U(0, 255), rho ~ N(0, 2)"""
    rng = np.random.default_rng(seed)
    Y = np.stack([rng.normal(0, (3, 6, 10)[l % 3], n) for l in range(L - 1)] + [rng.uniform(0, 255, n)]).astype(np.float32)
    x = (Y.astype(np.float64).sum(axis=0) + rng.normal(0, 2, n)).astype(np.float32)
    return x, Y


# ------------------------------------------------------------------------------------------------ CPU: the curve
GRID = np.linspace(-60.0, 60.0, 400001)      # sigma = 6: ten sigma either side, steps of 5e-5 sigma


@pytest.mark.parametrize("a", [0.0, 0.5, 1.0, 2.0, 3.0])
def test_the_curve_is_monotone_with_slope_a_at_0_the_identity_far_out_and_lipschitz(a):
    sigma = 6.0
    g = g_of(GRID, a, sigma)
    step = np.diff(g)
    assert np.all(step >= 0) and (a == 0.0 or np.all(step > 0))                     # non-decreasing at a = 0, else strictly
    assert np.all(step <= lipschitz(a) * np.diff(GRID) * (1 + 1e-9))                   # slope bounded by Lambda(a)
    tiny = np.array([-1e-6, 1e-6, 1e-9]) * sigma
    assert np.all(np.abs(g_of(tiny, a, sigma) / tiny - a) <= 1e-11)                    # g(d) / d -> a at 0
    far = np.concatenate([np.linspace(6, 50, 1001), -np.linspace(6, 50, 1001)]) * sigma
    assert np.all(np.abs(g_of(far, a, sigma) - far) < 1e-12 * np.abs(far))              # |g(d) - d| < 1e-12 |d| from 6 sigma on
    assert np.array_equal(g_of(-GRID, a, sigma), -g)                                   # odd


def test_the_curve_is_off_without_an_exp():
    d = np.array([np.inf, -3.0, 0.0, 1e300])
    assert g_of(d, 2.0, 0.0) is d and g_of(d, 1.0, 5.0) is d


def test_the_restatement_returns_an_integer_plane_under_unit_weights():
    rng = np.random.default_rng(3)
    for L in (1, 4, 16):
        Y = rng.normal(0, 50, (L, 20000)).astype(np.float32)
        x = rng.integers(0, 256, 20000).astype(np.float32)
        y = rule(x, Y, np.ones(L), 1.0)
        assert np.max(np.abs(y - x)) <= 8 * np.spacing(np.abs(Y.astype(np.float64)).sum(axis=0)).max()
        for kind in (ROUNDED8, U8):
            assert np.array_equal(store(y, kind).astype(np.float32), x)
        assert np.array_equal(store(y, F32)[x > 0], x[x > 0])


def test_header_constants_and_entry_points_are_mirrored(nle):
    text = open(os.path.join(ROOT, "include", "nle.h")).read()
    assert int(re.search(r"^#define\s+NLE_DETAIL_GAIN_MAX\s+(\d+)\s*$", text, flags=re.M).group(1)) == nle.DETAIL_GAIN_MAX == 3
    assert (nle.REGION_OUT_F32, nle.REGION_OUT_ROUNDED8, nle.REGION_OUT_U8) == (F32, ROUNDED8, U8)
    for name in ("nle_detail_combine", "nle_apply_detail"):
        assert name in nle.EXPORTED_SYMBOLS and hasattr(nle.lib(), name) and re.search(r"\b%s\s*\(" % name, text)
    assert callable(nle.Context.detail_combine) and callable(nle.NLEFilter.apply_detail)


# ------------------------------------------------------------------------------------------------ CPU: the CLI's refusals
ARGS8 = ["6", "8", "30", "30", "10", "8"]
W4 = ["1", "1", "1", "1"]
TAIL = ["missing.bmp", "o.png"] + ARGS8 + W4
REGION = ["--region", "mask.png:1,1,1,1"]


@pytest.mark.parametrize("exe,argv,option", [
    (ENHANCE, ["--residual-weight"], "--residual-weight"),
    (ENHANCE, ["--residual-weight"] + TAIL, "--residual-weight"),
    (ENHANCE, ["--residual-weight", "nan"] + TAIL, "--residual-weight"),
    (ENHANCE, ["--residual-weight", "inf"] + TAIL, "--residual-weight"),
    (ENHANCE, ["--residual-weight", "1x"] + TAIL, "--residual-weight"),
    (ENHANCE, ["--detail-sigma", "6", "--detail-gain"], "--detail-gain"),
    (ENHANCE, ["--detail-sigma", "6", "--detail-gain", "nan"] + TAIL, "--detail-gain"),
    (ENHANCE, ["--detail-sigma", "6", "--detail-gain", "3.01"] + TAIL, "--detail-gain"),
    (ENHANCE, ["--detail-sigma", "6", "--detail-gain", "-0.1"] + TAIL, "--detail-gain"),
    (ENHANCE, ["--detail-sigma"], "--detail-sigma"),
    (ENHANCE, ["--detail-sigma", "-1"] + TAIL, "--detail-sigma"),
    (ENHANCE, ["--detail-sigma", "inf"] + TAIL, "--detail-sigma"),
    (ENHANCE, ["--detail-gain", "2"] + TAIL, "--detail-gain"),
    (ENHANCE, ["--detail-gain", "2", "--detail-sigma", "0"] + TAIL, "--detail-gain"),
    (ENHANCE, ["--deep", "--detail-gain", "0"] + TAIL, "--detail-gain"),
    (ENHANCE, ["--residual-weight", "1"] + REGION + TAIL, "--residual-weight"),
    (ENHANCE, REGION + ["--detail-gain", "2", "--detail-sigma", "6"] + TAIL, "--detail-sigma"),
    (ENHANCE, REGION + ["--detail-sigma", "6", "--detail-gain", "1"] + TAIL, "--detail-gain"),
    (ENHANCE, ["--residual-weight", "1"] + TAIL + ["1"] * 13, "--residual-weight"),
    (DENOISE, ["--residual-weight", "1", "missing.bmp", "o.png"] + ARGS8 + ["10", "10", "2"], "--residual-weight"),
    (DENOISE, ["--detail-gain", "1", "missing.bmp", "o.png"] + ARGS8 + ["10", "10", "2"], "--detail-gain"),
    (DENOISE, ["--detail-sigma", "0", "missing.bmp", "o.png"] + ARGS8 + ["10", "10", "2"], "--detail-sigma"),
], ids=["weight-missing", "weight-no-number", "weight-nan", "weight-inf", "weight-garbage", "gain-missing", "gain-nan", "gain-above",
        "gain-below", "sigma-missing", "sigma-negative", "sigma-inf", "gain-without-sigma", "gain-with-sigma-0", "deep-gain-without-sigma",
        "weight-region", "region-curve", "region-inactive", "seventeen-weights", "denoise-weight", "denoise-gain", "denoise-sigma"])
def test_cli_refuses_before_anything_runs(tmp_path, exe, argv, option):
    """status 2 and one line on stderr that names the option; the input does not even exist, so nothing was read and no GPU
    call was made"""
    r = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert len(r.stderr.strip().splitlines()) == 1 and option in r.stderr and r.stdout == ""
    assert not os.listdir(tmp_path)


# ------------------------------------------------------------------------------------------------ GPU: the stage kernel
def dev_planes(ctx, x, Y, ox=0, ol=0, oo=0, stride=None, kind=F32, fill=float("nan")):
    """x, Y and a prefilled output on the device: base pointers ox, ol, oo elements past a 16-byte boundary, the layers
    `stride` floats apart, the output 64 elements longer than n"""
    import torch
    d = f"cuda:{ctx.device}"
    L, n = Y.shape
    stride = n if stride is None else stride
    tx = torch.zeros(n + 8, device=d)[ox:ox + n]
    tx.copy_(torch.from_numpy(np.array(x)))
    buf = torch.zeros(L * stride + 8, device=d)[ol:ol + L * stride]
    tY = buf.as_strided((L, n), (stride, 1))
    tY.copy_(torch.from_numpy(np.array(Y)))
    if kind == U8:
        out = torch.full((n + 64 + 8,), int(fill), dtype=torch.uint8, device=d)[oo:oo + n + 64]
    else:
        out = torch.full((n + 64 + 8,), fill, dtype=torch.float32, device=d)[oo:oo + n + 64]
    assert tx.data_ptr() % 16 == 4 * ox and tY.data_ptr() % 16 == 4 * ol and out.data_ptr() % 16 == (oo if kind == U8 else 4 * oo)
    return tx, tY, out


def check(ctx, x, Y, w, w_rho, a, sigma, kind, label="", **where):
    """one call of the stage kernel against the restatement; returns the number of differing pixels"""
    import torch
    n = x.size
    fills = (0x55, 0xAA) if kind == U8 else (float("nan"),)
    differ = 0
    curve = sigma != 0 and a != 1
    want = store(rule(x, Y, w, w_rho, a, sigma, np.longdouble if curve else np.float64), kind)
    for fill in fills:
        tx, tY, out = dev_planes(ctx, x, Y, kind=kind, fill=fill, **where)
        got = ctx.detail_combine(tx, tY, w, w_rho, a, sigma, kind, out=out[:n])
        assert got.data_ptr() == out.data_ptr()
        tail = out[n:].cpu().numpy()
        assert np.all(tail == int(fill)) if kind == U8 else np.all(np.isnan(tail)), "written past n"
        got = out[:n].cpu().numpy()
        if kind != U8:
            assert not np.any(np.isnan(got)), "a pixel was not written"
        if kind == ROUNDED8:
            got = unsigned_zero(got)
        if not curve:
            assert np.array_equal(got.view(np.uint8 if kind == U8 else np.int32), want.view(np.uint8 if kind == U8 else np.int32)), label
            continue
        bad = got != want
        differ = int(np.count_nonzero(bad))
        unit = np.spacing(np.abs(want[bad])).astype(np.float64) if kind == F32 else 1.0
        worst = float(np.max(np.abs(got[bad].astype(np.float64) - want[bad].astype(np.float64)) / unit)) if differ else 0.0
        print(f"{label} kind {kind}: {differ} of {n} differ from the longdouble restatement, worst {worst:.1f} units")
        assert differ <= n // 100000 and worst <= 1.0, (label, differ, worst)
    return differ


@pytest.fixture(scope="module")
def big():
    """2^20 + 1027 pixels, L = 4, of the kind the cap was measured on; never written to"""
    x, Y = planes((1 << 20) + 1027, 4, 41)
    x.setflags(write=False)
    Y.setflags(write=False)
    return x, Y


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("a,sigma", [(2.5, 0.0), (1.0, 6.0), (1.0, 0.0)], ids=["sigma-0", "gain-1", "both"])
def test_curve_off_is_the_fp64_restatement_bit_for_bit(ctx, big, kind, a, sigma):
    x, Y = big
    check(ctx, x, Y, [3.0, 3.0, 1.0, 1.05], 3.0, a, sigma, kind, "random")
    # multiples of 1/8 under weights that keep every product and sum exact: exact .5 ties and values either side of 0 and 255
    rng = np.random.default_rng(7)
    n = 200003
    Yq = (rng.integers(-80, 81, (2, n)) / 8.0).astype(np.float32)
    Yq[1] = (rng.integers(-400, 2800, n) / 8.0).astype(np.float32)
    xq = (rng.integers(-400, 2800, n) / 8.0).astype(np.float32)
    w, w_rho = [2.0, 0.5], 1.5
    y = rule(xq, Yq, w, w_rho)
    assert np.count_nonzero(np.abs(y - np.floor(y)) == 0.5) > 1000 and np.count_nonzero(y < -0.5) > 1000 and np.count_nonzero(y > 255.5) > 1000
    check(ctx, xq, Yq, w, w_rho, a, sigma, kind, "ties")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("a,sigma,w,w_rho", CURVES, ids=["boost", "core", "strong"])
def test_curve_on_against_the_longdouble_restatement(ctx, big, kind, a, sigma, w, w_rho):
    x, Y = big
    check(ctx, x, Y, w, w_rho, a, sigma, kind, f"a {a} sigma {sigma}")


WHERE = [dict(), dict(ox=1), dict(ol=2), dict(oo=3), dict(ox=3, ol=1, oo=2), dict(stride=1), dict(stride=2), dict(stride=3, ox=0, ol=0)]


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 2, 4, 5, 16])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 1027])
def test_shape_edges(ctx, n, L):
    """every size and layer count (4 and 5: either side of the few-layer instantiation), every base pointer 0 to 3 floats off
    a 16-byte boundary, layer strides that are no multiple of 4; curve off bit for bit, curve on within the cap (none of so few
    pixels may differ); outputs prefilled with NaN (bytes: two patterns), 64 elements longer than n"""
    x, Y = planes(n, L, 100 * L + n)
    w = list(np.linspace(3.0, 1.0, L))
    for where in WHERE:
        where = dict(where)
        if "stride" in where:
            where["stride"] = n + where["stride"]
        for kind in KINDS:
            check(ctx, x, Y, w, 2.0, 1.0, 0.0, kind, f"n {n} L {L} {where}", **where)
            assert check(ctx, x, Y, w, 2.0, 2.5, 6.0, kind, f"n {n} L {L} {where}", **where) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_past_the_grid_cap_the_stride_loop_wraps(ctx, kind):
    x, Y = planes(GRID_CAP_N, 2, 43)
    check(ctx, x, Y, [3.0, 1.0], 3.0, 1.0, 0.0, kind, "grid cap, vector form")
    check(ctx, x, Y, [3.0, 1.0], 3.0, 2.5, 6.0, kind, "grid cap, vector form")
    if kind == F32:     # and one pixel at a time: the second loop wraps four times as often
        check(ctx, x, Y, [3.0, 1.0], 3.0, 1.0, 0.0, kind, "grid cap, single pixels", ox=1)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 4, 16])
def test_unit_weights_return_an_integer_plane(ctx, L):
    rng = np.random.default_rng(50 + L)
    n = 100003
    Y = rng.normal(0, 50, (L, n)).astype(np.float32)
    x = rng.integers(0, 256, n).astype(np.float32)
    assert np.count_nonzero(x == 0) > 100 and np.count_nonzero(x == 255) > 100
    for kind in KINDS:
        tx, tY, out = dev_planes(ctx, x, Y, kind=kind, fill=0x55 if kind == U8 else float("nan"))
        got = ctx.detail_combine(tx, tY, np.ones(L), 1.0, out_kind=kind, out=out[:n]).cpu().numpy()
        if kind == F32:     # at x = 0 the residue of a few fp64 ulp has no integer to round to
            assert np.array_equal(got[x > 0], x[x > 0])
            assert np.all(np.abs(got[x == 0]) <= 8 * np.spacing(np.abs(Y.astype(np.float64)).sum(axis=0))[x == 0])
        else:
            assert np.array_equal(got.astype(np.float32), x)


def raw_combine(nle, ctx, x, Y, L, n, stride, w, w_rho, a, sigma, kind, out):
    ctx._sync_in()
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    wp = np.ascontiguousarray(w, dtype=np.float64).ctypes.data_as(C.c_void_p) if w is not None else None
    return nle.lib().nle_detail_combine(ctx._h, P(x), P(Y), L, n, stride, wp, w_rho, a, sigma, kind, P(out))


@pytest.mark.gpu
def test_refusals_leave_the_ctx_usable(nle, ctx):
    import torch
    n, L = 1000, 4
    x, Y = planes(n, L, 9)
    tx, tY, out = dev_planes(ctx, x, Y)
    w = [3.0, 3.0, 1.0, 1.0]
    want = store(rule(x, Y, w, 3.0), F32)
    nan, inf = float("nan"), float("inf")
    pool = torch.zeros(2 * L * n + 16, device=tx.device)
    pool[:L * n].copy_(tY.reshape(-1))
    inside = pool[:L * n].view(L, n)
    bad = [lambda: raw_combine(nle, ctx, tx, tY, 0, n, n, w, 3.0, 1.0, 0.0, F32, out),
           lambda: raw_combine(nle, ctx, tx, tY, 17, n, n, [1.0] * 17, 3.0, 1.0, 0.0, F32, out),
           lambda: raw_combine(nle, ctx, None, tY, L, n, n, w, 3.0, 1.0, 0.0, F32, out),
           lambda: raw_combine(nle, ctx, tx, None, L, n, n, w, 3.0, 1.0, 0.0, F32, out),
           lambda: raw_combine(nle, ctx, tx, tY, L, n, n, None, 3.0, 1.0, 0.0, F32, out),
           lambda: raw_combine(nle, ctx, tx, tY, L, n, n, w, 3.0, 1.0, 0.0, F32, None),
           lambda: raw_combine(nle, ctx, tx, tY, L, n, n, [3.0, nan, 1.0, 1.0], 3.0, 1.0, 0.0, F32, out),
           lambda: raw_combine(nle, ctx, tx, tY, L, n, n, [3.0, 3.0, 1.0, inf], 3.0, 1.0, 0.0, F32, out),
           lambda: raw_combine(nle, ctx, tx, tY, L, n, n, w, inf, 1.0, 0.0, F32, out),
           lambda: raw_combine(nle, ctx, tx, tY, L, n, n, w, nan, 1.0, 0.0, F32, out),
           lambda: raw_combine(nle, ctx, tx, tY, L, n, n, w, 3.0, -0.1, 6.0, F32, out),
           lambda: raw_combine(nle, ctx, tx, tY, L, n, n, w, 3.0, 3.1, 6.0, F32, out),
           lambda: raw_combine(nle, ctx, tx, tY, L, n, n, w, 3.0, nan, 6.0, F32, out),
           lambda: raw_combine(nle, ctx, tx, tY, L, n, n, w, 3.0, 2.0, -1.0, F32, out),
           lambda: raw_combine(nle, ctx, tx, tY, L, n, n, w, 3.0, 2.0, inf, F32, out),
           lambda: raw_combine(nle, ctx, tx, tY, L, n, n, w, 3.0, 2.0, nan, F32, out),
           lambda: raw_combine(nle, ctx, tx, tY, L, n, n, w, 3.0, 1.0, 0.0, 3, out),
           lambda: raw_combine(nle, ctx, tx, tY, L, n, n, w, 3.0, 1.0, 0.0, -1, out),
           lambda: raw_combine(nle, ctx, tx, tY, L, 0, n, w, 3.0, 1.0, 0.0, F32, out),
           lambda: raw_combine(nle, ctx, tx, tY, L, n, n - 1, w, 3.0, 1.0, 0.0, F32, out),
           lambda: raw_combine(nle, ctx, tx, tY, L, n, n, w, 3.0, 1.0, 0.0, F32, tx),                        # out is x
           lambda: raw_combine(nle, ctx, tx, tY, L, n, n, w, 3.0, 1.0, 0.0, F32, tx[n - 1:]),                # out meets x's last pixel
           lambda: raw_combine(nle, ctx, tx, inside, L, n, n, w, 3.0, 1.0, 0.0, F32, pool[2 * n + 5:]),      # out inside layer 2
           lambda: raw_combine(nle, ctx, tx, inside, L, n, n, w, 3.0, 1.0, 0.0, U8, pool[L * n - 1:])]       # bytes on the last layer's end
    for k, call in enumerate(bad):
        assert call() == nle.NLE_ERR_INVALID, k
        assert nle.lib().nle_last_error(ctx._h), k
        out.fill_(nan)
        assert raw_combine(nle, ctx, tx, tY, L, n, n, w, 3.0, 1.0, 0.0, F32, out) == nle.NLE_OK              # still usable
        assert np.array_equal(out[:n].cpu().numpy(), want), k
    # a neighbour is no overlap: the output right behind the last layer
    assert raw_combine(nle, ctx, tx, inside, L, n, n, w, 3.0, 1.0, 0.0, F32, pool[L * n:]) == nle.NLE_OK
    assert np.array_equal(pool[L * n:L * n + n].cpu().numpy(), want)
    with pytest.raises(nle.NLEError):
        ctx.detail_combine(tx, tY, w[:3], 3.0)
    with pytest.raises(nle.NLEError):
        ctx.detail_combine(tx[:-1], tY, w, 3.0)


# ------------------------------------------------------------------------------------------------ GPU: through a trained filter
SCENE_ARGS = dict(nr=6, nc=8, hx=30.0, hy=30.0, T=10, K=8)
SCENE_ARGV = ["6", "8", "30", "30", "10", "8"]
WIDE_ARGS = dict(nr=6, nc=8, hx=32.0, hy=30.0, T=10, K=10)
NL = 4


def scene48():
    """48 x 64: a 60 / 180 step, a 20 sin(col / 6) ramp and white texture integers(-4, 5), rounded and clipped"""
    rng = np.random.default_rng(15)
    rows, cols = np.mgrid[0:48, 0:64]
    x = np.where(cols < 32, 60.0, 180.0) + 20.0 * np.sin(cols / 6.0) + rng.integers(-4, 5, (48, 64))
    return np.clip(np.rint(x), 0, 255)


@pytest.fixture(scope="module")
def trained(nle, oracle, ctx):
    """name -> (the plane, the device filter, the oracle's fp64 layers of the plane); the layers are never written to"""
    out = {}
    for name, x, a in (("scene-48x64", scene48(), SCENE_ARGS), ("synthetic-96x128", oracle.synthetic_luminance(96, 128), WIDE_ARGS)):
        f = nle.NLEFilter(ctx).train_filter(x.astype(np.float32), a["nr"], a["nc"], a["hx"], a["hy"], a["T"], a["K"])
        V, S = oracle.train_filter(x, a["nr"], a["nc"], a["hx"], a["hy"], a["T"], a["K"])
        Yo = oracle.apply_layers(V, S, x, NL).reshape(NL, -1)
        Yo.setflags(write=False)
        out[name] = (x, f, Yo, (V, S))
    yield out
    for _, f, _, _ in out.values():
        f.close()


NAMES = ["scene-48x64", "synthetic-96x128"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_apply_detail_is_apply_layers_then_detail_combine(nle, ctx, trained, name):
    import torch
    x, f, _, _ = trained[name]
    seen = set()
    for plane in (x, x + 0.37 * np.cos(np.arange(x.size).reshape(x.shape))):      # the second: no integer plane
        tx = torch.as_tensor(plane.astype(np.float32), device=f"cuda:{ctx.device}")
        Y = f.apply_layers(tx, NL)
        for kind in KINDS:
            for a, sigma, w, w_rho in CURVES + [(1.0, 0.0, [3.0, 3.0, 1.0, 1.0], 3.0)]:
                one = f.apply_detail(tx, w, w_rho, a, sigma, kind)
                two = ctx.detail_combine(tx.reshape(-1), Y, w, w_rho, a, sigma, kind)
                assert one.dtype == two.dtype and torch.equal(one, two), (kind, a, sigma)
                seen.add(one.cpu().numpy().tobytes())
    assert len(seen) == 2 * 3 * 4       # every setting, kind and plane gave a result of its own


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_unit_weights_return_the_plane_which_the_plain_filter_does_not(nle, ctx, trained, name):
    """the test that fails without the feature.  Precondition, so that it is not vacuous: the part of the plane outside the
    span, measured on the device layers, is at least half of what the oracle gives for the scene, and more than 0.5 levels"""
    x, f, Yo, _ = trained[name]
    Y = f.apply_layers(x.astype(np.float32), NL).cpu().numpy().astype(np.float64)
    rms_dev = float(np.sqrt(np.mean((x.ravel() - Y.sum(axis=0)) ** 2)))
    rms_ora = float(np.sqrt(np.mean((x.ravel() - Yo.sum(axis=0)) ** 2)))
    print(f"{name}: rms of the out-of-span part: device {rms_dev:.3f}, oracle {rms_ora:.3f} levels")
    assert rms_dev >= 0.5 * rms_ora and rms_dev > 0.5
    got = f.apply_detail(x.astype(np.float32), [1.0] * NL, 1.0, out_kind=ROUNDED8).cpu().numpy()
    assert np.array_equal(got, x.ravel().astype(np.float32))
    plain = f.apply_rounded8(x.astype(np.float32), np.ones(len(f.eigvals))).cpu().numpy()
    moved = int(np.count_nonzero(plain != x.ravel()))
    print(f"{name}: the plain filter with the all-ones response moves {moved} of {x.size} pixels")
    assert moved > x.size // 10
    with pytest.raises(nle.NLEError):
        f.apply_detail(x[:-1].astype(np.float32), [1.0] * NL, 1.0)          # H W that is not the filter's
    with pytest.raises(nle.NLEError):
        f.apply_detail(x.astype(np.float32), [1.0] * 17, 1.0)
    with pytest.raises(nle.NLEError):
        f.apply_detail(x.astype(np.float32), [1.0] * NL, 1.0, gain=3.5, sigma=1.0)
    assert np.array_equal(f.apply_detail(x.astype(np.float32), [1.0] * NL, 1.0, out_kind=ROUNDED8).cpu().numpy(), got)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_against_the_oracle(nle, ctx, trained, name):
    x, f, Yo, _ = trained[name]
    worst = 0.0
    for a, sigma, w, w_rho in [(1.0, 0.0, [3.0, 3.0, 1.0, 1.0], 3.0), (2.5, 6.0, [3.0, 3.0, 1.0, 1.0], 3.0), (0.0, 4.0, [3.0, 3.0, 1.0, 1.0], 3.0)]:
        got = f.apply_detail(x.astype(np.float32), w, w_rho, a, sigma).cpu().numpy().astype(np.float64)
        # the fp64 rule on the oracle's fp64 layers (not rounded to fp32 on the way)
        S = Yo[0]
        for l in range(1, NL):
            S = S + Yo[l]
        ref = w_rho * g_of(x.ravel() - S, a, sigma)
        for l in range(NL - 1):
            ref = ref + w[l] * g_of(Yo[l], a, sigma)
        ref = ref + w[NL - 1] * Yo[NL - 1]
        err = float(np.linalg.norm(got - ref))
        bound = 1e-4 * lipschitz(a) * sum((abs(w[l]) + abs(w_rho)) * float(np.linalg.norm(Yo[l])) for l in range(NL))
        print(f"{name} a {a} sigma {sigma}: err {err:.3e} bound {bound:.3e} err / bound {err / bound:.3e}")
        worst = max(worst, err / bound)
        assert err <= bound
    print(f"{name}: largest err / bound {worst:.3e}")


# ------------------------------------------------------------------------------------------------ GPU: C++ surface and CLI
def colour_scene():
    """scene48 as an 8-bit BGR image: three tinted copies"""
    x = scene48()
    return np.clip(np.rint(np.stack([0.8 * x + 20, x, 0.9 * x + 10], axis=2)), 0, 255).astype(np.uint8)


def run_cli(lead, src, out, weights, env=None):
    r = subprocess.run([ENHANCE] + lead + [str(src), str(out)] + SCENE_ARGV + [repr(float(w)) for w in weights], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-1500:])
    return r.stdout


def train_scene(nle, ctx, guide):
    a = SCENE_ARGS
    return nle.NLEFilter(ctx).train_filter(guide, a["nr"], a["nc"], a["hx"], a["hy"], a["T"], a["K"])


@pytest.fixture(scope="module")
def bmp(tmp_path_factory):
    from PIL import Image
    bgr = colour_scene()
    path = tmp_path_factory.mktemp("detail8") / "in.bmp"
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(path)
    return path, bgr


def read_rgb8(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


@pytest.mark.gpu
def test_cli_residual_weight_1_returns_the_image_through_lab(nle, ctx, bmp, tmp_path):
    src, bgr = bmp
    run_cli(["--residual-weight", "1"], src, tmp_path / "o.png", [1, 1, 1, 1])
    lab, _ = ctx.bgr2lab8(bgr)
    want = ctx.lab2bgr8(lab).cpu().numpy()
    assert np.array_equal(read_rgb8(tmp_path / "o.png")[..., ::-1], want)
    run_cli([], src, tmp_path / "plain.png", [1, 1, 1, 1])
    assert not np.array_equal(read_rgb8(tmp_path / "plain.png")[..., ::-1], want)          # the plain filter loses the texture


@pytest.mark.gpu
@pytest.mark.parametrize("lead,kw", [(["--residual-weight", "3", "--detail-gain", "2.5", "--detail-sigma", "6"], dict(w_rho=3.0, a=2.5, sigma=6.0)),
                                     (["--detail-sigma", "4", "--sampler", "farthest", "--detail-gain", "0"], dict(w_rho=0.0, a=0.0, sigma=4.0, sampler=1)),
                                     (["--patch-radius", "1", "--residual-weight", "-0.5"], dict(w_rho=-0.5, a=1.0, sigma=0.0, patch=1))],
                         ids=["boost", "core-farthest", "negative-weight-patch"])
def test_cli_8_bit_equals_the_python_composition(nle, ctx, bmp, tmp_path, lead, kw):
    src, bgr = bmp
    w = [3.0, 3.0, 1.0, 1.0]
    run_cli(lead, src, tmp_path / "o.png", w)
    lab, L = ctx.bgr2lab8(bgr)
    try:
        ctx.set_patch_radius(kw.get("patch", 0))
        ctx.set_sampler(kw.get("sampler", 0))
        f = train_scene(nle, ctx, L)
    finally:
        ctx.set_patch_radius(0)
        ctx.set_sampler(0)
    y = f.apply_detail(L, w, kw["w_rho"], kw["a"], kw["sigma"], ROUNDED8)
    want = ctx.lab2bgr8(lab, L=y.reshape(L.shape)).cpu().numpy()
    plain = ctx.lab2bgr8(lab, L=f.apply_rounded8(L, nle.transform_eigenvalues(f.eigvals, w)).reshape(L.shape)).cpu().numpy()
    f.close()
    assert np.array_equal(read_rgb8(tmp_path / "o.png")[..., ::-1], want) and not np.array_equal(want, plain)


@pytest.mark.gpu
def test_cli_deep_equals_the_python_composition(nle, ctx, tmp_path):
    from test_deep_colour import gradient16
    from test_image_io16 import png_bytes, read_png16_rgb
    bgr = gradient16(48, 64, 5)
    src = tmp_path / "in.png"
    src.write_bytes(png_bytes(bgr[..., ::-1], filt=1))
    w = [3.0, 3.0, 1.0, 1.0]
    run_cli(["--deep", "--detail-gain", "2.5", "--residual-weight", "2", "--detail-sigma", "3"], src, tmp_path / "o.png", w)
    L, a, b, g = ctx.bgr16_to_lab(bgr)
    f = train_scene(nle, ctx, g)
    y = f.apply_detail(L, w, 2.0, 2.5, 3.0, F32)                         # on the unrounded L
    want = ctx.lab_to_bgr16(y.reshape(L.shape), a, b).cpu().numpy()
    plain = ctx.lab_to_bgr16(f.apply(L, nle.transform_eigenvalues(f.eigvals, w)).reshape(L.shape), a, b).cpu().numpy()
    f.close()
    assert np.array_equal(read_png16_rgb(tmp_path / "o.png")[..., ::-1], want) and not np.array_equal(want, plain)
    # inactive options: the bytes of the plain command
    run_cli(["--residual-weight", "0", "--deep", "--detail-gain", "1"], src, tmp_path / "inactive.png", w)
    assert np.array_equal(read_png16_rgb(tmp_path / "inactive.png")[..., ::-1], plain)


@pytest.mark.gpu
def test_cli_tonemap_equals_the_python_composition(nle, ctx, tmp_path):
    from test_image_io16 import read_png16_rgb
    from test_tonemap import scene_files
    src, bgr, _, _ = scene_files(tmp_path)["scene-48x64"]
    w = [2.0, 2.0, 1.0, 0.4]
    run_cli(["--detail-sigma", "5", "--tonemap", "--residual-weight", "1.5", "--detail-gain", "2"], src, tmp_path / "o.png", w)
    l_hi, R = ctx.hdr_range(bgr)
    x, g = ctx.hdr_to_loglum(bgr, l_hi, R)
    f = train_scene(nle, ctx, g)
    y = f.apply_detail(x, w, 1.5, 2.0, 5.0, F32)                         # on the unrounded log-luminance
    want = ctx.loglum_to_bgr16(y.reshape(x.shape), bgr, l_hi, R, w[-1], 1.0).cpu().numpy()          # the last weight is still the base weight
    plain = ctx.loglum_to_bgr16(f.apply(x, nle.transform_eigenvalues(f.eigvals, w)).reshape(x.shape), bgr, l_hi, R, w[-1], 1.0).cpu().numpy()
    f.close()
    assert np.array_equal(read_png16_rgb(tmp_path / "o.png")[..., ::-1], want) and not np.array_equal(want, plain)
    run_cli(["--tonemap", "--detail-gain", "1", "--residual-weight", "0"], src, tmp_path / "inactive.png", w)
    assert np.array_equal(read_png16_rgb(tmp_path / "inactive.png")[..., ::-1], plain)


@pytest.mark.gpu
def test_cli_inactive_options_give_the_bytes_of_the_plain_command(bmp, tmp_path):
    src, _ = bmp
    w = [3.0, 3.0, 1.0, 1.0]
    run_cli([], src, tmp_path / "plain.png", w)
    run_cli(["--residual-weight", "0", "--detail-gain", "1"], src, tmp_path / "a.png", w)
    run_cli(["--detail-sigma", "6", "--residual-weight", "-0"], src, tmp_path / "b.png", w)
    plain = (tmp_path / "plain.png").read_bytes()
    assert (tmp_path / "a.png").read_bytes() == plain and (tmp_path / "b.png").read_bytes() == plain


DRIVER = textwrap.dedent(r"""
    #include <cstdio>
    #include <cstdlib>
    #include <cstring>
    #include <functional>
    #include <string>
    #include <vector>
    #include "nle.h"
    #include "nle/filter.hpp"
    #include "nle/image_io.hpp"
    #define REQUIRE(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
    static bool same(const nle::Image& a, const nle::Image& b) {
        return a.rows == b.rows && a.cols == b.cols && std::memcmp(a.ptr<unsigned char>(), b.ptr<unsigned char>(), 3 * a.total()) == 0;
    }
    int main(int argc, char** argv) {   // in out mode
        const nle::Image im = nle::imread(argv[1]);
        REQUIRE(!im.empty() && im.depth() == nle::NLE_8U && im.channels() == 3);
        const std::vector<double> w = {3, 3, 1, 1};
        nle::NLEFilter f;
        f.verbose = false;
        f.trainForEnhancement(im, 6, 8, 30, 30, 10, 8);
        nle::DetailOptions on;
        on.residualWeight = 3, on.gain = 2.5, on.sigma = 6;
        if (std::string(argv[3]) == "group") {      // trained over a device group: active options are refused by name
            try {
                f.enhance(im, w, on);
                REQUIRE(false);
            } catch (const std::runtime_error& e) {
                REQUIRE(std::string(e.what()).find("DetailOptions") != std::string::npos);
            }
            nle::DetailOptions off;
            off.sigma = 6;
            REQUIRE(same(f.enhance(im, w, off), f.enhance(im, w)));      // inactive ones are the plain method, groups included
            std::printf("group OK\n");
            return 0;
        }
        const nle::Image plain = f.enhance(im, w);
        nle::DetailOptions off;
        REQUIRE(!off.active() && on.active() && same(f.enhance(im, w, off), plain));
        off.gain = 1, off.sigma = 6;
        REQUIRE(!off.active() && same(f.enhance(im, w, off), plain));
        off.gain = 2, off.sigma = 0;
        REQUIRE(!off.active() && same(f.enhance(im, w, off), plain));
        const nle::Image out = f.enhance(im, w, on);
        REQUIRE(!same(out, plain) && nle::imwrite(argv[2], out));
        nle::DetailOptions bad = on;
        bad.gain = 3.5;
        bool threw = false;
        try { f.enhance(im, w, bad); } catch (const std::runtime_error&) { threw = true; }
        REQUIRE(threw);
        threw = false;
        try { f.enhance(im, std::vector<double>(17, 1.0), on); } catch (const std::runtime_error&) { threw = true; }
        REQUIRE(threw);
        threw = false;
        try { f.toneMap(im, w, 1.0, on); } catch (const std::runtime_error&) { threw = true; }      // no 32F image
        REQUIRE(threw);
        REQUIRE(same(f.enhance(im, w, on), out));
        std::printf("detail OK\n");
        return 0;
    }
""")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("detaildrv")
    host, libdir = os.path.join(PKG_DIR, "host"), os.path.join(PKG_DIR, "lib")
    (d / "drv.cpp").write_text(DRIVER)
    b = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(d / "drv.cpp"),
                        *[os.path.join(host, s) for s in ("filter.cpp", "stages.cpp", "colour.cpp", "device_group.cpp", "image_io.cpp", "jpeg.cpp")],
                        "-L", libdir, "-lnle_hip", "-Wl,-rpath," + libdir, "-o", str(d / "drv")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    return str(d / "drv")


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_cpp_surface_equals_the_cli_and_inactive_options_are_the_plain_method(driver, bmp, tmp_path):
    src, _ = bmp
    env = {k: v for k, v in os.environ.items() if k != "NLE_DEVICES"}
    r = subprocess.run([driver, str(src), str(tmp_path / "drv.png"), "one"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "detail OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    run_cli(["--residual-weight", "3", "--detail-gain", "2.5", "--detail-sigma", "6"], src, tmp_path / "cli.png", [3, 3, 1, 1], env=env)
    assert np.array_equal(read_rgb8(tmp_path / "drv.png"), read_rgb8(tmp_path / "cli.png"))


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_a_group_trained_filter_is_refused(driver, bmp, tmp_path):
    """NLE_DEVICES with the same device twice forms a group: the train shards the image, enhance with active options throws"""
    src, _ = bmp
    r = subprocess.run([driver, str(src), str(tmp_path / "drv.png"), "group"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, NLE_DEVICES="0,0"))
    assert r.returncode == 0 and "group OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
