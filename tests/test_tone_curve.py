"""The base tone curve: shadows, highlights, auto levels, equalise (include/nle.h at nle_tone_combine
states the rule).  There is no reference for it, so the rule is restated here in numpy, operation by operation in fp64, and
the tests hold the histogram kernel, the host rule, the combine, the one-call form, the Python mirror and the `enhance`
options to it.

Bounds.  The histogram counts integers: all NLE_TONE_BINS + 2 counts equal numpy's.  The curve: lo and hi come from integer
comparisons and two exact products, so they are equal; the knots are ~15 fp64 operations on values in [0, 255], so
1e-12 * 255 is loose by three orders and still far below anything a wrong order or a contracted product would give.  The
combine with the detail curve off: every operation of the rule is one IEEE fp64 operation, the device equals the restatement
in every bit.  With it on: the bound of tests/test_detail_curve.py for its exp cases -- at most 1 pixel in 1e5 may differ, by
one fp32 ulp or one level (so none of the few thousand pixels here).  The base term itself is restated in fp64 in both cases:
it has no transcendental.  Identity knots T_k = 255 k / N over [0, 255]: B' differs from Bw by a few fp64 ulp of 255, so the
F32 kind is within one fp32 ulp of nle_detail_combine and the rounded kinds equal it wherever y is no exact .5 tie."""
import ctypes as C
import os
import re
import shutil
import subprocess
import textwrap

import numpy as np
import pytest

from conftest import GOLDEN, PKG_DIR, ROOT
from test_detail_curve import (F32, KINDS, NL, ROUNDED8, SCENE_ARGV, U8, colour_scene, dev_planes, g_of, planes, read_rgb8, rule, scene48,
                               store, train_scene, unsigned_zero)

ENHANCE = os.path.join(PKG_DIR, "bin", "enhance")
N = 1024
BINS = 4096


# ------------------------------------------------------------------------------------------------ the restatement
def np_hist(x, scale):
    """the BINS + 2 counts of the fp32 values x times scale"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(x, dtype=np.float32).astype(np.float64).ravel() * np.float64(scale)
        t = (v + 256.0) * 4.0
    counts = np.zeros(BINS + 2, dtype=np.int64)
    nan = np.isnan(t)
    counts[BINS + 1] += int(np.count_nonzero(nan)) + int(np.count_nonzero(t[~nan] >= BINS))
    counts[0] += int(np.count_nonzero(t[~nan] < 0))
    mid = t[~nan & (t >= 0) & (t < BINS)]
    counts[1:BINS + 1] += np.bincount(np.floor(mid).astype(np.int64), minlength=BINS)
    return counts


def np_C(t, s, h):
    u = 1.0 - t
    return (t + (s * t) * (u * u)) - (h * (t * t)) * u


def np_curve(counts, s=0.0, h=0.0, P=-1.0, A=0.0):
    """[lo, hi, T_0 .. T_N] by the text of the rule"""
    lo, hi = 0.0, 255.0
    if P >= 0 or A != 0:
        c = np.asarray(counts, dtype=np.int64)
        n = np.float64(int(c.sum()))
    if P >= 0:
        need = np.float64(P) / 100.0 * n
        below = (c[0] + np.cumsum(c[1:BINS + 1])).astype(np.float64) > need                  # k: counts[0] + sum_{j <= k}
        above = (c[BINS + 1] + np.cumsum(c[1:BINS + 1][::-1])[::-1]).astype(np.float64) > need  # k: counts[4097] + sum_{j >= k}
        if below.any() and above.any():
            klo, khi = int(np.argmax(below)), int(BINS - 1 - np.argmax(above[::-1]))
            l, hh = -256.0 + 0.25 * klo, -256.0 + 0.25 * (khi + 1)
            if not hh - l < 1:
                lo, hi = l, hh
    t = np.arange(N + 1, dtype=np.float64) / np.float64(N)
    m = t
    if A != 0:
        prefix = np.concatenate([[c[0]], c[0] + np.cumsum(c[1:BINS + 1])])       # prefix[k] = counts[0] + sum_{j < k}

        def F(v):
            q = (v + 256.0) * 4.0
            k = np.minimum(np.floor(q), BINS - 1).astype(np.int64)
            phi = q - k.astype(np.float64)
            return (prefix[k].astype(np.float64) + phi * c[1 + k].astype(np.float64)) / n
        F_lo = F(np.float64(lo))
        den = F(np.float64(hi)) - F_lo
        E = t if den == 0 else (F(lo + t * (hi - lo)) - F_lo) / den
        m = (1.0 - np.float64(A)) * t + np.float64(A) * E
    return np.concatenate([[lo, hi], 255.0 * np_C(m, np.float64(s), np.float64(h))])


def np_base(Bw, curve):
    """B' of the fp64 values Bw"""
    lo, hi, T = curve[0], curve[1], np.asarray(curve[2:], dtype=np.float64)
    ks = np.float64(N) / (hi - lo)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (Bw - lo) * ks
        j = np.clip(np.floor(np.nan_to_num(u, nan=0.0, posinf=float(N), neginf=-1.0)), 0, N - 1).astype(np.int64)
        f = u - j.astype(np.float64)
        return T[j] + f * (T[j + 1] - T[j])


def tone_rule(x, Y, w, w_rho, curve, a=1.0, sigma=0.0, dt=np.float64):
    """y of the rule: the detail terms in dtype dt (test_detail_curve's restatement), the base term in fp64"""
    x, Yd = np.asarray(x, dtype=np.float32).astype(dt), np.asarray(Y, dtype=np.float32).astype(dt)
    L = Yd.shape[0]
    with np.errstate(invalid="ignore"):
        S = Yd[0]
        for l in range(1, L):
            S = S + Yd[l]
        rho = x - S
        y = dt(w_rho) * g_of(rho, a, sigma, dt)
        for l in range(L - 1):
            y = y + dt(w[l]) * g_of(Yd[l], a, sigma, dt)
        Bw = np.float64(w[L - 1]) * np.asarray(Y, dtype=np.float32)[L - 1].astype(np.float64)
        return y + np_base(Bw, curve).astype(dt)


def store_nan(y, kind):
    """store() with a NaN y: NaN in the F32 kind, 0 in the other two"""
    with np.errstate(invalid="ignore"):
        v = y.astype(np.float32)
        if kind == F32:
            return v
        r = unsigned_zero(np.clip(np.rint(np.where(np.isnan(v), np.float32(0), v)), np.float32(0), np.float32(255)))
        return r if kind == ROUNDED8 else r.astype(np.uint8)


def manual_curve(lo, hi, s, h):
    t = np.arange(N + 1, dtype=np.float64) / N
    return np.concatenate([[lo, hi], 255.0 * np_C(t, s, h)])


IDENTITY = manual_curve(0.0, 255.0, 0.0, 0.0)


# ------------------------------------------------------------------------------------------------ CPU: surface
def test_header_constants_and_entry_points_are_mirrored(nle):
    text = open(os.path.join(ROOT, "include", "nle.h")).read()
    assert int(re.search(r"^#define\s+NLE_TONE_KNOTS\s+(\d+)\s*$", text, flags=re.M).group(1)) == nle.TONE_KNOTS == N + 1
    assert int(re.search(r"^#define\s+NLE_TONE_BINS\s+(\d+)\s*$", text, flags=re.M).group(1)) == nle.TONE_BINS == BINS
    for name in ("nle_plane_histogram", "nle_tone_curve", "nle_tone_combine", "nle_apply_tone"):
        assert name in nle.EXPORTED_SYMBOLS and hasattr(nle.lib(), name) and re.search(r"\b%s\s*\(" % name, text)
    assert callable(nle.Context.plane_histogram) and callable(nle.Context.tone_combine) and callable(nle.NLEFilter.apply_tone)
    # the new kernel ids follow the existing ones, which do not move
    assert nle.KERNEL_COUNT == 12 and nle.KERNEL_COUNT_ALL == 16
    names = [nle.lib().nle_kernel_name(k).decode() for k in range(nle.KERNEL_COUNT_ALL)]
    assert names[12:] == ["nlm8", "plane_noise", "plane_hist", "tone_combine"] and names[0] == "affinity"


# ------------------------------------------------------------------------------------------------ CPU: the curve
def spikes(*at):
    c = np.zeros(BINS + 2, dtype=np.int64)
    for i, v in at:
        c[i] += v
    return c


def flower_counts():
    """the counts of the flower's L channel as PIL gives it (mode "L", the 8-bit luma): min 0, max 207"""
    from PIL import Image
    L = np.asarray(Image.open(os.path.join(GOLDEN, "flower-50.bmp")).convert("L"))
    assert L.min() == 0 and L.max() == 207
    return np_hist(L.astype(np.float32), 1.0)


@pytest.fixture(scope="module")
def count_cases():
    rng = np.random.default_rng(5)
    smooth = np_hist(np.clip(rng.normal(110, 40, 50000), -300, 800), 1.0)
    return {"one-bin": spikes((1 + 1500, 1000)), "underflow": spikes((0, 77)), "overflow": spikes((BINS + 1, 77)),
            "two-spikes": spikes((1 + 1100, 300), (1 + 1900, 700)), "spikes-and-ends": spikes((0, 5), (1 + 1100, 90), (1 + 1900, 100), (BINS + 1, 5)),
            "smooth": smooth, "flower": flower_counts()}


PARAMS = [(0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 25.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 5.0, 0.5), (0.3, -0.2, -1.0, 1.0),
          (0.0, 0.0, -1.0, 0.5), (1.0, 1.0, 1.0, 1.0), (1.0, -1.0, 0.0, 0.5), (-1.0, 1.0, 25.0, 0.0), (-1.0, -1.0, 1.0, 1.0),
          (0.8, 0.0, -1.0, 0.0), (0.0, -0.7, -1.0, 0.0)]


def test_tone_curve_is_the_numpy_restatement(nle, count_cases):
    for name, counts in count_cases.items():
        for s, h, P, A in PARAMS:
            got = nle.tone_curve(counts, s, h, P, A)
            want = np_curve(counts, s, h, P, A)
            assert got.shape == (N + 3,)
            assert got[0] == want[0] and got[1] == want[1], (name, s, h, P, A, got[:2], want[:2])
            err = float(np.max(np.abs(got[2:] - want[2:])))
            assert err <= 1e-12 * 255, (name, s, h, P, A, err)
            assert np.all(np.diff(got[2:]) >= 0), (name, s, h, P, A)
            if A == 0:
                assert got[2] == 0 and got[-1] == 255
    # without statistics the counts may be absent
    assert np.array_equal(nle.tone_curve(None, 0.8, -0.3), np_curve(None, 0.8, -0.3))
    assert np.array_equal(nle.tone_curve(None), IDENTITY)


def test_levels_of_the_hand_made_counts_and_the_flower(nle, count_cases):
    lv = lambda name, P: tuple(nle.tone_curve(count_cases[name], 0, 0, P, 0)[:2])  # noqa: E731
    assert lv("flower", 0) == (0.0, 207.25) and lv("flower", 1) == (13.0, 150.25) and lv("flower", 5) == (26.0, 133.25)
    assert lv("one-bin", 0) == lv("one-bin", 25) == (0.0, 255.0)                  # a quarter level is narrower than 1
    assert lv("underflow", 0) == lv("overflow", 0) == (0.0, 255.0)                # no bin exists
    assert lv("two-spikes", 0) == (19.0, 219.25) and lv("two-spikes", 25) == (19.0, 219.25)
    # 5 + 90 + 100 + 5 pixels: the end counters hold the first and the last bin at 0 %; at 2.5 % they reach `need` = 5 and do
    # not exceed it, so the spikes decide
    assert lv("spikes-and-ends", 0) == (-256.0, 768.0)
    assert lv("spikes-and-ends", 2.5) == lv("spikes-and-ends", 25) == (19.0, 219.25)


def test_the_curve_family_has_the_stated_properties():
    t = np.linspace(0.0, 1.0, 20001)
    for s in np.linspace(-1, 1, 9):
        for h in np.linspace(-1, 1, 9):
            c = np_C(t, s, h)
            assert c[0] == 0 and c[-1] == 1 and np.all(np.diff(c) >= 0)
            assert abs((c[1] - c[0]) / t[1] - (1 + s)) < 1e-3 and abs((c[-1] - c[-2]) / t[1] - (1 + h)) < 1e-3
            assert np.max(np.abs(c - t)) <= 4.0 / 27.0 * (abs(s) + abs(h)) + 1e-12      # t u^2 and t^2 u peak at 4 / 27 = 0.1482


def raw_curve(nle, counts, s, h, P, A, out=True):
    cp = np.ascontiguousarray(counts, dtype=np.int64).ctypes.data_as(C.c_void_p) if counts is not None else None
    curve = np.zeros(N + 3)
    st = nle.lib().nle_tone_curve(cp, s, h, P, A, curve.ctypes.data_as(C.c_void_p) if out else None)
    return st, (nle.lib().nle_last_error(None) or b"").decode()


def test_tone_curve_refusals_have_their_messages(nle, count_cases):
    ok = count_cases["smooth"]
    nan, inf = float("nan"), float("inf")
    neg = ok.copy()
    neg[7] = -1
    for args, word in [((ok, 1.01, 0, -1, 0), "shadows"), ((ok, nan, 0, -1, 0), "shadows"), ((ok, 0, -1.01, -1, 0), "highlights"),
                       ((ok, 0, inf, -1, 0), "highlights"), ((ok, 0, 0, 25.5, 0), "clip_percent"), ((ok, 0, 0, nan, 0), "clip_percent"),
                       ((ok, 0, 0, inf, 0), "clip_percent"), ((ok, 0, 0, -1, 1.5), "equalise"), ((ok, 0, 0, -1, -0.1), "equalise"),
                       ((ok, 0, 0, -1, nan), "equalise"), ((None, 0, 0, 1, 0), "NULL"), ((None, 0, 0, -1, 0.5), "NULL"),
                       ((np.zeros(BINS + 2, dtype=np.int64), 0, 0, 1, 0), "sum to 0"), ((np.zeros(BINS + 2, dtype=np.int64), 0, 0, -1, 1), "sum to 0"),
                       ((neg, 0, 0, 1, 0), "negative")]:
        st, msg = raw_curve(nle, *args)
        assert st == nle.NLE_ERR_INVALID and msg.startswith("nle_tone_curve") and word in msg, (args[1:], msg)
        with pytest.raises(nle.NLEError, match=word):
            nle.tone_curve(*args)
    st, msg = raw_curve(nle, ok, 0, 0, -1, 0, out=False)
    assert st == nle.NLE_ERR_INVALID and "NULL" in msg
    assert raw_curve(nle, np.zeros(BINS + 2, dtype=np.int64), 0.5, 0, -1, 0)[0] == nle.NLE_OK     # counts that are not needed are not read
    with pytest.raises(nle.NLEError):
        nle.tone_curve(np.zeros(10, dtype=np.int64), 0, 0, 1, 0)


# ------------------------------------------------------------------------------------------------ GPU: the histogram
def hist_values(n, seed):
    """n fp32 values: U(-300, 800), bin edges k / 4, the ends of the range and what has no bin"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-300, 800, n).astype(np.float32)
    edges = (rng.integers(-1100, 3200, n) / 4.0).astype(np.float32)
    x = np.where(rng.random(n) < 0.3, edges, x)
    special = np.array([-256.0, np.nextafter(np.float32(-256), np.float32(-np.inf)), 767.75, 768.0, np.nextafter(np.float32(768), np.float32(0)),
                        np.nan, np.inf, -np.inf, -0.0, 0.0, 255.0, 128.0], dtype=np.float32)
    k = min(n, special.size)
    x[rng.permutation(n)[:k]] = special[:k]
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, 100003])
def test_histogram_equals_numpy(ctx, n):
    import torch
    for seed, scale in enumerate((1.0, 0.4, 3.0)):
        x = hist_values(n, 10 * n + seed)
        for off in (0, 1, 3):                                   # the pointer: on a 16-byte boundary, one and three floats past it
            buf = torch.zeros(n + 8, device=f"cuda:{ctx.device}")
            t = buf[off:off + n]
            t.copy_(torch.from_numpy(x))
            assert t.data_ptr() % 16 == 4 * off
            got = ctx.plane_histogram(t, scale)
            assert got.dtype == np.int64 and got.sum() == n
            assert np.array_equal(got, np_hist(x, scale)), (n, scale, off)


@pytest.mark.gpu
def test_histogram_of_flat_and_special_planes(nle, ctx):
    import torch
    d = f"cuda:{ctx.device}"
    flat = torch.full((70000,), 128.0, device=d)
    want = np.zeros(BINS + 2, dtype=np.int64)
    want[1 + (128 + 256) * 4] = 70000
    assert np.array_equal(ctx.plane_histogram(flat), want)                    # everything in one bin
    x = np.array([-256.0, np.nextafter(np.float32(-256), np.float32(-np.inf)), 767.75, 768.0, np.nan, np.inf, -np.inf, -0.0], dtype=np.float32)
    got = ctx.plane_histogram(torch.from_numpy(x).to(d))
    assert got[0] == 2 and got[1] == 1 and got[BINS] == 1 and got[BINS + 1] == 3 and got[1 + 1024] == 1 and got.sum() == 8
    assert np.array_equal(ctx.plane_histogram(torch.from_numpy(x).to(d), 0.0), np_hist(x, 0.0))      # inf * 0 is a NaN
    # steps of 64 equal values and a ramp: runs that begin and end inside a wave, and none at all
    steps = np.repeat(np.arange(0, 200, dtype=np.float32), 37)
    ramp = np.arange(0, 5000, dtype=np.float32) / 16
    for v in (steps, ramp):
        assert np.array_equal(ctx.plane_histogram(torch.from_numpy(v).to(d)), np_hist(v, 1.0))
    # refusals: nothing is enqueued, the ctx stays usable
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    out = np.zeros(BINS + 2, dtype=np.int64)
    op = out.ctypes.data_as(C.c_void_p)
    for call, word in [(lambda: nle.lib().nle_plane_histogram(ctx._h, P(flat), 0, 1.0, op), "n must be"),
                       (lambda: nle.lib().nle_plane_histogram(ctx._h, None, 10, 1.0, op), "NULL"),
                       (lambda: nle.lib().nle_plane_histogram(ctx._h, P(flat), 10, 1.0, None), "NULL"),
                       (lambda: nle.lib().nle_plane_histogram(ctx._h, P(flat), 10, float("nan"), op), "scale"),
                       (lambda: nle.lib().nle_plane_histogram(ctx._h, P(flat), 10, float("inf"), op), "scale")]:
        assert call() == nle.NLE_ERR_INVALID
        msg = nle.lib().nle_last_error(ctx._h).decode()
        assert msg.startswith("nle_plane_histogram") and word in msg, msg
        assert np.array_equal(ctx.plane_histogram(flat), want)


# ------------------------------------------------------------------------------------------------ GPU: the combine
FILL = -12345.0
LEVELS = manual_curve(13.0, 150.25, 0.8, -0.5)      # the flower's levels at 1 %; the base runs from below lo to above hi


def check_tone(ctx, x, Y, w, w_rho, curve, a, sigma, kind, label="", **where):
    """one call of the stage kernel against the restatement; NaN pixels must be NaN (F32) or 0"""
    n = x.size
    on = sigma != 0 and a != 1
    want = store_nan(tone_rule(x, Y, w, w_rho, curve, a, sigma, np.longdouble if on else np.float64), kind)
    tx, tY, out = dev_planes(ctx, x, Y, kind=kind, fill=0x55 if kind == U8 else FILL, **where)
    got = ctx.tone_combine(tx, tY, w, curve, w_rho, a, sigma, kind, out=out[:n])
    assert got.data_ptr() == out.data_ptr()
    tail = out[n:].cpu().numpy()
    assert np.all(tail == (0x55 if kind == U8 else np.float32(FILL))), "written past n"
    got = out[:n].cpu().numpy()
    if kind == ROUNDED8:
        got = unsigned_zero(got)
    if kind != U8:
        assert np.array_equal(np.isnan(got), np.isnan(want)), label
        keep = ~np.isnan(want)
        got, want = got[keep], want[keep]
        assert not np.any(got == np.float32(FILL)) or np.any(want == np.float32(FILL)), "a pixel was not written"
    if not on:
        view = np.uint8 if kind == U8 else np.int32
        assert np.array_equal(got.view(view), want.view(view)), label
        return
    bad = got != want
    differ = int(np.count_nonzero(bad))
    unit = np.spacing(np.abs(want[bad])).astype(np.float64) if kind == F32 else 1.0
    worst = float(np.max(np.abs(got[bad].astype(np.float64) - want[bad].astype(np.float64)) / unit)) if differ else 0.0
    print(f"{label} kind {kind}: {differ} of {got.size} differ from the longdouble restatement, worst {worst:.1f} units")
    assert differ <= n // 100000 and worst <= 1.0, (label, differ, worst)


WHERE = [dict(), dict(ox=1), dict(ol=2), dict(oo=3), dict(ox=3, ol=1, oo=2), dict(stride=1), dict(stride=2), dict(stride=3)]


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 2, 4, 5, 16])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4099])
def test_tone_combine_is_the_restatement(ctx, n, L):
    """every size and layer count, every base pointer off its 16-byte boundary, strides that are no multiple of 4; a base
    layer whose weighted values lie below lo, above hi and, from three pixels on, are NaN at one pixel"""
    x, Y = planes(n, L, 300 * L + n)
    Y = Y.copy()
    if n >= 3:
        Y[L - 1, n // 2] = np.nan
    w = list(np.linspace(3.0, 0.9, L))
    Bw = w[L - 1] * Y[L - 1].astype(np.float64)
    if n > 1000:
        assert np.nanmin(Bw) < 13.0 - 5 and np.nanmax(Bw) > 150.25 + 5
    for where in WHERE:
        where = dict(where)
        if "stride" in where:
            where["stride"] = n + where["stride"]
        for kind in KINDS:
            check_tone(ctx, x, Y, w, 2.0, LEVELS, 1.0, 0.0, kind, f"n {n} L {L} {where}", **where)
            check_tone(ctx, x, Y, w, 2.0, LEVELS, 2.5, 6.0, kind, f"n {n} L {L} {where}", **where)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 4, 16])
def test_identity_knots_reproduce_detail_combine(ctx, L):
    n = 4099
    x, Y = planes(n, L, 77 + L)
    w = list(np.linspace(2.0, 1.0, L))
    for a, sigma in ((1.0, 0.0), (2.5, 6.0)):
        y = rule(x, Y, w, 1.5, a, sigma)
        frac = np.abs(y - np.floor(y) - 0.5)
        assert np.min(frac) > 1e-9                         # no .5 tie, and none that a few fp64 ulp of 255 could make
        tx, tY, _ = dev_planes(ctx, x, Y)
        for kind in KINDS:
            det = ctx.detail_combine(tx, tY, w, 1.5, a, sigma, kind).cpu().numpy()
            ton = ctx.tone_combine(tx, tY, w, IDENTITY, 1.5, a, sigma, kind).cpu().numpy()
            if kind == F32:
                assert np.all(np.abs(ton.astype(np.float64) - det.astype(np.float64)) <= np.spacing(np.abs(det)).astype(np.float64))
            else:
                assert np.array_equal(ton, det)


def raw_tone(nle, ctx, x, Y, L, n, stride, w, w_rho, a, sigma, curve, kind, out):
    ctx._sync_in()
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    wp = np.ascontiguousarray(w, dtype=np.float64).ctypes.data_as(C.c_void_p) if w is not None else None
    cp = np.ascontiguousarray(curve, dtype=np.float64).ctypes.data_as(C.c_void_p) if curve is not None else None
    return nle.lib().nle_tone_combine(ctx._h, P(x), P(Y), L, n, stride, wp, w_rho, a, sigma, cp, kind, P(out))


@pytest.mark.gpu
def test_tone_combine_refusals_leave_the_ctx_usable(nle, ctx):
    n, L = 1000, 4
    x, Y = planes(n, L, 9)
    tx, tY, out = dev_planes(ctx, x, Y)
    w = [3.0, 3.0, 1.0, 1.0]
    want = store(tone_rule(x, Y, w, 3.0, LEVELS), F32)
    nan, inf = float("nan"), float("inf")

    def bent(i, v):
        c = LEVELS.copy()
        c[i] = v
        return c
    bad = [(lambda: raw_tone(nle, ctx, tx, tY, L, n, n, w, 3.0, 1.0, 0.0, None, F32, out), "NULL"),
           (lambda: raw_tone(nle, ctx, None, tY, L, n, n, w, 3.0, 1.0, 0.0, LEVELS, F32, out), "NULL"),
           (lambda: raw_tone(nle, ctx, tx, tY, L, n, n, w, 3.0, 1.0, 0.0, bent(0, nan), F32, out), "range"),
           (lambda: raw_tone(nle, ctx, tx, tY, L, n, n, w, 3.0, 1.0, 0.0, bent(1, inf), F32, out), "range"),
           (lambda: raw_tone(nle, ctx, tx, tY, L, n, n, w, 3.0, 1.0, 0.0, bent(1, 13.0), F32, out), "range"),
           (lambda: raw_tone(nle, ctx, tx, tY, L, n, n, w, 3.0, 1.0, 0.0, bent(1, 12.0), F32, out), "range"),
           (lambda: raw_tone(nle, ctx, tx, tY, L, n, n, w, 3.0, 1.0, 0.0, bent(2 + 500, nan), F32, out), "knot 500"),
           (lambda: raw_tone(nle, ctx, tx, tY, L, n, n, w, 3.0, 1.0, 0.0, bent(2 + N, inf), F32, out), "knot 1024"),
           (lambda: raw_tone(nle, ctx, tx, tY, 17, n, n, [1.0] * 17, 3.0, 1.0, 0.0, LEVELS, F32, out), "layers"),
           (lambda: raw_tone(nle, ctx, tx, tY, L, n, n, w, 3.0, 3.5, 6.0, LEVELS, F32, out), "gain"),
           (lambda: raw_tone(nle, ctx, tx, tY, L, n, n, w, 3.0, 1.0, 0.0, LEVELS, 3, out), "kind"),
           (lambda: raw_tone(nle, ctx, tx, tY, L, 0, n, w, 3.0, 1.0, 0.0, LEVELS, F32, out), "n must be"),
           (lambda: raw_tone(nle, ctx, tx, tY, L, n, n - 1, w, 3.0, 1.0, 0.0, LEVELS, F32, out), "stride"),
           (lambda: raw_tone(nle, ctx, tx, tY, L, n, n, w, 3.0, 1.0, 0.0, LEVELS, F32, tx), "overlaps")]
    for k, (call, word) in enumerate(bad):
        assert call() == nle.NLE_ERR_INVALID, k
        msg = nle.lib().nle_last_error(ctx._h).decode()
        assert msg.startswith("nle_tone_combine") and word in msg, (k, msg)
        out.fill_(nan)
        assert raw_tone(nle, ctx, tx, tY, L, n, n, w, 3.0, 1.0, 0.0, LEVELS, F32, out) == nle.NLE_OK
        assert np.array_equal(out[:n].cpu().numpy(), want), k
    with pytest.raises(nle.NLEError):
        ctx.tone_combine(tx, tY, w, LEVELS[:-1], 3.0)


# ------------------------------------------------------------------------------------------------ GPU: through a trained filter
W4 = [3.0, 3.0, 1.0, 0.9]
TONES = [dict(shadows=0.8), dict(highlights=-0.6), dict(clip_percent=1.0), dict(equalise=0.5),
         dict(shadows=0.5, highlights=-0.3, clip_percent=1.0, equalise=0.5)]


@pytest.fixture(scope="module")
def scene(nle, ctx):
    import torch
    x = scene48().astype(np.float32)
    f = train_scene(nle, ctx, x)
    tx = torch.as_tensor(x, device=f"cuda:{ctx.device}")
    Y = f.apply_layers(tx, NL)
    yield x, tx, f, Y
    f.close()


def compose(nle, ctx, tx, Y, w, w_rho, a, sigma, kind, shadows=0.0, highlights=0.0, clip_percent=-1.0, equalise=0.0):
    """the four stage calls; returns (out, curve)"""
    counts = ctx.plane_histogram(Y[len(w) - 1], w[-1]) if clip_percent >= 0 or equalise > 0 else None
    curve = nle.tone_curve(counts, shadows, highlights, clip_percent, equalise)
    return ctx.tone_combine(tx.reshape(-1), Y, w, curve, w_rho, a, sigma, kind), curve


@pytest.mark.gpu
def test_apply_tone_is_the_four_stage_calls(nle, ctx, scene):
    import torch
    x, tx, f, Y = scene
    seen = set()
    for tone in TONES:
        for kind in KINDS:
            for a, sigma, w_rho in ((1.0, 0.0, 0.0), (2.5, 6.0, 2.0)):
                one, c1 = f.apply_tone(tx, W4, w_rho, a, sigma, out_kind=kind, want_curve=True, **tone)
                two, c2 = compose(nle, ctx, tx, Y, W4, w_rho, a, sigma, kind, **tone)
                assert one.dtype == two.dtype and torch.equal(one, two), (tone, kind, a)
                assert np.array_equal(c1, c2)
                seen.add(one.cpu().numpy().tobytes())
        # the levels and the knots are numpy's for the device's own base layer
        base = Y[NL - 1].cpu().numpy()
        want = np_curve(np_hist(base, W4[-1]), tone.get("shadows", 0), tone.get("highlights", 0), tone.get("clip_percent", -1), tone.get("equalise", 0))
        assert c1[0] == want[0] and c1[1] == want[1] and np.max(np.abs(c1[2:] - want[2:])) <= 1e-12 * 255
    assert len(seen) == len(TONES) * 3 * 2
    # everything inactive: nle_apply_detail
    for kind in KINDS:
        for a, sigma, w_rho in ((1.0, 0.0, 0.0), (2.5, 6.0, 2.0)):
            one, c = f.apply_tone(tx, W4, w_rho, a, sigma, out_kind=kind, want_curve=True)
            assert torch.equal(one, f.apply_detail(tx, W4, w_rho, a, sigma, kind)) and np.array_equal(c, IDENTITY)
    for bad in (dict(shadows=1.5), dict(highlights=float("nan")), dict(clip_percent=26.0), dict(equalise=-0.5)):
        with pytest.raises(nle.NLEError, match="nle_tone_curve"):
            f.apply_tone(tx, W4, **bad)
    with pytest.raises(nle.NLEError):
        f.apply_tone(tx[:-1], W4, shadows=0.5)             # H W that is not the filter's
    with pytest.raises(nle.NLEError):
        f.apply_tone(tx, [1.0] * 17, shadows=0.5)


@pytest.mark.gpu
def test_shadows_move_the_base_and_leave_the_detail(nle, ctx, scene):
    """y_tone - y_detail = B' - w Y_{L-1}: two fp32 stores, each within half an fp32 ulp of its fp64 value"""
    x, tx, f, Y = scene
    yt = f.apply_tone(tx, W4, 2.0, 2.5, 6.0, shadows=0.8).cpu().numpy().astype(np.float64)
    yd = f.apply_detail(tx, W4, 2.0, 2.5, 6.0).cpu().numpy().astype(np.float64)
    Bw = W4[-1] * Y[NL - 1].cpu().numpy().astype(np.float64)
    lift = np_base(Bw, np_curve(None, 0.8)) - Bw
    assert np.max(lift) > 15                                        # the dark half is lifted by many levels
    half_ulps = 0.5 * (np.spacing(np.abs(yt).astype(np.float32)) + np.spacing(np.abs(yd).astype(np.float32))).astype(np.float64)
    assert np.all(np.abs((yt - yd) - lift) <= half_ulps + 1e-10)


def run_cli(lead, src, out, weights):
    r = subprocess.run([ENHANCE] + lead + [str(src), str(out)] + SCENE_ARGV + [repr(float(w)) for w in weights], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-1500:])
    return r.stdout


def tone_line(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("Tone curve:")]
    assert len(lines) == 1, stdout
    m = re.fullmatch(r"Tone curve: levels (\S+) (\S+)", lines[0])
    return float(m.group(1)), float(m.group(2))


CLI_TONE = ["--shadows", "0.5", "--auto-levels", "1", "--equalise", "0.5"]
KW_TONE = dict(shadows=0.5, clip_percent=1.0, equalise=0.5)


@pytest.mark.gpu
def test_cli_8_bit_equals_the_python_composition(nle, ctx, tmp_path):
    from PIL import Image
    bgr = colour_scene()
    src = tmp_path / "in.bmp"
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(src)
    stdout = run_cli(CLI_TONE + ["--residual-weight", "1"], src, tmp_path / "o.png", W4)
    lab, L = ctx.bgr2lab8(bgr)
    f = train_scene(nle, ctx, L)
    Y = f.apply_layers(L, NL)
    y, curve = compose(nle, ctx, L, Y, W4, 1.0, 1.0, 0.0, ROUNDED8, **KW_TONE)
    want = ctx.lab2bgr8(lab, L=y.reshape(L.shape)).cpu().numpy()
    plain = ctx.lab2bgr8(lab, L=f.apply_rounded8(L, nle.transform_eigenvalues(f.eigvals, W4)).reshape(L.shape)).cpu().numpy()
    f.close()
    assert np.array_equal(read_rgb8(tmp_path / "o.png")[..., ::-1], want) and not np.array_equal(want, plain)
    assert tone_line(stdout) == (curve[0], curve[1]) == tuple(np_curve(np_hist(Y[NL - 1].cpu().numpy(), W4[-1]), 0.5, 0, 1.0, 0.5)[:2])
    assert (curve[0], curve[1]) != (0.0, 255.0)
    # without the options, and with inactive ones: the bytes the tool wrote before, and no line
    out = run_cli([], src, tmp_path / "plain.png", W4)
    assert "Tone curve" not in out and np.array_equal(read_rgb8(tmp_path / "plain.png")[..., ::-1], plain)
    run_cli(["--shadows", "0", "--highlights", "-0"], src, tmp_path / "inactive.png", W4)
    assert (tmp_path / "inactive.png").read_bytes() == (tmp_path / "plain.png").read_bytes()


@pytest.mark.gpu
def test_cli_deep_equals_the_python_composition(nle, ctx, tmp_path):
    from test_deep_colour import gradient16
    from test_image_io16 import png_bytes, read_png16_rgb
    bgr = gradient16(48, 64, 5)
    src = tmp_path / "in.png"
    src.write_bytes(png_bytes(bgr[..., ::-1], filt=1))
    stdout = run_cli(["--deep"] + CLI_TONE, src, tmp_path / "o.png", W4)
    L, a, b, g = ctx.bgr16_to_lab(bgr)
    f = train_scene(nle, ctx, g)
    Y = f.apply_layers(L, NL)
    y, curve = compose(nle, ctx, L, Y, W4, 0.0, 1.0, 0.0, F32, **KW_TONE)                     # on the unrounded L
    want = ctx.lab_to_bgr16(y.reshape(L.shape), a, b).cpu().numpy()
    plain = ctx.lab_to_bgr16(f.apply(L, nle.transform_eigenvalues(f.eigvals, W4)).reshape(L.shape), a, b).cpu().numpy()
    f.close()
    assert np.array_equal(read_png16_rgb(tmp_path / "o.png")[..., ::-1], want) and not np.array_equal(want, plain)
    assert tone_line(stdout) == (curve[0], curve[1])


@pytest.mark.gpu
def test_a_ctx_that_ran_tone_calls_trains_and_enhances_like_a_fresh_one(nle, ctx, scene):
    x, tx, f, Y = scene
    f.apply_tone(tx, W4, 1.0, 2.0, 5.0, **KW_TONE)
    ctx.plane_histogram(Y[0], 2.0)
    resp = None
    outs = []
    fresh = nle.Context(0)
    try:
        for c in (ctx, fresh):
            g = train_scene(nle, c, x)
            resp = nle.transform_eigenvalues(g.eigvals, W4)
            outs.append((np.array(g.eigvals), g.apply_rounded8(x, resp).cpu().numpy()))
            g.close()
    finally:
        fresh.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------------------------------------ GPU: the C++ surface
DRIVER = textwrap.dedent(r"""
    #include <cstdio>
    #include <cstring>
    #include <stdexcept>
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
        const std::vector<double> w = {3, 3, 1, 0.9};
        nle::NLEFilter f;
        f.verbose = false;
        f.trainForEnhancement(im, 6, 8, 30, 30, 10, 8);
        nle::DetailOptions detail;
        detail.residualWeight = 1;
        nle::ToneOptions on, off;
        on.shadows = 0.5, on.clipPercent = 1, on.equalise = 0.5;
        REQUIRE(on.active() && !off.active());
        if (std::string(argv[3]) == "group") {      // trained over a device group: active options are refused by name
            try {
                f.enhance(im, w, detail, on);
                REQUIRE(false);
            } catch (const std::runtime_error& e) {
                REQUIRE(std::string(e.what()).find("ToneOptions") != std::string::npos);
            }
            REQUIRE(same(f.enhance(im, w, nle::DetailOptions(), off), f.enhance(im, w)));   // inactive ones are the plain method
            std::printf("group OK\n");
            return 0;
        }
        REQUIRE(!f.lastToneCurve().valid);
        REQUIRE(same(f.enhance(im, w, detail, off), f.enhance(im, w, detail)) && !f.lastToneCurve().valid);
        off.equalise = 0, off.clipPercent = -5;
        REQUIRE(!off.active() && same(f.enhance(im, w, nle::DetailOptions(), off), f.enhance(im, w)));
        const nle::Image out = f.enhance(im, w, detail, on);
        REQUIRE(!same(out, f.enhance(im, w, detail)) && nle::imwrite(argv[2], out));
        const nle::ToneLevels lv = f.lastToneCurve();
        REQUIRE(lv.valid && lv.hi - lv.lo >= 1 && !(lv.lo == 0 && lv.hi == 255));
        std::printf("levels %.17g %.17g\n", lv.lo, lv.hi);
        nle::ToneOptions bad = on;
        bad.shadows = 1.5;
        bool threw = false;
        try { f.enhance(im, w, detail, bad); } catch (const std::runtime_error&) { threw = true; }
        REQUIRE(threw);
        threw = false;
        try { f.enhance(im, std::vector<double>(17, 1.0), detail, on); } catch (const std::runtime_error&) { threw = true; }
        REQUIRE(threw);
        REQUIRE(same(f.enhance(im, w, detail, on), out));
        std::printf("tone OK\n");
        return 0;
    }
""")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("tonedrv")
    host, libdir = os.path.join(PKG_DIR, "host"), os.path.join(PKG_DIR, "lib")
    (d / "drv.cpp").write_text(DRIVER)
    b = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(d / "drv.cpp"),
                        *[os.path.join(host, s) for s in ("filter.cpp", "stages.cpp", "colour.cpp", "device_group.cpp", "image_io.cpp", "jpeg.cpp")],
                        "-L", libdir, "-lnle_hip", "-Wl,-rpath," + libdir, "-o", str(d / "drv")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    return str(d / "drv")


@pytest.fixture(scope="module")
def bmp(tmp_path_factory):
    from PIL import Image
    path = tmp_path_factory.mktemp("tone8") / "in.bmp"
    Image.fromarray(np.ascontiguousarray(colour_scene()[..., ::-1])).save(path)
    return path


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_cpp_surface_equals_the_cli_and_inactive_options_are_the_existing_method(driver, bmp, tmp_path):
    env = {k: v for k, v in os.environ.items() if k != "NLE_DEVICES"}
    r = subprocess.run([driver, str(bmp), str(tmp_path / "drv.png"), "one"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "tone OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    stdout = run_cli(CLI_TONE + ["--residual-weight", "1"], bmp, tmp_path / "cli.png", W4)
    assert np.array_equal(read_rgb8(tmp_path / "drv.png"), read_rgb8(tmp_path / "cli.png"))
    lo, hi = [float(v) for v in re.search(r"^levels (\S+) (\S+)$", r.stdout, flags=re.M).groups()]
    assert tone_line(stdout) == (lo, hi)


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_a_group_trained_filter_is_refused(driver, bmp, tmp_path):
    """NLE_DEVICES with the same device twice forms a group: the train shards the image, enhance with active options throws"""
    r = subprocess.run([driver, str(bmp), str(tmp_path / "drv.png"), "group"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, NLE_DEVICES="0,0"))
    assert r.returncode == 0 and "group OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
