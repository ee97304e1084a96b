"""HDR tone mapping: linear-light float BGR -> log-luminance on the scale of an 8-bit L plane ->
train on its 256-level guide, apply to the unrounded plane -> 16-bit sRGB.  There is no reference for it, so the definition
(include/nle.h at nle_hdr_range) is restated here in numpy -- in longdouble as the yardstick of the forward kernel, in fp64
for the range pass and the inverse -- and the tests hold the kernels, the Python mirror, the C++ surface and
`enhance --tonemap` to it.

Bounds.  Range: l_hi and R are two host logarithms of values the device finds exactly (max and min select, they do not
round): 1e-14 relative.  Forward: x is the fp32 rounding of an fp64 value whose absolute error is a few 1e-14 / R, so it is
within one fp32 ulp of the longdouble restatement and differs from it at all only where the longdouble value lies within
2^-40 relative of an fp32 rounding boundary; the guide differs only where the longdouble x lies within 1e-9 of a half-integer;
both kinds are counted, at most 1 pixel in 1e5, by one ulp and one level.  (x = 255 t + 255 cancels near x = 0: an
admissible pixel within ~1e-6 stops above the floor has no relative accuracy in any fp64 evaluation.  The kernel tests pass
scales of their own, as the entry points allow, and test_the_seeds_keep_the_restatements_own_near_ties_inside_the_cap checks
on the CPU that the fp64 restatement of the same inputs stays inside the cap; pixels AT the floor are exactly 0.)  Inverse:
codes equal searchsorted on the library's thr over the fp64 restatement except where a value is within 1e-12 relative of
a threshold (fp64 error, pow and exp2 included, is ~1e-16); those are counted (< 1 in 1e5) and may differ by one code."""
import os
import shutil
import subprocess
import textwrap

import numpy as np
import pytest

from conftest import GOLDEN, PKG_DIR, ROOT, rel_l2
from test_image_io16 import read_png16_rgb
from test_image_io_hdr import decode_rgbe, pfm, radiance

ENHANCE = os.path.join(PKG_DIR, "bin", "enhance")
DENOISE = os.path.join(PKG_DIR, "bin", "denoise")
GRID_CAP_PIXELS = 2048 * 256 * 2  # the launchers' grid cap times their block size times two pixels per thread: beyond it the
                                  # stride loop runs (in the single-pixel form, which unaligned pointers take, from half of it)
CAP = 1e-5                        # the share of pixels a waiver may cover


# ------------------------------------------------------------------------------------------------ the restatement
def lum(bgr, dt=np.float64):
    B, G, R = (bgr[..., k].astype(dt) for k in range(3))
    with np.errstate(invalid="ignore"):
        return (dt(0.212671) * R + dt(0.715160) * G) + dt(0.072169) * B


def hdr_range(bgr):
    """(l_hi, R) in fp64, or None when no pixel has a finite luminance > 0"""
    Y = lum(bgr)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(Y) & (Y > 0)
    if not ok.any():
        return None
    l_hi = np.log2(Y[ok].max())
    l_lo = max(np.log2(Y[ok].min()), l_hi - 24.0)
    R = l_hi - l_lo
    return float(l_hi), float(1.0 if R < 2.0 ** -20 else R)


def forward(bgr, l_hi, R, dt=np.float64):
    """x unrounded in dtype dt: 255 ((log2 Y - l_hi) / R) + 255 clamped into [0, 255]; Y <= 0, -inf and NaN give 0, +inf 255"""
    Y = lum(bgr, dt)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        pos = Y > 0
        x = dt(255.0) * ((np.log2(np.where(pos, Y, dt(1.0))) - dt(l_hi)) / dt(R)) + dt(255.0)
        return np.where(pos, np.clip(x, dt(0.0), dt(255.0)), dt(0.0))


def guide_of(x):
    return np.rint(x).astype(np.float32)


def inverse_linear(y, bgr, l_hi, R, c, s, dt=np.float64):
    """(..., 3) linear B, G, R out of the filtered plane y and the original colours, operation by operation"""
    y = np.asarray(y).astype(dt)
    Y = lum(bgr, dt)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        Yout = np.where(np.isnan(y), dt(0.0), np.exp2(((np.where(np.isnan(y), dt(0.0), y) - dt(255.0) * dt(c)) * dt(R)) / dt(255.0)))
        y_lo, y_hi = np.exp2(np.float64(l_hi) - np.float64(R)).astype(dt), np.exp2(np.float64(l_hi)).astype(dt)
        Yin = np.where(Y > y_lo, np.where(Y < y_hi, Y, y_hi), y_lo)
        C = bgr.astype(dt)
        r = np.where(C > 0, C, dt(0.0)) / Yin[..., None]
        return (r if s == 1 else np.power(r, dt(s))) * Yout[..., None]


def code_of(v, thr):
    """(number of c with thr[c] <= v) - 1, a NaN gives 0"""
    c = np.searchsorted(thr, v.astype(np.float64), side="right") - 1
    c[np.isnan(v)] = 0
    return c.astype(np.uint16)


def pixels(n, seed, stops=20.0, junk=True):
    """n linear-light BGR pixels whose channels span `stops` stops below 8.0, sprinkled (about 1 in 50) with NaN, +-inf, zeros
    and negatives in single channels and in whole pixels"""
    rng = np.random.default_rng(seed)
    bgr = (8.0 * np.exp2(-stops * rng.random((n, 3)))).astype(np.float32)
    if junk and n >= 50:
        bad = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.5, -1e-30], dtype=np.float32)
        i = rng.choice(n, n // 50, replace=False)
        bgr[i, rng.integers(0, 3, i.size)] = bad[rng.integers(0, bad.size, i.size)]
        j = rng.choice(n, n // 200 + 1, replace=False)
        bgr[j] = bad[rng.integers(0, bad.size, j.size)][:, None]
    return bgr


def near_fp32_boundary(x_ld, rel=2.0 ** -40):
    """where a longdouble value lies within `rel` relative of the midpoint of two neighbouring fp32 values"""
    f = x_ld.astype(np.float32)
    up = (f.astype(np.longdouble) + np.nextafter(f, np.float32(np.inf)).astype(np.longdouble)) / 2
    dn = (f.astype(np.longdouble) + np.nextafter(f, np.float32(-np.inf)).astype(np.longdouble)) / 2
    return np.minimum(np.abs(x_ld - up), np.abs(x_ld - dn)) <= rel * np.abs(x_ld)


def near_half(x_ld, eps=1e-9):
    return np.abs((x_ld - np.floor(x_ld)) - np.longdouble(0.5)) <= eps


N_ALL = GRID_CAP_PIXELS + 77
SEED = 31


def scales(bgr):
    """the two scales the kernel tests pass: the data's own top with the full 24 stops below it (nothing clamps but the
    sprinkled pixels), and a window of 12 stops that starts 1.5 stops below the top (both ends clamp)"""
    l_hi, _ = hdr_range(bgr)
    return {"wide": (l_hi, 24.0), "window": (l_hi - 1.5, 12.0)}


@pytest.fixture(scope="module")
def sets():
    """N_ALL pixels and, per scale, the longdouble x and what is stored of it"""
    bgr = pixels(N_ALL, SEED)
    out = {"bgr": bgr, "scales": scales(bgr)}
    for name, (l_hi, R) in out["scales"].items():
        x = forward(bgr, l_hi, R, np.longdouble)
        out[name] = {"ld": x, "x": x.astype(np.float32), "guide": guide_of(x)}
    for v in (out["bgr"],) + tuple(a for k in out["scales"] for a in out[k].values()):
        v.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def tab(nle):
    return nle.srgb16_tables()


# ------------------------------------------------------------------------------------------------ CPU: the definition
def test_restatement_range_scale_and_guide():
    bgr = pixels(1 << 18, 3)
    l_hi, R = hdr_range(bgr)
    Y = lum(bgr)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(Y) & (Y > 0)
    assert 18 < R <= 24 and l_hi == np.log2(Y[ok].max())
    x = forward(bgr, l_hi, R, np.longdouble)
    xf = x.astype(np.float32)
    assert np.all((x >= 0) & (x <= 255)) and np.all((xf >= 0) & (xf <= 255))
    assert xf[ok][np.argmax(Y[ok])] == 255.0 and xf.max() == 255.0                 # the brightest pixel is exactly 255
    g = guide_of(x)
    assert np.array_equal(g, np.rint(g)) and g.min() >= 0 and g.max() == 255 and np.max(np.abs(g - xf)) <= 0.5 + 1e-4
    # the floor: NaN, -inf, zeros and negatives are exactly 0; +inf is the ceiling
    with np.errstate(invalid="ignore"):
        assert np.all(xf[np.isnan(Y) | (Y <= 0)] == 0.0) and np.all(xf[Y == np.inf] == 255.0) and np.any(Y == np.inf)


def test_restatement_flat_image_and_the_24_stop_floor():
    flat = np.tile(np.array([[0.3, 0.2, 0.1]], dtype=np.float32), (1000, 1))
    l_hi, R = hdr_range(flat)
    assert R == 1.0 and np.all(forward(flat, l_hi, R, np.longdouble).astype(np.float32) == 255.0)
    deep = flat.copy()
    deep[:10] *= np.float32(2.0 ** -30)                        # 30 stops down: below the floor, which stays at 24
    deep[10:20] *= np.float32(2.0 ** -12)
    l_hi2, R2 = hdr_range(deep)
    x = forward(deep, l_hi2, R2, np.longdouble).astype(np.float32)
    assert l_hi2 == l_hi and R2 == 24.0 and np.all(x[:10] == 0.0) and np.all(x[10:20] == np.float32(127.5)) and np.all(x[20:] == 255.0)
    junk = np.array([[np.nan, 1, 1], [-1, -1, -1], [0, 0, 0], [np.inf, 1, 1], [np.inf, -np.inf, 1]], dtype=np.float32)
    assert hdr_range(junk) is None                              # nothing finite and positive: the call is refused


def test_restatement_forward_then_inverse_is_the_encoding_of_c_over_ymax(tab):
    """y = x (unrounded, in longdouble: this is the definition's own consistency, not the storage's), c = 1, s = 1: every
    channel comes back as the 16-bit code of C / Ymax, zero differing samples on 2^20 triples that span 20 stops"""
    bgr = pixels(1 << 20, 7, junk=False)
    l_hi, R = hdr_range(bgr)
    ld = np.longdouble
    x = forward(bgr, l_hi, R, ld)
    back = code_of(inverse_linear(x, bgr, l_hi, R, 1.0, 1.0, ld), tab[1])
    want = code_of(bgr.astype(ld) / lum(bgr).max().astype(ld), tab[1])
    assert np.count_nonzero(back != want) == 0
    assert len(np.unique(want)) > 30000 and want.max() > 60000       # the codes are spread over the whole scale


def test_the_seeds_keep_the_restatements_own_near_ties_inside_the_cap(sets):
    """what the GPU tests waive must be rare on their inputs to begin with: the fp64 restatement of the same pixels against the
    longdouble one, and the longdouble one's own near ties"""
    bgr, n = sets["bgr"], len(sets["bgr"])
    for name, (l_hi, R) in sets["scales"].items():
        ld, want = sets[name]["ld"], sets[name]["x"]
        x64 = forward(bgr, l_hi, R)
        got = x64.astype(np.float32)
        differ = got != want
        print(name, "fp64 against longdouble:", int(differ.sum()), "differ; near an fp32 boundary:", int(near_fp32_boundary(ld).sum()),
              "near a half:", int(near_half(ld).sum()))
        assert not np.any(differ & ~near_fp32_boundary(ld)) and differ.sum() <= n * CAP
        assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))
        # (the 2^-40 window itself holds about 2 pixels in 1e5, whatever the seed: 2^-39 of an fp32 ulp of ~2^-23.5 relative;
        # what is capped is what a waiver is used for, the pixels that differ)
        assert near_half(ld).sum() <= n * CAP
        gd = guide_of(x64) != sets[name]["guide"]
        assert not np.any(gd & ~near_half(ld))
        assert 0.001 < np.mean(want == 0.0) and (name == "wide" or np.mean(want == 255.0) > 0.01)     # the clamps are exercised


# ------------------------------------------------------------------------------------------------ CPU: the CLI's refusals
ARGV = ["6", "8", "16", "30", "10", "8"]
W4 = ["2", "2", "1", "0.4"]


@pytest.mark.parametrize("exe,argv", [
    (ENHANCE, ["--tonemap=1", "missing.hdr", "o.png"] + ARGV + W4),
    (ENHANCE, ["--tonemap-saturation", "0.6", "missing.hdr", "o.png"] + ARGV + W4),
    (ENHANCE, ["--tonemap", "--tonemap-saturation", "0", "missing.hdr", "o.png"] + ARGV + W4),
    (ENHANCE, ["--tonemap-saturation", "2.5", "--tonemap", "missing.hdr", "o.png"] + ARGV + W4),
    (ENHANCE, ["--tonemap", "--tonemap-saturation", "nan", "missing.hdr", "o.png"] + ARGV + W4),
    (ENHANCE, ["--tonemap", "--tonemap-saturation", "inf", "missing.hdr", "o.png"] + ARGV + W4),
    (ENHANCE, ["--tonemap", "--tonemap-saturation", "1x", "missing.hdr", "o.png"] + ARGV + W4),
    (ENHANCE, ["--tonemap", "--tonemap-saturation"]),
    (ENHANCE, ["--tonemap", "--chroma", "20", "missing.hdr", "o.png"] + ARGV + W4),
    (ENHANCE, ["--region", "mask.png:1,1,1,1", "--tonemap", "missing.hdr", "o.png"] + ARGV + W4),
    (ENHANCE, ["--deep", "--tonemap", "missing.hdr", "o.png"] + ARGV + W4),
    (ENHANCE, ["--tonemap", "--nystrom-report", "missing.hdr", "o.png"] + ARGV + W4),
    (ENHANCE, ["--exact", "--tonemap", "missing.hdr", "o.bmp"] + ARGV + W4),
    (ENHANCE, ["--tonemap", "missing.hdr", "png"] + ARGV + W4),
    (DENOISE, ["--tonemap", "missing.hdr", "o.png"] + ARGV + ["10", "10", "2"]),
    (DENOISE, ["--tonemap-saturation", "1", "missing.hdr", "o.png"] + ARGV + ["10", "10", "2"]),
], ids=["value", "saturation-alone", "saturation-zero", "saturation-above-2", "saturation-nan", "saturation-inf", "saturation-garbage",
        "saturation-without-value", "chroma", "region", "deep", "nystrom-report", "not-png", "no-extension", "denoise",
        "denoise-saturation"])
def test_cli_refuses_before_anything_runs(tmp_path, exe, argv):
    """status 2 and one line on stderr; the input does not even exist, so nothing was read and no GPU call was made"""
    r = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert len(r.stderr.strip().splitlines()) == 1 and "--tonemap" in r.stderr and r.stdout == ""
    assert not os.listdir(tmp_path)


def test_cli_unreadable_input_is_the_soft_failure_it_was(tmp_path):
    """a file no HDR reader takes: the empty image, a message, exit 0, nothing written -- as the reference does for any input"""
    (tmp_path / "not.hdr").write_bytes(b"#?RADIANCE\nFORMAT=32-bit_rle_xyze\n\n-Y 1 +X 1\n\0\0\0\0")
    for src in ("missing.hdr", "not.hdr"):
        r = subprocess.run([ENHANCE, "--tonemap", src, "o.png"] + ARGV + W4, capture_output=True, text=True, timeout=60, cwd=tmp_path)
        assert r.returncode == 0 and "Failed to read file from " + src in r.stderr and r.stdout == ""
    assert os.listdir(tmp_path) == ["not.hdr"]


def test_the_entry_points_are_exported(nle):
    for name in ("nle_hdr_range", "nle_hdr_to_loglum", "nle_loglum_to_bgr16"):
        assert name in nle.EXPORTED_SYMBOLS and hasattr(nle.lib(), name)
    for name in ("hdr_range", "hdr_to_loglum", "loglum_to_bgr16"):
        assert callable(getattr(nle.Context, name))


# ------------------------------------------------------------------------------------------------ GPU: the range pass
SIZES = [1, 255, 257, 37 * 53, N_ALL]


@pytest.fixture(scope="module")
def dev_bgr(ctx, sets):
    import torch
    return torch.from_numpy(sets["bgr"].copy()).to(f"cuda:{ctx.device}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES + [1001, 2048 * 256 + 1001])
def test_range_against_numpy(ctx, sets, dev_bgr, n):
    """every size, and from a pointer that is only 4-byte aligned (one pixel in): the single-pixel form"""
    for off in (0, 1):
        if off + n > N_ALL:
            continue
        want = hdr_range(sets["bgr"][off:off + n])
        t = dev_bgr[off:off + n]
        assert t.data_ptr() % 8 == (4 if off else 0)
        if want is None:
            with pytest.raises(Exception):
                ctx.hdr_range(t)
            continue
        l_hi, R = ctx.hdr_range(t)
        print(n, off, "l_hi", l_hi, want[0], "R", R, want[1])
        assert abs(l_hi - want[0]) <= 1e-14 * abs(want[0]) and abs(R - want[1]) <= 1e-14 * want[1]


@pytest.mark.gpu
def test_range_of_a_flat_plane_and_of_nothing_admissible(nle, ctx, dev_bgr):
    import torch
    flat = torch.full((37 * 53, 3), 0.25, device=dev_bgr.device)
    l_hi, R = ctx.hdr_range(flat)
    want = np.log2((0.212671 * 0.25 + 0.715160 * 0.25) + 0.072169 * 0.25)
    assert R == 1.0 and abs(l_hi - want) <= 1e-14 * abs(want)
    flat[5] = float("nan")
    flat[6] = float("inf")
    flat[7] = -3.0
    flat[8] = 0.0
    assert ctx.hdr_range(flat) == (l_hi, 1.0)
    bad = torch.tensor([[float("nan"), 1, 1], [-1, -1, -1], [0, 0, 0], [float("inf"), 1, 1], [float("inf"), float("-inf"), 1]],
                       device=dev_bgr.device).repeat(301, 1)
    with pytest.raises(nle.NLEError):
        ctx.hdr_range(bad)
    assert ctx.hdr_range(flat) == (l_hi, 1.0)                    # the ctx still works


# ------------------------------------------------------------------------------------------------ GPU: the forward kernel
@pytest.fixture(scope="module")
def dev(ctx, sets, dev_bgr):
    """the forward kernel's outputs on the whole set, per scale, on the device"""
    out = {}
    for name, (l_hi, R) in sets["scales"].items():
        x, g = ctx.hdr_to_loglum(dev_bgr, l_hi, R)
        out[name] = {"x": x, "guide": g}
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["wide", "window"])
def test_forward_kernel_against_the_longdouble_restatement(sets, dev, name):
    n = N_ALL
    ld, want = sets[name]["ld"], sets[name]["x"]
    got = dev[name]["x"].cpu().numpy()
    ulp = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    differ = got != want
    print(f"{name}: x {int(differ.sum())} of {n} differ, max {ulp.max():.1f} ulp")
    assert ulp.max() <= 1.0
    assert not np.any(differ & ~near_fp32_boundary(ld)), int(np.count_nonzero(differ & ~near_fp32_boundary(ld)))
    assert differ.sum() <= n * CAP
    gg, gw = dev[name]["guide"].cpu().numpy(), sets[name]["guide"]
    gd = gg != gw
    print(f"{name}: guide {int(gd.sum())} of {n} differ")
    assert not np.any(gd & ~near_half(ld)) and gd.sum() <= n * CAP and np.all(np.abs(gg - gw) <= 1.0)
    assert np.array_equal(gg, np.rint(gg)) and gg.min() >= 0 and gg.max() <= 255


def raw_forward(nle, ctx, bgr, n, l_hi, R, x, g):
    import ctypes as C
    ctx._sync_in()
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    return nle.lib().nle_hdr_to_loglum(ctx._h, P(bgr), n, C.c_double(l_hi), C.c_double(R), P(x), P(g))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_forward_shapes_and_optional_outputs(nle, ctx, sets, dev, dev_bgr, n):
    """every size against the full run's own first n values, bit for bit; x and guide NULL in every combination; outputs are
    prefilled with NaN and 64 elements longer: an element the kernel did not write, or wrote beyond n, shows"""
    import torch
    l_hi, R = sets["scales"]["window"]
    for mask in (1, 2, 3):
        outs = [torch.full((n + 64,), float("nan"), device=dev_bgr.device) for _ in range(2)]
        given = [outs[j] if mask >> j & 1 else None for j in range(2)]
        assert raw_forward(nle, ctx, dev_bgr[:n], n, l_hi, R, *given) == nle.NLE_OK
        for j, k in enumerate(("x", "guide")):
            assert bool(torch.isnan(outs[j][n:]).all()), (k, mask)
            if given[j] is None:
                assert bool(torch.isnan(outs[j][:n]).all())
            else:
                assert torch.equal(outs[j][:n].view(torch.int32), dev["window"][k][:n].view(torch.int32)), (k, mask)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1001, 2048 * 256 + 1001], ids=["one-sweep", "stride-loop"])
def test_unaligned_pointers_take_the_single_pixel_form(nle, ctx, sets, dev, dev_bgr, tab, n):
    """the kernels take two pixels per thread where the image and the planes are 8-byte aligned; an image that starts one
    pixel in and planes that start one element in (4-byte aligned) give the same bits one pixel at a time, both directions"""
    import ctypes as C
    import torch
    d = dev_bgr.device
    l_hi, R = sets["scales"]["window"]
    bgr = dev_bgr[1:n + 1]
    outs = [torch.full((n + 65,), float("nan"), device=d)[1:] for _ in range(2)]
    assert bgr.data_ptr() % 8 == 4 and all(o.data_ptr() % 8 == 4 for o in outs)
    assert raw_forward(nle, ctx, bgr, n, l_hi, R, *outs) == nle.NLE_OK
    for o, k in zip(outs, ("x", "guide")):
        assert torch.equal(o[:n].view(torch.int32), dev["window"][k][1:n + 1].view(torch.int32)) and bool(torch.isnan(o[n:]).all()), k
    # the inverse from the same unaligned planes into an output that starts one pixel in (2 bytes past 4-byte alignment)
    want = ctx.loglum_to_bgr16(dev["window"]["x"][1:n + 1].clone(), dev_bgr[1:n + 1].clone(), l_hi, R, 0.7, 1.0).cpu().numpy()
    back = torch.full((n + 2, 3), 7, dtype=torch.uint16, device=d)
    assert back[1:].data_ptr() % 4 == 2
    ctx._sync_in()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert nle.lib().nle_loglum_to_bgr16(ctx._h, P(outs[0]), P(bgr), n, C.c_double(l_hi), C.c_double(R), C.c_double(0.7), C.c_double(1.0),
                                         P(back[1:])) == nle.NLE_OK
    back = back.cpu().numpy()
    assert np.array_equal(back[1:n + 1], want) and np.all(back[0] == 7) and np.all(back[n + 1] == 7)


# ------------------------------------------------------------------------------------------------ GPU: the inverse kernel
def check_inverse(got, v, thr):
    """device codes against searchsorted on the fp64 restatement's values v; returns the number of samples near a threshold"""
    want = code_of(v, thr)
    with np.errstate(invalid="ignore"):
        lo, hi = thr[want], np.where(want == 65535, np.inf, thr[np.minimum(want.astype(np.int64) + 1, 65535)])
        near = ((np.abs(v - lo) <= 1e-12 * np.abs(v)) | (np.abs(v - hi) <= 1e-12 * np.abs(v))) & np.isfinite(v)   # inf saturates, exactly
    wrong = got != want
    assert not np.any(wrong & ~near), int(np.count_nonzero(wrong & ~near))
    assert np.all(np.abs(got.astype(np.int64) - want.astype(np.int64))[wrong] <= 1)
    return int(np.count_nonzero(near))


def inverse_inputs(sets, n, seed):
    """the first n pixels (NaN, infinite, zero and negative channels among them) and a plane y that leaves [0, 255] both ways
    and holds NaN and both infinities"""
    rng = np.random.default_rng(seed)
    y = rng.uniform(-20, 280, n).astype(np.float32)
    if n >= 100:
        y[rng.choice(n, n // 100, replace=False)] = np.float32("nan")
        y[:6] = [0.0, 255.0, np.inf, -np.inf, -1.0, 300.0]
    return y, sets["bgr"][:n]


@pytest.mark.gpu
@pytest.mark.parametrize("s", [1.0, 0.5, 2.0])
@pytest.mark.parametrize("c", [0.3, 1.0])
def test_inverse_kernel_against_the_restatement(ctx, sets, tab, s, c):
    n = 1 << 18
    l_hi, R = sets["scales"]["window"]
    y, bgr = inverse_inputs(sets, n, 41)
    got = ctx.loglum_to_bgr16(y, bgr, l_hi, R, c, s).cpu().numpy()
    v = inverse_linear(y, bgr, l_hi, R, c, s)
    near = check_inverse(got, v, tab[1])
    lo, hi = int(np.count_nonzero(got == 0)), int(np.count_nonzero(got == 65535))
    print(f"s = {s}, c = {c}: within 1e-12 of a threshold: {near}; saturated low / high: {lo} / {hi}")
    assert near < got.size * CAP
    assert lo > 1000 and hi > 1000                                # out of gamut both ways ran
    with np.errstate(invalid="ignore"):
        nan_c = np.isnan(bgr) | (bgr <= 0)
    assert np.all(got[np.isnan(y)] == 0) and np.all(got[nan_c] == 0)      # a NaN y is black; a NaN or negative channel is 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_inverse_shapes(nle, ctx, sets, dev_bgr, n):
    """every size against the full run's own first n pixels, into an over-long output whose tail stays untouched"""
    import ctypes as C
    import torch
    l_hi, R = sets["scales"]["wide"]
    y, _ = inverse_inputs(sets, N_ALL, 43)
    y = torch.from_numpy(y).to(dev_bgr.device)
    full = ctx.loglum_to_bgr16(y, dev_bgr, l_hi, R, 0.4, 0.8)
    out = torch.full((n + 16, 3), 9, dtype=torch.uint16, device=dev_bgr.device)
    ctx._sync_in()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert nle.lib().nle_loglum_to_bgr16(ctx._h, P(y), P(dev_bgr), n, C.c_double(l_hi), C.c_double(R), C.c_double(0.4), C.c_double(0.8),
                                         P(out)) == nle.NLE_OK
    assert torch.equal(out[:n].view(torch.int16), full[:n].view(torch.int16)) and bool((out[n:].view(torch.int16) == 9).all())


@pytest.mark.gpu
def test_refusals_leave_the_ctx_usable(nle, ctx, sets, dev, dev_bgr):
    import ctypes as C
    import torch
    d = dev_bgr.device
    n = 100
    l_hi, R = sets["scales"]["window"]
    x, g = torch.zeros(n, device=d), torch.zeros(n, device=d)
    out16 = torch.zeros((n, 3), dtype=torch.uint16, device=d)
    lib, P, D = nle.lib(), lambda t: C.c_void_p(t.data_ptr()), C.c_double  # noqa: E731
    nan, inf = float("nan"), float("inf")
    h = (C.c_double(), C.c_double())
    ctx._sync_in()

    def inverse(n=n, y=x, bgr=dev_bgr, l_hi=l_hi, R=R, c=0.4, s=1.0, out=out16):
        return lib.nle_loglum_to_bgr16(ctx._h, P(y) if y is not None else None, P(bgr) if bgr is not None else None, n, D(l_hi), D(R),
                                       D(c), D(s), P(out) if out is not None else None)
    bad = [lambda: raw_forward(nle, ctx, dev_bgr, -1, l_hi, R, x, g), lambda: raw_forward(nle, ctx, dev_bgr, n, l_hi, R, None, None),
           lambda: raw_forward(nle, ctx, None, n, l_hi, R, x, g)]
    bad += [lambda v=v: raw_forward(nle, ctx, dev_bgr, n, v, R, x, g) for v in (nan, inf, -inf)]
    bad += [lambda v=v: raw_forward(nle, ctx, dev_bgr, n, l_hi, v, x, g) for v in (nan, inf, 0.0, -1.0)]
    bad += [lambda: lib.nle_hdr_range(ctx._h, P(dev_bgr), -1, C.byref(h[0]), C.byref(h[1])),
            lambda: lib.nle_hdr_range(ctx._h, None, n, C.byref(h[0]), C.byref(h[1])),
            lambda: lib.nle_hdr_range(ctx._h, P(dev_bgr), n, None, C.byref(h[1]))]
    bad += [lambda: inverse(n=-1), lambda: inverse(y=None), lambda: inverse(bgr=None), lambda: inverse(out=None)]
    bad += [lambda v=v: inverse(l_hi=v) for v in (nan, inf)] + [lambda v=v: inverse(R=v) for v in (nan, inf, 0.0, -2.0)]
    bad += [lambda v=v: inverse(c=v) for v in (nan, inf, -inf)] + [lambda v=v: inverse(s=v) for v in (nan, inf, 0.0, -1.0, 2.0000001)]
    for i, call in enumerate(bad):
        assert call() == nle.NLE_ERR_INVALID, i
        assert lib.nle_last_error(ctx._h)
        assert raw_forward(nle, ctx, dev_bgr, n, l_hi, R, x, g) == nle.NLE_OK               # still usable
        assert torch.equal(x.view(torch.int32), dev["window"]["x"][:n].view(torch.int32))
        assert inverse(s=2.0) == nle.NLE_OK
    assert raw_forward(nle, ctx, dev_bgr, 0, l_hi, R, x, g) == nle.NLE_OK and inverse(n=0) == nle.NLE_OK     # n = 0: nothing to do
    with pytest.raises(nle.NLEError):
        ctx.loglum_to_bgr16(x[:50], dev_bgr[:n], l_hi, R, 1.0)
    with pytest.raises(nle.NLEError):
        ctx.hdr_range(torch.zeros((n, 3), dtype=torch.float64, device=d))


# ------------------------------------------------------------------------------------------------ GPU: end to end
ARGS = dict(nr=6, nc=8, hx=16.0, hy=30.0, T=10, K=8)
WEIGHTS = [2.0, 2.0, 1.0, 0.4]
STOPS = 10.0


def scene(H, W, seed):
    """two regions 10 stops apart (the left half dark, the right half bright), each with a tint of its own, times a smooth
    ramp of half a stop from top to bottom, times a texture of +-10 %; returns the float32 BGR image and the texture"""
    rng = np.random.default_rng(seed)
    rows, cols = np.mgrid[0:H, 0:W]
    bright = cols >= W // 2
    tint = np.where(bright[..., None], np.array([0.7, 0.9, 1.0]), np.array([1.0, 0.8, 0.6]))
    texture = 1.0 + 0.1 * rng.uniform(-1, 1, (H, W))
    level = np.where(bright, 1.0, 2.0 ** -STOPS) * np.exp2(0.5 * rows / H) * texture
    return (tint * level[..., None]).astype(np.float32), texture, bright


def to_rgbe(bgr):
    """(H, W, 4) uint8 R, G, B, E of a positive float image: the shared exponent of the largest channel, mantissas truncated"""
    rgb = bgr[..., ::-1].astype(np.float64)
    _, e = np.frexp(rgb.max(axis=2))
    m = np.floor(rgb * np.exp2(8.0 - e)[..., None])
    return np.concatenate([m, (e + 128)[..., None]], axis=2).astype(np.uint8)


def scene_files(d):
    """name -> (file, the float32 BGR image a reader makes of it, texture, bright): a PFM, which holds the floats themselves,
    and a run-length Radiance picture, which holds their RGBE roundings"""
    out = {}
    bgr, tex, bright = scene(48, 64, 5)
    (d / "scene-48x64.pfm").write_bytes(pfm(bgr[..., ::-1], little=True))
    out["scene-48x64"] = (d / "scene-48x64.pfm", bgr, tex, bright)
    bgr, tex, bright = scene(37, 53, 6)
    rgbe = to_rgbe(bgr)
    (d / "scene-37x53.hdr").write_bytes(radiance(rgbe, rle=True))
    out["scene-37x53"] = (d / "scene-37x53.hdr", decode_rgbe(rgbe), tex, bright)
    return out


def mirror_tonemap(nle, ctx, bgr, weights, sat=1.0, patch=0, sampler=0, exact=False):
    """the tone mapping composed from the Python mirror: (output codes, the filter, (x, guide, y), (l_hi, R))"""
    l_hi, R = ctx.hdr_range(bgr)
    x, g = ctx.hdr_to_loglum(bgr, l_hi, R)
    try:
        ctx.set_patch_radius(patch)
        ctx.set_sampler(sampler)
        if exact:
            ctx.set_mode(nle.MODE_EXACT_F64)
        f = nle.NLEFilter(ctx).train_filter(g, ARGS["nr"], ARGS["nc"], ARGS["hx"], ARGS["hy"], ARGS["T"], ARGS["K"])
    finally:
        ctx.set_patch_radius(0)
        ctx.set_sampler(0)
        ctx.set_mode(nle.MODE_AUTO)
    y = f.apply(x, nle.transform_eigenvalues(f.eigvals, weights)).reshape(x.shape)
    return ctx.loglum_to_bgr16(y, bgr, l_hi, R, weights[-1], sat).cpu().numpy(), f, (x, g, y), (l_hi, R)


def oracle_tonemap(oracle, tab, bgr, weights):
    """the same composition in fp64 on the CPU: the restatement around the oracle's filter; (codes, V, S, x, y)"""
    l_hi, R = hdr_range(bgr)
    x = forward(bgr, l_hi, R).astype(np.float32).astype(np.float64)
    g = np.rint(forward(bgr, l_hi, R))
    V, S = oracle.train_filter(g, ARGS["nr"], ARGS["nc"], ARGS["hx"], ARGS["hy"], ARGS["T"], ARGS["K"])
    y = oracle.apply_filter(V, x, oracle.transform_eigenvalues(S, weights))
    codes = code_of(inverse_linear(y.astype(np.float32), bgr, l_hi, R, weights[-1], 1.0), tab[1])
    return codes, V, S, x, y


def tone_figures(Y, bright):
    """of a luminance plane: log2 of the ratio of the two regions' mean luminance, and per region (dark, bright) the texture's
    log-amplitude -- the root mean square of log2 Y inside the region after every row's mean is taken out (the ramp runs
    along the rows' index, so it goes with the mean)"""
    ratio = float(np.log2(Y[bright].mean() / Y[~bright].mean()))
    amps = []
    for region in (~bright, bright):
        a = np.log2(Y[region]).reshape(-1, region[0].sum())
        a = a - a.mean(axis=1, keepdims=True)
        amps.append(float(np.sqrt(np.mean(a * a))))
    return ratio, amps[0], amps[1]


def output_luminance(codes, tab):
    return lum(tab[0][codes])


def run_cli(lead, src, out, weights=WEIGHTS):
    r = subprocess.run([ENHANCE] + lead + [str(src), str(out)] + ARGV + [repr(w) for w in weights], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-1500:])
    return r.stdout


DRIVER = textwrap.dedent(r"""
    #include <cstdio>
    #include <cstdlib>
    #include <functional>
    #include <string>
    #include <vector>
    #include "nle.h"
    #include "nle/filter.hpp"
    #include "nle/image_io.hpp"
    static bool throws(const std::function<void()>& fn) {
        try { fn(); } catch (const std::runtime_error&) { return true; }
        return false;
    }
    #define REQUIRE(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
    int main(int argc, char** argv) {   // in out nr nc hx hy T K w...
        const nle::Image im = nle::imreadHDR(argv[1]);
        REQUIRE(!im.empty() && im.depth() == nle::NLE_32F && im.channels() == 3);
        if (argc == 3 && std::string(argv[2]) == "group") {      // under NLE_DEVICES with two devices: refused, by name
            nle::NLEFilter f;
            f.verbose = false;
            try {
                f.trainForToneMapping(im, 6, 8, 16, 30, 10, 8);
                REQUIRE(false);
            } catch (const std::runtime_error& e) {
                REQUIRE(std::string(e.what()) == "Tone mapping runs on one device: unset NLE_DEVICES.");
            }
            std::printf("group OK\n");
            return 0;
        }
        std::vector<double> w;
        for (int i = 9; i < argc; ++i) w.push_back(std::atof(argv[i]));
        const int nr = std::atoi(argv[3]), nc = std::atoi(argv[4]), T = std::atoi(argv[7]), K = std::atoi(argv[8]);
        const double hx = std::atof(argv[5]), hy = std::atof(argv[6]);
        nle::NLEFilter f;
        f.verbose = false;
        f.chromaBandwidth = 20;                                  // refused, and nothing is trained
        REQUIRE(throws([&] { f.trainForToneMapping(im, nr, nc, hx, hy, T, K); }));
        f.chromaBandwidth = 0;
        f.trainForToneMapping(im, nr, nc, hx, hy, T, K);
        int d[8];
        f.diag(d);
        REQUIRE(d[0] == NLE_MODE_PHI_FREE);                     // the guide takes the default table path
        const nle::Image out = f.toneMap(im, w);
        REQUIRE(out.depth() == nle::NLE_16U && out.channels() == 3 && out.rows == im.rows && out.cols == im.cols);
        REQUIRE(nle::imwrite(argv[2], out));
        // the 8- and 16-bit methods refuse a 32F image, tone mapping refuses theirs, a size mismatch keeps the reference's message
        const std::vector<nle::Image> strokes(1, nle::Image(im.rows, im.cols, nle::NLE_8U, 1));
        nle::NLEFilter g;
        g.verbose = false;
        REQUIRE(throws([&] { g.trainForEnhancement(im, nr, nc, hx, hy, T, K); }));
        REQUIRE(throws([&] { g.trainForDenoise(im, nr, nc, hx, hy, T, K); }));
        REQUIRE(throws([&] { g.nystromResidual(im, nr, nc, hx, hy); }));
        REQUIRE(throws([&] { f.enhance(im, w); }));
        REQUIRE(throws([&] { f.enhanceRegions(im, strokes, {w}, w); }));
        REQUIRE(throws([&] { f.denoise(im, 2.0); }));
        REQUIRE(throws([&] { g.trainForToneMapping(nle::Image(im.rows, im.cols, nle::NLE_8U, 3), nr, nc, hx, hy, T, K); }));
        REQUIRE(throws([&] { f.toneMap(nle::Image(im.rows, im.cols, nle::NLE_16U, 3), w); }));
        REQUIRE(throws([&] { f.toneMap(im, w, 0.0); }));
        REQUIRE(throws([&] { f.toneMap(im, w, 2.5); }));
        f.chromaBandwidth = 20;
        REQUIRE(throws([&] { f.toneMap(im, w); }));
        f.chromaBandwidth = 0;
        nle::Image taller(im.rows + 1, im.cols, nle::NLE_32F, 3);
        for (size_t i = 0; i < taller.total() * 3; ++i) taller.ptr<float>()[i] = 0.5f;
        try {
            f.toneMap(taller, w);
            REQUIRE(false);
        } catch (const std::runtime_error& e) {
            REQUIRE(std::string(e.what()) == "Cannot apply filter on image with different size from the image filter was trained on.");
        }
        const nle::Image again = f.toneMap(im, w);
        REQUIRE(std::equal(again.ptr<unsigned short>(), again.ptr<unsigned short>() + 3 * im.total(), out.ptr<unsigned short>()));
        std::printf("tonemap OK\n");
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
def files(tmp_path_factory):
    return scene_files(tmp_path_factory.mktemp("tonee2e"))


@pytest.fixture(scope="module")
def mirrored(nle, ctx, files):
    """per scene: what the mirror composition makes of it"""
    out = {}
    for name, (_, bgr, _, _) in files.items():
        codes, f, planes, scale = mirror_tonemap(nle, ctx, bgr, WEIGHTS)
        out[name] = (codes, f, planes, scale)
    yield out
    for _, f, _, _ in out.values():
        f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["scene-48x64", "scene-37x53"])
def test_filter_on_the_guide_is_the_oracles_and_applies_to_the_unrounded_plane(nle, oracle, files, mirrored, name):
    _, bgr, _, _ = files[name]
    _, f, (x, g, y), (l_hi, R) = mirrored[name]
    assert f.diag()["formulation"] == nle.MODE_PHI_FREE                 # table mode
    want = hdr_range(bgr)
    assert abs(l_hi - want[0]) <= 1e-14 * abs(want[0]) and abs(R - want[1]) <= 1e-14 * want[1] and STOPS < R < STOPS + 1.2
    x64, g64 = x.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)
    assert np.array_equal(g64, np.rint(g64)) and np.max(np.abs(x64 - g64)) <= 0.5 + 1e-4 and np.any(x64 != g64) and x64.max() == 255.0
    V, S = oracle.train_filter(g64, ARGS["nr"], ARGS["nc"], ARGS["hx"], ARGS["hy"], ARGS["T"], ARGS["K"])
    assert len(S) == len(f.eigvals) and np.max(np.abs(f.eigvals - S)) <= 1e-8
    yo = oracle.apply_filter(V, x64, oracle.transform_eigenvalues(S, WEIGHTS))          # V f(Lambda) V^T x, x the UNROUNDED plane
    err = rel_l2(y.cpu().numpy().astype(np.float64), yo)
    print(name, "relative L2 of y:", "%.2e" % err)
    assert err < 1e-4


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
@pytest.mark.parametrize("name", ["scene-48x64", "scene-37x53"])
def test_cpp_surface_equals_the_mirror_byte_for_byte(driver, files, mirrored, tmp_path, name):
    r = subprocess.run([driver, str(files[name][0]), str(tmp_path / "drv.png")] + ARGV + [repr(w) for w in WEIGHTS], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "tonemap OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    assert np.array_equal(read_png16_rgb(tmp_path / "drv.png")[..., ::-1], mirrored[name][0])


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_a_device_group_is_refused(driver, files):
    """NLE_DEVICES with two devices (the same one twice forms a group too): trainForToneMapping throws, nothing is trained"""
    r = subprocess.run([driver, str(files["scene-37x53"][0]), "group"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, NLE_DEVICES="0,0"))
    assert r.returncode == 0 and "group OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["scene-48x64", "scene-37x53"])
def test_cli_equals_the_mirror_byte_for_byte(files, mirrored, tmp_path, name):
    stdout = run_cli(["--tonemap"], files[name][0], tmp_path / "cli.png")
    assert np.array_equal(read_png16_rgb(tmp_path / "cli.png")[..., ::-1], mirrored[name][0])
    lines = stdout.splitlines()         # stdout is today's: the four stage banners, min(K, 5) eigenvector lines, the closing line
    assert lines[:4] == ["Computing kernel", "Nystrom approximation", "Sinkhorn", "Orthogonalize"]
    assert len(lines) == 10 and all(ln.startswith(f"Eigvec {i} eigval: ") for i, ln in enumerate(lines[4:9]))
    assert lines[9] == "Done. Press any key in result window to exit."


@pytest.mark.gpu
@pytest.mark.parametrize("lead,kw", [(["--sampler", "farthest", "--tonemap"], dict(sampler=1)),
                                     (["--tonemap", "--patch-radius", "1"], dict(patch=1)),
                                     (["--tonemap", "--exact"], dict(exact=True)),
                                     (["--tonemap-saturation", "0.6", "--tonemap"], dict(sat=0.6))],
                         ids=["farthest", "patch", "exact", "saturation"])
def test_tonemap_with_the_other_options_equals_the_mirror(nle, ctx, files, mirrored, tmp_path, lead, kw):
    src, bgr, _, _ = files["scene-37x53"]
    want, f, _, _ = mirror_tonemap(nle, ctx, bgr, WEIGHTS, **kw)
    f.close()
    run_cli(lead, src, tmp_path / "o.png")
    assert np.array_equal(read_png16_rgb(tmp_path / "o.png")[..., ::-1], want)
    assert np.any(want != mirrored["scene-37x53"][0])                  # the option did something


# (log2 of the regions' mean-luminance ratio, the texture's log-amplitude in the dark region, in the bright region), in stops, of
# the fp64 oracle composition (oracle_tonemap, then tone_figures on the luminance of its codes), measured on the CPU
ORACLE_FIGURES = {
    "scene-48x64": (4.063505897620636, 0.0034673878498247277, 0.003379558564386157),    # the input: 10.2308, 0.08186, 0.08371
    "scene-37x53": (4.043712607366645, 0.010648699512964484, 0.004615055208254846),     # the input: 10.2334, 0.08108, 0.08062
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["scene-48x64", "scene-37x53"])
def test_it_tone_maps(files, mirrored, tab, name):
    """What the oracle composition does to the two scenes with weights 2 2 1 0.4 (fp64, on the CPU): the two regions, 10.23
    stops apart in the input, come out 4.06 and 4.04 stops apart -- the base weight 0.4 times the input's distance, nearly.
    The per-pixel texture, 0.082 stops in the input, comes out at 0.0035 / 0.0034 stops (48 x 64) and 0.0106 / 0.0046 stops
    (37 x 53): white noise lies outside the span of K = 8 eigenvectors, and y = V f(Lambda) V^T x keeps nothing outside it,
    whatever the weights -- the reference's enhance has the same property.  The GPU composition must give the oracle's
    figures within 1 %, compress the range, and keep no less texture than the oracle keeps."""
    _, bgr, _, bright = files[name]
    ratio, dark, light = tone_figures(output_luminance(mirrored[name][0], tab), bright)
    o_ratio, o_dark, o_light = ORACLE_FIGURES[name]
    print(name, "ratio %.5f (oracle %.5f), texture %.6f / %.6f (oracle %.6f / %.6f)" % (ratio, o_ratio, dark, light, o_dark, o_light))
    for got, want in ((ratio, o_ratio), (dark, o_dark), (light, o_light)):
        assert abs(got - want) <= 0.01 * abs(want)
    assert ratio < tone_figures(lum(bgr), bright)[0] and ratio < STOPS       # the range is compressed ...
    assert dark >= 0.99 * o_dark and light >= 0.99 * o_light                 # ... and the texture is not reduced by more than the oracle says


def test_the_oracle_figures_are_the_oracles(oracle, tab, tmp_path):
    """the numbers above, measured again (CPU only)"""
    for name, (_, bgr, _, bright) in scene_files(tmp_path).items():
        codes = oracle_tonemap(oracle, tab, bgr, WEIGHTS)[0]
        got = tone_figures(output_luminance(codes, tab), bright)
        assert all(abs(g - w) <= 1e-3 * abs(w) for g, w in zip(got, ORACLE_FIGURES[name])), (name, got)    # a tenth of what the GPU gets


# ------------------------------------------------------------------------------------------------ GPU: nothing else moved
def mirror_enhance8(nle, c, bgr8, args, weights):
    lab, L = c.bgr2lab8(bgr8)
    f = nle.NLEFilter(c).train_filter(L, args["nr"], args["nc"], args["hx"], args["hy"], args["T"], args["K"])
    y = f.apply_rounded8(L, nle.transform_eigenvalues(f.eigvals, weights))
    out = c.lab2bgr8(lab, L=y).cpu().numpy()
    f.close()
    return out


@pytest.mark.gpu
def test_eight_bit_and_deep_results_are_unchanged_after_tonemap_calls(nle, ctx, files, mirrored):
    """the shared ctx has run the new kernels and tone-mapping trains; a plain 8-bit train + enhance of flower on it is byte for
    byte the one of a fresh ctx, and so is a deep-colour round trip, whose threshold pairs the tone mapper shares"""
    from PIL import Image
    bgr8 = np.ascontiguousarray(np.asarray(Image.open(os.path.join(GOLDEN, "flower-50.bmp")).convert("RGB"))[..., ::-1])
    args = dict(nr=10, nc=20, hx=32.0, hy=30.0, T=10, K=10)
    codes, f, _, _ = mirror_tonemap(nle, ctx, files["scene-37x53"][1], WEIGHTS)
    f.close()
    assert np.array_equal(codes, mirrored["scene-37x53"][0])
    x16 = np.random.default_rng(8).integers(0, 65536, (1 << 16, 3), dtype=np.uint16)

    def both(c):
        L, a, b, g = c.bgr16_to_lab(x16)
        return mirror_enhance8(nle, c, bgr8, args, [3.0, 10.0, 1.0, 1.0]), [t.cpu().numpy() for t in (L, a, b, g)], c.lab_to_bgr16(L, a, b).cpu().numpy()
    got = both(ctx)
    fresh = nle.Context(0)
    try:
        want = both(fresh)
    finally:
        fresh.close()
    assert np.array_equal(got[0], want[0]) and np.any(got[0] != bgr8)
    assert all(np.array_equal(p.view(np.int32), q.view(np.int32)) for p, q in zip(got[1], want[1]))
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[2], x16)
