"""Deep-colour enhance: 16-bit sRGB -> float Lab -> train on the rounded L (the guide), apply to the
unrounded L -> 16-bit sRGB.  There is no reference for it (the reference is 8-bit only), so the definition is restated here
in numpy from the library's own tables (nle_srgb16_tables) -- in longdouble as the yardstick of the forward kernel, in fp64
for the inverse -- and the tests hold the tables, the kernels, the Python mirror, the C++ surface and `enhance --deep` to it.

Bounds.  Forward: L, a, b are fp32 roundings of fp64 values whose error is a few fp64 ulp, so they are within one fp32 ulp
of the longdouble restatement everywhere and differ from it at all only where the exact value lies within ~1e-16 relative
of an fp32 rounding boundary: at most 1 pixel in 1e5 may differ (the fp64 numpy restatement itself differs from the
longdouble one in 1 of 2 686 976 L values), which a wrong operation order or a fused multiply-add would exceed by orders of
magnitude.  The guide must be equal everywhere.  Inverse: codes must equal searchsorted on the library's thr, applied to
the fp64 restatement of the linear values, except where such a value is within 1e-12 relative of a threshold (fp64 error
is ~1e-16); those are counted (< 1 in 1e5) and may differ by one code."""
import os
import shutil
import subprocess
import textwrap

import numpy as np
import pytest

from conftest import GOLDEN, PKG_DIR, ROOT, rel_l2
from test_image_io16 import png_bytes, read_png16_rgb

ENHANCE = os.path.join(PKG_DIR, "bin", "enhance")
DENOISE = os.path.join(PKG_DIR, "bin", "denoise")
GRID_CAP_PIXELS = 2048 * 256 * 2  # the launchers' grid cap times their block size times two pixels per thread: beyond it the
                                  # stride loop runs (in the single-pixel form, which unaligned pointers take, from half of it)


# ------------------------------------------------------------------------------------------------ the restatement
def forward(bgr, tab, dt=np.float64):
    """(L, a, b) unrounded, in dtype dt, of (..., 3) uint16 BGR codes: the definition, operation by operation"""
    lin, _, F, _ = tab
    F = F.astype(dt)
    B, G, R = (lin[bgr[..., k]].astype(dt) for k in range(3))

    def f(t):
        big = t > 216.0 / 24389.0
        return np.where(big, np.cbrt(np.where(big, t, 1)), ((dt(24389.0) / dt(27.0)) * t + dt(16.0)) / dt(116.0))
    fx, fy, fz = (f((F[r, 0] * R + F[r, 1] * G) + F[r, 2] * B) for r in range(3))
    return (((dt(116.0) * fy - dt(16.0)) * dt(255.0)) / dt(100.0), dt(500.0) * (fx - fy) + dt(128.0),
            dt(200.0) * (fy - fz) + dt(128.0))


def guide_of(L):
    return np.clip(np.rint(L), 0, 255).astype(np.float32)


def inverse_linear(L, a, b, tab):
    """(..., 3) fp64 linear B, G, R of fp32 planes: the definition, operation by operation"""
    I = tab[3]
    L, a, b = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (L, a, b))
    with np.errstate(invalid="ignore"):
        Lc = np.where(L > 0.0, np.where(L < 255.0, L, 255.0), 0.0)      # a NaN counts as 0
        fy = ((Lc * 100.0) / 255.0 + 16.0) / 116.0
        fx = fy + (a - 128.0) / 500.0
        fz = fy - (b - 128.0) / 200.0

        def finv(f):
            return np.where(f > 6.0 / 29.0, (f * f) * f, ((116.0 * f - 16.0) * 27.0) / 24389.0)
        X, Y, Z = finv(fx), finv(fy), finv(fz)
        return np.stack([(I[r, 0] * X + I[r, 1] * Y) + I[r, 2] * Z for r in (2, 1, 0)], axis=-1)


def code_of(v, thr):
    """(number of c with thr[c] <= v) - 1, a NaN gives 0"""
    c = np.searchsorted(thr, v, side="right") - 1
    c[np.isnan(v)] = 0
    return c.astype(np.uint16)


def greys():
    c = np.arange(65536, dtype=np.uint16)
    return np.stack([c, c, c], axis=1)


def triples(n, seed, below=65536):
    return np.random.default_rng(seed).integers(0, below, (n, 3), dtype=np.uint16)


CORNERS = np.array([[b, g, r] for b in (0, 65535) for g in (0, 65535) for r in (0, 65535)], dtype=np.uint16)


@pytest.fixture(scope="module")
def tab(nle):
    return nle.srgb16_tables()


# ------------------------------------------------------------------------------------------------ CPU: the tables
def test_tables_agree_with_a_longdouble_restatement(tab):
    lin, thr, F, I = tab
    ld = np.longdouble

    def decode(v):
        return np.where(v <= ld("0.04045"), v / ld("12.92"), np.power((v + ld("0.055")) / ld("1.055"), ld("2.4")))
    c = np.arange(65536).astype(ld)
    want_lin = decode(c / ld(65535))
    want_thr = decode((c - ld(0.5)) / ld(65535))
    assert np.all(np.abs(lin - want_lin) <= 4 * np.spacing(lin))
    assert thr[0] == -np.inf and np.all(np.abs(thr[1:] - want_thr[1:]) <= 4 * np.spacing(thr[1:]))
    assert np.all(np.diff(thr) > 0)                                       # strictly increasing: the encoding is defined through it
    assert np.all(thr < lin) and np.all(lin[:-1] < thr[1:])               # thr[c] < lin[c] < thr[c + 1]
    assert np.array_equal(code_of(lin, thr), np.arange(65536, dtype=np.uint16))
    assert lin[0] == 0.0 and lin[65535] == 1.0
    assert np.max(np.abs(I @ F - np.eye(3))) <= 1e-14 and np.max(np.abs(F @ I - np.eye(3))) <= 1e-14
    M = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
    assert np.array_equal(F, M / ((M[:, 0] + M[:, 1]) + M[:, 2])[:, None])
    assert (F[1, 0] * lin[65535] + F[1, 1] * lin[65535]) + F[1, 2] * lin[65535] == 1.0      # white: Y = 1


def test_the_tables_are_host_only_and_refuse_null(nle):
    import ctypes as C
    buf = (C.c_double * 65536)()
    k = (C.c_double * 18)()
    assert nle.lib().nle_srgb16_tables(None, buf, k) == nle.NLE_ERR_INVALID
    assert nle.lib().nle_srgb16_tables(buf, None, k) == nle.NLE_ERR_INVALID
    assert nle.lib().nle_srgb16_tables(buf, buf, None) == nle.NLE_ERR_INVALID
    for name in ("nle_srgb16_tables", "nle_bgr16_to_lab", "nle_lab_to_bgr16"):
        assert name in nle.EXPORTED_SYMBOLS and hasattr(nle.lib(), name)


@pytest.mark.parametrize("name,make", [("greys", greys), ("random", lambda: triples(1 << 21, 1)),
                                       ("dark", lambda: triples(1 << 19, 2, below=600))])
def test_restatement_round_trips_through_fp32_planes(tab, name, make):
    """forward, fp32 storage, inverse is the identity in the fp64 restatement: why fp32 planes are enough"""
    x = make()
    L, a, b = (v.astype(np.float32) for v in forward(x, tab))
    back = code_of(inverse_linear(L, a, b, tab), tab[1])
    assert np.count_nonzero(back != x) == 0


# ------------------------------------------------------------------------------------------------ CPU: the CLI's refusals
ARGS8 = ["6", "8", "16", "30", "10", "8"]


@pytest.mark.parametrize("exe,argv", [
    (ENHANCE, ["--deep=1", "missing.png", "o.png"] + ARGS8 + ["3", "3", "1", "1"]),
    (ENHANCE, ["--deep", "--region", "mask.png:1,1,1,1", "missing.png", "o.png"] + ARGS8 + ["3", "3", "1", "1"]),
    (ENHANCE, ["--region", "mask.png:1,1,1,1", "--deep", "missing.png", "o.png"] + ARGS8 + ["3", "3", "1", "1"]),
    (ENHANCE, ["--exact", "--deep", "missing.png", "o.bmp"] + ARGS8 + ["3", "3", "1", "1"]),
    (ENHANCE, ["--deep", "missing.png", "png"] + ARGS8 + ["3", "3", "1", "1"]),
    (DENOISE, ["--deep", "missing.png", "o.png"] + ARGS8 + ["10", "10", "2"]),
    (DENOISE, ["--deep=0", "missing.png", "o.png"] + ARGS8 + ["10", "10", "2"]),
], ids=["value", "region", "region-first", "not-png", "no-extension", "denoise", "denoise-value"])
def test_cli_refuses_before_anything_runs(tmp_path, exe, argv):
    """status 2 and one line on stderr; the input does not even exist, so nothing was read and no GPU call was made"""
    r = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert len(r.stderr.strip().splitlines()) == 1 and "--deep" in r.stderr and r.stdout == ""
    assert not os.listdir(tmp_path)


# ------------------------------------------------------------------------------------------------ GPU: the two kernels
@pytest.fixture(scope="module")
def sets(tab):
    """all greys, 2^20 random triples, 2^19 triples below code 600, the eight cube corners -- and their longdouble reference"""
    x = np.concatenate([greys(), triples(1 << 20, 11), triples(1 << 19, 12, below=600), CORNERS])
    L, a, b = forward(x, tab, np.longdouble)
    ref = {"x": x, "L": L.astype(np.float32), "a": a.astype(np.float32), "b": b.astype(np.float32), "guide": guide_of(L)}
    for v in ref.values():
        v.setflags(write=False)
    return ref


@pytest.fixture(scope="module")
def dev(ctx, sets):
    """the forward kernel's outputs on the whole set, on the device"""
    L, a, b, g = ctx.bgr16_to_lab(sets["x"])
    return {"L": L, "a": a, "b": b, "guide": g}


@pytest.mark.gpu
def test_forward_kernel_against_the_longdouble_restatement(sets, dev):
    n = len(sets["x"])
    for k in ("L", "a", "b"):
        got, want = dev[k].cpu().numpy(), sets[k]
        ulp = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
        differ = int(np.count_nonzero(got != want))
        print(f"{k}: {differ} of {n} differ, max {ulp.max():.1f} ulp")
        assert ulp.max() <= 1.0, k
        assert differ <= n // 100000, (k, differ)
    assert np.array_equal(dev["guide"].cpu().numpy(), sets["guide"])
    # the eight corners: black is L = 0, a = b = 128 exactly; white is L = 255
    tail = {k: dev[k].cpu().numpy()[-8:] for k in dev}
    assert (tail["L"][0], tail["a"][0], tail["b"][0], tail["guide"][0]) == (0.0, 128.0, 128.0, 0.0)
    assert tail["L"][7] == 255.0 and tail["guide"][7] == 255.0


def raw_forward(nle, ctx, bgr, n, outs):
    import ctypes as C
    ctx._sync_in()
    p = [C.c_void_p(t.data_ptr()) if t is not None else None for t in outs]
    return nle.lib().nle_bgr16_to_lab(ctx._h, C.c_void_p(bgr.data_ptr()) if bgr is not None else None, n, *p)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 257, 37 * 53, GRID_CAP_PIXELS + 77])
def test_forward_shapes_and_optional_outputs(nle, ctx, sets, dev, n):
    """every size against the full run's own first n values, bit for bit; a, b and guide NULL in every combination; outputs
    are prefilled with NaN and 64 elements longer: an element the kernel did not write, or wrote beyond n, shows"""
    import torch
    x = torch.from_numpy(sets["x"][:n].copy()).to(dev["L"].device)
    for mask in range(8):
        outs = [torch.full((n + 64,), float("nan"), device=x.device) for _ in range(4)]
        given = [outs[0]] + [outs[j] if mask >> (j - 1) & 1 else None for j in (1, 2, 3)]
        assert raw_forward(nle, ctx, x, n, given) == nle.NLE_OK
        for j, k in enumerate(("L", "a", "b", "guide")):
            o = outs[j]
            assert bool(torch.isnan(o[n:]).all()), (k, mask)
            if given[j] is None:
                assert bool(torch.isnan(o[:n]).all())
            else:
                assert torch.equal(o[:n].view(torch.int32), dev[k][:n].view(torch.int32)), (k, mask)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1001, 2048 * 256 + 1001], ids=["one-sweep", "stride-loop"])
def test_unaligned_pointers_take_the_single_pixel_form(nle, ctx, sets, dev, n):
    """the kernels take two pixels per thread where the image is 4-byte and the planes are 8-byte aligned; an image that
    starts on an odd pixel (2-byte aligned) and planes that start on an odd element give the same bits one pixel at a time"""
    import ctypes as C
    import torch
    d = dev["L"].device     # the second n is past grid cap x block size: the single-pixel loops stride
    x = torch.from_numpy(sets["x"][:n + 1].copy()).to(d)[1:]
    outs = [torch.full((n + 65,), float("nan"), device=d)[1:] for _ in range(4)]
    assert x.data_ptr() % 4 == 2 and all(o.data_ptr() % 8 == 4 for o in outs)
    assert raw_forward(nle, ctx, x, n, outs) == nle.NLE_OK
    for o, k in zip(outs, ("L", "a", "b", "guide")):
        assert torch.equal(o[:n].view(torch.int32), dev[k][1:n + 1].view(torch.int32)) and bool(torch.isnan(o[n:]).all()), k
    back = torch.full((n + 2, 3), 7, dtype=torch.uint16, device=d)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ctx._sync_in()
    assert nle.lib().nle_lab_to_bgr16(ctx._h, P(outs[0]), P(outs[1]), P(outs[2]), n, P(back[1:])) == nle.NLE_OK
    back = back.cpu().numpy()
    assert np.array_equal(back[1:n + 1], sets["x"][1:n + 1]) and np.all(back[0] == 7) and np.all(back[n + 1] == 7)


@pytest.mark.gpu
def test_refusals_leave_the_ctx_usable(nle, ctx, sets, dev):
    import ctypes as C
    import torch
    d = dev["L"].device
    x = torch.from_numpy(sets["x"][:100].copy()).to(d)
    o = [torch.zeros(100, device=d) for _ in range(4)]
    out16 = torch.zeros((100, 3), dtype=torch.uint16, device=d)
    lib, P = nle.lib(), lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ctx._sync_in()
    bad = [lambda: raw_forward(nle, ctx, None, 100, o), lambda: raw_forward(nle, ctx, x, 100, [None] + o[1:]),
           lambda: raw_forward(nle, ctx, x, 0, o), lambda: raw_forward(nle, ctx, x, -5, o),
           lambda: lib.nle_lab_to_bgr16(ctx._h, None, P(o[1]), P(o[2]), 100, P(out16)),
           lambda: lib.nle_lab_to_bgr16(ctx._h, P(o[0]), P(o[1]), P(o[2]), 100, None),
           lambda: lib.nle_lab_to_bgr16(ctx._h, P(o[0]), P(o[1]), P(o[2]), 0, P(out16))]
    for call in bad:
        assert call() == nle.NLE_ERR_INVALID
        assert lib.nle_last_error(ctx._h)
        assert raw_forward(nle, ctx, x, 100, o) == nle.NLE_OK                     # still usable
        assert torch.equal(o[0].view(torch.int32), dev["L"][:100].view(torch.int32))
    with pytest.raises(nle.NLEError):
        ctx.lab_to_bgr16(o[0], o[1], o[2][:50])


def check_inverse(got, L, a, b, tab):
    """device codes against searchsorted on the fp64 restatement; returns the number of waived samples"""
    thr = tab[1]
    v = inverse_linear(L, a, b, tab)
    want = code_of(v, thr)
    with np.errstate(invalid="ignore"):
        lo, hi = thr[want], np.where(want == 65535, np.inf, thr[np.minimum(want.astype(np.int64) + 1, 65535)])
        near = (np.abs(v - lo) <= 1e-12 * np.abs(v)) | (np.abs(v - hi) <= 1e-12 * np.abs(v))
    wrong = got != want
    assert not np.any(wrong & ~near), int(np.count_nonzero(wrong & ~near))
    assert np.all(np.abs(got.astype(np.int64) - want.astype(np.int64))[wrong] <= 1)
    return int(np.count_nonzero(near))


@pytest.mark.gpu
def test_inverse_kernel_and_the_device_round_trip(ctx, tab, sets, dev):
    got = ctx.lab_to_bgr16(dev["L"], dev["a"], dev["b"]).cpu().numpy()
    assert np.array_equal(got, sets["x"])                                          # lab_to_bgr16(bgr16_to_lab(x)) == x
    L, a, b = (dev[k].cpu().numpy() for k in ("L", "a", "b"))
    near = check_inverse(got, L, a, b, tab)
    print("round trip: within 1e-12 of a threshold:", near)
    assert near < got.size / 1e5


@pytest.mark.gpu
def test_inverse_kernel_clamps_saturates_and_takes_nan(ctx, tab):
    rng = np.random.default_rng(21)
    n = 1 << 20
    L = rng.uniform(-20, 280, n).astype(np.float32)
    a = rng.uniform(0, 255, n).astype(np.float32)
    b = rng.uniform(0, 255, n).astype(np.float32)
    nan = np.float32("nan")
    special = np.array([[nan, 128, 128], [50, nan, 128], [50, 128, nan], [nan, nan, nan], [np.inf, 128, 128], [-np.inf, 128, 128],
                        [50, np.inf, 128], [50, 128, -np.inf], [0, 128, 128], [255, 128, 128], [300, 128, 128], [-1, 128, 128]],
                       dtype=np.float32)
    L, a, b = (np.concatenate([p, special[:, k]]) for k, p in enumerate((L, a, b)))
    got = ctx.lab_to_bgr16(L, a, b).cpu().numpy()
    near = check_inverse(got, L, a, b, tab)
    print("random planes: within 1e-12 of a threshold:", near, "saturated low / high:",
          int(np.count_nonzero(got == 0)), int(np.count_nonzero(got == 65535)))
    assert near < got.size / 1e5
    assert np.count_nonzero(got == 0) > 1000 and np.count_nonzero(got == 65535) > 1000      # out of gamut both ways ran
    s = got[n:]
    assert np.array_equal(s[0], [0, 0, 0]) and np.array_equal(s[3], [0, 0, 0])      # NaN L' counts as 0: black
    assert np.array_equal(s[1], [0, 0, 0]) and np.array_equal(s[2], [0, 0, 0])      # NaN a or b: every channel NaN, code 0
    assert np.array_equal(s[8], [0, 0, 0]) and np.array_equal(s[9], [65535] * 3) and np.array_equal(s[10], s[9])
    assert np.array_equal(s[11], s[8]) and np.array_equal(s[4], s[9]) and np.array_equal(s[5], s[8])


# ------------------------------------------------------------------------------------------------ GPU: end to end
ARGS = dict(nr=6, nc=8, hx=16.0, hy=30.0, T=10, K=8)
ARGV = ["6", "8", "16", "30", "10", "8"]
WEIGHTS = [3.0, 3.0, 1.0, 1.0]


def gradient16(H, W, seed):
    """a smooth 16-bit colour gradient plus noise, BGR"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([9000 + 30000 * x / W + 6000 * np.sin(y / 7.0), 20000 + 25000 * y / H, 52000 - 35000 * (x + y) / (H + W)], axis=2)
    return np.clip(np.rint(img + rng.normal(0, 250, img.shape)), 0, 65535).astype(np.uint16)


def flower16(H, W):
    """a crop of the golden flower, widened x257, BGR"""
    from PIL import Image
    rgb = np.asarray(Image.open(os.path.join(GOLDEN, "flower-50.bmp")).convert("RGB"))
    return np.ascontiguousarray(rgb[100:100 + H, 150:150 + W, ::-1]).astype(np.uint16) * 257


IMAGES = {"gradient-48x64": lambda: gradient16(48, 64, 5), "flower-37x53": lambda: flower16(37, 53)}


def mirror_enhance16(nle, ctx, bgr, weights, patch=0, sampler=0, hc=None, exact=False):
    """the deep-colour enhance composed from the Python mirror: (output codes, the filter, its planes)"""
    import torch
    L, a, b, g = ctx.bgr16_to_lab(bgr)
    try:
        ctx.set_patch_radius(patch)
        ctx.set_sampler(sampler)
        if exact:
            ctx.set_mode(nle.MODE_EXACT_F64)
        if hc is not None:      # the chroma affinity takes a and b rounded to the 8-bit path's levels, like the guide
            ar, br = torch.round(a).clamp(0, 255), torch.round(b).clamp(0, 255)
            ctx.set_chroma(ar, br, hc)
        f = nle.NLEFilter(ctx).train_filter(g, ARGS["nr"], ARGS["nc"], ARGS["hx"], ARGS["hy"], ARGS["T"], ARGS["K"])
    finally:
        ctx.set_chroma(None, None, 0.0)
        ctx.set_patch_radius(0)
        ctx.set_sampler(0)
        ctx.set_mode(nle.MODE_AUTO)
    y = f.apply(L, nle.transform_eigenvalues(f.eigvals, weights)).reshape(L.shape)
    return ctx.lab_to_bgr16(y, a, b).cpu().numpy(), f, (L, g)


def run_cli(lead, src, out, weights=WEIGHTS, argv=ARGV):
    r = subprocess.run([ENHANCE] + lead + [str(src), str(out)] + argv + [repr(w) for w in weights], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-1500:])
    return r.stdout


DRIVER = textwrap.dedent(r"""
    #include <cstdio>
    #include <cstdlib>
    #include <functional>
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
        const nle::Image im = nle::imread16(argv[1]);
        REQUIRE(!im.empty() && im.depth() == nle::NLE_16U && im.channels() == 3);
        std::vector<double> w;
        for (int i = 9; i < argc; ++i) w.push_back(std::atof(argv[i]));
        nle::NLEFilter f;
        f.verbose = false;
        f.trainForEnhancement(im, std::atoi(argv[3]), std::atoi(argv[4]), std::atof(argv[5]), std::atof(argv[6]), std::atoi(argv[7]),
                              std::atoi(argv[8]));
        int d[8];
        f.diag(d);
        REQUIRE(d[0] == NLE_MODE_PHI_FREE);                     // the guide takes the default table path
        const nle::Image out = f.enhance(im, w);
        REQUIRE(out.depth() == nle::NLE_16U && out.channels() == 3 && out.rows == im.rows && out.cols == im.cols);
        REQUIRE(nle::imwrite(argv[2], out));
        // what is not built for 16-bit images throws, a size mismatch keeps the reference's message, and the filter still works
        const std::vector<nle::Image> strokes(1, nle::Image(im.rows, im.cols, nle::NLE_8U, 1));
        REQUIRE(throws([&] { f.enhanceRegions(im, strokes, {w}, w); }));
        REQUIRE(throws([&] { f.denoise(im, 2.0); }));
        nle::NLEFilter g;
        g.verbose = false;
        REQUIRE(throws([&] { g.trainForDenoise(im, 4, 4, 16, 30, 10, 8); }));
        try {
            f.enhance(nle::Image(im.rows + 1, im.cols, nle::NLE_16U, 3), w);
            REQUIRE(false);
        } catch (const std::runtime_error& e) {
            REQUIRE(std::string(e.what()) == "Cannot apply filter on image with different size from the image filter was trained on.");
        }
        const nle::Image again = f.enhance(im, w);
        REQUIRE(std::equal(again.ptr<unsigned short>(), again.ptr<unsigned short>() + 3 * im.total(), out.ptr<unsigned short>()));
        std::printf("deep OK\n");
        return 0;
    }
""")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("deepdrv")
    host, libdir = os.path.join(PKG_DIR, "host"), os.path.join(PKG_DIR, "lib")
    (d / "drv.cpp").write_text(DRIVER)
    b = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(d / "drv.cpp"),
                        *[os.path.join(host, s) for s in ("filter.cpp", "stages.cpp", "colour.cpp", "device_group.cpp", "image_io.cpp", "jpeg.cpp")],
                        "-L", libdir, "-lnle_hip", "-Wl,-rpath," + libdir, "-o", str(d / "drv")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    return str(d / "drv")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(IMAGES))
def test_filter_on_the_guide_is_the_oracles_and_applies_to_the_unrounded_plane(nle, oracle, ctx, name):
    bgr = IMAGES[name]()
    _, f, (L, g) = mirror_enhance16(nle, ctx, bgr, WEIGHTS)
    assert f.diag()["formulation"] == nle.MODE_PHI_FREE                 # table mode
    L64, g64 = L.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)
    assert np.array_equal(g64, np.rint(g64)) and np.max(np.abs(L64 - g64)) <= 0.5 + 1e-4 and np.any(L64 != g64)
    V, S = oracle.train_filter(g64, ARGS["nr"], ARGS["nc"], ARGS["hx"], ARGS["hy"], ARGS["T"], ARGS["K"])
    assert len(S) == len(f.eigvals) and np.max(np.abs(f.eigvals - S)) <= 1e-8
    nl = 4
    Y = f.apply_layers(L, nl).cpu().numpy().astype(np.float64)
    Yo = oracle.apply_layers(V, S, L64, nl).reshape(nl, -1)            # V f(Lambda) V^T x in fp64, x the UNROUNDED plane
    errs = [rel_l2(Y[j], Yo[j]) for j in range(nl)]
    print(name, "per-layer relative L2:", ["%.2e" % e for e in errs])
    assert max(errs) < 1e-4, errs
    f.close()


@pytest.fixture(scope="module")
def mirror_files(nle, ctx, tmp_path_factory):
    """per image: the 16-bit PNG the tools read and the mirror composition's output codes.  The writer stores its samples
    (filter 0, stored blocks), so two files hold the same codes exactly when they are the same bytes"""
    d = tmp_path_factory.mktemp("deepe2e")
    out = {}
    for name, make in IMAGES.items():
        bgr = make()
        src = d / (name + ".png")
        src.write_bytes(png_bytes(bgr[..., ::-1], filt=1))
        want, f, _ = mirror_enhance16(nle, ctx, bgr, WEIGHTS)
        f.close()
        assert np.any(want != bgr)                                      # an edit happened
        out[name] = (src, want)
    return out


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
@pytest.mark.parametrize("name", list(IMAGES))
def test_cpp_surface_equals_the_mirror_byte_for_byte(driver, mirror_files, tmp_path, name):
    src, want = mirror_files[name]
    r = subprocess.run([driver, str(src), str(tmp_path / "drv.png")] + ARGV + [repr(w) for w in WEIGHTS], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "deep OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    assert np.array_equal(read_png16_rgb(tmp_path / "drv.png")[..., ::-1], want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(IMAGES))
def test_cli_equals_the_mirror_byte_for_byte(mirror_files, tmp_path, name):
    src, want = mirror_files[name]
    stdout = run_cli(["--deep"], src, tmp_path / "cli.png")
    assert np.array_equal(read_png16_rgb(tmp_path / "cli.png")[..., ::-1], want)
    # stdout is today's: the four stage banners, min(K, 5) eigenvector lines, the closing line
    lines = stdout.splitlines()
    assert lines[:4] == ["Computing kernel", "Nystrom approximation", "Sinkhorn", "Orthogonalize"]
    assert len(lines) == 10 and all(ln.startswith(f"Eigvec {i} eigval: ") for i, ln in enumerate(lines[4:9]))
    assert lines[9] == "Done. Press any key in result window to exit."


@pytest.mark.gpu
@pytest.mark.parametrize("lead,kw", [(["--sampler", "farthest", "--deep"], dict(sampler=1)),
                                     (["--deep", "--patch-radius", "1"], dict(patch=1)),
                                     (["--chroma", "20", "--deep"], dict(hc=20.0)),
                                     (["--deep", "--exact"], dict(exact=True)),
                                     (["--nystrom-report", "--deep"], dict())],
                         ids=["farthest", "patch", "chroma", "exact", "nystrom-report"])
def test_deep_with_the_other_options_equals_the_mirror(nle, ctx, tmp_path, lead, kw):
    bgr = IMAGES["flower-37x53"]()
    src, out = tmp_path / "in.png", tmp_path / "o.png"
    src.write_bytes(png_bytes(bgr[..., ::-1]))
    want, f, (_, g) = mirror_enhance16(nle, ctx, bgr, WEIGHTS, **kw)
    stdout = run_cli(lead, src, out)
    assert np.array_equal(read_png16_rgb(out)[..., ::-1], want)
    if "--nystrom-report" in lead:      # computed on the guide
        _, s = ctx.nystrom_residual(g, ARGS["nr"], ARGS["nc"], ARGS["hx"], ARGS["hy"])
        words = stdout.splitlines()[-1].replace("(", " ").replace(")", " ").replace(",", " ").split()
        assert words[:3] == ["Nystrom", "residual:", "mean"]
        assert abs(float(words[3]) - s["sum"] / g.numel()) <= 1e-5 * float(words[3]) and abs(float(words[5]) - s["max"]) <= 1e-5 * s["max"]
    f.close()


def mirror_enhance8(nle, c, bgr8, args, weights):
    lab, L = c.bgr2lab8(bgr8)
    f = nle.NLEFilter(c).train_filter(L, args["nr"], args["nc"], args["hx"], args["hy"], args["T"], args["K"])
    y = f.apply_rounded8(L, nle.transform_eigenvalues(f.eigvals, weights))
    out = c.lab2bgr8(lab, L=y).cpu().numpy()
    f.close()
    return out


@pytest.mark.gpu
def test_a_ramp_keeps_more_than_256_levels_only_with_deep(nle, tmp_path):
    """what the feature is for: a 16 x 1024 ramp over all codes, weights 3 3 1 1.  --deep leaves more than 256 distinct values
    in a row, which no 8-bit pipeline can; the default path on the same file gives at most 256 and is, bit for bit, what a
    ctx that never saw the new entry points computes from the file's high bytes"""
    from PIL import Image
    code = np.rint(np.arange(1024) * (65535 / 1023)).astype(np.uint16)
    ramp = np.repeat(np.repeat(code[None, :, None], 16, axis=0), 3, axis=2)
    src, deep, plain = tmp_path / "ramp.png", tmp_path / "deep.png", tmp_path / "plain.png"
    src.write_bytes(png_bytes(ramp))
    argv = ["4", "16", "32", "30", "10", "8"]
    run_cli(["--deep"], src, deep, argv=argv)
    run_cli([], src, plain, argv=argv)
    d = read_png16_rgb(deep)
    levels = [len(np.unique(d[8, :, k])) for k in range(3)]
    print("distinct values in row 8 with --deep:", levels)
    assert min(levels) > 256
    p = np.asarray(Image.open(plain))
    assert p.dtype == np.uint8 and p.shape == (16, 1024, 3) and max(len(np.unique(p[8, :, k])) for k in range(3)) <= 256
    fresh = nle.Context(0)
    try:
        want = mirror_enhance8(nle, fresh, (ramp >> 8).astype(np.uint8), dict(nr=4, nc=16, hx=32.0, hy=30.0, T=10, K=8), WEIGHTS)
    finally:
        fresh.close()
    assert np.array_equal(p[..., ::-1], want)


@pytest.mark.gpu
def test_eight_bit_enhance_is_unchanged_after_deep_calls(nle, ctx, sets, dev):
    """the shared ctx has run both new kernels (dev) and deep trains; a plain 8-bit train + enhance of flower on it is byte for
    byte the one of a fresh ctx"""
    from PIL import Image
    bgr8 = np.ascontiguousarray(np.asarray(Image.open(os.path.join(GOLDEN, "flower-50.bmp")).convert("RGB"))[..., ::-1])
    args = dict(nr=10, nc=20, hx=32.0, hy=30.0, T=10, K=10)
    out16, f, _ = mirror_enhance16(nle, ctx, flower16(37, 53), WEIGHTS)
    f.close()
    got = mirror_enhance8(nle, ctx, bgr8, args, [3.0, 10.0, 1.0, 1.0])
    fresh = nle.Context(0)
    try:
        want = mirror_enhance8(nle, fresh, bgr8, args, [3.0, 10.0, 1.0, 1.0])
    finally:
        fresh.close()
    assert np.array_equal(got, want) and np.any(got != bgr8)
