"""Region edits: nle_region_combine / nle_region_spread / nle_apply_regions, NLEFilter::enhanceRegions and
`enhance --region MASK:w1,w2,... [--region-spread T] [--region-floor F]`.

The restatement below is the contract of include/nle.h ("region edits"), in numpy.  A trained filter has K' pairs (V, lambda);
with stroke planes s_1 .. s_M, scales c_m, the spread t, the floor phi and the weights Wt[(M + 1)][L] (row 0 the background):

    spread   q_m = apply(s_m, c_m lambda^t)                  oracle.apply_filter on oracle.train_filter's V, cast to fp32
    layers   Y_l = apply_layers(x, L)                         oracle.apply_layers, cast to fp32
    combine  u_m = q_m > 0 ? q_m : 0 (a NaN counts as 0);  sigma = u_1 + .. + u_M;  d = sigma > phi ? sigma : phi
             alpha_m = u_m / d;  alpha_0 = 1 - sigma / d;  w_l = alpha_0 Wt[0][l] + .. + alpha_M Wt[M][l]
             y = w_0 Y_0 + .. + w_{L-1} Y_{L-1}               fp64, every operation on its own, ascending m and l

and the output kinds store (float)y, rint((float)y) saturated to [0, 255] as fp32, or that value as a byte."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, rel_l2

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_patch_affinity as tpa  # noqa: E402

ENHANCE, DENOISE = tpa.ENHANCE, tpa.DENOISE
FLOWER, FLOWER_ARGS, DENOISE_ARGS = tpa.FLOWER, tpa.FLOWER_ARGS, tpa.DENOISE_ARGS
FLOWER_BMP = os.path.join(GOLDEN, "flower-50.bmp")
PER_LAYER_TOL = 1e-4  # the project's standing per-layer bar: a spread is an apply with one response
SPREAD, FLOOR = 4.0, 0.05  # the defaults of the C++ surface and the CLI
F32, ROUNDED8, U8 = 0, 1, 2


# ----------------------------------------------------------------------------------------------- the restatement
def memberships(Q, floor):
    """alpha (M + 1, n) fp64 and sigma (n) of the fp32 spread planes Q (M, n)"""
    Q = np.asarray(Q, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        u = np.where(Q > 0, Q.astype(np.float64), 0.0)
    sigma = u[0].copy()
    for m in range(1, Q.shape[0]):
        sigma = sigma + u[m]
    d = np.where(sigma > floor, sigma, floor)
    return np.concatenate([(1.0 - sigma / d)[None], u / d]), sigma


def combine(Y, Q, Wt, floor):
    """y (n) fp64 of the fp32 layer planes Y (L, n), the fp32 spread planes Q (M, n) and Wt (M + 1, L)"""
    Y = np.asarray(Y, dtype=np.float32)
    Wt = np.asarray(Wt, dtype=np.float64)
    alpha, _ = memberships(Q, floor)
    assert Wt.shape == (alpha.shape[0], Y.shape[0])
    y = None
    for l in range(Y.shape[0]):
        w = alpha[0] * Wt[0, l]
        for m in range(1, alpha.shape[0]):
            w = w + alpha[m] * Wt[m, l]
        t = w * Y[l].astype(np.float64)
        y = t if y is None else y + t
    return y


def stored(y, kind):
    """what an output kind stores of the fp64 plane y"""
    v = np.asarray(y, dtype=np.float64).astype(np.float32)
    if kind == F32:
        return v
    r = np.minimum(np.float32(255), np.maximum(np.float32(0), np.rint(v)))  # k_plane_to_u8's rule
    return r if kind == ROUNDED8 else r.astype(np.uint8)


def boxes(H, W, corners, size):
    """0 / 1 stroke planes (M, H, W) fp32: a size x size box with its top-left corner at each (row, col)"""
    s = np.zeros((len(corners), H, W), dtype=np.float32)
    for m, (r, c) in enumerate(corners):
        s[m, r:r + size, c:c + size] = 1.0
    return s


def restated_spread(oracle, V, S, strokes, scale, t):
    """the fp32 spread planes (M, n)"""
    return np.stack([oracle.apply_filter(V, s.astype(np.float64), c * np.power(S, t)).ravel()
                     for s, c in zip(strokes, scale)]).astype(np.float32)


# the synthetic plane of the issue and its strokes; the weights: the background's row, then one row per region
SYNTH = tpa.SYNTH  # 72 x 96, nr 6, nc 8, hx 16, hy 30, T 10, K 12, L 4
SYNTH_CORNERS = [(0, 41), (17, 72), (50, 47)]
WT = np.array([[1.0, 1.0, 1.0, 1.0], [4.0, 3.0, 2.0, 1.0], [0.5, 0.5, 1.0, 1.0], [2.0, 0.25, 1.5, 1.0]])
FLOWER_CORNERS = [(167, 0), (199, 346)]

_cache = {}


def _synth(oracle):
    """(x, V, S, strokes (3, H, W), scale) of the synthetic plane, single-pixel affinities"""
    if "synth" not in _cache:
        H, W, nr, nc, hx, hy, T, K, _ = SYNTH
        x = oracle.synthetic_luminance(H, W)
        V, S = oracle.train_filter(x, nr, nc, hx, hy, T, K)
        _cache["synth"] = (x, V, S, boxes(H, W, SYNTH_CORNERS, 5), np.full(3, H * W / 25.0))
    return _cache["synth"]


def _flower(oracle):
    if "flower" not in _cache:
        x = tpa._flower_L(oracle)
        H, W = x.shape
        V, S = oracle.train_filter(x, FLOWER["nr"], FLOWER["nc"], FLOWER["hx"], FLOWER["hy"], FLOWER["T"], FLOWER["K"])
        _cache["flower"] = (x, V, S, boxes(H, W, FLOWER_CORNERS, 9), np.full(2, H * W / 81.0))
    return _cache["flower"]


def _restated_edit(oracle, key, M, L=4):
    """(Q (M, n) fp32, Y (L, n) fp32, y (n) fp64) of the restatement on a cached plane with its first M strokes"""
    k = (key, M, L)
    if k not in _cache:
        x, V, S, strokes, scale = _synth(oracle) if key == "synth" else _flower(oracle)
        Q = restated_spread(oracle, V, S, strokes[:M], scale[:M], SPREAD)
        Y = oracle.apply_layers(V, S, x, L).reshape(L, -1).astype(np.float32)
        _cache[k] = (Q, Y, combine(Y, Q, WT[:M + 1, :L], FLOOR))
    return _cache[k]


# ------------------------------------------------------------------------------------------------------ CPU tests
def test_restatement_by_hand_and_its_identities():
    """one pixel scalar by scalar; the memberships sum to 1; with M = 1 and equal rows y is the global edit"""
    rng = np.random.default_rng(7)
    L, M, n, phi = 4, 3, 64, 0.05
    Y = (rng.normal(size=(L, n)) * 40).astype(np.float32)
    Q = rng.normal(size=(M, n)).astype(np.float32) * np.float32(0.3)
    Q[:, :8] = np.abs(Q[:, :8]) * np.float32(0.01)  # under the floor
    Q[1, 9] = np.nan
    Wt = rng.normal(size=(M + 1, L))
    y = combine(Y, Q, Wt, phi)
    alpha, sigma = memberships(Q, phi)
    assert (sigma[:8] < phi).all() and (sigma[16:] > phi).any()
    for i in (3, 9, 40):
        u = [float(Q[m, i]) if Q[m, i] > 0 else 0.0 for m in range(M)]
        s = u[0]
        for m in range(1, M):
            s = s + u[m]
        d = s if s > phi else phi
        a = [1.0 - s / d] + [v / d for v in u]
        assert a == list(alpha[:, i])
        acc = None
        for l in range(L):
            w = a[0] * Wt[0, l]
            for m in range(1, M + 1):
                w = w + a[m] * Wt[m, l]
            t = w * float(Y[l, i])
            acc = t if acc is None else acc + t
        assert acc == y[i]
    assert np.abs(alpha.sum(0) - 1.0).max() <= 1e-15
    assert (alpha >= 0).all()
    w = rng.normal(size=L)
    y1 = combine(Y, Q[:1], np.stack([w, w]), phi)
    glob = (w[:, None] * Y.astype(np.float64)).sum(0)
    assert np.abs(y1 - glob).max() <= 1e-14 * np.abs(w[:, None] * Y).sum(0).max()


def test_restatement_is_continuous_where_the_spreads_pass_through_zero():
    """q scaled through zero (all spreads <= 0 on one side, the case a hard 'no influence' branch made discontinuous): y
    changes by O(delta)"""
    rng = np.random.default_rng(11)
    L, M, n, phi = 4, 2, 256, 0.05
    Y = (rng.normal(size=(L, n)) * 40).astype(np.float32)
    Q = np.abs(rng.normal(size=(M, n))).astype(np.float32)
    Wt = np.array([[1.0, 1, 1, 1], [4, 3, 2, 1], [0.5, 0.5, 1, 1]])
    y0 = combine(Y, Q * np.float32(0), Wt, phi)  # no influence at all: the background row
    assert np.array_equal(y0, combine(Y, -Q, Wt, phi))
    scale = np.abs(Y).sum(0).max() * np.abs(Wt).max()
    for delta in (1e-3, 1e-5, 1e-7):
        for sign in (1.0, -1.0):
            y = combine(Y, Q * np.float32(sign * delta), Wt, phi)
            # alpha_m <= delta |q| / phi and 1 - alpha_0 <= M delta |q| / phi: the weights move by at most 2 M delta max|q| / phi
            assert np.abs(y - y0).max() <= 2 * M * delta * float(Q.max()) / phi * scale
    # and across the floor itself: sigma either side of phi
    for eps in (1e-6, -1e-6):
        Qf = np.full((1, n), np.float32(phi * (1 + eps)))
        assert np.abs(combine(Y, Qf, Wt[:2], phi) - combine(Y, np.full((1, n), np.float32(phi)), Wt[:2], phi)).max() <= 1e-5 * scale


def test_region_edits_are_declared_exported_and_mirrored(nle):
    hdr = " ".join(open(os.path.join(ROOT, "include", "nle.h")).read().split())
    for decl in ("int nle_region_combine(nle_ctx* ctx, const float* d_layers, int L, const float* d_q, int M, long long n, "
                 "long long layer_stride, long long q_stride, const double* h_weights, double floor, int out_kind, "
                 "void* d_out);",
                 "int nle_region_spread(nle_filter* f, const float* d_strokes, int M, int H, int W, const double* h_scale, "
                 "double spread, float* d_q);",
                 "int nle_apply_regions(nle_filter* f, const float* d_x, int H, int W, int L, const float* d_strokes, int M, "
                 "const double* h_scale, double spread, double floor, const double* h_weights, int out_kind, void* d_out);",
                 "#define NLE_REGION_MAX 8", "#define NLE_REGION_LAYERS_MAX 16"):
        assert decl in hdr, decl
    from nle_amd import _abi
    assert (_abi.NLE_REGION_MAX, _abi.NLE_REGION_LAYERS_MAX) == (8, 16) == (nle.REGION_MAX, nle.REGION_LAYERS_MAX)
    assert (_abi.NLE_REGION_OUT_F32, _abi.NLE_REGION_OUT_ROUNDED8, _abi.NLE_REGION_OUT_U8) == (F32, ROUNDED8, U8)
    for name in ("nle_region_combine", "nle_region_spread", "nle_apply_regions"):
        assert name in _abi.SIGNATURES and name in nle.EXPORTED_SYMBOLS
        assert hasattr(nle.lib(), name)  # exported by the built library
    assert callable(getattr(nle.Context, "region_combine", None))
    assert callable(getattr(nle.NLEFilter, "region_spread", None)) and callable(getattr(nle.NLEFilter, "apply_regions", None))
    assert "Image enhanceRegions(" in open(os.path.join(ROOT, "include", "nle", "filter.hpp")).read()


NINE = [v for k in range(9) for v in ("--region", f"m{k}.png:1,2,3,4")]


@pytest.mark.parametrize("lead", [["--region", "m.png"], ["--region", "m.png:"], ["--region", ":1,2,3,4"],
                                  ["--region", "m.png:1,2,x,4"], ["--region", "m.png:1,,3,4"], ["--region", "m.png:1,2,3,nan"],
                                  ["--region", "m.png:1,2,3"], ["--region", "m.png:1,2,3,4,5"], NINE,
                                  ["--region-spread", "4"], ["--region-floor", "0.05"],
                                  ["--region", "m.png:1,2,3,4", "--region-spread", "0"],
                                  ["--region-spread", "-1", "--region", "m.png:1,2,3,4"],
                                  ["--region", "m.png:1,2,3,4", "--region-spread", "inf"],
                                  ["--region", "m.png:1,2,3,4", "--region-floor", "nan"],
                                  ["--region", "m.png:1,2,3,4", "--region-floor", "0"],
                                  ["--region", "m.png:1,2,3,4", "--region-floor", "tiny"]],
                         ids=lambda v: "_".join(v[:4]).replace("--", ""))
def test_cli_refuses_bad_region_options_before_any_gpu_call(lead, tmp_path):
    # HIP_VISIBLE_DEVICES=-1: no device is visible -- the refusal must not need one
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = tmp_path / "o.png"
    r = subprocess.run([ENHANCE] + lead + [FLOWER_BMP, str(out)] + FLOWER_ARGS, capture_output=True, text=True, timeout=60,
                       env=env)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "--region" in r.stderr
    assert r.stdout == "" and not out.exists()


@pytest.mark.parametrize("what", ["missing", "empty", "size"])
def test_cli_refuses_a_bad_mask_before_any_gpu_call(what, tmp_path):
    """a mask that cannot be read, marks no pixel, or is not of the image's size"""
    from PIL import Image
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    H, W = tpa._load_bgr("flower-50.bmp").shape[:2]
    mask = tmp_path / "m.png"
    if what != "missing":
        m = np.zeros((H, W - 1 if what == "size" else W, 3), dtype=np.uint8)
        m[:4, :4] = 255 if what == "size" else 127
        Image.fromarray(m).save(str(mask))
    out = tmp_path / "o.png"
    r = subprocess.run([ENHANCE, "--region", f"{mask}:4,3,2,1", FLOWER_BMP, str(out)] + FLOWER_ARGS, capture_output=True,
                       text=True, timeout=60, env=env)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "--region mask" in r.stderr
    assert r.stdout == "" and not out.exists()


@pytest.mark.parametrize("lead", [["--region", "m.png:2"], ["--region-spread", "4"], ["--region-floor", "0.05"]],
                         ids=lambda v: v[0].replace("--", ""))
def test_denoise_cli_refuses_region_options_before_any_gpu_call(lead, tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = tmp_path / "o.png"
    r = subprocess.run([DENOISE] + lead + [FLOWER_BMP, str(out)] + DENOISE_ARGS, capture_output=True, text=True, timeout=60,
                       env=env)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "--region" in r.stderr
    assert r.stdout == "" and not out.exists()


# ------------------------------------------------------------------------------------------------------ GPU tests
@pytest.fixture
def rctx(ctx):
    """the session ctx, handed back with the reference's affinity and auto mode whatever the test did"""
    yield ctx
    ctx.set_patch_radius(0)
    ctx.set_mode(0)


def _kernel_inputs(L, M, n, phi, seed):
    """random planes that reach every branch of the rule: mixed signs, all negative, zeros, NaN, sigma under the floor, equal
    to it and far above it; and pixels whose y is an exact half-integer (rounding ties of the 8-bit kinds): region 1 alone
    has influence there, so alpha_1 = u / u = 1 and alpha_0 = 0 exactly, Wt[1] = (1, 0, ..) and Y_0 = k + 1/2"""
    rng = np.random.default_rng(seed)
    Y = (rng.normal(size=(L, n)) * 60 + 100).astype(np.float32)
    Q = (rng.normal(size=(M, n)) * 0.5).astype(np.float32)
    Wt = rng.integers(-8, 9, size=(M + 1, L)) / 4.0
    Wt[1] = 0.0
    Wt[1, 0] = 1.0
    i = np.arange(n)
    Q[:, i % 8 == 1] = -np.abs(Q[:, i % 8 == 1]) - np.float32(0.1)
    Q[:, i % 8 == 2] = 0.0
    Q[:, i % 8 == 4] = np.abs(Q[:, i % 8 == 4])
    Q[M // 2, i % 8 == 4] = np.nan
    Q[:, i % 8 == 5] = -1.0
    Q[0, i % 8 == 5] = np.float32(phi)  # sigma == phi exactly (phi is an fp32 value): the `>` is false, d = phi
    Q[:, i % 8 == 6] = np.abs(Q[:, i % 8 == 6]) * np.float32(0.02 / M)
    Q[:, i % 8 == 7] = np.abs(Q[:, i % 8 == 7]) * np.float32(50)
    tie = i % 7 == 3
    Q[:, tie] = -0.5
    Q[0, tie] = 2.0
    Y[:, tie] = 0.0
    levels = rng.integers(-4, 300, size=int(tie.sum()))
    levels[:2] = (-4, 299)[:levels.size]  # both saturations
    Y[0, tie] = (levels + 0.5).astype(np.float32)
    return Y, Q, Wt, tie


def _strided(torch, rows, stride, offset, device):
    """a (len(rows), n) view with the given row stride and storage offset, holding `rows`; the rest of the buffer is NaN"""
    k, n = rows.shape
    buf = torch.full((offset + k * stride + 8,), float("nan"), dtype=torch.float32, device=device)
    view = torch.as_strided(buf, (k, n), (stride, 1), offset)
    view.copy_(torch.as_tensor(rows, device=device))
    return view


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 257, 4099])
@pytest.mark.parametrize("LM", [(1, 1), (4, 3), (16, 8)], ids=lambda v: f"L{v[0]}M{v[1]}")
def test_region_combine_is_the_restatement_bit_for_bit(nle, ctx, LM, n):
    import torch
    L, M = LM
    phi = float(np.float32(0.05))
    Y, Q, Wt, tie = _kernel_inputs(L, M, n, phi, seed=1000 * L + n)
    y = combine(Y, Q, Wt, phi)
    alpha, sigma = memberships(Q, phi)
    if n >= 257:  # the inputs reach what they are meant to reach
        assert (sigma == phi).any() and (sigma < phi).any() and (sigma > phi).any() and np.isnan(Q).any()
        assert tie.any() and np.array_equal(y[tie] - np.floor(y[tie]), np.full(int(tie.sum()), 0.5))
        assert (y[tie] < 0).any() and (y[tie] > 255).any()
    dev = f"cuda:{ctx.device}"
    pad = (n + 3) & ~3
    odd = n + 1 if (n + 1) % 4 else n + 2
    # layouts: 16-byte aligned planes (four pixels per thread, the last n mod 4 one at a time), and a base pointer offset
    # by one float with a plane stride that is no multiple of 4 (one pixel at a time throughout)
    for name, stride, off in (("aligned", pad, 0), ("offset", odd, 1)):
        Yd, Qd = _strided(torch, Y, stride, off, dev), _strided(torch, Q, stride, off, dev)
        for kind in (F32, ROUNDED8, U8):
            want = stored(y, kind)
            runs = []
            for _ in range(2):
                buf = torch.zeros(n + 8, dtype=torch.uint8 if kind == U8 else torch.float32, device=dev)
                out = buf[off:off + n]
                ctx.region_combine(Yd, Qd, Wt, phi, kind, out=out)
                torch.cuda.synchronize()
                got = buf.cpu().numpy()
                assert not got[:off].any() and not got[off + n:].any()  # nothing written either side of the plane
                runs.append(got[off:off + n])
            assert np.array_equal(runs[0], runs[1]), (name, kind)
            if kind == F32:
                assert np.array_equal(runs[0].view(np.uint32), want.view(np.uint32)), (name, kind)
            else:
                assert np.array_equal(runs[0], want), (name, kind)


def _train(nle, ctx, x, params):
    nr, nc, hx, hy, T, K = params
    return nle.NLEFilter(ctx).train_filter(np.asarray(x, dtype=np.float32), nr, nc, hx, hy, T, K)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["auto_tables", "materialised_f64", "patch_r1"])
def test_region_spread_meets_the_per_layer_bar(nle, oracle, rctx, form):
    H, W, nr, nc, hx, hy, T, K, _ = SYNTH
    x, V, S, strokes, scale = _synth(oracle)
    if form == "patch_r1":
        V, S, _ = tpa._restated(oracle, ("synthetic", 1), x, nr, nc, hx, hy, T, K, 1)
        rctx.set_patch_radius(1)
    rctx.set_mode(nle.MODE_MATERIALISED_F64 if form == "materialised_f64" else nle.MODE_AUTO)
    Q_o = restated_spread(oracle, V, S, strokes, scale, SPREAD)
    f = _train(nle, rctx, x, (nr, nc, hx, hy, T, K))
    assert f.diag()["formulation"] == (nle.MODE_PHI_FREE if form == "auto_tables" else nle.MODE_MATERIALISED_F64)
    Q = f.region_spread(strokes, scale, SPREAD).cpu().numpy()
    # scale None is c_m = 1, and the scale rides in fS: the same plane up to the rounding of one product
    Q1 = f.region_spread(strokes, None, SPREAD).cpu().numpy()
    f.close()
    errs = [rel_l2(Q[m], Q_o[m]) for m in range(3)]
    print(f"{form}: spread planes against the restatement, relative L2", ["%.2e" % e for e in errs],
          "mass sum q / sum s", ["%.4f" % (Q[m].sum() / (scale[m] * 25)) for m in range(3)])
    assert max(errs) <= PER_LAYER_TOL
    assert max(rel_l2(Q1[m] * scale[m], Q[m]) for m in range(3)) <= 1e-6


# max |alpha - alpha restated| measured on the MI355X (printed by the test below): 0 on the synthetic
# plane for M = 1, 2 and 3 (every fp32 spread value equals the restatement's), 1.27e-08 on flower (spread values one fp32
# ulp apart).  The assertion is 10 x the largest.
ALPHA_MEASURED = 1.27e-8
ALPHA_TOL = 10 * ALPHA_MEASURED
assert ALPHA_TOL <= 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("synth", 1), ("synth", 2), ("synth", 3), ("flower", 2)], ids=lambda c: f"{c[0]}-M{c[1]}")
def test_apply_regions_against_the_restatement(nle, oracle, rctx, case):
    key, M = case
    L = 4
    x, V, S, strokes, scale = _synth(oracle) if key == "synth" else _flower(oracle)
    Q_o, Y_o, y_o = _restated_edit(oracle, key, M, L)
    alpha_o, sigma_o = memberships(Q_o, FLOOR)
    under = float((sigma_o < FLOOR).mean())
    print(f"{key} M = {M}: {100 * under:.2f} % of the pixels are under the floor in the restatement")
    if key == "synth":  # both branches of the rule run (44 %, 19 % and 0.01 % in the restatement)
        assert under > 0.10 if M < 3 else under < 0.01
    params = SYNTH[2:8] if key == "synth" else (FLOWER["nr"], FLOWER["nc"], FLOWER["hx"], FLOWER["hy"], FLOWER["T"], FLOWER["K"])
    f = _train(nle, rctx, x, params)
    assert f.diag()["formulation"] == nle.MODE_PHI_FREE  # auto mode: the tables
    y = f.apply_regions(x, L, strokes[:M], WT[:M + 1, :L], scale[:M], SPREAD, FLOOR, F32).cpu().numpy()
    Q = f.region_spread(strokes[:M], scale[:M], SPREAD).cpu().numpy()
    f.close()
    alpha, _ = memberships(Q, FLOOR)
    d_alpha = float(np.abs(alpha - alpha_o).max())
    err = rel_l2(y, y_o)
    print(f"{key} M = {M}: y against the restatement, relative L2 {err:.2e}; max |alpha - alpha restated| {d_alpha:.2e}")
    assert err <= PER_LAYER_TOL
    assert d_alpha <= ALPHA_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["auto_tables", "materialised_f64"])
def test_apply_regions_is_its_three_calls_and_its_kinds_agree(nle, oracle, rctx, form):
    H, W, nr, nc, hx, hy, T, K, L = SYNTH
    x, _, _, strokes, scale = _synth(oracle)
    rctx.set_mode(nle.MODE_MATERIALISED_F64 if form == "materialised_f64" else nle.MODE_AUTO)
    f = _train(nle, rctx, x, (nr, nc, hx, hy, T, K))
    M = 3
    Wt = WT[:M + 1, :L]
    y = {k: f.apply_regions(x, L, strokes, Wt, scale, SPREAD, FLOOR, k).cpu().numpy() for k in (F32, ROUNDED8, U8)}
    layers = f.apply_layers(x.astype(np.float32), L)
    q = f.region_spread(strokes, scale, SPREAD)
    composed = rctx.region_combine(layers, q, Wt, FLOOR, F32).cpu().numpy()
    assert np.array_equal(composed.view(np.uint32), y[F32].view(np.uint32))
    assert np.array_equal(y[ROUNDED8], y[U8].astype(np.float32))
    assert np.array_equal(y[U8], stored(y[F32].astype(np.float64), U8))  # nle_apply_u8's rounding rule on the F32 plane
    assert len(np.unique(y[U8])) > 16
    # M = 1 with equal rows: the global edit, whatever the memberships are
    w = np.array([2.0, 3.0, 4.0, 1.0])
    y1 = f.apply_regions(x, L, strokes[:1], np.stack([w, w]), scale[:1], SPREAD, FLOOR, F32).cpu().numpy().astype(np.float64)
    Yl = layers.cpu().numpy().astype(np.float64)
    glob = (w[:, None] * Yl).sum(0)
    # alpha_0 + alpha_1 = 1 to an ulp of fp64, y is rounded to fp32 once: 2^-24 relative per pixel, far inside 1e-6
    e1 = rel_l2(y1, glob)
    e2 = rel_l2(y1, f.apply(x, oracle.transform_eigenvalues(f.eigvals, w)).cpu().numpy())
    print(f"{form}: M = 1, equal rows: against sum w_l layers {e1:.2e}, against apply(transform_eigenvalues(w)) {e2:.2e}")
    f.close()
    assert e1 <= 1e-6
    assert e2 <= 1e-4


def _null(nle, f, ctx, x, strokes, Wt, which):
    """nle_apply_regions with one pointer NULL"""
    import torch
    xs = torch.as_tensor(x, dtype=torch.float32, device=f"cuda:{ctx.device}")
    ss = torch.as_tensor(strokes, dtype=torch.float32, device=xs.device).contiguous()
    out = torch.empty(xs.numel(), dtype=torch.float32, device=xs.device)
    torch.cuda.synchronize()
    w = np.ascontiguousarray(Wt, dtype=np.float64)
    p = {"x": C.c_void_p(xs.data_ptr()), "strokes": C.c_void_p(ss.data_ptr()), "weights": w.ctypes.data_as(C.c_void_p),
         "out": C.c_void_p(out.data_ptr())}
    p[which] = None
    H, W = xs.shape
    return nle.lib().nle_apply_regions(f._f, p["x"], H, W, w.shape[1], p["strokes"], ss.shape[0], None, SPREAD, FLOOR,
                                       p["weights"], F32, p["out"])


@pytest.mark.gpu
def test_region_refusals_leave_the_ctx_usable(nle, oracle, rctx):
    import torch
    H, W, nr, nc, hx, hy, T, K, L = SYNTH
    x, V, S, strokes, scale = _synth(oracle)
    f = _train(nle, rctx, x, (nr, nc, hx, hy, T, K))
    fS = oracle.transform_eigenvalues(S, [2.0, 3.0, 4.0, 1.0])
    want = oracle.apply_filter(V, x, fS).ravel()

    def still_fine(flt=f):
        assert rel_l2(flt.apply(x, oracle.transform_eigenvalues(flt.eigvals, [2.0, 3.0, 4.0, 1.0])).cpu().numpy(), want) <= PER_LAYER_TOL

    def refused(fn):
        with pytest.raises(nle.NLEError) as e:
            fn()
        assert e.value.code == nle.NLE_ERR_INVALID and str(e.value)
        print("refused:", e.value)
        still_fine()

    def edit(M=2, L=4, spread=SPREAD, floor=FLOOR, kind=F32, plane=x, s=None, sc=None):
        s = np.zeros((M, H, W), dtype=np.float32) if s is None else s
        return f.apply_regions(plane, L, s, np.ones((M + 1, L)), sc, spread, floor, kind)

    refused(lambda: edit(M=0))
    refused(lambda: edit(M=nle.REGION_MAX + 1))
    refused(lambda: edit(L=0))
    refused(lambda: edit(L=nle.REGION_LAYERS_MAX + 1))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(lambda: edit(spread=bad))
        refused(lambda: edit(floor=bad))
        refused(lambda: f.region_spread(strokes, scale, bad))
        refused(lambda: rctx.region_combine(torch.zeros((2, 8), device="cuda"), torch.zeros((1, 8), device="cuda"),
                                            np.ones((2, 2)), bad, F32))
    refused(lambda: edit(sc=np.array([1.0, float("nan")])))
    refused(lambda: edit(kind=3))
    refused(lambda: edit(kind=-1))
    refused(lambda: edit(plane=x[:-1], s=np.zeros((2, H - 1, W), dtype=np.float32)))  # H W is not the filter's
    refused(lambda: f.region_spread(strokes[:, :-1], scale, SPREAD))
    refused(lambda: f.region_spread(np.zeros((nle.REGION_MAX + 1, H, W), dtype=np.float32), None, SPREAD))
    refused(lambda: rctx.region_combine(torch.zeros((17, 8), device="cuda"), torch.zeros((1, 8), device="cuda"),
                                        np.ones((2, 17)), FLOOR, F32))
    refused(lambda: rctx.region_combine(torch.zeros((2, 8), device="cuda"), torch.zeros((9, 8), device="cuda"),
                                        np.ones((10, 2)), FLOOR, F32))
    refused(lambda: rctx.region_combine(torch.zeros((2, 8), device="cuda"), torch.zeros((1, 8), device="cuda"),
                                        np.ones((2, 2)), FLOOR, 7))
    for which in ("x", "strokes", "weights", "out"):
        assert _null(nle, f, rctx, x, strokes, WT, which) == nle.NLE_ERR_INVALID
        assert nle.lib().nle_last_error(rctx._h)
        still_fine()
    assert nle.lib().nle_region_combine(rctx._h, None, 1, None, 1, 8, 8, 8, None, FLOOR, F32, None) == nle.NLE_ERR_INVALID
    assert nle.lib().nle_region_spread(f._f, None, 1, H, W, None, SPREAD, None) == nle.NLE_ERR_INVALID
    still_fine()
    # and the call that is not refused still gives the edit
    y = f.apply_regions(x, L, strokes, WT, scale, SPREAD, FLOOR, F32).cpu().numpy()
    assert rel_l2(y, _restated_edit(oracle, "synth", 3)[2]) <= PER_LAYER_TOL
    f.close()
    # world > 1: refused before any collective -- a shard of two whose all-reduce must never be called
    calls = []
    s = nle.Context(0)
    try:
        g = _train(nle, s, x, (nr, nc, hx, hy, T, K))
        s.set_shard(0, 2, 48, lambda t: calls.append(1))
        for fn in (lambda: g.apply_regions(x, L, strokes, WT, scale, SPREAD, FLOOR, F32),
                   lambda: g.region_spread(strokes, scale, SPREAD)):
            with pytest.raises(nle.NLEError) as e:
                fn()
            assert e.value.code == nle.NLE_ERR_INVALID and "world" in str(e.value) and not calls
        assert nle.lib().nle_ctx_set_shard(s._h, 0, 1, nle.ALLREDUCE_FN(0), None, None, 0) == 0
        still_fine(g)
        assert not calls
        g.close()
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------ CLI
def _write_masks(tmp_path, H, W):
    from PIL import Image
    paths = []
    for k, (r, c) in enumerate(FLOWER_CORNERS):
        m = np.zeros((H, W), dtype=np.uint8)
        m[r:r + 9, c:c + 9] = 255
        p = tmp_path / f"m{k + 1}.png"
        Image.fromarray(np.stack([m, m, m], axis=-1)).save(str(p))
        paths.append(str(p))
    return paths


@pytest.mark.gpu
def test_enhance_with_regions_matches_the_python_mirror(nle, oracle, rctx, tmp_path):
    from PIL import Image
    src = tpa._load_bgr("flower-50.bmp")
    H, W = src.shape[:2]
    m1, m2 = _write_masks(tmp_path, H, W)
    out = tmp_path / "out.png"
    r = subprocess.run([ENHANCE, "--region", f"{m1}:4,3,2,1", "--region", f"{m2}:0.5,0.5,1,1", "--region-spread", "4",
                        FLOWER_BMP, str(out)] + FLOWER_ARGS, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    got = np.asarray(Image.open(str(out)).convert("RGB"))[..., ::-1]
    # the same calls through the Python mirror: bgr2lab8 -> train -> apply_regions(ROUNDED8) -> lab2bgr8
    lab, L = rctx.bgr2lab8(src)
    f = nle.NLEFilter(rctx).train_filter(L, FLOWER["nr"], FLOWER["nc"], FLOWER["hx"], FLOWER["hy"], FLOWER["T"], FLOWER["K"])
    strokes = boxes(H, W, FLOWER_CORNERS, 9)
    scale = np.array([H * W / float(s.astype(np.float64).sum()) for s in strokes])
    Wt = np.array([FLOWER["weights"], [4.0, 3.0, 2.0, 1.0], [0.5, 0.5, 1.0, 1.0]])
    y = f.apply_regions(L, 4, strokes, Wt, scale, 4.0, FLOOR, ROUNDED8)
    plain = f.apply_rounded8(L, oracle.transform_eigenvalues(f.eigvals, FLOWER["weights"]))
    f.close()
    mirror = rctx.lab2bgr8(lab, L=y.view(H, W)).cpu().numpy()
    assert np.array_equal(got, mirror)
    # and it is an edit of its own: not what the global weights give
    assert not np.array_equal(mirror, rctx.lab2bgr8(lab, L=plain.view(H, W)).cpu().numpy())
