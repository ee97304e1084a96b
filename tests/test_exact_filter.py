"""The exact (Nystrom-free) filter: NLE_MODE_EXACT_F64 / nle_affinity_product64 / NLEFilter::exact / `--exact`.

The restatement below is the definition of include/nle.h in numpy: the dense K (sw = 1/hx^2, pw = 1/hy^2,
K_ij = exp(-sw (dr^2 + dc^2) - pw dy^2)), the reference's Sinkhorn order with inplaceReciprocal (r = 1; T times
c = recip(K r), r = recip(K c)), W = diag(r) K diag(c), Ws = (W + W^T) / 2, the min(K, N) largest eigenpairs of Ws by `eigh`,
the leading run >= 1e-10 kept, each eigenvector's entry of largest magnitude made positive (ties: the lowest index)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, rel_l2

ENHANCE = os.path.join(ROOT, "nonlocal-image-edit_amd", "bin", "enhance")
DENOISE = os.path.join(ROOT, "nonlocal-image-edit_amd", "bin", "denoise")
FLOWER = dict(nr=10, nc=20, hx=100.0, hy=30.0, T=50, K=30, weights=[2.0, 3.0, 4.0, 1.0])  # README.md:74
FLOWER_ARGS = ["10", "20", "100", "30", "50", "30", "2", "3", "4", "1"]
DENOISE_ARGS = ["10", "20", "100", "30", "10", "30", "10", "10", "2"]
EPS = 1e-10


# ----------------------------------------------------------------------------------------------- the restatement
def dense_K(y, hx, hy):
    y = np.asarray(y, dtype=np.float32).astype(np.float64)
    H, W = y.shape
    N = H * W
    f = y.ravel()
    rr = np.arange(N, dtype=np.int64) // W
    cc = np.arange(N, dtype=np.int64) % W
    sw, pw = 1.0 / (hx * hx), 1.0 / (hy * hy)
    d2 = ((rr[:, None] - rr[None]) ** 2 + (cc[:, None] - cc[None]) ** 2).astype(np.float64)
    dy = f[:, None] - f[None]
    return np.exp(-sw * d2 - pw * (dy * dy))


def inplace_reciprocal(v):
    out = np.zeros_like(v)
    m = np.abs(v) >= EPS
    out[m] = 1.0 / v[m]
    return out


def sign_rule(V):
    V = V.copy()
    for k in range(V.shape[1]):
        i = int(np.argmax(np.abs(V[:, k])))  # first maximum: the lowest index on ties
        if V[i, k] < 0:
            V[:, k] = -V[:, k]
    return V


def restatement(y, hx, hy, T, K):
    """(kept eigenvalues, their eigenvectors N x K', all eigenvalues descending) of the exact filter"""
    Kf = dense_K(y, hx, hy)
    N = Kf.shape[0]
    r = np.ones(N)
    for _ in range(T):
        c = inplace_reciprocal(Kf @ r)
        r = inplace_reciprocal(Kf @ c)
    Wm = r[:, None] * Kf * c[None]
    del Kf
    Ws = (Wm + Wm.T) / 2
    del Wm
    w, V = np.linalg.eigh(Ws)
    order = np.argsort(w)[::-1]
    w, V = w[order], V[:, order]
    top = w[:min(K, N)]
    kept = 0
    while kept < top.size and top[kept] >= EPS:
        kept += 1
    return w[:kept].copy(), sign_rule(V[:, :kept]), w


def layers(oracle, w, V, y, L):
    f = np.asarray(y, dtype=np.float32).astype(np.float64).ravel()
    resp = oracle.layer_responses(w, L)
    t = V.T @ f
    return np.stack([V @ (resp[j] * t) for j in range(L)])


def _load_bgr(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))[..., ::-1].copy()


def crossing_plane():
    """four levels 60 apart and a spatial bandwidth far beyond the plane: K has rank 4 up to rounding, so the spectrum of Ws
    falls from ~1e-2 to ~1e-16 across the cut at 1e-10"""
    rr, cc = np.mgrid[0:6, 0:8]
    return (60.0 * ((rr + cc) % 4)).astype(np.float64)


# ------------------------------------------------------------------------------------------------------ CPU tests
def test_mode_constant_is_declared_exported_and_mirrored(nle):
    hdr = open(os.path.join(ROOT, "include", "nle.h")).read()
    assert "#define NLE_MODE_EXACT_F64 6" in hdr and "#define NLE_EXACT_MAX_PIXELS 1048576" in hdr
    assert "int nle_affinity_product64(nle_ctx* ctx, const float* d_lum, int H, int W, double hx, double hy" in hdr
    from nle_amd import _abi
    assert _abi.NLE_MODE_EXACT_F64 == 6 and nle.MODE_EXACT_F64 == 6 and nle.EXACT_MAX_PIXELS == 1 << 20
    assert "nle_affinity_product64" in _abi.SIGNATURES and "nle_affinity_product64" in nle.EXPORTED_SYMBOLS
    assert hasattr(nle.lib(), "nle_affinity_product64")
    assert callable(getattr(nle.Context, "affinity_product64", None))
    assert "bool exact = false;" in open(os.path.join(ROOT, "include", "nle", "filter.hpp")).read()


def test_restatement_sign_rule_and_cut():
    V = np.array([[0.5, -0.6], [-0.5, 0.6], [0.7, 0.1]])
    S = sign_rule(V)
    assert np.array_equal(S[:, 0], V[:, 0]) and np.array_equal(S[:, 1], -V[:, 1])  # column 1: tie 0.6 / 0.6 -> index 0
    w, Vk, wall = restatement(crossing_plane(), 1e9, 30.0, 10, 8)
    assert w.size == 4 and wall[3] > 1e-4 and abs(wall[4]) < 1e-12
    assert np.allclose(Vk.T @ Vk, np.eye(4), atol=1e-12)


@pytest.mark.parametrize("tool", [ENHANCE, DENOISE], ids=["enhance", "denoise"])
@pytest.mark.parametrize("lead", [["--exact", "--patch-radius", "2"], ["--exact", "--sampler", "farthest"],
                                  ["--patch-radius", "2", "--exact"], ["--exact=1"]],
                         ids=["radius", "farthest", "radius_first", "value"])
def test_cli_refuses_exact_combinations_before_any_gpu_call(tool, lead, tmp_path):
    # HIP_VISIBLE_DEVICES=-1: no device is visible -- the refusal must not need one
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = tmp_path / "o.png"
    args = DENOISE_ARGS if tool == DENOISE else FLOWER_ARGS
    r = subprocess.run([tool] + lead + [os.path.join(GOLDEN, "flower-50.bmp"), str(out)] + args, capture_output=True,
                       text=True, timeout=60, env=env)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "--exact" in r.stderr
    assert r.stdout == "" and not out.exists()


# ------------------------------------------------------------------------------------------------------ GPU tests
@pytest.fixture(scope="module")
def ectx(nle):
    """a context of this module's own"""
    c = nle.Context(0)
    yield c
    c.close()


def train(nle, ctx, y, hx, hy, T, K, L=4, nr=2, nc=2):
    ctx.set_mode(nle.MODE_EXACT_F64)
    try:
        f = nle.NLEFilter(ctx).train_filter(np.asarray(y, dtype=np.float32), nr, nc, hx, hy, T, K)
    finally:
        ctx.set_mode(nle.MODE_AUTO)
    Y = f.apply_layers(np.asarray(y, dtype=np.float32), L).cpu().numpy().astype(np.float64)
    return f, Y


_KPLANES = {
    "64x64": (lambda o: o.synthetic_luminance(64, 64), 20.0, 30.0),
    "37x53": (lambda o: o.synthetic_luminance(37, 53), 9.0, 25.0),
    "1x3000": (lambda o: o.synthetic_luminance(1, 3000), 300.0, 30.0),
    "3000x1": (lambda o: o.synthetic_luminance(3000, 1), 300.0, 30.0),
}
_kcache = {}


@pytest.mark.gpu
@pytest.mark.parametrize("plane", list(_KPLANES))
@pytest.mark.parametrize("ncols", [1, 2, 3, 16, 17, 64, 130])
def test_affinity_product_matches_dense_K(nle, oracle, ectx, plane, ncols):
    make, hx, hy = _KPLANES[plane]
    if plane not in _kcache:
        y = make(oracle)
        _kcache[plane] = (y, dense_K(y, hx, hy))
    y, Kd = _kcache[plane]
    X = np.random.default_rng(ncols).standard_normal((Kd.shape[0], ncols))
    Y = ectx.affinity_product64(y.astype(np.float32), X, hx, hy).cpu().numpy()
    want = Kd @ X
    errs = [rel_l2(Y[:, j], want[:, j]) for j in range(ncols)]
    assert max(errs) <= 1e-12, max(errs)
    assert np.array_equal(Y, ectx.affinity_product64(y.astype(np.float32), X, hx, hy).cpu().numpy())  # deterministic


def _parity_cases(oracle):
    flower = np.load(os.path.join(GOLDEN, "flower_cfg1.npz"))["L_in"].astype(np.float64)[100:160, 150:240]
    bird = oracle.bgr_to_lab8(_load_bgr(os.path.join(GOLDEN, "readme", "bird.bmp")))[..., 0].astype(np.float64)[200:260, 150:240]
    return {
        "flower_crop": (flower, 6, 9, 100.0, 30.0, 50, 30, 4),
        "synthetic": (oracle.synthetic_luminance(48, 64), 6, 8, 12.0, 30.0, 10, 10, 4),
        "bird_crop": (bird, 6, 9, 1000.0, 20.0, 10, 9, 4),
    }


@pytest.fixture(scope="module")
def parity_refs(oracle):
    """the dense restatement of every parity case, computed once"""
    out = {}
    for name, (y, nr, nc, hx, hy, T, K, L) in _parity_cases(oracle).items():
        out[name] = restatement(y, hx, hy, T, K)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["flower_crop", "synthetic", "bird_crop"])
def test_exact_filter_matches_the_restatement(nle, oracle, ectx, parity_refs, case):
    y, nr, nc, hx, hy, T, K, L = _parity_cases(oracle)[case]
    w, V, wall = parity_refs[case]
    assert w.size == K and wall[K - 1] - wall[K] >= 1e-4  # well posed: the K-th pair is separated
    f, Y = train(nle, ectx, y, hx, hy, T, K, L, nr, nc)
    assert f.diag() == {"formulation": 6, "p": 0, "r_Ka": 0, "r_Wa": 0, "r_Q": K, "K": K, "chol_Ka": 0, "chol_Wa": 0}
    ev = f.eigvals
    assert ev.size == K and np.max(np.abs(ev - w)) <= 1e-9, np.max(np.abs(ev - w))
    Y_ref = layers(oracle, w, V, y, L)
    errs = [rel_l2(Y[j], Y_ref[j]) for j in range(L)]
    assert max(errs) <= 1e-6, errs
    Vg = f.eigvecs().cpu().numpy().astype(np.float64)[:, :K]
    checked = 0
    for k in range(K):
        left = np.inf if k == 0 else wall[k - 1] - wall[k]
        if min(left, wall[k] - wall[k + 1]) >= 1e-3:
            assert np.max(np.abs(Vg[:, k] - V[:, k])) <= 1e-6, k
            checked += 1
    assert checked >= 1
    msg = f"{case}: eigenvalues {np.max(np.abs(ev - w)):.1e}, per-layer " + str(["%.1e" % e for e in errs])
    if case == "flower_crop":  # what the feature is for: the grid Nystrom filter on the same crop
        f_g = nle.NLEFilter(ectx).train_filter(y.astype(np.float32), nr, nc, hx, hy, T, K)
        Y_g = f_g.apply_layers(y.astype(np.float32), L).cpu().numpy().astype(np.float64)
        msg += "; grid Nystrom against the exact filter per layer " + str(["%.4f" % rel_l2(Y_g[j], Y_ref[j]) for j in range(L)])
        f_g.close()
    print(msg)
    f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["small_K50", "crossing", "T1", "K1"])
def test_exact_filter_edge_cases(nle, oracle, ectx, case):
    y, hx, hy, T, K = {
        "small_K50": (oracle.synthetic_luminance(5, 7), 3.0, 30.0, 10, 50),
        "crossing": (crossing_plane(), 1e9, 30.0, 10, 8),
        "T1": (oracle.synthetic_luminance(40, 50), 10.0, 30.0, 1, 8),
        "K1": (oracle.synthetic_luminance(40, 50), 10.0, 30.0, 10, 1),
    }[case]
    w, V, wall = restatement(y, hx, hy, T, K)
    f, Y = train(nle, ectx, y, hx, hy, T, K)
    Kp = f.info()["K"]
    assert Kp == w.size, (Kp, w.size)
    if case == "small_K50":
        assert Kp <= 35
    if case == "crossing":
        assert Kp < K and wall[Kp - 1] >= 1e-9 and abs(wall[Kp]) <= 1e-11
    assert np.max(np.abs(f.eigvals - w)) <= 1e-9
    print(case, "K' =", Kp, "eigenvalue error %.1e" % np.max(np.abs(f.eigvals - w)))
    f.close()


@pytest.mark.gpu
def test_exact_filter_is_reproducible_and_its_forms_agree(nle, oracle, ectx):
    y = oracle.synthetic_luminance(48, 64)
    hx, hy, T, K, L = 12.0, 30.0, 10, 10, 4
    f1, Y1 = train(nle, ectx, y, hx, hy, T, K, L)
    f2, Y2 = train(nle, ectx, y, hx, hy, T, K, L)
    assert np.array_equal(f1.eigvals, f2.eigvals) and np.array_equal(Y1, Y2)
    ectx.set_mode(nle.MODE_EXACT_F64)
    try:
        fh = nle.NLEFilter(ectx).train_filter_host(y.astype(np.float32), 2, 2, hx, hy, T, K)
        fu = nle.NLEFilter(ectx).train_filter_host_u8(y.astype(np.uint8), 2, 2, hx, hy, T, K)
    finally:
        ectx.set_mode(nle.MODE_AUTO)
    H, W = y.shape
    for f in (fh, fu):
        assert np.array_equal(f.eigvals, f1.eigvals)
        assert np.array_equal(f.apply_layers(y.astype(np.float32), L).cpu().numpy().astype(np.float64), Y1)
        out = np.empty((L, H * W), dtype=np.float32)
        f.apply_layers_host(None, L, out)
        assert np.array_equal(out.astype(np.float64), Y1)
        fS = oracle.transform_eigenvalues(f.eigvals, [2.0, 3.0, 4.0, 1.0])
        u_host = np.empty(H * W, dtype=np.uint8)
        f.apply_u8_host(None, fS, u_host)
        assert np.array_equal(u_host, f1.apply_u8(y.astype(np.float32), fS).cpu().numpy().ravel())
    for f in (f1, f2, fh, fu):
        f.close()


@pytest.mark.gpu
def test_auto_mode_after_an_exact_train_is_unchanged(nle, oracle, ectx):
    y = oracle.synthetic_luminance(48, 64)
    args = (6, 8, 12.0, 30.0, 10, 10)
    f_e, _ = train(nle, ectx, y, 12.0, 30.0, 10, 10)
    f_e.close()
    ectx.set_mode(nle.MODE_AUTO)
    f_a = nle.NLEFilter(ectx).train_filter(y.astype(np.float32), *args)
    fresh = nle.Context(0)
    try:
        f_b = nle.NLEFilter(fresh).train_filter(y.astype(np.float32), *args)
        assert f_a.diag() == f_b.diag() and f_a.diag()["formulation"] != nle.MODE_EXACT_F64
        assert np.array_equal(f_a.eigvals, f_b.eigvals)
        assert np.array_equal(f_a.apply_layers(y.astype(np.float32), 4).cpu().numpy(),
                              f_b.apply_layers(y.astype(np.float32), 4).cpu().numpy())
        f_b.close()
    finally:
        fresh.close()
    f_a.close()


@pytest.mark.gpu
def test_exact_filter_refusals(nle, oracle):
    c = nle.Context(0)
    y = oracle.synthetic_luminance(30, 40)

    def refused(plane, K=5):
        with pytest.raises(nle.NLEError) as e:
            c.set_mode(nle.MODE_EXACT_F64)
            nle.NLEFilter(c).train_filter(np.asarray(plane, dtype=np.float32), 2, 2, 10.0, 30.0, 5, K)
        assert e.value.code == nle.NLE_ERR_INVALID
        print("refused:", e.value)

    try:
        c.set_patch_radius(2)
        refused(y)
        c.set_patch_radius(0)
        c.set_sampler(nle.SAMPLER_FARTHEST)
        refused(y)
        c.set_sampler(nle.SAMPLER_GRID)
        refused(y + 0.5)          # not integer valued
        refused(y, K=257)
        refused(np.zeros((1025, 1024)))
        f, _ = train(nle, c, y, 10.0, 30.0, 5, 5)  # still usable
        assert f.diag()["formulation"] == nle.MODE_EXACT_F64
        f.close()
    finally:
        c.close()
    calls = []
    s = nle.Context(0)
    try:
        s.set_shard(0, 2, 4, lambda t: calls.append(1) or pytest.fail("the all-reduce must not be called"))
        s.set_mode(nle.MODE_EXACT_F64)
        with pytest.raises(nle.NLEError) as e:
            nle.NLEFilter(s).train_filter(y.astype(np.float32), 2, 2, 10.0, 30.0, 5, 5)
        assert e.value.code == nle.NLE_ERR_INVALID and not calls
    finally:
        s.close()


@pytest.mark.gpu
def test_enhance_exact_matches_the_python_mirror(nle, oracle, ectx, tmp_path):
    from PIL import Image
    import torch
    src = _load_bgr(os.path.join(GOLDEN, "flower-50.bmp"))
    out = tmp_path / "flower-exact.png"
    r = subprocess.run([ENHANCE, "--exact", os.path.join(GOLDEN, "flower-50.bmp"), str(out)] + FLOWER_ARGS,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    got = np.asarray(Image.open(str(out)).convert("RGB"))[..., ::-1]
    # the same pipeline through the Python mirror: bgr2lab8 -> train_host_u8 (exact) -> apply_u8_host -> lab2bgr8
    H, W = src.shape[:2]
    lab, _ = ectx.bgr2lab8(src)
    L8 = lab[..., 0].cpu().numpy().copy()
    ectx.set_mode(nle.MODE_EXACT_F64)
    try:
        f = nle.NLEFilter(ectx).train_filter_host_u8(L8, FLOWER["nr"], FLOWER["nc"], FLOWER["hx"], FLOWER["hy"], FLOWER["T"],
                                                     FLOWER["K"])
    finally:
        ectx.set_mode(nle.MODE_AUTO)
    assert f.diag()["formulation"] == nle.MODE_EXACT_F64
    print("flower exact: K' =", f.info()["K"], "timings", f.timings())
    fS = oracle.transform_eigenvalues(f.eigvals, FLOWER["weights"])
    y8 = np.empty(H * W, dtype=np.uint8)
    f.apply_u8_host(None, fS, y8)
    f.close()
    Lf = torch.as_tensor(y8.reshape(H, W).astype(np.float32), device=lab.device)
    mirror = ectx.lab2bgr8(lab, L=Lf).cpu().numpy()
    assert np.array_equal(got, mirror)


@pytest.mark.gpu
def test_denoise_exact_runs(tmp_path):
    out = tmp_path / "flower-dn-exact.png"
    r = subprocess.run([DENOISE, "--exact", os.path.join(GOLDEN, "flower-50.bmp"), str(out)] + DENOISE_ARGS,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert out.exists() and out.stat().st_size > 0
