"""Farthest-point sample selection: nle_ctx_set_sampler / nle_sample_pixels / NLEFilter::sampler / `--sampler`.

The restatement below is the rule of include/nle.h, in numpy: p = the grid's sample count, s_0 = pixel (H/2, W/2),
D(i, j) = sw (double)(dr^2 + dc^2) + pw dy^2 (sw = 1/hx^2, pw = 1/hy^2, dr dc int64, dy = (double)y_i - (double)y_j, each
operation rounded on its own), m_i = min over the chosen samples of D(i, s) and -1 for a chosen pixel, s_k = argmax m
with ties to the smallest row-major index; the set is returned ascending.  The oracle comparisons replace
oracle.sample_pixels by (that set, its complement): every later stage is the oracle's own."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, rel_l2

ENHANCE = os.path.join(ROOT, "nonlocal-image-edit_amd", "bin", "enhance")
DENOISE = os.path.join(ROOT, "nonlocal-image-edit_amd", "bin", "denoise")
FLOWER = dict(nr=10, nc=20, hx=100.0, hy=30.0, T=50, K=30, weights=[2.0, 3.0, 4.0, 1.0])  # README.md:74
FLOWER_ARGS = ["10", "20", "100", "30", "50", "30", "2", "3", "4", "1"]
DENOISE_ARGS = ["10", "20", "100", "30", "10", "30", "10", "10", "2"]
PER_LAYER_TOL = 1e-4


# ----------------------------------------------------------------------------------------------- the restatement
def grid_count(oracle, H, W, nr, nc):
    sel_r, sel_c = oracle.sample_grid(H, W, nr, nc)
    return sel_r.size * sel_c.size


def farthest(y, p, hx, hy):
    """the p farthest-point samples of plane y (values taken as fp32, as the product reads them), ascending"""
    y = np.asarray(y, dtype=np.float32).astype(np.float64)
    H, W = y.shape
    N = H * W
    f = y.ravel()
    rr = np.arange(N, dtype=np.int64) // W
    cc = np.arange(N, dtype=np.int64) % W
    sw, pw = 1.0 / (hx * hx), 1.0 / (hy * hy)
    s = (H // 2) * W + W // 2
    chosen = [s]
    m = None
    for _ in range(p - 1):
        dr, dc = rr - rr[s], cc - cc[s]
        dy = f - f[s]
        d = sw * (dr * dr + dc * dc).astype(np.float64) + pw * (dy * dy)
        m = d if m is None else np.minimum(m, d)
        m[s] = -1.0
        s = int(np.argmax(m))  # first maximum: the smallest index on ties
        chosen.append(s)
    return np.sort(np.array(chosen, dtype=np.int64))


def farthest_brute(y, p, hx, hy):
    """the same rule from the full pairwise matrix D, one scalar comparison at a time"""
    y = np.asarray(y, dtype=np.float32).astype(np.float64)
    H, W = y.shape
    N = H * W
    sw, pw = 1.0 / (hx * hx), 1.0 / (hy * hy)
    D = np.empty((N, N))
    for i in range(N):
        for j in range(N):
            dr, dc = i // W - j // W, i % W - j % W
            dy = float(y.flat[i]) - float(y.flat[j])
            D[i, j] = sw * float(dr * dr + dc * dc) + pw * (dy * dy)
    chosen = [(H // 2) * W + W // 2]
    while len(chosen) < p:
        best, arg = -np.inf, -1
        for i in range(N):
            if i in chosen:
                continue
            v = min(D[i, s] for s in chosen)
            if v > best:
                best, arg = v, i
        chosen.append(arg)
    return np.sort(np.array(chosen, dtype=np.int64))


def use_set(monkeypatch, oracle, H, W, sel):
    """oracle.sample_pixels -> (sel, the rest), both ascending"""
    sel = np.asarray(sel, dtype=np.int64)
    keep = np.ones(H * W, dtype=bool)
    keep[sel] = False
    rest = np.arange(H * W)[keep]
    monkeypatch.setattr(oracle, "sample_pixels", lambda *a: (sel, rest))


def _load_bgr(name):
    from PIL import Image
    return np.asarray(Image.open(os.path.join(GOLDEN, name)).convert("RGB"))[..., ::-1].copy()


_cache = {}


def _flower_L(oracle):
    if "flowerL" not in _cache:
        _cache["flowerL"] = oracle.bgr_to_lab8(_load_bgr("flower-50.bmp"))[..., 0].astype(np.float64)
    return _cache["flowerL"]


# ------------------------------------------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("case", [(30, 44, 5, 6, 7.0, 20.0), (17, 23, 4, 3, 40.0, 9.0), (1, 50, 1, 7, 10.0, 30.0)])
def test_restatement_gives_p_distinct_sorted_indices_with_the_centre(oracle, case):
    H, W, nr, nc, hx, hy = case
    y = oracle.synthetic_luminance(H, W)
    p = grid_count(oracle, H, W, nr, nc)
    S = farthest(y, p, hx, hy)
    assert S.size == p and np.unique(S).size == p
    assert np.all(np.diff(S) > 0) and S[0] >= 0 and S[-1] < H * W
    assert (H // 2) * W + W // 2 in S


@pytest.mark.parametrize("case", [(5, 7, 3, 4, 3.0, 20.0), (6, 6, 2, 5, 1e6, 10.0), (4, 9, 4, 4, 2.0, 1e6)])
def test_restatement_equals_brute_force_pairwise(oracle, case):
    H, W, nr, nc, hx, hy = case
    y = oracle.synthetic_luminance(H, W)
    p = grid_count(oracle, H, W, nr, nc)
    assert np.array_equal(farthest(y, p, hx, hy), farthest_brute(y, p, hx, hy))
    c = np.full((H, W), 7.0)  # constant plane: every tie goes to the smallest index
    assert np.array_equal(farthest(c, p, hx, hy), farthest_brute(c, p, hx, hy))


def test_sampler_is_declared_exported_and_mirrored(nle):
    hdr = open(os.path.join(ROOT, "include", "nle.h")).read()
    assert "#define NLE_SAMPLER_GRID 0" in hdr and "#define NLE_SAMPLER_FARTHEST 1" in hdr
    assert "int nle_ctx_set_sampler(nle_ctx* ctx, int sampler);" in hdr
    assert "int nle_sample_pixels(nle_ctx* ctx, const float* d_lum, int H, int W, int n_row_samples" in hdr
    assert "int nle_filter_sample_pixels(const nle_filter* f, long long* h_idx, int* p);" in hdr
    from nle_amd import _abi
    assert _abi.NLE_SAMPLER_GRID == 0 and _abi.NLE_SAMPLER_FARTHEST == 1
    assert nle.SAMPLER_GRID == 0 and nle.SAMPLER_FARTHEST == 1
    for name in ("nle_ctx_set_sampler", "nle_sample_pixels", "nle_filter_sample_pixels"):
        assert name in _abi.SIGNATURES and name in nle.EXPORTED_SYMBOLS
        assert hasattr(nle.lib(), name)  # exported by the built library
    assert callable(getattr(nle.Context, "set_sampler", None)) and callable(getattr(nle.Context, "sample_pixels", None))
    assert callable(getattr(nle.NLEFilter, "sample_pixels", None))
    hpp = open(os.path.join(ROOT, "include", "nle", "filter.hpp")).read()
    assert "int sampler = 0;" in hpp


@pytest.mark.parametrize("tool", [ENHANCE, DENOISE], ids=["enhance", "denoise"])
@pytest.mark.parametrize("lead", [["--sampler", "random"], ["--sampler", "Farthest"], ["--sampler"],
                                  ["--patch-radius", "3", "--sampler", "kmeans"], ["--sampler", "", "--patch-radius", "3"],
                                  ["--sampler", "farthest", "--patch-radius", "9"]],
                         ids=["random", "case", "missing", "after_radius", "empty_before_radius", "bad_radius"])
def test_cli_refuses_a_bad_sampler_before_any_gpu_call(tool, lead, tmp_path):
    # HIP_VISIBLE_DEVICES=-1: no device is visible -- the refusal must not need one
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = tmp_path / "o.png"
    args = lead + ([os.path.join(GOLDEN, "flower-50.bmp"), str(out)] + FLOWER_ARGS if lead != ["--sampler"] else [])
    r = subprocess.run([tool] + args, capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert ("--sampler" in r.stderr) or ("--patch-radius" in r.stderr and lead[-1] == "9")
    assert r.stdout == "" and not out.exists()


# ------------------------------------------------------------------------------------------------------ GPU tests
@pytest.fixture
def sctx(ctx):
    """the session ctx, handed back with the grid, no patches and auto mode whatever the test did"""
    yield ctx
    ctx.set_sampler(0)
    ctx.set_patch_radius(0)
    ctx.set_mode(0)


def _planes(oracle):
    rng = np.random.default_rng(7)
    fl = _flower_L(oracle)
    return {
        "synthetic": (oracle.synthetic_luminance(48, 64), 6, 8, 12.0, 30.0),
        "flower": (fl, FLOWER["nr"], FLOWER["nc"], FLOWER["hx"], FLOWER["hy"]),
        "non_integer": (rng.uniform(-3.0, 300.0, (40, 52)).astype(np.float32), 5, 7, 9.0, 17.5),
        "constant": (np.full((33, 41), 128.0), 4, 6, 10.0, 30.0),
        "one_row": (oracle.synthetic_luminance(1, 300), 1, 40, 20.0, 30.0),
        "large_hx": (oracle.synthetic_luminance(50, 70), 6, 7, 1e7, 25.0),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("plane", ["synthetic", "flower", "non_integer", "constant", "one_row", "large_hx"])
def test_sample_pixels_equals_the_restatement_exactly(nle, oracle, sctx, plane):
    y, nr, nc, hx, hy = _planes(oracle)[plane]
    H, W = y.shape
    sctx.set_sampler(nle.SAMPLER_FARTHEST)
    got = sctx.sample_pixels(y, nr, nc, hx, hy)
    want = farthest(y, grid_count(oracle, H, W, nr, nc), hx, hy)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    sctx.set_sampler(nle.SAMPLER_GRID)
    assert np.array_equal(sctx.sample_pixels(y, nr, nc, hx, hy), oracle.sample_pixels(H, W, nr, nc)[0])


@pytest.mark.gpu
def test_sampler_is_deterministic_on_a_large_plane(nle, oracle, sctx):
    y = oracle.synthetic_luminance(2048, 2048)
    sctx.set_sampler(nle.SAMPLER_FARTHEST)
    a = sctx.sample_pixels(y, 20, 20, 200.0, 30.0)
    b = sctx.sample_pixels(y, 20, 20, 200.0, 30.0)
    assert a.size == 400 and np.unique(a).size == 400 and np.array_equal(a, b)


def _kernel64(nle, ctx, y, nr, nc, hx, hy):
    import ctypes as C
    import torch
    H, W = y.shape
    p = grid_count(__import__("nle_oracle"), H, W, nr, nc)
    lum = torch.as_tensor(np.asarray(y, dtype=np.float32), device="cuda:0").contiguous()
    Ka = np.zeros((p, p), dtype=np.float64)
    kab = torch.full((H * W, nle.ld(p)), -1.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    st = nle.lib().nle_compute_kernel64(ctx._h, C.c_void_p(lum.data_ptr()), H, W, nr, nc, float(hx), float(hy),
                                        Ka.ctypes.data_as(C.c_void_p), C.c_void_p(kab.data_ptr()))
    return st, Ka.T.copy(), kab.cpu().numpy(), p


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(24, 40, 4, 5, 8.0, 30.0, False), (37, 29, 5, 3, 6.0, 12.0, True)],
                         ids=["integer", "non_integer"])
def test_compute_kernel64_with_farthest_matches_the_oracle(nle, oracle, sctx, monkeypatch, case):
    H, W, nr, nc, hx, hy, frac = case
    y = oracle.synthetic_luminance(H, W) + (0.25 if frac else 0.0)
    sctx.set_sampler(nle.SAMPLER_FARTHEST)
    st, Ka, kab, p = _kernel64(nle, sctx, y, nr, nc, hx, hy)
    assert st == 0, nle.lib().nle_last_error(sctx._h)
    S = farthest(y, p, hx, hy)
    use_set(monkeypatch, oracle, H, W, S)
    perm, Ka_o, Kab_o = oracle.compute_kernel(y, nr, nc, hx, hy)
    assert np.array_equal(perm[:p], S)
    K_o = np.empty((H * W, p))
    K_o[perm[:p]] = Ka_o
    K_o[perm[p:]] = Kab_o.T
    for got, want in ((Ka, Ka_o), (kab[:, :p], K_o)):
        zero = want == 0.0
        assert np.all(got[zero] == 0.0)
        if frac:
            # k_affinity64 (the grid's kernel too, unchanged here) may contract its exponent into an fma; with non-integer
            # values that moves the argument by an ulp, i.e. K by about |ln K| ulps
            w = want[~zero]
            assert np.all(np.abs(got[~zero] - w) <= 4 * 2.0 ** -52 * np.maximum(1.0, -np.log(w)) * w)
        else:
            np.testing.assert_allclose(got[~zero], want[~zero], rtol=1e-14, atol=0)
    assert np.all(kab[:, p:] == 0.0)


def _train_apply(nle, ctx, y, nr, nc, hx, hy, T, K, L):
    f = nle.NLEFilter(ctx).train_filter(np.asarray(y, dtype=np.float32), nr, nc, hx, hy, T, K)
    Y = f.apply_layers(np.asarray(y, dtype=np.float32), L).cpu().numpy().astype(np.float64)
    return f, Y


def _with_chunks(mode, fn):
    old = os.environ.get("NLE_STREAM64_CHUNK_MB")
    if mode == 5:
        os.environ["NLE_STREAM64_CHUNK_MB"] = "1"  # several chunks per pass
    try:
        return fn()
    finally:
        if mode == 5:
            if old is None:
                del os.environ["NLE_STREAM64_CHUNK_MB"]
            else:
                os.environ["NLE_STREAM64_CHUNK_MB"] = old


SYNTH = (72, 96, 6, 8, 16.0, 30.0, 10, 12, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("plane,R", [("synthetic", 0), ("flower", 0), ("synthetic", 3)])
def test_train_apply_with_farthest_meets_the_bars(nle, oracle, sctx, monkeypatch, plane, R):
    if plane == "synthetic":
        H, W, nr, nc, hx, hy, T, K, L = SYNTH
        y = oracle.synthetic_luminance(H, W)
    else:
        y = _flower_L(oracle)
        H, W = y.shape
        nr, nc, hx, hy, T, K, L = FLOWER["nr"], FLOWER["nc"], FLOWER["hx"], FLOWER["hy"], FLOWER["T"], FLOWER["K"], 4
    S = farthest(y, grid_count(oracle, H, W, nr, nc), hx, hy)
    if R == 0:
        use_set(monkeypatch, oracle, H, W, S)
        info = []
        V_o, S_o = oracle.train_filter(y, nr, nc, hx, hy, T, K, info=info)
    else:  # the patch restatement of tests/test_patch_affinity.py on the same set
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        import test_patch_affinity as tpa
        use_set(monkeypatch, oracle, H, W, S)
        V_o, S_o, info = tpa.train_patch(oracle, y, nr, nc, hx, hy, T, K, R)
    Y_o = oracle.apply_layers(V_o, S_o, y, L).reshape(L, -1)
    cuts = [d["kept"] for d in info]
    sctx.set_sampler(nle.SAMPLER_FARTHEST)
    sctx.set_patch_radius(R)
    results = {}
    for mode in (nle.MODE_MATERIALISED_F64, nle.MODE_STREAMED_F64, nle.MODE_AUTO):
        sctx.set_mode(mode)
        f, Y = _with_chunks(mode, lambda: _train_apply(nle, sctx, y, nr, nc, hx, hy, T, K, L))
        d = f.diag()
        assert d["formulation"] == (nle.MODE_MATERIALISED_F64 if mode == nle.MODE_AUTO else mode)
        assert np.array_equal(f.sample_pixels(), S)
        assert [d["r_Ka"], d["r_Wa"], d["r_Q"]] == cuts
        assert d["K"] == S_o.size
        ev_err = rel_l2(f.eigvals, S_o)
        errs = [rel_l2(Y[j], Y_o[j]) for j in range(L)]
        print(f"{plane} R = {R} mode {mode}: cuts {cuts}, eigenvalues {ev_err:.1e}, per-layer", ["%.1e" % e for e in errs])
        assert ev_err < 1e-8
        assert max(errs) < PER_LAYER_TOL
        results[mode] = Y
        f.close()
    for j in range(L):
        assert rel_l2(results[nle.MODE_STREAMED_F64][j], results[nle.MODE_MATERIALISED_F64][j]) < 1e-6


def _exact_layers(oracle, y, hx, hy, T, K, L):
    """the dense filter: the full K (N x N), Sinkhorn, the top-K eigenpairs of the symmetrised W"""
    H, W = y.shape
    N = H * W
    f = y.ravel()
    rr = np.arange(N) // W
    cc = np.arange(N) % W
    Kf = np.exp(-((rr[:, None] - rr[None]) ** 2 + (cc[:, None] - cc[None]) ** 2) / hx ** 2 - (f[:, None] - f[None]) ** 2 / hy ** 2)
    c = np.ones(N)
    for _ in range(T):
        r = 1 / (Kf @ c)
        c = 1 / (Kf.T @ r)
    Wm = r[:, None] * Kf * c[None]
    del Kf
    Wm = (Wm + Wm.T) / 2
    w, V = np.linalg.eigh(Wm)
    idx = np.argsort(w)[::-1][:K]
    w, V = w[idx], V[:, idx]
    resp = oracle.layer_responses(w, L)
    return np.stack([V @ (resp[j] * (V.T @ f)) for j in range(L)])


@pytest.mark.gpu
def test_farthest_is_closer_to_the_exact_filter_on_a_flower_crop(nle, oracle, sctx):
    y = np.load(os.path.join(GOLDEN, "flower_cfg1.npz"))["L_in"].astype(np.float64)[100:160, 150:240]
    nr, nc, hx, hy, T, K, L = 6, 9, 100.0, 30.0, 50, 30, 4
    ex = _exact_layers(oracle, y, hx, hy, T, K, L)
    err = {}
    for name, s in (("grid", nle.SAMPLER_GRID), ("farthest", nle.SAMPLER_FARTHEST)):
        sctx.set_sampler(s)
        f, Y = _train_apply(nle, sctx, y, nr, nc, hx, hy, T, K, L)
        f.close()
        err[name] = [rel_l2(Y[j], ex[j]) for j in range(L)]
    print("relative error against the exact filter per layer:", {k: ["%.4f" % e for e in v] for k, v in err.items()})
    assert err["farthest"][0] * 4 <= err["grid"][0]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 4], ids=["auto_tables", "materialised_f64"])
def test_grid_by_default_changes_nothing(nle, oracle, sctx, mode):
    H, W, nr, nc, hx, hy, T, K, L = SYNTH
    y = oracle.synthetic_luminance(H, W)
    fresh = nle.Context(0)
    try:
        fresh.set_mode(mode)
        f0, Y0 = _train_apply(nle, fresh, y, nr, nc, hx, hy, T, K, L)
        if mode == 0:
            assert f0.diag()["formulation"] == nle.MODE_PHI_FREE  # the tables
        sctx.set_mode(mode)
        sctx.set_sampler(nle.SAMPLER_GRID)
        f1, Y1 = _train_apply(nle, sctx, y, nr, nc, hx, hy, T, K, L)
        sctx.set_sampler(nle.SAMPLER_FARTHEST)
        sctx.set_sampler(nle.SAMPLER_GRID)
        f2, Y2 = _train_apply(nle, sctx, y, nr, nc, hx, hy, T, K, L)
        for f, Y in ((f1, Y1), (f2, Y2)):
            assert f0.diag() == f.diag()
            assert np.array_equal(f0.eigvals, f.eigvals) and np.array_equal(Y0, Y)
            assert np.array_equal(f.sample_pixels(), oracle.sample_pixels(H, W, nr, nc)[0])
        for f in (f0, f1, f2):
            f.close()
    finally:
        fresh.close()


@pytest.mark.gpu
def test_refusals_leave_the_ctx_usable(nle, oracle, sctx):
    H, W, nr, nc, hx, hy, T, K, L = 40, 56, 4, 5, 12.0, 30.0, 5, 6, 3
    y = oracle.synthetic_luminance(H, W)

    def refused(fn):
        with pytest.raises(nle.NLEError) as e:
            fn()
        assert e.value.code == nle.NLE_ERR_INVALID
        print("refused:", e.value)

    refused(lambda: sctx.set_sampler(2))
    refused(lambda: sctx.set_sampler(-1))
    sctx.set_sampler(nle.SAMPLER_FARTHEST)
    for mode in (nle.MODE_MATERIALISED, nle.MODE_PHI_FREE, nle.MODE_PHI_FREE_EXP):  # fp32 / table / Phi-free forms
        sctx.set_mode(mode)
        refused(lambda: _train_apply(nle, sctx, y, nr, nc, hx, hy, T, K, L))
    sctx.set_mode(0)
    refused(lambda: sctx.compute_kernel(y.astype(np.float32), nr, nc, hx, hy))  # fp32 stage entry points
    refused(lambda: sctx.nystrom(y.astype(np.float32), nr, nc, hx, hy))
    f, _ = _train_apply(nle, sctx, y, nr, nc, hx, hy, T, K, L)  # still usable
    assert f.diag()["formulation"] == nle.MODE_MATERIALISED_F64
    f.close()
    sctx.set_sampler(nle.SAMPLER_GRID)
    f, Y = _train_apply(nle, sctx, y, nr, nc, hx, hy, T, K, L)
    V_o, S_o = oracle.train_filter(y, nr, nc, hx, hy, T, K)
    Y_o = oracle.apply_layers(V_o, S_o, y, L).reshape(L, -1)
    assert max(rel_l2(Y[j], Y_o[j]) for j in range(L)) < PER_LAYER_TOL
    f.close()


# ------------------------------------------------------------------------------------------------------ multi-rank
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


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
        ctx.set_sampler(nle.SAMPLER_FARTHEST)
        g = nle.sample_grid(H, W, nr, nc)
        ctx.set_shard(rank, world, g["n_sel_rows"] * g["n_sel_cols"], lambda t: dist.all_reduce(t))
        if slabs:
            ctx.set_slab_input(True)
            r0, r1 = nle.slab_rows(H, rank, world)
            try:
                nle.NLEFilter(ctx).train_filter(np.ascontiguousarray(x[r0:r1]), nr, nc, hx, hy, T, K, shape=(H, W))
                code = 0
            except nle.NLEError as e:
                code = e.code
            np.savez(os.path.join(outdir, f"rank{rank}.npz"), code=np.array([code]))
        else:
            sel = ctx.sample_pixels(x, nr, nc, hx, hy)
            f = nle.NLEFilter(ctx).train_filter(x, nr, nc, hx, hy, T, K)
            Y = f.apply_layers(x, L).cpu().numpy()
            info = f.info()
            np.savez(os.path.join(outdir, f"rank{rank}.npz"), Y=Y, S=f.eigvals, sel=sel, fsel=f.sample_pixels(),
                     form=np.array([f.diag()["formulation"]]), rows=np.array([info["row0"], info["row1"]]))
            f.close()
        ctx.close()
    finally:
        dist.destroy_process_group()


MR = (64, 80, 6, 8, 14.0, 30.0, 8, 10, 4)


@pytest.mark.gpu
def test_two_ranks_with_farthest_match_single_rank(nle, sctx, tmp_path):
    import torch.multiprocessing as mp
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
    H, W, nr, nc, hx, hy, T, K, L = MR
    x = synth.synthetic_luminance(H, W)
    sctx.set_sampler(nle.SAMPLER_FARTHEST)
    f1, Y1 = _train_apply(nle, sctx, x, nr, nc, hx, hy, T, K, L)
    S1, sel1 = f1.eigvals, f1.sample_pixels()
    f1.close()
    mp.spawn(_worker, args=(2, _free_port(), MR, str(tmp_path), False), nprocs=2, join=True)
    Y = np.zeros((L, H * W))
    for r in range(2):
        d = np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))
        r0, r1 = d["rows"]
        Y[:, r0 * W:r1 * W] = d["Y"]
        assert np.array_equal(d["sel"], sel1) and np.array_equal(d["fsel"], sel1)
        assert int(d["form"][0]) == nle.MODE_MATERIALISED_F64
        assert rel_l2(d["S"], S1) < 1e-9
    for j in range(L):
        assert rel_l2(Y[j], Y1[j]) < 1e-6, j


@pytest.mark.gpu
def test_slab_input_with_farthest_is_refused_on_every_rank(nle, tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), MR, str(tmp_path), True), nprocs=2, join=True)
    for r in range(2):
        assert int(np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))["code"][0]) == nle.NLE_ERR_INVALID


# ------------------------------------------------------------------------------------------------------ CLI
@pytest.mark.gpu
def test_enhance_with_farthest_matches_the_python_mirror(nle, oracle, sctx, tmp_path):
    from PIL import Image
    import torch
    src = _load_bgr("flower-50.bmp")
    out = tmp_path / "flower-fps.png"
    r = subprocess.run([ENHANCE, "--sampler", "farthest", os.path.join(GOLDEN, "flower-50.bmp"), str(out)] + FLOWER_ARGS,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    got = np.asarray(Image.open(str(out)).convert("RGB"))[..., ::-1]
    # the same pipeline through the Python mirror: bgr2lab8 -> train_host_u8 -> apply_u8_host -> lab2bgr8
    sctx.set_sampler(nle.SAMPLER_FARTHEST)
    H, W = src.shape[:2]
    lab, _ = sctx.bgr2lab8(src)
    L8 = lab[..., 0].cpu().numpy().copy()
    f = nle.NLEFilter(sctx).train_filter_host_u8(L8, FLOWER["nr"], FLOWER["nc"], FLOWER["hx"], FLOWER["hy"], FLOWER["T"],
                                                 FLOWER["K"])
    assert np.array_equal(f.sample_pixels(), farthest(L8, f.info()["p"], FLOWER["hx"], FLOWER["hy"]))
    fS = oracle.transform_eigenvalues(f.eigvals, FLOWER["weights"])
    y8 = np.empty(H * W, dtype=np.uint8)
    f.apply_u8_host(None, fS, y8)
    f.close()
    Lf = torch.as_tensor(y8.reshape(H, W).astype(np.float32), device=lab.device)
    mirror = sctx.lab2bgr8(lab, L=Lf).cpu().numpy()
    assert np.array_equal(got, mirror)


@pytest.mark.gpu
@pytest.mark.parametrize("lead", [["--sampler", "farthest"], ["--patch-radius", "2", "--sampler", "farthest"]],
                         ids=["farthest", "farthest_after_radius"])
def test_denoise_with_farthest_runs(tmp_path, lead):
    out = tmp_path / "flower-dn.png"
    r = subprocess.run([DENOISE] + lead + [os.path.join(GOLDEN, "flower-50.bmp"), str(out)] + DENOISE_ARGS,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert out.exists() and out.stat().st_size > 0
