"""Patch (non-local-means) affinities: nle_ctx_set_patch_radius / NLEFilter::patchRadius / `--patch-radius`.

The restatement below is the contract of include/nle.h, in numpy: S_ij = the integer sum of squared differences of the
(2R + 1)^2 patches around pixel i and sample j (reflect-101 borders), K_ij = exp(-sw d2_ij - pwd S_ij) with
pwd = (1/hy^2) / (2R + 1)^2, evaluated in that order; K_A and K_AB alike.  Every later stage is the oracle's own
(nystrom_approximation, sinkhorn_with_scalings, orthogonalize, apply_layers), permuted back as oracle.train_filter does.
At R = 0 the restatement is oracle.compute_kernel bit for bit (checked below), so it restates nothing new there."""
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
def _reflect101(t, n):
    t = np.asarray(t)
    return np.where(t < 0, -t, np.where(t >= n, 2 * n - 2 - t, t))


def patches(y, R):
    """(H W) x (2R + 1)^2 int64: row i = the patch around pixel i (row-major scan), entry (dy + R)(2R + 1) + dx + R"""
    y = np.asarray(y)
    H, W = y.shape
    P = 2 * R + 1
    pad = y[np.ix_(_reflect101(np.arange(-R, H + R), H), _reflect101(np.arange(-R, W + R), W))].astype(np.int64)
    out = np.empty((H * W, P * P), dtype=np.int64)
    for dy in range(P):
        for dx in range(P):
            out[:, dy * P + dx] = pad[dy:dy + H, dx:dx + W].ravel()
    return out


def _patch_neg_dist(pa, ra, ca, pb, rb, cb, sw, pwd):
    # S exactly: |a|^2 + |b|^2 - 2 a.b, every partial sum an integer below 2^53 (255^2 * 225 < 2^24), so fp64 is exact
    a = pa.astype(np.float64)
    b = pb.astype(np.float64)
    S = np.rint((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)).astype(np.int64)
    dr = ra[:, None].astype(np.int64) - rb[None, :].astype(np.int64)
    dc = ca[:, None].astype(np.int64) - cb[None, :].astype(np.int64)
    return -sw * (dr * dr + dc * dc).astype(np.float64) - pwd * S.astype(np.float64)


def compute_kernel_patch(oracle, y, nr, nc, hx, hy, R, chunk=1 << 15):
    """(perm, Ka, Kab) in the oracle's [selected; rest] order, like oracle.compute_kernel"""
    y = np.asarray(y, dtype=np.float64)
    assert np.array_equal(y, np.rint(y)) and y.min() >= 0 and y.max() <= 255
    H, W = y.shape
    sel, rest = oracle.sample_pixels(H, W, nr, nc)
    sw, pwd = 1.0 / (hx * hx), (1.0 / (hy * hy)) / (2 * R + 1) ** 2
    Pt = patches(y.astype(np.int64), R)
    ps, sr, sc = Pt[sel], sel // W, sel % W
    Ka = np.exp(_patch_neg_dist(ps, sr, sc, ps, sr, sc, sw, pwd))
    Kab = np.empty((sel.size, rest.size))
    for s in range(0, rest.size, chunk):
        rr = rest[s:s + chunk]
        Kab[:, s:s + chunk] = np.exp(_patch_neg_dist(ps, sr, sc, Pt[rr], rr // W, rr % W, sw, pwd))
    return np.concatenate([sel, rest]), Ka, Kab


def train_patch(oracle, y, nr, nc, hx, hy, T, K, R):
    """oracle.train_filter with the patch affinities: (V N x K' pixel order, eigvals, cut diagnostics of Ka, Wa, Q)"""
    perm, Ka, Kab = compute_kernel_patch(oracle, y, nr, nc, hx, hy, R)
    info = []
    lam, phi = oracle.nystrom_approximation(Ka, Kab, info=info)
    del Kab
    Wa, Wab, _, _ = oracle.sinkhorn_with_scalings(phi, lam, T)
    V, S = oracle.orthogonalize(Wa, Wab, K, info=info)
    out = np.empty_like(V)
    out[perm] = V
    return out, S, info


def _cut_margin(info):
    """smallest factor between an eigenvalue either side of the three cuts and 1e-10"""
    m = np.inf
    for d in info:
        for v in (d["last_kept"], d["first_dropped"]):
            if v is not None and v > 0:
                m = min(m, abs(np.log10(v / 1e-10)))
    return 10 ** m


def _load_bgr(name):
    from PIL import Image
    return np.asarray(Image.open(os.path.join(GOLDEN, name)).convert("RGB"))[..., ::-1].copy()


_cache = {}


def _flower_L(oracle):
    if "flowerL" not in _cache:
        _cache["flowerL"] = oracle.bgr_to_lab8(_load_bgr("flower-50.bmp"))[..., 0].astype(np.float64)
    return _cache["flowerL"]


def _restated(oracle, key, y, nr, nc, hx, hy, T, K, R):
    if key not in _cache:
        _cache[key] = train_patch(oracle, y, nr, nc, hx, hy, T, K, R)
    return _cache[key]


# ------------------------------------------------------------------------------------------------------ CPU tests
def test_restatement_at_radius_0_is_the_oracle_s_kernel_bit_for_bit(oracle):
    for (H, W, nr, nc, hx, hy) in [(30, 44, 5, 6, 7.0, 20.0), (17, 23, 4, 3, 40.0, 9.0)]:
        y = oracle.synthetic_luminance(H, W)
        perm0, Ka0, Kab0 = oracle.compute_kernel(y, nr, nc, hx, hy)
        perm, Ka, Kab = compute_kernel_patch(oracle, y, nr, nc, hx, hy, 0)
        assert np.array_equal(perm, perm0)
        assert np.array_equal(Ka, Ka0) and np.array_equal(Kab, Kab0)


def test_restatement_patches_reflect_101(oracle):
    y = np.arange(4 * 5).reshape(4, 5)
    P = patches(y, 2)
    # pixel (0, 0): rows -2..2 -> 2 1 0 1 2, cols likewise (BORDER_DEFAULT: gfedcb|abcdefgh|gfedcba)
    want = y[np.ix_([2, 1, 0, 1, 2], [2, 1, 0, 1, 2])].ravel()
    assert np.array_equal(P[0], want)
    want = y[np.ix_([1, 2, 3, 2, 1], [2, 3, 4, 3, 2])].ravel()  # pixel (3, 4)
    assert np.array_equal(P[19], want)


def test_patch_radius_is_declared_exported_and_mirrored(nle):
    hdr = open(os.path.join(ROOT, "include", "nle.h")).read()
    assert "int nle_ctx_set_patch_radius(nle_ctx* ctx, int radius);" in hdr
    assert "#define NLE_PATCH_RADIUS_MAX 7" in hdr
    from nle_amd import _abi
    assert _abi.NLE_PATCH_RADIUS_MAX == 7
    assert "nle_ctx_set_patch_radius" in _abi.SIGNATURES and "nle_ctx_set_patch_radius" in nle.EXPORTED_SYMBOLS
    assert hasattr(nle.lib(), "nle_ctx_set_patch_radius")  # exported by the built library
    assert callable(getattr(nle.Context, "set_patch_radius", None))
    hpp = open(os.path.join(ROOT, "include", "nle", "filter.hpp")).read()
    assert "int patchRadius = 0;" in hpp


@pytest.mark.parametrize("tool", [ENHANCE, DENOISE], ids=["enhance", "denoise"])
@pytest.mark.parametrize("radius", ["9", "-1", "8", "two"])
def test_cli_refuses_a_bad_patch_radius_before_any_gpu_call(tool, radius, tmp_path):
    # HIP_VISIBLE_DEVICES=-1: no device is visible -- the refusal must not need one
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = tmp_path / "o.png"
    r = subprocess.run([tool, "--patch-radius", radius, os.path.join(GOLDEN, "flower-50.bmp"), str(out)] + FLOWER_ARGS,
                       capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "--patch-radius" in r.stderr and radius in r.stderr
    assert r.stdout == "" and not out.exists()


# ------------------------------------------------------------------------------------------------------ GPU tests
@pytest.fixture
def pctx(ctx):
    """the session ctx, handed back with the reference's affinity and auto mode whatever the test did"""
    yield ctx
    ctx.set_patch_radius(0)
    ctx.set_mode(0)


def _kernel64(nle, ctx, y, nr, nc, hx, hy):
    import ctypes as C
    import torch
    H, W = y.shape
    g = nle.sample_grid(H, W, nr, nc)
    p = g["n_sel_rows"] * g["n_sel_cols"]
    lum = torch.as_tensor(y.astype(np.float32), device="cuda:0").contiguous()
    Ka = np.zeros((p, p), dtype=np.float64)
    kab = torch.full((H * W, nle.ld(p)), -1.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    st = nle.lib().nle_compute_kernel64(ctx._h, C.c_void_p(lum.data_ptr()), H, W, nr, nc, float(hx), float(hy),
                                        Ka.ctypes.data_as(C.c_void_p), C.c_void_p(kab.data_ptr()))
    return st, Ka.T.copy(), kab.cpu().numpy(), p


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(24, 40, 4, 5, 8.0, 30.0, 1), (48, 64, 6, 8, 12.0, 25.0, 3), (8, 21, 3, 6, 10.0, 30.0, 7),
                                  (37, 12, 5, 3, 6.0, 12.0, 3)])
def test_compute_kernel64_with_patches_matches_the_restatement(nle, oracle, pctx, case):
    H, W, nr, nc, hx, hy, R = case
    y = oracle.synthetic_luminance(H, W)
    pctx.set_patch_radius(R)
    st, Ka, kab, p = _kernel64(nle, pctx, y, nr, nc, hx, hy)
    assert st == 0, nle.lib().nle_last_error(pctx._h)
    perm, Ka_o, Kab_o = compute_kernel_patch(oracle, y, nr, nc, hx, hy, R)
    K_o = np.empty((H * W, p))  # natural pixel order, every pixel (the sample pixels' rows are rows of Ka)
    K_o[perm[:p]] = Ka_o
    K_o[perm[p:]] = Kab_o.T
    for got, want in ((Ka, Ka_o), (kab[:, :p], K_o)):
        zero = want == 0.0
        assert np.all(got[zero] == 0.0)
        np.testing.assert_allclose(got[~zero], want[~zero], rtol=1e-14, atol=0)
    assert np.all(kab[:, p:] == 0.0)
    print(f"R = {R}: {H} x {W}, p = {p}, K_AB in [{K_o.min():.2e}, {K_o.max():.2e}]")


def _train_apply(nle, ctx, y, nr, nc, hx, hy, T, K, L):
    f = nle.NLEFilter(ctx).train_filter(y.astype(np.float32), nr, nc, hx, hy, T, K)
    Y = f.apply_layers(y.astype(np.float32), L).cpu().numpy().astype(np.float64)
    return f, Y


SYNTH = (72, 96, 6, 8, 16.0, 30.0, 10, 12, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("plane", ["synthetic", "flower"])
def test_train_apply_with_patches_meets_the_bars_in_every_fp64_form(nle, oracle, pctx, plane, R):
    if plane == "synthetic":
        H, W, nr, nc, hx, hy, T, K, L = SYNTH
        y = oracle.synthetic_luminance(H, W)
    else:
        y = _flower_L(oracle)
        H, W = y.shape
        nr, nc, hx, hy, T, K, L = FLOWER["nr"], FLOWER["nc"], FLOWER["hx"], FLOWER["hy"], FLOWER["T"], FLOWER["K"], 4
    V_o, S_o, info = _restated(oracle, (plane, R), y, nr, nc, hx, hy, T, K, R)
    Y_o = oracle.apply_layers(V_o, S_o, y, L).reshape(L, -1)
    cuts = [d["kept"] for d in info]
    print(f"{plane} R = {R}: restated cuts {cuts}, K' = {S_o.size}, nearest eigenvalue to the 1e-10 cut is "
          f"{_cut_margin(info):.1f}x away")
    pctx.set_patch_radius(R)
    results = {}
    for mode in (nle.MODE_MATERIALISED_F64, nle.MODE_STREAMED_F64, nle.MODE_AUTO):
        pctx.set_mode(mode)
        old = os.environ.get("NLE_STREAM64_CHUNK_MB")
        if mode == nle.MODE_STREAMED_F64:
            os.environ["NLE_STREAM64_CHUNK_MB"] = "1"  # several chunks per pass
        try:
            f, Y = _train_apply(nle, pctx, y, nr, nc, hx, hy, T, K, L)
        finally:
            if mode == nle.MODE_STREAMED_F64:
                if old is None:
                    del os.environ["NLE_STREAM64_CHUNK_MB"]
                else:
                    os.environ["NLE_STREAM64_CHUNK_MB"] = old
        d = f.diag()
        want_form = nle.MODE_MATERIALISED_F64 if mode == nle.MODE_AUTO else mode
        assert d["formulation"] == want_form
        assert [d["r_Ka"], d["r_Wa"], d["r_Q"]] == cuts
        assert d["K"] == S_o.size
        ev_err = rel_l2(f.eigvals, S_o)
        errs = [rel_l2(Y[j], Y_o[j]) for j in range(L)]
        print(f"  mode {mode}: eigenvalues {ev_err:.1e}, per-layer", ["%.1e" % e for e in errs])
        assert ev_err < 1e-8
        assert max(errs) < PER_LAYER_TOL
        results[mode] = Y
        f.close()
    for j in range(L):  # the two fp64 forms agree as tests/test_gpu_parity.py holds them
        assert rel_l2(results[nle.MODE_STREAMED_F64][j], results[nle.MODE_MATERIALISED_F64][j]) < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 4], ids=["auto_tables", "materialised_f64"])
def test_radius_0_changes_nothing(nle, oracle, pctx, mode):
    H, W, nr, nc, hx, hy, T, K, L = SYNTH
    y = oracle.synthetic_luminance(H, W)
    fresh = nle.Context(0)
    try:
        fresh.set_mode(mode)
        f0, Y0 = _train_apply(nle, fresh, y, nr, nc, hx, hy, T, K, L)
        pctx.set_mode(mode)
        pctx.set_patch_radius(3)
        pctx.set_patch_radius(0)
        f1, Y1 = _train_apply(nle, pctx, y, nr, nc, hx, hy, T, K, L)
        assert f0.diag() == f1.diag()
        assert np.array_equal(f0.eigvals, f1.eigvals) and np.array_equal(Y0, Y1)
        f0.close()
        f1.close()
    finally:
        fresh.close()


@pytest.mark.gpu
def test_refusals_leave_the_ctx_usable(nle, oracle, pctx):
    H, W, nr, nc, hx, hy, T, K, L = 40, 56, 4, 5, 12.0, 30.0, 5, 6, 3
    y = oracle.synthetic_luminance(H, W)

    def refused(fn):
        with pytest.raises(nle.NLEError) as e:
            fn()
        assert e.value.code == nle.NLE_ERR_INVALID
        print("refused:", e.value)

    refused(lambda: pctx.set_patch_radius(8))
    refused(lambda: pctx.set_patch_radius(-1))
    pctx.set_patch_radius(3)
    for mode in (nle.MODE_MATERIALISED, nle.MODE_PHI_FREE, nle.MODE_PHI_FREE_EXP):  # fp32 / table / Phi-free forms
        pctx.set_mode(mode)
        refused(lambda: _train_apply(nle, pctx, y, nr, nc, hx, hy, T, K, L))
    pctx.set_mode(0)
    refused(lambda: _train_apply(nle, pctx, y + 0.5, nr, nc, hx, hy, T, K, L))        # not integer valued
    refused(lambda: _train_apply(nle, pctx, y + 256.0, nr, nc, hx, hy, T, K, L))      # not in [0, 255]
    refused(lambda: _train_apply(nle, pctx, y[:3], 3, nc, hx, hy, T, K, L))           # R >= min(H, W)
    refused(lambda: pctx.compute_kernel(y.astype(np.float32), nr, nc, hx, hy))        # fp32 stage entry point
    st, _, _, _ = _kernel64(nle, pctx, y + 0.5, nr, nc, hx, hy)
    assert st == nle.NLE_ERR_INVALID
    st, _, _, _ = _kernel64(nle, pctx, y[:3], 3, nc, hx, hy)
    assert st == nle.NLE_ERR_INVALID
    # still usable: the same ctx trains at R = 3 and, back at R = 0, exactly as a fresh ctx does
    f, _ = _train_apply(nle, pctx, y, nr, nc, hx, hy, T, K, L)
    assert f.diag()["formulation"] == nle.MODE_MATERIALISED_F64
    f.close()
    pctx.set_patch_radius(0)
    f, Y = _train_apply(nle, pctx, y, nr, nc, hx, hy, T, K, L)
    V_o, S_o = oracle.train_filter(y, nr, nc, hx, hy, T, K)
    Y_o = oracle.apply_layers(V_o, S_o, y, L).reshape(L, -1)
    assert max(rel_l2(Y[j], Y_o[j]) for j in range(L)) < PER_LAYER_TOL
    f.close()


# ------------------------------------------------------------------------------------------------------ multi-rank
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, args, R, outdir, slabs):
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
        ctx.set_patch_radius(R)
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
            f = nle.NLEFilter(ctx).train_filter(x, nr, nc, hx, hy, T, K)
            Y = f.apply_layers(x, L).cpu().numpy()
            info = f.info()
            np.savez(os.path.join(outdir, f"rank{rank}.npz"), Y=Y, S=f.eigvals, form=np.array([f.diag()["formulation"]]),
                     rows=np.array([info["row0"], info["row1"]]))
            f.close()
        ctx.close()
    finally:
        dist.destroy_process_group()


MR = (64, 80, 6, 8, 14.0, 30.0, 8, 10, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_ranks_with_patches_match_single_rank(nle, pctx, tmp_path, world):
    import torch.multiprocessing as mp
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
    H, W, nr, nc, hx, hy, T, K, L = MR
    x = synth.synthetic_luminance(H, W)
    pctx.set_patch_radius(3)
    f1, Y1 = _train_apply(nle, pctx, x, nr, nc, hx, hy, T, K, L)
    S1 = f1.eigvals
    f1.close()
    mp.spawn(_worker, args=(world, _free_port(), MR, 3, str(tmp_path), False), nprocs=world, join=True)
    Y = np.zeros((L, H * W))
    for r in range(world):
        d = np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))
        r0, r1 = d["rows"]
        Y[:, r0 * W:r1 * W] = d["Y"]
        assert int(d["form"][0]) == nle.MODE_MATERIALISED_F64
        assert rel_l2(d["S"], S1) < 1e-9
    for j in range(L):
        assert rel_l2(Y[j], Y1[j]) < 1e-6, j


@pytest.mark.gpu
def test_slab_input_with_patches_is_refused_on_every_rank(nle, tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), MR, 3, str(tmp_path), True), nprocs=2, join=True)
    for r in range(2):
        assert int(np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))["code"][0]) == nle.NLE_ERR_INVALID


# ------------------------------------------------------------------------------------------------------ CLI
@pytest.mark.gpu
def test_enhance_with_patch_radius_matches_the_python_mirror_and_the_restatement(nle, oracle, pctx, tmp_path):
    from PIL import Image
    src = _load_bgr("flower-50.bmp")
    out = tmp_path / "flower-r3.png"
    r = subprocess.run([ENHANCE, "--patch-radius", "3", os.path.join(GOLDEN, "flower-50.bmp"), str(out)] + FLOWER_ARGS,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    got = np.asarray(Image.open(str(out)).convert("RGB"))[..., ::-1]
    # the same pipeline through the Python mirror: bgr2lab8 -> train_host_u8 -> apply_u8_host -> lab2bgr8
    import torch
    pctx.set_patch_radius(3)
    H, W = src.shape[:2]
    lab, _ = pctx.bgr2lab8(src)
    L8 = lab[..., 0].cpu().numpy().copy()
    f = nle.NLEFilter(pctx).train_filter_host_u8(L8, FLOWER["nr"], FLOWER["nc"], FLOWER["hx"], FLOWER["hy"], FLOWER["T"],
                                                 FLOWER["K"])
    fS = oracle.transform_eigenvalues(f.eigvals, FLOWER["weights"])
    y8 = np.empty(H * W, dtype=np.uint8)
    f.apply_u8_host(None, fS, y8)
    f.close()
    Lf = torch.as_tensor(y8.reshape(H, W).astype(np.float32), device=lab.device)
    mirror = pctx.lab2bgr8(lab, L=Lf).cpu().numpy()
    assert np.array_equal(got, mirror)
    # the clamped 8-bit L plane against the restatement's
    y = L8.astype(np.float64)
    V_o, S_o, _ = _restated(oracle, ("flower", 3), y, FLOWER["nr"], FLOWER["nc"], FLOWER["hx"], FLOWER["hy"], FLOWER["T"],
                            FLOWER["K"], 3)
    y_o = oracle.apply_filter(V_o, y, oracle.transform_eigenvalues(S_o, FLOWER["weights"]))
    L_o = np.rint(np.clip(y_o, 0, 255)).astype(np.int64).ravel()
    diff = y8.astype(np.int64) - L_o
    same = float(np.mean(diff == 0))
    print(f"enhance --patch-radius 3: L plane equal to the restatement's on {100 * same:.3f} % of pixels, "
          f"max |diff| {np.abs(diff).max()}")
    assert same >= 0.999 and np.abs(diff).max() <= 1


@pytest.mark.gpu
def test_denoise_with_patch_radius_runs(tmp_path):
    out = tmp_path / "flower-dn.png"
    r = subprocess.run([DENOISE, "--patch-radius", "3", os.path.join(GOLDEN, "flower-50.bmp"), str(out)] + DENOISE_ARGS,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert out.exists() and out.stat().st_size > 0
