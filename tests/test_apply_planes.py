"""nle_apply_planes: one filter applied to several planes in one call (include/nle.h).

The contract is bitwise: every output of a batched call is the bits `apply`, `apply_layers` or `apply_rounded8` write for
that plane and those responses alone, in every formulation.  On a table filter with level-sorted rows the reduce half of the
batch is one pass of `k_sorted_reduce_planes` per group of NP planes (four up to 12 sample columns, two beyond), so the
shapes below are the smallest at which that kernel can differ from `k_sorted_pass`: each of its three pixel-loop forms, the
column counts where the combine's slices, the NP switch and the register budget change, more image rows than persistent
workgroups (the next-row prefetch), rows of one to three levels (hundreds of chunks in one level), widths that are no
multiple of four.  Which path ran is read off `kernel_stats()`: ceil(P / NP) reduce launches on the batched path, P on the
one-by-one route.  Outputs are compared as bit patterns (uint32 views), so NaN and infinity count like any value.

One train per shape, shared by the tests that need it; the single-call references of a shape are computed once.
"""
import math
import os
import re
import shutil
import socket
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT, load_oracle, rel_l2
from test_bandwidth_regimes import GRIDS, HY, NR, T, K, bandwidth, forms, grid_spec

F32, ROUNDED8 = 0, 1
P_SWEEP = (1, 2, 3, 4, 5, 9, 16)
NRESP_PATTERNS = ([4, 1, 1], [3, 2], [1, 5, 1, 2])


# ------------------------------------------------------------------------------------------------ CPU: the surface
def test_apply_planes_is_declared_mirrored_and_exported(nle):
    header = " ".join(open(os.path.join(ROOT, "include", "nle.h")).read().split())
    assert ("int nle_apply_planes(nle_filter* f, const float* d_x, int P, long long x_stride, int H, int W, "
            "const int* h_nresp, const double* h_resp, int out_kind, float* d_y, long long y_stride);") in header
    assert re.search(r"#define NLE_PLANES_MAX 16\b", header)
    assert "BIT FOR BIT" in header                                      # the contract is stated where the call is declared
    abi = nle._abi
    assert "nle_apply_planes" in abi.SIGNATURES and abi.NLE_PLANES_MAX == 16 and nle.PLANES_MAX == 16
    res, args = abi.SIGNATURES["nle_apply_planes"]
    assert len(args) == 11
    assert hasattr(nle.lib(), "nle_apply_planes")                       # the built library exports it
    assert callable(getattr(nle.NLEFilter, "apply_planes", None))
    hpp = open(os.path.join(ROOT, "include", "nle", "filter.hpp")).read()
    assert "applyPlanes(const std::vector<Image>& channels" in hpp


def test_no_new_environment_switch():
    text = open(os.path.join(PKG_DIR, "csrc", "switches.h")).read()
    assert len(set(re.findall(r'"(NLE_[A-Z0-9_]+)"', text))) == 20


# ------------------------------------------------------------------------------------------------ helpers
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def np_for(nc):
    """planes per reduce launch on the batched path (sorted_planes_per_launch)"""
    return 4 if nc <= 12 else 2


def make_planes(x_train, count):
    """`count` H x W fp32 planes cycling through the six kinds: seeded normal, a 0/1 stroke, a constant, the training plane,
    a plane scaled by 1e30 and one scaled by 1e-30"""
    H, W = x_train.shape
    rng = np.random.default_rng(7)
    rr, cc = np.mgrid[0:H, 0:W]
    out = []
    for m in range(count):
        kind = m % 6
        if kind == 0:
            p = rng.standard_normal((H, W))
        elif kind == 1:
            p = ((rr // max(H // 4, 1) + cc // max(W // 5, 1) + m) % 3 == 0).astype(np.float64)
        elif kind == 2:
            p = np.full((H, W), 37.5 + m)
        elif kind == 3:
            p = x_train.astype(np.float64)
        elif kind == 4:
            p = rng.standard_normal((H, W)) * 1e30
        else:
            p = rng.standard_normal((H, W)) * 1e-30
        out.append(p.astype(np.float32))
    return np.stack(out)


class Shape:
    """a trained filter, its planes and the single-call references, made once"""

    def __init__(self, nle, ctx, x, nr, nc, hx, env=(), mode=None, patch=0, n_eig=K, hy=HY, iters=T):
        self.nle, self.ctx, self.nc = nle, ctx, nc
        self.x = np.asarray(x, dtype=np.float32)
        self.H, self.W = self.x.shape
        with forms(*env):
            if mode is not None:
                ctx.set_mode(mode)
            if patch:
                ctx.set_patch_radius(patch)
            try:
                self.f = nle.NLEFilter(ctx).train_filter(self.x, nr, nc, hx, hy, iters, n_eig)
            finally:
                ctx.set_mode(nle.MODE_AUTO)
                ctx.set_patch_radius(0)
        self.ev = self.f.eigvals.copy()
        self.Kp = self.f.info()["K"]
        self.planes = make_planes(self.x, 16)
        rng = np.random.default_rng(11)
        # one response per plane: a transformed-eigenvalue vector for the first, seeded positive values for the others
        self.resp = [nle.transform_eigenvalues(self.ev, [2.0, 3.0, 4.0])] + [rng.uniform(0.1, 2.0, self.Kp) for _ in range(15)]
        self._single = {}

    def single(self, m, kind):
        """apply / apply_rounded8 of plane m with its response: computed once"""
        if (m, kind) not in self._single:
            fn = self.f.apply if kind == F32 else self.f.apply_rounded8
            self._single[(m, kind)] = fn(self.planes[m], self.resp[m]).cpu().numpy()
        return self._single[(m, kind)]

    def reduce_launches(self, fn):
        self.ctx.profile(1)
        try:
            out = fn()
            n = self.ctx.kernel_stats()["apply_reduce"][0]
        finally:
            self.ctx.profile(0)
        return out, n

    def check_ones(self, P, kind, expect_launches=None):
        """P planes, one response each, against the P single calls"""
        out, n = self.reduce_launches(lambda: self.f.apply_planes(self.planes[:P], self.resp[:P], out_kind=kind).cpu().numpy())
        for m in range(P):
            assert same_bits(out[m], self.single(m, kind)), (P, m, kind)
        if expect_launches is not None:
            assert n == expect_launches, (P, n, expect_launches)
        return out

    def check_pattern(self, nresp, kind):
        """plane m with nresp[m] responses: layer responses where there are several (against apply_layers too)"""
        nle, f = self.nle, self.f
        responses = [nle.layer_responses(self.ev, L) if L > 1 else self.resp[m][None] for m, L in enumerate(nresp)]
        out = f.apply_planes(self.planes[:len(nresp)], responses, out_kind=kind).cpu().numpy()
        j = 0
        for m, L in enumerate(nresp):
            if kind == F32 and L > 1:
                assert same_bits(out[j:j + L], f.apply_layers(self.planes[m], L).cpu().numpy()), (nresp, m)
            for l in range(L):
                fn = f.apply if kind == F32 else f.apply_rounded8
                assert same_bits(out[j + l], fn(self.planes[m], responses[m][l]).cpu().numpy()), (nresp, m, l, kind)
            j += L
        assert j == out.shape[0]

    def close(self):
        self.f.close()


_SHAPES = {}


def shape(key, make):
    """one Shape per key for the whole module; a failed train is kept and raised again (device code that failed once is not
    started a second time)"""
    if key not in _SHAPES:
        try:
            _SHAPES[key] = make()
        except (Exception, pytest.fail.Exception) as e:
            _SHAPES[key] = e
            raise
    if isinstance(_SHAPES[key], BaseException):
        raise RuntimeError("the train of %s failed earlier: %r" % (key, _SHAPES[key]))
    return _SHAPES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_shapes():
    yield
    for s in _SHAPES.values():
        if isinstance(s, Shape):
            s.close()
    _SHAPES.clear()


def the_kernel_name(nle):
    names = [nle.lib().nle_kernel_name(k).decode() for k in range(nle.KERNEL_COUNT)]
    return names[nle._abi.NLE_K_APPLY_REDUCE]


# ------------------------------------------------------------------------------------------------ GPU: kernel forms
FORM_CASES = [(g, b, ()) for g in ("a", "b", "c") for b in ("M-", "M+", "U")] + [("b", "M-", ("NLE_SORTED_NO_MOMENTS",))]


def form_shape(nle, ctx, grid, band, env):
    def make():
        oracle = load_oracle()
        H, W, nc = GRIDS[grid]["H"], GRIDS[grid]["W"], GRIDS[grid]["nc"]
        hx = bandwidth(grid_spec(H, W, nc), W, band)
        return Shape(nle, ctx, oracle.synthetic_luminance(H, W), NR, nc, hx, env=env)
    return shape(("form", grid, band, env), make)


@pytest.mark.gpu
def test_the_profile_slot_is_apply_reduce(nle):
    assert the_kernel_name(nle) == "apply_reduce"


@pytest.mark.gpu
@pytest.mark.parametrize("grid,band,env", FORM_CASES, ids=["%s:%s%s" % (g, b, ":no_moments" if e else "") for g, b, e in FORM_CASES])
def test_every_kernel_form_matches_single_calls_bitwise(nle, ctx, grid, band, env):
    """moment form (M-), table form (M+, U; the recurrence never survives M+), recurrence form (b, M-, moments off): every
    P of the sweep with one response per plane, both out kinds, and the launch count of the batched path"""
    s = form_shape(nle, ctx, grid, band, env)
    assert s.f.diag()["formulation"] == nle.MODE_PHI_FREE
    NP = np_for(s.nc)
    for kind in (F32, ROUNDED8):
        for P in P_SWEEP:
            s.check_ones(P, kind, expect_launches=math.ceil(P / NP))
    for nresp in NRESP_PATTERNS:                 # R = 6, 5, 9: crosses the expand group of four (a) and of two (b, c)
        for kind in (F32, ROUNDED8):
            s.check_pattern(nresp, kind)


@pytest.mark.gpu
def test_two_batched_calls_are_bitwise_equal(nle, ctx):
    s = form_shape(nle, ctx, "a", "M-", ())
    a = s.f.apply_planes(s.planes[:9], s.resp[:9]).cpu().numpy()
    b = s.f.apply_planes(s.planes[:9], s.resp[:9]).cpu().numpy()
    assert same_bits(a, b)


@pytest.mark.gpu
def test_strides_larger_than_the_plane_and_a_misaligned_input(nle, ctx):
    """planes 4-byte aligned only (an odd float offset, an odd stride) and outputs a stride apart"""
    import torch
    s = form_shape(nle, ctx, "b", "M-", ())
    P, n = 5, s.H * s.W
    xs, ys = n + 13, n + 7
    buf = torch.zeros(1 + P * xs, dtype=torch.float32, device="cuda:0")
    for m in range(P):
        buf[1 + m * xs:1 + m * xs + n] = torch.as_tensor(s.planes[m].ravel(), device="cuda:0")
    view = torch.as_strided(buf, (P, s.H, s.W), (xs, s.W, 1), storage_offset=1)
    assert view.data_ptr() % 16 != 0 and (xs * 4) % 16 != 0
    obuf = torch.full((P * ys,), -1.0, dtype=torch.float32, device="cuda:0")
    out = torch.as_strided(obuf, (P, n), (ys, 1))
    got = s.f.apply_planes(view, s.resp[:P], out=out)
    assert got.data_ptr() == obuf.data_ptr()
    res = obuf.cpu().numpy()
    for m in range(P):
        assert same_bits(res[m * ys:m * ys + n], s.single(m, F32)), m
        assert np.all(res[m * ys + n:(m + 1) * ys] == -1.0)              # nothing written between the planes


# ------------------------------------------------------------------------------------------------ GPU: column-count edges
@pytest.mark.gpu
@pytest.mark.parametrize("nc", [1, 2, 11, 12, 13])
def test_column_count_edges(nle, ctx, nc):
    """24 x 130: one column has no moment form; 11 / 12 are the slice edges of the combine; 12 / 13 the NP switch"""
    def make():
        H, W = 24, 130
        hx = bandwidth(grid_spec(H, W, nc), W, "M-")
        return Shape(nle, ctx, load_oracle().synthetic_luminance(H, W), NR, nc, hx, n_eig=min(K, NR * nc))
    s = shape(("edge", nc), make)
    assert s.f.diag()["formulation"] == nle.MODE_PHI_FREE
    NP = np_for(nc)
    for kind in (F32, ROUNDED8):
        for P in (2, 3, 5):
            s.check_ones(P, kind, expect_launches=math.ceil(P / NP))
    s.check_pattern([1, 5, 1, 2], F32)


# ------------------------------------------------------------------------------------------------ GPU: the row pipeline
@pytest.mark.gpu
@pytest.mark.parametrize("nc", [4, 16])
def test_more_rows_than_persistent_workgroups(nle, ctx, nc):
    """H = 1100 > 2 x 256 workgroups: the row loop of a workgroup runs more than once, with the next row's prefetch"""
    def make():
        H, W = 1100, 48
        return Shape(nle, ctx, load_oracle().synthetic_luminance(H, W), NR, nc, W / 3.0)
    s = shape(("tall", nc), make)
    assert s.f.diag()["formulation"] == nle.MODE_PHI_FREE
    NP = np_for(nc)
    for P in (3, 5):
        s.check_ones(P, F32, expect_launches=math.ceil(P / NP))
    s.check_ones(4, ROUNDED8, expect_launches=math.ceil(4 / NP))


# ------------------------------------------------------------------------------------------------ GPU: flat and odd rows
def block_image(H, W):
    """rows of one, two or three levels in turn (levels differ between row bands, so the image is not constant)"""
    x = np.empty((H, W))
    cc = np.arange(W)
    for r in range(H):
        base = 40.0 + 10.0 * (r // 3)
        k = r % 3
        x[r] = base if k == 0 else base + 30.0 * (cc * (k + 1) // W)
    return x


@pytest.mark.gpu
def test_flat_rows_with_hundreds_of_chunks_in_one_level(nle, ctx):
    def make():
        H, W = 36, 700                          # a one-level row of 700 pixels: 350 chunks of two
        return Shape(nle, ctx, block_image(H, W), NR, 7, W / 4.0)
    s = shape(("flat",), make)
    assert s.f.diag()["formulation"] == nle.MODE_PHI_FREE
    for kind in (F32, ROUNDED8):
        for P in (2, 4, 5):
            s.check_ones(P, kind, expect_launches=math.ceil(P / 4))
    s.check_pattern([3, 2], F32)


@pytest.mark.gpu
@pytest.mark.parametrize("W", [61, 67])
def test_widths_that_are_no_multiple_of_four(nle, ctx, W):
    def make():
        return Shape(nle, ctx, load_oracle().synthetic_luminance(40, W), NR, 6, W / 3.0)
    s = shape(("odd", W), make)
    for kind in (F32, ROUNDED8):
        for P in (3, 4, 9):
            s.check_ones(P, kind, expect_launches=math.ceil(P / 4))


@pytest.mark.gpu
def test_too_few_rows_for_the_samples_is_refused_as_today(nle, ctx):
    x = load_oracle().synthetic_luminance(3, 64).astype(np.float32)
    with pytest.raises(nle.NLEError) as e:
        nle.NLEFilter(ctx).train_filter(x, 4, 8, 16.0, HY, T, K)
    assert e.value.code == nle.NLE_ERR_INVALID and "must be <= that of image" in str(e.value)
    s = form_shape(nle, ctx, "a", "M-", ())     # the ctx is still usable
    s.check_ones(2, F32)


# ------------------------------------------------------------------------------------------------ GPU: which path ran
@pytest.mark.gpu
def test_one_by_one_routes_launch_one_reduce_per_plane(nle, ctx):
    """MATERIALISED_F64 and a table filter trained without sorted rows: P reduce launches, the same bits"""
    oracle = load_oracle()
    H, W, nc = GRIDS["a"]["H"], GRIDS["a"]["W"], GRIDS["a"]["nc"]
    hx = bandwidth(grid_spec(H, W, nc), W, "M-")
    x = oracle.synthetic_luminance(H, W)
    m64 = shape(("m64",), lambda: Shape(nle, ctx, x, NR, nc, hx, mode=nle.MODE_MATERIALISED_F64))
    assert m64.f.diag()["formulation"] == nle.MODE_MATERIALISED_F64
    uns = shape(("unsorted",), lambda: Shape(nle, ctx, x, NR, nc, hx, env=("NLE_NO_SORTED_ROWS",)))
    assert uns.f.diag()["formulation"] == nle.MODE_PHI_FREE
    for s in (m64, uns):
        for kind in (F32, ROUNDED8):
            s.check_ones(5, kind, expect_launches=5)
        s.check_pattern([3, 2], F32)
    # the same table filter with sorted rows: two launches for five planes, and the unsorted filter's bits
    srt = form_shape(nle, ctx, "a", "M-", ())
    srt.check_ones(5, F32, expect_launches=2)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _two_rank_worker(rank, world, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    import __graft_entry__ as entry
    nle = entry.load_package()
    synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        H, W, nr, nc = 96, 128, 6, 8
        x = synth.synthetic_luminance(H, W).astype(np.float32)
        ctx = nle.Context(0)
        g = nle.sample_grid(H, W, nr, nc)
        ctx.set_shard(rank, world, g["n_sel_rows"] * g["n_sel_cols"], lambda t: dist.all_reduce(t))
        f = nle.NLEFilter(ctx).train_filter(x, nr, nc, 32.0, 30.0, 6, 10)
        planes = make_planes(x, 3)
        rng = np.random.default_rng(3)
        resp = [rng.uniform(0.1, 2.0, f.info()["K"]) for _ in range(3)]
        ctx.profile(1)
        out = f.apply_planes(planes, resp).cpu().numpy()
        launches = ctx.kernel_stats()["apply_reduce"][0]
        ctx.profile(0)
        ok = all(same_bits(out[m], f.apply(planes[m], resp[m]).cpu().numpy()) for m in range(3))
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), launches=launches, ok=ok, formulation=f.diag()["formulation"])
        f.close()
        ctx.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_two_ranks_go_one_by_one(nle, tmp_path):
    """world > 1 (the callback all-reduce of test_multirank_gpu.py): P reduce launches per rank, the single calls' bits"""
    import torch.multiprocessing as mp
    mp.spawn(_two_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        d = np.load(tmp_path / f"rank{r}.npz")
        assert int(d["formulation"]) == nle.MODE_PHI_FREE
        assert bool(d["ok"]) and int(d["launches"]) == 3, (r, d["ok"], d["launches"])


# ------------------------------------------------------------------------------------------------ GPU: other formulations
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["patch", "exact", "materialised_f32"])
def test_other_formulations_go_one_by_one_bitwise(nle, ctx, which):
    oracle = load_oracle()
    if which == "exact":
        make = lambda: Shape(nle, ctx, oracle.synthetic_luminance(32, 32), 2, 2, 10.0, mode=nle.MODE_EXACT_F64, n_eig=5, iters=5)
    elif which == "patch":
        make = lambda: Shape(nle, ctx, oracle.synthetic_luminance(48, 64), NR, 6, 20.0, patch=1)
    else:
        make = lambda: Shape(nle, ctx, oracle.synthetic_luminance(48, 64), NR, 6, 20.0, mode=nle.MODE_MATERIALISED)
    s = shape(("other", which), make)
    assert s.f.diag()["formulation"] != nle.MODE_PHI_FREE
    for kind in (F32, ROUNDED8):
        s.check_ones(3, kind, expect_launches=3)
    s.check_pattern([3, 2], F32)
    s.check_pattern([1, 2], ROUNDED8)


# ------------------------------------------------------------------------------------------------ GPU: the oracle
@pytest.mark.gpu
def test_a_batch_against_the_oracle(nle, ctx):
    """grid a, M-, P = 3, nresp = [3, 1, 1] against the oracle's apply at the standing bar: 1e-4 relative L2 per output.
    Planes: the training plane (its three layers), a 0/1 block stroke and the mirrored training plane."""
    oracle = load_oracle()
    s = form_shape(nle, ctx, "a", "M-", ())
    H, W, nc = s.H, s.W, s.nc
    x = oracle.synthetic_luminance(H, W)
    V_o, S_o = oracle.train_filter(x, NR, nc, bandwidth(grid_spec(H, W, nc), W, "M-"), HY, T, K)
    rr, cc = np.mgrid[0:H, 0:W]
    stroke = ((rr >= 8) & (rr < 30) & (cc >= 40) & (cc < 150)).astype(np.float64)
    mirror = x[::-1, ::-1].copy()
    fs1 = oracle.transform_eigenvalues(S_o, [2.0, 3.0, 4.0])
    fs2 = np.asarray(S_o, dtype=np.float64) ** 4.0
    out = s.f.apply_planes(np.stack([x, stroke, mirror]).astype(np.float32),
                           [nle.layer_responses(S_o, 3), fs1, fs2]).cpu().numpy().astype(np.float64)
    ref = np.concatenate([oracle.apply_layers(V_o, S_o, x, 3).reshape(3, -1),
                          oracle.apply_filter(V_o, stroke, fs1).reshape(1, -1),
                          oracle.apply_filter(V_o, mirror, fs2).reshape(1, -1)])
    errs = [rel_l2(out[j], ref[j]) for j in range(5)]
    print("apply_planes vs oracle, relative L2 per output:", ["%.2e" % e for e in errs])
    assert max(errs) <= 1e-4, errs


# ------------------------------------------------------------------------------------------------ GPU: the users
@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 3, 8])
def test_region_spread_is_m_single_applies(nle, ctx, M):
    s = form_shape(nle, ctx, "a", "M-", ())
    strokes = s.planes[:M].copy()
    scale = np.linspace(0.5, 2.0, M)
    (q, n) = s.reduce_launches(lambda: s.f.region_spread(strokes, scale=scale, spread=4.0).cpu().numpy())
    assert n == math.ceil(M / 4)
    for m in range(M):
        fS = np.array([scale[m] * math.pow(v, 4.0) for v in s.ev])      # c_m pow(lambda_k, t), the C library's pow
        assert same_bits(q[m], s.f.apply(strokes[m], fS).cpu().numpy()), m


@pytest.mark.gpu
def test_apply_regions_is_the_three_stage_calls(nle, ctx):
    import torch
    s = form_shape(nle, ctx, "a", "M-", ())
    M, L = 2, 4
    strokes = np.stack([s.planes[1], s.planes[7]])
    w = np.array([[1.0, 1.0, 1.0, 1.0], [2.0, 3.0, 4.0, 1.0], [0.5, 0.5, 2.0, 1.0]])
    for kind in (nle.REGION_OUT_F32, nle.REGION_OUT_ROUNDED8, nle.REGION_OUT_U8):
        (got, n) = s.reduce_launches(lambda: s.f.apply_regions(s.x, L, strokes, w, out_kind=kind).cpu().numpy())
        assert n == 1                                                   # [x; s_1, s_2]: one group
        layers = s.f.apply_layers(s.x, L)
        q = s.f.region_spread(strokes)
        want = ctx.region_combine(layers, q, w, out_kind=kind).cpu().numpy()
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), kind
    del torch


CPP_DRIVER = textwrap.dedent(r"""
    #include <cmath>
    #include <cstdio>
    #include <cstring>
    #include "nle/filter.hpp"
    int main() {
        const int H = 48, W = 64;
        nle::Image L(H, W, nle::NLE_64F, 1), S(H, W, nle::NLE_64F, 1);
        for (int r = 0; r < H; ++r)
            for (int c = 0; c < W; ++c) {
                L.at<double>(r, c) = std::floor(128 + 60 * std::sin(0.2 * r) * std::cos(0.15 * c) + 20 * ((r * 7 + c * 13) % 5) / 5.0);
                S.at<double>(r, c) = (r > 10 && r < 30 && c > 20 && c < 50) ? 1.0 : 0.0;
            }
        nle::NLEFilter f;
        f.verbose = false;
        f.trainFilter(L, 4, 5, 16.0, 30.0, 10, 8);
        nle::Vec ev = f.eigvals(), a(ev.size()), b(ev.size()), c(ev.size());
        for (int i = 0; i < ev.size(); ++i) a(i) = ev(i), b(i) = ev(i) * ev(i), c(i) = 2.0 - ev(i);
        std::vector<nle::Image> out = f.applyPlanes({L, S}, {{a, b}, {c}});
        if (out.size() != 3) return 2;
        const nle::Image want[3] = {f.apply(L, a), f.apply(L, b), f.apply(S, c)};
        for (int j = 0; j < 3; ++j)
            if (out[j].rows != H || out[j].cols != W || std::memcmp(out[j].ptr<double>(), want[j].ptr<double>(), sizeof(double) * H * W) != 0) {
                std::printf("output %d differs\n", j);
                return 1;
            }
        bool threw = false;
        try {
            f.applyPlanes({L, S}, {{a}});
        } catch (const std::runtime_error&) {
            threw = true;
        }
        if (!threw) return 3;
        std::printf("applyPlanes OK\n");
        return 0;
    }
""")


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_cpp_apply_planes_matches_apply(tmp_path):
    host = os.path.join(PKG_DIR, "host")
    libdir = os.path.join(PKG_DIR, "lib")
    (tmp_path / "drv.cpp").write_text(CPP_DRIVER)
    b = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(tmp_path / "drv.cpp"),
                        *[os.path.join(host, s) for s in ("filter.cpp", "stages.cpp", "colour.cpp", "device_group.cpp", "image_io.cpp", "jpeg.cpp")],
                        "-L", libdir, "-lnle_hip", "-Wl,-rpath," + libdir, "-o", str(tmp_path / "drv")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(tmp_path / "drv")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "applyPlanes OK" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-1000:])


# ------------------------------------------------------------------------------------------------ GPU: refusals
@pytest.mark.gpu
def test_every_refusal_leaves_the_ctx_usable(nle, ctx):
    import ctypes as C
    import torch
    s = form_shape(nle, ctx, "a", "M-", ())
    lib, f, H, W, n, Kp = nle.lib(), s.f, s.H, s.W, s.H * s.W, s.Kp
    P = 3
    xbuf = torch.as_tensor(s.planes[:P].reshape(-1), device="cuda:0").contiguous()
    ybuf = torch.zeros(8 * n, dtype=torch.float32, device="cuda:0")
    resp = np.ascontiguousarray(np.stack(s.resp[:8]))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    X, Y, R = C.c_void_p(xbuf.data_ptr()), C.c_void_p(ybuf.data_ptr()), ptr(resp)
    ones = np.ones(16, dtype=np.int32)

    def call(x=X, P=P, xs=n, H=H, W=W, nresp=ptr(ones), r=R, kind=F32, y=Y, ys=n):
        return lib.nle_apply_planes(f._f, x, P, xs, H, W, nresp, r, kind, y, ys)

    def refused(what, **kw):
        st = call(**kw)
        msg = (lib.nle_last_error(ctx._h) or b"").decode()
        assert st == nle.NLE_ERR_INVALID and msg, (what, st, msg)
        # a plain apply still matches afterwards
        assert same_bits(f.apply(s.planes[0], s.resp[0]).cpu().numpy(), s.single(0, F32)), what
        return msg

    assert call() == nle.NLE_OK
    assert "planes" in refused("P = 0", P=0)
    refused("P = 17", P=17, nresp=None)
    bad = ones.copy()
    bad[1] = 0
    refused("nresp = 0", nresp=ptr(bad))
    bad[1] = 65
    refused("nresp = 65", nresp=ptr(bad))
    big = np.full(16, 43, dtype=np.int32)                                # 3 x 43 = 129 > 128
    assert "128" in refused("R > 128", nresp=ptr(big))
    refused("d_x NULL", x=None)
    refused("h_resp NULL", r=None)
    refused("d_y NULL", y=None)
    refused("out kind 2", kind=2)
    refused("out kind -1", kind=-1)
    refused("x stride < plane", xs=n - 1)
    refused("y stride < plane", ys=n - 1)
    assert refused("H W mismatch", H=H - 1) == "Number of values in channel must match that of training image."
    # overlap: an output inside an input plane, and an input inside the output range
    refused("output inside input", y=C.c_void_p(xbuf.data_ptr() + 4 * (n + 5)))
    both = torch.zeros(6 * n, dtype=torch.float32, device="cuda:0")
    three = np.array([3], dtype=np.int32)                                # outputs at 0, 2n, 4n; the input begins inside output 1
    refused("input inside outputs", x=C.c_void_p(both.data_ptr() + 4 * (2 * n + 5)), P=1, nresp=ptr(three),
            y=C.c_void_p(both.data_ptr()), ys=2 * n)
    # NULL h_nresp means one response per plane
    assert call(nresp=None) == nle.NLE_OK
    got = ybuf.cpu().numpy()
    for m in range(P):
        assert same_bits(got[m * n:(m + 1) * n], s.single(m, F32)), m
