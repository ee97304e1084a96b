"""The hand-over from the Sinkhorn loop to the Gram stage on the default train (csrc/sample_space.hip: SampleSinkhorn::run,
train_tables).

On one rank with the full eigensolve of Q and W_A's root on the host, a train whose ctx has its page-locked staging block
downloads the last pass's row sums into that block, queues the Gram kernels and the reduce half, and only then waits --
for an event behind the download, not for the stream.  A fresh ctx has no staging block yet (it is sized from what the
first call asked for), so its first train takes the earlier order: a blocking copy, the Gram stage queued after it.  Both
orders must give the same bits: the tests compare later trains of one ctx with the first train of a fresh one,
array_equal, and one test reads the host's stage marks to show which order each train took.

Shapes: 5 x 31 and 16 x 256 with a 2 x 1 grid (two samples: the smallest p-sized side), 40 x 61 and 9 x 4099 with a 3 x 5
grid (W no multiple of 4 or of 256, one and several rows per sample row).
"""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HX, HY, T, L = 24.0, 30.0, 10, 4
CASES = [(5, 31, 2, 1, 2), (40, 61, 3, 5, 8), (16, 256, 2, 1, 2), (9, 4099, 3, 5, 8)]   # H, W, sample rows, sample columns, K


def _planes(oracle, H, W):
    x = oracle.synthetic_luminance(H, W)
    assert np.array_equal(x, np.rint(x)) and x.min() >= 0 and x.max() <= 255
    x2 = np.ascontiguousarray(255.0 - x[::-1, ::-1])
    assert not np.array_equal(x, x2)
    return x.astype(np.float32), x2.astype(np.float32)


def _dev(a):
    import torch
    return torch.as_tensor(a, device="cuda:0")


def _train_apply(nle, c, x_train, x_apply, case):
    """(eigvals, layers, timings, wall ms of the train) of one train + apply on ctx c"""
    H, W, nr, nc, K = case
    f = nle.NLEFilter(c)
    t0 = time.perf_counter()
    f.train_filter(_dev(x_train), nr, nc, HX, HY, T, K)
    wall = 1e3 * (time.perf_counter() - t0)
    assert f.diag()["formulation"] == nle.MODE_PHI_FREE       # the table formulation: the path under test
    Y = f.apply_layers(_dev(x_apply), L).cpu().numpy()
    out = (np.array(f.eigvals), Y, f.timings(), wall)
    f.close()
    return out


def _fresh(nle, x_train, x_apply, case):
    c = nle.Context(0)
    try:
        return _train_apply(nle, c, x_train, x_apply, case)
    finally:
        c.close()


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}x{c[1]}_grid{c[2]}x{c[3]}")
def runs(request, nle, oracle):
    """every train + apply the tests compare, made once per shape"""
    case = request.param
    x, x2 = _planes(oracle, case[0], case[1])
    ref = {"x": _fresh(nle, x, x, case), "x2": _fresh(nle, x2, x2, case), "x_apply_x2": _fresh(nle, x, x2, case)}
    c = nle.Context(0)
    try:
        same = [_train_apply(nle, c, x, x, case),        # first train of the ctx: the earlier order
                _train_apply(nle, c, x, x, case),        # staging block in place: operands on the device, Gram first
                _train_apply(nle, c, x2, x2, case),      # another plane behind it
                _train_apply(nle, c, x, x2, case)]       # apply on a plane that is not the training plane
    finally:
        c.close()
    return ref, same


def _same(a, b):
    assert np.isfinite(a[1]).all() and np.abs(a[1]).max() > 1.0
    assert np.array_equal(a[0], b[0]), "eigenvalues differ"
    assert np.array_equal(a[1], b[1]), "layers differ"


def test_back_to_back_trains_equal_fresh_contexts(runs):
    ref, same = runs
    _same(same[0], ref["x"])
    _same(same[1], ref["x"])
    _same(same[2], ref["x2"])


def test_apply_on_another_plane_equals_a_fresh_context(runs):
    ref, same = runs
    _same(same[3], ref["x_apply_x2"])
    assert not np.array_equal(same[3][1], ref["x"][1])        # (the other plane was really filtered)


def test_stage_timers_are_positive_and_within_the_wall_time(runs):
    ref, same = runs
    for eig, Y, t, wall in list(ref.values()) + same:
        stages = [t[k] for k in ("setup", "sinkhorn", "gram", "project")]
        print("stages", ["%.3f" % s for s in stages], "host %.3f total %.3f wall %.3f ms" % (t["host"], t["total"], wall))
        assert all(s > 0 for s in stages) and t["host"] > 0 and t["total"] > 0, t
        # the four stages are disjoint stretches of one stream inside the call
        assert sum(stages) <= t["total"] <= wall, (t, wall)


def test_the_second_train_of_a_ctx_queues_the_gram_stage_before_it_waits(nle, oracle, monkeypatch, capfd):
    """the host's stage marks (NLE_TRACE): the first train of a ctx drains the stream before the Gram stage, the next one
    marks "gram enqueued" ahead of the wait -- without this the tests above would pass on the earlier order alone"""
    case = CASES[1]
    x, _ = _planes(oracle, case[0], case[1])
    monkeypatch.setenv("NLE_TRACE", "1")
    c = nle.Context(0)
    try:
        capfd.readouterr()
        _train_apply(nle, c, x, x, case)
        first = capfd.readouterr().err
        _train_apply(nle, c, x, x, case)
        second = capfd.readouterr().err
    finally:
        c.close()
    assert "ss: sinkhorn sync" in first and "ss: gram enqueued" not in first
    assert "ss: gram enqueued" in second
    assert second.index("ss: passes enqueued") < second.index("ss: gram enqueued") < second.index("ss: sinkhorn sync")


def test_eigvecs_on_demand_after_a_gram_first_train(nle, oracle):
    """V on demand reads c at every pixel: finite everywhere, the rows at the sample pixels are the exact sample rows, and
    the whole of V is what a fresh ctx (the earlier order) gives, bit for bit"""
    case = CASES[1]
    H, W, nr, nc, K = case
    x, _ = _planes(oracle, H, W)

    def V_of(c, warm_up):
        for _ in range(warm_up):
            nle.NLEFilter(c).train_filter(_dev(x), nr, nc, HX, HY, T, K).close()
        f = nle.NLEFilter(c).train_filter(_dev(x), nr, nc, HX, HY, T, K)
        out = (f.eigvecs().cpu().numpy(), f.sample_pixels(), f.info()["K"])
        f.close()
        return out

    c0, c1 = nle.Context(0), nle.Context(0)
    try:
        V0, pix0, K0 = V_of(c0, 0)
        V1, pix1, K1 = V_of(c1, 1)
    finally:
        c0.close(), c1.close()
    assert np.isfinite(V1).all() and K1 == K0 and np.array_equal(pix1, pix0) and pix1.size == nr * nc
    assert (np.abs(V1[pix1, :K1]).max(axis=1) > 0).all()
    assert np.array_equal(V1[pix1], V0[pix1]), "sample rows differ"
    assert np.array_equal(V1, V0)


# ---- the verdict of the level check: this train path reads it as before; what follows it on the ctx must be unchanged ----
# (No +inf / NaN plane is trained here: a NaN anywhere in the plane reaches the host eigensolver of the fp64 formulations --
# through K_A from a sample pixel, through the Gram matrix from any other -- which does not survive it.  The check
# kernel's own answer on those bit patterns is asked below through nle_table_levels.)
VH, VW, VNR, VNC, VK, VL = 40, 61, 3, 5, 8, 3
PER_LAYER_TOL = 1e-4   # tests/test_gpu_parity.py: the bar for layers against the oracle


def _sample_pixel(nle):
    g = nle.sample_grid(VH, VW, VNR, VNC)
    return g["row_off"] + g["row_step"], g["col_off"] + g["col_step"]


def _train_v(nle, c, x, K=VK):
    return nle.NLEFilter(c).train_filter(_dev(np.ascontiguousarray(x, dtype=np.float32)), VNR, VNC, HX, HY, T, K)


@pytest.fixture(scope="module")
def warm(nle, oracle):
    """a ctx that has trained once (its staging block is in place: its trains queue the Gram stage first), the clean plane,
    and what a fresh ctx makes of that plane"""
    x = oracle.synthetic_luminance(VH, VW)
    c0 = nle.Context(0)
    f = _train_v(nle, c0, x)
    ref = (np.array(f.eigvals), f.apply_layers(_dev(x.astype(np.float32)), VL).cpu().numpy())
    f.close(), c0.close()
    c = nle.Context(0)
    _train_v(nle, c, x).close()
    yield c, x, ref
    c.close()


def _clean_train_is_the_fresh_one(nle, warm):
    c, x, ref = warm
    f = _train_v(nle, c, x)
    assert f.diag()["formulation"] == nle.MODE_PHI_FREE
    assert np.array_equal(np.array(f.eigvals), ref[0])
    assert np.array_equal(f.apply_layers(_dev(x.astype(np.float32)), VL).cpu().numpy(), ref[1])
    f.close()


@pytest.mark.parametrize("where", ["first", "last", "sample", "mid"])
@pytest.mark.parametrize("bad", [12.5, 256.0, -1.0])
def test_one_offending_value_takes_the_fp64_formulation(nle, oracle, warm, bad, where):
    c, x0, _ = warm
    pos = {"first": (0, 0), "last": (VH - 1, VW - 1), "sample": _sample_pixel(nle), "mid": (VH // 2 + 1, VW // 2)}[where]
    x = x0.copy()
    x[pos] = bad
    f = _train_v(nle, c, x)
    assert f.diag()["formulation"] in (nle.MODE_MATERIALISED_F64, nle.MODE_STREAMED_F64)
    assert f.level_tiles() == (0, 16)
    Y = f.apply_layers(_dev(x.astype(np.float32)), VL).cpu().numpy().astype(np.float64)
    f.close()
    V_o, S_o = oracle.train_filter(x, VNR, VNC, HX, HY, T, VK)
    Y_o = oracle.apply_layers(V_o, S_o, x, VL).reshape(VL, -1)
    errs = [float(np.linalg.norm(Y[j] - Y_o[j]) / np.linalg.norm(Y_o[j])) for j in range(VL)]
    print(f"{bad} at {pos}: per-layer rel L2 vs oracle", ["%.2e" % e for e in errs])
    assert max(errs) < PER_LAYER_TOL, errs
    _clean_train_is_the_fresh_one(nle, warm)


@pytest.mark.parametrize("name", ["one tile", "0 and 255", "all 16 tiles"])
def test_level_tiles_are_what_numpy_says_of_the_plane(nle, oracle, warm, name):
    c, x0, _ = warm
    s = (x0 - x0.min()) / (x0.max() - x0.min())
    x = {"one tile": np.rint(96 + 15 * s), "0 and 255": np.where(s > np.median(s), 255.0, 0.0),
         "all 16 tiles": np.rint(255 * s)}[name]
    tiles = np.unique((x // 16).astype(int))
    assert {"one tile": tiles.size == 1, "0 and 255": list(tiles) == [0, 15], "all 16 tiles": tiles.size == 16}[name]
    f = _train_v(nle, c, x)
    assert f.diag()["formulation"] == nle.MODE_PHI_FREE
    assert f.level_tiles() == (int(tiles.min()), int(tiles.max() - tiles.min() + 1))
    f.close()


def test_phi_free_beyond_256_samples_still_refuses_a_plane_that_is_not_integer(nle, oracle):
    H, W, nr, nc = 40, 61, 17, 16                                  # 272 samples: only the tables are Phi-free there
    x = oracle.synthetic_luminance(H, W)
    c = nle.Context(0)
    try:
        c.set_mode(nle.MODE_PHI_FREE)
        f = nle.NLEFilter(c).train_filter(_dev(x.astype(np.float32)), nr, nc, 4.0, HY, T, 8)   # (and leaves the staging block)
        assert f.diag()["formulation"] == nle.MODE_PHI_FREE and f.info()["p"] > 256
        f.close()
        x[H // 2, W // 2] = 12.5
        with pytest.raises(nle.NLEError) as e:
            nle.NLEFilter(c).train_filter(_dev(x.astype(np.float32)), nr, nc, 4.0, HY, T, 8)
        assert e.value.code == nle.NLE_ERR_INVALID
        x[H // 2, W // 2] = 12.0
        f = nle.NLEFilter(c).train_filter(_dev(x.astype(np.float32)), nr, nc, 4.0, HY, T, 8)   # the ctx stays usable
        assert f.diag()["formulation"] == nle.MODE_PHI_FREE
        f.close()
    finally:
        c.close()


@pytest.mark.parametrize("shape", [(5, 31), (40, 61), (16, 256), (9, 4099)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_level_check_refuses_non_finite_values_at_every_position(nle, oracle, warm, shape):
    c = warm[0]
    H, W = shape
    x0 = oracle.synthetic_luminance(H, W).astype(np.float32)
    assert c.table_levels(_dev(x0))[0] == 0
    g = nle.sample_grid(H, W, 2, 1)
    for pos in [(0, 0), (H - 1, W - 1), (g["row_off"], g["col_off"]), (H // 2, W // 2)]:
        for bad in (np.inf, -np.inf, np.nan, 12.5, 256.0, -1.0):
            x = x0.copy()
            x[pos] = bad
            assert c.table_levels(_dev(x))[0] != 0, (pos, bad)
