"""What the table formulation hands from train to apply (csrc/sample_space.hip: train_tables), on a 64 x 97 plane with a
4 x 5 sample grid.

The filter must not depend on the caller's plane once nle_train has returned.  With level-sorted rows it keeps no copy of
the plane (nothing on the apply path reads it) and rebuilds it from the sorted rows and the sample values when V is asked
for; without them (NLE_NO_SORTED_ROWS) it keeps a copy.  D and the exact sample rows of V are written on the device in
the layout apply reads.

The plane is the oracle's synthetic plane (integer valued) with level 0 and level 255 set at two pixels, one row of a
single level that holds no samples, and the grid's sample rows as they are.

What checks the rebuild (k_rows_from_sorted).  Every sorted-path filter drops its plane, so two of them agreeing says
nothing about it.  The independent reference is the filter trained with NLE_NO_SORTED_ROWS: it projects V from its copy
of the caller's plane, never from sorted rows.  Row i of V is c_i k_i^T D with k_i[a] = exp(-d^2/hx^2 - (x_i - x_a)^2/hy^2):
a level of pixel i that is off by one moves every entry of k_i by a factor exp(-(2 dv + 1)/hy^2), at least 1/900 = 1.1e-3
relative at hy = 30, and a pixel never written (0 from the fresh allocation, or garbage) by far more.  The two forms
themselves differ only in the order of fp64 sums (tests/test_gpu_parity.py holds them to 1e-6 on the layers) and in the
fp32 rounding of V (2^-24 per entry), so every row of V is held to 1e-6 of its own norm: three orders below the
smallest error a wrong pixel makes, at every pixel -- levels 0 and 255, the flat row and the sample rows included.
"""
import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu

H, W, NR, NC, HX, HY, T = 64, 97, 4, 5, 24.0, 30.0, 10
PER_LAYER_TOL = 1e-4   # tests/test_gpu_parity.py: the bar for layers against the oracle
K_MAX = 128            # the largest K' the table formulation takes (tables_apply)


@pytest.fixture(scope="module")
def plane(nle, oracle):
    x = oracle.synthetic_luminance(H, W).copy()
    g = nle.sample_grid(H, W, NR, NC)
    sample_rows = {g["row_off"] + i * g["row_step"] for i in range(g["n_sel_rows"])}
    flat = next(r for r in range(7, H) if r not in sample_rows)
    x[flat, :] = 77.0
    free = next(r for r in range(H) if r not in sample_rows and r != flat)
    x[free, 3], x[free, 90] = 0.0, 255.0
    assert np.array_equal(x, np.rint(x)) and x.min() == 0.0 and x.max() == 255.0
    assert any((x[r] != x[r, 0]).any() for r in sample_rows)          # a row with sample pixels, not flat
    assert (x[flat] == 77.0).all()
    return x


@pytest.fixture()
def tables(nle, ctx):
    ctx.set_mode(2)
    yield
    ctx.set_mode(0)


_oracle_cache = {}


def _oracle_layers(oracle, x, K, L):
    if K not in _oracle_cache:
        _oracle_cache[K] = oracle.train_filter(x, NR, NC, HX, HY, T, K)
    V_o, S_o = _oracle_cache[K]
    return S_o, oracle.apply_layers(V_o, S_o, x, L).reshape(L, -1)


def _train(nle, ctx, d_plane, K):
    f = nle.NLEFilter(ctx).train_filter(d_plane, NR, NC, HX, HY, T, K)
    assert f.diag()["formulation"] == nle.MODE_PHI_FREE
    return f


def _pair(nle, ctx, plane, K=50):
    """(filter whose training plane was left alone, filter whose training plane was zeroed after the train, a fresh copy)"""
    import torch
    x32 = torch.as_tensor(plane.astype(np.float32), device="cuda:0")
    kept, doomed, fresh = x32.clone(), x32.clone(), x32.clone()
    f0 = _train(nle, ctx, kept, K)
    f1 = _train(nle, ctx, doomed, K)
    doomed.zero_()
    torch.cuda.synchronize()
    return f0, f1, fresh


def test_layers_do_not_depend_on_the_callers_plane(nle, ctx, tables, plane):
    f0, f1, fresh = _pair(nle, ctx, plane)
    Y0 = f0.apply_layers(fresh, 4).cpu().numpy()
    Y1 = f1.apply_layers(fresh, 4).cpu().numpy()
    assert np.isfinite(Y0).all() and np.abs(Y0).max() > 1.0
    assert np.array_equal(Y1, Y0)
    f0.close(), f1.close()


def _unsorted_filter(nle, ctx, plane, monkeypatch, K=50):
    """a filter on the LDS-atomic kernels, which keeps a copy of the caller's plane; proves that the switch took effect"""
    import torch
    monkeypatch.setenv("NLE_NO_SORTED_ROWS", "1")
    f = _train(nle, ctx, torch.as_tensor(plane.astype(np.float32), device="cuda:0"), K)
    monkeypatch.delenv("NLE_NO_SORTED_ROWS")
    return f


def _levels_39_to_215(oracle):
    x = oracle.synthetic_luminance(H, W)
    assert x.min() >= 32 and x.max() < 224         # the 16-level tiles 0, 1, 14 and 15 do not occur
    return x


def test_the_switch_selects_the_unsorted_path_per_call(nle, oracle, ctx, tables, monkeypatch):
    """only sorted rows know which level tiles occur (nle_filter_level_tiles): (0, 16) on a plane without the outer tiles
    means there are none -- the observable the no-sorted-rows cases below rest on"""
    x = _levels_39_to_215(oracle)
    f = _unsorted_filter(nle, ctx, x, monkeypatch)
    assert f.level_tiles() == (0, 16)
    f.close()
    import torch
    f = _train(nle, ctx, torch.as_tensor(x.astype(np.float32), device="cuda:0"), 50)
    t0, nt = f.level_tiles()
    assert t0 >= 2 and t0 + nt <= 14
    f.close()


def test_eigvecs_on_demand_after_the_plane_is_gone(nle, ctx, tables, plane, monkeypatch):
    f0, f1, fresh = _pair(nle, ctx, plane)
    mn1, mx1 = f1.eigvec_range(3)                      # leading columns only, from a temporary plane: the filter is unchanged
    V1 = f1.eigvecs().cpu().numpy()
    V0 = f0.eigvecs().cpu().numpy()
    mn0, mx0 = f0.eigvec_range(3)
    assert np.isfinite(V0).all() and np.abs(V0).max() > 0
    assert np.array_equal(V1, V0)
    assert np.array_equal(mn1, mn0) and np.array_equal(mx1, mx0)
    # the rebuilt plane against one that was never rebuilt: V projected from the copy the unsorted path keeps
    f_ref = _unsorted_filter(nle, ctx, plane, monkeypatch)
    K = f_ref.info()["K"]
    assert f1.info()["K"] == K
    V_ref = f_ref.eigvecs().cpu().numpy()[:, :K].astype(np.float64)
    V = V1[:, :K].astype(np.float64)
    sign = np.sign((V * V_ref).sum(0))                 # an eigenvector's sign is free
    assert (sign != 0).all()
    d = np.linalg.norm(V * sign - V_ref, axis=1)
    n = np.linalg.norm(V_ref, axis=1)
    worst = int((d / n).argmax())
    print(f"V from the rebuilt plane vs V from the kept copy: worst row {worst} (image row {worst // W}, col {worst % W}), "
          f"|dV| / |V| = {(d / n).max():.2e}; bar 1e-6")
    assert n.min() > 0
    assert (d <= 1e-6 * n).all(), (worst, float((d / n).max()))
    # the range accessor rebuilt its own temporary plane, before V existed (bar: tests/test_gpu_parity.py's for this accessor)
    assert np.allclose(mn1, V1[:, :3].min(0), rtol=0, atol=1e-6) and np.allclose(mx1, V1[:, :3].max(0), rtol=0, atol=1e-6)
    # and the apply path after V exists is still the same one
    assert np.array_equal(f1.apply_layers(fresh, 4).cpu().numpy(), f0.apply_layers(fresh, 4).cpu().numpy())
    for f in (f0, f1, f_ref):
        f.close()


def test_wide_layout_of_D_and_the_sample_rows(nle, oracle, ctx, tables, plane):
    """a 12 x 12 grid (p = 144) keeps all K = 128 eigenvectors, the most the path takes: D and the sample rows are written
    on the device with the widest row stride, and k_apply_small reads 128 columns of them"""
    import torch
    nr, nc, hx, K, L = 12, 12, 12.0, K_MAX, 6
    V_o, S_o = oracle.train_filter(plane, nr, nc, hx, HY, T, K)
    assert S_o.size == K
    Y_o = oracle.apply_layers(V_o, S_o, plane, L).reshape(L, -1)
    x32 = torch.as_tensor(plane.astype(np.float32), device="cuda:0")
    f = nle.NLEFilter(ctx).train_filter(x32, nr, nc, hx, HY, T, K)
    assert f.diag()["formulation"] == nle.MODE_PHI_FREE and f.info()["K"] == K
    Y = f.apply_layers(x32, L).cpu().numpy().astype(np.float64)
    errs = [rel_l2(Y[j], Y_o[j]) for j in range(L)]
    print("p = 144, K = 128, L = 6: per-layer rel L2 vs oracle", ["%.2e" % e for e in errs])
    for j in range(L):
        assert errs[j] < PER_LAYER_TOL, f"layer {j}: {errs[j]:.3e}"
    f.close()


@pytest.mark.parametrize("L", [1, 6])
@pytest.mark.parametrize("K", [1, 50, K_MAX])
def test_layers_match_the_oracle(nle, oracle, ctx, tables, plane, K, L):
    import torch
    S_o, Y_o = _oracle_layers(oracle, plane, K, L)
    x32 = torch.as_tensor(plane.astype(np.float32), device="cuda:0")
    f = _train(nle, ctx, x32, K)
    assert f.info()["K"] == S_o.size
    Y = f.apply_layers(x32, L).cpu().numpy().astype(np.float64)
    errs = [rel_l2(Y[j], Y_o[j]) for j in range(L)]
    print(f"K = {K} (kept {S_o.size}), L = {L}: per-layer rel L2 vs oracle", ["%.2e" % e for e in errs],
          "layer norms", ["%.2e" % np.linalg.norm(Y_o[j]) for j in range(L)])
    for j in range(L):
        assert errs[j] < PER_LAYER_TOL, f"layer {j}: {errs[j]:.3e}"
    f.close()


def test_without_sorted_rows_the_copy_is_kept(nle, ctx, tables, plane, monkeypatch):
    """(that NLE_NO_SORTED_ROWS takes effect on the call it is set for: test_the_switch_selects_the_unsorted_path_per_call)"""
    f_sorted, _, fresh = _pair(nle, ctx, plane)
    Y_sorted = f_sorted.apply_layers(fresh, 4).cpu().numpy().astype(np.float64)
    monkeypatch.setenv("NLE_NO_SORTED_ROWS", "1")
    f0, f1, fresh = _pair(nle, ctx, plane)
    Y0 = f0.apply_layers(fresh, 4).cpu().numpy()
    Y1 = f1.apply_layers(fresh, 4).cpu().numpy()       # the unsorted kernels read the filter's plane in every apply
    assert np.array_equal(Y1, Y0)
    assert np.array_equal(f1.eigvecs().cpu().numpy(), f0.eigvecs().cpu().numpy())
    # the same filter up to the order of the fp64 sums (tests/test_gpu_parity.py holds the two forms to 1e-6)
    for j in range(4):
        assert rel_l2(Y0[j].astype(np.float64), Y_sorted[j]) < 1e-6, j
    for f in (f_sorted, f0, f1):
        f.close()
