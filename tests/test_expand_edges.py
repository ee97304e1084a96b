"""The expand half of the table apply (k_sorted_expand) at the edges of its row pipeline.

The kernel runs one workgroup per compute unit; each walks rows r, r + CUs, r + 2 CUs, ... and requests the next row's
descriptor, indices, table values and first c values while it works on the current one.  The heights here are the ones at
which that hand-over can go wrong: H = 3 (fewer rows than workgroups: no workgroup has a next row), H = CUs + 1 (exactly
one workgroup has a second row) and H = 2 CUs + 5 (some workgroups take three rows, most two).  Layers: 1, 4 (a full
launch of the four-layer instantiation) and 5 (a full group and a remainder); grids with 10 sample columns (four layers
per launch) and 13 (the two-layer instantiation, column factors by recurrence where the bandwidth allows).

Reference: the same train and apply on the unsorted kernels (NLE_NO_SORTED_ROWS: k_hist_dot in image order).  The two are
not bit-equal -- the unsorted train sums with LDS atomics and differs from run to run in its last bits (CHANGELOG.md) -- so
the bars are the ones tests/test_bandwidth_regimes.py holds a forced form to against the default run
(_agrees_across_forms): eigenvalues within 1e-10, every plane within 1e-7 relative L2, and no pixel further than A_REL
max|Y[j]| beyond one fp32 ulp.  The sample pixels are written by k_scatter_samples and compared like the rest.
"""
import contextlib
import os

import numpy as np
import pytest

from conftest import rel_l2
from test_bandwidth_regimes import A_REL, ULP32

W, HX, HY, T, K = 64, 16.0, 30.0, 3, 8
LAYERS = (1, 4, 5)


def n_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


HEIGHTS = {"3": lambda: 3, "cus+1": lambda: n_cus() + 1, "2cus+5": lambda: 2 * n_cus() + 5}


@contextlib.contextmanager
def unsorted_rows():
    assert "NLE_NO_SORTED_ROWS" not in os.environ
    os.environ["NLE_NO_SORTED_ROWS"] = "1"
    try:
        yield
    finally:
        del os.environ["NLE_NO_SORTED_ROWS"]


def run(nle, ctx, x, nr, nc):
    """eigenvalues and, per L, the L layers of x on a filter trained here (one train for all three L)"""
    f = nle.NLEFilter(ctx).train_filter(x, nr, nc, HX, HY, T, K)
    try:
        assert f.diag()["formulation"] == nle.MODE_PHI_FREE
        assert nle.sample_grid(x.shape[0], W, nr, nc)["n_sel_cols"] == nc
        return f.eigvals.copy(), {L: f.apply_layers(x, L).cpu().numpy().reshape(L, -1) for L in LAYERS}
    finally:
        f.close()


_RUNS = {}


def both(nle, oracle, ctx, hname, nc):
    """(sorted, unsorted, sorted again) results of one shape, computed once; a failure is kept and raised again"""
    key = (hname, nc)
    if key not in _RUNS:
        try:
            H = HEIGHTS[hname]()
            nr = 1 if H < 8 else 4
            x = oracle.synthetic_luminance(H, W).astype(np.float32)
            assert np.all(x == np.rint(x)) and x.min() >= 0 and x.max() <= 255
            srt = run(nle, ctx, x, nr, nc)
            with unsorted_rows():
                uns = run(nle, ctx, x, nr, nc)
            _RUNS[key] = (srt, uns, run(nle, ctx, x, nr, nc))
        except (Exception, pytest.fail.Exception) as e:
            _RUNS[key] = e
            raise
    if isinstance(_RUNS[key], BaseException):
        raise RuntimeError("the device runs of %s failed earlier: %r" % (key, _RUNS[key]))
    return _RUNS[key]


def excess(Y, ref):
    """max over the pixels of (|Y - ref| - 2^-23 |ref|) / max|ref|, floored at 0 (test_bandwidth_regimes.excess, one plane)"""
    Y, ref = Y.astype(np.float64), ref.astype(np.float64)
    d = np.abs(Y - ref) - ULP32 * np.abs(ref)
    if not np.all(np.isfinite(d)):
        return np.inf
    return max(0.0, float(d.max())) / float(np.abs(ref).max())


@pytest.mark.gpu
@pytest.mark.parametrize("nc", [10, 13])
@pytest.mark.parametrize("hname", list(HEIGHTS))
@pytest.mark.parametrize("L", LAYERS)
def test_expand_on_sorted_rows_agrees_with_the_unsorted_kernels(nle, oracle, ctx, hname, nc, L):
    (ev_s, Y_s), (ev_u, Y_u), _ = both(nle, oracle, ctx, hname, nc)
    assert ev_s.size == ev_u.size == K
    e_eig = rel_l2(ev_s, ev_u)
    figs = [(rel_l2(Y_s[L][j], Y_u[L][j]), excess(Y_s[L][j], Y_u[L][j])) for j in range(L)]
    print("H %s nC %d L %d: bitwise %s, eig %.2e," % (hname, nc, L, np.array_equal(Y_s[L], Y_u[L]), e_eig),
          ["l2 %.2e excess %.2e" % f for f in figs])
    assert e_eig < 1e-10, e_eig
    for j, (l2, e) in enumerate(figs):
        assert l2 < 1e-7, (j, l2)
        assert e <= A_REL, "layer %d: a pixel is %.3e max|Y| beyond one fp32 ulp of the unsorted kernels (bound %.1e)" % (j, e, A_REL)


@pytest.mark.gpu
@pytest.mark.parametrize("nc", [10, 13])
@pytest.mark.parametrize("hname", list(HEIGHTS))
def test_expand_on_sorted_rows_is_bitwise_reproducible(nle, oracle, ctx, hname, nc):
    """a second train and apply on the sorted rows: the same bits (no atomics, and no row of the pipeline reads what another
    is still writing)"""
    (ev_s, Y_s), _, (ev_2, Y_2) = both(nle, oracle, ctx, hname, nc)
    assert np.array_equal(ev_s, ev_2)
    for L in LAYERS:
        assert np.array_equal(Y_s[L], Y_2[L]), L
