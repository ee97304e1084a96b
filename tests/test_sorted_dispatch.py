"""Every column count reaches its kernel: the table formulation at nC = 1 .. 36 on each of its three kernel families.

The launchers of csrc/sorted.hip, csrc/sorted_planes.hip and csrc/tables.hip map the run-time column count onto one
instantiation per count (dispatch_columns, csrc/launch.h).  The other tests visit 1, 2, 4, 7, 8, 10-13, 16, 20, 30, 33
and 36 columns and not every form at each; a slip at, say, 23 columns would pass them.  Here each count trains and applies
three ways on a 24 x 148 plane (a few thousand pixels):

  as it is                                   moment pass, index-sum Gram, sorted expand
  NLE_SORTED_NO_MOMENTS + NLE_GRAM_PAIRS     the table pass up to 12 columns and the recurrence beyond; k_sorted_gram up to 11
                                             columns and k_sorted_gram_wide from 12 (its rows per launch change at 13, 17, 22, 33)
  NLE_NO_SORTED_ROWS                         k_hist_pix, k_hist_dot and the unsorted Gram

hx = W / 8 sits inside all three bandwidth predicates (sorted_moments_ok, sorted_recurrence, sorted_gsum_ok) at every
count, so no count falls back to another form; on the CPU oracle every count trains and keeps exactly the K asked for.
The bars are the ones the suite already holds for these pairs: layers against the oracle 1e-4 (test_gpu_parity.py),
forced forms against the default 1e-10 / 1e-7 and unsorted against sorted 1e-9 / 1e-6 (test_gpu_parity.py,
test_bandwidth_regimes.py); the default run twice is bitwise equal.
"""
import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu

H, W, NR, HY, T, L = 24, 148, 3, 30.0, 5, 3
HX = W / 8.0
FORCED = ("NLE_SORTED_NO_MOMENTS", "NLE_GRAM_PAIRS")
UNSORTED = ("NLE_NO_SORTED_ROWS",)
FORM_ENV = ("NLE_SORTED_TABLE", "NLE_SORTED_NO_MOMENTS", "NLE_GRAM_PAIRS", "NLE_NO_SORTED_ROWS", "NLE_ALL_LEVEL_TILES",
            "NLE_SORTED_WGS_PER_CU")


@pytest.fixture(scope="module")
def plane(oracle):
    x = oracle.synthetic_luminance(H, W)
    assert np.array_equal(x, np.rint(x)) and x.min() >= 40 and x.max() <= 216
    return x


@pytest.fixture()
def tables(ctx):
    ctx.set_mode(2)
    yield
    ctx.set_mode(0)


def _run(nle, ctx, monkeypatch, x32, nc, K, env=()):
    for k in FORM_ENV:
        monkeypatch.delenv(k, raising=False)
    for k in env:
        monkeypatch.setenv(k, "1")
    f = nle.NLEFilter(ctx).train_filter(x32, NR, nc, HX, HY, T, K)
    d, ev = f.diag(), f.eigvals.copy()
    Y = f.apply_layers(x32, L).cpu().numpy().reshape(L, -1)
    f.close()
    for k in env:
        monkeypatch.delenv(k)
    return d, ev, Y


@pytest.mark.parametrize("nc", range(1, 37))
def test_every_form_of_a_column_count_runs_and_agrees(nle, oracle, ctx, tables, monkeypatch, plane, nc):
    K = min(8, 3 * nc)
    x32 = plane.astype(np.float32)
    V_o, S_o = oracle.train_filter(plane, NR, nc, HX, HY, T, K)
    assert S_o.size == K                                       # the inputs: the oracle keeps the K asked for
    Y_o = oracle.apply_layers(V_o, S_o, plane, L).reshape(L, -1)

    base = _run(nle, ctx, monkeypatch, x32, nc, K)
    runs = {"default": base, "forced": _run(nle, ctx, monkeypatch, x32, nc, K, FORCED),
            "unsorted": _run(nle, ctx, monkeypatch, x32, nc, K, UNSORTED)}
    again = _run(nle, ctx, monkeypatch, x32, nc, K)

    for name, (d, ev, Y) in runs.items():
        assert d["formulation"] == nle.MODE_PHI_FREE, (nc, name, d)
        assert d["K"] == S_o.size and ev.size == S_o.size, (nc, name, d)
        errs = [rel_l2(Y[j], Y_o[j]) for j in range(L)]
        print("nc %d %s: layers against the oracle %s" % (nc, name, " ".join("%.2e" % e for e in errs)))
        assert np.isfinite(Y).all() and max(errs) < 1e-4, (nc, name, errs)

    _, ev0, Y0 = base
    for name, e_bar, y_bar in (("forced", 1e-10, 1e-7), ("unsorted", 1e-9, 1e-6)):
        _, ev, Y = runs[name]
        e_err, y_err = rel_l2(ev, ev0), [rel_l2(Y[j], Y0[j]) for j in range(L)]
        print("nc %d %s against default: eigenvalues %.2e layers %s" % (nc, name, e_err, " ".join("%.2e" % e for e in y_err)))
        assert e_err < e_bar, (nc, name, e_err)
        assert max(y_err) < y_bar, (nc, name, y_err)

    assert again[1].tobytes() == ev0.tobytes() and again[2].tobytes() == Y0.tobytes(), nc
