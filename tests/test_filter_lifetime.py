"""Who owns a filter's device memory, and when it goes back (csrc/pipeline_internal.h: nle_filter, DevBuf).

A filter holds its eigenvectors (fp32, fp64 or both), its table state and -- trained from a host plane -- the training plane
in buffers that return to the workspace cache of the ctx they were made on: when the filter is closed, and when a train fails
after the filter object exists.  A ctx that is closed before its filter leaves the filter's V and plane alive (they are freed
with the filter) and takes the table state with it.  None of that may change a number: a block that comes back out of the
cache is fully rewritten by the next train, so every comparison below is bitwise.

Every form a filter's state takes appears once: the table form (V implicit) and the same after eigvecs() has materialised the
fp32 V, the fp32 V of MODE_MATERIALISED, the fp64 V of auto mode on a plane that is not integer valued and the same with the
fp32 copy beside it, MODE_STREAMED_F64, MODE_EXACT_F64 (on the 24 x 32 crop: N = 768 pixels against a basis of 96 columns, so
the block Lanczos branch runs), and a host-trained filter applied to the plane it kept.  No case reads the amount of free
device memory: the cards are shared.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W, NR, NC, HX, HY, T, K, L = 48, 64, 6, 8, 32.0, 30.0, 4, 8, 3

# form -> (mode, plane, expected formulation, materialise V after the train, host-trained)
FORMS = {
    "tables": ("MODE_AUTO", "int", "MODE_PHI_FREE", False, False),
    "tables+V": ("MODE_AUTO", "int", "MODE_PHI_FREE", True, False),
    "materialised": ("MODE_MATERIALISED", "int", "MODE_MATERIALISED", False, False),
    "auto_f64": ("MODE_AUTO", "frac", "MODE_MATERIALISED_F64", False, False),
    "auto_f64+V": ("MODE_AUTO", "frac", "MODE_MATERIALISED_F64", True, False),
    "streamed_f64": ("MODE_STREAMED_F64", "int", "MODE_STREAMED_F64", False, False),
    "exact": ("MODE_EXACT_F64", "crop", "MODE_EXACT_F64", False, False),
    "host": ("MODE_AUTO", "int", "MODE_PHI_FREE", False, True),
}


@pytest.fixture(scope="module")
def planes(oracle):
    x = oracle.synthetic_luminance(H, W).astype(np.float32)
    assert np.array_equal(x, np.rint(x))
    return {"int": x, "frac": x + np.float32(0.25), "crop": np.ascontiguousarray(x[:24, :32]),
            "crop_frac": np.ascontiguousarray(x[:24, :32]) + np.float32(0.25)}


def _train(nle, ctx, mode, x, host=False, nr=NR, nc=NC):
    ctx.set_mode(getattr(nle, mode))
    try:
        flt = nle.NLEFilter(ctx)
        return (flt.train_filter_host if host else flt.train_filter)(x, nr, nc, HX, HY, T, K)
    finally:
        ctx.set_mode(nle.MODE_AUTO)


def _state(flt):
    """what the accessors that need no ctx answer"""
    return flt.info(), flt.diag(), flt.eigvals


def _run(nle, ctx, planes, form):
    """(filter, layers, state) of one form; the filter is the caller's to close"""
    mode, kind, formulation, want_V, host = FORMS[form]
    x = planes[kind]
    flt = _train(nle, ctx, mode, x, host)
    assert flt.diag()["formulation"] == getattr(nle, formulation)
    if want_V:
        assert np.isfinite(flt.eigvecs().cpu().numpy()).all()
    if host:
        Y = flt.apply_layers_host(None, L, np.empty((L, x.size), dtype=np.float32))
    else:
        Y = flt.apply_layers(x, L).cpu().numpy()
    assert np.isfinite(Y).all() and np.abs(Y).max() > 1.0
    return flt, Y, _state(flt)


def _assert_same(got, want):
    (Y, (info, diag, ev)), (Y0, (info0, diag0, ev0)) = got, want
    assert info == info0 and diag == diag0
    assert np.array_equal(ev, ev0)
    assert np.array_equal(Y, Y0)


@pytest.mark.parametrize("form", list(FORMS))
def test_a_closed_filters_blocks_are_recycled_without_a_trace(nle, ctx, planes, form):
    flt, Y0, s0 = _run(nle, ctx, planes, form)
    flt.close()
    flt, Y1, s1 = _run(nle, ctx, planes, form)  # the same sizes: served from the blocks the first one gave back
    flt.close()
    _assert_same((Y1, s1), (Y0, s0))


@pytest.mark.parametrize("form", list(FORMS))
def test_a_filter_outlives_its_ctx(nle, planes, form):
    own = nle.Context(0)
    flt, Y0, s0 = _run(nle, own, planes, form)
    own.close()
    info, diag, ev = _state(flt)  # the orphaned handle still answers
    assert info == s0[0] and diag == s0[1] and np.array_equal(ev, s0[2])
    flt.close()
    fresh = nle.Context(0)
    flt, Y1, s1 = _run(nle, fresh, planes, form)
    flt.close()
    fresh.close()
    _assert_same((Y1, s1), (Y0, s0))


REFUSALS = {
    # the plane is checked on the device (check_exact_plane) after the filter object exists
    "exact_plane": ("MODE_EXACT_F64", "crop_frac", "crop", NR, NC,
                    "NLE_MODE_EXACT_F64 needs an integer-valued luminance plane in [0, 255] (the L channel of 8-bit Lab)"),
    # 272 samples: too many for the generic Phi-free kernels, and the table kernels need integer levels
    "phi_free_plane": ("MODE_PHI_FREE", "frac", "int", 17, 16,
                       "Phi-free path: more than 256 samples needs an integer-valued luminance plane"),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_a_train_that_fails_late_leaves_the_ctx_as_it_was(nle, planes, case):
    mode, bad, good, nr, nc, text = REFUSALS[case]

    def outputs(c):
        flt = _train(nle, c, mode, planes[good], nr=nr, nc=nc)
        Y = flt.apply_layers(planes[good], L).cpu().numpy()
        s = _state(flt)
        flt.close()
        return Y, s

    c = nle.Context(0)
    with pytest.raises(nle.NLEError) as e:
        _train(nle, c, mode, planes[bad], nr=nr, nc=nc)
    assert e.value.code == nle.NLE_ERR_INVALID and str(e.value) == text
    after = outputs(c)
    c.close()
    fresh = nle.Context(0)
    want = outputs(fresh)
    fresh.close()
    assert np.isfinite(want[0]).all() and np.abs(want[0]).max() > 1.0
    _assert_same(after, want)
