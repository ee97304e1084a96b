"""Apply on the plane the filter was trained on: the reduce half training left behind against the one apply computes.

A single-rank table filter with level-sorted rows keeps, from training, m = K^T (c o x) and x at the samples for its own
plane, and the plane itself in one byte per pixel; apply compares its input with that plane by content and, on a match,
skips its reduce half.  `Context.set_train_reduce(False)` turns both halves off.  Everything here is compared
bit for bit (array_equal on the fp32 outputs).  The verdict stays on the device -- the reduce kernels are launched either
way and return at once on a match -- so no counter shows which path ran: what these tests hold is that every path gives
the bits of the switch-off path, on the training plane, on an equal copy, and on a plane that differs in one pixel
(where reusing training's m would show in the output).  That the reuse is taken at all is the benchmark's business.

Shape: H = 70, W = 203 -- no multiple of four, rows shorter than a workgroup of the sorted kernels (512 chunks), and
70 * 203 = 14210 = 4 * 3552 + 2 pixels, so the check's scalar tail runs behind its four-pixel loads -- with 5 x 7 samples,
T = 3, K = 8, L = 3.  One train per switch setting, shared by the tests.
"""
import contextlib

import numpy as np
import pytest

H, W, NR, NC, HX, HY, T, K, L = 70, 203, 5, 7, 40.0, 30.0, 3, 8, 3


@contextlib.contextmanager
def switched_off(ctx):
    ctx.set_train_reduce(False)
    try:
        yield
    finally:
        ctx.set_train_reduce(True)


class Trained:
    """the plane on the device, a filter trained on it with the reuse on and one with it off"""

    def __init__(self, nle, oracle, ctx):
        import torch
        self.nle, self.ctx = nle, ctx
        self.x_np = oracle.synthetic_luminance(H, W).astype(np.float32)
        assert np.all(self.x_np == np.rint(self.x_np)) and self.x_np.min() >= 0 and self.x_np.max() <= 255
        self.x = torch.tensor(self.x_np, device="cuda:0")
        self.on = nle.NLEFilter(ctx).train_filter(self.x, NR, NC, HX, HY, T, K)
        with switched_off(self.ctx):
            self.off = nle.NLEFilter(ctx).train_filter(self.x, NR, NC, HX, HY, T, K)
        assert self.on.diag()["formulation"] == nle.MODE_PHI_FREE == self.off.diag()["formulation"]
        self.sample_pix = np.asarray(self.on.sample_pixels()).ravel()

    def layers(self, f, x):
        """apply_layers and one weighted apply of x"""
        Y = f.apply_layers(x, L).cpu().numpy().reshape(L, -1)
        y = f.apply(x, self.nle.transform_eigenvalues(f.eigvals, [2.0, 3.0, 4.0])).cpu().numpy().reshape(1, -1)
        return np.concatenate([Y, y])

    def slow(self, x):
        """the switch-off output on x: the filter trained without the reuse, applied without it"""
        with switched_off(self.ctx):
            return self.layers(self.off, x)


@pytest.fixture(scope="module")
def tr(nle, oracle, ctx):
    t = Trained(nle, oracle, ctx)
    yield t
    t.on.close()
    t.off.close()


@pytest.mark.gpu
def test_training_is_the_same_with_and_without_the_reuse(tr):
    assert np.array_equal(tr.on.eigvals, tr.off.eigvals)


@pytest.mark.gpu
def test_fast_path_equals_slow_path_on_the_training_plane(tr):
    fast = tr.layers(tr.on, tr.x)
    assert np.array_equal(fast, tr.slow(tr.x))
    # the switch set at apply time alone also takes the slow path, on the filter that holds training's reduce half
    with switched_off(tr.ctx):
        again = tr.layers(tr.on, tr.x)
    assert np.array_equal(again, fast)


def _changed_pixels(tr):
    samples = set(int(v) for v in tr.sample_pix)
    non_sample = next(i for i in range(W + 3, H * W) if i not in samples)
    return {"non_sample": non_sample, "sample": int(tr.sample_pix[len(tr.sample_pix) // 2]), "last": H * W - 1}


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["non_sample", "sample", "last"])
def test_a_changed_pixel_is_caught(tr, which):
    """the same buffer, one pixel changed in place after training"""
    pix = _changed_pixels(tr)[which]
    assert (pix in set(int(v) for v in tr.sample_pix)) == (which == "sample")
    flat = tr.x.view(-1)
    old = float(flat[pix])
    try:
        flat[pix] = old + 1.0 if old < 255.0 else old - 1.0
        got = tr.layers(tr.on, tr.x)
        want = tr.slow(tr.x)
    finally:
        flat[pix] = old
    assert np.array_equal(got, want), "the changed plane was taken for the training plane"
    assert not np.array_equal(got, tr.slow(tr.x)), "the changed pixel does not show in the output: the case proves nothing"


@pytest.mark.gpu
def test_an_equal_copy_in_another_buffer(tr):
    import torch
    copy = torch.tensor(tr.x_np, device="cuda:0")
    assert copy.data_ptr() != tr.x.data_ptr()
    assert np.array_equal(tr.layers(tr.on, copy), tr.layers(tr.on, tr.x))


@pytest.mark.gpu
def test_minus_zero_in_place_of_level_zero(tr, nle, ctx):
    """-0.0f equals 0.0f as a number and differs in its bits: the check compares bits, so such a plane computes its own m,
    and -0 * c adds nothing to any sum: the outputs are those of the plane with +0"""
    import torch
    x0 = tr.x_np.copy()
    x0[3, 5] = 0.0
    x0[H - 1, W - 1] = 0.0
    xt = torch.tensor(x0, device="cuda:0")
    f = nle.NLEFilter(ctx).train_filter(xt, NR, NC, HX, HY, T, K)
    try:
        same = tr.layers(f, xt)
        xm = xt.clone()
        xm.view(-1)[3 * W + 5] = -0.0
        assert torch.equal(xm, xt) and not np.array_equal(xm.cpu().numpy().view(np.uint32), x0.view(np.uint32))
        got = tr.layers(f, xm)
    finally:
        f.close()
    assert np.array_equal(got, same)
