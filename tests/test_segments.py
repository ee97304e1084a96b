"""Automatic regions: nle_segment_init / nle_segment_stats / nle_segment_assign / nle_filter_segment and their Python mirror.

The restatement below is the contract of include/nle.h ("automatic regions"), in numpy.  A trained filter has K' pairs
(V, lambda); labels l_i in 0 .. C - 1, one byte per pixel; the spread t.  One iteration, from labels l:

    counts    n_c = #{i : l_i = c}; a cluster with n_c = 0 is inactive
    spread    q_c = apply(indicator of c, (N / n_c) lambda^t), 0 for an inactive cluster, an fp32 plane
    means     m_c = (sum over the members of c of (double)q_c[i]) / n_c, +inf for an inactive cluster
    reassign  score_c = m_c - 2 (double)q_c[i]; a NaN score counts as +inf; l'_i = the smallest c with the smallest score;
              where every score is +inf the pixel keeps l_i
    objective J = (sum over the active c of n_c m_c) / N, for the labels that entered the iteration

Stop when an iteration changes no label, or after the cap.  The start: equal-population cuts on the quarter-level histogram of
a plane, b_c = the first bin whose cumulative count reaches floor(N c / C) + 1, l_i = #{c : bin(x_i) >= b_c}."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, rel_l2

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_patch_affinity as tpa  # noqa: E402
import test_region_edits as tre  # noqa: E402

SYNTH = tpa.SYNTH  # 72 x 96, nr 6, nc 8, hx 16, hy 30, T 10, K 12, L 4
SPREAD = 4.0
PER_LAYER_TOL = 1e-4  # the project's standing per-layer bar: a spread is an apply with one response
BINS = 4096
INF = float("inf")


# ----------------------------------------------------------------------------------------------- the restatement
def bins(x):
    """bin(x) = floor((x + 256) 4) clamped to [-1, 4096], a NaN taken as 4096"""
    t = (np.asarray(x, dtype=np.float32).astype(np.float64).ravel() + 256.0) * 4.0
    with np.errstate(invalid="ignore"):
        b = np.where(np.isnan(t), float(BINS), np.clip(np.floor(t), -1.0, float(BINS)))
    return b.astype(np.int64)


def histogram(x):
    """the counts of nle_plane_histogram(x, 1): underflow, the 4096 bins, overflow and NaN"""
    return np.bincount(bins(x) + 1, minlength=BINS + 2).astype(np.int64)


def start_cuts(counts, N, Cn):
    cum = counts[0] + np.cumsum(counts[1:BINS + 1])
    cuts = []
    for c in range(1, Cn):
        hit = np.nonzero(cum >= (N * c) // Cn + 1)[0]
        cuts.append(int(hit[0]) if hit.size else BINS)
    return np.array(cuts, dtype=np.int64)


def start_labels(x, Cn):
    """(labels uint8, cuts) of the equal-population start"""
    b = bins(x)
    cuts = start_cuts(histogram(x), b.size, Cn)
    return (b[None, :] >= cuts[:, None]).sum(0).astype(np.uint8), cuts


def indicators(labels, Cn):
    return (np.asarray(labels)[None, :] == np.arange(Cn)[:, None]).astype(np.float32)


def stats(Q, labels, Cn, dtype=np.float64):
    """counts and the sums of q_{l_i}[i] over the members (a stride-0 Q is one plane for every cluster)"""
    labels = np.asarray(labels)
    own = np.asarray(Q)[labels, np.arange(labels.size)].astype(dtype)
    return (np.bincount(labels, minlength=Cn).astype(np.int64),
            np.array([own[labels == c].sum(dtype=dtype) for c in range(Cn)], dtype=dtype))


def means(counts, sums):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(counts > 0, np.asarray(sums, dtype=np.float64) / counts, INF)


def assign(Q, m, labels):
    """(new labels, new counts, changed) of one reassignment"""
    Q = np.asarray(Q, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        s = np.asarray(m, dtype=np.float64)[:, None] - 2.0 * Q.astype(np.float64)
    s = np.where(np.isnan(s), INF, s)
    best = s.min(0)
    new = np.where(best == INF, np.asarray(labels), s.argmin(0)).astype(np.uint8)  # argmin: the first of equal scores
    return new, np.bincount(new, minlength=Q.shape[0]).astype(np.int64), int((new != labels).sum())


def objective(counts, m):
    J = 0.0
    for c in range(len(counts)):
        if counts[c]:
            J = J + float(counts[c]) * m[c]
    return J / float(counts.sum())


def oracle_spread(oracle, V, S, labels, Cn, t):
    """the fp32 spread planes (C, n) of the labels' indicator planes, scale N / n_c (0: inactive)"""
    n = labels.size
    counts = np.bincount(labels, minlength=Cn)
    ind = indicators(labels, Cn).astype(np.float64)
    return np.stack([oracle.apply_filter(V, ind[c], (n / counts[c] if counts[c] else 0.0) * np.power(S, t))
                     for c in range(Cn)]).astype(np.float32)


def iterate(oracle, V, S, labels, Cn, t, max_iter):
    """the loop on the oracle's filter: (labels, objective history, converged, spreads of the last iteration)"""
    labels = np.asarray(labels, dtype=np.uint8).copy()
    hist, converged, Q = [], False, None
    while len(hist) < max_iter and not converged:
        Q = oracle_spread(oracle, V, S, labels, Cn, t)
        counts, sums = stats(Q, labels, Cn)
        m = means(counts, sums)
        hist.append(objective(counts, m))
        labels, _, changed = assign(Q, m, labels)
        converged = changed == 0
    return labels, hist, converged, Q


_cache = {}


def _synth(oracle):
    if "synth" not in _cache:
        H, W, nr, nc, hx, hy, T, K, _ = SYNTH
        x = oracle.synthetic_luminance(H, W)
        _cache["synth"] = (x,) + tuple(oracle.train_filter(x, nr, nc, hx, hy, T, K))
    return _cache["synth"]


BLOCKS = (48, 64, 6, 8, 16.0, 30.0, 10, 12)  # H, W, nr, nc, hx, hy, T, K


def _blocks():
    """the three-block scene: levels 60 / 128 / 200 under integer noise, and its truth"""
    H, W = BLOCKS[:2]
    truth = np.zeros((H, W), dtype=np.uint8)
    truth[:, 22:] = 1
    truth[26:, 40:] = 2
    x = np.array([60.0, 128.0, 200.0])[truth] + np.random.default_rng(5).integers(-3, 4, size=(H, W))
    return x, truth.ravel()


# ------------------------------------------------------------------------------------------------------ CPU tests
def test_restatement_by_hand():
    """five pixels, three clusters, scalar by scalar: a tie, a NaN, an inactive cluster, a pixel whose scores are all +inf"""
    nan = float("nan")
    Q = np.array([[1.0, 0.5, nan, nan, -0.0],
                  [1.0, 2.0, 0.25, nan, 0.0],
                  [9.0, 9.0, 9.0, nan, 9.0]], dtype=np.float32)
    m = np.array([1.5, 1.5, INF])  # cluster 2 is inactive
    old = np.array([2, 0, 1, 2, 1], dtype=np.uint8)
    new, counts, changed = assign(Q, m, old)
    # pixel 0: scores -0.5, -0.5, +inf: the tie goes to the smaller c.  pixel 1: 0.5, -2.5.  pixel 2: NaN -> +inf, 1.0.
    # pixel 3: NaN, NaN, +inf - NaN: nothing is finite, the label stays.  pixel 4: 1.5 + 0 and 1.5 - 0 tie: cluster 0.
    assert new.tolist() == [0, 1, 1, 2, 0] and counts.tolist() == [2, 2, 1] and changed == 3
    for i in range(5):
        best, arg = INF, -1
        for c in range(3):
            s = float(m[c]) - 2.0 * float(Q[c, i])
            if s != s:
                s = INF
            if s < best:
                best, arg = s, c
        assert (old[i] if arg < 0 else arg) == new[i]
    # an inactive cluster attracts nothing, whatever its plane holds
    assert not (assign(np.full((2, 4), 100.0, dtype=np.float32), [INF, 0.0], np.zeros(4, np.uint8))[0] == 0).any()
    # every cluster inactive: nothing moves
    assert assign(Q, [INF] * 3, old)[2] == 0
    # stats: each pixel contributes its own cluster's value; means; the objective
    Qs = np.arange(15, dtype=np.float32).reshape(3, 5)
    counts, sums = stats(Qs, np.array([0, 0, 2, 2, 2]), 3)
    assert counts.tolist() == [2, 0, 3] and sums.tolist() == [1.0, 0.0, 12.0 + 13.0 + 14.0]
    mm = means(counts, sums)
    assert mm.tolist() == [0.5, INF, 13.0] and objective(counts, mm) == (2 * 0.5 + 3 * 13.0) / 5
    # the start: five levels into two clusters of three and two, an out-of-range value and a NaN at the two ends
    lab, cuts = start_labels(np.array([-300.0, 5.0, 5.25, 900.0, nan]), 3)
    assert bins([-300.0, 5.0, 5.25, 900.0, nan]).tolist() == [-1, 1044, 1045, 4096, 4096]
    assert cuts.tolist() == [1044, 4096] and lab.tolist() == [0, 1, 1, 2, 2]
    assert start_labels(np.full(7, 3.0), 4)[0].tolist() == [3] * 7  # a flat plane: every cut is its bin, one cluster holds all


def test_start_cut_rule_at_the_boundary():
    """b_c is the FIRST bin whose cumulative count reaches floor(N c / C) + 1: three pixels at 10 are not enough for 3"""
    x = np.array([10.0, 10.0, 20.0, 20.0, 20.0])
    lab, cuts = start_labels(x, 2)  # needs 5 // 2 + 1 = 3: reached at bin(20)
    assert cuts.tolist() == [(20 + 256) * 4] and lab.tolist() == [0, 0, 1, 1, 1]
    x = np.array([10.0, 10.0, 10.0, 20.0, 20.0])
    lab, cuts = start_labels(x, 2)  # reached at bin(10): the cut sits at the level itself and cluster 0 is empty
    assert cuts.tolist() == [(10 + 256) * 4] and lab.tolist() == [1] * 5


@pytest.mark.parametrize("Cn", [2, 3, 4])
def test_objective_never_drops_and_the_loop_settles_on_the_oracle(oracle, Cn):
    x, V, S = _synth(oracle)
    lab0, _ = start_labels(x, Cn)
    labels, hist, converged, _ = iterate(oracle, V, S, lab0, Cn, SPREAD, 40)
    steps = np.diff(hist)
    print(f"C = {Cn}: {len(hist)} iterations, J {hist[0]:.6f} -> {hist[-1]:.6f}, smallest step {steps.min() if steps.size else 0:.2e}")
    assert converged and len(hist) <= 40
    # the spreads are fp32 planes: J is known to 1e-6 |J|
    assert all(hist[k + 1] >= hist[k] - 1e-6 * abs(hist[k]) for k in range(len(hist) - 1))
    assert np.bincount(labels, minlength=Cn).sum() == x.size


def test_three_blocks_end_at_the_truth_on_the_oracle(oracle):
    x, truth = _blocks()
    H, W, nr, nc, hx, hy, T, K = BLOCKS
    V, S = oracle.train_filter(x, nr, nc, hx, hy, T, K)
    lab0, _ = start_labels(x, 3)
    assert not np.array_equal(lab0, truth)  # the loop has work to do
    labels, hist, converged, _ = iterate(oracle, V, S, lab0, 3, SPREAD, 40)
    print(f"three blocks: {len(hist)} iterations, {int((lab0 != truth).sum())} start labels off the truth")
    assert converged and np.array_equal(labels, truth)


def test_segments_are_declared_exported_and_mirrored(nle):
    hdr = " ".join(open(os.path.join(ROOT, "include", "nle.h")).read().split())
    for decl in ("int nle_segment_init(nle_ctx* ctx, const float* d_x, long long n, int C, unsigned char* d_labels, int* h_cuts);",
                 "int nle_segment_stats(nle_ctx* ctx, const float* d_q, int C, long long n, long long q_stride, "
                 "const unsigned char* d_labels, long long* h_counts, double* h_sums);",
                 "int nle_segment_assign(nle_ctx* ctx, const float* d_q, int C, long long n, long long q_stride, const double* h_m, "
                 "unsigned char* d_labels, float* d_indicators, long long ind_stride, long long* h_counts, long long* h_changed);",
                 "int nle_filter_segment(nle_filter* f, int H, int W, int C, double spread, int max_iter, unsigned char* d_labels, "
                 "float* d_q, long long q_stride, long long* h_counts, double* h_objective, int* h_iters, int* h_converged);",
                 "#define NLE_SEGMENT_ITERATIONS_MAX 200"):
        assert decl in hdr, decl
    from nle_amd import _abi
    assert _abi.NLE_SEGMENT_ITERATIONS_MAX == 200 == nle.SEGMENT_ITERATIONS_MAX
    assert _abi.NLE_KERNEL_COUNT_ALL == 16  # the segment kernels have no ids
    for name in ("nle_segment_init", "nle_segment_stats", "nle_segment_assign", "nle_filter_segment"):
        assert name in _abi.SIGNATURES and name in nle.EXPORTED_SYMBOLS
        assert hasattr(nle.lib(), name)  # exported by the built library
    for name in ("segment_init", "segment_stats", "segment_assign"):
        assert callable(getattr(nle.Context, name, None)), name
    assert callable(getattr(nle.NLEFilter, "segment", None))


# ------------------------------------------------------------------------------------------------------ GPU tests
@pytest.fixture
def sctx(ctx):
    """the session ctx, handed back in auto mode whatever the test did"""
    yield ctx
    ctx.set_mode(0)


CS = [1, 2, 3, 5, 8]
NS = [1, 3, 4, 5, 1023, 4 * 256 * 4096 + 5]  # the last: the grid-stride loop of four pixels per thread takes a second trip


def _layouts(n):
    """(name, plane stride, offset in elements): planes n apart on an aligned base (for n no multiple of 4 the stride alone
    forbids the 16-byte accesses), planes n + 3 apart with every pointer off by one element or byte, and 16-byte aligned
    planes at n rounded up"""
    return (("stride_n", n, 0), ("offset", n + 3, 1), ("aligned", (n + 3) & ~3, 0))


def _strided(torch, rows, stride, offset, dev, fill=float("nan")):
    k, n = rows.shape
    buf = torch.full((offset + k * stride + 8,), fill, dtype=torch.float32, device=dev)
    view = torch.as_strided(buf, (k, n), (stride, 1), offset)
    view.copy_(torch.as_tensor(rows, device=dev))
    return buf, view


def _label_view(torch, labels, offset, dev):
    buf = torch.full((labels.size + offset + 8,), 255, dtype=torch.uint8, device=dev)
    buf[offset:offset + labels.size] = torch.as_tensor(labels, device=dev)
    return buf, buf[offset:offset + labels.size]


def _plant_nans(Q, seed):
    """one NaN in a random cluster at every 11th pixel, all clusters NaN at every 13th"""
    rng = np.random.default_rng(seed)
    Cn, n = Q.shape
    i = np.arange(n)
    one = np.nonzero(i % 11 == 2)[0]
    Q[rng.integers(0, Cn, size=one.size), one] = np.nan
    Q[:, i % 13 == 4] = np.nan
    return Q


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("Cn", CS)
def test_segment_assign_is_the_restatement_exactly(nle, ctx, Cn, n):
    import torch
    dev = f"cuda:{ctx.device}"
    rng = np.random.default_rng(100 * Cn + n % 9973)
    Q = rng.normal(size=(Cn, n)).astype(np.float32)
    m = rng.normal(size=Cn) * 0.5
    old = rng.integers(0, Cn, size=n).astype(np.uint8)
    i = np.arange(n)
    if Cn >= 2:
        m[1] = m[0]
        tie = i % 7 == 3  # clusters 0 and 1 share the best score: 0 must win
        Q[:, tie] = -3.0
        Q[:2, tie] = 5.0
        zero = i % 17 == 6  # +0 against -0 under equal means: the scores are equal
        Q[:, zero] = -3.0
        Q[0, zero], Q[1, zero] = 0.0, -0.0
    if Cn >= 4:
        m[Cn - 1] = m[Cn - 2]
        tie2 = i % 7 == 5  # the same between the last two clusters: the smaller of them
        Q[:, tie2] = -3.0
        Q[Cn - 2:, tie2] = 5.0
    Q = _plant_nans(Q, n)
    one_off = m.copy()
    if Cn >= 3:
        one_off[2] = INF  # one cluster inactive
    variants = [("means", one_off)]
    if n <= 1023:
        variants += [("first inactive", np.concatenate([[INF], m[1:]])), ("all inactive", np.full(Cn, INF))]
    for vname, mv in variants:
        want, want_counts, want_changed = assign(Q, mv, old)
        if vname == "means" and n >= 1023:  # the inputs reach what they are meant to reach
            assert (want_changed > 0 or Cn == 1) and np.isnan(Q).all(0).any()
            clean = ~np.isnan(Q).any(0)
            if Cn >= 2:
                assert (want[(i % 7 == 3) & clean] == 0).all()
                assert (want[(i % 17 == 6) & (i % 7 != 3) & (i % 7 != 5) & clean] == 0).all()
            if Cn >= 4:
                assert (want[(i % 7 == 5) & clean] == Cn - 2).all()
            if Cn >= 3:
                assert not (want[clean] == 2).any()
        if vname == "all inactive":
            assert want_changed == 0
        for lname, stride, off in _layouts(n):
            _, Qd = _strided(torch, Q, stride, off, dev)
            for with_ind in (True, False):
                lbuf, lab = _label_view(torch, old, off, dev)
                ibuf = ind = None
                if with_ind:
                    ibuf, ind = _strided(torch, np.full((Cn, n), 7.0, dtype=np.float32), stride, off, dev, fill=7.0)
                got = ctx.segment_assign(Qd, mv, lab, indicators=ind)
                torch.cuda.synchronize()
                where = (vname, lname, with_ind)
                lb = lbuf.cpu().numpy()
                assert (lb[:off] == 255).all() and (lb[off + n:] == 255).all(), where  # nothing written either side
                assert np.array_equal(lb[off:off + n], want), where
                assert np.array_equal(got[0], want_counts) and got[1] == want_changed, where
                if with_ind:
                    assert np.array_equal(ind.cpu().numpy(), indicators(want, Cn)), where
                    flat = ibuf.cpu().numpy()
                    mask = np.ones(flat.size, dtype=bool)
                    for c in range(Cn):
                        mask[off + c * stride: off + c * stride + n] = False
                    assert (flat[mask] == 7.0).all(), where  # nor between the planes


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("Cn", CS)
def test_segment_stats_counts_and_sums(nle, ctx, Cn, n):
    import torch
    dev = f"cuda:{ctx.device}"
    rng = np.random.default_rng(7 * Cn + n % 9973)
    # labels that change from pixel to pixel, and runs of eight (inside a segment four aligned pixels share theirs)
    scattered = rng.integers(0, Cn, size=n).astype(np.uint8)
    runs = np.repeat(rng.integers(0, Cn, size=(n + 7) // 8), 8)[:n].astype(np.uint8)
    for labels in (scattered, runs):
        Qi = rng.integers(-1000, 1001, size=(Cn, n)).astype(np.float32)
        Qr = (rng.normal(size=(Cn, n)) * 3 + 1).astype(np.float32)
        counts_i, sums_i = stats(Qi, labels, Cn)
        counts_r, sums_r = stats(Qr, labels, Cn, dtype=np.longdouble)
        own = np.abs(Qr[labels, np.arange(n)].astype(np.longdouble))
        # the worst case of an fp64 sum of n_c terms in any order: (n_c - 1) 2^-53 sum |q| to first order; n_c 2^-52 bounds it
        bound = np.array([counts_r[c] * 2.0 ** -52 * float(own[labels == c].sum()) for c in range(Cn)])
        for lname, stride, off in _layouts(n):
            _, lab = _label_view(torch, labels, off, dev)
            _, Qd = _strided(torch, Qi, stride, off, dev)
            got = ctx.segment_stats(Qd, lab)
            assert np.array_equal(got[0], counts_i) and np.array_equal(got[1], sums_i), lname  # integers: exact in any order
            _, Qd = _strided(torch, Qr, stride, off, dev)
            a, b = ctx.segment_stats(Qd, lab), ctx.segment_stats(Qd, lab)
            assert np.array_equal(a[0], counts_r) and np.array_equal(a[0], b[0]), lname
            assert np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)), lname  # two calls: the same bits
            err = np.abs(a[1].astype(np.longdouble) - sums_r).astype(np.float64)
            assert (err <= bound).all(), (lname, err, bound)
            # q_stride = 0: every cluster reads the one plane
            one = Qd[0].expand(Cn, n) if Cn > 1 else Qd
            got = ctx.segment_stats(one, lab)
            want = stats(np.broadcast_to(Qr[0], (Cn, n)), labels, Cn, dtype=np.longdouble)
            own0 = np.abs(Qr[0].astype(np.longdouble))
            bound0 = np.array([counts_r[c] * 2.0 ** -52 * float(own0[labels == c].sum()) for c in range(Cn)])
            assert np.array_equal(got[0], counts_r), lname
            assert (np.abs(got[1].astype(np.longdouble) - want[1]).astype(np.float64) <= bound0).all(), lname


@pytest.mark.gpu
def test_segment_stats_refuses_a_label_out_of_range(nle, ctx):
    import torch
    dev = f"cuda:{ctx.device}"
    for Cn, n, at in ((3, 1023, 700), (8, 5, 4), (1, 4, 0)):
        labels = np.zeros(n, dtype=np.uint8)
        labels[at] = Cn
        Q = torch.ones((Cn, n), dtype=torch.float32, device=dev)
        with pytest.raises(nle.NLEError) as e:
            ctx.segment_stats(Q, labels)
        assert e.value.code == nle.NLE_ERR_INVALID and "label" in str(e.value)
        with pytest.raises(nle.NLEError) as e:
            ctx.segment_assign(Q, np.zeros(Cn), labels)
        assert e.value.code == nle.NLE_ERR_INVALID and "label" in str(e.value)
        labels[at] = 0
        assert ctx.segment_stats(Q, labels)[0].tolist() == [n] + [0] * (Cn - 1)  # the ctx is usable
    # four aligned pixels that share a label out of range (the 16-byte load of a shared label must not be taken for them)
    labels = np.zeros(16, dtype=np.uint8)
    labels[4:8] = 2
    with pytest.raises(nle.NLEError) as e:
        ctx.segment_stats(torch.ones((2, 16), dtype=torch.float32, device=dev), labels)
    assert e.value.code == nle.NLE_ERR_INVALID and "4 labels" in str(e.value)


def _init_plane(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "levels":
        return rng.integers(0, 256, size=n).astype(np.float32)
    if kind == "flat":
        return np.full(n, 77.0, dtype=np.float32)
    x = (rng.normal(size=n) * 200 + 128).astype(np.float32)  # fractional, with values either side of [-256, 768)
    x[0], x[1], x[2] = -300.0, 900.0, np.nan
    x[3:5] = (-256.0, 767.99)[:max(0, min(2, n - 3))]
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 1023, 72 * 96])
@pytest.mark.parametrize("Cn", [2, 3, 8])
@pytest.mark.parametrize("kind", ["levels", "fractional", "flat"])
def test_segment_init_is_the_restatement_exactly(nle, ctx, kind, Cn, n):
    import torch
    dev = f"cuda:{ctx.device}"
    x = _init_plane(kind, n, 31 * Cn + n)
    want, cuts = start_labels(x, Cn)
    if kind == "flat":
        assert len(np.unique(want)) == 1
    if kind == "fractional":
        assert np.isnan(x).any() and (x < -256).any() and (x >= 768).any()
    assert np.array_equal(ctx.plane_histogram(x), histogram(x))  # the restated histogram is the library's
    for off in (0, 1):  # 16-byte loads, and one pixel at a time
        buf = torch.zeros(n + off + 4, dtype=torch.float32, device=dev)
        buf[off:off + n] = torch.as_tensor(x, device=dev)
        labels, got_cuts = ctx.segment_init(buf[off:off + n], Cn)
        assert np.array_equal(got_cuts, cuts), (off, got_cuts, cuts)
        assert np.array_equal(labels.cpu().numpy(), want), off


# ---- the loop
MODES = ["auto_tables", "streamed_f64"]


def _train(nle, sctx, x, params, mode):
    sctx.set_mode(nle.MODE_STREAMED_F64 if mode == "streamed_f64" else nle.MODE_AUTO)
    nr, nc, hx, hy, T, K = params
    f = nle.NLEFilter(sctx).train_filter(np.asarray(x, dtype=np.float32), nr, nc, hx, hy, T, K)
    assert f.diag()["formulation"] == (nle.MODE_STREAMED_F64 if mode == "streamed_f64" else nle.MODE_PHI_FREE)
    return f


def _composed_step(nle, ctx, f, labels, Cn, H, W):
    """one iteration made with the mirror's public calls; labels: a device tensor, left alone.  -> (new labels, q, counts,
    means)"""
    import torch
    n = H * W
    ind = (labels[None, :] == torch.arange(Cn, device=labels.device, dtype=torch.uint8)[:, None]).to(torch.float32)
    counts = np.bincount(labels.cpu().numpy(), minlength=Cn)
    scale = np.array([n / c if c else 0.0 for c in counts])
    q = f.region_spread(ind.view(Cn, H, W), scale, SPREAD)
    got_counts, sums = ctx.segment_stats(q, labels)
    assert np.array_equal(got_counts, counts)
    m = means(counts, sums)
    new = labels.clone()
    ctx.segment_assign(q, m, new)
    return new, q, counts, m


@pytest.mark.gpu
@pytest.mark.parametrize("Cn", [2, 3, 8])
@pytest.mark.parametrize("mode", MODES)
def test_one_iteration_is_its_composition_and_agrees_with_the_oracle(nle, oracle, sctx, mode, Cn):
    H, W = SYNTH[:2]
    n = H * W
    x, V, S = _synth(oracle)
    f = _train(nle, sctx, x, SYNTH[2:8], mode)
    labels, _ = sctx.segment_init(np.asarray(x, dtype=np.float32), Cn)
    assert np.array_equal(labels.cpu().numpy(), start_labels(x, Cn)[0])
    for step in range(3):
        before = labels.clone()
        composed, q, counts, m = _composed_step(nle, sctx, f, before, Cn, H, W)
        r = f.segment(Cn, SPREAD, 1, labels=labels)
        assert r["iterations"] == 1 and r["labels"].data_ptr() == labels.data_ptr()
        assert np.array_equal(labels.cpu().numpy(), composed.cpu().numpy()), step  # bit for bit the composition
        assert np.array_equal(r["counts"], np.bincount(composed.cpu().numpy(), minlength=Cn))
        assert r["objective"][0] == objective(counts, m)
        # against the oracle, from the device's own labels
        lab_h, q_h = before.cpu().numpy(), q.cpu().numpy()
        q_o = oracle_spread(oracle, V, S, lab_h, Cn, SPREAD)
        errs = [rel_l2(q_h[c], q_o[c]) for c in range(Cn) if counts[c]]
        assert max(errs) <= PER_LAYER_TOL, errs
        m_o = means(*stats(q_o, lab_h, Cn))
        active = counts > 0
        delta = 2 * (np.abs(m[active] - m_o[active]).max() + 2 * np.abs(q_h.astype(np.float64) - q_o).max())
        with np.errstate(invalid="ignore"):
            s = np.sort(np.where(active[:, None], m_o[:, None] - 2.0 * q_o.astype(np.float64), INF), axis=0)
        margin = s[1] - s[0] if Cn > 1 else np.full(n, INF)
        sure = margin > delta
        want = assign(q_o, m_o, lab_h)[0]
        got = labels.cpu().numpy()
        print(f"{mode} C = {Cn} step {step}: spreads {max(errs):.2e}, delta {delta:.2e}, {100 * (1 - sure.mean()):.3f} % of the "
              f"pixels under it, {int((got != want).sum())} labels differ from the oracle's")
        assert np.array_equal(got[sure], want[sure])
        assert (~sure).mean() <= 0.02
    f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("Cn", [2, 4])
@pytest.mark.parametrize("mode", MODES)
def test_the_loop_to_convergence(nle, oracle, sctx, mode, Cn):
    H, W = SYNTH[:2]
    n = H * W
    x, _, _ = _synth(oracle)
    f = _train(nle, sctx, x, SYNTH[2:8], mode)
    r = f.segment(Cn, SPREAD, 40, want_spreads=True)
    J = r["objective"]
    print(f"{mode} C = {Cn}: {r['iterations']} iterations, converged {r['converged']}, J {J[0]:.6f} -> {J[-1]:.6f}")
    assert len(J) == r["iterations"] <= 40
    assert all(J[k + 1] >= J[k] - 1e-6 * abs(J[k]) for k in range(len(J) - 1))
    assert r["counts"].sum() == n
    final = r["labels"].cpu().numpy()
    assert np.array_equal(r["counts"], np.bincount(final, minlength=Cn))
    if r["converged"]:  # one more step changes nothing, and the spreads handed out are that step's
        again = f.segment(Cn, SPREAD, 1, labels=r["labels"].clone(), want_spreads=True)
        assert again["converged"] and np.array_equal(again["labels"].cpu().numpy(), final)
        assert np.array_equal(again["spreads"].cpu().numpy().view(np.uint32), r["spreads"].cpu().numpy().view(np.uint32))
    # the spreads are those of the returned labels
    _, q, _, _ = _composed_step(nle, sctx, f, r["labels"], Cn, H, W)
    assert np.array_equal(q.cpu().numpy().view(np.uint32), r["spreads"].cpu().numpy().view(np.uint32))
    # a second run is the first, bit for bit
    r2 = f.segment(Cn, SPREAD, 40, want_spreads=True)
    assert np.array_equal(r2["labels"].cpu().numpy(), final) and r2["iterations"] == r["iterations"]
    assert np.array_equal(r2["objective"].view(np.uint64), J.view(np.uint64))
    assert np.array_equal(r2["spreads"].cpu().numpy().view(np.uint32), r["spreads"].cpu().numpy().view(np.uint32))
    # and 40 chained calls of one iteration each
    labels, _ = sctx.segment_init(np.asarray(x, dtype=np.float32), Cn)
    hist = []
    for _ in range(40):
        one = f.segment(Cn, SPREAD, 1, labels=labels)
        hist.append(one["objective"][0])
        if one["converged"]:
            break
    assert np.array_equal(labels.cpu().numpy(), final)
    assert np.array_equal(np.array(hist).view(np.uint64), J.view(np.uint64))
    f.close()


@pytest.mark.gpu
def test_three_blocks_end_at_the_truth_and_feed_the_region_combine(nle, sctx):
    x, truth = _blocks()
    H, W = BLOCKS[:2]
    f = _train(nle, sctx, x, BLOCKS[2:], "auto_tables")
    r = f.segment(3, SPREAD, 40, want_spreads=True)
    assert r["converged"] and np.array_equal(r["labels"].cpu().numpy(), truth)
    assert np.array_equal(r["counts"], np.bincount(truth, minlength=3))
    layers = f.apply_layers(x.astype(np.float32), 4)
    y = sctx.region_combine(layers, r["spreads"], tre.WT, tre.FLOOR, tre.F32).cpu().numpy()
    want = tre.stored(tre.combine(layers.cpu().numpy(), r["spreads"].cpu().numpy(), tre.WT, tre.FLOOR), tre.F32)
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32))  # the bound of tests/test_region_edits.py: the bits
    f.close()


@pytest.mark.gpu
def test_filter_segment_refusals_leave_the_ctx_usable(nle, oracle, sctx):
    import torch
    H, W, nr, nc, hx, hy, T, K, _ = SYNTH
    n = H * W
    x, V, S = _synth(oracle)
    f = _train(nle, sctx, x, (nr, nc, hx, hy, T, K), "auto_tables")
    fS = oracle.transform_eigenvalues(S, [2.0, 3.0, 4.0, 1.0])
    want = oracle.apply_filter(V, x, fS).ravel()

    def still_fine(flt=f):
        assert rel_l2(flt.apply(x, oracle.transform_eigenvalues(flt.eigvals, [2.0, 3.0, 4.0, 1.0])).cpu().numpy(), want) <= PER_LAYER_TOL

    def refused(fn, word=None):
        with pytest.raises(nle.NLEError) as e:
            fn()
        assert e.value.code == nle.NLE_ERR_INVALID and str(e.value)
        assert word is None or word in str(e.value)
        still_fine()

    zeros = lambda: torch.zeros(n, dtype=torch.uint8, device="cuda")  # noqa: E731
    refused(lambda: f.segment(0, labels=zeros()), "segments")
    refused(lambda: f.segment(nle.REGION_MAX + 1, labels=zeros()), "segments")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused(lambda: f.segment(2, spread=bad, labels=zeros()), "spread")
    for bad in (0, -1, nle.SEGMENT_ITERATIONS_MAX + 1):
        refused(lambda: f.segment(2, max_iter=bad, labels=zeros()), "iterations")
    refused(lambda: f.segment(2, labels=np.full(n, 2, dtype=np.uint8)), "label")  # a start label that is no cluster
    lab = zeros()
    counts, obj = np.zeros(8, dtype=np.int64), np.zeros(4)
    iters, conv = C.c_int(0), C.c_int(0)
    args = dict(labels=C.c_void_p(lab.data_ptr()), counts=counts.ctypes.data_as(C.c_void_p), obj=obj.ctypes.data_as(C.c_void_p),
                iters=C.byref(iters), conv=C.byref(conv))

    def raw(Hh=H, Ww=W, **null):
        a = dict(args, **{k: None for k in null})
        return nle.lib().nle_filter_segment(f._f, Hh, Ww, 2, SPREAD, 4, a["labels"], None, 0, a["counts"], a["obj"], a["iters"],
                                            a["conv"])
    for which in ("labels", "counts", "obj", "iters", "conv"):
        assert raw(**{which: True}) == nle.NLE_ERR_INVALID and nle.lib().nle_last_error(sctx._h)
        still_fine()
    assert raw(Hh=H - 1) == nle.NLE_ERR_INVALID and raw(Hh=0, Ww=n) == nle.NLE_ERR_INVALID  # H W is not the filter's
    still_fine()
    assert raw() == nle.NLE_OK and iters.value >= 1  # d_q may be NULL
    assert nle.lib().nle_segment_init(sctx._h, None, 8, 2, None, None) == nle.NLE_ERR_INVALID
    assert nle.lib().nle_segment_stats(sctx._h, None, 2, 8, 8, None, None, None) == nle.NLE_ERR_INVALID
    assert nle.lib().nle_segment_assign(sctx._h, None, 2, 8, 8, None, None, None, 0, None, None) == nle.NLE_ERR_INVALID
    q = torch.zeros((2, 8), dtype=torch.float32, device="cuda")
    refused(lambda: sctx.segment_init(q[0], 0), "segments")
    refused(lambda: sctx.segment_init(q[0], 9), "segments")
    refused(lambda: sctx.segment_stats(torch.as_strided(q, (2, 8), (4, 1)), np.zeros(8, dtype=np.uint8)), "stride")
    refused(lambda: sctx.segment_assign(q, np.zeros(2), np.zeros(8, dtype=np.uint8), indicators=q), "overlap")
    # the mirror hands pointers to kernels: a wrong length, type or device never reaches the library
    short, host = torch.zeros(n - 1, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8)
    for bad in (short, host, torch.zeros(n, dtype=torch.int32, device="cuda"), np.zeros(n + 1, dtype=np.uint8)):
        refused(lambda: f.segment(2, labels=bad), "labels must be")
    for bad in (torch.zeros(7, dtype=torch.uint8, device="cuda"), torch.zeros(8, dtype=torch.uint8)):
        refused(lambda: sctx.segment_stats(q, bad), "labels must be")
        refused(lambda: sctx.segment_assign(q, np.zeros(2), bad), "labels must be")
    for bad in (q.cpu(), q.double(), q[0]):
        refused(lambda: sctx.segment_stats(bad, np.zeros(8, dtype=np.uint8)), "planes")
        refused(lambda: sctx.segment_assign(bad, np.zeros(2), np.zeros(8, dtype=np.uint8)), "planes")
    refused(lambda: sctx.segment_assign(q, np.zeros(2), np.zeros(8, dtype=np.uint8), indicators=torch.zeros((2, 8))), "planes")
    refused(lambda: sctx.segment_assign(q, np.zeros(3), np.zeros(8, dtype=np.uint8)), "means")
    refused(lambda: sctx.segment_init(torch.zeros(8), 2), "cuda")
    f.close()
    # world > 1: refused before any collective -- a shard of two whose all-reduce must never be called
    calls = []
    s = nle.Context(0)
    try:
        g = nle.NLEFilter(s).train_filter(np.asarray(x, dtype=np.float32), nr, nc, hx, hy, T, K)
        s.set_shard(0, 2, 48, lambda t: calls.append(1))
        with pytest.raises(nle.NLEError) as e:
            g.segment(2, labels=zeros())
        assert e.value.code == nle.NLE_ERR_INVALID and "world" in str(e.value) and not calls
        assert nle.lib().nle_ctx_set_shard(s._h, 0, 1, nle.ALLREDUCE_FN(0), None, None, 0) == 0
        still_fine(g)
        assert not calls
        g.close()
    finally:
        s.close()
