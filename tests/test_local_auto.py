"""Per-region auto levels and equalise: membership-weighted histograms (include/nle.h at
nle_region_histograms states the rule).  There is no reference for it, so the rule is restated here in numpy on top of the
restatements it is made of (tests/test_local_adjust.py's memberships, tests/test_tone_curve.py's bins and curve).

Bounds.  The counts are integers and every operation that leads to them is one IEEE fp64 operation (the memberships of the
local rule, one product by a power of two, one sum, one truncation; the bin of nle_plane_histogram): the device equals the
restatement exactly, in every counter, whatever the order of the pixels and of the merges.  The composite is compared bit
for bit with the stage calls it is defined as."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_detail_curve import F32, KINDS, ROUNDED8
from test_local_adjust import FLOOR, member_planes, memberships
from test_tone_curve import BINS, np_curve, np_hist

ONE = 65536
NS = [1, 3, 63, 64, 65, 4099, 32768 + 5]      # 4099: past one trip of a workgroup's loop (1024 lanes x 4); the last: two workgroups
MS = [1, 2, 4, 8]


# ------------------------------------------------------------------------------------------------ the restatement
def np_bins(y, scale):
    """the counter 0 .. BINS + 1 of every fp32 value of y times scale (np_hist's rule, value by value)"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(y, dtype=np.float32).astype(np.float64).ravel() * np.float64(scale)
        t = (v + 256.0) * 4.0
        b = np.full(t.shape, BINS + 1, dtype=np.int64)                 # NaN, and t >= BINS
        b[t < 0] = 0
        mid = (t >= 0) & (t < BINS)
        b[mid] = 1 + np.floor(t[mid]).astype(np.int64)
    return b


def np_weights(Q, floor):
    """omega_0 .. omega_M, (M + 1, n) int64"""
    alpha = memberships(Q, floor)
    with np.errstate(invalid="ignore"):
        return np.where(alpha > 0, np.floor(alpha * 65536.0 + 0.5), 0.0).astype(np.int64)      # alpha >= 0: truncation is the floor


def np_region_hist(y, Q, scale, floor=FLOOR, row_on=None):
    """(M + 1, BINS + 2) int64; the sums stay below 2^53, so the float64 weights of bincount add exactly"""
    omega = np_weights(Q, floor)
    out = np.zeros((omega.shape[0], BINS + 2), dtype=np.int64)
    for m in range(omega.shape[0]):
        if row_on is None or row_on[m]:
            got = np.bincount(np_bins(y, scale[m]), weights=omega[m].astype(np.float64), minlength=BINS + 2)
            assert got.max() < 2.0 ** 53
            out[m] = got.astype(np.int64)
    return out


def base_values(n, seed):
    """a base layer with everything the bin rule tells apart: NaN, +-inf, values exactly on bin edges, values that fall into
    the underflow and overflow counters under the scales of `row_scales`, and U(0, 255) for the rest"""
    rng = np.random.default_rng(seed)
    y = rng.uniform(0.0, 255.0, n).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 0.25, 17.75, 255.0, -256.0, 767.75, 768.0, -256.25, 1e30, -1e30, 400.0, -200.0],
                       dtype=np.float32)
    if n >= 4 * special.size:
        at = rng.choice(n, special.size, replace=False)
        y[at] = special
        edges = rng.choice(n, n // 8, replace=False)
        y[edges] = np.float32(0.25) * rng.integers(-1100, 3200, edges.size).astype(np.float32)      # edges, and beyond both ends
    elif n >= 3:
        y[:3] = special[[0, 1, 5]]
    return y


def row_scales(M):
    """one scale per row: 1, a negative one, one that pushes the plane into the overflow counter, small ones"""
    return np.array([1.0, -0.5, 3.5, 0.9, 1.0, -2.0, 0.01, 1.25, 2.0][:M + 1])


def test_header_constants_and_entry_points_are_mirrored(nle):
    text = open(os.path.join(ROOT, "include", "nle.h")).read()
    assert int(re.search(r"^#define\s+NLE_REGION_WEIGHT_ONE\s+(\d+)\s*$", text, flags=re.M).group(1)) == nle.REGION_WEIGHT_ONE == ONE
    for name in ("nle_region_histograms", "nle_apply_local_auto"):
        assert name in nle.EXPORTED_SYMBOLS and hasattr(nle.lib(), name) and re.search(r"\b%s\s*\(" % name, text)
    assert callable(nle.Context.region_histograms) and callable(nle.NLEFilter.apply_local_auto)
    assert nle.KERNEL_COUNT == 12 and nle.KERNEL_COUNT_ALL == 16        # no new kernel ids


# ------------------------------------------------------------------------------------------------ CPU: the consequences
def hard_planes(n, M, seed, phi=FLOOR):
    """owner 0 .. M per pixel (0: the background); the owner's q >= phi, every other q <= 0 or NaN"""
    rng = np.random.default_rng(seed)
    owner = rng.integers(0, M + 1, n)
    q = -rng.uniform(0.0, 2.0, (M, n)).astype(np.float32)
    q[rng.random((M, n)) < 0.1] = np.nan
    q[rng.random((M, n)) < 0.1] = 0.0
    for m in range(1, M + 1):
        mine = owner == m
        q[m - 1, mine] = np.maximum(rng.uniform(0.0, 3.0, int(mine.sum())), phi).astype(np.float32)
    q[0, owner == 1] = np.where(rng.random(int((owner == 1).sum())) < 0.3, np.float32(phi), q[0, owner == 1])   # q == phi exactly
    return q, owner


@pytest.mark.parametrize("M", MS)
def test_restated_consequences_a_and_b(M):
    n = 20000
    y = base_values(n, 3 + M)
    sc = row_scales(M)
    Qa = -np.abs(member_planes(n, M, 5))                                   # (a): every q <= 0 or NaN
    h = np_region_hist(y, Qa, sc)
    assert np.array_equal(h[0], ONE * np_hist(y, sc[0])) and not h[1:].any()
    Q, owner = hard_planes(n, M, 17 + M, np.float32(FLOOR))                # (b): hard memberships
    h = np_region_hist(y, Q, sc)
    for m in range(M + 1):
        assert np.array_equal(h[m], ONE * np_hist(y[owner == m], sc[m])), m


def test_restated_consequence_c_the_mass_of_a_pixel():
    """|sum_m omega_m - 65536| <= (M + 1) / 2 + 1: every omega_m is within 1/2 of alpha_m 65536, and the alpha_m sum to 1 up to
    a few roundings (one unit of 2^-53 x 65536 is far below the 1 that is allowed for it)"""
    rng = np.random.default_rng(1)
    worst = {}
    for M in MS:
        for floor in (0.05, 0.5, 3.0):
            Q = rng.uniform(-0.3, 1.5, (M, 200000)).astype(np.float32)
            Q[:, ::7] *= np.float32(0.01)
            total = np_weights(Q, floor).sum(axis=0)
            worst[M] = max(worst.get(M, 0), int(np.abs(total - ONE).max()))
            assert np.all(np.abs(total - ONE) <= (M + 1) / 2 + 1), (M, floor)
    print("largest |sum omega - 65536| per M:", worst)


def tie_planes(n):
    """(d): M = 1, phi = 0.5, q = (2 k + 1) / 262144: alpha 65536 = k + 0.5 exactly"""
    k = np.arange(n, dtype=np.int64)
    q = ((2 * k + 1).astype(np.float64) / 262144.0).astype(np.float32)
    assert np.array_equal(q.astype(np.float64) * 262144.0, (2 * k + 1).astype(np.float64)) and q.max() < 0.5
    return q[None, :], k


def test_restated_consequence_d_a_tie_rounds_up():
    Q, k = tie_planes(40000)
    al = memberships(Q, 0.5)
    assert np.array_equal(al[1] * 65536.0, k + 0.5)
    assert np.array_equal(np_weights(Q, 0.5)[1], k + 1)


def test_tone_curve_is_invariant_under_the_common_factor(nle):
    """nle_tone_curve on a row scaled by 65536 is bit for bit the curve of the unscaled counts, and both are the restatement's"""
    rng = np.random.default_rng(9)
    cases = [np_hist(base_values(50000, 2), 1.0), np_hist(rng.normal(90, 30, 3000), 1.0), np_hist(np.full(10, 77.0), 1.0)]
    for counts in cases:
        for s, h, P, A in ((0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.3, -0.2, -1.0, 1.0), (0.5, 0.0, 5.0, 0.4), (0.0, 0.0, 25.0, 1.0)):
            a = nle.tone_curve(counts, s, h, P, A)
            b = nle.tone_curve(ONE * counts, s, h, P, A)
            assert np.array_equal(a.view(np.int64), b.view(np.int64)), (s, h, P, A)
            assert np.array_equal(b, np_curve(ONE * counts, s, h, P, A))


# ------------------------------------------------------------------------------------------------ GPU: the stage call
WHERE = [dict(), dict(oy=1), dict(oq=1), dict(oy=3, oq=2), dict(oy=1, oq=1), dict(qextra=1), dict(qextra=2), dict(qextra=4, oy=2)]


def dev_planes(ctx, y, Q, oy=0, oq=0, qextra=0):
    """y and Q on the device: base pointers oy, oq elements past a 16-byte boundary, the planes n + qextra floats apart"""
    import torch
    d = f"cuda:{ctx.device}"
    n = y.size

    def put(v, off, extra):
        v = np.atleast_2d(v)
        s = n + extra
        buf = torch.zeros(v.shape[0] * s + 8, device=d)[off:off + v.shape[0] * s]
        t = buf.as_strided((v.shape[0], n), (s, 1))
        t.copy_(torch.from_numpy(np.array(v)))
        assert t.data_ptr() % 16 == 4 * off
        return t
    return put(y, oy, 0)[0], put(Q, oq, qextra)


def row_on_cases(M):
    yield None
    yield [m == M // 2 + 1 for m in range(M + 1)]          # a single row
    yield [m % 2 == 0 for m in range(M + 1)]               # every second row
    yield [m % 2 == 1 for m in range(M + 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("n", NS)
def test_region_histograms_are_the_restatement(ctx, n, M):
    """every size and region count; rows on and off; base pointers off their 16-byte boundary and strides that are no
    multiple of 4; NaN, +-inf, bin edges, underflow and overflow in y; a negative scale and a scale per row; NaN, negative
    and infinite q, sums below the floor, rows without influence"""
    y = base_values(n, 100 * M + n)
    Q = member_planes(n, M, 7000 * M + n)
    if n > 100:
        Q[M - 1, 70] = np.inf                                # alpha is NaN in every row of this pixel: it counts nowhere
        assert np.all(np_weights(Q, FLOOR)[:, 70] == 0)
    sc = row_scales(M)
    if n > 4000:
        al = memberships(Q, FLOOR)
        assert np.any((al[0] > 0) & (al[0] < 1)) and all(np.any(al[m] == 0) and np.any(al[m] > 0) for m in range(M + 1))
        full = np_region_hist(y, Q, sc)
        assert full[0, 0] > 0 and full[0, BINS + 1] > 0 and full[1, 0] > 0                              # under- and overflow
    for row_on in row_on_cases(M):
        want = np_region_hist(y, Q, sc, FLOOR, row_on)
        for where in WHERE:
            ty, tQ = dev_planes(ctx, y, Q, **where)
            got = ctx.region_histograms(ty, tQ, sc, row_on, FLOOR)
            assert got.dtype == np.int64 and got.shape == want.shape
            assert np.array_equal(got, want), (n, M, row_on, where, np.argwhere(got != want)[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 4, 8])
def test_consequences_a_and_b_against_plane_histogram(nle, ctx, M):
    import torch
    n = 30001
    y = base_values(n, 40 + M)
    sc = row_scales(M)
    ty, tQ = dev_planes(ctx, y, -np.abs(member_planes(n, M, 5)))
    got = ctx.region_histograms(ty, tQ, sc)
    assert np.array_equal(got[0], ONE * ctx.plane_histogram(ty, sc[0])) and not got[1:].any()           # (a)
    Q, owner = hard_planes(n, M, 23 + M, np.float32(FLOOR))
    ty, tQ = dev_planes(ctx, y, Q, oy=1, qextra=3)
    got = ctx.region_histograms(ty, tQ, sc)
    for m in range(M + 1):                                                                             # (b)
        mine = torch.as_tensor(y[owner == m], device=ty.device)
        alone = ctx.plane_histogram(mine, sc[m])
        assert np.array_equal(got[m], ONE * alone), m
        for s, h, P, A in ((0.0, 0.0, 1.0, 0.0), (0.4, -0.3, 2.0, 0.6)):
            assert np.array_equal(nle.tone_curve(got[m], s, h, P, A).view(np.int64), nle.tone_curve(alone, s, h, P, A).view(np.int64))


@pytest.mark.gpu
def test_soft_memberships_everywhere_and_sums_below_the_floor(ctx):
    rng = np.random.default_rng(77)
    n, M = 20011, 8
    y = base_values(n, 1)
    Q = rng.uniform(0.0, 1.0, (M, n)).astype(np.float32)          # every region has a share of every pixel
    Q[:, n // 2:] *= np.float32(0.002)                            # sigma < phi: the background keeps most
    sc = row_scales(M)
    assert np.all(memberships(Q, FLOOR)[0, n // 2:] > 0.5)
    for floor in (FLOOR, 0.5, 3.0):
        ty, tQ = dev_planes(ctx, y, Q)
        assert np.array_equal(ctx.region_histograms(ty, tQ, sc, None, floor), np_region_hist(y, Q, sc, floor))


@pytest.mark.gpu
def test_consequence_d_a_tie_rounds_up(ctx):
    n = 40000
    Q, k = tie_planes(n)
    y = np.full(n, 100.0, dtype=np.float32)
    ty, tQ = dev_planes(ctx, y, Q)
    got = ctx.region_histograms(ty, tQ, [1.0, 1.0], None, 0.5)
    b = int(np_bins(y[:1], 1.0)[0])
    assert got[1, b] == int((k + 1).sum()) and got[1].sum() == got[1, b]
    assert np.array_equal(got, np_region_hist(y, Q, [1.0, 1.0], 0.5))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [32768, 65536, 3 * 65536 + 1, (1 << 22) + 3])
def test_a_flat_plane_puts_all_its_weight_into_one_counter(ctx, n):
    """the worst case for atomics on one address, and the width of the workgroup's 32-bit counters: 65536 pixels of full
    weight in one bin are 2^32.  The launcher's grid rule gives a workgroup 32768 pixels and no more, whatever n is, so no n
    makes a workgroup see 65536; the sizes here are one workgroup's full share (2^31 in one counter), the n at which a
    single workgroup would wrap, and sizes over many workgroups.  M = 1, q = 0: row 0 holds exactly 65536 n."""
    import torch
    d = f"cuda:{ctx.device}"
    ty, tQ = torch.full((n,), 100.0, device=d), torch.zeros((1, n), device=d)
    got = ctx.region_histograms(ty, tQ, [1.0, 1.0])
    b = 1 + (100 + 256) * 4
    assert got[0, b] == ONE * n and got.sum() == ONE * n
    tQ.fill_(1.0)                                            # and all of it in row 1
    got = ctx.region_histograms(ty, tQ, [1.0, 2.0])
    assert got[1, 1 + (200 + 256) * 4] == ONE * n and got.sum() == ONE * n


def raw_hist(nle, ctx, y, Q, M, n, qs, scale, row_on, floor, counts=True):
    ctx._sync_in()
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    A = lambda v, dt=np.float64: np.ascontiguousarray(v, dtype=dt).ctypes.data_as(C.c_void_p) if v is not None else None  # noqa: E731
    out = np.full((M + 1 if 1 <= M <= 8 else 9, BINS + 2), -1, dtype=np.int64)
    st = nle.lib().nle_region_histograms(ctx._h, P(y), P(Q), M, n, qs, A(scale), A(row_on, np.int32), floor,
                                         out.ctypes.data_as(C.c_void_p) if counts else None)
    return st, out


@pytest.mark.gpu
def test_refusals_have_their_messages_and_leave_the_ctx_usable(nle, ctx):
    n, M = 1000, 2
    y, Q, sc = base_values(n, 8), member_planes(n, M, 9), row_scales(2)
    ty, tQ = dev_planes(ctx, y, Q)
    want = np_region_hist(y, Q, sc)
    nan, inf = float("nan"), float("inf")
    good = dict(y=ty, Q=tQ, M=M, n=n, qs=n, scale=sc, row_on=None, floor=FLOOR, counts=True)

    def call(**kw):
        args = dict(good)
        args.update(kw)
        return raw_hist(nle, ctx, **args)
    F = "nle_region_histograms"
    null, stride, floor_ = F + ": NULL pointer", F + ": the plane stride is smaller than n", F + ": the region floor must be finite and > 0, got "
    bad = [(dict(y=None), null), (dict(Q=None), null), (dict(scale=None), null), (dict(counts=False), null),
           (dict(M=0), F + " takes 1 to 8 regions, got 0"), (dict(M=9, scale=np.ones(10)), F + " takes 1 to 8 regions, got 9"),
           (dict(n=0), F + ": n must be >= 1"), (dict(n=-5), F + ": n must be >= 1"),
           (dict(qs=n - 1), stride), (dict(qs=-1), stride), (dict(M=1, scale=[1.0, 1.0], qs=n - 1), stride),      # one plane: refused all the same
           (dict(scale=[1.0, nan, 1.0]), F + ": the scale of row 1 is not finite"),
           (dict(scale=[inf, 1.0, 1.0]), F + ": the scale of row 0 is not finite"),
           (dict(floor=0.0), floor_ + "0.000000"), (dict(floor=-1.0), floor_ + "-1.000000"), (dict(floor=inf), floor_ + "inf"),
           (dict(floor=nan), None)]
    for k, (kw, text) in enumerate(bad):
        st, _ = call(**kw)
        assert st == nle.NLE_ERR_INVALID, k
        msg = nle.lib().nle_last_error(ctx._h).decode()
        if text is None:                                      # the sign a C library prints a NaN with is its own
            assert msg in (floor_ + "nan", floor_ + "-nan"), (k, msg)
        else:
            assert msg == text, (k, msg)
    import torch
    for kw in (dict(y=ty.double()), dict(q=tQ.cpu()), dict(y=ty.cpu()), dict(q=tQ.to(torch.float16))):      # the mirror hands no such pointer on
        args = dict(y=ty, q=tQ)
        args.update(kw)
        with pytest.raises(nle.NLEError, match="region_histograms: float32 tensors on this ctx's device expected"):
            ctx.region_histograms(args["y"], args["q"], sc)
    st, got = call()
    assert st == nle.NLE_OK and np.array_equal(got, want)
    st, got = call(row_on=[0, 0, 0])                          # no row is on: zeros, and nothing to launch
    assert st == nle.NLE_OK and not got.any()
    assert np.array_equal(ctx.plane_histogram(ty, 1.0), np_hist(y, 1.0))


# ------------------------------------------------------------------------------------------------ GPU: the composite
H_, W_, L_, M_ = 24, 32, 3, 2
TRAIN = dict(nr=4, nc=4, hx=30.0, hy=30.0, T=10, K=8)
W3 = np.array([[3.0, 1.5, 0.9], [2.0, 2.0, 1.1], [1.0, 1.0, 1.0]])
DETAIL = np.array([[1.0, 2.5, 6.0], [0.0, 1.0, 0.0], [0.5, 0.5, 4.0]])
NONE_ = (0.0, 0.0, -1.0, 0.0)


def small_scene():
    """24 x 32: a dark block (levels 20 .. 60) beside a bright one (150 .. 250), integers"""
    rng = np.random.default_rng(4)
    x = np.where(np.arange(W_)[None, :] < W_ // 2, rng.integers(20, 61, (H_, W_)), rng.integers(150, 251, (H_, W_)))
    return x.astype(np.float32)


def small_strokes():
    s = np.zeros((M_, H_, W_), dtype=np.float32)
    s[0, 6:18, 3:12] = 1.0
    s[1, 6:18, 20:29] = 1.0
    return s, [s[m].size / float(s[m].sum()) for m in range(M_)]


@pytest.fixture(scope="module")
def small(nle, ctx):
    import torch
    x = small_scene()
    f = nle.NLEFilter(ctx).train_filter(x, TRAIN["nr"], TRAIN["nc"], TRAIN["hx"], TRAIN["hy"], TRAIN["T"], TRAIN["K"])
    tx = torch.as_tensor(x, device=f"cuda:{ctx.device}")
    s, scale = small_strokes()
    Y = f.apply_layers(tx, L_)
    q = f.region_spread(s, scale, 4.0)
    yield dict(x=x, tx=tx, f=f, s=s, scale=scale, Y=Y, q=q)
    f.close()


def staged(nle, ctx, sc, tone, kind, q=None):
    """the five calls of the header, given the first two; returns (out, curves (M + 1, knots + 2), counts or None)"""
    q = sc["q"] if q is None else q
    hist_on = [t[2] >= 0 or t[3] > 0 for t in tone]
    counts = ctx.region_histograms(sc["Y"][L_ - 1], q, W3[:, L_ - 1], hist_on, FLOOR) if any(hist_on) else None
    curves = []
    for m, (s, h, P, A) in enumerate(tone):
        if (s, h, P, A) == NONE_ or (s == 0 and h == 0 and P < 0 and A == 0):
            curves.append(None)
        elif hist_on[m] and counts[m].sum() >= ONE:
            curves.append(nle.tone_curve(counts[m], s, h, P, A))
        else:
            curves.append(nle.tone_curve(None, s, h))
    out = ctx.local_combine(sc["tx"].reshape(-1), sc["Y"], q, W3, DETAIL, curves, FLOOR, kind)
    cv = np.stack([np.zeros(nle.TONE_KNOTS + 2) if c is None else c for c in curves])
    return out, cv, counts


TONES = [[(0.0, 0.0, 1.0, 0.0), NONE_, NONE_],
         [NONE_, (0.3, -0.2, 0.0, 0.5), (0.0, 0.0, -1.0, 1.0)],
         [(0.5, 0.0, 2.0, 0.4), (0.0, 0.4, -1.0, 0.0), (0.0, 0.0, 25.0, 0.0)]]


@pytest.mark.gpu
def test_apply_local_auto_is_the_five_stage_calls(nle, ctx, small):
    import torch
    sc = small
    f = sc["f"]
    seen = set()
    for tone in TONES:
        for kind in KINDS:
            one, q1, cv1 = f.apply_local_auto(sc["tx"], L_, sc["s"], W3, tone, DETAIL, sc["scale"], 4.0, FLOOR, kind, want_spreads=True,
                                              want_curves=True)
            two, cv2, _ = staged(nle, ctx, sc, tone, kind)
            assert one.dtype == two.dtype and torch.equal(one, two), (tone, kind)
            assert torch.equal(q1, sc["q"])
            assert np.array_equal(cv1.view(np.int64), cv2.view(np.int64))
            assert torch.equal(f.apply_local_auto(sc["tx"], L_, sc["s"], W3, tone, DETAIL, sc["scale"], 4.0, FLOOR, kind), one)
            seen.add(one.cpu().numpy().tobytes())
    assert len(seen) == len(TONES) * 3
    # the levels come from the row's own histogram: at 25 % the whole plane's levels would begin in the dark block (below 60),
    # row 2's begin in the bright block its stroke lies in
    assert cv2[2, 0] > 100 and cv2[2, 1] < 255


@pytest.mark.gpu
def test_without_levels_and_equalise_it_is_apply_local(nle, ctx, small):
    import torch
    sc = small
    f = sc["f"]
    for tone in ([NONE_, NONE_, NONE_], [(0.8, 0.0, -1.0, 0.0), NONE_, (0.0, -0.6, -1.0, 0.0)]):
        curves = [None if t == NONE_ else nle.tone_curve(None, t[0], t[1]) for t in tone]
        for kind in KINDS:
            one, cv = f.apply_local_auto(sc["tx"], L_, sc["s"], W3, tone, DETAIL, sc["scale"], 4.0, FLOOR, kind, want_curves=True)
            two = f.apply_local(sc["tx"], L_, sc["s"], W3, DETAIL, curves, sc["scale"], 4.0, FLOOR, kind)
            assert torch.equal(one, two), (tone, kind)
            for m in range(M_ + 1):
                assert np.array_equal(cv[m], np.zeros_like(cv[m]) if curves[m] is None else curves[m])


@pytest.mark.gpu
def test_a_row_without_mass_takes_the_fallback_curve(nle, ctx, small):
    """a stroke with the scale 0 spreads to q = 0 everywhere and has no membership anywhere: its row sums to 0, less than one
    pixel's mass, and its curve is the one of its two slopes alone"""
    import torch
    sc = small
    f = sc["f"]
    scale = [sc["scale"][0], 0.0]
    q = f.region_spread(sc["s"], scale, 4.0)
    counts = ctx.region_histograms(sc["Y"][L_ - 1], q, W3[:, L_ - 1], None, FLOOR)
    assert counts[2].sum() < ONE <= counts[1].sum()
    tone = [NONE_, (0.0, 0.0, 1.0, 0.5), (0.3, 0.1, 1.0, 0.5)]
    one, cv = f.apply_local_auto(sc["tx"], L_, sc["s"], W3, tone, DETAIL, scale, 4.0, FLOOR, F32, want_curves=True)
    assert np.array_equal(cv[2], nle.tone_curve(None, 0.3, 0.1))
    assert np.array_equal(cv[1], nle.tone_curve(counts[1], 0.0, 0.0, 1.0, 0.5))
    two, cv2, _ = staged(nle, ctx, sc, tone, F32, q=q)
    assert torch.equal(one, two) and np.array_equal(cv, cv2)


@pytest.mark.gpu
def test_composite_refusals(nle, ctx, small):
    sc = small
    f = sc["f"]
    ok = [NONE_, (0.0, 0.0, 1.0, 0.0), NONE_]
    for m, bad, word in ((1, (0.0, 0.0, 26.0, 0.0), "clip_percent"), (0, (1.5, 0.0, -1.0, 0.0), "shadows"),
                         (2, (0.0, float("nan"), -1.0, 0.0), "highlights"), (2, (0.0, 0.0, -1.0, 1.5), "equalise")):
        tone = list(ok)
        tone[m] = bad
        with pytest.raises(nle.NLEError, match=r"nle_apply_local_auto: row %d: .*%s" % (m, word)):
            f.apply_local_auto(sc["tx"], L_, sc["s"], W3, tone, DETAIL, sc["scale"])
    with pytest.raises(nle.NLEError, match="nle_apply_local_auto.*spread"):
        f.apply_local_auto(sc["tx"], L_, sc["s"], W3, ok, DETAIL, sc["scale"], spread=0.0)
    with pytest.raises(nle.NLEError, match="nle_apply_local_auto.*floor"):
        f.apply_local_auto(sc["tx"], L_, sc["s"], W3, ok, DETAIL, sc["scale"], floor=0.0)
    d2 = DETAIL.copy()
    d2[1, 1] = 3.5
    with pytest.raises(nle.NLEError, match="nle_apply_local_auto: row 1: the detail gain"):
        f.apply_local_auto(sc["tx"], L_, sc["s"], W3, ok, d2, sc["scale"])
    with pytest.raises(nle.NLEError, match="nle_apply_local_auto"):
        f.apply_local_auto(sc["tx"][:-1], L_, sc["s"][:, :-1], W3, ok, DETAIL, sc["scale"])          # H W that is not the filter's
    import torch
    assert torch.equal(f.apply_local_auto(sc["tx"], L_, sc["s"], W3, ok, DETAIL, sc["scale"]), staged(nle, ctx, sc, ok, F32)[0])


@pytest.mark.gpu
def test_levels_stretch_their_own_block_and_leave_the_other(nle, ctx, small):
    """the stage calls on hard membership planes (alpha is 0 or 1): `levels = 0` on the dark block's row alone.  The row's
    histogram is the dark block's own, so lo and hi are its smallest and largest weighted base value up to a bin, and the
    block's curved base runs over the curve's whole range [T_0, T_N] = [0, 255] up to the share of one bin at each end.  Every byte of the
    other block is what the combine gives without the option."""
    import torch
    sc = small
    dark = (np.arange(W_)[None, :] < W_ // 2).repeat(H_, axis=0).ravel()
    hard = torch.as_tensor(np.stack([dark, ~dark]).astype(np.float32), device=sc["tx"].device)
    Wp = np.tile([0.0, 0.0, 1.0], (M_ + 1, 1))                       # the base layer alone, no detail: y is the curved base
    base = sc["Y"][L_ - 1].cpu().numpy().astype(np.float64)
    counts = ctx.region_histograms(sc["Y"][L_ - 1], hard, Wp[:, L_ - 1], [0, 1, 0], FLOOR)
    assert np.array_equal(counts[1], ONE * np_hist(base[dark], 1.0)) and not counts[0].any() and not counts[2].any()
    curve = nle.tone_curve(counts[1], 0.0, 0.0, 0.0, 0.0)
    lo, hi = curve[:2]
    assert lo <= base[dark].min() < lo + 0.25 and hi - 0.25 <= base[dark].max() < hi and hi - lo < 200
    y0 = ctx.local_combine(sc["tx"].reshape(-1), sc["Y"], hard, Wp, None, None, FLOOR, ROUNDED8).cpu().numpy()
    y1 = ctx.local_combine(sc["tx"].reshape(-1), sc["Y"], hard, Wp, None, [None, curve, None], FLOOR, ROUNDED8).cpu().numpy()
    assert np.array_equal(y1[~dark], y0[~dark])
    step = 255.0 * 0.25 / (hi - lo)                                   # what one bin of the base is worth after the stretch
    assert y1[dark].min() <= step + 0.5 and y1[dark].max() >= 255.0 - step - 0.5
    assert y0[dark].max() - y0[dark].min() < 200
