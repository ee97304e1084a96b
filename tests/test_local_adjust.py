"""Local adjustments: per-region detail, tone and saturation (include/nle.h at nle_local_combine states
the rule).  There is no reference for it, so the rule is restated here in numpy on top of the restatements of the rules it
is made of (tests/test_region_edits.py's memberships in meaning, tests/test_detail_curve.py's `rule`, tests/test_tone_curve.py's
`tone_rule`), in two precisions: float64 in the rule's own order, the yardstick wherever no exp is evaluated (the device
reproduces it bit for bit), and longdouble, the yardstick with a detail curve on.

Bounds.  Every row's detail curve off: each operation of the rule is one IEEE fp64 operation, base tone curves included, so
the device equals the float64 restatement in every bit.  A detail curve on: tests/test_tone_curve.py's bars (check_tone) --
at most n // 100000 pixels (none at these sizes) differ from the longdouble restatement, by at most one fp32 spacing or one
level; test_float64_restatement_meets_the_cap shows on the CPU that the rule alone (float64 against longdouble) meets that
for every seed the GPU cases use, so a miss on the device is the device's.  Chroma: no transcendental, bit for bit.
Identities (a) .. (e) of the header: (a), (b) bitwise up to the sign of a zero; (c), (d), (e) to the bounds derived at the tests."""
import ctypes as C
import os
import re
import shutil
import subprocess
import textwrap

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT
from test_detail_curve import F32, KINDS, NL, ROUNDED8, U8, colour_scene, planes, read_rgb8, rule, scene48, train_scene, unsigned_zero
from test_tone_curve import WHERE, manual_curve, store_nan, tone_rule

ENHANCE = os.path.join(PKG_DIR, "bin", "enhance")
FLOOR = 0.05
FILL = -12345.0
EPS = 2.0 ** -53
NS = [1, 3, 4, 5, 1023, 4099]
LS = [1, 2, 4, 5, 16]
MS = [1, 2, 8]


# ------------------------------------------------------------------------------------------------ the restatement
def memberships(Q, floor, dt=np.float64):
    """alpha_0 .. alpha_M, (M + 1, n), of the fp32 planes Q (M, n)"""
    Q = np.asarray(Q, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        u = np.where(Q > 0, Q, np.float32(0)).astype(dt)          # a NaN compares false: it counts as 0
        sigma = u[0]
        for m in range(1, u.shape[0]):
            sigma = sigma + u[m]
        d = np.where(sigma > dt(floor), sigma, dt(floor))
        return np.stack([dt(1.0) - sigma / d] + [u[m] / d for m in range(u.shape[0])])


def blend(alpha, rows, dt=np.float64):
    """((c_0 + c_1) + ..) + c_M with c_m = alpha_m > 0 ? alpha_m rows_m : 0; rows_m an array or a scalar"""
    y = None
    with np.errstate(invalid="ignore"):
        for m in range(alpha.shape[0]):
            c = np.where(alpha[m] > 0, alpha[m] * np.asarray(rows[m], dtype=dt), dt(0.0))
            y = c if y is None else y + c
    return y


def local_rule(x, Y, Q, W, detail, curves, floor=FLOOR, dt=np.float64):
    """y of the rule in dtype dt (the base tone curve always in fp64, as tone_rule has it): W (M + 1, L), detail (M + 1, 3) =
    (w_rho, gain, sigma), curves M + 1 entries, None or a curve"""
    alpha = memberships(Q, floor, dt)
    rows = []
    for m in range(alpha.shape[0]):
        w_rho, a, sigma = detail[m]
        if curves is not None and curves[m] is not None:
            rows.append(tone_rule(x, Y, W[m], w_rho, curves[m], a, sigma, dt))
        else:
            rows.append(rule(x, Y, W[m], w_rho, a, sigma, dt))
    return blend(alpha, rows, dt)


def chroma_rule(a, b, Q, s, floor=FLOOR):
    """(a', b') as fp32: c = the blend of the saturations, 128 + c (a - 128), each rounded once"""
    c = blend(memberships(Q, floor), [np.float64(v) for v in s])
    a, b = np.asarray(a, dtype=np.float32).astype(np.float64), np.asarray(b, dtype=np.float32).astype(np.float64)
    return (128.0 + c * (a - 128.0)).astype(np.float32), (128.0 + c * (b - 128.0)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the inputs
def member_planes(n, M, seed):
    """M planes of n fp32 values: negative, NaN, sums below and above the floor, regions that have no influence on a pixel
    (what the kernel skips), a pixel with none at all and one where region 1 has all of it"""
    rng = np.random.default_rng(seed)
    q = rng.uniform(-1.0, 1.5, (M, n)).astype(np.float32)
    owner = rng.integers(0, M + 2, n)                   # 0, M + 1: as drawn; m: only region m may be positive here
    for m in range(M):
        lone = (owner >= 1) & (owner <= M) & (owner != m + 1)
        q[m, lone] = -np.abs(q[m, lone])
    q[:, rng.random(n) < 0.2] *= np.float32(0.004)      # sums below the floor: the background keeps a share
    for _ in range(1 + n // 200):
        q[rng.integers(M), rng.integers(n)] = np.nan
    q[:, 0] = -1.0
    if n > 1:
        q[:, 1] = 0.0
        q[0, 1] = FLOOR                                  # sigma == floor exactly: alpha_1 = 1, alpha_0 = 0
    return q


def case_planes(n, L, M):
    """x, Y, Q of the combine cases; from three pixels on one base-layer pixel is NaN"""
    x, Y = planes(n, L, 1000 * M + 300 * L + n)
    Y = Y.copy()
    if n >= 3:
        Y[L - 1, n // 2] = np.nan
    return x, Y, member_planes(n, M, 7000 * M + 31 * L + n)


GAINS, SIGMAS = (2.5, 0.0, 3.0, 0.5), (6.0, 4.0, 20.0)


def row_curve(m):
    return manual_curve(13.0 + m, 150.25 + 3 * m, (0.8, -0.4, 0.3)[m % 3], (-0.5, 0.6, 0.0)[m % 3])


def row_params(M, L, config, seed=0):
    """W, detail, curves of the M + 1 rows.  config: "off" no curve of either kind (nothing in LDS); "base" detail curves off,
    a base curve on every row (all M + 1 in LDS); "mixed" detail curves on odd rows, one base curve, on the last row (one in
    LDS); "all" both on every row"""
    rng = np.random.default_rng(100 * M + L + seed)
    W = rng.uniform(0.5, 3.0, (M + 1, L))
    W[:, L - 1] = rng.uniform(0.9, 1.6, M + 1)          # the weighted base runs from below every lo to above every hi
    detail = np.zeros((M + 1, 3))
    curves = [None] * (M + 1)
    for m in range(M + 1):
        on = config == "all" or (config == "mixed" and m % 2 == 1)
        detail[m] = (rng.uniform(0.0, 2.0), GAINS[m % 4] if on else (1.0, 2.5)[m % 2], SIGMAS[m % 3] if on else (6.0, 0.0)[m % 2])
        if config in ("base", "all") or (config == "mixed" and m == M):
            curves[m] = row_curve(m)
    exp_on = any(d[2] != 0 and d[1] != 1 for d in detail)
    assert exp_on == (config in ("mixed", "all"))
    return W, detail, curves, exp_on


CONFIGS = ["off", "base", "mixed", "all"]


# ------------------------------------------------------------------------------------------------ CPU
def test_header_constants_and_entry_points_are_mirrored(nle):
    text = open(os.path.join(ROOT, "include", "nle.h")).read()
    assert int(re.search(r"^#define\s+NLE_LOCAL_SATURATION_MAX\s+(\d+)\s*$", text, flags=re.M).group(1)) == nle.LOCAL_SATURATION_MAX == 4
    assert nle.REGION_MAX == 8 and nle.REGION_LAYERS_MAX == 16
    for name in ("nle_local_combine", "nle_local_chroma", "nle_apply_local"):
        assert name in nle.EXPORTED_SYMBOLS and hasattr(nle.lib(), name) and re.search(r"\b%s\s*\(" % name, text)
    assert callable(nle.Context.local_combine) and callable(nle.Context.local_chroma) and callable(nle.NLEFilter.apply_local)
    assert nle.KERNEL_COUNT == 12 and nle.KERNEL_COUNT_ALL == 16        # no new kernel ids


def cap_differences(want, got, kind):
    """(pixels that differ, the worst difference in fp32 spacings or levels)"""
    with np.errstate(invalid="ignore"):
        bad = (got != want) & ~(np.isnan(got.astype(np.float64)) & np.isnan(want.astype(np.float64)))
    differ = int(np.count_nonzero(bad))
    unit = np.spacing(np.abs(want[bad])).astype(np.float64) if kind == F32 else 1.0
    worst = float(np.max(np.abs(got[bad].astype(np.float64) - want[bad].astype(np.float64)) / unit)) if differ else 0.0
    return differ, worst


@pytest.mark.parametrize("M", MS)
def test_float64_restatement_meets_the_cap(M):
    """the cap of the curve-on GPU cases -- at most n // 100000 pixels off the longdouble restatement, by at most one unit --
    is met by the rule alone in float64, on every input and setting those cases use"""
    total = 0
    for n in NS:
        for L in LS:
            x, Y, Q = case_planes(n, L, M)
            for config in ("mixed", "all"):
                W, detail, curves, _ = row_params(M, L, config)
                y64 = local_rule(x, Y, Q, W, detail, curves)
                yld = local_rule(x, Y, Q, W, detail, curves, dt=np.longdouble)
                for kind in KINDS:
                    differ, worst = cap_differences(store_nan(yld, kind), store_nan(y64, kind), kind)
                    total += differ
                    assert differ <= n // 100000 and worst <= 1.0, (n, L, M, config, kind, differ, worst)
    assert total == 0


def test_restated_identities():
    """(a), (b), (c) and (e) on the restatement itself: what the GPU identities hold the kernel to is true of the rule"""
    n, L = 4099, 4
    x, Y = planes(n, L, 5)
    for M in MS:
        W, detail, curves, _ = row_params(M, L, "all")
        single = [tone_rule(x, Y, W[m], detail[m][0], curves[m], detail[m][1], detail[m][2]) for m in range(M + 1)]
        Q = member_planes(n, M, 11)
        Qa = -np.abs(Q)                                                     # (a): every q <= 0 or NaN
        assert np.array_equal(local_rule(x, Y, Qa, W, detail, curves), single[0])
        if M == 1:                                                          # (b): q_1 >= floor everywhere
            Qb = np.maximum(np.nan_to_num(np.abs(Q), nan=1.0), np.float32(FLOOR)).astype(np.float32)
            Qb[0, :50] = FLOOR
            assert np.array_equal(local_rule(x, Y, Qb, W, detail, curves), single[1])
        # (c): all rows equal -- sigma has M - 1 roundings, every alpha_m one more (alpha_0 two), every product one, the sum M:
        # at most 2 M + 4 roundings, each of a value no larger than |y| (the c_m have y's sign and sum to it)
        Wc, dc, cc = np.tile(W[0], (M + 1, 1)), np.tile(detail[0], (M + 1, 1)), [curves[0]] * (M + 1)
        y = local_rule(x, Y, Q, Wc, dc, cc)
        assert np.all(np.abs(y - single[0]) <= (2 * M + 4) * EPS * np.abs(single[0]) * (1 + 1e-9))
        # (e): the saturations all 1
        c = blend(memberships(Q, FLOOR), [1.0] * (M + 1))
        assert np.all(np.abs(c - 1.0) <= (2 * M + 4) * EPS)


# ------------------------------------------------------------------------------------------------ GPU: the stage kernel
LOCAL_WHERE = [dict(w) for w in WHERE] + [dict(oq=1), dict(oq=3, ox=1, ol=2, oo=1), dict(lstride=1), dict(qstride=2)]


def dev_local(ctx, x, Y, Q, ox=0, ol=0, oq=0, oo=0, stride=0, lstride=0, qstride=0, kind=F32):
    """x, Y, Q and a prefilled output on the device: base pointers ox, ol, oq, oo elements past a 16-byte boundary, the layers
    n + stride + lstride floats apart and the membership planes n + stride + qstride, the output 64 elements longer than n"""
    import torch
    d = f"cuda:{ctx.device}"
    n = x.size

    def put(v, off, extra):
        v = np.atleast_2d(v)
        s = n + extra
        buf = torch.zeros(v.shape[0] * s + 8, device=d)[off:off + v.shape[0] * s]
        t = buf.as_strided((v.shape[0], n), (s, 1))
        t.copy_(torch.from_numpy(np.array(v)))
        assert t.data_ptr() % 16 == 4 * off
        return t
    tx, tY, tQ = put(x, ox, 0)[0], put(Y, ol, stride + lstride), put(Q, oq, stride + qstride)
    if kind == U8:
        out = torch.full((n + 64 + 8,), 0x55, dtype=torch.uint8, device=d)[oo:oo + n + 64]
    else:
        out = torch.full((n + 64 + 8,), FILL, dtype=torch.float32, device=d)[oo:oo + n + 64]
    assert out.data_ptr() % 16 == (oo if kind == U8 else 4 * oo)
    return tx, tY, tQ, out


def check_local(ctx, x, Y, Q, W, detail, curves, want, exp_on, kind, label, **where):
    """one call of the stage kernel against the stored restatement `want`: bit for bit without an exp, check_tone's bars with"""
    n = x.size
    tx, tY, tQ, out = dev_local(ctx, x, Y, Q, kind=kind, **where)
    got = ctx.local_combine(tx, tY, tQ, W, detail, curves, FLOOR, kind, out=out[:n])
    assert got.data_ptr() == out.data_ptr()
    tail = out[n:].cpu().numpy()
    assert np.all(tail == (0x55 if kind == U8 else np.float32(FILL))), "written past n"
    got = out[:n].cpu().numpy()
    if kind != U8:
        got = unsigned_zero(got)                        # the sign of a zero is left open (a skipped row's 0 is +0)
        want = unsigned_zero(want)
        assert np.array_equal(np.isnan(got), np.isnan(want)), label
        keep = ~np.isnan(want)
        got, want = got[keep], want[keep]
        assert not np.any(got == np.float32(FILL)) or np.any(want == np.float32(FILL)), "a pixel was not written"
    if not exp_on:
        view = np.uint8 if kind == U8 else np.int32
        assert np.array_equal(got.view(view), want.view(view)), label
        return
    differ, worst = cap_differences(want, got, kind)
    if differ:
        print(f"{label} kind {kind}: {differ} of {got.size} differ from the longdouble restatement, worst {worst:.1f} units")
    assert differ <= n // 100000 and worst <= 1.0, (label, differ, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("n", NS)
def test_local_combine_is_the_restatement(ctx, n, L, M):
    """every size, layer count and region count; every base pointer off its 16-byte boundary, strides that are no multiple
    of 4; memberships negative, NaN, below and above the floor; a NaN base pixel; base values below lo and above hi; no,
    one and all M + 1 tone curves in LDS"""
    x, Y, Q = case_planes(n, L, M)
    if n > 1000:
        assert np.nanmin(0.9 * Y[L - 1]) < 13.0 - 5 and np.nanmax(1.6 * Y[L - 1]) > 150.25 + 3 * M + 5
        al = memberships(Q, FLOOR)
        assert np.any((al[0] > 0) & (al[0] < 1)) and np.any(np.all(al[1:] == 0, axis=0)) and np.any(al[0] == 0)
        assert all(np.any(al[m] == 0) and np.any(al[m] > 0) for m in range(M + 1))       # every row is skipped somewhere
    for config in CONFIGS:
        W, detail, curves, exp_on = row_params(M, L, config)
        y = local_rule(x, Y, Q, W, detail, curves, dt=np.longdouble if exp_on else np.float64)
        if n >= 3:
            assert np.isnan(y[n // 2])
        for kind in KINDS:
            want = store_nan(y, kind)
            for where in LOCAL_WHERE:
                check_local(ctx, x, Y, Q, W, detail, curves, want, exp_on, kind, f"n {n} L {L} M {M} {config} {where}", **where)


def single_row(ctx, tx, tY, W, detail, curves, m, kind):
    w_rho, a, sigma = detail[m]
    if curves is not None and curves[m] is not None:
        return ctx.tone_combine(tx, tY, W[m], curves[m], w_rho, a, sigma, kind)
    return ctx.detail_combine(tx, tY, W[m], w_rho, a, sigma, kind)


def same_up_to_zero_sign(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    if a.dtype == np.uint8:
        return np.array_equal(a, b)
    a, b = unsigned_zero(a), unsigned_zero(b)
    return np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 4, 16])
def test_identities_a_and_b_single_rows_are_the_detail_and_tone_kernels_bit_for_bit(ctx, L):
    n = 4099
    x, Y = planes(n, L, 40 + L)
    for M in (1, 8):
        for config in CONFIGS:
            W, detail, curves, _ = row_params(M, L, config)
            Q = member_planes(n, M, 3 + M)
            Qa = -np.abs(Q)                              # (a): every q <= 0 or NaN
            tx, tY, tQ, _ = dev_local(ctx, x, Y, Qa)
            for kind in KINDS:
                got = ctx.local_combine(tx, tY, tQ, W, detail, curves, FLOOR, kind)
                assert same_up_to_zero_sign(got, single_row(ctx, tx, tY, W, detail, curves, 0, kind)), ("a", L, M, config, kind)
            if M == 1:                                   # (b): q_1 >= floor everywhere, exactly the floor at some pixels
                Qb = np.maximum(np.nan_to_num(np.abs(Q), nan=1.0), np.float32(FLOOR)).astype(np.float32)
                Qb[0, :50] = FLOOR
                tx, tY, tQ, _ = dev_local(ctx, x, Y, Qb)
                for kind in KINDS:
                    got = ctx.local_combine(tx, tY, tQ, W, detail, curves, FLOOR, kind)
                    assert same_up_to_zero_sign(got, single_row(ctx, tx, tY, W, detail, curves, 1, kind)), ("b", L, config, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 4, 16])
def test_identity_c_equal_rows_are_the_single_row(ctx, L):
    """y differs from the single-row y by at most 2 M + 4 fp64 roundings (test_restated_identities): the fp32 store by at
    most one spacing, the 8-bit kinds nowhere but within 1e-9 of a tie of the single-row value"""
    n = 4099
    x, Y = planes(n, L, 60 + L)
    for M in MS:
        Q = member_planes(n, M, 9 + M)
        for config in ("off", "all"):
            W, detail, curves, _ = row_params(M, L, config)
            Wc, dc, cc = np.tile(W[0], (M + 1, 1)), np.tile(detail[0], (M + 1, 1)), [curves[0]] * (M + 1)
            w_rho, a, sigma = dc[0]                                                  # the single row, in fp64
            y1 = tone_rule(x, Y, Wc[0], w_rho, cc[0], a, sigma) if cc[0] is not None else rule(x, Y, Wc[0], w_rho, a, sigma)
            tie = np.abs(np.abs(y1 - np.floor(y1)) - 0.5) <= 1e-9
            assert np.count_nonzero(tie) < n // 100
            tx, tY, tQ, _ = dev_local(ctx, x, Y, Q)
            for kind in KINDS:
                got = ctx.local_combine(tx, tY, tQ, Wc, dc, cc, FLOOR, kind).cpu().numpy()
                one = single_row(ctx, tx, tY, Wc, dc, cc, 0, kind).cpu().numpy()
                if kind == F32:
                    assert np.all(np.abs(got.astype(np.float64) - one.astype(np.float64)) <= np.spacing(np.abs(one)).astype(np.float64))
                else:
                    assert np.array_equal(got[~tie], one[~tie]), (L, M, config, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 4, 16])
def test_identity_d_plain_rows_are_the_region_combine_up_to_association(ctx, L):
    """every curve off, w_rho = 0, no base curve: both kernels evaluate sum_m sum_l alpha_m W[m][l] Y_l in fp64, the region
    kernel blending the weights first, this one the rows' sums.  Either is within (M + L + 2) roundings of the terms' absolute
    sum of the exact value, so the two fp32 stores differ by at most one spacing plus twice that; the 8-bit kinds are equal
    wherever the value is not within 1e-9 of a tie"""
    n = 4099
    x, Y = planes(n, L, 80 + L)
    for M in MS:
        Q = member_planes(n, M, 13 + M)
        W, detail, _, _ = row_params(M, L, "off")
        detail[:, 0] = 0.0
        al = memberships(Q, FLOOR)
        mag = (al[:, None, :] * np.abs(W)[:, :, None] * np.abs(Y.astype(np.float64))[None]).sum(axis=(0, 1))
        y = local_rule(x, Y, Q, W, detail, None)
        tie = np.abs(np.abs(y - np.floor(y)) - 0.5) <= 1e-9
        tx, tY, tQ, _ = dev_local(ctx, x, Y, Q)
        for kind in KINDS:
            got = ctx.local_combine(tx, tY, tQ, W, detail, None, FLOOR, kind).cpu().numpy()
            reg = ctx.region_combine(tY, tQ, W, FLOOR, kind).cpu().numpy()
            if kind == F32:
                bound = np.spacing(np.abs(reg)).astype(np.float64) + 2 * (M + L + 2) * 2 * EPS * mag
                assert np.all(np.abs(got.astype(np.float64) - reg.astype(np.float64)) <= bound)
            else:
                assert np.array_equal(got[~tie], reg[~tie]), (L, M, kind)


# ------------------------------------------------------------------------------------------------ GPU: chroma
def dev_chroma(ctx, a, b, Q, oa=0, ob=0, oq=0, ooa=0, oob=0, qextra=0):
    import torch
    d = f"cuda:{ctx.device}"
    n = a.size
    ta = torch.full((n + 64 + 8,), FILL, device=d)[oa:oa + n + 64]
    tb = torch.full((n + 64 + 8,), FILL, device=d)[ob:ob + n + 64]
    ta[:n].copy_(torch.from_numpy(a))
    tb[:n].copy_(torch.from_numpy(b))
    s = n + qextra
    tQ = torch.zeros(Q.shape[0] * s + 8, device=d)[oq:oq + Q.shape[0] * s].as_strided((Q.shape[0], n), (s, 1))
    tQ.copy_(torch.from_numpy(Q))
    oa_ = torch.full((n + 64 + 8,), FILL, device=d)[ooa:ooa + n + 64]
    ob_ = torch.full((n + 64 + 8,), FILL, device=d)[oob:oob + n + 64]
    return ta, tb, tQ, oa_, ob_


CHROMA_WHERE = [dict(), dict(oa=1), dict(ob=2), dict(oq=3), dict(ooa=1), dict(oob=3), dict(oa=3, ob=1, oq=2, ooa=2, oob=1),
                dict(qextra=1), dict(qextra=2), dict(qextra=3)]


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 8])
@pytest.mark.parametrize("n", NS)
def test_local_chroma_is_the_restatement_bit_for_bit(ctx, n, M):
    rng = np.random.default_rng(17 * n + M)
    a, b = rng.uniform(0, 255, n).astype(np.float32), rng.uniform(0, 65535 / 257.0, n).astype(np.float32)
    if n >= 3:
        a[n // 2] = np.nan
    Q = member_planes(n, M, 23 * n + M)
    s = np.array([1.0, 0.0, 4.0, 0.5, 1.75, 0.25, 3.0, 1.0, 2.0])[:M + 1]
    wa, wb = chroma_rule(a, b, Q, s)
    for where in CHROMA_WHERE:
        for inplace in (False, True):
            ta, tb, tQ, oa, ob = dev_chroma(ctx, a, b, Q, **where)
            if inplace:
                ga, gb = ctx.local_chroma(ta[:n], tb[:n], tQ, s, FLOOR, out="inplace")
                assert ga.data_ptr() == ta.data_ptr() and gb.data_ptr() == tb.data_ptr()
                oa, ob = ta, tb
            else:
                ctx.local_chroma(ta[:n], tb[:n], tQ, s, FLOOR, out=(oa[:n], ob[:n]))
                assert np.array_equal(ta[:n].cpu().numpy().view(np.int32), a.view(np.int32))    # the inputs are not touched
            for t, want in ((oa, wa), (ob, wb)):
                got = t.cpu().numpy()
                assert np.all(got[n:] == np.float32(FILL)), "written past n"
                assert np.array_equal(unsigned_zero(got[:n]).view(np.int32), unsigned_zero(want).view(np.int32)), (n, M, where, inplace)
    # (e): saturations all 1 -- c = 1 up to (2 M + 4) 2^-53, so a' = a up to one fp32 spacing
    ta, tb, tQ, oa, ob = dev_chroma(ctx, a, b, Q)
    ga, gb = ctx.local_chroma(ta[:n], tb[:n], tQ, np.ones(M + 1), FLOOR)
    for g, v in ((ga, a), (gb, b)):
        g = g.cpu().numpy()
        keep = ~np.isnan(v)
        assert np.array_equal(np.isnan(g), np.isnan(v))
        assert np.all(np.abs(g[keep].astype(np.float64) - v[keep].astype(np.float64)) <= np.spacing(np.abs(v[keep])).astype(np.float64))


# ------------------------------------------------------------------------------------------------ GPU: refusals
def same_f32(got, want):
    """fp32 results equal bit for bit, NaN where NaN and the sign of a zero apart"""
    got, want = unsigned_zero(np.asarray(got)), unsigned_zero(np.asarray(want))
    keep = ~np.isnan(want)
    return np.array_equal(np.isnan(got), ~keep) and np.array_equal(got[keep].view(np.int32), want[keep].view(np.int32))


def raw_local(nle, ctx, x, Y, Q, L, M, n, ls, qs, W, detail, on, curves, floor, kind, out):
    ctx._sync_in()
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    A = lambda v, dt=np.float64: np.ascontiguousarray(v, dtype=dt).ctypes.data_as(C.c_void_p) if v is not None else None  # noqa: E731
    return nle.lib().nle_local_combine(ctx._h, P(x), P(Y), L, P(Q), M, n, ls, qs, A(W), A(detail), A(on, np.int32), A(curves),
                                       floor, kind, P(out))


def raw_chroma(nle, ctx, a, b, Q, M, n, qs, s, floor, oa, ob):
    ctx._sync_in()
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    sp = np.ascontiguousarray(s, dtype=np.float64).ctypes.data_as(C.c_void_p) if s is not None else None
    return nle.lib().nle_local_chroma(ctx._h, P(a), P(b), P(Q), M, n, qs, sp, floor, P(oa), P(ob))


@pytest.mark.gpu
def test_refusals_have_their_messages_and_leave_the_ctx_usable(nle, ctx):
    import torch
    n, L, M = 1000, 4, 2
    x, Y, Q = case_planes(n, L, M)
    W, detail, curves, _ = row_params(M, L, "base")
    on = np.ones(M + 1, dtype=np.int32)
    cv = np.stack(curves)
    tx, tY, tQ, out = dev_local(ctx, x, Y, Q)
    want = store_nan(local_rule(x, Y, Q, W, detail, curves), F32)
    nan, inf = float("nan"), float("inf")

    def bent(arr, idx, v):
        arr = np.array(arr, dtype=np.float64)
        arr[idx] = v
        return arr
    good = (tx, tY, tQ, L, M, n, n, n, W, detail, on, cv, FLOOR, F32, out)

    def call(**kw):
        names = ("x", "Y", "Q", "L", "M", "n", "ls", "qs", "W", "detail", "on", "curves", "floor", "kind", "out")
        args = dict(zip(names, good))
        args.update(kw)
        return lambda: raw_local(nle, ctx, *[args[k] for k in names])
    bad = [(call(x=None), "NULL"), (call(Y=None), "NULL"), (call(Q=None), "NULL"), (call(out=None), "NULL"), (call(W=None), "NULL"),
           (call(detail=None), "NULL"), (call(curves=None), "NULL curves"),
           (call(L=0), "layers"), (call(L=17, W=np.ones((M + 1, 17))), "layers"), (call(M=0), "regions"), (call(M=9), "regions"),
           (call(W=bent(W, (1, 2), nan)), "row 1: weight 2"), (call(detail=bent(detail, (2, 0), inf)), "row 2: the residual weight"),
           (call(detail=bent(detail, (0, 1), 3.5)), "row 0: the detail gain"), (call(detail=bent(detail, (1, 1), -0.1)), "gain"),
           (call(detail=bent(detail, (1, 1), nan)), "gain"), (call(detail=bent(detail, (1, 2), -1.0)), "row 1: the detail sigma"),
           (call(detail=bent(detail, (0, 2), inf)), "sigma"), (call(floor=0.0), "floor"), (call(floor=nan), "floor"), (call(floor=inf), "floor"),
           (call(curves=bent(cv, (1, 0), nan)), "row 1: the curve's range"), (call(curves=bent(cv, (2, 1), cv[2, 0])), "row 2: the curve's range"),
           (call(curves=bent(cv, (0, 2 + 500), nan)), "row 0: knot 500"), (call(curves=bent(cv, (2, 2 + 1024), inf)), "row 2: knot 1024"),
           (call(kind=3), "kind"), (call(n=0), "n must be"), (call(ls=n - 1), "stride"), (call(qs=n - 1), "stride"),
           (call(out=tx), "overlaps the plane"), (call(out=tY[2]), "overlaps a layer"), (call(out=tQ[1]), "overlaps a membership plane")]
    for k, (f, word) in enumerate(bad):
        assert f() == nle.NLE_ERR_INVALID, k
        msg = nle.lib().nle_last_error(ctx._h).decode()
        assert msg.startswith("nle_local_combine") and word in msg, (k, msg)
    # a row that is off is not read: a curve of NaNs behind a flag of 0
    off = on.copy()
    off[1] = 0
    out.fill_(nan)
    assert call(on=off, curves=bent(cv, (1, slice(None)), nan))() == nle.NLE_OK
    c2 = list(curves)
    c2[1] = None
    assert same_f32(out[:n].cpu().numpy(), store_nan(local_rule(x, Y, Q, W, detail, c2), F32))
    assert not same_f32(out[:n].cpu().numpy(), want)
    # chroma
    d = f"cuda:{ctx.device}"
    ta, tb = torch.full((n,), 100.0, device=d), torch.full((n,), 150.0, device=d)
    big = torch.zeros(3 * n, device=d)
    oa, ob = big[:n], big[n:2 * n]
    s = [1.0, 0.5, 2.0]
    cbad = [(lambda: raw_chroma(nle, ctx, None, tb, tQ, M, n, n, s, FLOOR, oa, ob), "NULL"),
            (lambda: raw_chroma(nle, ctx, ta, tb, tQ, M, n, n, None, FLOOR, oa, ob), "NULL"),
            (lambda: raw_chroma(nle, ctx, ta, tb, tQ, M, n, n, s, FLOOR, oa, None), "NULL"),
            (lambda: raw_chroma(nle, ctx, ta, tb, tQ, 9, n, n, [1.0] * 10, FLOOR, oa, ob), "regions"),
            (lambda: raw_chroma(nle, ctx, ta, tb, tQ, M, n, n, [1.0, 4.5, 1.0], FLOOR, oa, ob), "row 1: the saturation"),
            (lambda: raw_chroma(nle, ctx, ta, tb, tQ, M, n, n, [-0.1, 1.0, 1.0], FLOOR, oa, ob), "row 0: the saturation"),
            (lambda: raw_chroma(nle, ctx, ta, tb, tQ, M, n, n, [1.0, 1.0, nan], FLOOR, oa, ob), "row 2: the saturation"),
            (lambda: raw_chroma(nle, ctx, ta, tb, tQ, M, n, n, s, -1.0, oa, ob), "floor"),
            (lambda: raw_chroma(nle, ctx, ta, tb, tQ, M, 0, n, s, FLOOR, oa, ob), "n must be"),
            (lambda: raw_chroma(nle, ctx, ta, tb, tQ, M, n, n - 1, s, FLOOR, oa, ob), "stride"),
            (lambda: raw_chroma(nle, ctx, ta, tb, tQ, M, n, n, s, FLOOR, tb, ob), "d_a_out overlaps d_b"),
            (lambda: raw_chroma(nle, ctx, ta, tb, tQ, M, n, n, s, FLOOR, oa, big[n // 2:n // 2 + n]), "d_b_out overlaps d_a_out"),
            (lambda: raw_chroma(nle, ctx, big[1:n + 1], tb, tQ, M, n, n, s, FLOOR, oa, ob), "d_a_out overlaps d_a"),
            (lambda: raw_chroma(nle, ctx, ta, tb, tQ, M, n, n, s, FLOOR, tQ[0], ob), "membership")]
    for k, (f, word) in enumerate(cbad):
        assert f() == nle.NLE_ERR_INVALID, k
        msg = nle.lib().nle_last_error(ctx._h).decode()
        assert msg.startswith("nle_local_chroma") and word in msg, (k, msg)
    assert raw_chroma(nle, ctx, ta, tb, tQ, M, n, n, s, FLOOR, ta, tb) == nle.NLE_OK          # in place is allowed
    # after all of them the stage call gives what it gave, and the ctx trains and applies like a fresh one
    out.fill_(nan)
    assert call()() == nle.NLE_OK
    assert same_f32(out[:n].cpu().numpy(), want)
    xs = scene48().astype(np.float32)
    outs = []
    fresh = nle.Context(0)
    try:
        for c in (ctx, fresh):
            g = train_scene(nle, c, xs)
            outs.append((np.array(g.eigvals), g.apply_rounded8(xs, nle.transform_eigenvalues(g.eigvals, [3.0, 3.0, 1.0, 0.9])).cpu().numpy()))
            g.close()
    finally:
        fresh.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------------------------------------ GPU: through a trained filter
W4 = [3.0, 3.0, 1.0, 0.9]


def block_strokes(H=48, W=64):
    """three strokes, one in each third of the scene's width"""
    s = np.zeros((3, H, W), dtype=np.float32)
    for m in range(3):
        s[m, 10:38, 4 + 21 * m:17 + 21 * m] = 1.0
    return s


def stroke_scale(s):
    return [s[m].size / float(s[m].astype(np.float64).sum()) for m in range(s.shape[0])]


@pytest.fixture(scope="module")
def scene(nle, ctx):
    import torch
    x = scene48().astype(np.float32)
    f = train_scene(nle, ctx, x)
    tx = torch.as_tensor(x, device=f"cuda:{ctx.device}")
    yield x, tx, f
    f.close()


@pytest.mark.gpu
def test_apply_local_is_the_three_stage_calls(nle, ctx, scene):
    import torch
    x, tx, f = scene
    s = block_strokes()
    scale = stroke_scale(s)
    M = s.shape[0]
    Y = f.apply_layers(tx, NL)
    q = f.region_spread(s, scale, 4.0)
    seen = set()
    for config in CONFIGS:
        W, detail, curves, _ = row_params(M, NL, config)
        for kind in KINDS:
            one, q1 = f.apply_local(tx, NL, s, W, detail, curves, scale, 4.0, FLOOR, kind, want_spreads=True)
            two = ctx.local_combine(tx.reshape(-1), Y, q, W, detail, curves, FLOOR, kind)
            assert one.dtype == two.dtype and torch.equal(one, two), (config, kind)
            assert torch.equal(q1, q)
            assert torch.equal(f.apply_local(tx, NL, s, W, detail, curves, scale, 4.0, FLOOR, kind), one)     # without d_q_out
            seen.add(one.cpu().numpy().tobytes())
    assert len(seen) == len(CONFIGS) * 3
    W, detail, curves, _ = row_params(M, NL, "all")
    for bad, word in ((dict(spread=0.0), "spread"), (dict(floor=float("nan")), "floor"), (dict(scale=[1.0, float("inf"), 1.0]), "scale")):
        kw = dict(scale=scale, spread=4.0, floor=FLOOR)
        kw.update(bad)
        with pytest.raises(nle.NLEError, match="nle_apply_local.*" + word):
            f.apply_local(tx, NL, s, W, detail, curves, **kw)
    with pytest.raises(nle.NLEError, match="nle_apply_local"):
        f.apply_local(tx[:-1], NL, s[:, :-1], W, detail, curves)                # H W that is not the filter's
    d2 = detail.copy()
    d2[2, 1] = 3.5
    with pytest.raises(nle.NLEError, match="nle_apply_local: row 2: the detail gain"):
        f.apply_local(tx, NL, s, W, d2, curves)
    assert torch.equal(f.apply_local(tx, NL, s, W, detail, curves, scale, 4.0, FLOOR, F32),
                       ctx.local_combine(tx.reshape(-1), Y, q, W, detail, curves, FLOOR, F32))


@pytest.mark.gpu
def test_shadows_and_saturation_act_on_their_block_and_leave_the_others(nle, ctx):
    """the three-block scene of tests/test_segments.py, tinted.  Row 1 (the dark block) gets shadows = 0.8 and saturation = 0;
    every other key of every row is the background's, so against the call whose rows are all the background's
    y' - y = alpha_1 (B'_1 - Bw) exactly, and |B' - Bw| <= 255 (4 / 27) 0.8 = 30.3 levels (the header's bound on the curve).
    Hard memberships (the blocks' indicator planes: alpha is 0 or 1): the other two blocks keep their bytes, the dark block's
    base is lifted by 0.8 t (1 - t)^2 255 = 27 levels at Bw = 0.9 * 60 (more than 15 is asked) and goes grey, the channels
    equal up to the 1 level the integer Lab -> BGR conversion leaves between them for a = b = 128 (the oracle's table walk
    gives exactly 1).  Spread strokes (alpha_1 > 0 everywhere on this scene, the diffusion is positive): the change is bounded
    by alpha_1 times the curve's bound, pixel by pixel, so it dies out with the membership."""
    import test_segments as tsg
    x, truth = tsg._blocks()
    H, W, nr, nc, hx, hy, T, K = tsg.BLOCKS
    bgr = np.clip(np.rint(np.stack([0.8 * x + 20, x, 0.9 * x + 10], axis=2)), 0, 255).astype(np.uint8)
    lab, L = ctx.bgr2lab8(bgr)
    f = nle.NLEFilter(ctx).train_filter(L, nr, nc, hx, hy, T, K)
    Y = f.apply_layers(L, NL)
    W_all = np.tile(W4, (4, 1))
    curves = [None, nle.tone_curve(None, 0.8, 0.0), None, None]
    sat = [1.0, 0.0, 1.0, 1.0]
    import torch
    hard = torch.as_tensor(np.stack([(truth == m).astype(np.float32) for m in range(3)]), device=L.device)

    def image(y, q, sat):
        a, b = ctx.lab8_channel(lab, 1).reshape(-1), ctx.lab8_channel(lab, 2).reshape(-1)
        if sat is not None:
            ctx.local_chroma(a, b, q, sat, FLOOR, out="inplace")
        return ctx.lab2bgr8(lab, L=y.view(H, W), a=a.view(H, W), b=b.view(H, W)).cpu().numpy().reshape(-1, 3).astype(int)
    y0 = ctx.local_combine(L.reshape(-1), Y, hard, W_all, None, None, FLOOR, ROUNDED8)
    y1 = ctx.local_combine(L.reshape(-1), Y, hard, W_all, None, curves, FLOOR, ROUNDED8)
    img0, img1 = image(y0, hard, None), image(y1, hard, sat)
    y0, y1 = y0.cpu().numpy(), y1.cpu().numpy()
    dark = truth == 0
    assert np.array_equal(y1[~dark], y0[~dark]) and np.array_equal(img1[~dark], img0[~dark])
    assert np.mean(y1[dark] - y0[dark]) > 15
    assert np.all(img1[dark].max(axis=1) - img1[dark].min(axis=1) <= 1)
    assert np.mean(img0[dark].max(axis=1) - img0[dark].min(axis=1)) > 5          # it was tinted
    # spread strokes, one inside every block
    s = np.zeros((3, H, W), dtype=np.float32)
    s[0, 8:40, 4:18] = 1.0
    s[1, 4:22, 28:60] = 1.0
    s[2, 30:46, 44:62] = 1.0
    assert all(np.all(truth.reshape(H, W)[s[m] > 0] == m) for m in range(3))
    z0, q = f.apply_local(L, NL, s, W_all, None, None, stroke_scale(s), 4.0, FLOOR, F32, want_spreads=True)
    z1 = f.apply_local(L, NL, s, W_all, None, curves, stroke_scale(s), 4.0, FLOOR, F32)
    f.close()
    al = memberships(q.cpu().numpy(), FLOOR)
    dz = z1.cpu().numpy().astype(np.float64) - z0.cpu().numpy().astype(np.float64)
    inside = s[0].ravel() > 0
    print(f"alpha_1: {al[1][inside].mean():.3f} inside its stroke, {al[1][truth == 1].mean():.4f} and {al[1][truth == 2].mean():.4f} "
          f"in the other blocks; mean lift inside {dz[inside].mean():.1f}, largest change outside the dark block {np.abs(dz[~dark]).max():.2f}")
    assert np.all(np.abs(dz) <= al[1] * 255.0 * (4.0 / 27.0) * 0.8 + 1e-3)          # 1e-3: the two fp32 stores of values below 512
    assert np.mean(dz[inside]) > 15 and np.mean(al[1][inside]) > 0.5


# ------------------------------------------------------------------------------------------------ GPU: CLI and C++ surface
def run_cli(lead, src, out, weights):
    from test_detail_curve import SCENE_ARGV
    r = subprocess.run([ENHANCE] + lead + [str(src), str(out)] + SCENE_ARGV + [repr(float(w)) for w in weights], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-1500:])
    return r.stdout


def write_masks(tmp_path, s):
    from PIL import Image
    paths = []
    for m in range(s.shape[0]):
        p = tmp_path / f"mask{m}.png"
        Image.fromarray((s[m] * 255).astype(np.uint8)).save(p)
        paths.append(str(p))
    return paths


# the command line's rows: the background, then one spec per stroke
CLI_BG = ["--residual-weight", "1", "--detail-gain", "2.5", "--detail-sigma", "6", "--shadows", "0.3", "--saturation", "1.25"]
CLI_SPECS = ["weights=2/2/1/1,gain=0.5,shadows=0.8,saturation=0", "residual=0,sigma=0,gain=1,highlights=-0.6", "shadows=0,saturation=2.5"]
PY_W = np.array([W4, [2.0, 2.0, 1.0, 1.0], W4, W4])
PY_DETAIL = np.array([[1.0, 2.5, 6.0], [1.0, 0.5, 6.0], [0.0, 1.0, 0.0], [1.0, 2.5, 6.0]])
PY_TONE = [(0.3, 0.0), (0.8, 0.0), (0.3, -0.6), (0.0, 0.0)]
PY_SAT = [1.25, 0.0, 1.25, 2.5]


def py_curves(nle):
    return [nle.tone_curve(None, sh, hl) if (sh, hl) != (0.0, 0.0) else None for sh, hl in PY_TONE]


@pytest.mark.gpu
def test_cli_8_bit_equals_the_python_composition(nle, ctx, tmp_path):
    from PIL import Image
    bgr = colour_scene()
    H, W = bgr.shape[:2]
    src = tmp_path / "in.bmp"
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(src)
    s = block_strokes()
    masks = write_masks(tmp_path, s)
    lead = list(CLI_BG)
    for m in range(3):
        lead += ["--local", masks[m] + ":" + CLI_SPECS[m]]
    run_cli(lead + ["--region-spread", "3", "--region-floor", "0.1"], src, tmp_path / "o.png", W4)
    lab, L = ctx.bgr2lab8(bgr)
    f = train_scene(nle, ctx, L)
    y, q = f.apply_local(L, NL, s, PY_W, PY_DETAIL, py_curves(nle), stroke_scale(s), 3.0, 0.1, ROUNDED8, want_spreads=True)
    a, b = ctx.lab8_channel(lab, 1).reshape(-1), ctx.lab8_channel(lab, 2).reshape(-1)
    ctx.local_chroma(a, b, q, PY_SAT, 0.1, out="inplace")
    want = ctx.lab2bgr8(lab, L=y.view(H, W), a=a.view(H, W), b=b.view(H, W)).cpu().numpy()
    plain = ctx.lab2bgr8(lab, L=f.apply_rounded8(L, nle.transform_eigenvalues(f.eigvals, W4)).reshape(L.shape)).cpu().numpy()
    f.close()
    got = read_rgb8(tmp_path / "o.png")[..., ::-1]
    assert np.array_equal(got, want) and not np.array_equal(want, plain)
    # the options in the other order write the same bytes
    run_cli(lead[len(CLI_BG):] + ["--region-floor", "0.1", "--region-spread", "3"] + CLI_BG, src, tmp_path / "o2.png", W4)
    assert (tmp_path / "o2.png").read_bytes() == (tmp_path / "o.png").read_bytes()


@pytest.mark.gpu
def test_cli_deep_equals_the_python_composition(nle, ctx, tmp_path):
    from test_deep_colour import gradient16
    from test_image_io16 import png_bytes, read_png16_rgb
    bgr = gradient16(48, 64, 5)
    src = tmp_path / "in.png"
    src.write_bytes(png_bytes(bgr[..., ::-1], filt=1))
    s = block_strokes()
    masks = write_masks(tmp_path, s)
    lead = ["--deep"] + list(CLI_BG)
    for m in range(3):
        lead += ["--local", masks[m] + ":" + CLI_SPECS[m]]
    run_cli(lead, src, tmp_path / "o.png", W4)
    L, a, b, g = ctx.bgr16_to_lab(bgr)
    f = train_scene(nle, ctx, g)
    y, q = f.apply_local(L, NL, s, PY_W, PY_DETAIL, py_curves(nle), stroke_scale(s), 4.0, FLOOR, F32, want_spreads=True)   # on the unrounded L
    plain = ctx.lab_to_bgr16(f.apply(L, nle.transform_eigenvalues(f.eigvals, W4)).reshape(L.shape), a, b).cpu().numpy()
    a2, b2 = ctx.local_chroma(a.reshape(-1), b.reshape(-1), q, PY_SAT, FLOOR)
    want = ctx.lab_to_bgr16(y.reshape(L.shape), a2.reshape(L.shape), b2.reshape(L.shape)).cpu().numpy()
    f.close()
    assert np.array_equal(read_png16_rgb(tmp_path / "o.png")[..., ::-1], want) and not np.array_equal(want, plain)


@pytest.mark.gpu
def test_cli_segments_equal_the_python_composition(nle, ctx, tmp_path):
    from PIL import Image
    bgr = colour_scene()
    H, W = bgr.shape[:2]
    src = tmp_path / "in.bmp"
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(src)
    stdout = run_cli(["--segments", "3", "--shadows", "0.3", "--local", "@1:weights=2/2/1/1,shadows=0.8,saturation=0", "--local", "@2:highlights=-0.6"],
                     src, tmp_path / "o.png", W4)
    assert len(re.findall(r"^Segment \d: \d+ pixels", stdout, flags=re.M)) == 3 and "Segments: 3 iterations" in stdout
    lab, L = ctx.bgr2lab8(bgr)
    f = train_scene(nle, ctx, L)
    r = f.segment(3, want_spreads=True)
    Wt = np.array([W4, W4, [2.0, 2.0, 1.0, 1.0], W4])                     # the background, then segments 0, 1, 2
    detail = np.tile([0.0, 1.0, 0.0], (4, 1))
    curves = [nle.tone_curve(None, 0.3, 0.0), nle.tone_curve(None, 0.3, 0.0), nle.tone_curve(None, 0.8, 0.0), nle.tone_curve(None, 0.3, -0.6)]
    y = ctx.local_combine(L.reshape(-1), f.apply_layers(L, NL), r["spreads"], Wt, detail, curves, FLOOR, ROUNDED8)
    a, b = ctx.lab8_channel(lab, 1).reshape(-1), ctx.lab8_channel(lab, 2).reshape(-1)
    ctx.local_chroma(a, b, r["spreads"], [1.0, 1.0, 0.0, 1.0], FLOOR, out="inplace")
    want = ctx.lab2bgr8(lab, L=y.view(H, W), a=a.view(H, W), b=b.view(H, W)).cpu().numpy()
    f.close()
    assert np.array_equal(read_rgb8(tmp_path / "o.png")[..., ::-1], want)


@pytest.mark.gpu
def test_specs_that_name_the_backgrounds_values_write_the_plain_image_up_to_ties(nle, ctx, tmp_path):
    """identity (c) through the tool: every key of every spec equals the background's, so y is the single-row y up to
    2 M + 4 fp64 roundings and the stored level differs only where that y lies within ~1e-13 of a .5 tie.  The scene has
    3072 pixels: a tie that close is not expected at all, and more than 3 (one pixel in a thousand) would be a defect."""
    from PIL import Image
    bgr = colour_scene()
    src = tmp_path / "in.bmp"
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(src)
    masks = write_masks(tmp_path, block_strokes())
    bg = ["--residual-weight", "1", "--detail-gain", "2.5", "--detail-sigma", "6", "--shadows", "0.3"]
    spec = "weights=3/3/1/0.9,residual=1,gain=2.5,sigma=6,shadows=0.3,highlights=0,saturation=1"
    run_cli(bg, src, tmp_path / "plain.png", W4)
    run_cli(bg + ["--saturation", "1"] + sum([["--local", m + ":" + spec] for m in masks], []), src, tmp_path / "local.png", W4)
    a, b = read_rgb8(tmp_path / "plain.png").astype(int), read_rgb8(tmp_path / "local.png").astype(int)
    differ = np.any(a != b, axis=2)
    ties = int(np.count_nonzero(differ))
    print(f"{ties} of {differ.size} pixels differ between the plain command and the all-background --local command")
    assert ties <= 3
    assert np.all(np.abs(a - b)[differ] <= 3) if ties else True       # one level of L moves a channel by a few codes at most


DRIVER = textwrap.dedent(r"""
    #include <cstdio>
    #include <cstring>
    #include <stdexcept>
    #include <string>
    #include <vector>
    #include "nle.h"
    #include "nle/filter.hpp"
    #include "nle/image_io.hpp"
    #define REQUIRE(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)
    static bool same(const nle::Image& a, const nle::Image& b) {
        return a.rows == b.rows && a.cols == b.cols && std::memcmp(a.ptr<unsigned char>(), b.ptr<unsigned char>(), 3 * a.total()) == 0;
    }
    template <class F>
    static bool throws(F&& f, const char* word) {
        try { f(); } catch (const std::runtime_error& e) { return std::string(e.what()).find(word) != std::string::npos; }
        return false;
    }
    int main(int argc, char** argv) {   // in out mode mask0 mask1 mask2
        const nle::Image im = nle::imread(argv[1]);
        REQUIRE(!im.empty() && im.depth() == nle::NLE_8U && im.channels() == 3);
        std::vector<nle::Image> strokes;
        for (int m = 0; m < 3; ++m) {
            const nle::Image mask = nle::imread(argv[4 + m]);
            REQUIRE(!mask.empty());
            nle::Image s(mask.rows, mask.cols, nle::NLE_8U, 1);
            for (size_t i = 0; i < mask.total(); ++i) s.ptr<unsigned char>()[i] = mask.ptr<unsigned char>()[i * mask.channels()];
            strokes.push_back(s);
        }
        nle::NLEFilter f;
        f.verbose = false;
        f.keepTrainPlane = std::string(argv[3]) == "one";
        f.trainForEnhancement(im, 6, 8, 30, 30, 10, 8);
        nle::LocalEdit bg;                       // the rows of the command line in the test
        bg.weights = {3, 3, 1, 0.9};
        bg.detail.residualWeight = 1, bg.detail.gain = 2.5, bg.detail.sigma = 6;
        bg.shadows = 0.3, bg.saturation = 1.25;
        std::vector<nle::LocalEdit> edits(3, bg);
        edits[0].weights = {2, 2, 1, 1}, edits[0].detail.gain = 0.5, edits[0].shadows = 0.8, edits[0].saturation = 0;
        edits[1].weights.clear();                // empty: the background's
        edits[1].detail = nle::DetailOptions(), edits[1].highlights = -0.6;
        edits[2].shadows = 0, edits[2].saturation = 2.5;
        if (std::string(argv[3]) == "group") {   // trained over a device group: refused by name
            REQUIRE(throws([&] { f.enhanceLocal(im, strokes, edits, bg, 3, 0.1); }, "Local adjustments run on one device"));
            REQUIRE(throws([&] { f.enhanceSegmentsLocal(im, bg, edits); }, "Local adjustments run on one device"));
            std::printf("group OK\n");
            return 0;
        }
        const nle::Image out = f.enhanceLocal(im, strokes, edits, bg, 3, 0.1);
        REQUIRE(nle::imwrite(argv[2], out) && !same(out, f.enhance(im, bg.weights)));
        REQUIRE(same(f.enhanceLocal(im, strokes, edits, bg, 3, 0.1), out));
        // refusals in the style of the neighbours
        REQUIRE(throws([&] { f.enhanceLocal(im, {}, {}, bg); }, "1 to 8 strokes"));
        REQUIRE(throws([&] { f.enhanceLocal(im, strokes, {bg}, bg); }, "one edit per stroke"));
        nle::LocalEdit bad = bg;
        bad.weights = {1, 2};
        REQUIRE(throws([&] { f.enhanceLocal(im, strokes, {bg, bad, bg}, bg); }, "Row 2 of the local adjustment has 2 weights"));
        bad = bg, bad.saturation = 4.5;
        REQUIRE(throws([&] { f.enhanceLocal(im, strokes, {bg, bg, bad}, bg); }, "saturation"));
        bad = bg, bad.shadows = 1.5;
        REQUIRE(throws([&] { f.enhanceLocal(im, strokes, {bad, bg, bg}, bg); }, "shadows"));
        bad = bg, bad.detail.gain = 3.5;
        REQUIRE(throws([&] { f.enhanceLocal(im, strokes, {bad, bg, bg}, bg); }, "gain"));
        bad = bg, bad.weights.assign(17, 1.0);
        REQUIRE(throws([&] { f.enhanceLocal(im, strokes, {bad, bad, bad}, bad); }, "1 to 16 weights"));
        nle::Image hdr(im.rows, im.cols, nle::NLE_32F, 3);
        REQUIRE(throws([&] { f.enhanceLocal(hdr, strokes, edits, bg); }, "enhanceLocal"));
        REQUIRE(throws([&] { f.enhanceSegmentsLocal(im, bg, edits); }, "needs a segment()"));
        nle::SegmentOptions so;
        so.count = 3;
        f.segment(so);
        REQUIRE(throws([&] { f.enhanceSegmentsLocal(im, bg, std::vector<nle::LocalEdit>(4, bg)); }, "at most one edit per segment"));
        const nle::Image seg = f.enhanceSegmentsLocal(im, bg, {bg, edits[0]});       // segment 2 is missing: the background's
        REQUIRE(same(seg, f.enhanceSegmentsLocal(im, bg, {bg, edits[0], bg})) && !same(seg, out));
        REQUIRE(nle::imwrite((std::string(argv[2]) + ".seg.png").c_str(), seg));
        REQUIRE(same(f.enhanceLocal(im, strokes, edits, bg, 3, 0.1), out));
        std::printf("local OK\n");
        return 0;
    }
""")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("localdrv")
    host, libdir = os.path.join(PKG_DIR, "host"), os.path.join(PKG_DIR, "lib")
    (d / "drv.cpp").write_text(DRIVER)
    b = subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(d / "drv.cpp"),
                        *[os.path.join(host, s) for s in ("filter.cpp", "stages.cpp", "colour.cpp", "device_group.cpp", "image_io.cpp", "jpeg.cpp")],
                        "-L", libdir, "-lnle_hip", "-Wl,-rpath," + libdir, "-o", str(d / "drv")],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    return str(d / "drv")


@pytest.fixture(scope="module")
def bmp_and_masks(tmp_path_factory):
    from PIL import Image
    d = tmp_path_factory.mktemp("local8")
    path = d / "in.bmp"
    Image.fromarray(np.ascontiguousarray(colour_scene()[..., ::-1])).save(path)
    return path, write_masks(d, block_strokes())


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_cpp_surface_equals_the_cli(driver, bmp_and_masks, tmp_path):
    bmp, masks = bmp_and_masks
    env = {k: v for k, v in os.environ.items() if k != "NLE_DEVICES"}
    r = subprocess.run([driver, str(bmp), str(tmp_path / "drv.png"), "one"] + masks, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "local OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    lead = list(CLI_BG)
    for m in range(3):
        lead += ["--local", masks[m] + ":" + CLI_SPECS[m]]
    run_cli(lead + ["--region-spread", "3", "--region-floor", "0.1"], bmp, tmp_path / "cli.png", W4)
    assert np.array_equal(read_rgb8(tmp_path / "drv.png"), read_rgb8(tmp_path / "cli.png"))
    run_cli(["--segments", "3"] + CLI_BG + ["--local", "@1:" + CLI_SPECS[0]], bmp, tmp_path / "cliseg.png", W4)
    assert np.array_equal(read_rgb8(str(tmp_path / "drv.png") + ".seg.png"), read_rgb8(tmp_path / "cliseg.png"))


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_a_group_trained_filter_is_refused(driver, bmp_and_masks, tmp_path):
    """NLE_DEVICES with the same device twice forms a group: the train shards the image, the local edits throw"""
    bmp, masks = bmp_and_masks
    r = subprocess.run([driver, str(bmp), str(tmp_path / "drv.png"), "group"] + masks, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, NLE_DEVICES="0,0"))
    assert r.returncode == 0 and "group OK" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
