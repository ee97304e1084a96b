"""The fp64 stage kernels of csrc/generic64.hip, each ALONE against numpy on the same fp64 inputs: k_tsgemm64
(nle_ts_gemm64), k_row_scalings64 (nle_row_scalings64), k_gram64d + k_gram64d_reduce (nle_gram64), k_rowpass64<NCL>
(nle_sinkhorn_scalings64) -- the kernels every formulation auto mode can select runs on.

Data.  Strictly positive entries, (|N(0,1)| + 0.1) / sqrt(width): every dot product then has condition number 1
(sum |x_i y_i| == |sum x_i y_i|), so a dropped or doubled term is an O(1/k) RELATIVE error of the entry it belongs to
and no reference quantity is small enough to be left out of a comparison.

Tolerances are derived, not measured.  A k-term fp64 dot product, in any summation order, with or without fma, obeys
    |computed - exact| <= g(k) * sum_i |x_i| |y_i|,      g(k) = k u / (1 - k u),  u = 2^-53
(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  The reference product is formed in np.longdouble
(x87 extended: 64-bit significand, its own error 2^-11 of the bound), and every assertion is ELEMENTWISE:
    ts_gemm64        |C - A B|   <= g(kd + 2) (|A| |B|);  the columns nc .. nle_ld(nc) of C exactly zero
    row_scalings64   |out - 1/s| <= g(r + 3) / s,  s = X u          (r-term dot, one division, positive data)
    gram64           |G - Z^T Z| <= g(M + 2 r + 12) (|Z|^T |Z|),  Z = diag(c) X with c from the longdouble reference: the
                     device's own c_i carries up to g(r + 3) relative error and enters squared (the 2 r); G == G^T exactly;
                     h_u == NULL (c = 1): g(M + 2)
    sinkhorn_scalings64   errors compound over 2T passes, so no closed bound: the project's figure for this stage, relative
                     L2 <= 1e-10 on u_c and u_r (the tolerance of the reference's unit tests, and what the fp32 kernel's test
                     asserts), against the loop of test_sinkhorn_gram_rowscale_kernels run in longdouble
The comparison helpers are plain functions of (result, inputs); test_checkers_* (no GPU) feed them numpy's own float64
results, which must pass, and the mutations a wrong tile / chunk / tail would produce, each of which must fail.

Leading dimension.  include/nle.h promises "any value >= the logical width" for the fp64 entry points: every case runs
twice, padding columns zero and padding columns NaN, and the two results must be identical bit for bit.
"""
import numpy as np
import pytest

if np.finfo(np.longdouble).nmant < 63:
    pytest.skip("np.longdouble has no 64-bit significand on this platform: the high-precision reference these tests "
                "compare against cannot be formed", allow_module_level=True)

LD = np.longdouble
U = 2.0 ** -53
SINKHORN_TOL = 1e-10
EPS = 1e-10   # NLE_EPS, include/filter.hpp:14


def g(k):
    return k * U / (1.0 - k * U)


def nle_ld(n):
    return (n + 3) & ~3


# ------------------------------------------------------------------ inputs
def positive(rng, M, width):
    return (np.abs(rng.standard_normal((M, width))) + 0.1) / np.sqrt(width)


def padded(X, ld, pad):
    """X (M x width) inside an M x ld buffer whose other columns hold `pad` (0.0 or NaN)"""
    M, width = X.shape
    out = np.full((M, ld), pad, dtype=np.float64)
    out[:, :width] = X
    return out


def ld_of(kind, width):
    return {"r": width, "ld4": nle_ld(width), "r+1": width + 1, "r+37": width + 37}[kind]


# ------------------------------------------------------------------ references (longdouble) and checkers
def recip_ld(s):
    out = np.zeros_like(s)
    m = np.abs(s) >= EPS
    out[m] = 1 / s[m]
    return out


def check_ts_gemm(C, A, B):
    """C: M x nle_ld(nc) result for A (M x kd) B (kd x nc)"""
    C, A, B = np.asarray(C), np.asarray(A), np.asarray(B)
    (M, kd), nc = A.shape, B.shape[1]
    assert C.shape == (M, nle_ld(nc)), (C.shape, M, nc)
    assert np.all(C[:, nc:] == 0), "padding columns of the output must be exactly zero"
    assert np.isfinite(C).all()
    ref = A.astype(LD) @ B.astype(LD)
    mag = np.abs(A).astype(LD) @ np.abs(B).astype(LD)
    err = np.abs(C[:, :nc].astype(LD) - ref)
    bad = err > g(kd + 2) * mag
    assert not bad.any(), (f"{int(bad.sum())} entries beyond g({kd + 2}) |A||B|; first at {np.argwhere(bad)[0].tolist()}, "
                           f"max err/bound {float((err / (g(kd + 2) * mag)).max()):.3g}")


def check_row_scalings(out, X, u):
    out, X, u = np.asarray(out), np.asarray(X), np.asarray(u)
    M, r = X.shape
    assert out.shape == (M,) and np.isfinite(out).all()
    s = X.astype(LD) @ u.astype(LD)
    assert (s > EPS).all(), "test data must be positive"
    err = np.abs(out.astype(LD) - 1 / s)
    bad = err > g(r + 3) / s
    assert not bad.any(), (f"{int(bad.sum())} rows beyond g({r + 3}) / s; first {int(np.argwhere(bad)[0][0])}, "
                           f"max err/bound {float((err * s / g(r + 3)).max()):.3g}")


def check_gram(G, X, u):
    """G: r x r result for sum_i c_i^2 x_i x_i^T, c = recip(X u) (u None: 1)"""
    G, X = np.asarray(G), np.asarray(X)
    M, r = X.shape
    assert G.shape == (r, r) and np.isfinite(G).all()
    assert np.array_equal(G, G.T), "G must be exactly symmetric"
    Xl = X.astype(LD)
    if u is None:
        Z, k = Xl, M + 2
    else:
        Z, k = Xl * recip_ld(Xl @ np.asarray(u).astype(LD))[:, None], M + 2 * r + 12
    ref = Z.T @ Z
    mag = np.abs(Z).T @ np.abs(Z)
    err = np.abs(G.astype(LD) - ref)
    bad = err > g(k) * mag
    assert not bad.any(), (f"{int(bad.sum())} entries beyond g({k}) |Z|^T|Z|; first at {np.argwhere(bad)[0].tolist()}, "
                           f"max err/bound {float((err / (g(k) * mag)).max()):.3g}")


def sinkhorn_reference(X, lam, T):
    """u_c = lam o X^T r_{T-1}, u_r = lam o X^T c_T (src/filter.cpp:238-245), in longdouble"""
    P, lam = np.asarray(X).astype(LD), np.asarray(lam).astype(LD)
    rv = np.ones(P.shape[0], dtype=LD)
    for _ in range(T):
        uc = lam * (P.T @ rv)
        c = recip_ld(P @ uc)
        ur = lam * (P.T @ c)
        rv = recip_ld(P @ ur)
    return uc, ur


def check_sinkhorn(uc, ur, X, lam, T):
    """returns the two measured relative L2 errors (for the record); asserts both <= 1e-10"""
    uc, ur = np.asarray(uc), np.asarray(ur)
    r = np.asarray(X).shape[1]
    assert uc.shape == (r,) and ur.shape == (r,)
    assert np.isfinite(uc).all() and np.isfinite(ur).all(), "non-finite scalings"
    uc_ref, ur_ref = sinkhorn_reference(X, lam, T)
    ec = float(np.linalg.norm(uc.astype(LD) - uc_ref) / np.linalg.norm(uc_ref))
    er = float(np.linalg.norm(ur.astype(LD) - ur_ref) / np.linalg.norm(ur_ref))
    assert ec <= SINKHORN_TOL and er <= SINKHORN_TOL, (ec, er)
    return ec, er


# ------------------------------------------------------------------ checker self-test (CPU): the bounds have teeth
def _rejects(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return True
    return False


def _c_pad(Cm, nc):
    out = np.zeros((Cm.shape[0], nle_ld(nc)))
    out[:, :nc] = Cm
    return out


@pytest.mark.parametrize("M,kd,nc", [(40, 33, 33), (257, 5, 35), (1000, 200, 50), (33, 1, 32)])
def test_checkers_ts_gemm(M, kd, nc):
    rng = np.random.default_rng(M + kd + nc)
    A, B = positive(rng, M, kd), positive(rng, kd, nc)
    good = _c_pad(A @ B, nc)
    check_ts_gemm(good, A, B)                                  # numpy's own float64 product passes
    # one k-term dropped, in one entry and in all of them
    k = kd // 2
    m = good.copy()
    m[M // 2, nc // 2] -= A[M // 2, k] * B[k, nc // 2]
    assert _rejects(check_ts_gemm, m, A, B)
    m = good.copy()
    m[:, :nc] -= np.outer(A[:, k], B[k])
    assert _rejects(check_ts_gemm, m, A, B)
    # one term doubled
    m = good.copy()
    m[0, 0] += A[0, kd - 1] * B[kd - 1, 0]
    assert _rejects(check_ts_gemm, m, A, B)
    # one 16 x 16 output tile transposed; one tile taken from its mirror position (tile (0, 1) <- tile (1, 0))
    m = good.copy()
    m[16:32, 0:16] = good[16:32, 0:16].T
    assert _rejects(check_ts_gemm, m, A, B)
    m = good.copy()
    m[0:16, 16:32] = good[16:32, 0:16]
    assert _rejects(check_ts_gemm, m, A, B)
    # the last (partial) row tile not written; the tail k-step (kd % 4 terms) not summed
    m = good.copy()
    m[(M - 1) // 16 * 16:] = 0.0
    assert _rejects(check_ts_gemm, m, A, B)
    if kd % 4 and kd > 4:
        t = kd // 4 * 4
        assert _rejects(check_ts_gemm, _c_pad(A[:, :t] @ B[:t], nc), A, B)
    # one padding column of the output non-zero
    if nle_ld(nc) > nc:
        m = good.copy()
        m[M // 3, nc] = 1e-300
        assert _rejects(check_ts_gemm, m, A, B)
    # a NaN anywhere
    m = good.copy()
    m[M - 1, nc - 1] = np.nan
    assert _rejects(check_ts_gemm, m, A, B)


@pytest.mark.parametrize("M,r", [(40, 33), (1000, 17), (600, 130), (257, 1)])
def test_checkers_gram(M, r):
    rng = np.random.default_rng(M * 7 + r)
    X = positive(rng, M, r)
    u = rng.uniform(0.5, 2.0, r)
    c = 1.0 / (X @ u)
    Z = X * c[:, None]
    for uu, ZZ in ((u, Z), (None, X)):
        good = ZZ.T @ ZZ
        good = np.triu(good) + np.triu(good, 1).T              # exactly symmetric, as the device's mirror makes it
        check_gram(good, X, uu)                                # numpy's own float64 product passes
        m = good - np.outer(ZZ[M // 2], ZZ[M // 2])            # one k-term (row) dropped
        assert _rejects(check_gram, m, X, uu)
        rows = max(((M + 255) // 256 + 3) // 4 * 4, 256)       # the last row chunk omitted (gram64d_chunk_rows)
        last = (M - 1) // rows * rows
        assert _rejects(check_gram, good - ZZ[last:].T @ ZZ[last:], X, uu)
        assert _rejects(check_gram, good - ZZ[M - M % 4:].T @ ZZ[M - M % 4:], X, uu) or M % 4 == 0   # the short last k-step
        if r > 32:
            m = good.copy()                                    # one off-diagonal tile transposed (symmetry kept)
            m[0:16, 16:32] = good[0:16, 16:32].T
            m[16:32, 0:16] = m[0:16, 16:32].T
            assert _rejects(check_gram, m, X, uu)
            m = good.copy()                                    # a lower tile not mirrored: taken from its own position
            m[16:32, 0:16] = good[0:16, 16:32]
            assert _rejects(check_gram, m, X, uu)
            m = good.copy()                                    # a tile taken from another tile pair's slot
            m[0:16, 16:32] = good[0:16, 0:16]
            m[16:32, 0:16] = m[0:16, 16:32].T
            assert _rejects(check_gram, m, X, uu)
        m = good.copy()                                        # asymmetric by one ulp
        if r > 1:
            m[0, r - 1] = np.nextafter(m[0, r - 1], np.inf)
            assert _rejects(check_gram, m, X, uu)
    # c_i taken without the square
    assert _rejects(check_gram, (X * np.sqrt(c)[:, None]).T @ (X * np.sqrt(c)[:, None]), X, u)


@pytest.mark.parametrize("M,r", [(40, 33), (1000, 65), (5, 1), (300, 2048)])
def test_checkers_row_scalings_and_sinkhorn(M, r):
    rng = np.random.default_rng(M * 3 + r)
    X = positive(rng, M, r)
    u = rng.uniform(0.5, 2.0, r)
    good = 1.0 / (X @ u)
    check_row_scalings(good, X, u)
    if r > 1:
        assert _rejects(check_row_scalings, 1.0 / (X[:, :-1] @ u[:-1]), X, u)          # last column dropped
        assert _rejects(check_row_scalings, 1.0 / (X[:, 1:] @ u[1:]), X, u)            # first column dropped
    m = good.copy()
    m[M - 1] = 0.0                                                                     # last row not written
    assert _rejects(check_row_scalings, m, X, u)
    m = good.copy()
    m[M // 2] = np.inf
    assert _rejects(check_row_scalings, m, X, u)
    lam = np.sort(rng.uniform(0.5, 2.0, r))[::-1].copy()
    for T in (1, 4):
        # the same loop in numpy float64 passes
        rv = np.ones(M)
        for _ in range(T):
            uc = lam * (X.T @ rv)
            c = 1.0 / (X @ uc)
            ur = lam * (X.T @ c)
            rv = 1.0 / (X @ ur)
        ec, er = check_sinkhorn(uc, ur, X, lam, T)
        assert ec < 1e-13 and er < 1e-13
        # the last row left out of every pass; one iteration too many; NaN scalings
        if M > 1:
            uc2, ur2 = (np.asarray(v, dtype=np.float64) for v in sinkhorn_reference(X[:-1], lam, T))
            assert _rejects(check_sinkhorn, uc2, ur2, X, lam, T)
        if T == 1 and r > 1:   # (it contracts fast: a fifth iteration moves the scalings by less than the tolerance)
            uc3, ur3 = (np.asarray(v, dtype=np.float64) for v in sinkhorn_reference(X, lam, 2))
            assert _rejects(check_sinkhorn, uc3, ur3, X, lam, T)
        assert _rejects(check_sinkhorn, np.full(r, np.nan), ur, X, lam, T)
        assert _rejects(check_sinkhorn, ur, uc, X, lam, T)                             # the two swapped


# ------------------------------------------------------------------ case lists (from the switches in generic64.hip)
WIDTHS = [1, 3, 4, 5, 15, 16, 17, 31, 33]               # around the 16-wide MFMA tile and the k-step of 4
ROWS = [1, 2, 3, 4, 5, 15, 16, 17, 255, 256, 257, 1000, 4099]   # 1000: four Gram chunks, the last short, not a multiple of 4
LD_KINDS = ["r", "ld4", "r+1", "r+37"]
BIG_ROWS = 70001                                         # above 65536: gram64d_chunk_rows leaves 256


def _pairwise():
    """every (width, leading-dimension kind) pair, the row counts cycling through ROWS against them"""
    out = []
    for wi, w in enumerate(WIDTHS):
        for ki, kind in enumerate(LD_KINDS):
            i = wi * len(LD_KINDS) + ki
            out.append((ROWS[(i * 5 + wi) % len(ROWS)], w, kind))
    return out


STAGE_CASES = _pairwise() + [
    (BIG_ROWS, 33, "r+1"), (4099, 33, "ld4"), (1000, 33, "r"), (1000, 17, "r"), (257, 16, "ld4"), (4099, 1, "r"),
    (300, 8, 2304),                                       # a narrow block of a wide matrix
]
# every k_rowpass64<NCL> instantiation and its neighbours: logical widths at the switch points (with and without
# padding), and a narrow logical width inside a row stride at the switch points
ROWPASS_CASES = (
    [(257, r, kind) for r, kind in [(64, "r"), (65, "r+1"), (128, "ld4"), (129, "r"), (256, "r+37"), (257, "ld4"),
                                    (512, "r"), (513, "r+1"), (1024, "ld4"), (1025, "r"), (2047, "r+1")]]
    + [(100, 2048, "r"), (33, 2048, "r+37")]              # r = 2048 is the documented maximum
    + [(1000, 33, ldx) for ldx in (64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048)]
)


def _ld(kind, width):
    return kind if isinstance(kind, int) else ld_of(kind, width)


def _ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


def _both_paddings(M, width, kind, seed):
    """the same matrix with zero and with NaN padding columns, on the device; the logical block on the host"""
    import torch
    rng = np.random.default_rng(seed)
    X = positive(rng, M, width)
    ldx = _ld(kind, width)
    pads = [0.0] if ldx == width else [0.0, np.nan]
    return X, [torch.as_tensor(padded(X, ldx, p), device="cuda") for p in pads], rng


# ------------------------------------------------------------------ GPU: each kernel alone against longdouble numpy
def _gemm_cases():
    out = []
    for i, (M, kd, kind) in enumerate(_pairwise()):
        out.append((M, kd, WIDTHS[(i * 2 + 3) % len(WIDTHS)], kind, 0))
    out += [(BIG_ROWS, 33, 33, "r+1", 0), (4099, 200, 50, "ld4", 0), (300, 7, 260, "r", 0), (129, 300, 33, "r+37", 0),
            (1000, 17, 1, "ld4", 0), (257, 1, 33, "r+1", 0), (16, 16, 16, "r", 0), (17, 17, 17, "ld4", 0),
            (300, 8, 5, 2304, 0),
            # a row sub-block, d_A + q * lda (host/stages.cpp: sinkhorn's Wab from the rows below the samples)
            (257, 33, 31, "ld4", 37), (1000, 16, 15, "r+1", 16), (4099, 5, 33, "r", 4098), (256, 31, 3, "r+37", 1)]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("M,kd,nc,kind,q", _gemm_cases(), ids=_ids(_gemm_cases()))
def test_ts_gemm64_matches_longdouble(nle, ctx, M, kd, nc, kind, q):
    X, devs, rng = _both_paddings(M, kd, kind, 1000 * kd + nc + M)
    B = positive(rng, kd, nc)
    outs = [ctx.ts_gemm64(d[q:], kd, B).cpu().numpy() for d in devs]
    check_ts_gemm(outs[0], X[q:], B)
    for o in outs[1:]:
        assert np.array_equal(o, outs[0]), "NaN in the padding columns of A changed the product"


@pytest.mark.gpu
@pytest.mark.parametrize("M,r,kind", STAGE_CASES + ROWPASS_CASES[::3], ids=_ids(STAGE_CASES + ROWPASS_CASES[::3]))
def test_row_scalings64_matches_longdouble(nle, ctx, M, r, kind):
    X, devs, rng = _both_paddings(M, r, kind, 77 * r + M)
    u = rng.uniform(0.5, 2.0, r)
    outs = [ctx.row_scalings64(d, r, u).cpu().numpy() for d in devs]
    check_row_scalings(outs[0], X, u)
    for o in outs[1:]:
        assert np.array_equal(o, outs[0]), "NaN in the padding columns changed the scalings"


@pytest.mark.gpu
def test_row_scalings64_reciprocal_zeroing(nle, oracle, ctx):
    """inplaceReciprocal (src/filter.cpp:42-54): |s| < 1e-10 -> 0, never Inf; bit for bit against the oracle (every
    sum below is exact in fp64, and 1 / s is one correctly rounded division on both sides)"""
    import torch
    rows = np.array([[1, 2], [0, 0], [3, -3], [1e-6, 0], [2.0 ** -34, 0], [-2.0 ** -34, 0], [2.0 ** -33, 0], [-2.0 ** -33, 0],
                     [0, -0.0], [2.0 ** -1000, 2.0 ** -1000], [-4, 1]], dtype=np.float64)
    u = np.array([1.0, 1.0])
    ref, _ = oracle.inplace_reciprocal(rows @ u)
    assert ref[1] == 0 and ref[2] == 0 and ref[4] == 0 and ref[5] == 0 and ref[6] != 0 and ref[7] != 0   # 2^-34 < 1e-10 < 2^-33
    for ldx, pad in ((2, 0.0), (4, 0.0), (3, np.nan), (39, np.nan)):
        out = ctx.row_scalings64(torch.as_tensor(padded(rows, ldx, pad), device="cuda"), 2, u).cpu().numpy()
        assert np.array_equal(out, ref), (ldx, out, ref)
        assert np.isfinite(out).all()


_GRAM_CASES = STAGE_CASES + [(1000, 129, "r+1"), (257, 260, "ld4"), (17, 513, "r"), (BIG_ROWS, 17, "ld4")]


@pytest.mark.gpu
@pytest.mark.parametrize("M,r,kind", _GRAM_CASES, ids=_ids(_GRAM_CASES))
def test_gram64_matches_longdouble(nle, ctx, M, r, kind):
    X, devs, rng = _both_paddings(M, r, kind, 31 * r + M)
    u = rng.uniform(0.5, 2.0, r)
    for uu in (u, None):
        outs = [ctx.gram64(d, r, uu) for d in devs]
        check_gram(outs[0], X, uu)
        for o in outs[1:]:
            assert np.array_equal(o, outs[0]), "NaN in the padding columns changed the Gram matrix"


_SINK_CASES = [(M, r, kind, (1, 4)[i % 2]) for i, (M, r, kind) in enumerate(STAGE_CASES + ROWPASS_CASES)]


@pytest.mark.gpu
@pytest.mark.parametrize("M,r,kind,T", _SINK_CASES, ids=_ids(_SINK_CASES))
def test_sinkhorn_scalings64_matches_longdouble(nle, ctx, M, r, kind, T):
    X, devs, rng = _both_paddings(M, r, kind, 13 * r + M + T)
    lam = np.sort(rng.uniform(0.5, 2.0, r))[::-1].copy()
    outs = [ctx.sinkhorn_scalings64(d, r, lam, T) for d in devs]
    ec, er = check_sinkhorn(outs[0][0], outs[0][1], X, lam, T)
    print(f"sinkhorn64 M={M} r={r} ld={_ld(kind, r)} T={T}: rel L2 u_c {ec:.2e} u_r {er:.2e} (tolerance {SINKHORN_TOL:.0e})")
    for uc, ur in outs[1:]:
        assert np.array_equal(uc, outs[0][0]) and np.array_equal(ur, outs[0][1]), \
            "NaN in the padding columns changed the Sinkhorn scalings"


@pytest.mark.gpu
def test_sinkhorn_scalings64_bounds_the_logical_width_not_the_stride(nle, ctx):
    """r <= 2048 is the limit (one lane holds 32 columns); the row stride is free"""
    import torch
    X = torch.zeros((4, 2304), dtype=torch.float64, device="cuda")
    with pytest.raises(nle.NLEError):
        ctx.sinkhorn_scalings64(X, 2049, np.ones(2049), 1)
    X[:, :8] = 0.25
    uc, ur = ctx.sinkhorn_scalings64(X, 8, np.ones(8), 1)
    check_sinkhorn(uc, ur, X[:, :8].cpu().numpy(), np.ones(8), 1)
    # a status, not a fault, on the arguments the header rules out
    with pytest.raises(nle.NLEError):
        ctx.sinkhorn_scalings64(X, 8, np.ones(8), 0)
