"""k_gemm64s (csrc/generic64.hip) alone, through nle_gemm64s, at the edges of its tiles and of its operand windows.

    C(i,j) = dl[i] (sum_k A(i,k) dk[k] B(k,j)) dr[j] + add(i,j)

Shapes.  kk in {1, 3, 4, 15, 16, 17, 52, 196, 200} (below, at and past one MFMA step of 4 k and one group of 16 k; the
products of the default workload) and, with w = nle_gemm64s_window(), kk = w, w + 1 and 2 w + 5 (one window exactly, a
second window of one k, a third window: the double-buffered loop's every branch); m, n in {1, 15, 16, 17, 50, 200}
(a fraction of a tile, a tile, a tile and one row, several workgroups).  Every (kk, m, n) runs with each of dl / dk / dr /
add present and absent (16 combinations).

Operand forms, the same in every case: A is stored transposed and addressed through its strides; B is a sub-block that
starts at row 3 of a wider buffer; C is row-major with a leading dimension of n + 5 whose padding, pre-filled with NaN,
must still be NaN afterwards; add is column-major with a padded leading dimension.

Bound (elementwise, as for every fp64 dot product of kk terms):  |C - ref| <= (kk + 2) 2^-53 (|dl| (|A| |dk| |B|) |dr|).
It is rigorous for these inputs: dl, dk and dr are signed powers of two, so the scalings round nothing and the MFMA
chain's kk fused multiply-adds are the only roundings of the product (<= kk u times the absolute sum, Higham section
3.1); |add| <= 0.9 times that absolute sum, so the rounding of the final addition is below 1.9 u times it.  A scaling left
out, applied to the wrong index or applied twice changes an entry by a factor of two or more.  The reference is numpy on
the same fp64 inputs, accumulated in np.longdouble where that is wider than fp64 (its own error is then 2^-11 of the
bound), formed once per kk for the 200 x 200 product; every smaller (m, n) is a leading sub-block of it.
"""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
MN = (1, 15, 16, 17, 50, 200)
NMAX = 200
KK_FIXED = (1, 3, 4, 15, 16, 17, 52, 196, 200)
KK_WINDOW = ("w", "w+1", "2w+5")
WIDE = np.longdouble if np.finfo(np.longdouble).nmant >= 63 else np.float64


def _pow2(rng, n):
    return np.ldexp(rng.choice([-1.0, 1.0], n), rng.integers(-3, 4, n))


def _case(kk, seed):
    """inputs, reference and absolute sum of the full 200 x 200 product with kk terms"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((NMAX, kk))
    B = rng.standard_normal((kk, NMAX))
    dl, dk, dr = _pow2(rng, NMAX), _pow2(rng, kk), _pow2(rng, NMAX)
    plain = (A.astype(WIDE) @ B.astype(WIDE))                       # dk absent
    scaled = ((A * dk).astype(WIDE) @ B.astype(WIDE))               # A dk is exact
    S_plain = np.abs(A) @ np.abs(B)
    S_scaled = (np.abs(A) * np.abs(dk)) @ np.abs(B)
    # |add| <= 0.9 x the smallest absolute sum any combination of scalings gives the entry
    smallest = np.minimum(S_plain, S_scaled) * np.minimum(1.0, np.abs(dl))[:, None] * np.minimum(1.0, np.abs(dr))[None, :]
    add = rng.uniform(-0.9, 0.9, (NMAX, NMAX)) * smallest
    return dict(A=A, B=B, dl=dl, dk=dk, dr=dr, add=add, plain=plain, scaled=scaled, S_plain=S_plain, S_scaled=S_scaled)


@pytest.mark.parametrize("kk_spec", KK_FIXED + KK_WINDOW)
def test_gemm64s_against_numpy(nle, ctx, kk_spec):
    import torch
    w = int(nle.lib().nle_gemm64s_window())
    assert w >= 16 and w % 16 == 0
    kk = {"w": w, "w+1": w + 1, "2w+5": 2 * w + 5}.get(kk_spec, kk_spec)
    c = _case(kk, seed=1000 + kk)
    dev = torch.device("cuda:0")
    lda, ldb, ldadd = NMAX + 3, NMAX + 5, NMAX + 7
    At = np.full((kk, lda), np.nan)                 # A(i, k) at k * lda + i
    At[:, :NMAX] = c["A"].T
    Bbuf = np.full((kk + 3, ldb), np.nan)           # B(k, j) at (k + 3) * ldb + j
    Bbuf[3:, :NMAX] = c["B"]
    addT = np.full((NMAX, ldadd), np.nan)           # add(i, j) at j * ldadd + i
    addT[:, :NMAX] = c["add"].T
    d_At, d_B, d_add = (torch.as_tensor(v, device=dev) for v in (At, Bbuf, addT))
    d_dl, d_dk, d_dr = (torch.as_tensor(c[k], device=dev) for k in ("dl", "dk", "dr"))
    worst = 0.0
    for m, n in itertools.product(MN, MN):
        for use_dl, use_dk, use_dr, use_add in itertools.product((False, True), repeat=4):
            ldc = n + 5
            d_C = torch.full((m, ldc), float("nan"), dtype=torch.float64, device=dev)
            ctx.gemm64s(m, n, kk, d_At, (1, lda), d_B[3:], (ldb, 1), d_C, (ldc, 1),
                        dl=d_dl if use_dl else None, dk=d_dk if use_dk else None, dr=d_dr if use_dr else None,
                        add=d_add if use_add else None, sadd=(1, ldadd) if use_add else (0, 0))
            C = d_C.cpu().numpy()
            what = (kk, m, n, use_dl, use_dk, use_dr, use_add)
            assert np.isnan(C[:, n:]).all(), ("padding of C written", what)
            ref = (c["scaled"] if use_dk else c["plain"])[:m, :n]
            S = (c["S_scaled"] if use_dk else c["S_plain"])[:m, :n].copy()
            if use_dl:
                ref = ref * c["dl"][:m, None].astype(WIDE)
                S *= np.abs(c["dl"][:m, None])
            if use_dr:
                ref = ref * c["dr"][None, :n].astype(WIDE)
                S *= np.abs(c["dr"][None, :n])
            if use_add:
                ref = ref + c["add"][:m, :n].astype(WIDE)
            err = np.abs((C[:, :n].astype(WIDE) - ref).astype(np.float64))
            bound = (kk + 2) * U * S
            assert np.isfinite(C[:, :n]).all(), what
            ratio = float((err / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (what, ratio, np.unravel_index(int((err / bound).argmax()), err.shape))
    print(f"gemm64s kk = {kk}: worst error / bound over {len(MN) ** 2 * 16} launches: {worst:.3f}")


def test_gemm64s_many_tiles_take_the_streaming_kernel(nle, ctx):
    """more than 1024 output tiles (one workgroup per CU) go to k_gemm64s_stream: 520 x 520 is 33 x 33 = 1089 tiles, its
    edge tiles 8 wide; kk = 52 and one window plus one; all four scalings on, operands strided as above"""
    import torch
    dev = torch.device("cuda:0")
    m = n = 520
    w = int(nle.lib().nle_gemm64s_window())
    for kk in (52, w + 1):
        rng = np.random.default_rng(kk)
        A, B = rng.standard_normal((m, kk)), rng.standard_normal((kk, n))
        dl, dk, dr = _pow2(rng, m), _pow2(rng, kk), _pow2(rng, n)
        S = np.abs(dl)[:, None] * ((np.abs(A) * np.abs(dk)) @ np.abs(B)) * np.abs(dr)[None, :]
        add = rng.uniform(-0.9, 0.9, (m, n)) * S
        ref = dl[:, None].astype(WIDE) * ((A * dk).astype(WIDE) @ B.astype(WIDE)) * dr[None, :].astype(WIDE) + add.astype(WIDE)
        d_At = torch.as_tensor(np.ascontiguousarray(A.T), device=dev)
        d_B, d_add = torch.as_tensor(B, device=dev), torch.as_tensor(np.ascontiguousarray(add.T), device=dev)
        d_C = torch.full((m, n + 5), float("nan"), dtype=torch.float64, device=dev)
        ctx.gemm64s(m, n, kk, d_At, (1, m), d_B, (n, 1), d_C, (n + 5, 1), dl=torch.as_tensor(dl, device=dev),
                    dk=torch.as_tensor(dk, device=dev), dr=torch.as_tensor(dr, device=dev), add=d_add, sadd=(1, m))
        C = d_C.cpu().numpy()
        assert np.isnan(C[:, n:]).all()
        err = np.abs((C[:, :n].astype(WIDE) - ref).astype(np.float64))
        assert (err <= (kk + 2) * U * S).all(), (kk, float((err / ((kk + 2) * U * S)).max()))


def test_gemm64s_in_place_add_and_empty_shapes(nle, ctx):
    """add == C with C's strides (the accumulate form the orthogonalisation uses), and m, n or kk of 0: nothing written
    for an empty C; kk = 0 leaves dl 0 dr + add"""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    m, n, kk = 50, 17, 52
    A, B, C0 = rng.standard_normal((m, kk)), rng.standard_normal((kk, n)), rng.standard_normal((m, n))
    d_A, d_B, d_C = (torch.as_tensor(v, device=dev) for v in (A, B, C0.copy()))
    ctx.gemm64s(m, n, kk, d_A, (kk, 1), d_B, (n, 1), d_C, (n, 1), add=d_C, sadd=(n, 1))
    err = np.abs(d_C.cpu().numpy() - (A.astype(WIDE) @ B.astype(WIDE) + C0).astype(np.float64))
    assert (err <= (kk + 2) * U * (np.abs(A) @ np.abs(B) + np.abs(C0))).all()
    d_C = torch.as_tensor(C0.copy(), device=dev)
    for mm, nn in ((0, n), (m, 0)):
        ctx.gemm64s(mm, nn, kk, d_A, (kk, 1), d_B, (n, 1), d_C, (n, 1))
        assert np.array_equal(d_C.cpu().numpy(), C0)
    ctx.gemm64s(m, n, 0, d_A, (kk, 1), d_B, (n, 1), d_C, (n, 1), add=d_C, sadd=(n, 1))
    assert np.array_equal(d_C.cpu().numpy(), C0)
