#!/usr/bin/env python3
"""Quality of the residual-greedy sampler (NLE_SAMPLER_RESIDUAL) beside the grid and the farthest-point sampler: CPU, fp64
numpy, the oracle's 1e-10 cut.  No GPU: the three sample sets come from the numpy restatements of the rules
(tests/test_sampler.py: farthest; tests/test_residual_sampler.py: residual_greedy), every later stage is the oracle's.

1. The README planes at their own arguments and sample count: the Nystrom residual r = 1 - k^T pinv(K_A) k (pinv at the
   cut) on 20 000 probe pixels (seed 0): max r and mean r; and K_A's smallest kept eigenvalue, or its rank where the cut
   drops some.
2. 60 x 90 crops with a 6 x 9 budget against the EXACT dense filter (the full K, Sinkhorn on it, its top-K eigenpairs; T and
   K of the pair, K <= 30, L = 4, hx / 10 for the crops other than flower): relative L2 error of detail layer 1, and cond2
   of K_A.

    python tools/residual_sampler_quality.py            # writes profiles/r14_residual_sampler_quality.txt
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "r14_residual_sampler_quality.txt")
EPS = 1e-10
KINDS = ("grid", "farthest", "residual")
# name, pair, crop (None: the centre 60 x 90), hx of the crop
CROPS = [("flower [100:160, 150:240]", "flower", (100, 160, 150, 240), 100.0),
         ("flower [40:100, 60:150]", "flower", (40, 100, 60, 150), 100.0),
         ("red-cherries centre", "red-cherries", None, 40.0),
         ("brickwall centre", "brickwall", None, 100.0),
         ("bird centre", "bird", None, 100.0)]


def sets(oracle, tsa, trs, y, nr, nc, hx, hy):
    H, W = y.shape
    grid = oracle.sample_pixels(H, W, nr, nc)[0]
    p = grid.size
    order, _, n_residual, _ = trs.residual_greedy(y, p, hx, hy)
    return {"grid": np.sort(grid), "farthest": tsa.farthest(y, p, hx, hy), "residual": np.sort(order)}, p, n_residual


def affinity(y, rows, cols, hx, hy):
    """K(rows, cols) of plane y, the rule's operation order"""
    W = y.shape[1]
    f = np.asarray(y, dtype=np.float32).astype(np.float64).ravel()
    dr = (rows // W)[:, None] - (cols // W)[None, :]
    dc = (rows % W)[:, None] - (cols % W)[None, :]
    dy = f[rows][:, None] - f[cols][None, :]
    return np.exp(-(1.0 / (hx * hx)) * (dr * dr + dc * dc).astype(np.float64) - (1.0 / (hy * hy)) * (dy * dy))


def spectrum(y, S, hx, hy):
    lam, V = np.linalg.eigh(affinity(y, S, S, hx, hy))
    lam, V = lam[::-1], V[:, ::-1]
    kept = int(np.argmax(lam < EPS)) if np.any(lam < EPS) else lam.size  # the leading run of eigenvalues >= the cut
    return lam[:kept], V[:, :kept]


def full_plane_row(oracle, tsa, trs, name, y, nr, nc, hx, hy):
    S, p, n_residual = sets(oracle, tsa, trs, y, nr, nc, hx, hy)
    probe = np.sort(np.random.default_rng(0).choice(y.size, size=min(20000, y.size), replace=False))
    cells = []
    for kind in KINDS:
        lam, V = spectrum(y, S[kind], hx, hy)
        B = affinity(y, probe, S[kind], hx, hy) @ V
        r = 1.0 - (B * B / lam[None, :]).sum(1)
        r[np.isin(probe, S[kind])] = 0.0
        cells.append((r.max(), r.mean(), ("%.1e" % lam[-1]) if lam.size == p else "rank %d" % lam.size))
    return ("%-14s %4d %5d | " % (name, p, n_residual) + " / ".join("%.2e" % c[0] for c in cells) + " | " +
            " / ".join("%.1e" % c[1] for c in cells) + " | " + " / ".join(c[2] for c in cells))


def crop_row(oracle, tsa, trs, monkey, name, y, hx, hy, T, K):
    nr, nc, L = 6, 9, 4
    H, W = y.shape
    S, p, n_residual = sets(oracle, tsa, trs, y, nr, nc, hx, hy)
    ex = tsa._exact_layers(oracle, y, hx, hy, T, K, L)
    errs, conds = [], []
    for kind in KINDS:
        rest = np.setdiff1d(np.arange(H * W), S[kind])
        monkey(lambda *a, s=S[kind], r=rest: (s, r))
        V_o, S_o = oracle.train_filter(y, nr, nc, hx, hy, T, K)
        Y = oracle.apply_layers(V_o, S_o, y, L).reshape(L, -1)
        errs.append(float(np.linalg.norm(Y[0] - ex[0]) / np.linalg.norm(ex[0])))
        lam = np.linalg.eigvalsh(affinity(y, S[kind], S[kind], hx, hy))
        conds.append(lam[-1] / lam[0])
    monkey(None)  # the oracle's own grid again
    return ("%-28s %3d | " % (name, n_residual) + " / ".join("%.4f" % e for e in errs) + " | " +
            " / ".join("%.0e" % c for c in conds))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--only", default="", help="just the pairs whose name contains this")
    a = ap.parse_args()
    from PIL import Image
    import readme_pairs as rp
    import test_residual_sampler as trs
    import test_sampler as tsa
    oracle = entry.load_oracle()
    planes = {}
    for pr in rp.PAIRS:
        bgr = np.asarray(Image.open(rp.paths(pr)[0]).convert("RGB"))[..., ::-1].copy()
        planes[pr[0]] = (oracle.bgr_to_lab8(bgr)[..., 0].astype(np.float64), pr)
    lines = [__doc__.split("\n\n")[0].replace("\n", " "), "",
             "1. README planes, own arguments, 20 000 probe pixels, K_A at the 1e-10 cut (grid / farthest / residual)", "",
             "pair              p n_res | max r                          | mean r                    | lambda_min kept, or rank"]
    print("\n".join(lines), flush=True)
    for name, (y, pr) in planes.items():
        if a.only and a.only not in name:
            continue
        t0 = time.time()
        lines.append(full_plane_row(oracle, tsa, trs, name, y, pr[3], pr[4], pr[5], pr[6]))
        print(lines[-1], "  (%.0f s)" % (time.time() - t0), flush=True)
    head = ["", "2. 60 x 90 crops, 6 x 9 budget, against the exact dense filter, detail layer 1 (grid / farthest / residual)", "",
            "crop                       n_res | layer-1 error              | cond2 K_A"]
    lines += head
    print("\n".join(head), flush=True)
    real = oracle.sample_pixels

    def monkey(fn):
        oracle.sample_pixels = fn if fn else real

    try:
        for name, pair, box, hx in CROPS:
            if a.only and a.only not in pair:
                continue
            y, pr = planes[pair]
            H, W = y.shape
            r0, r1, c0, c1 = box if box else (H // 2 - 30, H // 2 + 30, W // 2 - 45, W // 2 + 45)
            lines.append(crop_row(oracle, tsa, trs, monkey, name, y[r0:r1, c0:c1].copy(), hx, pr[6], pr[7], min(pr[8], 30)))
            print(lines[-1], flush=True)
    finally:
        oracle.sample_pixels = real
    if not a.only:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        print("wrote", a.out)


if __name__ == "__main__":
    main()
