#!/usr/bin/env python3
"""How far the Nystrom filters are from the exact filter on the README pairs at full size -> profiles/r6_exact_vs_nystrom.txt.

    python tools/exact_quality.py [--only NAME]

For every pair of tests/readme_pairs.py at its own arguments (nRow, nCol, hx, hy, T, K, weights): the L channel of the
input (PIL decode, the fixed-point 8-bit Lab of nle_bgr2lab8), the filter trained three ways on the GPU -- grid Nystrom
(auto mode), farthest-point Nystrom (NLE_SAMPLER_FARTHEST) and exact (NLE_MODE_EXACT_F64) -- and per layer (L = number of
weights) the relative L2 of the Nystrom layers against the exact ones, plus the fraction of the 8-bit output L bytes
(apply_u8 with the README weights) that differ from the exact filter's.  The answer at full size to DESIGN.md section 3.6.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "r6_exact_vs_nystrom.txt")


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only")
    a = ap.parse_args()
    from PIL import Image
    import readme_pairs as rp
    import __graft_entry__ as entry
    nle = entry.load_package()
    ctx = nle.Context(0)
    lines = ["# tools/exact_quality.py on one MI355X: README pairs at full size and their own arguments",
             "# rel L2 of each Nystrom filter's layers against the exact filter (NLE_MODE_EXACT_F64), layer 0 first;",
             "# u8 diff = fraction of the 8-bit output L bytes (apply_u8, README weights) that differ from the exact filter's",
             "# name          H x W      K' exact  exact train s | grid: layers, u8 diff | farthest: layers, u8 diff"]
    for name, src, _, nr, nc, hx, hy, T, K, w in rp.PAIRS:
        if a.only and name != a.only:
            continue
        bgr = np.asarray(Image.open(os.path.join(rp.GOLDEN, src)).convert("RGB"))[..., ::-1].copy()
        lab, _ = ctx.bgr2lab8(bgr)
        x = lab[..., 0].cpu().numpy().astype(np.float32)
        H, W = x.shape
        wts = [float(v) for v in w]
        L = len(wts)
        out = {}
        for kind in ("exact", "grid", "farthest"):
            ctx.set_mode(nle.MODE_EXACT_F64 if kind == "exact" else nle.MODE_AUTO)
            ctx.set_sampler(nle.SAMPLER_FARTHEST if kind == "farthest" else nle.SAMPLER_GRID)
            t0 = time.time()
            f = nle.NLEFilter(ctx).train_filter(x, nr, nc, hx, hy, T, K)
            dt = time.time() - t0
            Y = f.apply_layers(x, L).cpu().numpy().astype(np.float64)
            u8 = f.apply_u8(x, nle.transform_eigenvalues(f.eigvals, wts)).cpu().numpy().ravel()
            out[kind] = (Y, u8, f.info()["K"], dt)
            f.close()
        ctx.set_mode(nle.MODE_AUTO)
        ctx.set_sampler(nle.SAMPLER_GRID)
        Ye, ue, Ke, te = out["exact"]
        row = f"{name:13s} {H:4d} x {W:4d}  {Ke:3d}  {te:8.1f} |"
        for kind in ("grid", "farthest"):
            Y, u8, _, _ = out[kind]
            row += " " + " ".join("%.3g" % rel(Y[j], Ye[j]) for j in range(L)) + ", %.4f |" % float(np.mean(u8 != ue))
        lines.append(row)
        print(row, flush=True)
    ctx.close()
    if not a.only:
        with open(OUT, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
