#!/usr/bin/env python3
"""The Nystrom residual of the README pairs beside their measured distance from the exact filter ->
profiles/r12_nystrom_residual.json.  A record, not a gate.

    python tools/nystrom_residual_report.py [--only NAME]

For every pair of tests/readme_pairs.py at its own arguments (nRow, nCol, hx, hy): the L channel of the input (PIL decode, the
fixed-point 8-bit Lab of nle_bgr2lab8) and nle_nystrom_residual (NLE_RESID_AUTO) with the grid and with the farthest sampler:
mean r, max r and its pixel, the share of pixels with r > 0.5.  Beside them the first detail layer's relative L2 against the
exact filter that profiles/r6_exact_vs_nystrom.txt records for the same pair and sampler (tools/exact_quality.py), and the
Spearman rank correlation of mean r with that error over the pairs: per sampler and over both together; and in how many
pairs the sampler with the smaller mean r is also the one closer to the exact filter.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "r12_nystrom_residual.json")
EXACT = os.path.join(ROOT, "profiles", "r6_exact_vs_nystrom.txt")


def recorded_errors():
    """{name: {"grid": first detail layer's rel L2 vs exact, "farthest": ...}} from profiles/r6_exact_vs_nystrom.txt"""
    out = {}
    for line in open(EXACT):
        if line.startswith("#") or "|" not in line:
            continue
        head, grid, far = [s.strip() for s in line.split("|")[:3]]
        out[head.split()[0]] = {"grid": float(grid.split()[0]), "farthest": float(far.split()[0])}
    return out


def ranks(v):
    order = np.argsort(np.asarray(v, dtype=np.float64), kind="stable")
    r = np.empty(len(v))
    r[order] = np.arange(len(v))
    return r


def spearman(a, b):
    ra, rb = ranks(a), ranks(b)
    return float(np.corrcoef(ra, rb)[0, 1])


def summarise_within(pairs, have):
    agree = [n for n in have if (pairs[n]["grid"]["mean_r"] < pairs[n]["farthest"]["mean_r"]) ==
             (pairs[n]["grid"]["layer1_rel_l2_vs_exact"] < pairs[n]["farthest"]["layer1_rel_l2_vs_exact"])]
    return "%d of %d" % (len(agree), len(have))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    from PIL import Image
    import readme_pairs as rp
    import __graft_entry__ as entry
    nle = entry.load_package()
    errs = recorded_errors()
    ctx = nle.Context(0)
    pairs = {}
    for name, src, _, nr, nc, hx, hy, T, K, w in rp.PAIRS:
        if a.only and name != a.only:
            continue
        bgr = np.asarray(Image.open(os.path.join(rp.GOLDEN, src)).convert("RGB"))[..., ::-1].copy()
        _, L = ctx.bgr2lab8(bgr)
        H, W = L.shape
        rec = dict(H=H, W=W, n_row=nr, n_col=nc, hx=hx, hy=hy)
        for kind in ("grid", "farthest"):
            ctx.set_sampler(nle.SAMPLER_FARTHEST if kind == "farthest" else nle.SAMPLER_GRID)
            _, s = ctx.nystrom_residual(L, nr, nc, hx, hy, want_map=False)
            rec[kind] = dict(mean_r=s["sum"] / (H * W), max_r=s["max"], argmax=list(divmod(s["argmax"], W)),
                             share_above_half=s["count"] / (H * W),
                             layer1_rel_l2_vs_exact=errs.get(name, {}).get(kind))
        ctx.set_sampler(nle.SAMPLER_GRID)
        pairs[name] = rec
        print(name, json.dumps(rec), flush=True)
    ctx.close()
    out = {"what": "nle_nystrom_residual of the README pairs at their own arguments beside the first detail layer's relative L2 "
                   "against the exact filter (profiles/r6_exact_vs_nystrom.txt)", "pairs": pairs}
    have = [n for n in pairs if pairs[n]["grid"]["layer1_rel_l2_vs_exact"] is not None]
    if len(have) >= 3:
        cols = {k: ([pairs[n][k]["mean_r"] for n in have], [pairs[n][k]["layer1_rel_l2_vs_exact"] for n in have])
                for k in ("grid", "farthest")}
        out["spearman_mean_r_vs_layer1_error"] = {
            "pairs": len(have), "grid": spearman(*cols["grid"]), "farthest": spearman(*cols["farthest"]),
            "both": spearman(cols["grid"][0] + cols["farthest"][0], cols["grid"][1] + cols["farthest"][1])}
        # within a pair: does the sampler with the smaller mean r also have the smaller error?
        out["pairs_where_the_sampler_with_smaller_mean_r_has_the_smaller_error"] = summarise_within(pairs, have)
        print(json.dumps(out["spearman_mean_r_vs_layer1_error"]), out["pairs_where_the_sampler_with_smaller_mean_r_has_the_smaller_error"])
    if not a.only:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
