#!/usr/bin/env python3
"""Cost of the farthest-point sampler (nle_ctx_set_sampler(NLE_SAMPLER_FARTHEST), csrc/sampler.hip).

1. The sampler alone (nle_sample_pixels, wall time around the call, after a warm-up call) on the synthetic plane at
   512^2 and 4096^2 with p = 200 and at 8192^2 with p = 900: milliseconds, microseconds per round (one launch each),
   the bytes a round moves (per pixel 4 of the plane, 8 of m read, 8 of m written) and their fraction of 8 TB/s.
2. Train + apply (T and K of the pair, L = 4) with the farthest sampler against the grid, auto mode, on the README pairs
   (their L planes at the README arguments) and on cfg2.

    python tools/sampler_timing.py                     # writes profiles/r5_sampler_timing.json
    python tools/sampler_timing.py --only 4096 --reps 1 --no-write   # one 4096^2 sampler run (for rocprofv3)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402

HBM_PEAK = 8.0e12
OUT = os.path.join(ROOT, "profiles", "r5_sampler_timing.json")
SIZES = [(512, 512, 10, 20), (4096, 4096, 20, 10), (8192, 8192, 30, 30)]  # H, W, nRow, nCol: p = 200, 200, 900
FORMS = {0: "auto", 1: "materialised_f32", 2: "tables_f64", 3: "phi_free_exp", 4: "materialised_f64", 5: "streamed_f64"}


def time_sampler(nle, ctx, x, nr, nc, hx, hy, reps):
    import torch
    ctx.set_sampler(nle.SAMPLER_FARTHEST)
    ctx.sample_pixels(x, nr, nc, hx, hy)  # warm: workspace cache, code objects
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        sel = ctx.sample_pixels(x, nr, nc, hx, hy)  # returns after the list is on the host
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    ctx.set_sampler(nle.SAMPLER_GRID)
    return best, sel.size


def time_train(nle, ctx, lum8, nr, nc, hx, hy, T, K, sampler, reps):
    ctx.set_sampler(sampler)
    f = nle.NLEFilter(ctx)
    H, W = lum8.shape
    out = np.empty((4, H * W), dtype=np.float32)

    def once():
        f.train_filter_host_u8(lum8, nr, nc, hx, hy, T, K)
        f.apply_layers_host(None, 4, out)

    once()
    t0 = time.perf_counter()
    for _ in range(reps):
        once()
    ms = (time.perf_counter() - t0) * 1e3 / reps
    d = f.diag()
    f.close()
    ctx.set_sampler(nle.SAMPLER_GRID)
    return ms, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", type=int, default=0, help="just the sampler at this size (512, 4096 or 8192)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import torch
    nle = entry.load_package()
    synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
    ctx = nle.Context(0)
    out = {"device": torch.cuda.get_device_name(0), "hbm_peak_TBps": HBM_PEAK / 1e12,
           "sampler": [], "train_apply": []}
    for H, W, nr, nc in SIZES:
        if a.only and a.only != H:
            continue
        x = torch.as_tensor(synth.synthetic_luminance(H, W).astype(np.float32), device="cuda:0")
        ms, p = time_sampler(nle, ctx, x, nr, nc, W / 4, 30.0, a.reps)
        bytes_round = 20 * H * W
        us_round = ms * 1e3 / p
        row = dict(H=H, W=W, p=p, sampler_ms=round(ms, 3), us_per_round=round(us_round, 2), bytes_per_round=bytes_round,
                   hbm_fraction=round(bytes_round / (us_round * 1e-6) / HBM_PEAK, 3))
        out["sampler"].append(row)
        print("sampler", json.dumps(row), flush=True)
        del x
    if not a.only:
        import readme_pairs as rp
        from PIL import Image
        cases = []
        for pr in rp.PAIRS:
            path = rp.paths(pr)[0]
            bgr = np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"))[..., ::-1])
            lab, _ = ctx.bgr2lab8(bgr)
            cases.append((pr[0], lab[..., 0].cpu().numpy().copy(), pr[3], pr[4], pr[5], pr[6], pr[7], pr[8]))
        c2 = synth.CONFIGS["cfg2"]
        cases.append(("cfg2", synth.synthetic_luminance(c2["H"], c2["W"]).astype(np.uint8), c2["n_row"], c2["n_col"], c2["hx"],
                      c2["hy"], c2["T"], c2["K"]))
        for name, lum8, nr, nc, hx, hy, T, K in cases:
            row = dict(case=name, H=int(lum8.shape[0]), W=int(lum8.shape[1]), nRow=nr, nCol=nc, T=T, K=K)
            for tag, s in (("grid", nle.SAMPLER_GRID), ("farthest", nle.SAMPLER_FARTHEST)):
                ms, d = time_train(nle, ctx, lum8, nr, nc, hx, hy, T, K, s, a.reps)
                row[tag + "_ms"] = round(ms, 3)
                row[tag + "_form"] = FORMS.get(d["formulation"], d["formulation"])
            row["ratio"] = round(row["farthest_ms"] / row["grid_ms"], 2)
            out["train_apply"].append(row)
            print("train_apply", json.dumps(row), flush=True)
    ctx.close()
    if not a.no_write:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
