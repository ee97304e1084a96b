#!/usr/bin/env python3
"""Cost of the residual-greedy sampler (nle_ctx_set_sampler(NLE_SAMPLER_RESIDUAL), csrc/sampler.hip) beside the
farthest-point sampler at the same shapes.

Wall time around nle_sample_pixels (it returns after the list is on the host) on the synthetic plane, hx = W / 4, hy = 30:
the residual sampler at 512^2 with p = 200, 4096^2 with p = 200 and 2048^2 with p = 400; the farthest sampler at the same
shapes and at 8192^2 with p = 900 (its working set, the plane and m, lies beyond the Infinity Cache there, as the residual
sampler's factor always does).  Per child process: one warm-up call, then the median of --reps calls, the two samplers
alternating shape by shape; then the median and max - min over --runs fresh child processes, each under its own time limit
(the first failing child ends the run).

Algorithmic bytes: residual sum_k (8 k + 44) N over the p rounds (per pixel 8 k of the factor read, 8 written, 16 for d, 16
for m, 4 of the plane; every round counted as a residual round, so after a fallback the figure overstates the traffic: see
n_residual); farthest 20 N per round.

    python tools/residual_sampler_timing.py            # writes profiles/r14_residual_sampler_timing.json
    python tools/residual_sampler_timing.py --child --only 4096 --kind residual --reps 1   # one shape (for rocprofv3)
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

HBM_PEAK = 8.0e12
OUT = os.path.join(ROOT, "profiles", "r14_residual_sampler_timing.json")
# H, W, nRow, nCol, which samplers
SHAPES = [(512, 512, 10, 20, ("residual", "farthest")), (4096, 4096, 20, 10, ("residual", "farthest")),
          (2048, 2048, 20, 20, ("residual", "farthest")), (8192, 8192, 30, 30, ("farthest",))]


def algorithmic_bytes(kind, N, p):
    return sum((8 * k + 44) * N for k in range(p)) if kind == "residual" else 20 * N * p


def child(a):
    import torch
    nle = entry.load_package()
    synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
    ctx = nle.Context(0)
    rows = []
    for H, W, nr, nc, kinds in SHAPES:
        if a.only and a.only != H:
            continue
        x = torch.as_tensor(synth.synthetic_luminance(H, W).astype(np.float32), device="cuda:0")
        for kind in kinds:
            if a.kind and a.kind != kind:
                continue
            ctx.set_sampler(nle.SAMPLER_RESIDUAL if kind == "residual" else nle.SAMPLER_FARTHEST)
            sel = ctx.sample_pixels(x, nr, nc, W / 4, 30.0)  # warm: workspace cache, code objects
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                ctx.sample_pixels(x, nr, nc, W / 4, 30.0)
                ms.append((time.perf_counter() - t0) * 1e3)
            row = dict(kind=kind, H=H, W=W, p=int(sel.size), ms=float(np.median(ms)))
            if kind == "residual" and not a.only:
                row["n_residual"] = int(ctx.sample_pixels_order(x, nr, nc, W / 4, 30.0)["n_residual"])
            rows.append(row)
        ctx.set_sampler(nle.SAMPLER_GRID)
        del x
    ctx.close()
    print("CHILD " + json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help="measure in this process and print one CHILD line")
    ap.add_argument("--only", type=int, default=0, help="just this size (512, 2048, 4096 or 8192)")
    ap.add_argument("--kind", default="", choices=["", "residual", "farthest"])
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds per child process")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.child:
        return child(a)
    import torch
    per_run = []
    for i in range(a.runs):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
        if r.returncode != 0 or not line:
            print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
            raise SystemExit("child %d failed (status %d): stopping" % (i, r.returncode))
        per_run.append(json.loads(line[-1][6:]))
        print("run", i, line[-1][6:], flush=True)
    rows = []
    for j, first in enumerate(per_run[0]):
        ms = [run[j]["ms"] for run in per_run]
        N, p = first["H"] * first["W"], first["p"]
        nbytes = algorithmic_bytes(first["kind"], N, p)
        med = float(np.median(ms))
        row = dict(first, ms=round(med, 3), ms_runs=[round(v, 3) for v in ms], spread_ms=round(max(ms) - min(ms), 3),
                   algorithmic_bytes=nbytes, TBps=round(nbytes / (med * 1e-3) / 1e12, 3),
                   hbm_fraction=round(nbytes / (med * 1e-3) / HBM_PEAK, 3))
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "hbm_peak_TBps": HBM_PEAK / 1e12,
           "method": "wall time of nle_sample_pixels, median of %d after a warm-up per child, median and max - min of %d fresh "
                     "child processes; the two samplers alternate shape by shape inside a child" % (a.reps, a.runs),
           "sampler": rows}
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
