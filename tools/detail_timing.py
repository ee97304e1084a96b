#!/usr/bin/env python3
"""Cost of the out-of-span detail layer and the detail curve (nle_detail_combine / nle_apply_detail)
beside the region combine on one MI355X -> profiles/r24_detail_timing.json.

    kernels   KERNEL time of k_detail_combine with the curve off and with it on (gain 2.5, sigma 6) and of k_region_combine
              with M = 1, all at 4096^2, L = 4, F32 out.  One child process under `rocprofv3 --kernel-trace` (a run of its own;
              nothing else is traced): per round region, detail (curve off), region, detail (curve on), `--reps` rounds after
              a warm-up round; each figure is the median of its dispatches' End - Start in the trace.  Both kernels read
              L + 1 planes and write one (24 B per pixel); `hbm_fraction` is those bytes over that time against the 8 TB/s
              HBM peak.  `spread` is the second region dispatch of a round over the first: the same kernel on the same
              data, so what the shared host and the dispatch order alone do to a figure.
    gate      k_detail_combine at most 1.25 x k_region_combine (the first of each round) in the same run, with the curve off
              and with it on.  The verdicts are recorded, nothing is loosened if one misses.
    enhance   cfg4's arguments, device resident: train + apply_rounded8 (the plain enhance) and train + apply_detail with
              active options (w_rho 3, gain 2.5, sigma 6, ROUNDED8), alternating; median wall time of `--runs` runs, host
              clock around a synchronise.

    python tools/detail_timing.py [--out FILE]
    python tools/detail_timing.py --child      # what the traced child runs
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
OUT = os.path.join(ROOT, "profiles", "r24_detail_timing.json")
SIDE, L = 4096, 4
BYTES = 4 * (L + 1) + 4
# trace name -> the keys of its dispatches within one round, in order
KERNELS = {"k_region_combine": ("region", "region_again"), "k_detail_combine": ("detail_curve_off", "detail_curve_on")}
CHILD_TIMEOUT = 240
LIMIT = 1.25
WEIGHTS, W_RHO, GAIN, SIGMA = [3.0, 3.0, 1.0, 1.0], 3.0, 2.5, 6.0


def planes(n):
    """layers and a plane of the kind the filter makes: detail layers N(0, 3 | 6 | 10), a base U(0, 255), rho ~ N(0, 2)"""
    import torch
    g = torch.Generator(device="cuda:0").manual_seed(7)
    Y = torch.empty((L, n), device="cuda:0")
    for l, s in enumerate((3.0, 6.0, 10.0)):
        Y[l].normal_(0, s, generator=g)
    Y[L - 1].uniform_(0, 255, generator=g)
    x = Y.sum(dim=0) + torch.empty(n, device="cuda:0").normal_(0, 2, generator=g)
    q = torch.empty((1, n), device="cuda:0").uniform_(0, 2, generator=g)
    return x, Y, q


def calls_of(nle, ctx):
    import torch
    x, Y, q = planes(SIDE * SIDE)
    out = torch.empty(SIDE * SIDE, device="cuda:0")
    wt = np.array([WEIGHTS, [1.0, 2.0, 1.0, 1.0]])
    region = lambda: ctx.region_combine(Y, q, wt, 0.05, nle.REGION_OUT_F32, out=out)  # noqa: E731
    calls = [("region", region), ("detail_curve_off", lambda: ctx.detail_combine(x, Y, WEIGHTS, W_RHO, 1.0, 0.0, nle.REGION_OUT_F32, out=out)),
             ("region_again", region), ("detail_curve_on", lambda: ctx.detail_combine(x, Y, WEIGHTS, W_RHO, GAIN, SIGMA, nle.REGION_OUT_F32, out=out))]
    for _, fn in calls:     # warm-up round
        fn()
    torch.cuda.synchronize()
    return calls


def child(reps):
    """the traced program: a warm-up round, then `reps` rounds of the four calls"""
    import __graft_entry__ as entry
    nle = entry.load_package()
    ctx = nle.Context(0)
    calls = calls_of(nle, ctx)
    for _ in range(reps):
        for _, fn in calls:
            fn()
    ctx.close()


def traced(reps):
    """key -> the durations (ns) of its dispatches in the last `reps` rounds of a kernel trace of one child"""
    d = tempfile.mkdtemp(prefix="detail_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--child", "--reps", str(reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=tempfile.gettempdir())
        if r.returncode != 0:
            raise RuntimeError(f"traced child failed ({r.returncode}): {r.stderr[-1500:]}")
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError(f"no kernel trace written under {d}: {[p for p, _, _ in os.walk(d)]}")
        rows = []
        for f in files:
            with open(f) as fh:
                rows += [(int(x["Start_Timestamp"]), int(x["End_Timestamp"]), x["Kernel_Name"]) for x in csv.DictReader(fh)]
        rows.sort()
        out = {}
        for kname, keys in KERNELS.items():
            ns = [e - s for s, e, n in rows if kname + "<" in n or kname + "(" in n or n.endswith(kname)]
            if len(ns) < reps * len(keys):
                raise RuntimeError(f"{kname}: {len(ns)} dispatches in the trace, {reps * len(keys)} expected; names: "
                                   f"{sorted({n for _, _, n in rows})[:12]}")
            ns = ns[-reps * len(keys):]
            for j, key in enumerate(keys):
                out[key] = ns[j::len(keys)]
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.reps)
    rec = {"reps": a.reps, "runs": a.runs, "side": SIDE, "layers": L, "kernels": {}, "enhance": {}}
    # ---- kernel times: one traced child, before this process opens the device
    ns = traced(a.reps)
    n = SIDE * SIDE
    for k, v in ns.items():
        s = statistics.median(v) * 1e-9
        rec["kernels"][k] = {"kernel_ms": s * 1e3, "min_ms": min(v) * 1e-6, "max_ms": max(v) * 1e-6, "bytes_per_pixel": BYTES,
                             "hbm_fraction": BYTES * n / s / HBM_PEAK}
    ker = rec["kernels"]
    print("kernels:", {k: round(v["kernel_ms"], 4) for k, v in ker.items()}, flush=True)
    rec["spread"] = ker["region_again"]["kernel_ms"] / ker["region"]["kernel_ms"]
    rec["gate"] = {"of": "kernel times at 4096^2, L = 4, F32, medians of traced dispatches, against k_region_combine (M = 1) of the same run",
                   "limit": LIMIT}
    for key in ("detail_curve_off", "detail_curve_on"):
        r = ker[key]["kernel_ms"] / ker["region"]["kernel_ms"]
        rec["gate"][key] = {"ratio": r, "met": bool(r <= LIMIT)}
    print("spread:", rec["spread"], "gate:", rec["gate"], flush=True)

    import __graft_entry__ as entry
    import torch
    nle = entry.load_package()
    synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
    ctx = nle.Context(0)
    rec["device"] = torch.cuda.get_device_name(0)
    # ---- train + enhance at cfg4's arguments, with and without active options
    cfg = dict(synth.CONFIGS["cfg4"])
    lum = torch.from_numpy(synth.synthetic_luminance(cfg["H"], cfg["W"]).astype(np.float32)).to("cuda:0")
    f = nle.NLEFilter(ctx)

    def plain():
        f.train_filter(lum, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], cfg["T"], cfg["K"])
        return f.apply_rounded8(lum, nle.transform_eigenvalues(f.eigvals, WEIGHTS))

    def detail():
        f.train_filter(lum, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], cfg["T"], cfg["K"])
        return f.apply_detail(lum, WEIGHTS, W_RHO, GAIN, SIGMA, nle.REGION_OUT_ROUNDED8)
    for fn in (plain, detail):
        fn()
        torch.cuda.synchronize()
    times = {"plain": [], "detail": []}
    for _ in range(a.runs):
        for name, fn in (("plain", plain), ("detail", detail)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    for name, ts in times.items():
        rec["enhance"][name] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}
    rec["enhance"]["config"] = "cfg4"
    rec["enhance"]["formulation"] = f.diag()["formulation"]
    rec["enhance"]["detail_minus_plain_ms"] = rec["enhance"]["detail"]["median_ms"] - rec["enhance"]["plain"]["median_ms"]
    print("enhance cfg4:", rec["enhance"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    f.close()
    ctx.close()


if __name__ == "__main__":
    main()
