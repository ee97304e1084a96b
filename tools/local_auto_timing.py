#!/usr/bin/env python3
"""Cost of the per-region histograms (nle_region_histograms / nle_apply_local_auto) on one MI355X ->
profiles/r31_local_auto.json.

    kernels   KERNEL time at 4096^2, L = 4, M in {1, 4, 8}: k_region_hist with every row on and with one row on (row 1), on
              memberships in bands (one region owns a pixel, the rest are 0) and on memberships that overlap everywhere (every
              q in [0.1, 1]), over a U(0, 255) base layer and over a flat one (all weight of a row in one counter: the worst
              case for atomics on one address); beside them k_plane_hist on the same two planes and k_local_combine with
              every curve off on the band memberships.  One child process under `rocprofv3 --kernel-trace` (a run of its own;
              nothing else is traced); `--reps` rounds after a warm-up round; each figure is the median of its dispatches'
              End - Start in the trace.  `hbm_fraction` is the bytes the kernel has to read (4 (M + 1) per pixel for the
              region histogram, 4 for the plane histogram, 4 (L + M + 1) + 4 for the combine) over that time against the
              8 TB/s HBM peak.
    enhance   cfg4's arguments, device resident, four band strokes, every detail curve on: train + apply_local (the rows'
              curves from their two slopes) against train + apply_local_auto (levels = 1 and equalise = 0.5 on every row),
              alternating; median wall time of `--runs` runs, host clock around a synchronise.

    python tools/local_auto_timing.py [--out FILE]
    python tools/local_auto_timing.py --child      # what the traced child runs
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
OUT = os.path.join(ROOT, "profiles", "r31_local_auto.json")
SIDE, L, MS = 4096, 4, (1, 4, 8)
CHILD_TIMEOUT = 400
WEIGHTS, W_RHO, GAIN, SIGMA, FLOOR = [3.0, 3.0, 1.0, 1.0], 3.0, 2.5, 6.0, 0.05
HIST_KEYS = tuple(f"{rows}_{mem}_{base}" for rows in ("all", "one") for mem in ("bands", "overlap") for base in ("uniform", "flat"))


def keys_of():
    """trace name -> the keys of its dispatches within one round, in order"""
    return {"k_plane_hist": ["plane_uniform", "plane_flat"], "k_local_combine": [f"local_off_bands_M{M}" for M in MS],
            "k_region_hist": [f"hist_{k}_M{M}" for M in MS for k in HIST_KEYS]}


def bytes_of(key):
    if key.startswith("plane"):
        return 4
    M = int(key.rsplit("_M", 1)[1])
    return 4 * (L + M + 1) + 4 if key.startswith("local") else 4 * (M + 1)


def planes(n):
    """layers and a plane of the kind the filter makes: detail layers N(0, 3 | 6 | 10), a base U(0, 255), rho ~ N(0, 2)"""
    import torch
    g = torch.Generator(device="cuda:0").manual_seed(7)
    Y = torch.empty((L, n), device="cuda:0")
    for l, s in enumerate((3.0, 6.0, 10.0)):
        Y[l].normal_(0, s, generator=g)
    Y[L - 1].uniform_(0, 255, generator=g)
    x = Y.sum(dim=0) + torch.empty(n, device="cuda:0").normal_(0, 2, generator=g)
    return x, Y


def member_planes(n, M, overlap):
    import torch
    if overlap:
        g = torch.Generator(device="cuda:0").manual_seed(11 + M)
        return torch.empty((M, n), device="cuda:0").uniform_(0.1, 1.0, generator=g)
    owner = (torch.arange(n, device="cuda:0") * M) // n
    return (owner[None, :] == torch.arange(M, device="cuda:0")[:, None]).to(torch.float32)


def rows_of(nle, M, on):
    W = np.tile(WEIGHTS, (M + 1, 1)) * (1.0 + 0.05 * np.arange(M + 1))[:, None]
    detail = np.tile([W_RHO, GAIN if on else 1.0, SIGMA if on else 0.0], (M + 1, 1))
    curves = [nle.tone_curve(None, 0.8 - 0.15 * m, -0.3) for m in range(M + 1)] if on else None
    return W, detail, curves


def calls_of(nle, ctx):
    import torch
    n = SIDE * SIDE
    x, Y = planes(n)
    base = {"uniform": Y[L - 1], "flat": torch.full((n,), 100.0, device="cuda:0")}
    out = torch.empty(n, device="cuda:0")
    calls = [(f"plane_{b}", lambda b=b: ctx.plane_histogram(base[b], 1.0)) for b in ("uniform", "flat")]
    for M in MS:
        q = {"bands": member_planes(n, M, False), "overlap": member_planes(n, M, True)}
        W_off, d_off, _ = rows_of(nle, M, False)
        calls.append((f"local_off_bands_M{M}", lambda q=q, W=W_off, d=d_off: ctx.local_combine(x, Y, q["bands"], W, d, None, FLOOR,
                                                                                              nle.REGION_OUT_F32, out=out)))
        scale = W_off[:, L - 1]
        for rows in ("all", "one"):
            on = None if rows == "all" else [m == 1 for m in range(M + 1)]
            for mem in ("bands", "overlap"):
                for b in ("uniform", "flat"):
                    calls.append((f"hist_{rows}_{mem}_{b}_M{M}", lambda q=q, on=on, mem=mem, b=b, scale=scale:
                                  ctx.region_histograms(base[b], q[mem], scale, on, FLOOR)))
    for _, fn in calls:     # warm-up round
        fn()
    torch.cuda.synchronize()
    return calls


def child(reps):
    """the traced program: a warm-up round, then `reps` rounds of the calls"""
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
    d = tempfile.mkdtemp(prefix="local_auto_trace_")
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
        for kname, keys in keys_of().items():
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
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.reps)
    rec = {"counters": "32-bit LDS counters for the rows that are on, one launch, 32768 pixels per workgroup (the only layout built)",
           "reps": a.reps, "runs": a.runs, "side": SIDE, "layers": L, "regions": list(MS), "kernels": {}, "enhance": {}}
    # ---- kernel times: one traced child, before this process opens the device
    ns = traced(a.reps)
    n = SIDE * SIDE
    for k, v in ns.items():
        s = statistics.median(v) * 1e-9
        rec["kernels"][k] = {"kernel_ms": s * 1e3, "min_ms": min(v) * 1e-6, "max_ms": max(v) * 1e-6, "bytes_per_pixel": bytes_of(k),
                             "hbm_fraction": bytes_of(k) * n / s / HBM_PEAK}
    print("kernels:", {k: (round(v["kernel_ms"], 4), round(v["hbm_fraction"], 3)) for k, v in rec["kernels"].items()}, flush=True)

    import __graft_entry__ as entry
    import torch
    nle = entry.load_package()
    synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
    ctx = nle.Context(0)
    rec["device"] = torch.cuda.get_device_name(0)
    # ---- train + enhance at cfg4's arguments: four local rows with everything on, without and with the rows' own histograms
    cfg = dict(synth.CONFIGS["cfg4"])
    H, Wd = cfg["H"], cfg["W"]
    lum = torch.from_numpy(synth.synthetic_luminance(H, Wd).astype(np.float32)).to("cuda:0")
    M = 4
    strokes = member_planes(H * Wd, M, False).reshape(M, H, Wd)
    W, detail, curves = rows_of(nle, M, True)
    tone = [(0.8 - 0.15 * m, -0.3, 1.0, 0.5) for m in range(M + 1)]
    f = nle.NLEFilter(ctx)

    def train():
        f.train_filter(lum, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], cfg["T"], cfg["K"])

    def local():
        train()
        return f.apply_local(lum, L, strokes, W, detail, curves, [float(M)] * M, 4.0, FLOOR, nle.REGION_OUT_ROUNDED8)

    def local_auto():
        train()
        return f.apply_local_auto(lum, L, strokes, W, tone, detail, [float(M)] * M, 4.0, FLOOR, nle.REGION_OUT_ROUNDED8)
    fns = (("local", local), ("local_auto", local_auto))
    for _, fn in fns:
        fn()
        torch.cuda.synchronize()
    times = {name: [] for name, _ in fns}
    for _ in range(a.runs):
        for name, fn in fns:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    for name, ts in times.items():
        rec["enhance"][name] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}
    rec["enhance"]["config"] = "cfg4"
    rec["enhance"]["auto_minus_local_ms"] = rec["enhance"]["local_auto"]["median_ms"] - rec["enhance"]["local"]["median_ms"]
    print("enhance cfg4:", rec["enhance"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    f.close()
    ctx.close()


if __name__ == "__main__":
    main()
