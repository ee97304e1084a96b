#!/usr/bin/env python3
"""Cost of the tone-mapping wrapper (nle_hdr_range / nle_hdr_to_loglum / nle_loglum_to_bgr16) beside
the deep-colour one (nle_bgr16_to_lab / nle_lab_to_bgr16) on one MI355X -> profiles/r23_tonemap_timing.json.

    kernels   KERNEL time of k_hdr_range (and its one-block second stage), k_hdr_to_loglum (both outputs), k_loglum_to_bgr16
              (saturation 1 and 0.6: the second takes three fp64 pow per pixel), k_bgr16_to_lab (all four outputs) and
              k_lab_to_bgr16, at 4096^2 and 512^2.  One child process per size under `rocprofv3 --kernel-trace` (a run of
              its own; nothing else is traced): the calls alternate `--reps` times after a warm-up round, and each kernel's
              figure is the median of its dispatches' End - Start in the trace.  `hbm_fraction` = the bytes the kernel must
              move (range 12 in; forward 12 in + 8 out; inverse 16 in + 6 out; deep: 6 in + 16 out, 12 in + 6 out) over that
              time, against the 8 TB/s HBM peak.
    gate      against the deep-colour kernels of the same run, never against the new code itself: k_hdr_to_loglum at most
              1.25 x k_bgr16_to_lab, k_loglum_to_bgr16 (saturation 1) at most 1.5 x k_lab_to_bgr16, k_hdr_range (both
              stages) at most k_bgr16_to_lab, at 4096^2.  The verdicts are recorded, nothing is loosened if one misses.
    calls     the same entry points as a caller sees them, untraced, in this process: host clock around one call (output
              allocation, the launches, one stream synchronise; the range call also a 16-byte download).  Recorded beside the
              kernel times, not in their place.
    tonemap   cfg4's arguments, device resident: deep = bgr16_to_lab + train on the guide + apply on the unrounded L +
              lab_to_bgr16; tonemap = hdr_range + hdr_to_loglum + train on the guide + apply on the unrounded x +
              loglum_to_bgr16.  Median wall time of `--runs` runs, each ending in a synchronise.

    python tools/tonemap_timing.py [--out FILE]
    python tools/tonemap_timing.py --child SIDE      # what one traced child runs
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
OUT = os.path.join(ROOT, "profiles", "r23_tonemap_timing.json")
BYTES = {"hdr_range": 12, "hdr_range_final": 0, "hdr_to_loglum": 12 + 8, "loglum_to_bgr16": 16 + 6, "loglum_to_bgr16_sat": 16 + 6,
         "bgr16_to_lab": 6 + 16, "lab_to_bgr16": 12 + 6}
# trace name -> (key of the first, key of the second dispatch per round) -- the inverse runs twice per round
KERNELS = {"k_hdr_range": ("hdr_range",), "k_hdr_range_final": ("hdr_range_final",), "k_hdr_to_loglum": ("hdr_to_loglum",),
           "k_loglum_to_bgr16": ("loglum_to_bgr16", "loglum_to_bgr16_sat"), "k_bgr16_to_lab": ("bgr16_to_lab",),
           "k_lab_to_bgr16": ("lab_to_bgr16",)}
SIDES = (4096, 512)
CHILD_TIMEOUT = 240
GATES = {"hdr_to_loglum": ("bgr16_to_lab", 1.25), "loglum_to_bgr16": ("lab_to_bgr16", 1.5), "hdr_range_both_stages": ("bgr16_to_lab", 1.0)}


def source(side):
    """an image-like HDR plane: smooth gradients over twelve stops, a tint that varies, +-10 % noise; float32 BGR"""
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:side, 0:side].astype(np.float32)
    level = np.exp2(-12.0 * x / side + 1.5 * np.sin(y / 97.0)) * (1.0 + 0.1 * rng.uniform(-1, 1, (side, side)).astype(np.float32))
    tint = np.stack([0.6 + 0.4 * y / side, 0.8 + 0.0 * x, 1.0 - 0.3 * x / side], axis=2)
    return (tint * level[..., None]).astype(np.float32)


def calls_of(ctx, side):
    import torch
    hdr = torch.from_numpy(source(side)).to("cuda:0")
    l_hi, rng = ctx.hdr_range(hdr)
    x, _ = ctx.hdr_to_loglum(hdr, l_hi, rng)
    bgr16 = ctx.loglum_to_bgr16(x, hdr, l_hi, rng, 1.0)          # an image for the deep kernels: the identity tone map
    L, A, B, _ = ctx.bgr16_to_lab(bgr16)
    calls = {"hdr_range": lambda: ctx.hdr_range(hdr), "bgr16_to_lab": lambda: ctx.bgr16_to_lab(bgr16),
             "hdr_to_loglum": lambda: ctx.hdr_to_loglum(hdr, l_hi, rng), "lab_to_bgr16": lambda: ctx.lab_to_bgr16(L, A, B),
             "loglum_to_bgr16": lambda: ctx.loglum_to_bgr16(x, hdr, l_hi, rng, 0.4),
             "loglum_to_bgr16_sat": lambda: ctx.loglum_to_bgr16(x, hdr, l_hi, rng, 0.4, 0.6)}
    for fn in calls.values():   # warm-up round
        fn()
    torch.cuda.synchronize()
    return calls


def child(side, reps):
    """the traced program: the set-up conversions and a warm-up round, then `reps` rounds of the calls"""
    import __graft_entry__ as entry
    nle = entry.load_package()
    ctx = nle.Context(0)
    calls = calls_of(ctx, side)
    for _ in range(reps):
        for fn in calls.values():
            fn()
    ctx.close()


def traced(side, reps):
    """key -> the durations (ns) of its dispatches in the last `reps` rounds of a kernel trace of one child"""
    d = tempfile.mkdtemp(prefix="tonemap_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--child", str(side), "--reps", str(reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=tempfile.gettempdir())
        if r.returncode != 0:
            raise RuntimeError(f"traced child {side} failed ({r.returncode}): {r.stderr[-1500:]}")
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
            ns = [e - s for s, e, n in rows if kname + "(" in n or n.endswith(kname)]
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
    ap.add_argument("--child", metavar="SIDE")
    a = ap.parse_args()
    if a.child:
        return child(int(a.child), a.reps)
    rec = {"reps": a.reps, "runs": a.runs, "kernels": {}, "calls": {}, "tonemap": {}}
    # ---- kernel times: one traced child per size, before this process opens the device
    for side in SIDES:
        ns = traced(side, a.reps)
        n = side * side
        row = {}
        for k, v in ns.items():
            s = statistics.median(v) * 1e-9
            row[k] = {"kernel_ms": s * 1e3, "min_ms": min(v) * 1e-6, "max_ms": max(v) * 1e-6, "bytes_per_pixel": BYTES[k],
                      "hbm_fraction": BYTES[k] * n / s / HBM_PEAK}
        row["hdr_range_both_stages"] = {"kernel_ms": row["hdr_range"]["kernel_ms"] + row["hdr_range_final"]["kernel_ms"]}
        rec["kernels"][f"{side}x{side}"] = row
        print(f"kernels {side}^2:", {k: round(v["kernel_ms"], 4) for k, v in row.items()}, flush=True)
    big = rec["kernels"]["4096x4096"]
    rec["gate"] = {"of": "kernel times at 4096^2, medians of traced dispatches, against the deep-colour kernels of the same run"}
    for new, (old, limit) in GATES.items():
        r = big[new]["kernel_ms"] / big[old]["kernel_ms"]
        rec["gate"][new] = {"against": old, "limit": limit, "ratio": r, "met": bool(r <= limit)}
    print("gate:", rec["gate"], flush=True)

    import __graft_entry__ as entry
    import torch
    nle = entry.load_package()
    synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
    ctx = nle.Context(0)
    rec["device"] = torch.cuda.get_device_name(0)
    # ---- whole calls, as a caller sees them (not kernel times)
    for side in SIDES:
        calls = calls_of(ctx, side)
        times = {k: [] for k in calls}
        for _ in range(a.reps):
            for k, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                times[k].append(time.perf_counter() - t0)
        rec["calls"][f"{side}x{side}"] = {k: {"ms_per_call": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3} for k, ts in times.items()}
        print(f"calls {side}^2:", {k: round(v["ms_per_call"], 4) for k, v in rec["calls"][f"{side}x{side}"].items()}, flush=True)

    # ---- train + tone map at cfg4's arguments, beside the deep path on the same plane
    cfg = dict(synth.CONFIGS["cfg4"])
    H, W = cfg["H"], cfg["W"]
    lum = synth.synthetic_luminance(H, W)      # levels 0..255: the deep input is its grey, the HDR input 2^((lum - 255) 12 / 255),
    g8 = np.clip(np.rint(lum), 0, 255).astype(np.uint8)      # twelve stops, so that both paths train on this plane's levels
    bgr16 = torch.from_numpy(np.repeat((g8.astype(np.uint16) * 257)[..., None], 3, axis=2)).to("cuda:0")
    hdr = torch.from_numpy(np.repeat(np.exp2((g8.astype(np.float64) - 255.0) * 12.0 / 255.0).astype(np.float32)[..., None], 3, axis=2)).to("cuda:0")
    weights = [2.0, 2.0, 1.0, 0.4]
    f = nle.NLEFilter(ctx)

    def deep():
        L, A, B, G = ctx.bgr16_to_lab(bgr16)
        f.train_filter(G, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], cfg["T"], cfg["K"])
        y = f.apply(L, nle.transform_eigenvalues(f.eigvals, weights))
        return ctx.lab_to_bgr16(y.reshape(L.shape), A, B)

    def tonemap():
        l_hi, rng = ctx.hdr_range(hdr)
        x, g = ctx.hdr_to_loglum(hdr, l_hi, rng)
        f.train_filter(g, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], cfg["T"], cfg["K"])
        y = f.apply(x, nle.transform_eigenvalues(f.eigvals, weights))
        return ctx.loglum_to_bgr16(y, hdr, l_hi, rng, weights[-1])
    for fn in (deep, tonemap):
        fn()
        torch.cuda.synchronize()
    times = {"deep": [], "tonemap": []}
    for _ in range(a.runs):
        for name, fn in (("deep", deep), ("tonemap", tonemap)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    for name, ts in times.items():
        rec["tonemap"][name] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}
    rec["tonemap"]["formulation"] = f.diag()["formulation"]
    rec["tonemap"]["tonemap_minus_deep_ms"] = rec["tonemap"]["tonemap"]["median_ms"] - rec["tonemap"]["deep"]["median_ms"]
    print("tonemap cfg4:", rec["tonemap"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    f.close()
    ctx.close()


if __name__ == "__main__":
    main()
