#!/usr/bin/env python3
"""Cost of the deep-colour wrapper (nle_bgr16_to_lab / nle_lab_to_bgr16) beside the 8-bit one
(nle_bgr2lab8 / nle_lab2bgr8) on one MI355X -> profiles/r22_deep_colour_timing.json.

    kernels   KERNEL time of k_bgr16_to_lab (all four outputs), k_lab_to_bgr16, k_bgr2lab8 (Lab image and L plane) and
              k_lab2bgr8 (L replaced), at 4096^2 and 512^2, on an image-like plane (smooth gradients plus noise) and on
              uniformly random codes (every table gather on a cache line of its own: the worst case of the L2-resident
              tables, which the 8-bit kernels' LDS tables do not have).  One child process per size and input under
              `rocprofv3 --kernel-trace` (a run of its own; nothing else is traced): the four calls alternate `--reps` times
              after a warm-up round, and each kernel's figure is the median of its dispatches' End - Start in the trace.
              `hbm_fraction` = the bytes the kernel must move (deep: 6 in + 16 out, 12 in + 6 out; 8 bit: 3 in + 7 out,
              7 in + 3 out) over that time, against the 8 TB/s HBM peak.
    gate      the deep pair may take at most 3 x the 8-bit pair's summed kernel time at 4096^2 (2 x for the bytes, 1.5 x for
              three fp64 cube roots and the threshold search); the verdict is recorded for both inputs, nothing is loosened if
              it misses.
    calls     the same four entry points as a caller sees them, untraced, in this process: host clock around one call (output
              allocation, one launch, one stream synchronise).  About 0.03 ms of every figure is that fixed cost, a third of
              an 8-bit call and a tenth of a deep one, so these are not kernel times and no ratio of them is the gate.
    enhance   cfg4's arguments, device resident: 8 bit = bgr2lab8 + train + apply_rounded8 + lab2bgr8, deep = bgr16_to_lab +
              train on the guide + apply on the unrounded L + lab_to_bgr16 (that apply cannot take over training's reduce
              half: its plane is not the level plane).  Median wall time of `--runs` runs, each ending in a synchronise.

    python tools/deep_colour_timing.py [--out FILE]
    python tools/deep_colour_timing.py --child SIDE KIND      # what one traced child runs
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
OUT = os.path.join(ROOT, "profiles", "r22_deep_colour_timing.json")
BYTES = {"bgr16_to_lab": 6 + 16, "lab_to_bgr16": 12 + 6, "bgr2lab8": 3 + 7, "lab2bgr8": 7 + 3}
KERNELS = {"bgr16_to_lab": "k_bgr16_to_lab", "lab_to_bgr16": "k_lab_to_bgr16", "bgr2lab8": "k_bgr2lab8", "lab2bgr8": "k_lab2bgr8"}
SIDES, KINDS = (4096, 512), ("image", "random")
CHILD_TIMEOUT = 240


def source(side, kind):
    """image: smooth colour gradients plus noise of 250 codes (what a photograph's neighbourhoods look like to the table
    gathers: one wave's codes fall on a few cache lines); random: uniform codes"""
    rng = np.random.default_rng(7)
    if kind == "random":
        return rng.integers(0, 65536, (side, side, 3), dtype=np.uint16)
    y, x = np.mgrid[0:side, 0:side].astype(np.float32)
    img = np.stack([9000 + 30000 * x / side + 6000 * np.sin(y / 97.0), 20000 + 25000 * y / side,
                    52000 - 35000 * (x + y) / (2 * side)], axis=2)
    return np.clip(np.rint(img + rng.normal(0, 250, img.shape).astype(np.float32)), 0, 65535).astype(np.uint16)


def four_calls(ctx, side, kind):
    import torch
    src = source(side, kind)
    bgr16 = torch.from_numpy(src).to("cuda:0")
    bgr8 = torch.from_numpy((src >> 8).astype(np.uint8)).to("cuda:0")
    L, A, B, _ = ctx.bgr16_to_lab(bgr16)
    lab, L8 = ctx.bgr2lab8(bgr8)
    calls = {"bgr16_to_lab": lambda: ctx.bgr16_to_lab(bgr16), "lab_to_bgr16": lambda: ctx.lab_to_bgr16(L, A, B),
             "bgr2lab8": lambda: ctx.bgr2lab8(bgr8), "lab2bgr8": lambda: ctx.lab2bgr8(lab, L=L8)}
    for fn in calls.values():   # warm-up round
        fn()
    torch.cuda.synchronize()
    return calls


def child(side, kind, reps):
    """the traced program: a warm-up round (and the two set-up conversions), then `reps` rounds of the four calls"""
    import __graft_entry__ as entry
    nle = entry.load_package()
    ctx = nle.Context(0)
    calls = four_calls(ctx, side, kind)
    for _ in range(reps):
        for fn in calls.values():
            fn()
    ctx.close()


def traced(side, kind, reps):
    """kernel name -> the durations (ns) of its last `reps` dispatches in a kernel trace of one child"""
    d = tempfile.mkdtemp(prefix="deep_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--child", str(side), kind, "--reps", str(reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT, cwd=tempfile.gettempdir())
        if r.returncode != 0:
            raise RuntimeError(f"traced child {side} {kind} failed ({r.returncode}): {r.stderr[-1500:]}")
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError(f"no kernel trace written under {d}: {[p for p, _, _ in os.walk(d)]}")
        rows = []
        for f in files:
            with open(f) as fh:
                rows += [(int(x["Start_Timestamp"]), int(x["End_Timestamp"]), x["Kernel_Name"]) for x in csv.DictReader(fh)]
        rows.sort()
        out = {}
        for key, kname in KERNELS.items():
            ns = [e - s for s, e, n in rows if kname + "(" in n or n.endswith(kname)]
            if len(ns) < reps:
                raise RuntimeError(f"{kname}: {len(ns)} dispatches in the trace, {reps} expected; names: {sorted({n for _, _, n in rows})[:12]}")
            out[key] = ns[-reps:]
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--child", nargs=2, metavar=("SIDE", "KIND"))
    a = ap.parse_args()
    if a.child:
        return child(int(a.child[0]), a.child[1], a.reps)
    rec = {"reps": a.reps, "runs": a.runs, "kernels": {}, "calls": {}, "enhance": {}}
    # ---- kernel times: one traced child per shape, before this process opens the device
    for side in SIDES:
        for kind in KINDS:
            ns = traced(side, kind, a.reps)
            n = side * side
            row = {}
            for k, v in ns.items():
                s = statistics.median(v) * 1e-9
                row[k] = {"kernel_ms": s * 1e3, "min_ms": min(v) * 1e-6, "max_ms": max(v) * 1e-6, "bytes_per_pixel": BYTES[k],
                          "hbm_fraction": BYTES[k] * n / s / HBM_PEAK}
            deep = row["bgr16_to_lab"]["kernel_ms"] + row["lab_to_bgr16"]["kernel_ms"]
            eight = row["bgr2lab8"]["kernel_ms"] + row["lab2bgr8"]["kernel_ms"]
            row["deep_pair_ms"], row["eight_bit_pair_ms"], row["ratio"] = deep, eight, deep / eight
            rec["kernels"][f"{side}x{side}_{kind}"] = row
            print(f"kernels {side}^2 {kind}:", {k: round(v["kernel_ms"], 4) for k, v in row.items() if isinstance(v, dict)},
                  "ratio %.2f" % (deep / eight), flush=True)
    rec["gate"] = {"limit": 3.0, "of": "summed kernel time of the pair at 4096^2, medians of traced dispatches"}
    for kind in KINDS:
        r = rec["kernels"][f"4096x4096_{kind}"]["ratio"]
        rec["gate"][kind] = {"deep_pair_over_eight_bit_pair_at_4096": r, "met": bool(r <= 3.0)}
    print("gate:", rec["gate"], flush=True)

    import __graft_entry__ as entry
    import torch
    nle = entry.load_package()
    synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
    ctx = nle.Context(0)
    rec["device"] = torch.cuda.get_device_name(0)
    # ---- whole calls, as a caller sees them (not kernel times)
    for side in SIDES:
        calls = four_calls(ctx, side, "image")
        times = {k: [] for k in calls}
        for _ in range(a.reps):
            for k, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                times[k].append(time.perf_counter() - t0)
        rec["calls"][f"{side}x{side}_image"] = {k: {"ms_per_call": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3}
                                                for k, ts in times.items()}
        print(f"calls {side}^2 image:", {k: round(v["ms_per_call"], 4) for k, v in rec["calls"][f"{side}x{side}_image"].items()},
              flush=True)

    # ---- train + enhance at cfg4's arguments
    cfg = dict(synth.CONFIGS["cfg4"])
    H, W = cfg["H"], cfg["W"]
    lum = synth.synthetic_luminance(H, W)      # levels 0..255; both inputs are greys of it, so both paths train on this plane
    g8 = np.clip(np.rint(lum), 0, 255).astype(np.uint8)
    bgr8 = torch.from_numpy(np.repeat(g8[..., None], 3, axis=2)).to("cuda:0")
    bgr16 = torch.from_numpy(np.repeat((g8.astype(np.uint16) * 257)[..., None], 3, axis=2)).to("cuda:0")
    weights = [3.0, 3.0, 1.0, 1.0]
    f = nle.NLEFilter(ctx)

    def eight():
        lab, L = ctx.bgr2lab8(bgr8)
        f.train_filter(L, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], cfg["T"], cfg["K"])
        y = f.apply_rounded8(L, nle.transform_eigenvalues(f.eigvals, weights))
        return ctx.lab2bgr8(lab, L=y)

    def deep():
        L, A, B, G = ctx.bgr16_to_lab(bgr16)
        f.train_filter(G, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], cfg["T"], cfg["K"])
        y = f.apply(L, nle.transform_eigenvalues(f.eigvals, weights))
        return ctx.lab_to_bgr16(y.reshape(L.shape), A, B)
    for name, fn in (("eight_bit", eight), ("deep", deep)):
        fn()
        torch.cuda.synchronize()
    times = {"eight_bit": [], "deep": []}
    for _ in range(a.runs):
        for name, fn in (("eight_bit", eight), ("deep", deep)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    for name, ts in times.items():
        rec["enhance"][name] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}
    rec["enhance"]["formulation"] = f.diag()["formulation"]
    rec["enhance"]["deep_minus_eight_bit_ms"] = rec["enhance"]["deep"]["median_ms"] - rec["enhance"]["eight_bit"]["median_ms"]
    print("enhance cfg4:", rec["enhance"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    f.close()
    ctx.close()


if __name__ == "__main__":
    main()
