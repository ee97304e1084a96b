#!/usr/bin/env python3
"""Cost of the base tone curve (nle_plane_histogram / nle_tone_combine / nle_apply_tone) beside the
detail combine on one MI355X -> profiles/r28_tone.json.

    kernels   KERNEL time of k_plane_hist (one plane of 4096^2: a U(0, 255) base layer, and the same size all 128.0) and of
              k_tone_combine in the three output kinds beside k_detail_combine (F32), all at 4096^2, L = 4, the detail curve
              off.  One child process under `rocprofv3 --kernel-trace` (a run of its own; nothing else is traced): per round
              detail, hist, hist (flat), tone F32, tone ROUNDED8, tone U8, detail again; `--reps` rounds after a warm-up round;
              each figure is the median of its dispatches' End - Start in the trace.  `hbm_fraction` is the bytes the kernel
              has to move (hist: 4 B per pixel; the combines: 4 (L + 1) in and 4 or 1 out) over that time against the 8 TB/s
              HBM peak.  `spread` is the second detail dispatch of a round over the first.
    enhance   cfg4's arguments, device resident: train + apply_detail (w_rho 3, gain 2.5, sigma 6, ROUNDED8), the same through
              apply_tone with shadows alone (no histogram) and with all four options (histogram, its copy to the host, the
              curve on the host, the upload of the knots), alternating; median wall time of `--runs` runs, host clock around
              a synchronise.

    python tools/tone_timing.py [--out FILE]
    python tools/tone_timing.py --child      # what the traced child runs
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
OUT = os.path.join(ROOT, "profiles", "r28_tone.json")
SIDE, L = 4096, 4
# trace name -> the keys of its dispatches within one round, in order
KERNELS = {"k_detail_combine": ("detail", "detail_again"), "k_plane_hist": ("hist", "hist_flat"),
           "k_tone_combine": ("tone_f32", "tone_rounded8", "tone_u8")}
BYTES = {"detail": 4 * (L + 1) + 4, "detail_again": 4 * (L + 1) + 4, "hist": 4, "hist_flat": 4, "tone_f32": 4 * (L + 1) + 4,
         "tone_rounded8": 4 * (L + 1) + 4, "tone_u8": 4 * (L + 1) + 1}
CHILD_TIMEOUT = 240
WEIGHTS, W_RHO, GAIN, SIGMA = [3.0, 3.0, 1.0, 1.0], 3.0, 2.5, 6.0
TONE = dict(shadows=0.5, highlights=-0.3, clip_percent=1.0, equalise=0.5)


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


def calls_of(nle, ctx):
    import torch
    n = SIDE * SIDE
    x, Y = planes(n)
    flat = torch.full((n,), 128.0, device="cuda:0")
    out = torch.empty(n, device="cuda:0")
    out8 = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    curve = nle.tone_curve(ctx.plane_histogram(Y[L - 1], WEIGHTS[-1]), **TONE)
    detail = lambda: ctx.detail_combine(x, Y, WEIGHTS, W_RHO, 1.0, 0.0, nle.REGION_OUT_F32, out=out)  # noqa: E731
    tone = lambda kind, o: (lambda: ctx.tone_combine(x, Y, WEIGHTS, curve, W_RHO, 1.0, 0.0, kind, out=o))  # noqa: E731
    calls = [("detail", detail), ("hist", lambda: ctx.plane_histogram(Y[L - 1], WEIGHTS[-1])), ("hist_flat", lambda: ctx.plane_histogram(flat)),
             ("tone_f32", tone(nle.REGION_OUT_F32, out)), ("tone_rounded8", tone(nle.REGION_OUT_ROUNDED8, out)),
             ("tone_u8", tone(nle.REGION_OUT_U8, out8)), ("detail_again", detail)]
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
    d = tempfile.mkdtemp(prefix="tone_trace_")
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
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.reps)
    rec = {"reps": a.reps, "runs": a.runs, "side": SIDE, "layers": L, "tone": TONE, "kernels": {}, "enhance": {}}
    # ---- kernel times: one traced child, before this process opens the device
    ns = traced(a.reps)
    n = SIDE * SIDE
    for k, v in ns.items():
        s = statistics.median(v) * 1e-9
        rec["kernels"][k] = {"kernel_ms": s * 1e3, "min_ms": min(v) * 1e-6, "max_ms": max(v) * 1e-6, "bytes_per_pixel": BYTES[k],
                             "hbm_fraction": BYTES[k] * n / s / HBM_PEAK}
    ker = rec["kernels"]
    print("kernels:", {k: round(v["kernel_ms"], 4) for k, v in ker.items()}, flush=True)
    rec["spread"] = ker["detail_again"]["kernel_ms"] / ker["detail"]["kernel_ms"]
    rec["tone_over_detail"] = {k: ker[k]["kernel_ms"] / ker["detail"]["kernel_ms"] for k in ("tone_f32", "tone_rounded8", "tone_u8")}
    print("spread:", rec["spread"], "tone / detail:", rec["tone_over_detail"], flush=True)

    import __graft_entry__ as entry
    import torch
    nle = entry.load_package()
    synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
    ctx = nle.Context(0)
    rec["device"] = torch.cuda.get_device_name(0)
    # ---- train + enhance at cfg4's arguments: the detail options alone, and with the tone curve
    cfg = dict(synth.CONFIGS["cfg4"])
    lum = torch.from_numpy(synth.synthetic_luminance(cfg["H"], cfg["W"]).astype(np.float32)).to("cuda:0")
    f = nle.NLEFilter(ctx)

    def train():
        f.train_filter(lum, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], cfg["T"], cfg["K"])

    def detail():
        train()
        return f.apply_detail(lum, WEIGHTS, W_RHO, GAIN, SIGMA, nle.REGION_OUT_ROUNDED8)

    def shadows():
        train()
        return f.apply_tone(lum, WEIGHTS, W_RHO, GAIN, SIGMA, shadows=0.5, out_kind=nle.REGION_OUT_ROUNDED8)

    def tone():
        train()
        return f.apply_tone(lum, WEIGHTS, W_RHO, GAIN, SIGMA, out_kind=nle.REGION_OUT_ROUNDED8, **TONE)
    fns = (("detail", detail), ("tone_shadows_only", shadows), ("tone_all_options", tone))
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
    rec["enhance"]["formulation"] = f.diag()["formulation"]
    for name in ("tone_shadows_only", "tone_all_options"):
        rec["enhance"][name + "_minus_detail_ms"] = rec["enhance"][name]["median_ms"] - rec["enhance"]["detail"]["median_ms"]
    print("enhance cfg4:", rec["enhance"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    f.close()
    ctx.close()


if __name__ == "__main__":
    main()
