#!/usr/bin/env python3
"""Cost of nle_nystrom_residual against what a user could compose before it -> profiles/r12_nystrom_residual_timing.json.

cfg4 (4096^2, 20 x 10 samples) and cfg2 (512^2, 10 x 20) of synthetic.py, synthetic integer planes, the grid sampler.

Yardstick, from the PARENT commit's library (--baseline PATH, loaded by path in its own child processes): what a user of that
library can do for the same map and summary -- nle_compute_kernel64 for K_A and the N x ld(p) fp64 affinity rows of the whole
plane, numpy's eigh of K_A and F = V diag(1 / sqrt(lambda)) at the cut, nle_ts_gemm64, and torch for 1 - sum_j t_ij^2 and the
four summary figures.  Against it, from this build: nle_nystrom_residual with NLE_RESID_AUTO, NLE_RESID_FUSED and
NLE_RESID_ROWS, map and summary.  A figure is the wall time of the whole call chain from the plane on the device to the summary
on the host (every entry point synchronises the ctx's stream before it returns; the torch tail ends in .item()), after one
warm-up; per child the median of --reps, then the median and max - min of --runs alternating child processes (parent, this,
parent, ...), each under its own time limit; the first failing child ends the run.

Gate, relative to the parent and the measured spreads, no fixed figure: at both sizes AUTO beats the yardstick by more than
the larger of the two spreads.  Route choice: FUSED against ROWS of this build in the same children; the record says which is
faster and by how much.  The maps of the three forms and of the yardstick are compared in the child (largest difference).

Kernel rate (a record, not a gate): --kernel-stats CSV takes the kernel_stats csv of a separate
`rocprofv3 --kernel-trace --stats -- python tools/nystrom_residual_timing.py --child this --cfg cfg4 --reps 3` run and adds the
fused kernel's average duration and its TFLOP/s (2 N p m flop) to the record, beside the 47.6 TF of
profiles/r1_mfma_f64_micro.jsonl.

    python tools/nystrom_residual_timing.py --baseline /path/to/parent/libnle_hip.so
    python tools/nystrom_residual_timing.py --kernel-stats CSV      # adds the kernel rate to the record written before
"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "r12_nystrom_residual_timing.json")
CHILD_TIMEOUT = 420
TAG = "NYSTROM_RESIDUAL_TIMING "
THRESH = 0.5
MFMA_F64_MICRO_TF = 47.6  # profiles/r1_mfma_f64_micro.jsonl: 14 independent accumulators, 2 waves per SIMD


def _timed(torch, fn, reps):
    ms = []
    for _ in range(reps + 1):  # the first call warms the workspace cache and the code objects
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms[1:])


def child(a):
    import ctypes as C
    import __graft_entry__ as entry
    import torch
    nle = entry.load_package()
    parent = a.child == "parent"
    if parent:  # the parent's library does not export the new call: the mirror must not ask for it
        nle._SIGNATURES.pop("nle_nystrom_residual", None)
    synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
    ctx = nle.Context(0)
    out = {"device": torch.cuda.get_device_name(0), "lib": os.environ.get("NLE_LIB_PATH", "this build"), "configs": {}}
    for name in a.cfg:
        cfg = synth.CONFIGS[name]
        H, W, nr, nc, hx, hy = cfg["H"], cfg["W"], cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"]
        N = H * W
        x = torch.as_tensor(synth.synthetic_luminance(H, W).astype(np.float32), device="cuda:0")
        g = nle.sample_grid(H, W, nr, nc)
        p = g["n_sel_rows"] * g["n_sel_cols"]
        rec = dict(H=H, W=W, N=N, p=p)
        keep = {}

        def composed():
            # what the parent's ABI offers: K_A and all affinity rows, the factor on the host, the product, torch for the rest
            Ka = np.zeros((p, p), dtype=np.float64)
            kab = torch.empty((N, nle.ld(p)), dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            nle._check(nle.lib().nle_compute_kernel64(ctx._h, C.c_void_p(x.data_ptr()), H, W, nr, nc, float(hx), float(hy),
                                                      Ka.ctypes.data_as(C.c_void_p), C.c_void_p(kab.data_ptr())), ctx._h)
            w, v = np.linalg.eigh(Ka)
            w, v = w[::-1], v[:, ::-1]
            m = 0
            while m < p and w[m] >= 1e-10:
                m += 1
            F = v[:, :m] / np.sqrt(w[:m])[None, :]
            T = ctx.ts_gemm64(kab, p, F)
            r = 1.0 - (T[:, :m] * T[:, :m]).sum(1)
            keep["map"], keep["m"] = r.to(torch.float32), m
            keep["summary"] = (float(r.sum().item()), float(r.max().item()), int(r.argmax().item()), int((r > THRESH).sum().item()))

        def call(form):
            def run():
                keep["map"], s = ctx.nystrom_residual(x, nr, nc, hx, hy, form=form, thresh=THRESH)
                keep["summary"] = (s["sum"], s["max"], s["argmax"], s["count"])
            return run

        if parent:
            rec["composed_ms"] = _timed(torch, composed, a.reps)
            rec["kept"] = keep["m"]
            rec["composed_summary"] = keep["summary"]
        else:
            maps = {}
            for label, form in (("auto", nle.RESID_AUTO), ("fused", nle.RESID_FUSED), ("rows", nle.RESID_ROWS)):
                rec[label + "_ms"] = _timed(torch, call(form), a.reps)
                rec[label + "_summary"] = keep["summary"]
                maps[label] = keep["map"].ravel().clone()
            keep.clear()
            if not a.no_compare:  # the same map as the composition, to rounding
                composed()
                rec["kept"] = keep["m"]
                rec["composed_summary"] = keep["summary"]
                for label in maps:
                    rec["max_abs_diff_%s_vs_composed" % label] = float((maps[label] - keep["map"]).abs().max().item())
            rec["auto_equals_fused_bitwise"] = bool(torch.equal(maps["auto"], maps["fused"]))
        keep.clear()
        out["configs"][name] = rec
        torch.cuda.empty_cache()
    ctx.close()
    print(TAG + json.dumps(out), flush=True)


def run_child(a, what):
    env = dict(os.environ)
    if what == "parent":
        env["NLE_LIB_PATH"] = os.path.abspath(a.baseline)
    else:
        env.pop("NLE_LIB_PATH", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--reps", str(a.reps), "--cfg"] + a.cfg
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT, env=env)
    if r.returncode != 0:  # nothing more is started on the GPU after a failure
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"child '{what}' failed with status {r.returncode}: stopping")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith(TAG)][-1]
    return json.loads(line[len(TAG):])


def kernel_rate(path, rec):
    """the fused kernel's row of a rocprofv3 kernel_stats csv -> average ms and TFLOP/s at cfg4's N, p, m"""
    with open(path, newline="") as fh:
        rows = [r for r in csv.DictReader(fh) if "k_nystrom_resid64" in r["Name"]]
    if not rows:
        raise SystemExit("no k_nystrom_resid64 row in " + path)
    row = max(rows, key=lambda r: float(r["TotalDurationNs"]))
    avg_ms = float(row["AverageNs"]) * 1e-6
    flop = 2.0 * rec["N"] * rec["p"] * rec["kept"]
    return dict(kernel=row["Name"].split("(")[0], calls=int(row["Calls"]), average_ms=avg_ms, min_ms=float(row["MinNs"]) * 1e-6,
                flop=flop, tflops=flop / (avg_ms * 1e-3) / 1e12, mfma_f64_micro_tflops=MFMA_F64_MICRO_TF,
                share_of_micro=flop / (avg_ms * 1e-3) / 1e12 / MFMA_F64_MICRO_TF,
                source="rocprofv3 --kernel-trace --stats, a run of its own (cfg4)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", help="the parent commit's libnle_hip.so")
    ap.add_argument("--cfg", nargs="*", default=["cfg4", "cfg2"])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", choices=["parent", "this"])
    ap.add_argument("--no-compare", action="store_true", help="child: skip the comparison against the composition")
    ap.add_argument("--kernel-stats", help="kernel_stats csv of a separate rocprofv3 run of `--child this --cfg cfg4`")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.kernel_stats and not a.baseline:  # add the kernel rate of a separate profiler run to an existing record
        out = json.load(open(a.out))
        out["fused_kernel_rate"] = kernel_rate(a.kernel_stats, out["configs"]["cfg4"])
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
        print(json.dumps(out["fused_kernel_rate"]))
        return
    if not a.baseline or not os.path.exists(a.baseline):
        raise SystemExit("--baseline: the parent commit's libnle_hip.so is needed (its calls are the yardstick)")
    runs = {"parent": [], "this": []}
    for i in range(a.runs):  # alternating
        for what in ("parent", "this"):
            runs[what].append(run_child(a, what))
            print(f"run {i} {what}: done", flush=True)
    out = {"workload": "synthetic integer planes (synthetic.py), grid sampler, thresh %g" % THRESH,
           "method": "wall milliseconds of the whole call chain, plane on the device to summary on the host, the device idle "
                     "before and after; median of %d per child after one warm-up, then the median and max - min of %d "
                     "alternating child processes; `parent` = the parent commit's library loaded by path, composing "
                     "nle_compute_kernel64 + numpy eigh + nle_ts_gemm64 + a torch row reduction" % (a.reps, a.runs),
           "device": runs["this"][0]["device"], "configs": {}, "gates": {}}
    ok = True
    for name in a.cfg:
        rec = {k: v for k, v in runs["this"][0]["configs"][name].items() if not k.endswith("_ms")}
        med, spread = {}, {}
        for what in ("parent", "this"):
            for key in [k for k in runs[what][0]["configs"][name] if k.endswith("_ms")]:
                v = [r["configs"][name][key] for r in runs[what]]
                med[key], spread[key] = statistics.median(v), max(v) - min(v)
                rec[key] = dict(median=med[key], spread=spread[key], runs=v)
        sp = max(spread["composed_ms"], spread["auto_ms"])
        gate = bool(med["composed_ms"] - med["auto_ms"] > sp)
        ok = ok and gate
        rec["auto_vs_composed"] = dict(parent_ms=med["composed_ms"], this_ms=med["auto_ms"], ratio=med["auto_ms"] / med["composed_ms"],
                                       larger_spread_ms=sp, gate_faster_by_more_than_spread=gate)
        faster = "fused" if med["fused_ms"] < med["rows_ms"] else "rows"
        rec["route_choice"] = dict(fused_ms=med["fused_ms"], rows_ms=med["rows_ms"], faster=faster,
                                   by_factor=max(med["fused_ms"], med["rows_ms"]) / min(med["fused_ms"], med["rows_ms"]),
                                   larger_spread_ms=max(spread["fused_ms"], spread["rows_ms"]))
        out["configs"][name] = rec
        print(name, json.dumps(dict(auto_vs_composed=rec["auto_vs_composed"], route_choice=rec["route_choice"])), flush=True)
    out["gates"] = {"auto_beats_the_composed_yardstick_at_every_size": ok}
    if a.kernel_stats:
        out["fused_kernel_rate"] = kernel_rate(a.kernel_stats, out["configs"]["cfg4"])
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("gates:", out["gates"])
    print("wrote", a.out)


if __name__ == "__main__":
    main()
