#!/usr/bin/env python3
"""Cost of the region edits (nle_apply_regions) at cfg4 and cfg2, M = 2 strokes, L = 4 layers -> profiles/r8_region_timing.json.

Per configuration, on the synthetic plane in auto mode (the tables): the time of one nle_apply_regions and its split into the
three calls it composes -- nle_apply_layers, nle_region_spread (M applies) and nle_region_combine -- with nle_apply_rounded8,
the global edit it replaces, beside it.  Every entry point synchronises the ctx's stream before it returns, so each figure
is the time between two events recorded on that stream around one call (launches, kernels and the final synchronisation).

The combine's yardstick is a device-to-device copy, timed the same way (event, copy, synchronise, event) in the same session:
child processes alternate between the edits and the copy, `--runs` of each (a fresh process per run, each under its own time
limit; the first failure ends the session).  The combine moves B = (L + M + 1) 4 N bytes (L + M planes in, one out); the copy
that moves as many bytes copies B / 2 (it reads and writes each one), and the copy OF B bytes is recorded too.  The combine is
stated as a multiple of either and as a fraction of the 8 TB/s HBM peak.  No gate.

    python tools/region_timing.py            # writes the record
    python tools/region_timing.py --child edits --cfg cfg4
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
OUT = os.path.join(ROOT, "profiles", "r8_region_timing.json")
M, L, SPREAD, FLOOR = 2, 4, 4.0, 0.05
WT = [[2.0, 3.0, 4.0, 1.0], [4.0, 3.0, 2.0, 1.0], [0.5, 0.5, 1.0, 1.0]]
CHILD_TIMEOUT = 240


def _timed(torch, stream, fn, reps):
    """median milliseconds between two events on `stream` around fn() (which ends with the stream synchronised)"""
    ms = []
    with torch.cuda.stream(stream):
        for _ in range(reps + 1):  # the first call warms the workspace cache and the code objects
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms[1:])


def child(a):
    import __graft_entry__ as entry
    import torch
    nle = entry.load_package()
    synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
    ctx = nle.Context(0)
    out = {"device": torch.cuda.get_device_name(0), "configs": {}}
    for name in a.cfg:
        cfg = synth.CONFIGS[name]
        H, W = cfg["H"], cfg["W"]
        N = H * W
        B = (L + M + 1) * 4 * N
        rec = dict(H=H, W=W, N=N, bytes_moved=B)
        if a.child == "copy":
            for label, nbytes in (("copy_same_traffic_ms", B // 2), ("copy_of_B_bytes_ms", B)):
                src = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda:0").normal_()
                dst = torch.empty_like(src)
                torch.cuda.synchronize()

                def copy():
                    dst.copy_(src)
                    ctx._stream.synchronize()

                rec[label] = _timed(torch, ctx._stream, copy, a.reps)
                del src, dst
        else:
            x = torch.as_tensor(synth.synthetic_luminance(H, W).astype(np.float32), device="cuda:0")
            s = np.zeros((M, H, W), dtype=np.float32)
            b = max(H // 64, 4)  # two square strokes, 1 / 4096 of the plane each
            s[0, H // 4:H // 4 + b, W // 4:W // 4 + b] = 1.0
            s[1, 3 * H // 4:3 * H // 4 + b, 2 * W // 3:2 * W // 3 + b] = 1.0
            scale = np.array([N / float(p.sum()) for p in s])
            strokes = torch.as_tensor(s, device="cuda:0")
            f = nle.NLEFilter(ctx).train_filter(x, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], cfg["T"], cfg["K"])
            rec["formulation"] = f.diag()["formulation"]
            fS = nle.transform_eigenvalues(f.eigvals, WT[0])
            layers = torch.empty((L, N), dtype=torch.float32, device="cuda:0")
            q = torch.empty((M, N), dtype=torch.float32, device="cuda:0")
            y = torch.empty(N, dtype=torch.float32, device="cuda:0")
            rec["apply_regions_ms"] = _timed(torch, ctx._stream, lambda: f.apply_regions(
                x, L, strokes, WT, scale, SPREAD, FLOOR, nle.REGION_OUT_ROUNDED8, out=y), a.reps)
            rec["layers_ms"] = _timed(torch, ctx._stream, lambda: f.apply_layers(x, L, out=layers), a.reps)
            rec["spreads_ms"] = _timed(torch, ctx._stream, lambda: f.region_spread(strokes, scale, SPREAD, out=q), a.reps)
            rec["combine_ms"] = _timed(torch, ctx._stream, lambda: ctx.region_combine(
                layers, q, WT, FLOOR, nle.REGION_OUT_ROUNDED8, out=y), a.reps)
            rec["apply_rounded8_ms"] = _timed(torch, ctx._stream, lambda: f.apply_rounded8(x, fS, out=y), a.reps)
            f.close()
        out["configs"][name] = rec
    ctx.close()
    print("REGION_TIMING " + json.dumps(out), flush=True)


def run_child(a, what):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--reps", str(a.reps), "--cfg"] + a.cfg
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    if r.returncode != 0:  # nothing more is started on the GPU after a failure
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"child '{what}' failed with status {r.returncode}: stopping")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("REGION_TIMING ")][-1]
    return json.loads(line[len("REGION_TIMING "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", nargs="*", default=["cfg4", "cfg2"])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--child", choices=["edits", "copy"])
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = {"edits": [], "copy": []}
    for i in range(a.runs):  # alternating
        for what in ("edits", "copy"):
            runs[what].append(run_child(a, what))
            print(f"run {i} {what}: done", flush=True)
    out = {"workload": "synthetic plane (synthetic.py), auto mode, M = %d strokes, L = %d layers, spread %g, floor %g, "
                       "NLE_REGION_OUT_ROUNDED8" % (M, L, SPREAD, FLOOR),
           "method": "milliseconds between two events on the ctx's stream around one call (every entry point synchronises "
                     "the stream before it returns; the copy is timed the same way); median of %d calls per child, then "
                     "the median (and max - min) of %d alternating child processes" % (a.reps, a.runs),
           "hbm_peak_TBps": HBM_PEAK / 1e12, "device": runs["edits"][0]["device"], "configs": {}}
    for name in a.cfg:
        rec = dict(runs["edits"][0]["configs"][name])
        for what in ("edits", "copy"):
            for key in [k for k in runs[what][0]["configs"][name] if k.endswith("_ms")]:
                v = [r["configs"][name][key] for r in runs[what]]
                rec[key] = statistics.median(v)
                rec[key.replace("_ms", "_runs_ms")] = v
                rec[key.replace("_ms", "_spread_ms")] = max(v) - min(v)
        rec["three_calls_ms"] = rec["layers_ms"] + rec["spreads_ms"] + rec["combine_ms"]
        rec["apply_regions_over_apply_rounded8"] = rec["apply_regions_ms"] / rec["apply_rounded8_ms"]
        rec["combine_over_copy_same_traffic"] = rec["combine_ms"] / rec["copy_same_traffic_ms"]
        rec["combine_over_copy_of_B_bytes"] = rec["combine_ms"] / rec["copy_of_B_bytes_ms"]
        rec["combine_fraction_of_hbm_peak"] = rec["bytes_moved"] / (rec["combine_ms"] * 1e-3) / HBM_PEAK
        rec["MP_per_s_apply_regions"] = rec["N"] / (rec["apply_regions_ms"] * 1e-3) / 1e6
        out["configs"][name] = rec
        print(name, json.dumps({k: v for k, v in rec.items() if not k.endswith("_runs_ms")}), flush=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
