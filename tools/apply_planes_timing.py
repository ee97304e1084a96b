#!/usr/bin/env python3
"""Cost of nle_apply_planes and of its first users against the parent commit -> profiles/r11_apply_planes_timing.json.

cfg4 (4096^2, 20 x 10 samples, K = 50) and cfg2 (512^2) of synthetic.py, synthetic integer planes, auto mode (the tables).
Yardsticks, from the PARENT commit's library (--baseline PATH, loaded by path in its own child processes, as
tools/chroma_timing.py does): P x nle_apply, nle_region_spread (M = 2, 4, 8), nle_apply_regions (M = 2, L = 4) and two
nle_apply_rounded8.  Against them, from this build: nle_apply_planes at P = 1, 2, 3, 4, 8, the same region calls, and the a / b
pair of the denoiser as one nle_apply_planes(P = 2, ROUNDED8).

Every entry point synchronises the ctx's stream before it returns, so a figure is the time between two events recorded on that
stream around the call(s) after one warm-up; per child the median of --reps, then the median and max - min of --runs
alternating child processes (parent, this, parent, ...), each under its own time limit; the first failing child ends the run.

Beside each ratio stands the ratio of the algorithmic bytes of either pixel half, (10 + 4 P) / (14 P).  Gates, relative to the
parent and the measured spreads, no fixed figure:
  1  for every configuration and P >= 2 the batched call beats P parent calls by more than the larger of the two spreads;
  2  at P = 1 nle_apply_planes is within the spread of the parent's nle_apply.

    python tools/apply_planes_timing.py --baseline /path/to/parent/libnle_hip.so
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

OUT = os.path.join(ROOT, "profiles", "r11_apply_planes_timing.json")
PS = (1, 2, 3, 4, 8)
MS = (2, 4, 8)
L, SPREAD, FLOOR = 4, 4.0, 0.05
WT = [[2.0, 3.0, 4.0, 1.0], [4.0, 3.0, 2.0, 1.0], [0.5, 0.5, 1.0, 1.0]]
CHILD_TIMEOUT = 300
TAG = "APPLY_PLANES_TIMING "


def _timed(torch, stream, fn, reps):
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
    parent = a.child == "parent"
    if parent:  # the parent's library does not export the new call: the mirror must not ask for it
        nle._SIGNATURES.pop("nle_apply_planes", None)
    synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
    ctx = nle.Context(0)
    out = {"device": torch.cuda.get_device_name(0), "lib": os.environ.get("NLE_LIB_PATH", "this build"), "configs": {}}
    for name in a.cfg:
        cfg = synth.CONFIGS[name]
        H, W = cfg["H"], cfg["W"]
        N = H * W
        x = torch.as_tensor(synth.synthetic_luminance(H, W).astype(np.float32), device="cuda:0")
        planes = torch.stack([x] + [torch.as_tensor(synth.synthetic_luminance(H, W, seed=100 + m).astype(np.float32),
                                                    device="cuda:0") for m in range(1, max(PS))])
        s = np.zeros((max(MS), H, W), dtype=np.float32)
        b = max(H // 64, 4)
        for m in range(max(MS)):  # square strokes, 1 / 4096 of the plane each
            r0, c0 = (m + 1) * H // 10, ((3 * m + 1) % 9 + 1) * W // 11
            s[m, r0:r0 + b, c0:c0 + b] = 1.0
        strokes = torch.as_tensor(s, device="cuda:0")
        f = nle.NLEFilter(ctx).train_filter(x, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], cfg["T"], cfg["K"])
        rec = dict(H=H, W=W, N=N, formulation=f.diag()["formulation"])
        Kp = f.info()["K"]
        fS = nle.transform_eigenvalues(f.eigvals, WT[0])
        y = torch.empty((max(PS), N), dtype=torch.float32, device="cuda:0")
        q = torch.empty((max(MS), N), dtype=torch.float32, device="cuda:0")
        resp = [fS] * max(PS)
        for P in PS:
            def singles(P=P):
                for m in range(P):
                    f.apply(planes[m], fS, out=y[m])
            if parent:
                rec["apply_x%d_ms" % P] = _timed(torch, ctx._stream, singles, a.reps)
            else:
                rec["apply_planes_%d_ms" % P] = _timed(torch, ctx._stream, lambda P=P: f.apply_planes(planes[:P], resp[:P], out=y[:P]), a.reps)
        if not parent:
            rec["apply_x1_ms"] = _timed(torch, ctx._stream, lambda: f.apply(planes[0], fS, out=y[0]), a.reps)
        for M in MS:
            scale = np.array([N / float(p.sum()) for p in s[:M]])
            rec["region_spread_%d_ms" % M] = _timed(torch, ctx._stream, lambda M=M, scale=scale: f.region_spread(
                strokes[:M], scale, SPREAD, out=q[:M]), a.reps)
        scale2 = np.array([N / float(p.sum()) for p in s[:2]])
        rec["apply_regions_ms"] = _timed(torch, ctx._stream, lambda: f.apply_regions(
            x, L, strokes[:2], WT, scale2, SPREAD, FLOOR, nle.REGION_OUT_ROUNDED8, out=y[0]), a.reps)
        if parent:
            def pair():
                f.apply_rounded8(planes[0], fS, out=y[0])
                f.apply_rounded8(planes[1], fS, out=y[1])
        else:
            def pair():
                f.apply_planes(planes[:2], resp[:2], out_kind=nle.REGION_OUT_ROUNDED8, out=y[:2])
        rec["denoise_pair_ms"] = _timed(torch, ctx._stream, pair, a.reps)
        assert Kp == len(fS)
        f.close()
        out["configs"][name] = rec
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline", help="the parent commit's libnle_hip.so")
    ap.add_argument("--cfg", nargs="*", default=["cfg4", "cfg2"])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--child", choices=["parent", "this"])
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.baseline or not os.path.exists(a.baseline):
        raise SystemExit("--baseline: the parent commit's libnle_hip.so is needed (its calls are the yardsticks)")
    runs = {"parent": [], "this": []}
    for i in range(a.runs):  # alternating
        for what in ("parent", "this"):
            runs[what].append(run_child(a, what))
            print(f"run {i} {what}: done", flush=True)
    out = {"workload": "synthetic integer planes (synthetic.py), auto mode; L = %d, spread %g, floor %g" % (L, SPREAD, FLOOR),
           "method": "milliseconds between two events on the ctx's stream around the call(s), every entry point synchronising "
                     "before it returns; median of %d per child after one warm-up, then the median and max - min of %d "
                     "alternating child processes; `parent` = the parent commit's library loaded by path" % (a.reps, a.runs),
           "device": runs["this"][0]["device"], "configs": {}, "gates": {}}
    ok1, ok2 = True, True
    for name in a.cfg:
        rec = {k: v for k, v in runs["this"][0]["configs"][name].items() if not k.endswith("_ms")}
        med, spread = {}, {}
        for what in ("parent", "this"):
            for key in [k for k in runs[what][0]["configs"][name] if k.endswith("_ms")]:
                v = [r["configs"][name][key] for r in runs[what]]
                med[(what, key)], spread[(what, key)] = statistics.median(v), max(v) - min(v)
                rec["%s.%s" % (what, key)] = dict(median=med[(what, key)], spread=spread[(what, key)], runs=v)
        rows = {}
        for P in PS:
            pk, tk = ("parent", "apply_x%d_ms" % P), ("this", "apply_planes_%d_ms" % P)
            sp = max(spread[pk], spread[tk])
            row = dict(parent_ms=med[pk], this_ms=med[tk], ratio=med[tk] / med[pk], byte_ratio=(10 + 4 * P) / (14.0 * P),
                       larger_spread_ms=sp)
            if P >= 2:
                row["gate1_faster_by_more_than_spread"] = bool(med[pk] - med[tk] > sp)
                ok1 = ok1 and row["gate1_faster_by_more_than_spread"]
            else:
                row["gate2_within_spread"] = bool(abs(med[tk] - med[pk]) <= sp)
                ok2 = ok2 and row["gate2_within_spread"]
            rows["P=%d" % P] = row
        rec["apply_planes_vs_P_parent_applies"] = rows
        users = {}
        for key, P in [("region_spread_%d_ms" % M, M) for M in MS] + [("apply_regions_ms", 3), ("denoise_pair_ms", 2)]:
            users[key[:-3]] = dict(parent_ms=med[("parent", key)], this_ms=med[("this", key)],
                                   ratio=med[("this", key)] / med[("parent", key)],
                                   byte_ratio_of_the_reduce_half=(10 + 4 * P) / (14.0 * P),
                                   larger_spread_ms=max(spread[("parent", key)], spread[("this", key)]))
        rec["users"] = users
        out["configs"][name] = rec
        print(name, json.dumps(dict(planes=rows, users=users)), flush=True)
    out["gates"] = {"1_batched_beats_P_parent_calls_for_every_P_ge_2": ok1, "2_P_eq_1_within_spread_of_parent_apply": ok2}
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("gates:", out["gates"])
    print("wrote", a.out)


if __name__ == "__main__":
    main()
