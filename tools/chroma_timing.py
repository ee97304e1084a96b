#!/usr/bin/env python3
"""Cost of the chroma-aware affinities (nle_ctx_set_chroma) at cfg2 and cfg4, T = 10, L = 4 -> profiles/r7_chroma_timing.json.

Per variant: the per-launch milliseconds of the affinity kernel (nle_ctx_kernel_stats under NLE_K_AFFINITY) in
NLE_MODE_MATERIALISED_F64 -- the same p, the same 1 Mi-pixel chunks for every variant -- and train + apply wall time:

    off_R0 / off_R1 / off_R3 / off_R5 / off_R7      k_affinity64 and k_patch_affinity64 without chroma
    chroma_R0 / chroma_R1 / chroma_R3               k_affinity64<true> and the chroma patch kernel (hc = 20)

The yardsticks are the chroma-off kernels of a BASELINE library (the parent commit's build, --baseline PATH), timed in the
same session as this tree's library, the two alternating, `--runs` child processes each (a fresh process per run: each
under its own time limit, and the first failure ends the session).  Medians are compared; the margin of "chroma off costs
nothing" is the spread (max - min) of the baseline's own runs.

    python tools/chroma_timing.py --baseline /path/to/parent/libnle_hip.so     # writes the record
    python tools/chroma_timing.py --child                                     # one run of this tree's library, JSON on stdout
    python tools/chroma_timing.py --child --cfg cfg4 --only chroma_R3          # one variant (for rocprofv3 --kernel-trace --stats)
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
OUT = os.path.join(ROOT, "profiles", "r7_chroma_timing.json")
CHUNK = 1 << 20  # build_phi64's affinity chunk (literal.hip; the rows come from samples.hip's AffinityRows64)
HC = 20.0
OFF = [("off_R0", 0, False), ("off_R1", 1, False), ("off_R3", 3, False), ("off_R5", 5, False), ("off_R7", 7, False)]
CHROMA = [("chroma_R0", 0, True), ("chroma_R1", 1, True), ("chroma_R3", 3, True)]
CHILD_TIMEOUT = 240


def child(a):
    import __graft_entry__ as entry
    import torch
    nle = entry.load_package()
    has_chroma = True
    path = os.environ.get("NLE_LIB_PATH")
    if path:  # a baseline library may predate the chroma entry points: bind what it has
        probe = ctypes.CDLL(path)
        for name in ("nle_ctx_set_chroma", "nle_filter_chroma"):
            if not hasattr(probe, name):
                nle._SIGNATURES.pop(name, None)
                has_chroma = False
    synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
    ctx = nle.Context(0)
    ctx.set_mode(nle.MODE_MATERIALISED_F64)
    out = {"device": torch.cuda.get_device_name(0), "library": path or nle.LIB_PATH, "configs": {}}
    for name in a.cfg:
        cfg = dict(synth.CONFIGS[name])
        cfg["T"], cfg["L"] = 10, 4
        H, W = cfg["H"], cfg["W"]
        x, pa, pb = (torch.as_tensor(synth.synthetic_luminance(H, W, seed=s).astype(np.float32), device="cuda:0")
                     for s in (1234, 77, 4242))
        g = nle.sample_grid(H, W, cfg["n_row"], cfg["n_col"])
        p = g["n_sel_rows"] * g["n_sel_cols"]
        ldp = nle.ld(p)
        rows = {}
        for label, R, chroma in OFF + (CHROMA if has_chroma else []):
            if a.only and label not in a.only:
                continue
            ctx.set_patch_radius(R)
            if has_chroma:
                ctx.set_chroma(pa if chroma else None, pb if chroma else None, HC)
            f = nle.NLEFilter(ctx)

            def once():
                f.train_filter(x, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], cfg["T"], cfg["K"])
                f.apply_layers(x, cfg["L"])
                torch.cuda.synchronize()

            once()  # warm: workspace cache, code objects
            t0 = time.perf_counter()
            for _ in range(a.reps):
                once()
            ms = (time.perf_counter() - t0) * 1e3 / a.reps
            ctx.profile(1)
            once()
            launches, aff_ms = ctx.kernel_stats()[nle.lib().nle_kernel_name(0).decode()]
            ctx.profile(0)
            d = f.diag()
            f.close()
            pl = aff_ms / launches
            rows[label] = dict(R=R, chroma=chroma, launches=launches, per_launch_ms=pl, train_apply_ms=round(ms, 3),
                               formulation=d["formulation"],
                               hbm_fraction_of_writes=min(CHUNK, H * W) * ldp * 8 / (pl * 1e-3) / HBM_PEAK)
        out["configs"][name] = dict(H=H, W=W, p=p, ld=ldp, chunk_rows=min(CHUNK, H * W), K=cfg["K"], variants=rows)
    if has_chroma:
        ctx.set_chroma(None, None, 0.0)
    ctx.close()
    print("CHROMA_TIMING " + json.dumps(out), flush=True)


def run_child(a, lib):
    env = dict(os.environ)
    if lib:
        env["NLE_LIB_PATH"] = lib
    else:
        env.pop("NLE_LIB_PATH", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--cfg"] + a.cfg
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    if r.returncode != 0:  # nothing more is started on the GPU after a failure
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"child failed with status {r.returncode} ({'baseline' if lib else 'this tree'}): stopping")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHROMA_TIMING ")][-1]
    return json.loads(line[len("CHROMA_TIMING "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", nargs="*", default=["cfg4", "cfg2"])
    ap.add_argument("--baseline", help="the parent commit's libnle_hip.so")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--only", nargs="*", help="(--child) only these variants")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.baseline or not os.path.exists(a.baseline):
        raise SystemExit("--baseline: the parent commit's libnle_hip.so is needed (its kernels are the yardsticks)")
    runs = {"baseline": [], "new": []}
    for i in range(a.runs):  # alternating
        for who, lib in (("baseline", os.path.abspath(a.baseline)), ("new", None)):
            runs[who].append(run_child(a, lib))
            print(f"run {i} {who}: done", flush=True)
    out = {"workload": "synthetic integer Lab triple (synthetic.py seeds 1234 / 77 / 4242), T = 10, L = 4, "
                       "NLE_MODE_MATERIALISED_F64, hc = %g" % HC,
           "method": "per launch = NLE_K_AFFINITY ms / launches of one profiled train; median of %d alternating child "
                     "processes per library; spread = max - min" % a.runs,
           "hbm_peak_TBps": HBM_PEAK / 1e12, "device": runs["new"][0]["device"], "configs": {}}
    for name in a.cfg:
        c0 = runs["new"][0]["configs"][name]
        rec = {k: c0[k] for k in ("H", "W", "p", "ld", "chunk_rows", "K")}
        for who in ("baseline", "new"):
            tab = {}
            for label in runs[who][0]["configs"][name]["variants"]:
                v = [r["configs"][name]["variants"][label] for r in runs[who]]
                pl = [x["per_launch_ms"] for x in v]
                tab[label] = dict(per_launch_ms=pl, median_ms=statistics.median(pl), spread_ms=max(pl) - min(pl),
                                  launches=v[0]["launches"],
                                  train_apply_ms=statistics.median(x["train_apply_ms"] for x in v),
                                  hbm_fraction_of_writes=statistics.median(x["hbm_fraction_of_writes"] for x in v))
            rec[who] = tab
        b, n = rec["baseline"], rec["new"]
        rec["gate_chroma_R0_not_slower_than_baseline_patch_R1"] = dict(
            chroma_R0_ms=n["chroma_R0"]["median_ms"], baseline_off_R1_ms=b["off_R1"]["median_ms"],
            holds=n["chroma_R0"]["median_ms"] <= b["off_R1"]["median_ms"])
        rec["chroma_R0_vs_baseline_k_affinity64"] = n["chroma_R0"]["median_ms"] / b["off_R0"]["median_ms"]
        rec["record_chroma_R3_between_baseline_R5_and_R7"] = dict(
            chroma_R3_ms=n["chroma_R3"]["median_ms"], baseline_off_R5_ms=b["off_R5"]["median_ms"],
            baseline_off_R7_ms=b["off_R7"]["median_ms"],
            between=b["off_R5"]["median_ms"] <= n["chroma_R3"]["median_ms"] <= b["off_R7"]["median_ms"])
        rec["chroma_off_costs_nothing"] = {
            label: dict(new_ms=n[label]["median_ms"], baseline_ms=b[label]["median_ms"], margin_ms=b[label]["spread_ms"],
                        holds=n[label]["median_ms"] <= b[label]["median_ms"] + b[label]["spread_ms"])
            for label in ("off_R0", "off_R1")}
        out["configs"][name] = rec
        print(name, json.dumps({k: rec[k] for k in rec if k not in ("baseline", "new")}), flush=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
