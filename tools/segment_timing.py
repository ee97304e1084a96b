#!/usr/bin/env python3
"""Cost of automatic regions (nle_segment_stats / nle_segment_assign / nle_filter_segment) on one
MI355X -> profiles/r29_segments.json.

    kernels    KERNEL time of k_segment_stats (with its fold) and k_segment_assign (indicator planes requested) at 4096^2 for
               C = 4 and C = 8, on random planes; labels random per pixel (every wave gathers from all C planes: the worst
               case) and, for stats, also in bands of 64 rows (what segments look like: a wave gathers from one plane).  One child process under `rocprofv3 --kernel-trace` (a run of its
               own; nothing else is traced): per round and C stats, assign, stats on bands; `--reps` rounds after a
               warm-up round; each figure is the median of its dispatches' End - Start in the trace.  `hbm_fraction` is the
               bytes the kernel has to move over that time against the 8 TB/s HBM peak: assign reads C planes and a byte and
               writes C planes and a byte, stats reads one gathered value and a byte.  The assign call rewrites its label
               tensor in place, so after the warm-up round the labels are a fixed point: the timed dispatches change no
               label and move the same bytes.
    iteration  cfg4's arguments (4096^2, 200 samples, K = 50), device resident: one nle_filter_segment call with max_iter = 1
               (spread + stats + assign + the download, and the start's pass that writes the indicator planes of the labels
               given), median wall time of `--runs` calls, host clock around a synchronise.
    natural    tests/golden/flower-50.bmp's L plane resampled to 4096^2 (bilinear, rounded to levels): train + segment under
               the cap of 40 iterations, C = 4; wall time, iterations, counts, and `label_moves`: the labels each iteration
               changed, from the same start through one-iteration calls (whether the loop settled or ran into the cap).
    bench      `--bench-lines FILE`: lines `parent <json>` / `head <json>`, the result lines of bench.py run on the parent
               commit and on this one alternately in one session; their values go into the same JSON with the rule the last
               refactors used: the head's median may not fall below the smaller parent value minus the parents' spread.

    python tools/segment_timing.py [--out FILE] [--bench-lines FILE]
    python tools/segment_timing.py --child      # what the traced child runs
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
OUT = os.path.join(ROOT, "profiles", "r29_segments.json")
SIDE, COUNTS = 4096, (4, 8)
STATS = tuple(f"stats_c{c}{kind}" for c in COUNTS for kind in ("", "_banded"))
KERNELS = {"k_segment_stats": STATS, "k_segment_fold": tuple(k.replace("stats", "fold") for k in STATS),
           "k_segment_assign": tuple(f"assign_c{c}" for c in COUNTS)}
BYTES = {k: 5 for k in STATS}
BYTES.update({f"assign_c{c}": 8 * c + 2 for c in COUNTS})
CHILD_TIMEOUT = 300


def calls_of(nle, ctx):
    import torch
    n = SIDE * SIDE
    g = torch.Generator(device="cuda:0").manual_seed(7)
    calls = []
    for c in COUNTS:
        q = torch.empty((c, n), device="cuda:0").normal_(1.0, 0.5, generator=g)
        ind = torch.empty((c, n), device="cuda:0")
        labels = torch.randint(0, c, (n,), device="cuda:0", generator=g).to(torch.uint8)
        m = np.linspace(0.9, 1.1, c)
        banded = (torch.arange(n, device="cuda:0") // (SIDE * 64) % c).to(torch.uint8)  # bands of 64 rows: what segments look like
        calls.append((f"stats_c{c}", lambda q=q, labels=labels: ctx.segment_stats(q, labels)))
        calls.append((f"assign_c{c}", lambda q=q, labels=labels, m=m, ind=ind: ctx.segment_assign(q, m, labels, indicators=ind)))
        calls.append((f"stats_c{c}_banded", lambda q=q, labels=banded: ctx.segment_stats(q, labels)))
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
    d = tempfile.mkdtemp(prefix="segment_trace_")
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


def flower_plane(torch):
    """the L plane of tests/golden/flower-50.bmp at SIDE x SIDE: bilinear, rounded to levels"""
    from PIL import Image
    import __graft_entry__ as entry
    oracle = entry.load_oracle()
    bgr = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "flower-50.bmp")).convert("RGB"))[..., ::-1].copy()
    L = torch.from_numpy(oracle.bgr_to_lab8(bgr)[..., 0].astype(np.float32)).to("cuda:0")
    big = torch.nn.functional.interpolate(L[None, None], size=(SIDE, SIDE), mode="bilinear", align_corners=False)[0, 0]
    return big.round().clamp(0, 255).contiguous()


def bench_values(path):
    vals = {"parent": [], "head": []}
    for line in open(path):
        who, _, rest = line.strip().partition(" ")
        if who in vals and rest.startswith("{"):
            vals[who].append(json.loads(rest)["value"])
    return vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--bench-lines", default=None)
    ap.add_argument("--kernels-only", action="store_true", help="the kernel trace alone, printed, nothing written")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.reps)
    rec = {"reps": a.reps, "runs": a.runs, "side": SIDE, "kernels": {}, "iteration": {}, "natural": {}}
    # ---- kernel times: one traced child, before this process opens the device
    ns = traced(a.reps)
    n = SIDE * SIDE
    for k, v in ns.items():
        s = statistics.median(v) * 1e-9
        rec["kernels"][k] = {"kernel_ms": s * 1e3, "min_ms": min(v) * 1e-6, "max_ms": max(v) * 1e-6}
        if k in BYTES:
            rec["kernels"][k].update(bytes_per_pixel=BYTES[k], hbm_fraction=BYTES[k] * n / s / HBM_PEAK)
    print("kernels:", {k: (round(v["kernel_ms"], 4), round(v.get("hbm_fraction", 0), 3)) for k, v in rec["kernels"].items()}, flush=True)

    if a.kernels_only:
        return
    import __graft_entry__ as entry
    import torch
    nle = entry.load_package()
    synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
    ctx = nle.Context(0)
    rec["device"] = torch.cuda.get_device_name(0)
    cfg = dict(synth.CONFIGS["cfg4"])
    f = nle.NLEFilter(ctx)

    def sync_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    # ---- one iteration at cfg4's arguments
    lum = torch.from_numpy(synth.synthetic_luminance(cfg["H"], cfg["W"]).astype(np.float32)).to("cuda:0")
    f.train_filter(lum, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], cfg["T"], cfg["K"])
    for c in COUNTS:
        labels, _ = ctx.segment_init(lum, c)
        f.segment(c, 4.0, 1, labels=labels)
        ts = [sync_ms(lambda: f.segment(c, 4.0, 1, labels=labels))[0] for _ in range(a.runs)]
        rec["iteration"][f"c{c}"] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}
    rec["iteration"]["config"] = "cfg4"
    rec["iteration"]["formulation"] = f.diag()["formulation"]
    print("one iteration:", rec["iteration"], flush=True)

    # ---- a natural image at 4096^2: train + segment to convergence
    big = flower_plane(torch)
    hx = 100.0 * SIDE / 400.0

    def natural():
        f.train_filter(big, 10, 20, hx, 30.0, cfg["T"], cfg["K"])
        return f.segment(4, 4.0, 40)
    natural()
    runs = [sync_ms(natural) for _ in range(3)]
    last = runs[-1][1]
    labels, _ = ctx.segment_init(big, 4)
    moves = []
    for _ in range(last["iterations"]):
        before = labels.clone()
        f.segment(4, 4.0, 1, labels=labels)
        moves.append(int((labels != before).sum().item()))
    rec["natural"] = {"image": "tests/golden/flower-50.bmp, L resampled to 4096^2", "segments": 4, "train_plus_segment_ms":
                      statistics.median(t for t, _ in runs), "iterations": last["iterations"], "converged": last["converged"],
                      "counts": last["counts"].tolist(), "label_moves": moves, "objective": [float(v) for v in last["objective"]]}
    print("natural:", {k: v for k, v in rec["natural"].items() if k != "objective"}, flush=True)
    f.close()
    ctx.close()

    if a.bench_lines:
        v = bench_values(a.bench_lines)
        rec["bench"] = {"order": "parent, head, parent, head", "unit": "MP/s", **v}
        if len(v["parent"]) >= 2 and v["head"]:
            spread = max(v["parent"]) - min(v["parent"])
            rec["bench"].update(parent_spread=spread, floor=min(v["parent"]) - spread, head_median=statistics.median(v["head"]),
                                holds=statistics.median(v["head"]) >= min(v["parent"]) - spread)
        print("bench:", rec["bench"], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
