#!/usr/bin/env python3
"""Cost of the patch (non-local-means) affinities (nle_ctx_set_patch_radius) at cfg2 and cfg4, T = 10, L = 4, auto mode.

For every radius R in {0, 1, 2, 3, 5, 7}: train + apply milliseconds and the formulation auto mode took, and the
per-launch milliseconds of the affinity kernel (nle_ctx_kernel_stats under NLE_K_AFFINITY) -- k_patch_affinity64 for
R > 0 -- against k_affinity64 at R = 0 forced into NLE_MODE_MATERIALISED_F64 (same p, same 1 Mi-pixel chunks), with
the HBM fraction of each on the bytes it writes (chunk rows x ld x 8 per launch, against the 8 TB/s vendor peak).

    python tools/patch_timing.py                          # writes profiles/r5_patch_timing.json
    python tools/patch_timing.py --cfg cfg4 --radius 3 --reps 1 --no-write   # one train + apply (for rocprofv3)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

HBM_PEAK = 8.0e12
OUT = os.path.join(ROOT, "profiles", "r5_patch_timing.json")
CHUNK = 1 << 20  # build_phi64's affinity chunk (literal.hip; the rows come from samples.hip's AffinityRows64)


def run(nle, ctx, x, cfg, R, mode, reps):
    import torch
    ctx.set_mode(mode)
    ctx.set_patch_radius(R)
    f = nle.NLEFilter(ctx)
    L = cfg["L"]

    def once():
        f.train_filter(x, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], cfg["T"], cfg["K"])
        f.apply_layers(x, L)
        torch.cuda.synchronize()

    once()  # warm: workspace cache, code objects
    t0 = time.perf_counter()
    for _ in range(reps):
        once()
    ms = (time.perf_counter() - t0) * 1e3 / reps
    ctx.profile(1)
    once()
    launches, aff_ms = ctx.kernel_stats()[nle.lib().nle_kernel_name(0).decode()]
    ctx.profile(0)
    d = f.diag()
    f.close()
    ctx.set_patch_radius(0)
    ctx.set_mode(0)
    return ms, d, launches, aff_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", nargs="*", default=["cfg2", "cfg4"])
    ap.add_argument("--radius", nargs="*", type=int, default=[0, 1, 2, 3, 5, 7])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import torch
    nle = entry.load_package()
    synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
    ctx = nle.Context(0)
    names = {nle.MODE_MATERIALISED_F64: "materialised_f64", nle.MODE_STREAMED_F64: "streamed_f64",
             nle.MODE_PHI_FREE: "tables_f64", nle.MODE_PHI_FREE_EXP: "phi_free_exp", nle.MODE_MATERIALISED: "materialised_f32"}
    out = {"workload": "synthetic integer plane (synthetic.py), T = 10, L = 4, auto mode", "hbm_peak_TBps": HBM_PEAK / 1e12,
           "device": torch.cuda.get_device_name(0), "configs": {}}
    for name in a.cfg:
        cfg = dict(synth.CONFIGS[name])
        cfg["T"], cfg["L"] = 10, 4
        H, W = cfg["H"], cfg["W"]
        x = torch.as_tensor(synth.synthetic_luminance(H, W).astype(np.float32), device="cuda:0")
        g = nle.sample_grid(H, W, cfg["n_row"], cfg["n_col"])
        p = g["n_sel_rows"] * g["n_sel_cols"]
        ldp = nle.ld(p)
        rows = []

        def per_launch(launches, aff_ms):
            if not launches:
                return None, None
            ms = aff_ms / launches
            rows_per = min(CHUNK, H * W)  # every launch but possibly the last covers one chunk
            return ms, rows_per * ldp * 8 / (ms * 1e-3) / HBM_PEAK

        base = None
        if 0 in a.radius:
            _, _, n0, t0 = run(nle, ctx, x, cfg, 0, nle.MODE_MATERIALISED_F64, 1)
            ms0, frac0 = per_launch(n0, t0)
            base = dict(kernel="k_affinity64", launches=n0, per_launch_ms=ms0, hbm_fraction_of_writes=frac0)
        for R in a.radius:
            ms, d, n, t = run(nle, ctx, x, cfg, R, nle.MODE_AUTO, a.reps)
            row = dict(R=R, train_apply_ms=round(ms, 3), formulation=names.get(d["formulation"], d["formulation"]),
                       r_Ka=d["r_Ka"], r_Wa=d["r_Wa"], r_Q=d["r_Q"], K=d["K"])
            if R > 0:
                pl, frac = per_launch(n, t)
                row.update(kernel="k_patch_affinity64", launches=n, per_launch_ms=pl, hbm_fraction_of_writes=frac)
                if base and base["per_launch_ms"]:
                    row["vs_k_affinity64"] = pl / base["per_launch_ms"]
            rows.append(row)
            print(name, json.dumps(row), flush=True)
        out["configs"][name] = dict(H=H, W=W, p=p, ld=ldp, chunk_rows=min(CHUNK, H * W), K=cfg["K"],
                                    k_affinity64_materialised_f64=base, radii=rows)
        if base:
            print(name, "k_affinity64 (R = 0, materialised_f64):", json.dumps(base), flush=True)
    ctx.close()
    if not a.no_write:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
