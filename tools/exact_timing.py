#!/usr/bin/env python3
"""Train-stage times of the exact filter (NLE_MODE_EXACT_F64) -> profiles/r6_exact_timing.json.

    python tools/exact_timing.py                 # every config, one child process each, writes the record
    python tools/exact_timing.py --only flower   # one config, prints its JSON line
    python tools/exact_timing.py --products      # the stage product at N = 65536 (256 x 256), ncols 1, 2, 64, 128: what
                                                 # `rocprofv3 --kernel-trace --stats` times for profiles/r6_exact_kernel_stats.csv

Each config runs in a child process with NLE_TRACE=1, whose stderr line `exact: N .., B block products ..` gives the
operator-application count.  A 32 x 32 exact train warms the code objects first.  Times are nle_filter_timings:
[1] Sinkhorn, [2] the eigensolver's operator products, [3] orthogonalisation + Ritz + V assembly, [4] host algebra,
[5] wall total of the train call.
"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "r6_exact_timing.json")

#        name              plane                    hx     hy    T   K
CONFIGS = [
    ("synthetic_128", ("synthetic", 128, 128), 32.0, 30.0, 10, 30),
    ("synthetic_256", ("synthetic", 256, 256), 64.0, 30.0, 10, 30),
    ("flower", ("flower",), 100.0, 30.0, 50, 30),              # README.md:74, full size (400 x 267)
    ("synthetic_512", ("synthetic", 512, 512), 128.0, 30.0, 10, 30),
    ("rock2_size", ("synthetic", 584, 876), 500.0, 10.0, 50, 50),  # rock2's size (876 x 584) and README arguments
]


def _plane(spec, nle, ctx):
    import numpy as np
    import __graft_entry__ as entry
    if spec[0] == "synthetic":
        synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
        return synth.synthetic_luminance(spec[1], spec[2]).astype(np.float32)
    from PIL import Image
    bgr = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "flower-50.bmp")).convert("RGB"))[..., ::-1].copy()
    lab, _ = ctx.bgr2lab8(bgr)
    return lab[..., 0].cpu().numpy().astype(np.float32)


def child(name):
    import numpy as np
    import __graft_entry__ as entry
    nle = entry.load_package()
    ctx = nle.Context(0)
    ctx.set_mode(nle.MODE_EXACT_F64)
    warm = nle.NLEFilter(ctx).train_filter(np.full((32, 32), 7.0, dtype=np.float32), 2, 2, 8.0, 30.0, 2, 4)
    warm.close()
    spec, hx, hy, T, K = [c[1:] for c in CONFIGS if c[0] == name][0]
    y = _plane(spec, nle, ctx)
    f = nle.NLEFilter(ctx).train_filter(y, 2, 2, hx, hy, T, K)
    ms = f.timings()
    print(json.dumps({"name": name, "H": int(y.shape[0]), "W": int(y.shape[1]), "N": int(y.size), "hx": hx, "hy": hy, "T": T,
                      "K": K, "K_kept": f.info()["K"], "lambda_1": float(f.eigvals[0]), "lambda_K": float(f.eigvals[-1]),
                      "ms": {"sinkhorn": ms["sinkhorn"], "products": ms["gram"], "ortho_ritz_v": ms["project"],
                             "host": ms["host"], "total": ms["total"]}}), flush=True)
    f.close()
    ctx.close()


def products():
    """the stage product at N = 65536 with ncols 1, 2, 64, 128: one warm-up and one timed call each"""
    import numpy as np
    import torch
    import __graft_entry__ as entry
    nle = entry.load_package()
    synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
    ctx = nle.Context(0)
    y = synth.synthetic_luminance(256, 256).astype(np.float32)
    for nc in (1, 2, 64, 128):
        X = torch.ones((y.size, nc), dtype=torch.float64, device="cuda:0")
        for _ in range(2):
            ctx.affinity_product64(y, X, 64.0, 30.0)
        torch.cuda.synchronize()
        print("product ncols", nc, "done", flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only")
    ap.add_argument("--child")
    ap.add_argument("--products", action="store_true")
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.child)
        return
    if a.products:
        products()
        return
    rows = []
    for name, *_ in CONFIGS:
        if a.only and name != a.only:
            continue
        env = dict(os.environ, NLE_TRACE="1")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], capture_output=True, text=True,
                           env=env, timeout=900)
        if r.returncode != 0:
            print(r.stdout, r.stderr, file=sys.stderr)
            raise SystemExit(f"{name}: child exited {r.returncode}")
        row = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        m = re.findall(r"exact: N (\d+), (\d+) block products of up to (\d+) columns \(x2\), (\d+) restarts", r.stderr)
        N, B, b, rs = (int(v) for v in m[-1])  # the last train of the child is the measured one
        row.update(block_products=B, block_columns=b, product_columns=2 * b, restarts=rs)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if not a.no_write and not a.only:
        with open(OUT, "w") as fh:
            json.dump({"tool": "tools/exact_timing.py", "device": "MI355X", "configs": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
