#!/usr/bin/env python3
"""Cost and effect of the MSE-guided denoiser on one MI355X -> profiles/r25_glide.json.

    kernels   per-launch milliseconds from nle_ctx_kernel_stats (HIP events around the launch) at 4096^2: k_nlm8 at
              (P, S) = (1, 10), (2, 10), (3, 10), the noise kernels, and the reduce half of nle_filter_coefficients for three
              planes; `--reps` launches each after a warm-up launch.  `coefficients_call_ms` is the whole call, host clock
              around a synchronise.  k_nlm8's `gmadds_per_s` counts brute force's (2P + 1)^2 (2S + 1)^2 multiply-adds per pixel,
              the figure the issue quotes, not what the kernel executes (it shares row products between pixels).
    flows     trainForDenoise + denoise composed through the Python mirror, device resident (no file, no upload), cfg4's
              train arguments, sigma colour = sigma space = 10, shrink factor 2, under the four option combinations; the first
              (bilateral, no glide) is the flow this project always had.  Median wall time of `--runs` runs after a warm-up
              run, the combinations alternating.
    quality   PSNR against the clean image on the 64 x 96 piecewise-constant scene of tests/test_glide_denoise.py (Gaussian
              noise, sigma 12, added in BGR): the noisy input, the four combinations, and the image whose three Lab planes
              went through the bilateral filter alone and through non-local means alone.

    python tools/glide_report.py [--out FILE] [--reps N] [--runs N]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "r25_glide.json")
SC, SS, SHRINK = 10, 10, 2.0
QUALITY = dict(shape=(64, 96), seed=7, n_row=8, n_col=12, hx=12.0, hy=15.0, T=10, K=20, k=6.0, sc=10, ss=3)


def nlm_params(sigma):
    """nle::DenoiseOptions' table: P, S, h"""
    return (1 if sigma <= 15 else 2 if sigma <= 30 else 3), 10, (0.40 if sigma <= 30 else 0.35) * sigma


def colour_scene(H, W, seed, sigma=12.0):
    rng = np.random.default_rng(seed)
    rr, cc = np.mgrid[0:H, 0:W]
    region = np.where(cc < 0.4 * W + 0.15 * rr, 0, np.where(rr < 0.55 * H, 1, 2))
    clean = np.array([[40, 40, 160], [200, 180, 60], [150, 230, 240]], dtype=np.float64)[region]
    noisy = np.clip(np.rint(clean + rng.normal(0.0, sigma, clean.shape)), 0, 255)
    return clean.astype(np.uint8), noisy.astype(np.uint8)


def psnr(a, b):
    return 10.0 * math.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def prefilter(ctx, x, nlm, sc, ss):
    """(sigma or None, the pre-filtered plane)"""
    if not nlm:
        return None, ctx.bilateral8(x, sc, ss)
    s = ctx.plane_noise(x)[1]
    P, S, h = nlm_params(s)
    return s, (x.clone() if h == 0 else ctx.nlm8(x, P, S, s, h))


def flow(nle, ctx, d_bgr, q, glide, nlm):
    """NLEFilter::trainForDenoise + denoise with these options, through the mirror: the BGR image on the device"""
    import torch
    H, W = d_bgr.shape[:2]
    lab, L = ctx.bgr2lab8(d_bgr)
    f = nle.NLEFilter(ctx).train_filter(prefilter(ctx, L, nlm, q["sc"], q["ss"])[1], q["n_row"], q["n_col"], q["hx"], q["hy"],
                                        q["T"], q["K"])
    try:
        ev = f.eigvals
        planes = torch.stack([ctx.lab8_channel(lab, ch) for ch in range(3)])
        if not glide:
            resp = np.minimum(ev, 1.0) ** q["k"]
            ab = f.apply_planes(planes[1:], [resp, resp], out_kind=nle.REGION_OUT_ROUNDED8)
            return ctx.lab2bgr8(lab, prefilter(ctx, planes[0], nlm, q["sc"], q["ss"])[1], ab[0].view(H, W), ab[1].view(H, W))
        sig, pres = [], []
        for ch in range(3):
            s, p = prefilter(ctx, planes[ch], nlm, q["sc"], q["ss"])
            sig.append(s if nlm else ctx.plane_noise(planes[ch])[1])
            pres.append(p)
        b = f.coefficients(torch.stack(pres))
        resp = [np.minimum(np.maximum(ev, 0.0), 1.0) ** nle.mse_shrink(ev, b[ch], sig[ch], q["k"], 256)[0] for ch in range(3)]
        y = f.apply_planes(planes, resp, out_kind=nle.REGION_OUT_ROUNDED8)
        return ctx.lab2bgr8(lab, y[0].view(H, W), y[1].view(H, W), y[2].view(H, W))
    finally:
        f.close()


COMBOS = (("bilateral", False, False), ("nlm", False, True), ("glide_bilateral", True, False), ("glide_nlm", True, True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    import torch
    nle = entry.load_package()
    synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
    cfg = synth.CONFIGS["cfg4"]
    H, W = cfg["H"], cfg["W"]
    ctx = nle.Context(0)
    rng = np.random.default_rng(12)
    base = synth.synthetic_luminance(H, W)
    rr, cc = np.mgrid[0:H, 0:W]
    bgr = np.stack([base * 0.8 + 20 * np.sin(cc / 97.0), base, base * 0.9 + 25 * np.cos(rr / 61.0)], axis=-1)
    bgr = np.clip(np.rint(bgr + rng.normal(0.0, 12.0, bgr.shape)), 0, 255).astype(np.uint8)
    d_bgr = torch.as_tensor(bgr, device="cuda:0")
    lab, L = ctx.bgr2lab8(d_bgr)
    res = {"workload": f"{H}x{W}", "noise_sigma_added_bgr": 12.0, "reps": args.reps, "runs": args.runs, "kernels": {}, "flows_ms": {},
           "method": "kernels: nle_ctx_kernel_stats ms / launches (HIP events), one warm-up launch first; flows: median host-clock "
                     "wall time around a device synchronise, combinations alternating, one warm-up run first"}

    def per_launch(name, fn):
        fn()                                   # warm-up
        ctx.profile(True)
        for _ in range(args.reps):
            fn()
        n, ms = ctx.kernel_stats()[name]
        ctx.profile(False)
        return ms / n, n

    sigma_L = ctx.plane_noise(L)[1]
    res["plane_noise_sigma_L"] = round(sigma_L, 4)
    for P in (1, 2, 3):
        ms, n = per_launch("nlm8", lambda: ctx.nlm8(L, P, 10, sigma_L, 0.4 * sigma_L))
        madds = float(H) * W * (2 * P + 1) ** 2 * 21 ** 2
        res["kernels"][f"k_nlm8_P{P}_S10"] = {"ms": round(ms, 3), "launches": n, "gmadds_per_s": round(madds / ms / 1e6, 1)}
    ms, n = per_launch("plane_noise", lambda: ctx.plane_noise(L))
    res["kernels"]["plane_noise_partial_plus_fold"] = {"ms": round(ms, 4), "launches": n,
                                                       "gbytes_per_s": round(4.0 * H * W / ms / 1e6, 1)}
    q4 = dict(n_row=cfg["n_row"], n_col=cfg["n_col"], hx=cfg["hx"], hy=cfg["hy"], T=cfg["T"], K=cfg["K"], k=SHRINK, sc=SC, ss=SS)
    f = nle.NLEFilter(ctx).train_filter(ctx.bilateral8(L, SC, SS), q4["n_row"], q4["n_col"], q4["hx"], q4["hy"], q4["T"], q4["K"])
    planes = torch.stack([ctx.lab8_channel(lab, ch) for ch in range(3)])
    ms, n = per_launch("apply_reduce", lambda: f.coefficients(planes))
    res["kernels"]["coefficients_3_planes_reduce_kernel"] = {"ms": round(ms, 4), "launches": n}
    f.coefficients(planes)
    torch.cuda.synchronize()
    walls = []
    for _ in range(max(args.reps, 3)):
        t0 = time.perf_counter()
        f.coefficients(planes)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    res["kernels"]["coefficients_3_planes_call_ms"] = round(statistics.median(walls), 3)
    f.close()

    for _, glide, nlm in COMBOS:               # warm-up run of every combination
        flow(nle, ctx, d_bgr, q4, glide, nlm)
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in COMBOS}
    for _ in range(args.runs):
        for name, glide, nlm in COMBOS:
            t0 = time.perf_counter()
            flow(nle, ctx, d_bgr, q4, glide, nlm)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    for name in times:
        res["flows_ms"][name] = {"median": round(statistics.median(times[name]), 2), "min": round(min(times[name]), 2),
                                 "max": round(max(times[name]), 2)}

    clean, noisy = colour_scene(*QUALITY["shape"], QUALITY["seed"])
    d_noisy = torch.as_tensor(noisy, device="cuda:0")
    quality = {"noisy": round(psnr(noisy, clean), 3)}
    for name, glide, nlm in COMBOS:
        quality[name] = round(psnr(flow(nle, ctx, d_noisy, QUALITY, glide, nlm).cpu().numpy(), clean), 3)
    qlab, _ = ctx.bgr2lab8(d_noisy)
    for name, nlm in (("bilateral_only", False), ("nlm_only", True)):
        pl = [prefilter(ctx, ctx.lab8_channel(qlab, ch), nlm, QUALITY["sc"], QUALITY["ss"])[1] for ch in range(3)]
        quality[name] = round(psnr(ctx.lab2bgr8(qlab, *pl).cpu().numpy(), clean), 3)
    res["quality_psnr_db"] = quality
    res["quality_scene"] = {k: QUALITY[k] for k in ("shape", "seed", "n_row", "n_col", "hx", "hy", "T", "K", "k", "sc", "ss")}
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
