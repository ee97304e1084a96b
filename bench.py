#!/usr/bin/env python3
"""Headline benchmark: megapixels/s end-to-end enhance (BASELINE.json `metric`).

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

One "step" = one pass of the hot path over one synthetic luminance plane that is already
resident in HBM: NLEFilter::trainFilter (affinity blocks -> Nystrom -> Sinkhorn -> orthogonalise)
followed by the per-layer spectral recomposition (NLEFilter::apply, one output plane per layer),
through the C ABI of libnle_hip.so.  Workload = BASELINE.json configs[3] ("cfg4": 4096x4096,
20x10 = 200 samples, K = 50, T = 10, L = 4), the configuration the metric is quoted on.

N > 1: the SAME image is sharded by image-row slabs over the ranks (strong scaling); the only
exchange steps are the small fp64 all-reduces of the Sinkhorn column sums, the Gram partials and
V^T x (torch.distributed "nccl" == RCCL over xGMI).

`value` is the HBM-resident figure (the bench contract: inputs already in HBM when the timed region starts);
`ms_per_step` the milliseconds of one timed step.  A plain run does only that: set up, `--warmup` steps, `--steps` timed
steps, the outputs if `--dump-outputs DIR` is given, and the JSON line.

--dump-outputs DIR  after the timed steps, what the last timed step computed, as .npy files:
                layers.npy   float32 (L, n) the L per-layer planes (this rank's pixels, row-major); a plane larger than
                             the 64 MB budget is replaced by a fixed sample of its pixels (numpy default_rng(0), sorted,
                             the same pixels on every layer), so that the file stays comparable between builds;
                eigvals.npy  float64 (K,) the eigenvalues the trained filter kept.
                N > 1: every rank writes its own `layers_rank<r>.npy`; rank 0 writes `eigvals.npy`.
                The input plane is the seeded synthetic plane of the config: the same arguments give the same inputs.

--full adds, in the same run, everything else the benchmark measures and checks (the options that tune these legs
act only with --full):
  kernels, roofline  per-kernel HIP-event times of the timed region (nle_ctx_profile, recorded on the stream the
                kernels run on; the events cost the timed steps some stream gaps) and the dominant kernel's
                algorithmic bytes (or flops) per launch divided by its average launch duration, against the MI355X peak;
  host_to_host  SURVEY.md section 8d's own metric -- wall time from the fp32 plane in HOST memory to the L per-layer
                planes back in HOST memory: H2D + train + apply + D2H, median of >= 5 runs after 2 warm-ups
                (nle_train_host + nle_apply_layers_host on page-locked buffers; one upload, the download of a finished
                layer overlapped with the next one's kernels), and its 8-bit forms;
  soak, pipelined, affinity_pass  steps after the timed region, images in flight, the stand-alone affinity passes;
  cpu_baseline  oracle/nle_cpu_baseline.cpp (a port of the reference's algorithm) timed on this box's host cores
                (rank 0, N = 1 only);
  N > 1: shard_check (the sharded output against a single-GPU run, before anything is timed) and replicas.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.29 TB/s measured copy)
FP32_PEAK_TF = 157.3        # MI355X_MICROARCH.md: fp32-input MFMA == fp32 vector peak
FP64_MFMA_PEAK_TF = 78.6    # MI355X FP64 matrix peak (spec; SURVEY.md section 8d quotes ~79 TFLOP/s fp64)
LDS_F64_ATOMIC_PEAK = 1.49e12  # measured: tools/micro/lds_atomic_bench.hip, ds_add_f64 on a 256 x 11 histogram, random levels


def gram_on_index_sums(grid, W, hx):
    """mirror of sorted_gsum_ok (csrc/sorted.hip): on the equispaced sample grid the Gram stage runs on 2 nC - 1 index-sum
    tables per image row and 2 nR - 1 GEMM rows instead of nC (nC + 1) / 2 and nR (nR + 1) / 2"""
    if os.environ.get("NLE_GRAM_PAIRS") or W > 8192:
        return False
    cs, nC = float(grid["col_step"]), float(grid["n_sel_cols"])
    return 2.0 * W * W / (hx * hx) < 600.0 and (2.0 * cs * W + 2.0 * nC * cs * cs) / (hx * hx) < 600.0


def roofline_models(info, L, form, grid, lazy=False, gsum=False, level_tiles=16):
    """kernel name -> (bound, algorithmic units per launch, peak) for this rank (n = pixels of its slab).

    Per-unit figures are SURVEY.md section 8(d)'s (fp32 storage, s = 4 B) where the kernel still does the
    work that formula describes.  `form`:
      materialised     Phi streamed: Sinkhorn B_C/(2T) = n r s bytes per pass (HBM), GEMMs on the fp32 MFMA
      phi_free_exp     affinities regenerated: Sinkhorn pass = n p (8 flop + 1 exp + 4 flop) on the fp32 vector
                       pipe ("valu", 157.3 TFLOP/s, the same figure as the fp32 MFMA), Gram/projection on
                       the fp64 MFMA with r -> p
      phi_free_tables  quantised luminance: the Sinkhorn and Gram passes are table look-ups whose own
                       traffic/flops are listed (they are LDS-atomic / latency bound, far from either roof);
                       the projection is the fp64-MFMA Nystrom-extension GEMM F_E = 2 n p K."""
    n, r, p, K = info["n_local"], info["r"], info["p"], info["K"]
    nC, nR = grid["n_sel_cols"], grid["n_sel_rows"]
    rows = info["row1"] - info["row0"]
    s = 4.0
    m = {
        "affinity": ("hbm", n * s * (1 + p), HBM_PEAK_GBS),              # B_A = N s (1 + p)
        "apply_reduce": ("hbm", n * s * (K + 1), HBM_PEAK_GBS),          # B_F, first pass: V and x
        "apply_expand": ("hbm", n * s * (K + L), HBM_PEAK_GBS),          # B_F, second pass: V in, L planes out
    }
    if form == "materialised":
        m["nystrom_extend"] = ("mfma", 2.0 * n * p * r, FP32_PEAK_TF)    # F_B = 2 N p r
        m["sinkhorn_pass"] = ("hbm", n * r * s, HBM_PEAK_GBS)            # B_C / (2T)
        m["gram"] = ("mfma", 2.0 * n * r * r, FP32_PEAK_TF)              # F_D = 2 N r^2
        m["project"] = ("mfma", 2.0 * n * r * K, FP32_PEAK_TF)           # F_E = 2 N r K
    else:
        m["project"] = ("mfma", 2.0 * n * p * K, FP64_MFMA_PEAK_TF)      # F_E with r -> p, fp64 MFMA
        if form == "phi_free_exp":
            m["sinkhorn_pass"] = ("valu", n * p * (8.0 + 1.0 + 4.0), FP32_PEAK_TF)
            m["gram"] = ("mfma", 2.0 * n * p * p, FP64_MFMA_PEAK_TF)     # F_D with r -> p
        else:
            # one (16 level_tiles) x nC fp64 table per image row: the columns of 16-level tiles that do not occur in the
            # plane are neither made, stored nor contracted (nle_filter_level_tiles; 12 of 16 on the synthetic plane)
            tab = rows * 16.0 * level_tiles * nC * 8.0
            npair = nC * (nC + 1) / 2.0
            ldm = ((nR * (nR + 1) // 2) + 15) // 16 * 16
            m["sink_tables"] = ("hbm", tab, HBM_PEAK_GBS)                # g written
            # level-sorted rows (sorted.hip): 2 B of sorted column index per pixel + the row's chunk table (512 x 8 B
            # + 516 B) instead of 4 B of luminance
            srt = n * 2.0 + rows * (512 * 8.0 + 516.0)
            m["sinkhorn_pass"] = ("hbm", srt + 2.0 * tab, HBM_PEAK_GBS)  # sorted row + g in + h out
            if gsum:  # index sums: 2 nC - 1 tables per image row, GEMM with 2 nR - 1 (padded to 16) rows
                ntab, ldm = 2.0 * nC - 1.0, ((2 * nR - 1) + 15) // 16 * 16
            else:
                ntab = npair
            m["gram_rows"] = ("hbm", srt + n * 8.0 + rows * 16.0 * level_tiles * ntab * 8.0, HBM_PEAK_GBS)
            m["gram_gemm"] = ("mfma", 2.0 * ldm * 256.0 * ntab * rows, FP64_MFMA_PEAK_TF)
            if lazy:  # V stays implicit: apply runs on the tables too (bytes the two kernels really move)
                m["apply_reduce"] = ("hbm", srt + n * (8.0 + s) + tab, HBM_PEAK_GBS)      # sorted row, c, x in; h out
                lb = max(1, min(L, 4, (144 * 1024) // (256 * (nC | 1) * 8)))             # layers per expand launch
                W_img = n / max(rows, 1)
                px_in = srt if (nC <= 12 and W_img <= 4096) else n * s   # k_sorted_expand reads the sorted row, k_hist_dot the luminance
                m["apply_expand"] = ("hbm", px_in + n * 8.0 + lb * (tab + n * s), HBM_PEAK_GBS)  # pixels, c; per layer g in, y out
    return m


def load_traffic():
    """HBM bytes per launch from the COMMITTED PMC summary (tools/prof.sh + tools/pmc_summary.py):
    ({kernel-name substring: bytes}, file name); rocprofv3 cannot run inside bench.py, so `traffic` is a record of an
    earlier run of the same command, not a measurement of this one -- the line says so (`traffic_source`)."""
    import csv
    import glob
    out = {}
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_final_hbm_traffic.csv")))   # the newest round's final run
    if not files:
        return out, None
    for row in csv.DictReader(open(files[-1])):
        out[row["kernel"]] = float(row["hbm_bytes_per_launch"])
    return out, os.path.relpath(files[-1], ROOT)


def kernel_symbols(form, lazy):
    """bench kernel name -> substrings of the HIP kernel symbol that ran for it (for the PMC table)"""
    if form == "materialised":
        return {"nystrom_extend": ("k_tsgemm<7, true>",), "sinkhorn_pass": ("k_rowpass<8",), "gram": ("k_gram(",),
                "project": ("k_tsgemm<2, false>",), "apply_expand": ("k_apply_expand",),
                "apply_reduce": ("k_rowpass<4",), "affinity": ("k_affinity",)}
    sym = {"project": ("k_project64_res", "k_project64"), "apply_expand": ("k_apply_expand",),
           "apply_reduce": ("k_rowpass<4",)}
    if form == "phi_free_exp":
        sym.update({"sinkhorn_pass": ("k_sink_pass",), "gram": ("k_gram64",)})
    else:
        sym.update({"sinkhorn_pass": ("k_sorted_pass", "k_hist_pix"), "sink_tables": ("k_hist_g",),
                    "gram_rows": ("k_sorted_gsum", "k_sorted_gram", "k_ghist_rows"), "gram_gemm": ("k_ghist_gemm",)})
        if lazy:  # the apply's reduce half is the pass kernel in its XVEC mode: same symbol as the Sinkhorn pass
            sym.update({"apply_expand": ("k_sorted_expand", "k_hist_dot"), "apply_reduce": ("k_sorted_pass", "k_hist_pix")})
    return sym


DUMP_BYTES = 60 << 20   # --dump-outputs: payload of all files together, under 64 MB with the .npy headers


def dump_outputs(path, out, eigvals, rank, world):
    """--dump-outputs: this rank's L layer planes of the last timed step (float32; a fixed seeded sample of its pixels when
    the planes exceed the budget) and the filter's eigenvalues (float64), as DIR/<name>.npy"""
    import torch
    os.makedirs(path, exist_ok=True)
    L, n = out.shape
    ev = np.ascontiguousarray(eigvals, dtype=np.float64)
    keep = min(n, (DUMP_BYTES - ev.nbytes) // world // (4 * L))
    if keep < n:
        idx = np.sort(np.random.default_rng(0).choice(n, keep, replace=False))
        out = out.index_select(1, torch.as_tensor(idx, device=out.device))
    np.save(os.path.join(path, "layers.npy" if world == 1 else f"layers_rank{rank}.npy"), out.float().cpu().numpy())
    if rank == 0:
        np.save(os.path.join(path, "eigvals.npy"), ev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beside the headline figure (per-kernel times and roofline, "
                         "host-to-host, soak, images in flight, affinity passes, CPU baseline; N > 1: shard check, replicas)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy (layers.npy, eigvals.npy)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl == RCCL; gloo for rehearsals)")
    ap.add_argument("--comm", default="rccl", choices=["rccl", "torch"],
                    help="N > 1: 'rccl' = the library's own ncclAllReduce on its stream (communicator bootstrapped over "
                         "torch.distributed); 'torch' = torch.distributed.all_reduce through the callback ABI")
    ap.add_argument("--no-replicas", action="store_true", help="N > 1: skip the replica-throughput leg")
    ap.add_argument("--no-pipelined", action="store_true", help="N = 1: skip the images-in-flight throughput leg")
    ap.add_argument("--no-affinity", action="store_true", help="N = 1: skip the stand-alone affinity-pass roofline legs")
    ap.add_argument("--full-plane-input", action="store_true",
                    help="N > 1: every rank holds the whole plane (default: slab input, a rank holds and uploads its rows only)")
    ap.add_argument("--same-device", action="store_true",
                    help="rehearsal on a 1-GPU box: every rank uses cuda:0 (needs --backend gloo)")
    ap.add_argument("--simulate-world", type=int, default=0,
                    help="timing only, one GPU: run rank 0 of a W-way row shard whose 'all-reduce' scales the rank's partial sums "
                         "by W (results are meaningless, the per-rank compute time at 1/W of the rows is not)")
    ap.add_argument("--inflight", type=int, default=1, help="images in flight on one GPU (throughput mode, opt-in)")
    ap.add_argument("--mode", type=int, default=0, help="0 auto, 1 materialised Phi, 2 Phi-free (NLE_MODE_*)")
    ap.add_argument("--h2h-runs", type=int, default=7, help="host-to-host (section 8d) runs after 2 warm-ups; 0 skips")
    ap.add_argument("--soak-seconds", type=float, default=5.0,
                    help="N = 1: after the timed region keep stepping for this long (reported as `soak`; 0 skips) -- the timed "
                         "region alone is ~0.2 s, too short for an external GPU-busy sampler to see")
    ap.add_argument("--allow-callback-fallback", action="store_true",
                    help="N > 1: if the native RCCL communicator cannot be created, time the torch.distributed callback path "
                         "instead of exiting non-zero")
    ap.add_argument("--cpu-sample", type=int, default=768, help="side of the CPU-baseline sample image")
    ap.add_argument("--cpu-threads", type=int, default=16, help="BLAS threads for the CPU baseline (<= visible cores)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    import torch

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with torch.distributed.run --nproc-per-node N for --gpus N")
    if args.same_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist_mod
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist_mod.init_process_group("nccl", device_id=torch.device(f"cuda:{local_rank}"))
        else:
            dist_mod.init_process_group(args.backend)
        dist = dist_mod

    nle = entry.load_package()
    from importlib import import_module  # noqa: F401
    synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
    cfg = dict(synth.CONFIGS[args.config])
    H, W, L = cfg["H"], cfg["W"], cfg["L"]

    ctx = nle.Context(local_rank)
    ctx.set_mode(args.mode)
    g = nle.sample_grid(H, W, cfg["n_row"], cfg["n_col"])
    p = g["n_sel_rows"] * g["n_sel_cols"]
    comm_kind = "none"
    rccl_ranks = 0
    if world > 1:
        comm_kind = "torch.distributed all_reduce via callback"
        if args.comm == "rccl" and args.backend == "nccl" and not args.same_device:
            # bootstrap: rank 0's ncclUniqueId travels over the torch process group, then every rank joins the
            # library's own communicator; from here on the data path never enters Python
            uid = torch.zeros(128, dtype=torch.uint8, device=f"cuda:{local_rank}")
            if rank == 0:
                uid = torch.tensor(list(nle.rccl_unique_id()), dtype=torch.uint8, device=f"cuda:{local_rank}")
            dist.broadcast(uid, 0)
            ok = 1
            try:
                ctx.init_rccl(rank, world, bytes(uid.cpu().tolist()))
            except Exception as e:  # noqa: BLE001
                ok = 0
                print(f"[bench] rank {rank}: native RCCL init failed ({e!r})", file=sys.stderr, flush=True)
            # every rank must take the same path: agree on the outcome over the torch process group
            okt = torch.tensor([ok], dtype=torch.int32, device=f"cuda:{local_rank}")
            dist.all_reduce(okt, op=dist.ReduceOp.MIN)
            if int(okt.item()) == 1:
                comm_kind = "native RCCL (ncclAllReduce in place on the ctx stream)"
                rccl_ranks = world
            elif not args.allow_callback_fallback:
                # a silent fall-back would time a different data path than the one the line claims: fail loudly, in every rank
                print(f"[bench] rank {rank}: no native RCCL communicator on every rank; exiting (--allow-callback-fallback "
                      "times the torch callback path instead)", file=sys.stderr, flush=True)
                dist.destroy_process_group()
                sys.exit(3)
            else:
                ctx.close()            # a half-initialised communicator is not reused
                ctx = nle.Context(local_rank)
                ctx.set_mode(args.mode)
        if comm_kind.startswith("torch"):
            ctx.set_shard(rank, world, p, lambda t: dist.all_reduce(t))
    elif args.simulate_world > 1:
        # rank 0 of a W-way shard without its peers: the "all-reduce" scales this rank's partial sums by W -- what the sum over
        # W statistically alike slabs comes to -- so that the p-sized algebra sees matrices like the real run's (left
        # unscaled they are a different problem: at cfg5 the 1e-10 cut then removes 145 eigenvalues of Wa instead of 100
        # and the solver takes another route)
        sw_ = float(args.simulate_world)
        ctx.set_shard(0, args.simulate_world, p, lambda t: t.mul_(sw_))

    lum = torch.as_tensor(synth.synthetic_luminance(H, W).astype(np.float32), device=f"cuda:{local_rank}")
    n_local = ctx.local_pixels(H, W)
    out = torch.empty((L, n_local), dtype=torch.float32, device=lum.device)
    flt = nle.NLEFilter(ctx)
    # N > 1: a rank keeps only its own rows of the image (nle_ctx_set_slab_input); the p sample values travel in one
    # small all-reduce
    slab_input = world > 1 and not args.full_plane_input
    lum_in = lum
    if slab_input:
        ctx.set_slab_input(True)
        r0_, r1_ = nle.slab_rows(H, rank, world)
        lum_in = lum[r0_:r1_].contiguous()

    def step():
        flt.train_filter(lum_in, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], cfg["T"], cfg["K"], shape=(H, W))
        flt.apply_layers(lum_in, L, out=out)

    def fence():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # --inflight M (opt-in, single GPU): M images in flight, each on its own ctx/stream/host thread, so that one
    # image's p-sized host algebra overlaps another's kernels.  Throughput mode; the default (1) is the latency
    # of one image, which is what `value` is quoted on.
    lanes = [(ctx, flt, out)]
    for _ in range(1, args.inflight):
        c2 = nle.Context(local_rank)
        c2.set_mode(args.mode)
        lanes.append((c2, nle.NLEFilter(c2), torch.empty_like(out)))

    def run_steps(n):
        if len(lanes) == 1:
            for _ in range(n):
                step()
            return
        import threading

        def work(i):
            torch.cuda.set_device(local_rank)
            _, f_i, o_i = lanes[i]
            for _ in range(i, n, len(lanes)):
                f_i.train_filter(lum, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], cfg["T"], cfg["K"])
                f_i.apply_layers(lum, L, out=o_i)
        th = [threading.Thread(target=work, args=(i,)) for i in range(len(lanes))]
        for t_ in th:
            t_.start()
        for t_ in th:
            t_.join()

    run_steps(args.warmup * len(lanes))
    # N > 1: before anything is timed, this rank's rows of the sharded result against the same rows of an unsharded run on
    # this GPU (only the order of the fp64 sums differs between the two; the test suite's bar for that is 1e-6)
    shard_check = None
    if world > 1 and args.full:
        c1 = nle.Context(local_rank)
        c1.set_mode(args.mode)
        f1 = nle.NLEFilter(c1)
        f1.train_filter(lum, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], cfg["T"], cfg["K"])
        full = f1.apply_layers(lum, L)
        r0_, r1_ = nle.slab_rows(H, rank, world)
        mine = full[:, r0_ * W:r1_ * W]
        errs = [float(torch.linalg.norm(out[j].double() - mine[j].double()) / torch.linalg.norm(mine[j].double())) for j in range(L)]
        worst = torch.tensor([max(errs)], dtype=torch.float64, device=lum.device)
        dist.all_reduce(worst, op=dist.ReduceOp.MAX)
        shard_check = {"max_rel_l2_per_layer_vs_single_gpu": float(worst.item()), "matches": bool(worst.item() <= 1e-6)}
        del full, mine
        f1.close()
        c1.close()
        if not shard_check["matches"]:
            print(f"[bench] rank {rank}: sharded output differs from the single-GPU result ({shard_check})", file=sys.stderr, flush=True)
            dist.destroy_process_group()
            sys.exit(4)
    if args.full:
        for c_, _, _ in lanes:
            c_.profile(1)   # HIP events around the N-sized kernels of the timed region
    fence()
    t0 = time.perf_counter()
    run_steps(args.steps)
    fence()
    elapsed = time.perf_counter() - t0
    stats = {}
    if args.full:
        for c_, _, _ in lanes:
            for k_, (n_, ms_) in c_.kernel_stats().items():
                a_ = stats.get(k_, (0, 0.0))
                stats[k_] = (a_[0] + n_, a_[1] + ms_)
            c_.profile(False)
    info = flt.info()
    stage_ms = flt.timings()
    if args.dump_outputs:
        _, f_last, out_last = lanes[(args.steps - 1) % len(lanes)]   # the lane that ran the last timed step
        dump_outputs(args.dump_outputs, out_last, f_last.eigvals, rank, world)
    soak = None
    if world == 1 and args.full and args.soak_seconds > 0 and args.simulate_world <= 1 and len(lanes) == 1:
        ts_, t_end = [], time.perf_counter() + args.soak_seconds
        while time.perf_counter() < t_end:
            t1_ = time.perf_counter()
            step()
            ts_.append(time.perf_counter() - t1_)      # apply_layers returns when the layers are written
        fence()
        a_ = np.sort(np.asarray(ts_)) * 1e3
        soak = {"steps": int(a_.size), "seconds": float(a_.sum() / 1e3), "ms_median": float(np.median(a_)),
                "ms_p99": float(a_[min(a_.size - 1, int(0.99 * a_.size))]), "ms_max": float(a_[-1]),
                "what": "consecutive train + apply steps on the same ctx right after the timed region (not part of `value`)"}
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=lum.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    ms_per_step = elapsed * 1e3 / args.steps
    value = (H * W / 1e6) / (elapsed / args.steps)

    # ---- N > 1, second leg: replicas -- every rank filters its OWN image, no collective in the data path (weak scaling)
    replicas = None
    if world > 1 and args.full and not args.no_replicas and args.simulate_world <= 1:
        c_r = nle.Context(local_rank)
        c_r.set_mode(args.mode)
        f_r = nle.NLEFilter(c_r)
        out_r = torch.empty((L, H * W), dtype=torch.float32, device=lum.device)
        for _ in range(args.warmup):
            f_r.train_filter(lum, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], cfg["T"], cfg["K"])
            f_r.apply_layers(lum, L, out=out_r)
        fence()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            f_r.train_filter(lum, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], cfg["T"], cfg["K"])
            f_r.apply_layers(lum, L, out=out_r)
        fence()
        tr_ = torch.tensor([time.perf_counter() - t1], dtype=torch.float64, device=lum.device)
        dist.all_reduce(tr_, op=dist.ReduceOp.MAX)
        el_r = float(tr_.item())
        replicas = {"value": world * (H * W / 1e6) / (el_r / args.steps), "unit": "MP/s", "scaling": "weak",
                    "ms_per_step": el_r * 1e3 / args.steps,
                    "what": f"{world} independent images, one per GPU, no collective in the data path"}
        f_r.close()
        c_r.close()

    # ---- throughput with several images in flight (N = 1): each image on its own ctx / stream / host thread, so that one
    # image's p-sized host algebra (W_A root, eig(Q): ~2.7 ms of the 7.5) runs under another image's kernels.  Reported
    # beside `value`, which stays the one-image-at-a-time figure.
    pipelined = None
    if world == 1 and args.full and args.simulate_world <= 1 and args.inflight == 1 and not args.no_pipelined:
        import threading
        pipelined = []
        for M in (2, 3):
            pl = []
            for _ in range(M):
                c2 = nle.Context(local_rank)
                c2.set_mode(args.mode)
                pl.append((c2, nle.NLEFilter(c2), torch.empty_like(out)))

            def work(i, n, pl=pl, M=M):
                torch.cuda.set_device(local_rank)
                _, f_i, o_i = pl[i]
                for _ in range(i, n, M):
                    f_i.train_filter(lum, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], cfg["T"], cfg["K"])
                    f_i.apply_layers(lum, L, out=o_i)

            def run(n):
                th = [threading.Thread(target=work, args=(i, n)) for i in range(M)]
                for t_ in th:
                    t_.start()
                for t_ in th:
                    t_.join()
            nimg = max(3 * args.steps, 12)   # enough images for the pipeline's start-up and drain to wash out
            run(2 * M)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            run(nimg)
            torch.cuda.synchronize()
            el = time.perf_counter() - t1
            same = bool(torch.equal(pl[0][2], out))
            pipelined.append({"images_in_flight": M, "value": (H * W / 1e6) * nimg / el, "unit": "MP/s",
                              "ms_per_image": el * 1e3 / nimg, "images": nimg, "matches_single_image_output": same})
            for c2, f2_, _ in pl:
                f2_.close()
                c2.close()

    # ---- SURVEY.md section 8d's metric: host plane -> host layers, median of >= 5 runs after 2 warm-ups.  N > 1 (slab
    # input): every rank uploads its own rows and downloads its own rows of the layers, max over ranks per run
    h2h = None
    if (world == 1 or slab_input) and args.full and args.simulate_world <= 1 and args.h2h_runs > 0:
        rows0, rows1 = nle.slab_rows(H, rank, world) if world > 1 else (0, H)
        h_lum = ctx.host_alloc((rows1 - rows0, W))
        h_lum[...] = synth.synthetic_luminance(H, W).astype(np.float32)[rows0:rows1]
        h_out = ctx.host_alloc((L, n_local))
        f2 = nle.NLEFilter(ctx)
        ts = []
        for it in range(2 + args.h2h_runs):
            fence()
            t1 = time.perf_counter()
            f2.train_filter_host(h_lum, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], cfg["T"], cfg["K"], shape=(H, W))
            f2.apply_layers_host(None, L, h_out)          # returns when the last layer is in host memory
            ts.append(time.perf_counter() - t1)
        ts = ts[2:]
        if dist is not None:
            tt = torch.tensor(ts, dtype=torch.float64, device=lum.device)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            ts = tt.tolist()
        ref = out.cpu().numpy()
        same = bool(np.array_equal(ref, h_out))
        h2h_diff = 0.0 if same else float(np.abs(ref - h_out).max() / max(np.abs(ref).max(), 1e-30))
        med = float(np.median(ts))
        h2h = {"value": (H * W / 1e6) / med, "unit": "MP/s", "ms_median": med * 1e3, "ms_min": min(ts) * 1e3,
               "ms_max": max(ts) * 1e3, "runs": len(ts), "warmup": 2,
               "bytes_h2d": int(h_lum.nbytes), "bytes_d2h": int(h_out.nbytes),
               "what": "SURVEY.md section 8d: fp32 plane in page-locked host memory -> train -> L per-layer planes back in "
                       "page-locked host memory, one image at a time (nle_train_host + nle_apply_layers_host)"
                       + ("; per rank: its own rows up, its own rows of the layers down; max over ranks" if world > 1 else ""),
               "matches_device_resident_output": same, "max_rel_diff_vs_device_resident_output": h2h_diff}
        # the same path with what `enhance` actually brings home (src/filter.cpp:428-436): the weighted sum of the layers,
        # clamped and rounded to ONE 8-bit plane on the device (nle_apply_u8_host) -- N bytes down instead of 4 L N
        wts = {4: [2.0, 3.0, 4.0, 1.0], 6: [2.0, 3.0, 3.0, 4.0, 4.0, 1.0]}.get(L, [2.0] * (L - 1) + [1.0])
        h_u8 = ctx.host_alloc((n_local,), dtype=np.uint8)
        ts8 = []
        for it in range(2 + args.h2h_runs):
            fence()
            t1 = time.perf_counter()
            f2.train_filter_host(h_lum, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], cfg["T"], cfg["K"], shape=(H, W))
            f2.apply_u8_host(None, nle.transform_eigenvalues(f2.eigvals, wts), h_u8)
            ts8.append(time.perf_counter() - t1)
        ts8 = ts8[2:]
        if dist is not None:
            tt = torch.tensor(ts8, dtype=torch.float64, device=lum.device)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            ts8 = tt.tolist()
        want8 = torch.round(torch.clamp(sum(float(w_) * out[j] for j, w_ in enumerate(wts)), 0, 255))
        d8 = (want8 - torch.as_tensor(h_u8, device=lum.device).float()).abs()
        med8 = float(np.median(ts8))
        h2h["u8_plane"] = {"value": (H * W / 1e6) / med8, "unit": "MP/s", "ms_median": med8 * 1e3, "ms_min": min(ts8) * 1e3,
                           "runs": len(ts8), "bytes_h2d": int(h_lum.nbytes), "bytes_d2h": int(h_u8.nbytes), "weights": wts,
                           "what": "the same host plane -> train -> ONE clamped, rounded 8-bit plane of the weighted layer sum back in "
                                   "host memory (nle_train_host + nle_apply_u8_host): what NLEFilter::enhance merges back",
                           "pixels_differing_from_the_rounded_sum_of_the_fp32_layers": int((d8 > 0).sum().item()),
                           "max_level_difference": float(d8.max().item())}
        # and from the 8-bit plane itself (what getLuminanceChannel hands over, src/filter.cpp:460-469): N bytes up, N bytes down
        h_in8 = ctx.host_alloc((rows1 - rows0, W), dtype=np.uint8)
        h_in8[...] = h_lum.astype(np.uint8)
        h_u8b = ctx.host_alloc((n_local,), dtype=np.uint8)
        ts88 = []
        for it in range(2 + args.h2h_runs):
            fence()
            t1 = time.perf_counter()
            f2.train_filter_host_u8(h_in8, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], cfg["T"], cfg["K"], shape=(H, W))
            f2.apply_u8_host(None, nle.transform_eigenvalues(f2.eigvals, wts), h_u8b)
            ts88.append(time.perf_counter() - t1)
        ts88 = ts88[2:]
        if dist is not None:
            tt = torch.tensor(ts88, dtype=torch.float64, device=lum.device)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            ts88 = tt.tolist()
        med88 = float(np.median(ts88))
        h2h["u8_in_u8_out"] = {"value": (H * W / 1e6) / med88, "unit": "MP/s", "ms_median": med88 * 1e3, "ms_min": min(ts88) * 1e3,
                               "runs": len(ts88), "bytes_h2d": int(h_in8.nbytes), "bytes_d2h": int(h_u8b.nbytes),
                               "what": "the 8-bit luminance plane up (nle_train_host_u8), the 8-bit filtered plane down "
                                       "(nle_apply_u8_host): one byte per pixel each way",
                               "equals_the_fp32_input_path": bool(np.array_equal(h_u8b, h_u8))}
        f2.close()

    # ---- roofline of the dominant kernel (this rank's launches; --full only: it needs the HIP events of the timed region)
    ran = {k for k, v in stats.items() if v[0] > 0}
    form = "materialised" if "nystrom_extend" in ran else ("phi_free_tables" if "gram_gemm" in ran else "phi_free_exp")
    formulation = flt.diag()["formulation"]
    form_label = {1: "materialised_f32", 2: "phi_free_tables", 3: "phi_free_exp_f32", 4: "materialised_f64",
                  5: "streamed_f64 (no N x r matrix: fp64 affinity rows regenerated chunk by chunk)"}.get(formulation, form)
    lazy = form == "phi_free_tables" and "project" not in ran      # whether V stayed implicit: known from the events only
    per_kernel, roofline = None, None
    if args.full:
        gsum = form == "phi_free_tables" and gram_on_index_sums(g, W, cfg["hx"])
        lev_t0, lev_nt = flt.level_tiles()
        models = roofline_models(info, L, form, g, lazy, gsum, lev_nt)
        # (the committed PMC summary was collected at N = 1 on the default config: per-launch bytes of a row slab or of
        # another config differ, so `traffic` is only attached to that case)
        traffic, traffic_file = load_traffic() if (world == 1 and args.config == "cfg4" and args.simulate_world <= 1) else ({}, None)
        per_kernel = {}
        for name, (launches, total_ms) in stats.items():
            if launches == 0:
                continue
            avg_ms = total_ms / launches
            rec = {"launches_per_step": launches / args.steps, "avg_ms": avg_ms, "total_ms_per_step": total_ms / args.steps}
            if name in models:
                bound, units, peak = models[name]
                if bound == "hbm":
                    ach, unit = units / (avg_ms * 1e-3) / 1e9, "GB/s"
                else:
                    ach, unit = units / (avg_ms * 1e-3) / 1e12, "TFLOP/s"
                rec.update({"bound": bound, "achieved": ach, "peak": peak, "unit": unit, "frac": ach / peak})
                if name == "sinkhorn_pass" and form != "materialised":
                    rec["hbm_equivalent_GBs"] = info["n_local"] * info["r"] * 4.0 / (avg_ms * 1e-3) / 1e9
                if form == "phi_free_tables" and name in ("sinkhorn_pass", "apply_reduce", "gram_rows"):
                    # what bounds the level-sorted pixel kernels: fp64 multiply-adds on the vector pipe (2 nC per pixel
                    # for a pass + the reciprocal; for the Gram nC(nC+1)/2 + nC in the pair form, a recurrence step + an add per
                    # index-sum table otherwise) and nC LDS table reads per pixel
                    nc_ = g["n_sel_cols"]
                    fma = (2 * nc_ + 8) if name != "gram_rows" else ((2 * (2 * nc_ - 1) + 2) if gsum else (nc_ * (nc_ + 1) // 2 + nc_))
                    rec["valu_f64"] = {"achieved": 2.0 * fma * info["n_local"] / (avg_ms * 1e-3) / 1e12, "peak": FP64_MFMA_PEAK_TF,
                                       "unit": "TFLOP/s (fp64 vector == matrix peak)",
                                       "frac": 2.0 * fma * info["n_local"] / (avg_ms * 1e-3) / 1e12 / FP64_MFMA_PEAK_TF}
                rec["traffic"] = None
                for sym in kernel_symbols(form, lazy).get(name, ()):
                    hit = [v for k, v in traffic.items() if sym in k]
                    if hit:
                        rec["traffic"] = hit[0]
                        break
            per_kernel[name] = rec
        dom = max((k for k in per_kernel if "bound" in per_kernel[k]), key=lambda k: per_kernel[k]["total_ms_per_step"])
        d = per_kernel[dom]
        roofline = {"kernel": dom, "bound": d["bound"], "achieved": d["achieved"], "peak": d["peak"], "unit": d["unit"],
                    "frac": d["frac"], "traffic": d.get("traffic"), "avg_launch_ms": d["avg_ms"],
                    "launches_per_step": d["launches_per_step"],
                    "algorithmic_bytes_per_launch" if d["bound"] == "hbm" else "algorithmic_flops_per_launch": models[dom][1],
                    "traffic_source": (f"{traffic_file}: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command on an earlier "
                                       "box, committed; NOT measured inside this run") if d.get("traffic") else None,
                    "level_tiles": {"first": lev_t0, "count": lev_nt, "of": 16}}
        if "valu_f64" in d:
            roofline["valu_f64"] = d["valu_f64"]

    # ---- the materialising affinity pass (north_star: ">= 40 % HBM-bandwidth roofline on the affinity pass"): the default
    # path never writes K_AB, so the kernels of the stage-level API / the literal formulations are timed here by
    # themselves, HIP events on the ctx's stream, in the same run.  k_affinity: fp32 rows, B_A = N s (1 + p) (SURVEY.md
    # section 8d); k_affinity64: the fp64 rows of NLE_MODE_STREAMED_F64 (libm exp), one 2 GB chunk as that mode makes them
    affinity_pass = None
    if world == 1 and args.full and args.simulate_world <= 1 and not args.no_affinity:
        affinity_pass = {}
        ldp = nle.ld(p)
        free_b, _ = torch.cuda.mem_get_info()
        if H * W * ldp * 4.0 < 0.5 * free_b:
            ms_a, kab = ctx.bench_affinity(lum, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], reps=10)
            del kab
            b_a = H * W * 4.0 * (1 + p)
            affinity_pass["k_affinity"] = {"bound": "hbm", "avg_ms": ms_a, "launches": 10, "algorithmic_bytes_per_launch": b_a,
                                           "achieved": b_a / (ms_a * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                           "frac": b_a / (ms_a * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                           "what": f"computeKernel's K_AB materialised in fp32: {H}x{W} pixels x {p} samples, read 4 B + write 4 p B per pixel"}
        rows64 = max(1, min(H, int((2048 << 20) // (W * ldp * 8))))
        ms_b, bytes_b = ctx.bench_affinity64(lum, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], rows64, reps=10)
        b_b = rows64 * W * (4.0 + 8.0 * p)
        affinity_pass["k_affinity64"] = {"bound": "hbm", "avg_ms": ms_b, "launches": 10, "algorithmic_bytes_per_launch": b_b,
                                         "achieved": b_b / (ms_b * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                         "frac": b_b / (ms_b * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                         "what": f"fp64 affinity rows (libm exp) of {rows64} image rows x {p} samples = one chunk of the streamed "
                                                 "fp64 formulation: read 4 B + write 8 p B per pixel"}
        ctx.trim()

    # ---- CPU baseline (rank 0, N = 1 only): oracle/nle_cpu_baseline.cpp, the C++17 + OpenMP streaming restatement of the
    # hot path (pinned against the numpy oracle by tests/test_cpu_baseline.py), on this box's host cores -- at the
    # workload's FULL size when the host has the memory for Phi (N x r doubles, like the reference's N x p matrices) and
    # the run is estimated to fit the budget, else on a bounded sample of the same workload; and on ONE thread (the
    # reference is single threaded: Eigen without OpenMP, CMakeLists.txt:40-46) on a bounded sample
    cpu = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        import subprocess
        exe = entry.cpu_baseline_binary()
        try:
            ncores = len(os.sched_getaffinity(0))
        except AttributeError:
            ncores = os.cpu_count() or 1
        ncores = min(ncores, args.cpu_threads)

        def run_cpu(Hs, Ws, threads):
            hx_s = cfg["hx"] * Ws / W     # same bandwidth relative to the image
            r_ = subprocess.run([exe] + [str(v) for v in (Hs, Ws, cfg["n_row"], cfg["n_col"], hx_s, cfg["hy"], cfg["T"],
                                                              cfg["K"], L, threads)], capture_output=True, text=True, check=True)
            return json.loads(r_.stdout.strip().splitlines()[-1])

        # one thread: bounded sample (~10 s)
        H1 = W1 = min(H, W, max(128, args.cpu_sample * 2 // 3))
        d1 = run_cpu(H1, W1, 1)
        mp1 = H1 * W1 / 1e6 / d1["seconds"]
        # all cores: full size if Phi + V fit the host's free memory and the estimate (perfect scaling of the 1-thread
        # rate, x2 for the memory-bound passes) stays under ~75 s; else a sample sized for ~20 s
        try:
            avail = int([ln for ln in open("/proc/meminfo") if ln.startswith("MemAvailable")][0].split()[1]) * 1024
        except Exception:  # noqa: BLE001
            avail = 0
        need = H * W * 8.0 * (p + cfg["K"] + 4) * 1.15
        est_full = 2.0 * (H * W / 1e6) / (mp1 * ncores)
        if avail > need and est_full < 75.0:
            Hs, Ws, how = H, W, "the workload's own size"
        else:
            side = int(min(H, W, max(256, (20.0 * mp1 * ncores / 2.0 * 1e6) ** 0.5)))
            side = min(side, int((0.5 * avail / (8.0 * (p + cfg["K"] + 4))) ** 0.5)) if avail else side
            Hs = Ws = max(256, side // 64 * 64)
            how = "a bounded sample of the same workload (all N-sized work is linear in N)"
        dn = run_cpu(Hs, Ws, ncores)
        cpu = {"value": (Hs * Ws / 1e6) / dn["seconds"], "unit": "MP/s", "cores": ncores, "kind": "port",
               "sample": f"{Hs}x{Ws} synthetic image = {how}; same samples/K/T/L; oracle/nle_cpu_baseline.cpp (C++17 + OpenMP, fp64, "
                         f"Phi held in memory like the reference's N x p matrices), {ncores} threads, {dn['seconds']:.1f} s",
               "stage_seconds": dn["stages"],
               "single_thread": {"value": mp1, "unit": "MP/s", "cores": 1,
                                 "sample": f"{H1}x{W1}, same program, 1 thread, {d1['seconds']:.1f} s", "stage_seconds": d1["stages"]}}

    if rank == 0:
        line = {
            # `value` is the device-resident figure the bench contract asks for (plane in HBM -> layers in HBM); SURVEY.md
            # section 8d's own definition (host plane -> host layers) is `host_to_host.value` of the same line
            "metric": ("megapixels/sec end-to-end enhance (4K img, m=200, K=50)" if args.config == "cfg4" else
                       f"megapixels/sec end-to-end enhance ({H}x{W} img, m={p}, K={cfg['K']})")
                      + "; device-resident input and output (host->host per SURVEY 8d: host_to_host.value)",
            "value": value, "unit": "MP/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"{args.config}: {H}x{W} synthetic luminance, {cfg['n_row']}x{cfg['n_col']} samples "
                                   f"(p={p}), K={cfg['K']}, T={cfg['T']}, L={L} layers; device-resident: the luminance plane is in HBM when the "
                                   f"timed region starts and the {L} layer planes are left in HBM (no PCIe inside `value`)",
                       "parallelism": (f"row-slab x{world}" if world > 1 else
                                       f"TIMING ONLY: rank 0 of a simulated {args.simulate_world}-way row shard, partial sums scaled by {args.simulate_world} in place of the all-reduce"
                                       if args.simulate_world > 1 else "single GPU")
                       + (f", {args.inflight} images in flight" if args.inflight > 1 else ""),
                       "formulation": form_label + (" (V implicit, apply in sample space)" if lazy else ""),
                       "storage": ("fp64 tables, histograms, reductions and MFMA; fp32 output planes; V implicit" if lazy else
                                   "fp64 affinities, Phi / chunks, V, reductions and MFMA; fp32 output planes"
                                   if formulation in (4, 5) else
                                   "fp64 tables, histograms, reductions and MFMA; fp32 output planes"
                                   if formulation == 2 and not args.full else
                                   "fp64 reductions and Gram/projection MFMA; fp32 affinities, V and outputs")},
            "full": bool(args.full),
            "host_to_host": h2h,
            "slab_input": bool(slab_input),
            "pipelined": pipelined,
            "replicas": replicas,
            "comm": comm_kind,
            "rccl_ranks": rccl_ranks,
            "shard_check": shard_check,
            "soak": soak,
            "roofline": roofline,
            "affinity_pass": affinity_pass,
            "cpu_baseline": cpu,
            "kernels": per_kernel,
            "stage_ms_last_step": stage_ms,
        }
        print(json.dumps(line), flush=True)
    flt.close()
    ctx.close()
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
