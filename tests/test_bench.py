"""bench.py's contract: a plain run times `--steps` steps and prints the headline line and nothing else measured;
`--dump-outputs DIR` writes what the last timed step computed; `--full` adds the other legs of the same run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, rel_l2

BENCH = os.path.join(ROOT, "bench.py")
EXTRAS = ("host_to_host", "pipelined", "soak", "roofline", "affinity_pass", "cpu_baseline", "kernels")


def _bench(tmp_path, *args, timeout=600):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1"] + [str(a) for a in args], capture_output=True, text=True,
                       timeout=timeout, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_options_without_a_gpu():
    r = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_ones_outputs(nle, tmp_path):
    import torch
    d = _bench(tmp_path, "--steps", 3, "--warmup", 1, "--config", "cfg2", "--dump-outputs", tmp_path / "out")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "MP/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["full"] is False
    assert abs(d["value"] - 512 * 512 / 1e6 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    for k in EXTRAS:
        assert d[k] is None, k
    assert sorted(os.listdir(tmp_path / "out")) == ["eigvals.npy", "layers.npy"]
    Y = np.load(tmp_path / "out" / "layers.npy")
    S = np.load(tmp_path / "out" / "eigvals.npy")
    assert Y.dtype == np.float32 and Y.shape == (4, 512 * 512) and S.dtype == np.float64 and S.shape == (10,)
    # the same workload in this process: cfg2's seeded synthetic plane, train + apply through the ABI
    import __graft_entry__ as entry
    synth = entry._load("nle_amd_synthetic", os.path.join(entry.PKG_DIR, "synthetic.py"))
    cfg = synth.CONFIGS["cfg2"]
    x = torch.as_tensor(synth.synthetic_luminance(512, 512).astype(np.float32), device="cuda:0")
    c = nle.Context(0)
    f = nle.NLEFilter(c).train_filter(x, cfg["n_row"], cfg["n_col"], cfg["hx"], cfg["hy"], cfg["T"], cfg["K"])
    Y0 = f.apply_layers(x, cfg["L"]).cpu().numpy()
    S0 = np.array(f.eigvals)
    f.close()
    c.close()
    assert np.allclose(S, S0, rtol=1e-12, atol=0)
    for j in range(4):
        assert rel_l2(Y[j], Y0[j]) < 1e-7, j


@pytest.mark.gpu
def test_full_run_keeps_the_other_legs(tmp_path):
    d = _bench(tmp_path, "--steps", 2, "--warmup", 1, "--config", "cfg2", "--full", "--soak-seconds", 1, "--h2h-runs", 3,
               "--cpu-sample", 192)
    assert d["full"] is True and d["steps"] == 2
    for k in EXTRAS:
        assert d[k] is not None, k
    assert d["host_to_host"]["matches_device_resident_output"] is True
    assert all(p["matches_single_image_output"] for p in d["pipelined"])
    assert d["roofline"]["bound"] in ("hbm", "mfma", "valu") and d["roofline"]["frac"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["soak"]["steps"] > 0
