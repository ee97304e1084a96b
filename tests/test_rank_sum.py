"""The host-mediated all-reduce of a device group (host/rank_sum.hpp: barrier, per-rank slots, sum in rank order, fail /
recover) on its own, without a GPU: tools/micro/rank_sum_check.cpp -- a program with its own main -- built with
ThreadSanitizer and run once.  It covers G in {1, 2, 3, 5} threads and n in {1, 2049} doubles: 200 back-to-back rounds of
values whose order of addition shows, every rank ending with the bits of the rank-order sum; one round in which a rank
fails instead of arriving (the others throw, nobody hangs); a clean round after recover()."""
import os
import platform
import shutil
import subprocess

import pytest

from conftest import PKG_DIR, ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_rank_sum_under_thread_sanitizer(tmp_path):
    exe = tmp_path / "rank_sum_check"
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=thread", "-Wall", "-Werror",
                        "-I", os.path.join(PKG_DIR, "host"), os.path.join(ROOT, "tools", "micro", "rank_sum_check.cpp"),
                        "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]   # rank_sum.hpp alone: no HIP, no nle.h
    run = ["timeout", "60", str(exe)]
    # ThreadSanitizer's runtime maps its shadow at fixed addresses and gives up at start ("unexpected memory mapping") where
    # the kernel randomises mappings over more bits than it was built for: no randomisation for this one process
    no_aslr = ["setarch", platform.machine(), "-R"]
    if shutil.which("setarch") and subprocess.run(no_aslr + ["true"], capture_output=True).returncode == 0:
        run = no_aslr + run
    r = subprocess.run(run, capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-1500:])
    assert "ThreadSanitizer" not in r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "rank_sum_check OK"
    cases = [l for l in lines if l.startswith("G=")]
    assert [l.split(":")[0] for l in cases] == [f"G={g} n={n}" for g in (1, 2, 3, 5) for n in (1, 2049)]
    for l in cases:
        assert l.endswith("sums ok, order shows yes, failed round ok, stays failed yes, after recover ok"), l
