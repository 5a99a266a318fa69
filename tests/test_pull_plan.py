"""gossip::pull_shape (csrc/pull_plan.h: the one rule for k_pull's launch shape, read by the tile-list
builder, the fold-write decision and the launcher) as pure host code: a stand-alone program with its
own main (tests/pull_plan/pull_plan_check.cpp), compiled with -fsanitize=address,undefined and run.
It pins the word-lanes and edge-lanes against a written-out table, checks the invariants of every
shape for windows of 1 .. 2048 words, and that TickPlan::reset keeps its vectors' storage."""
import os
import subprocess

from conftest import PKG, ROOT


def test_pull_plan_asan_ubsan(tmp_path):
    exe = str(tmp_path / "pull_plan_check")
    src = os.path.join(ROOT, "tests", "pull_plan", "pull_plan_check.cpp")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                        "-I" + os.path.join(PKG, "csrc"), src, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "checks passed" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
