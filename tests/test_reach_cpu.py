"""Reach profiles, the parts that need no device: the coverage_hops helper against hand-computed
rows, and the carry-save bit planes of k_reach (csrc/reach_kernel.h) as pure host code -- a
stand-alone program with its own main (tests/reach_planes/reach_planes_check.cpp), compiled with
-fsanitize=address,undefined and run."""
import os
import subprocess

import numpy as np

from conftest import PKG, ROOT


def test_coverage_hops_hand_rows(gossip):
    rows = np.array([
        [1, 3, 4, 2, 0, 0],   # total 10: cumulative 1 4 8 10
        [0, 0, 0, 0, 0, 0],   # nobody reached
        [7, 0, 0, 0, 0, 0],   # a single bin
        [0, 0, 5, 0, 0, 5],   # a gap, then the last bin
        [1, 1, 1, 1, 0, 0],   # exact ties: 2 of 4 at hop 1, 3 of 4 at hop 2
    ], dtype=np.uint32)
    assert gossip.coverage_hops(rows, 0.5).tolist() == [2, -1, 0, 2, 1]
    assert gossip.coverage_hops(rows, 0.9).tolist() == [3, -1, 0, 5, 3]
    assert gossip.coverage_hops(rows, 1.0).tolist() == [3, -1, 0, 5, 3]
    assert gossip.coverage_hops(rows, 0.75).tolist() == [2, -1, 0, 5, 2]
    assert gossip.coverage_hops(rows, 0.4).tolist() == [1, -1, 0, 2, 1]   # 4 of 10 exactly at hop 1
    assert gossip.coverage_hops(rows, 0.1).tolist() == [0, -1, 0, 2, 0]   # 1 of 10 exactly at hop 0
    # exact tie where frac x total is not a binary fraction: 9 of 10 at hop 1, 27 of 30 at hop 1
    assert gossip.coverage_hops(np.array([[8, 1, 1]]), 0.9).tolist() == [1]
    assert gossip.coverage_hops(np.array([[20, 7, 3]]), 0.9).tolist() == [1]
    # one row given as a vector; large counts stay exact
    assert gossip.coverage_hops(np.array([0, 2, 2]), 0.5).tolist() == [1]
    big = np.array([[2**31, 2**31, 1]], dtype=np.uint32)
    assert gossip.coverage_hops(big, 0.5).tolist() == [1] and gossip.coverage_hops(big, 1.0).tolist() == [2]
    out = gossip.coverage_hops(rows, 0.5)
    assert out.dtype == np.int64 and out.shape == (5,)


def test_reach_planes_asan_ubsan(tmp_path):
    exe = str(tmp_path / "reach_planes_check")
    src = os.path.join(ROOT, "tests", "reach_planes", "reach_planes_check.cpp")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                        "-I" + os.path.join(PKG, "csrc"), src, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "checks passed" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_reach_abi_mirror(gossip):
    # the flag, the ledger id and the counters appended at the end of the mirror (gossip.h order)
    assert gossip.F_REACH == 512 and gossip.K_REACH == 5
    names = [f[0] for f in gossip.gossip_counters._fields_]
    assert names[-4:] == ["reach_launches", "reach_ms", "reach_bytes", "reach_slots_ms"]
    assert names[names.index("pull_fold_rows") + 1] == "reach_launches"
    hdr = open(os.path.join(ROOT, "include", "gossip.h")).read()
    assert "#define GOSSIP_F_REACH 512u" in hdr and "#define GOSSIP_K_REACH 5" in hdr
