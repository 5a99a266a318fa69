"""gossip::order_peers (csrc/internal.h: the row permutation behind the engine option peer_order) as
pure host code: a stand-alone program with its own main (tests/order_peers/order_peers_check.cpp),
compiled with -fsanitize=address,undefined and run.  It checks that every row is a permutation of its
input, that the order is (distinct-peer count descending, id ascending), and that empty rows and
n = 0 work, at several thread counts."""
import os
import subprocess

from conftest import PKG, ROOT


def test_order_peers_asan_ubsan(tmp_path):
    exe = str(tmp_path / "order_peers_check")
    src = os.path.join(ROOT, "tests", "order_peers", "order_peers_check.cpp")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "csrc"),
                        src, "-o", exe, "-lpthread"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "checks passed" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
