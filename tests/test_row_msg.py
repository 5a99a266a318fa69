"""The row partition's message rules (csrc/row_msg.h: the one layout, the chunk geometry and the
broadcast capacities that the packer, the unpacker and the three transports of engine.hip read) as
pure host code: a stand-alone program with its own main (tests/row_msg/row_msg_check.cpp), compiled
with -fsanitize=address,undefined and run.  It pins the prefix sizes and the capacities against
written-out values, checks the length's inverse and its refusals, and that the chunks of every rank
extent of 0 .. 5000 rows tile it on 512-row granules with the liveness in the last one."""
import os
import subprocess

from conftest import PKG, ROOT


def test_row_msg_asan_ubsan(tmp_path):
    exe = str(tmp_path / "row_msg_check")
    src = os.path.join(ROOT, "tests", "row_msg", "row_msg_check.cpp")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                        "-I" + os.path.join(PKG, "csrc"), src, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "checks passed" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
