"""The launch ledger (csrc/launch_ledger.h: the key of a k_pull instantiation, the dispatch rule from
a launch's conditions to the instantiation, the list of instantiations the rule can select, the
per-engine launch counts) as pure host code: a stand-alone program with its own main
(tests/launch_ledger/launch_ledger_check.cpp), compiled with -fsanitize=address,undefined and run.
The ABI's enumeration is checked against the same table from Python (no device needed)."""
import os
import subprocess

from conftest import PKG, ROOT


def test_launch_ledger_asan_ubsan(tmp_path):
    exe = str(tmp_path / "launch_ledger_check")
    src = os.path.join(ROOT, "tests", "launch_ledger", "launch_ledger_check.cpp")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                        "-I" + os.path.join(PKG, "csrc"), src, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "checks passed" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_pull_instantiations_abi(gossip):
    got = gossip.pull_instantiations()
    assert len(got) == 27 and len({r.key for r in got}) == 27
    assert all(r.kernel == gossip.K_PULL and r.arg == 0 and r.launches == 0 and r.strided == 0 for r in got)
    keys = {(r.lpw, r.epn, r.flags) for r in got}
    shapes = {(8, 1), (8, 2), (8, 4), (8, 8), (16, 1), (16, 2), (16, 4), (32, 1), (32, 2)}
    want = {(l, e, 0) for l, e in shapes} | {(32, 1, gossip.PULL_NT), (16, 1, gossip.PULL_NT)}
    want |= {(32, 1, gossip.PULL_SP | f) for f in range(32) if not f & gossip.PULL_SP}
    assert len(want) == 27 and keys == want
    # caller-owned arrays, NULL to size, a short array refused
    import ctypes as C
    lib = gossip.load_library()
    cnt = C.c_uint32(0)
    assert lib.gossip_pull_instantiations(None, 0, C.byref(cnt)) == 0 and cnt.value == 27
    arr = (gossip.gossip_launch_record * 26)()
    assert lib.gossip_pull_instantiations(arr, 26, C.byref(cnt)) == gossip.E_INVAL and cnt.value == 27
    assert lib.gossip_pull_instantiations(arr, 26, None) == gossip.E_INVAL
    assert lib.gossip_engine_get_launches(None, None, 0, C.byref(cnt)) == gossip.E_INVAL
