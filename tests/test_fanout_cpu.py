"""Fanout-limited gossip, the parts that need no device: the model (fanout_ref.py) against the closed
form of a flood at forwarding probability 1, the selection rule of libgossip.so against the model's
on a few thousand tuples, the same vectors through csrc/fanout_kernel.h as pure host code (a
stand-alone program with its own main, tests/fanout_rule/fanout_rule_check.cpp, compiled with
-fsanitize=address,undefined and run), the threshold formula, and the ABI mirror."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fanout_ref as F
import structured as S
from cases import L, T0
from conftest import PKG, ROOT

SEEDS = (1, 2, 0xFFFFFFFF, 0x1_0000_0001, 0x8000_0000_0000_0001, 0xFFFF_FFFF_FFFF_FFFF, 0xDEADBEEF_00000000)
THRS = (0, 1, 1 << 31, 0xFFFFFFFE, 0xFFFFFFFF, 0x55555555)


def _vectors():
    """(seed, u, v, c, tick, thr) tuples: both directions of every pair, copies 0 and 1, the boundary
    thresholds, node ids near 2^32 - 1, seeds with high bits set, ticks up to 2^32 - 1."""
    rng = np.random.default_rng(77)
    nodes = np.concatenate([rng.integers(0, 1 << 20, 40), [0, 1, 2, 0xFFFFFFFF, 0xFFFFFFFE, 0x80000000, 0x7FFFFFFF]])
    out = []
    for i in range(600):
        u, v = (int(x) for x in rng.choice(nodes, 2, replace=False))
        tick = int(rng.choice([0, 1, 1000, 12345678, 0xFFFFFFFF, int(rng.integers(0, 1 << 32))]))
        seed = SEEDS[i % len(SEEDS)]
        thr = THRS[(i // len(SEEDS)) % len(THRS)] if i % 3 else int(rng.integers(0, 1 << 32))
        for c in (0, 1):
            out.append((seed, u, v, c, tick, thr))
            out.append((seed, v, u, c, tick, thr))
    return out


@pytest.mark.parametrize("name", ["ladder_parallel", "components", "gnp"])
def test_model_is_the_flood_at_probability_one(name):
    # bfs_reference is pinned to ORACLE A by test_structured_cases.py
    if name == "ladder_parallel":
        f = S.family(name)
        n, a, b, ev, t_cut = f["n"], f["a"], f["b"], f["ev"], f["t_cut"]
    elif name == "components":
        n, a, b = S.components()
        ev, t_cut = S.events(n, 30, 4, 13, must_include=range(n - 3, n)), S.t_cut_for(30)
    else:
        n = 300
        rng = np.random.default_rng(5)
        iu = np.triu_indices(n, 1)
        m = rng.random(len(iu[0])) < 6.0 / n
        a, b = iu[0][m].astype(np.uint32), iu[1][m].astype(np.uint32)
        ev, t_cut = S.events(n, 6, 8, 9), S.t_cut_for(6)
    want = S.bfs_reference(n, a, b, ev, L, t_cut)
    got = F.run(n, a, b, ev, L, t_cut, np.full(n, F.ALWAYS, np.uint32), seed=3)
    for k in ("gen", "recv", "fwd", "sent", "processed", "peers"):
        assert np.array_equal(got[k], want[k]), (name, k)
    for x, y in zip(S.sorted_trace(got["trace"]), S.sorted_trace(want["trace"])):
        assert np.array_equal(x, y), name
    assert int(got["reach"].sum()) == int(want["processed"].sum())
    # and a real threshold thins it: fewer sends, no more receptions
    thin = F.run(n, a, b, ev, L, t_cut, F.thresholds(2, want["peers"]), seed=3)
    assert thin["sent"].sum() < want["sent"].sum() and np.all(thin["recv"] <= want["recv"])
    assert np.array_equal(thin["gen"], want["gen"])


def test_library_rule_equals_model(gossip):
    vec = _vectors()
    assert len(vec) >= 2000
    got = np.array([gossip.fanout_selected(*r) for r in vec])
    want = np.array([bool(F.selected(r[0], r[1], r[2], r[3], r[4], r[5])) for r in vec])
    assert np.array_equal(got, want)
    assert 0.2 < got.mean() < 0.8  # both outcomes occur
    by_thr = {t: got[[r[5] == t for r in vec]] for t in (0, 0xFFFFFFFF)}
    assert not by_thr[0].any() and by_thr[0xFFFFFFFF].all()
    # one Philox call serves both directions: at equal thresholds the two directions differ somewhere
    half = [(r, q) for r, q in zip(vec[0::2], vec[1::2]) if r[5] == 1 << 31]
    assert any(gossip.fanout_selected(*r) != gossip.fanout_selected(*q) for r, q in half)


def test_threshold_frequencies(gossip):
    # forwarding probability thr / 2^32: 4,000 draws at 1/4, 1/2, 3/4 (binomial sd < 0.008)
    for thr in (1 << 30, 1 << 31, 3 << 30):
        hits = sum(gossip.fanout_selected(11, 3, 9, 0, t, thr) for t in range(4000))
        assert abs(hits / 4000 - thr / 2 ** 32) < 0.04, thr


def test_fanout_rule_asan_ubsan(tmp_path):
    vec = _vectors()
    want = [bool(F.selected(*r)) for r in vec]
    vfile = tmp_path / "vectors.txt"
    vfile.write_text("".join(" ".join(str(int(x)) for x in r) + f" {int(w)}\n" for r, w in zip(vec, want)))
    # set_fanout's thresholds: the integer formula for degrees 0 .. 257 (and a few fanouts)
    tfile = tmp_path / "thresholds.txt"
    lines = []
    for k in (1, 2, 3, 8, 64, 257):
        for deg in range(258):
            t = 0xFFFFFFFF if deg <= k else (k << 32) // deg
            assert int(F.thresholds(k, [deg])[0]) == t
            lines.append(f"{k} {deg} {t}\n")
    tfile.write_text("".join(lines))
    exe = str(tmp_path / "fanout_rule_check")
    src = os.path.join(ROOT, "tests", "fanout_rule", "fanout_rule_check.cpp")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                        "-I" + os.path.join(PKG, "csrc"), src, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    r = subprocess.run([exe, str(vfile), str(tfile)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert f"{len(vec)} vectors" in r.stdout and "checks passed" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_unique_ids(gossip):
    ev = S.events(50, 4, 5, 3, id_mask=0x3)
    assert len(np.unique(ev["share_id"])) < len(ev)
    out = gossip.unique_ids(ev)
    assert out.dtype == gossip.GEN_EVENT_DTYPE and out is not ev
    assert np.array_equal(out["share_id"], np.arange(1, len(ev) + 1))
    assert np.array_equal(out["ns"], ev["ns"]) and np.array_equal(out["node"], ev["node"])
    assert len(gossip.unique_ids(ev[:0])) == 0


def test_fanout_abi_mirror(gossip):
    assert gossip.K_FANOUT == 6 and gossip.FANOUT_ALWAYS == 0xFFFFFFFF
    hdr = open(os.path.join(ROOT, "include", "gossip.h")).read()
    assert "#define GOSSIP_K_FANOUT 6" in hdr
    m = re.search(r"typedef struct gossip_fanout_counters \{(.*?)\} gossip_fanout_counters;", hdr, flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"\b(uint64_t|double)\s+(\w+);", body)
    mirror = [(("uint64_t" if t is C.c_uint64 else "double"), n) for n, t in gossip.gossip_fanout_counters._fields_]
    assert fields == mirror == [("uint64_t", "launches"), ("uint64_t", "selected_in"), ("uint64_t", "selected_out"),
                                ("uint64_t", "entries"), ("double", "ms"), ("uint64_t", "bytes")]
    assert C.sizeof(gossip.gossip_fanout_counters) == 48
    # gossip_counters is not extended: its last four fields stay the reach counters
    assert [f[0] for f in gossip.gossip_counters._fields_][-4:] == ["reach_launches", "reach_ms", "reach_bytes",
                                                                   "reach_slots_ms"]
    ledger = open(os.path.join(PKG, "csrc", "launch_ledger.h")).read()
    assert "LK_FANOUT = 6" in ledger and "kLaunchKernels = 7" in ledger
    # NULL arguments are refused without a device
    lib = gossip.load_library()
    assert lib.gossip_engine_set_fanout(None, 3, 1) == gossip.E_INVAL
    assert lib.gossip_engine_set_forward_thresholds(None, None, 1) == gossip.E_INVAL
    assert lib.gossip_engine_get_fanout_counters(None, None) == gossip.E_INVAL
