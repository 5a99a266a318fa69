"""Multi-round push, the parts that need no device: the bit-sliced down-counters of k_rounds
(csrc/rounds_kernel.h) as pure host code -- a stand-alone program with its own main
(tests/rounds_planes/rounds_planes_check.cpp), compiled with -fsanitize=address,undefined and run -- and the
model (rounds_ref.py) against ground that is already pinned: the fault and exact-k models at r = 1, the
closed form of a flood, hand cases on a 5-node path, and the ABI mirror."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fanout_exact_ref as X
import fanout_ref as F
import faults_ref as R
import rounds_ref as M
import structured as S
from cases import L, T0
from conftest import PKG, ROOT

ALWAYS = 0xFFFFFFFF
FIRST = T0 // L
FAR = T0 + 60 * L
FOREVER = np.iinfo(np.int64).max
KEYS = ("gen", "recv", "fwd", "sent", "processed", "peers", "reach", "arrivals", "counted")


def test_rounds_planes_asan_ubsan(tmp_path):
    exe = str(tmp_path / "rounds_planes_check")
    src = os.path.join(ROOT, "tests", "rounds_planes", "rounds_planes_check.cpp")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                        "-I" + os.path.join(PKG, "csrc"), src, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "checks passed" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def _base(gossip):
    topo = gossip.Topology.gnp(1000, 8.0 / 999.0, 7, gossip.TOPO_SKIP)
    return topo, S.events(1000, 6, 8, 8)


def _crash(n, fraction, tick_from, seed=3):
    rng = np.random.default_rng(seed)
    return tuple((int(v), tick_from, FOREVER) for v in np.sort(rng.choice(n, int(n * fraction), replace=False)))


def _equal(got, want, what):
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (what, k)
    for x, y in zip(got["trace"], want["trace"]):
        assert np.array_equal(x, y), what
    assert got["dropped"] == want["dropped"], what
    assert sorted(got["lost_by_tick"]) == sorted(want["lost_by_tick"]), what
    for t in want["lost_by_tick"]:
        assert np.array_equal(got["lost_by_tick"][t], want["lost_by_tick"][t]), (what, t)


@pytest.mark.parametrize("name", ["fanout", "faults", "flood_faults", "cut"])
def test_model_at_one_round_is_the_fault_model(gossip, name):
    topo, ev = _base(gossip)
    a, b = topo.links()
    thr = F.thresholds(3, topo.degrees()[0]) if name != "flood_faults" else np.full(1000, ALWAYS, np.uint32)
    kw = {}
    if name != "fanout":
        kw = dict(outages=_crash(1000, 0.2, FIRST + 3), loss_thr=gossip.loss_threshold(0.1), loss_seed=9)
    t_cut = S.t_cut_for(6) if name == "cut" else FAR
    want = R.run(1000, a, b, ev, L, t_cut, thr, 1, **kw)
    got = M.run(1000, a, b, ev, L, t_cut, 1, thr=thr, seed=1, **kw)
    _equal(got, want, name)
    assert got["resent"] == 0 and int(want["recv"].sum()) > 0
    if name != "fanout":
        assert want["dropped"] > 0 and len(want["lost_by_tick"]) > 3


@pytest.mark.parametrize("faults", [False, True])
def test_model_at_one_round_is_the_exact_model(gossip, faults):
    topo, ev = _base(gossip)
    a, b = topo.links()
    kw = dict(outages=_crash(1000, 0.2, FIRST + 3), loss_thr=gossip.loss_threshold(0.3), loss_seed=5) if faults else {}
    want = X.run(1000, a, b, ev, L, S.t_cut_for(6), 2, 4, **kw)
    got = M.run(1000, a, b, ev, L, S.t_cut_for(6), 1, k=2, seed=4, **kw)
    _equal(got, want, ("exact", faults))
    assert got["resent"] == 0 and int(want["recv"].sum()) > 0


def _alive_ticks(ev_ns, contact_tick, r, t_cut):
    """Send ticks of a contact made in contact_tick: the ticks X of its r rounds in which the column is alive."""
    x = contact_tick[:, None] + np.arange(r)[None, :]
    return np.sum(ev_ns[:, None] + (x - (ev_ns // L)[:, None]) * L < t_cut, axis=1)


@pytest.mark.parametrize("r", [2, 3, 5, 16])
def test_flood_closed_form(gossip, r):
    # every threshold 0xffffffff and no faults: the first contacts are the flood's whatever r
    topo, ev = _base(gossip)
    a, b = topo.links()
    one = R.run(1000, a, b, ev, L, FAR, np.full(1000, ALWAYS, np.uint32), 1)
    got = M.run(1000, a, b, ev, L, FAR, r)
    for k in ("gen", "recv", "fwd", "processed", "reach", "arrivals"):
        assert np.array_equal(got[k], one[k]), k
    for x, y in zip(S.sorted_trace(got["trace"]), S.sorted_trace(one["trace"])):
        assert np.array_equal(x, y)
    assert np.array_equal(got["sent"], np.uint64(r) * one["sent"]) and int(one["sent"].sum()) > 0
    assert got["resent"] == (r - 1) * len(one["trace"][0])
    # a cut inside the floods: sent is the hand count of the alive Send ticks of every first contact
    t_cut = S.t_cut_for(6)
    one = R.run(1000, a, b, ev, L, t_cut, np.full(1000, ALWAYS, np.uint32), 1)
    got = M.run(1000, a, b, ev, L, t_cut, r)
    assert np.array_equal(got["recv"], one["recv"]) and np.array_equal(got["reach"], one["reach"])
    node, sid, tick, _hop, _via = one["trace"]
    ns_of = dict(zip(ev["share_id"].tolist(), ev["ns"].tolist()))
    ev_ns = np.array([ns_of[int(s)] for s in sid], np.int64)
    rounds = _alive_ticks(ev_ns, tick.astype(np.int64), r, t_cut)
    assert rounds.min() >= 1 and rounds.min() < r  # the cut shortens some
    want = np.zeros(1000, np.uint64)
    np.add.at(want, node, one["peers"][node].astype(np.uint64) * rounds.astype(np.uint64))
    assert np.array_equal(got["sent"], want)
    assert got["resent"] == int(rounds.sum()) - len(rounds)


# ---- hand cases: the path 0-1-2-3-4, one share born at node 0 in the first tick ----
def _path():
    a, b = np.arange(4, dtype=np.uint32), np.arange(1, 5, dtype=np.uint32)
    ev = np.zeros(1, S.GEN_EVENT_DTYPE)
    ev["ns"], ev["node"], ev["share_id"] = T0 + 1, 0, 1
    return 5, a, b, ev


def _hops(m):
    tn, _, _, th, tv = m["trace"]
    return {int(v): int(h) for v, h, via in zip(tn, th, tv) if via}


def test_hand_receiver_down_at_its_first_delivery():
    n, a, b, ev = _path()
    outages = ((2, FIRST + 2, FIRST + 3),)
    one = M.run(n, a, b, ev, L, FAR, 1, outages=outages)
    assert _hops(one) == {1: 1} and one["recv"].tolist() == [0, 1, 0, 0, 0] and one["sent"].tolist() == [1, 2, 0, 0, 0]
    two = M.run(n, a, b, ev, L, FAR, 2, outages=outages)
    assert _hops(two) == {1: 1, 2: 3, 3: 4, 4: 5}
    assert two["sent"].tolist() == [2, 4, 4, 4, 2] and two["resent"] == 5
    assert two["reach"][0, :6].tolist() == [1, 1, 0, 1, 1, 1]


def test_hand_sender_down_in_its_second_round():
    n, a, b, ev = _path()
    # node 1: contact in FIRST + 1, Sends in FIRST + 1 and FIRST + 3, none in FIRST + 2
    got = M.run(n, a, b, ev, L, FAR, 3, outages=((1, FIRST + 2, FIRST + 3),))
    up = M.run(n, a, b, ev, L, FAR, 3)
    assert up["sent"].tolist() == [3, 6, 6, 6, 3] and got["sent"].tolist() == [3, 4, 6, 6, 3]
    assert _hops(got) == _hops(up) == {1: 1, 2: 2, 3: 3, 4: 4} and got["resent"] == up["resent"] - 1
    # only the third round delivers: node 2 is down for the arrivals of the first round, node 1 makes no second
    got = M.run(n, a, b, ev, L, FAR, 3, outages=((1, FIRST + 2, FIRST + 3), (2, FIRST + 2, FIRST + 4)))
    assert _hops(got) == {1: 1, 2: 4, 3: 5, 4: 6} and got["sent"].tolist() == [3, 4, 6, 6, 3]
    # at r = 2 the third round does not exist
    got = M.run(n, a, b, ev, L, FAR, 2, outages=((1, FIRST + 2, FIRST + 3), (2, FIRST + 2, FIRST + 4)))
    assert _hops(got) == {1: 1} and got["sent"].tolist() == [2, 2, 0, 0, 0]


def test_hand_column_dies_at_the_cut_mid_rounds():
    n, a, b, ev = _path()
    # alive in FIRST, FIRST + 1, FIRST + 2; node 3's arrival in FIRST + 3 is past the cut
    got = M.run(n, a, b, ev, L, T0 + 2 * L + L // 3, 3)
    assert _hops(got) == {1: 1, 2: 2} and got["sent"].tolist() == [3, 4, 2, 0, 0] and got["resent"] == 3


COVERAGE_SEED = 1  # the fanout and loss seed of the coverage condition below (it holds for this one)


def test_coverage_grows_with_rounds_on_the_base_inputs(gossip):
    topo, ev = _base(gossip)
    a, b = topo.links()
    tot = {}
    for r in (1, 3):
        m = M.run(1000, a, b, ev, L, FAR, r, k=2, seed=COVERAGE_SEED, loss_thr=gossip.loss_threshold(0.3), loss_seed=COVERAGE_SEED)
        tot[r] = int(m["reach"].sum())
    print("total reach at r = 1, 3:", tot)
    assert tot[3] > tot[1] > 0


def test_rounds_abi_mirror(gossip):
    hdr = open(os.path.join(ROOT, "include", "gossip.h")).read()
    m = re.search(r"typedef struct gossip_rounds_counters \{(.*?)\} gossip_rounds_counters;", hdr, flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    ctype = {C.c_uint64: "uint64_t", C.c_double: "double"}
    assert re.findall(r"\b(uint64_t|double)\s+(\w+);", body) == [(ctype[t], n) for n, t in gossip.gossip_rounds_counters._fields_]
    assert [n for n, _ in gossip.gossip_rounds_counters._fields_] == ["launches", "resent_bits", "rows_visited", "ms", "bytes"]
    assert C.sizeof(gossip.gossip_rounds_counters) == 40
    assert gossip.K_ROUNDS == 7 and "#define GOSSIP_K_ROUNDS 7" in hdr
    assert [M.planes(r) for r in (2, 3, 4, 5, 8, 9, 16)] == [1, 2, 2, 3, 3, 4, 4]
    lib = gossip.load_library()
    assert lib.gossip_engine_set_rounds(None, 2) == gossip.E_INVAL
    assert lib.gossip_engine_get_rounds_counters(None, None) == gossip.E_INVAL
