"""Fault injection, the parts that need no device: the loss rule of libgossip.so against the model's
(faults_ref.py) on 10,000 tuples, its frequencies, the independence of the two directions and of the
copies of a link, the model against ground that is already pinned (the fanout model without faults; the
closed form of a flood on the graph without the crashed nodes), the outage-file reader, and the ABI mirror."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fanout_ref as F
import faults_ref as R
import structured as S
from cases import L, T0
from conftest import ROOT

ALWAYS = 0xFFFFFFFF
FAR = T0 + 60 * L


def _tuples(count=10_000):
    """(seed, u, v, c, tick, thr): random, with the boundary thresholds, u > v as often as u < v, node ids
    and ticks up to 2^32 - 1 and 64-bit seeds."""
    rng = np.random.default_rng(2024)
    seeds = [1, 2, 0xFFFFFFFF, 0x1_0000_0001, 0x8000_0000_0000_0001, 0xFFFF_FFFF_FFFF_FFFF, 0xDEADBEEF_00000000]
    thrs = [0, 1, 0xFFFFFFFE, 0xFFFFFFFF, 1 << 31, 0x55555555]
    out = []
    for i in range(count):
        u, v = (int(x) for x in rng.integers(0, 1 << 32, 2, dtype=np.uint64))
        if i % 5 == 0:
            u, v = u & 0xFFFFF, v & 0xFFFFF
        if u == v:
            v ^= 1
        seed = seeds[i % len(seeds)] if i % 2 else int(rng.integers(0, 1 << 64, dtype=np.uint64))
        thr = thrs[(i // 2) % len(thrs)] if i % 3 else int(rng.integers(0, 1 << 32))
        tick = int(rng.choice([0, 1, 1000, 0xFFFFFFFF, int(rng.integers(0, 1 << 32))]))
        out.append((seed, u, v, int(rng.integers(0, 3)), tick, thr))
    return out


def test_library_rule_equals_model(gossip):
    vec = _tuples()
    assert len(vec) == 10_000
    assert sum(r[1] > r[2] for r in vec) > 3000 and sum(r[1] < r[2] for r in vec) > 3000
    assert any(r[0] >> 32 for r in vec) and {0, 1, 0xFFFFFFFE, ALWAYS} <= {r[5] for r in vec}
    got = np.array([gossip.fault_lost(*r) for r in vec])
    want = np.array([bool(R.lost(*r)) for r in vec])
    assert np.array_equal(got, want)
    thr = np.array([r[5] for r in vec], np.uint64)
    assert not got[thr == 0].any() and got[thr == ALWAYS].all()
    assert not got[thr == 1].any() and got[thr == 0xFFFFFFFE].all()  # (a word of 0 or 2^32 - 1: 2^-32 each)
    assert 0.2 < got.mean() < 0.8  # both outcomes occur


def test_loss_frequency(gossip):
    # 2^16 links at loss_thr = 2^31: a fair coin each, sd of the mean 0.5 / 2^8
    m = 1 << 16
    u = np.arange(m, dtype=np.uint64) * 3 + 1
    v = u + 1 + (np.arange(m, dtype=np.uint64) % 7)
    lib = gossip.load_library()
    lost = np.array([lib.gossip_fault_lost(7, int(a), int(b), 0, 123, 1 << 31) for a, b in zip(u, v)], bool)
    assert abs(lost.mean() - 0.5) < 4 * 0.5 / np.sqrt(m)
    assert np.array_equal(lost, R.lost(7, u, v, 0, 123, 1 << 31))  # and link by link the model's


def test_directions_and_copies_draw_different_words(gossip):
    # one Philox call serves both directions of a link (words 0 and 1) and each copy has its own counter:
    # at probability 1/2 the two outcomes are independent coins, so they differ on about half the links
    m = 1 << 12
    u = np.arange(m, dtype=np.uint64) * 5 + 2
    v = u + 3
    fwd, back = R.lost(9, u, v, 0, 77, 1 << 31), R.lost(9, v, u, 0, 77, 1 << 31)
    c0, c1 = fwd, R.lost(9, u, v, 1, 77, 1 << 31)
    tol = 4 * 0.5 / np.sqrt(m)
    assert abs((fwd != back).mean() - 0.5) < tol and abs((c0 != c1).mean() - 0.5) < tol
    for i in range(0, m, 16):
        a, b = int(u[i]), int(v[i])
        assert gossip.fault_lost(9, a, b, 0, 77, 1 << 31) == bool(fwd[i])
        assert gossip.fault_lost(9, b, a, 0, 77, 1 << 31) == bool(back[i])
        assert gossip.fault_lost(9, a, b, 1, 77, 1 << 31) == bool(c1[i])
    # its own key constant: the loss draw is not the fanout draw of the same (seed, link, copy, tick)
    sel = F.selected(9, u, v, 0, 77, 1 << 31)
    assert abs((sel != fwd).mean() - 0.5) < tol


def _base(gossip):
    topo = gossip.Topology.gnp(1000, 8.0 / 999.0, 7, gossip.TOPO_SKIP)
    return topo, S.events(1000, 6, 8, 8)


def test_model_without_faults_is_the_fanout_model(gossip):
    topo, ev = _base(gossip)
    a, b = topo.links()
    thr = F.thresholds(3, topo.degrees()[0])
    want = F.run(1000, a, b, ev, L, FAR, thr, 1)
    got = R.run(1000, a, b, ev, L, FAR, thr, 1, outages=(), loss_thr=0)
    for k in ("gen", "recv", "fwd", "sent", "processed", "peers", "reach", "arrivals"):
        assert np.array_equal(got[k], want[k]), k
    for x, y in zip(got["trace"], want["trace"]):
        assert np.array_equal(x, y)
    assert got["dropped"] == 0 and int(want["recv"].sum()) > 0
    # with loss on, the model's draws of the first ticks are the library's, copy by copy
    lossy = R.run(1000, a, b, ev, L, T0 + 8 * L, thr, 1, loss_thr=1 << 30, loss_seed=(1 << 40) + 3)
    u, v, c, _ = F.copies(1000, a, b)
    assert 0 < int(lossy["recv"].sum()) and len(lossy["lost_by_tick"]) >= 3
    for tick in sorted(lossy["lost_by_tick"])[:3]:
        lib_lost = [gossip.fault_lost((1 << 40) + 3, int(u[j]), int(v[j]), int(c[j]), tick, 1 << 30) for j in range(0, len(u), 7)]
        assert lib_lost == lossy["lost_by_tick"][tick][::7].tolist()


@pytest.mark.parametrize("name", ["base", "ladder_parallel"])
def test_model_with_a_crash_set_is_the_flood_on_the_remaining_graph(gossip, name, tmp_path):
    # bfs_reference is pinned to ORACLE A by test_structured_cases.py
    if name == "base":
        topo, ev = _base(gossip)
        n, (a, b), t_cut = 1000, topo.links(), S.t_cut_for(6)
    else:
        f = S.family(name)
        n, a, b, ev, t_cut = f["n"], f["a"], f["b"], f["ev"], f["t_cut"]
    rng = np.random.default_rng(3)
    crash = np.sort(rng.choice(n, n // 5, replace=False))
    is_c = np.zeros(n, bool)
    is_c[crash] = True
    outages = [(int(v), 0, 1 << 40) for v in crash]
    # the crash set through the library's file reader: whole-run outages in ns come back as these ticks
    path = tmp_path / "crash.txt"
    path.write_text("".join(f"{int(v)} 0 {(1 << 40) * L}\n" for v in crash))
    nodes, t0, t1, skipped = gossip.load_outages(n, L, str(path))
    assert [(int(x), int(y), int(z)) for x, y, z in zip(nodes, t0, t1)] == outages and skipped == 0
    got = R.run(n, a, b, ev, L, t_cut, np.full(n, ALWAYS, np.uint32), 3, outages=outages)
    keep = ~is_c[np.asarray(a, np.int64)] & ~is_c[np.asarray(b, np.int64)]
    ev_up = ev[~is_c[ev["node"]]]
    want = S.bfs_reference(n, a[keep], b[keep], ev_up, L, t_cut)
    assert np.array_equal(got["recv"], want["recv"]) and int(want["recv"].sum()) > 0
    assert not got["recv"][crash].any() and not got["gen"][crash].any()
    assert got["dropped"] == int(is_c[ev["node"]].sum()) > 0
    # an up node whose every peer crashed still generates in the model (it has peers; its Sends deliver nothing)
    full = S.bfs_reference(n, a, b, ev_up, L, t_cut)
    assert np.array_equal(got["gen"], full["gen"])
    # a Send to a down node is made: sent counts the full degree of every node that processed a share
    assert np.array_equal(got["sent"], got["peers"].astype(np.uint64) * (got["gen"] + got["recv"]).astype(np.uint64))
    assert int(got["sent"].sum()) > int(want["sent"].sum())
    # the first receptions, by (node, share, hop), are the remaining graph's
    gt, wt = S.sorted_trace(got["trace"]), S.sorted_trace(want["trace"])
    g1, w1 = gt[4] == 1, wt[4] == 1
    for i in (0, 1, 3):
        assert np.array_equal(gt[i][g1], wt[i][w1])


def test_outage_file_reader(gossip, tmp_path):
    lat = 5_000_000
    p = tmp_path / "outages.txt"
    # down in tick T iff from_ns <= T * L < to_ns: ceil on both ends
    p.write_text("3 0 5000000\n"            # ticks [0, 1)
                 "4 1 5000001\n"            # ticks [1, 2)
                 "\n"
                 "5\t10000000  20000001\r\n"  # ticks [2, 5)
                 "6 5000001 9999999\n"      # no tick start inside: skipped
                 "7 12 12\n")               # empty: skipped
    nodes, t0, t1, skipped = gossip.load_outages(10, lat, str(p))
    assert nodes.tolist() == [3, 4, 5] and t0.tolist() == [0, 1, 2] and t1.tolist() == [1, 2, 5] and skipped == 2
    for text, match in (("3 0 5000000\n4 x 9\n", "line 2"), ("1 2\n", "line 1"), ("1 2 3 4\n", "line 1"), ("11 0 9\n", "line 1"),
                        ("1 -2 3\n", "line 1"), ("0 0 1\n\n2 9 3\n", "line 3")):
        p.write_text(text)
        with pytest.raises(gossip.GossipError, match=match) as e:
            gossip.load_outages(10, lat, str(p))
        assert e.value.code == gossip.E_INVAL
    with pytest.raises(gossip.GossipError, match="cannot read"):
        gossip.load_outages(10, lat, str(tmp_path / "missing.txt"))


def test_helpers(gossip):
    assert gossip.loss_threshold(0.0) == 0 and gossip.loss_threshold(1.0) == ALWAYS
    assert gossip.loss_threshold(0.5) == 1 << 31 and gossip.loss_threshold(0.25) == 1 << 30
    with pytest.raises(gossip.GossipError):
        gossip.loss_threshold(1.5)
    nodes, t0, t1 = gossip.crash_outages(1000, 0.1, 7)
    assert len(nodes) == 100 == len(np.unique(nodes)) and nodes.max() < 1000 and np.all(np.diff(nodes) > 0)
    assert np.all(t0 == 7) and np.all(t1 == np.iinfo(np.int64).max)
    again = gossip.crash_outages(1000, 0.1, 7)
    assert np.array_equal(nodes, again[0])
    assert not np.array_equal(nodes, gossip.crash_outages(1000, 0.1, 7, seed=2)[0])
    assert gossip.crash_outages(1000, 0.1, 7, 9)[2].tolist() == [9] * 100
    assert len(gossip.crash_outages(10, 0.0, 1)[0]) == 0


def test_faults_abi_mirror(gossip):
    hdr = open(os.path.join(ROOT, "include", "gossip.h")).read()

    def fields(name):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, flags=re.S)
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        return re.findall(r"\b(uint64_t|uint32_t|int64_t)\s+(\w+);", body)

    ctype = {C.c_uint64: "uint64_t", C.c_uint32: "uint32_t", C.c_int64: "int64_t"}
    for name, cls in (("gossip_outage", gossip.gossip_outage), ("gossip_fault_counters", gossip.gossip_fault_counters)):
        assert fields(name) == [(ctype[t], n) for n, t in cls._fields_], name
    assert [n for n, _ in gossip.gossip_fault_counters._fields_] == ["launches", "down_node_ticks", "lost_copies", "down_copies",
                                                                     "dropped_generations"]
    assert C.sizeof(gossip.gossip_outage) == 24 == gossip.OUTAGE_DTYPE.itemsize and C.sizeof(gossip.gossip_fault_counters) == 40
    assert "0x4C4F5353" in hdr and R.LOSS_KEY1 == 0x4C4F5353
    # NULL arguments are refused without a device
    lib = gossip.load_library()
    assert lib.gossip_engine_set_outages(None, 0, None) == gossip.E_INVAL
    assert lib.gossip_engine_set_link_loss(None, 1, 1) == gossip.E_INVAL
    assert lib.gossip_engine_get_fault_counters(None, None) == gossip.E_INVAL
