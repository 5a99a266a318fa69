"""Fault injection on the device (k_fanout_count_faults, csrc/fanout_kernel.h) against the model
(faults_ref.py): engine and model agree EXACTLY on per-node gen, recv, fwd, sent and processed and on
edge_events, and with F_TRACE | F_REACH on the (node, share, hop, via) set and the reach table; the GPU-side
fault counters equal the model's.  The model is pinned to the fanout model and to the closed form of a
flood without the crashed nodes by test_faults_cpu.py; one case here goes to ORACLE A directly.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import fanout_ref as F
import faults_ref as R
import structured as S
import thinning_ref as TH
from cases import L, T0

pytestmark = pytest.mark.gpu

ALWAYS = 0xFFFFFFFF
FIRST = T0 // L                      # gossip_engine_first_tick of every engine here
FOREVER = np.iinfo(np.int64).max
FAR = T0 + 60 * L
STAT_KEYS = ("gen", "recv", "fwd", "sent", "processed")


@functools.lru_cache(maxsize=None)
def _base(gossip):  # the base inputs of test_fanout_gpu.py
    topo = gossip.Topology.gnp(1000, 8.0 / 999.0, 7, gossip.TOPO_SKIP)
    return topo, S.events(1000, 6, 8, 8)


@functools.lru_cache(maxsize=None)
def _tail(gossip, n):
    n, a, b = S.ring_chords(n, 7)
    return gossip.Topology.from_links(n, a, b), S.events(n, 12, min(2, n), 100 + n), S.t_cut_for(12)


@functools.lru_cache(maxsize=None)
def _ladder(gossip):
    n, a, b = S.ladder(seed=11, parallel=True)
    ev = S.events(n, 10, 6, 12, must_include=range(len(S.LADDER_DEGS)))
    return gossip.Topology.from_links(n, a, b), ev, T0 + 40 * L


@functools.lru_cache(maxsize=None)
def _ring65(gossip):  # one share born at node 0 in the first tick
    n, a, b = S.ring_chords(65, 0)
    ev = np.zeros(1, S.GEN_EVENT_DTYPE)
    ev["ns"], ev["node"], ev["share_id"] = T0 + 1, 0, 1
    return gossip.Topology.from_links(n, a, b), ev, T0 + 70 * L


def _crash(n, fraction, tick_from, seed=3):
    rng = np.random.default_rng(seed)
    return tuple((int(v), tick_from, FOREVER) for v in np.sort(rng.choice(n, int(n * fraction), replace=False)))


_MODEL = {}


def _model(topo, ev, t_cut, thr=None, fan_seed=1, outages=(), loss_thr=0, loss_seed=1):
    thr = np.full(topo.num_nodes, ALWAYS, np.uint32) if thr is None else np.ascontiguousarray(thr, np.uint32)
    key = (id(topo), ev.tobytes(), t_cut, thr.tobytes(), fan_seed, tuple(outages), loss_thr, loss_seed)
    if key not in _MODEL:
        a, b = topo.links()
        m = R.run(topo.num_nodes, a, b, ev, L, t_cut, thr, fan_seed, outages=outages, loss_thr=loss_thr, loss_seed=loss_seed)
        assert np.array_equal(m["peers"], topo.degrees()[0])
        _MODEL[key] = m
    return _MODEL[key]


def _engine(gossip, topo, ev, t_cut, outages=None, loss_thr=None, loss_seed=1, k=None, fan_seed=1, fanout_last=False, flags=0,
            opts=(), snaps=(), trace=True, **kw):
    """outages / loss_thr None: that setter is not called."""
    fl = gossip.F_REACH | (gossip.F_TRACE if trace else 0) | flags
    eng = gossip.Engine(topo.num_nodes, L, T0, t_cut, flags=fl, **kw)
    for name, v in dict(opts).items():
        eng.set_option(name, v)
    eng.set_topology(topo)
    if k is not None and not fanout_last:
        eng.set_fanout(k, fan_seed)
    if outages is not None:
        o = np.array(outages, np.int64).reshape(-1, 3)
        eng.set_outages(o[:, 0], o[:, 1], o[:, 2])
    if loss_thr is not None:
        eng.set_link_loss(int(loss_thr), loss_seed)
    if k is not None and fanout_last:
        eng.set_fanout(k, fan_seed)
    for t in snaps:
        eng.add_snapshot(t)
    eng.set_schedule(ev)
    return eng


def _result(eng, trace=True):
    eng.sync()
    st, c = eng.stats(), eng.counters()
    out = dict(gen=st.gen, recv=st.recv, fwd=st.fwd, sent=st.sent, processed=st.processed, peers=st.peers,
               edge_events=int(c.edge_events), reach=eng.reach(), counters=c, launches=eng.launches(),
               fanout=eng.fanout_counters(), faults=eng.fault_counters(), ticks=(eng.first_tick, eng.end_tick))
    if trace:
        out["trace"] = eng.trace()
    return out


def _hops_set(trace):
    node, sid, _tick, hop, via = (np.asarray(x, np.int64) for x in trace)
    o = np.lexsort((sid, node))
    return node[o], sid[o], hop[o], via[o]


def _same(got, want, what, trace=True):
    for k in STAT_KEYS:
        if not np.array_equal(got[k], want[k]):
            bad = np.flatnonzero(np.asarray(got[k]) != np.asarray(want[k]))
            raise AssertionError(f"{what}: {k} differs at {len(bad)} nodes, first "
                                 f"{[(int(v), int(got[k][v]), int(want[k][v])) for v in bad[:6]]} (node, engine, model)")
    assert got["edge_events"] == int(want["sent"].sum()), what
    assert np.array_equal(got["reach"], want["reach"]), what
    if trace:
        for x, y in zip(_hops_set(got["trace"]), _hops_set(want["trace"])):
            assert np.array_equal(x, y), what
        assert np.array_equal(np.sort(got["trace"][2]), np.sort(want["trace"][2])), what  # the ticks too


def _records(res, gossip):
    return {r.arg: r for r in res["launches"] if r.kernel == gossip.K_FANOUT}


def _run(gossip, topo, ev, t_cut, what, outages=(), loss_thr=0, loss_seed=1, k=None, fan_seed=1, trace=True, **kw):
    """One engine run compared with the model, fault counters included; returns (engine result, model)."""
    eng = _engine(gossip, topo, ev, t_cut, outages=outages, loss_thr=loss_thr, loss_seed=loss_seed, k=k, fan_seed=fan_seed,
                  trace=trace, **kw)
    try:
        eng.run()
        got = _result(eng, trace)
    finally:
        eng.close()
    thr = F.thresholds(k, topo.degrees()[0]) if k is not None else np.full(topo.num_nodes, ALWAYS, np.uint32)
    want = _model(topo, ev, t_cut, thr, fan_seed, tuple(outages), loss_thr, loss_seed)
    _same(got, want, what, trace)
    f, first, end = got["faults"], *got["ticks"]
    assert f.dropped_generations == want["dropped"], what
    rec = _records(got, gossip)
    if len(outages) or loss_thr:  # every tick of the run is thinned with faults
        assert f.launches == got["counters"].ticks == end - first == rec[3].launches == rec[2].launches and 1 not in rec, what
        a, b = topo.links()
        counts = R.fault_counts(topo.num_nodes, a, b, thr, fan_seed, outages, loss_thr, loss_seed, range(first, end))
        assert (f.down_node_ticks, f.lost_copies, f.down_copies) == counts, what
        assert got["fanout"].launches == f.launches, what  # the thinning passes of a faults-only engine are reported
    else:
        assert (f.launches, f.down_node_ticks, f.lost_copies, f.down_copies) == (0, 0, 0, 0) and 3 not in rec, what
    # the totals of the thinning passes: the model of the thinned lists (thinning_ref.py), over the ticks of the run
    tot = TH.of_topology(topo, thr=thr if k is not None else None, seed=fan_seed, outages=tuple(outages), loss_thr=loss_thr,
                         loss_seed=loss_seed).totals(range(first, first + int(got["counters"].ticks)))
    fo = got["fanout"]
    assert fo.launches == got["counters"].ticks, what
    assert (fo.selected_in, fo.selected_out) == (tot["selected_in"], tot["selected_out"]), (what, tot)
    assert (f.down_node_ticks, f.lost_copies, f.down_copies) == (tot["down_node_ticks"], tot["lost_copies"], tot["down_copies"]), what
    return got, want


# ---- chunk edges ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [0, 1])
@pytest.mark.parametrize("n", [2, 63, 64, 65, 129, 513])
def test_chunk_edges(gossip, n, grid):
    # a ragged last 64-node chunk, chunks whose entry range is not 64-aligned; grid 1: a wave strides several
    topo, ev, t_cut = _tail(gossip, n)
    outages = tuple((v, FIRST + 2, FIRST + 6) for v in range(0, n, 3))
    got, want = _run(gossip, topo, ev, t_cut, ("chunks", n, grid), outages=outages, opts=dict(fanout_grid=grid))
    rec = _records(got, gossip)
    assert set(rec) == {3, 2}
    if n == 513 and grid == 1:
        assert rec[3].strided > 0 and rec[2].strided > 0
    plain = _model(topo, ev, t_cut)
    assert got["faults"].down_node_ticks == 4 * len(outages)
    if n > 2:
        assert int(want["recv"].sum()) < int(plain["recv"].sum())  # the outages bite


# ---- interval edges on a ring: one share from node 0, node 5 is at hop 5 (tick FIRST + 5) ------------------
def _hop_of(m, node):
    tn, _, _, th, tv = m["trace"]
    h = th[(tn == node) & (tv == 1)]
    return int(h[0]) if len(h) else None


@pytest.mark.parametrize("name,outages,hop5", [
    ("exact", ((5, FIRST + 5, FIRST + 6),), 60),            # down in the arrival tick: missed; later from the other side
    ("earlier", ((5, FIRST + 4, FIRST + 5),), 5),           # tick_to = the arrival tick: up, receives
    ("later", ((5, FIRST + 6, FIRST + 7),), 5),             # received and forwarded in FIRST + 5, down afterwards
    ("to_is_arrival", ((5, FIRST + 1, FIRST + 5),), 5),
    ("forever", ((5, FIRST + 5, FOREVER),), None),          # the flood on that arc stops there for the rest of the run
    ("forever_32", ((5, FIRST + 5, 1 << 40),), None),
])
def test_interval_edges(gossip, name, outages, hop5):
    topo, ev, t_cut = _ring65(gossip)
    got, want = _run(gossip, topo, ev, t_cut, ("interval", name), outages=outages)
    assert _hop_of(want, 5) == hop5 and _hop_of(want, 4) == 4 and int(got["recv"][5]) == (hop5 is not None)
    if hop5 == 5:
        assert _hop_of(want, 6) == 6
    else:
        assert _hop_of(want, 6) == 59  # node 6 hears of it from node 7 only
    if name == "later":  # tick FIRST + 5 thins for FIRST + 6, where row 5 is down: its two in-copies, once
        assert int(got["sent"].sum()) == 2 * 65 and got["faults"].down_copies == 2


def test_touching_intervals_equal_their_merge(gossip):
    topo, ev, t_cut = _ring65(gossip)
    merged = ((5, FIRST + 3, FIRST + 7), (9, FIRST + 9, FIRST + 10))
    forms = (((5, FIRST + 3, FIRST + 5), (9, FIRST + 9, FIRST + 10), (5, FIRST + 5, FIRST + 7)),   # touching
             ((5, FIRST + 4, FIRST + 7), (5, FIRST + 3, FIRST + 6), (9, FIRST + 9, FIRST + 10), (5, FIRST + 4, FIRST + 5)))
    ref, want = _run(gossip, topo, ev, t_cut, "merged", outages=merged)
    assert _hop_of(want, 5) == 60 and _hop_of(want, 9) == 56
    for o in forms:
        got, _ = _run(gossip, topo, ev, t_cut, ("touching", len(o)), outages=o)
        for k in STAT_KEYS + ("reach",):
            assert np.array_equal(got[k], ref[k]), k
        for x, y in zip(S.sorted_trace(got["trace"]), S.sorted_trace(ref["trace"])):
            assert np.array_equal(x, y)
        assert got["faults"].down_node_ticks == ref["faults"].down_node_ticks == 5


# ---- dropped generations -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["own_tick", "whole_run", "all_down"])
def test_dropped_generations(gossip, name):
    topo, ev = _base(gossip)
    tick = (ev["ns"] // L).astype(np.int64)
    if name == "own_tick":  # events 0, 7, 20 and 47: their node is down exactly in their generation tick
        outages = tuple((int(ev["node"][k]), int(tick[k]), int(tick[k]) + 1) for k in (0, 7, 20, 47))
    elif name == "whole_run":
        outages = tuple((int(v), 0, FOREVER) for v in np.unique(ev["node"][[1, 2, 30]]))
    else:
        outages = tuple((v, FIRST - 5, FOREVER) for v in range(topo.num_nodes))
    snaps = (T0 + 3 * L + L // 2, T0 + 5 * L + 7)
    eng = _engine(gossip, topo, ev, FAR, outages=outages, snaps=snaps)
    try:
        eng.run()
        got = _result(eng)
        snap = [eng.snapshot(i) for i in range(2)]
    finally:
        eng.close()
    want = _model(topo, ev, FAR, outages=outages)
    _same(got, want, ("dropped", name))
    dropped = np.array([R.down_mask(topo.num_nodes, outages, int(tick[k]))[ev["node"][k]] for k in range(len(ev))])
    assert got["faults"].dropped_generations == want["dropped"] == int(dropped.sum()) > 0
    assert not want["counted"][dropped].any()
    assert not got["reach"][dropped].any() and got["reach"][want["counted"]][:, 0].all()  # all-zero reach rows
    for i, ts in enumerate(snaps):
        assert snap[i][0] == ts and snap[i][2] == R.snapshot_total(want, ev, ts), (name, i)
        assert snap[i][1] == int(np.sum((ev["ns"] < ts) & want["counted"])), (name, i)  # not in the generation totals
    if name == "own_tick":
        assert want["dropped"] == 4 and int(want["gen"].sum()) == len(ev) - 4
    if name == "all_down":
        assert want["dropped"] == len(ev)
        for k in STAT_KEYS:
            assert not got[k].any(), k
        assert got["edge_events"] == 0 and not got["reach"].any() and len(got["trace"][0]) == 0
        assert snap[0][1] == snap[0][2] == 0
        f = got["faults"]
        assert f.lost_copies == 0 and f.down_node_ticks == f.launches * topo.num_nodes
        assert f.down_copies == f.launches * int(want["peers"].sum())


# ---- loss ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [0, 1 << 30, 1 << 31, ALWAYS])
def test_loss_on_the_ladder(gossip, thr):
    topo, ev, t_cut = _ladder(gossip)
    peers, sockets = topo.degrees()
    assert (peers > sockets).any()  # multiplicity 2: two copies, two draws
    got, want = _run(gossip, topo, ev, t_cut, ("loss", thr), loss_thr=thr, loss_seed=5, opts=dict(fanout_grid=1))
    full = _model(topo, ev, t_cut)
    if thr == 0:
        assert np.array_equal(got["recv"], full["recv"]) and got["faults"].lost_copies == 0
    elif thr == ALWAYS:
        assert not got["recv"].any() and np.array_equal(got["sent"], got["peers"].astype(np.uint64) * got["gen"])
        assert got["faults"].lost_copies == got["faults"].launches * int(peers.sum())
    else:
        assert 0 < int(got["recv"].sum()) < int(full["recv"].sum()) and got["faults"].lost_copies > 0
    # sent counts every made Send: the full degree of every node that processed a share
    assert np.array_equal(got["sent"], got["peers"].astype(np.uint64) * got["processed"])


# ---- with fanout -------------------------------------------------------------------------------------------------
def test_with_fanout_both_setter_orders_and_seeds(gossip):
    topo, ev = _base(gossip)
    outages = _crash(topo.num_nodes, 0.2, FIRST + 3)
    loss = gossip.loss_threshold(0.1)
    runs = {}
    for tag, last, seed in (("fanout_first", False, 1), ("fanout_last", True, 1), ("other_seed", False, 2)):
        runs[tag] = _run(gossip, topo, ev, FAR, ("fanout", tag), outages=outages, loss_thr=loss, loss_seed=9, k=3, fan_seed=seed,
                         fanout_last=last)
    a, b, c = (runs[t][0] for t in ("fanout_first", "fanout_last", "other_seed"))
    for k in STAT_KEYS + ("reach",):
        assert np.array_equal(a[k], b[k]), k  # a later fanout setter discards neither outages nor loss
    assert not np.array_equal(a["recv"], c["recv"])
    # the loss draw of a link does not change with the fanout seed: link by link, tick by tick
    la, lc = runs["fanout_first"][1]["lost_by_tick"], runs["other_seed"][1]["lost_by_tick"]
    common = sorted(set(la) & set(lc))
    assert len(common) >= 10 and all(np.array_equal(la[t], lc[t]) for t in common)
    assert 0.05 < np.mean([la[t].mean() for t in common]) < 0.15
    no_faults = F.run(topo.num_nodes, *topo.links(), ev, L, FAR, F.thresholds(3, topo.degrees()[0]), 1)
    assert 0 < int(a["recv"].sum()) < int(no_faults["recv"].sum())
    # fanout decides whether a Send is made: fewer than the flood's, and down nodes' Sends stop with them
    assert int(a["sent"].sum()) < int((a["peers"].astype(np.uint64) * a["processed"]).sum())
    f = a["faults"]
    assert f.lost_copies > 0 and f.down_copies > 0 and a["fanout"].selected_in < a["fanout"].selected_out


# ---- off means off ---------------------------------------------------------------------------------------------
def test_off_means_off(gossip):
    topo, ev = _base(gossip)
    t_cut = S.t_cut_for(6)
    res = {}
    for tag, kw in (("plain", {}), ("cleared", dict(outages=(), loss_thr=0))):
        eng = _engine(gossip, topo, ev, t_cut, **kw)
        try:
            eng.run()
            res[tag] = _result(eng)
        finally:
            eng.close()
    plain, off = res["plain"], res["cleared"]
    for k in STAT_KEYS + ("peers", "reach"):
        assert np.array_equal(plain[k], off[k]), k
    assert plain["edge_events"] == off["edge_events"]
    for x, y in zip(S.sorted_trace(plain["trace"]), S.sorted_trace(off["trace"])):
        assert np.array_equal(x, y)
    # an engine that calls neither setter launches nothing new
    assert not _records(plain, gossip)
    f = plain["faults"]
    assert (f.launches, f.down_node_ticks, f.lost_copies, f.down_copies, f.dropped_generations) == (0, 0, 0, 0, 0)
    assert plain["fanout"].launches == 0
    # cleared faults: the thinning path without the faults variant
    f = off["faults"]
    assert (f.launches, f.down_node_ticks, f.lost_copies, f.down_copies, f.dropped_generations) == (0, 0, 0, 0, 0)
    assert set(_records(off, gossip)) == {1, 2}


def test_second_call_replaces_and_reset_timing_clears(gossip):
    topo, ev = _base(gossip)
    first = _crash(topo.num_nodes, 0.5, FIRST, seed=8)
    outages = _crash(topo.num_nodes, 0.2, FIRST + 3)
    eng = gossip.Engine(topo.num_nodes, L, T0, FAR, flags=gossip.F_REACH)
    try:
        eng.set_topology(topo)
        o = np.array(first, np.int64)
        eng.set_outages(o[:, 0], o[:, 1], o[:, 2])
        eng.set_link_loss(1 << 31, 4)
        o = np.array(outages, np.int64)
        eng.set_outages(o[:, 0], o[:, 1], o[:, 2])   # replaces the first set
        eng.set_link_loss(0)                         # loss off again
        eng.set_schedule(ev)
        eng.run(FIRST + 10)
        eng.sync()
        assert eng.fault_counters().launches == 10
        eng.reset_timing()
        f = eng.fault_counters()
        assert (f.launches, f.down_node_ticks, f.lost_copies, f.down_copies) == (0, 0, 0, 0)
        eng.run()
        got = _result(eng, trace=False)
    finally:
        eng.close()
    want = _model(topo, ev, FAR, outages=outages)
    _same(got, want, "replaced", trace=False)
    assert got["faults"].launches == got["ticks"][1] - FIRST - 10 and got["faults"].dropped_generations == want["dropped"]


# ---- against ORACLE A ----------------------------------------------------------------------------------------------
def test_crash_set_against_oracle_a(gossip, oracle):
    topo, ev = _base(gossip)
    n, t_cut = topo.num_nodes, S.t_cut_for(6)
    outages = _crash(n, 0.2, 0, seed=17)
    is_c = np.zeros(n, bool)
    is_c[[o[0] for o in outages]] = True
    eng = _engine(gossip, topo, ev, t_cut, outages=outages)
    try:
        eng.run()
        got = _result(eng)
    finally:
        eng.close()
    a, b = topo.links()
    keep = ~is_c[a.astype(np.int64)] & ~is_c[b.astype(np.int64)]
    ev_up = ev[~is_c[ev["node"]]]
    r = oracle.run_replay(n, L, T0, t_cut, a[keep], b[keep], ev_up["ns"], ev_up["node"], ev_up["share_id"], trace=True)
    assert np.array_equal(got["recv"], r.recv) and int(r.recv.sum()) > 0
    node, sid, tick, hop, via = S.sorted_trace(got["trace"])
    tn, ti, tt, th, tv = S.sorted_trace(r.trace)
    g1, o1 = via == 1, tv == 1
    assert np.array_equal(node[g1], tn[o1]) and np.array_equal(sid[g1], ti[o1])
    assert np.array_equal(tick[g1], tt[o1] // L) and np.array_equal(hop[g1], th[o1])
    assert got["faults"].dropped_generations == int(is_c[ev["node"]].sum()) > 0


# ---- invariance ------------------------------------------------------------------------------------------------------
def _faulted(gossip):
    topo, ev = _base(gossip)
    return topo, ev, _crash(topo.num_nodes, 0.2, FIRST + 3), gossip.loss_threshold(0.1)


INVARIANTS = [("default", {}, 0), ("pull_grid", dict(pull_grid=1), 0), ("late_age", dict(late_age=0), 0),
              ("dense_rows", dict(dense_rows=1), 0), ("pull_batch", dict(pull_batch=1), 0), ("tile_per_tick", {}, 32)]


@pytest.mark.parametrize("name,opts,flags", INVARIANTS, ids=[i[0] for i in INVARIANTS])
def test_option_invariance(gossip, name, opts, flags):
    topo, ev, outages, loss = _faulted(gossip)
    assert flags in (0, gossip.F_TILE_PER_TICK)
    _run(gossip, topo, ev, S.t_cut_for(6), ("option", name), outages=outages, loss_thr=loss, loss_seed=9, opts=opts, flags=flags)


@pytest.mark.parametrize("count,by_tick", [(2, 0), (3, 0), (2, 1), (3, 1)])
def test_share_shards_add_up(gossip, count, by_tick):
    topo, ev, outages, loss = _faulted(gossip)
    fl = gossip.F_SHARD_BY_TICK if by_tick else 0
    want = _model(topo, ev, FAR, outages=outages, loss_thr=loss, loss_seed=9)
    parts = []
    for r in range(count):
        eng = _engine(gossip, topo, ev, FAR, outages=outages, loss_thr=loss, loss_seed=9, flags=fl, trace=False, shard_rank=r,
                      shard_count=count)
        try:
            eng.run()
            parts.append(_result(eng, trace=False))
        finally:
            eng.close()
    assert sum(int(p["gen"].sum()) > 0 for p in parts) >= 2  # the shares really are split
    tot = {k: sum(p[k].astype(np.uint64) for p in parts) for k in STAT_KEYS + ("reach",)}
    tot["edge_events"] = sum(p["edge_events"] for p in parts)
    _same(tot, want, ("shards", count, by_tick), trace=False)


# ---- stepping ------------------------------------------------------------------------------------------------------------
def test_stepping(gossip):
    topo, ev, outages, loss = _faulted(gossip)
    eng = _engine(gossip, topo, ev, FAR, outages=outages, loss_thr=loss, loss_seed=9)
    try:
        for t in range(eng.first_tick + 1, eng.end_tick + 1):  # tick by tick
            eng.run(t)
        got = _result(eng)
    finally:
        eng.close()
    want = _model(topo, ev, FAR, outages=outages, loss_thr=loss, loss_seed=9)
    _same(got, want, "stepping")
    one, _ = _run(gossip, topo, ev, FAR, "one run", outages=outages, loss_thr=loss, loss_seed=9)
    for k in STAT_KEYS + ("reach",):
        assert np.array_equal(got[k], one[k]), k
    assert [getattr(got["faults"], k) for k, _ in gossip.gossip_fault_counters._fields_] == \
           [getattr(one["faults"], k) for k, _ in gossip.gossip_fault_counters._fields_]


# ---- refusals ------------------------------------------------------------------------------------------------------------
def _refused(gossip, code, match, fn):
    with pytest.raises(gossip.GossipError, match=match) as e:
        fn()
    assert e.value.code == code


def test_refusals(gossip):
    topo, ev = _base(gossip)
    n = topo.num_nodes

    def make(flags=0, mode=None, part=None, opts=(), graph=True):
        eng = gossip.Engine(n, L, T0, FAR, flags=flags, mode=gossip.MODE_AUTO if mode is None else mode)
        if part:
            eng.set_row_partition(*part)
        for name, v in dict(opts).items():
            eng.set_option(name, v)
        if graph:
            eng.set_topology(topo)
        return eng

    def both(eng, code, match):
        _refused(gossip, code, match, lambda: eng.set_outages([1], [FIRST], [FIRST + 1]))
        _refused(gossip, code, match, lambda: eng.set_link_loss(0.5, 1))

    for kw, match in [(dict(flags=gossip.F_HOP_BATCH), "HOP_BATCH"), (dict(flags=gossip.F_HANDSHAKE), "HANDSHAKE"),
                      (dict(part=(0, 2)), "row partition"), (dict(mode=gossip.MODE_DENSE), "DENSE"),
                      (dict(opts=dict(young=1)), "young")]:
        eng = make(**kw)
        try:
            both(eng, gossip.E_INVAL, match)
        finally:
            eng.close()
    eng = make(graph=False)
    try:
        both(eng, gossip.E_STATE, "graph")
        eng.set_topology(topo)
        _refused(gossip, gossip.E_INVAL, "outage 1: node 1000", lambda: eng.set_outages([3, n], [FIRST, FIRST], [FIRST + 1, FIRST + 1]))
        _refused(gossip, gossip.E_INVAL, "outage 2: tick_from", lambda: eng.set_outages([3, 4, 5], FIRST, [FIRST + 1, FIRST + 2, FIRST]))
        _refused(gossip, gossip.E_INVAL, "outage 0: tick_from", lambda: eng.set_outages([3], [FIRST + 2], [FIRST + 1]))
        # a refused call left the engine as it was: not in the thinning mode, where forcing young on is refused
        eng.set_option("young", 1)
        eng.set_option("young", -1)
        eng.set_outages([3], [FIRST], [FIRST + 1])
        assert eng.mode == gossip.MODE_CSR
        _refused(gossip, gossip.E_INVAL, "young", lambda: eng.set_option("young", 1))  # forcing it on afterwards
        bad = ev.copy()  # colliding ids: the first collision is named
        bad["share_id"][5] = bad["share_id"][2]
        _refused(gossip, gossip.E_INVAL, f"unique share ids: id {int(bad['share_id'][5])} of node {int(bad['node'][5])}",
                 lambda: eng.set_schedule(bad))
        eng.set_schedule(gossip.unique_ids(bad))
        both(eng, gossip.E_STATE, "before the schedule")
    finally:
        eng.close()
    # AUTO on a graph dense enough for DENSE mode resolves to CSR once a fault setter ran
    dtopo = gossip.Topology.gnp(2048, 0.08, 3, gossip.TOPO_SKIP)
    eng = gossip.Engine(2048, L, T0, FAR)
    try:
        eng.set_topology(dtopo)
        assert eng.mode == gossip.MODE_DENSE
        eng.set_link_loss(0.5)
        assert eng.mode == gossip.MODE_CSR
    finally:
        eng.close()


# ---- the command-line tool -----------------------------------------------------------------------------------------------
def test_cli_outages_and_loss(gossip, tmp_path):
    from conftest import PKG
    sim = os.path.join(PKG, "lib", "gossip_sim")
    n, p, lat = 200, 0.04, 5_000_000
    t0, t_cut = gossip.seconds_to_ns(5.0), gossip.seconds_to_ns(8.9)
    topo = gossip.Topology.gnp(n, p, 5, gossip.TOPO_EXACT)
    ev = gossip.unique_ids(gossip.make_schedule(n, 6, t0, t_cut))
    rng = np.random.default_rng(4)
    ofile = tmp_path / "outages.txt"
    lines = [f"{int(v)} {t0 + int(rng.integers(0, 2_000_000_000))} {t0 + int(rng.integers(2_000_000_000, 4_000_000_000))}\n"
             for v in rng.choice(n, 60, replace=False)]
    lines.append(f"7 {t0 + 1} {t0 + 2}\n")  # an empty tick range: skipped
    ofile.write_text("".join(lines))
    nodes, tf, tt, skipped = gossip.load_outages(n, lat, str(ofile))
    assert len(nodes) == 60 and skipped == 1
    eng = gossip.Engine(n, lat, t0, t_cut, flags=gossip.F_REACH)
    try:
        eng.set_topology(topo)
        eng.set_outages(nodes, tf, tt)
        eng.set_link_loss(0.25, 5)
        eng.set_schedule(ev)
        eng.run()
        eng.sync()
        st, reach, fc = eng.stats(), eng.reach(), eng.fault_counters()
    finally:
        eng.close()
    assert fc.dropped_generations > 0 and fc.lost_copies > 0 and fc.down_copies > 0 and int(st.recv.sum()) > 0
    out = str(tmp_path / "reach.txt")
    args = [sim, f"--numNodes={n}", f"--connectionProb={p}", "--simTime=9", "--seed=5", "--nodeSeed=6", "--uniqueIds",
            "--outages", str(ofile), "--loss", "0.25", "--lossSeed", "5", "--reach", out]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert gossip.format_statistics(st) in r.stdout
    assert "60 interval(s)" in r.stdout and "1 line(s) with an empty tick range skipped" in r.stdout
    rows = [line.split() for line in open(out)]
    assert len(rows) == len(ev) and [int(x[3]) for x in rows] == reach.sum(axis=1).tolist()
    # a malformed outage line fails and names the line
    ofile.write_text(lines[0] + "12 abc 99\n")
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "line 2" in r.stderr and "outages.txt" in r.stderr
    # all three options need --uniqueIds
    r = subprocess.run([x for x in args if x != "--uniqueIds"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--uniqueIds" in r.stderr
    ofile.write_text(lines[0])
    for opt in (["--outages", str(ofile)], ["--loss", "0.25"], ["--lossSeed", "5"]):  # each one alone
        r = subprocess.run(args[:6] + opt, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--uniqueIds" in r.stderr, opt
    # a loss below 2^-32 would round to "off": refused, not run without loss
    r = subprocess.run(args[:7] + ["--loss", "1e-11"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "resolution" in r.stderr
