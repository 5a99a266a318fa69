"""Reach profiles (GOSSIP_F_REACH: k_reach + k_reach_slots, csrc/reach_kernel.h) against ORACLE A.

reach[k][h] = nodes whose first contact with event k's share came from k's column at hop h.  The
first-contact trace is the specification: every case histograms ORACLE A's trace by (share_id, hop)
and compares it with the engine's table summed over the events of each share_id; every case also
runs the engine with F_TRACE | F_REACH and asserts that the engine's own trace gives the same
histogram.  The cases walk the places a tick's new bits can live (dense rows behind occupancy bits,
young slots and overflowed nodes, folded rows masked by either source), the flush boundaries of the
bit planes, the hop clamp, DENSE mode, the fidelity layers and the sums over engines.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import structured as S
from cases import L, T0
from conftest import PKG

pytestmark = pytest.mark.gpu

RM_NZ, RM_WS, RM_FOLDF, RM_FOLDS = 1, 2, 4, 8  # k_reach's tile modes in the launch ledger (gossip.h)


def _hist(ids, sid, hop, hops):
    """(len(ids), hops) counts of trace records by (share_id, min(hop, hops - 1)); ids sorted, unique."""
    m = np.zeros((len(ids), hops), np.int64)
    idx = np.searchsorted(ids, sid)
    assert np.array_equal(ids[idx], sid)
    np.add.at(m, (idx, np.minimum(np.asarray(hop, np.int64), hops - 1)), 1)
    return m


def _by_id(ids, ev, table):
    """The per-event table summed over the events of each share_id."""
    m = np.zeros((len(ids), table.shape[1]), np.int64)
    np.add.at(m, np.searchsorted(ids, ev["share_id"]), table.astype(np.int64))
    return m


def _engine(gossip, topo, ev, t_cut, flags=0, opts=(), lat=L, mode=None, trace=True, link=None, part=None, **kw):
    fl = gossip.F_REACH | (gossip.F_TRACE if trace else 0) | flags
    eng = gossip.Engine(topo.num_nodes, lat, T0, t_cut, flags=fl, mode=gossip.MODE_AUTO if mode is None else mode, **kw)
    if part:
        eng.set_row_partition(*part)
    for k, v in dict(opts).items():
        eng.set_option(k, v)
    eng.set_topology(topo)
    if link:
        eng.set_link_timing(*link)
    eng.set_schedule(ev)
    return eng


def _check(gossip, eng, ev, r, what, hops=32):
    """The engine's table == ORACLE A's trace histogram == the engine's own trace histogram, the
    totals are the table's column sums, every tick was counted and every first contact is in it."""
    table = eng.reach()
    assert table.shape == (len(ev), hops) and table.dtype == np.uint32, what
    ids = np.unique(ev["share_id"])
    got = _by_id(ids, ev, table)
    want = _hist(ids, r.trace[1], r.trace[3], hops)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: reach differs from ORACLE A's trace in {len(bad)} (id, hop) bins, first "
                             f"{[(int(ids[i]), int(h), int(got[i, h]), int(want[i, h])) for i, h in bad[:6]]} (id, hop, engine, oracle)")
    node, sid, tick, hop, via = eng.trace()
    assert np.array_equal(got, _hist(ids, sid, hop, hops)), what
    tot = eng.reach_totals()
    assert tot.dtype == np.uint64 and np.array_equal(tot, table.astype(np.uint64).sum(axis=0)), what
    c = eng.counters()
    assert c.reach_launches == c.ticks > 0, what
    assert int(table.sum()) == int(eng.stats().processed.sum()) == len(r.trace[0]), what
    assert c.reach_bytes > 0, what
    c.launches = eng.launches()
    return table, c


def _reach_modes(c):
    """Union of the tile modes k_reach's launches covered, and the k_reach_slots variants that ran."""
    rows = [r.arg for r in c.launches if r.kernel == 5 and r.arg >= 16]
    slots = {r.arg for r in c.launches if r.kernel == 5 and r.arg < 16}
    return functools.reduce(lambda x, y: x | y, rows, 0) & 15, slots


def _oracle(oracle, topo, ev, t_cut, lat=L, **kw):
    a, b = topo.links()
    return oracle.run_replay(topo.num_nodes, lat, T0, t_cut, a, b, ev["ns"], ev["node"], ev["share_id"], trace=True, **kw)


@functools.lru_cache(maxsize=None)
def _gnp(gossip, oracle, n, deg, ticks, per_tick, seed):
    """G(n, p) of mean degree deg, per_tick births in each of `ticks` ticks, the cut inside the tick
    after the last birth tick (keep masks on floods still running), with ORACLE A's run."""
    topo = gossip.Topology.gnp(n, deg / (n - 1), seed, gossip.TOPO_SKIP)
    ev = S.events(n, ticks, per_tick, seed + 1)
    t_cut = S.t_cut_for(ticks)
    return topo, ev, t_cut, _oracle(oracle, topo, ev, t_cut)


@functools.lru_cache(maxsize=None)
def _family(gossip, oracle, name):
    f = S.family(name)
    topo = gossip.Topology.from_links(f["n"], f["a"], f["b"])
    return f, topo, _oracle(oracle, topo, f["ev"], f["t_cut"])


# ---- base ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pull_nt", [0, 1])
@pytest.mark.parametrize("young", [0, 1])
def test_base(gossip, oracle, young, pull_nt):
    topo, ev, t_cut, r = _gnp(gossip, oracle, 4096, 16.0, 24, 4, 301)
    eng = _engine(gossip, topo, ev, t_cut, gossip.F_TILE_PER_TICK, dict(young=young, pull_nt=pull_nt))
    try:
        eng.run()
        eng.sync()
        table, c = _check(gossip, eng, ev, r, ("base", young, pull_nt))
        assert c.words_hw > 64 and c.pull_nt == pull_nt
        modes, slots = _reach_modes(c)
        assert modes & RM_NZ
        assert (bool(modes & RM_WS) and slots == {1} and c.young_launches > 0) if young else (not slots and not modes & RM_WS)
        # unique ids: a share's row sums to the nodes it reached before the cut, its own node at hop 0
        sums = table.sum(axis=1)
        assert np.all(table[sums > 0, 0] == 1) and sums.max() <= 4096 and (sums > 1).any()
        h50, h90 = gossip.coverage_hops(table, 0.5), gossip.coverage_hops(table, 0.9)
        assert np.all((h50 >= 0) == (sums > 0)) and np.all(h50 <= h90)
    finally:
        eng.close()


# ---- flush boundaries of the bit planes, ragged row chunks -------------------------------------------
@pytest.mark.parametrize("flush", [1, 3, None])
@pytest.mark.parametrize("n", [4001, 130])
def test_flush_boundaries(gossip, oracle, n, flush):
    if n == 130:
        # the complete graph: at hop 1 a share's column is set in every row but its source's, within one
        # launch -- each lane adds 8 or 9 consecutive all-ones words of its column, across flushes at the
        # caps 1 and 3 and up the carry chain
        pairs = np.array([(i, j) for i in range(130) for j in range(i + 1, 130)], np.uint32)
        topo = gossip.Topology.from_links(130, pairs[:, 0].copy(), pairs[:, 1].copy())
        ev = S.events(130, 12, 2, 77)
        t_cut = T0 + 80 * L
        r = _oracle(oracle, topo, ev, t_cut)
    else:
        topo, ev, t_cut, r = _gnp(gossip, oracle, n, 16.0, 20, 2, 310 + n)
    opts = dict(young=0) if flush is None else dict(young=0, reach_flush=flush)
    eng = _engine(gossip, topo, ev, t_cut, gossip.F_TILE_PER_TICK, opts)
    try:
        assert eng.get_option("reach_flush") == (255 if flush is None else flush)
        eng.run()
        eng.sync()
        table, c = _check(gossip, eng, ev, r, ("flush", n, flush))
        if n == 130:
            assert np.all(table[:, 0] == 1) and np.all(table[:, 1] == 129) and np.all(table[:, 2:] == 0)
    finally:
        eng.close()


# ---- young slots: entries, overflowed nodes' dense rows, both k_reach_slots variants -----------------
@pytest.mark.parametrize("case", ["overflow", "skip", "many_tiles"])
def test_young_slots(gossip, oracle, case):
    f, topo, r = _family(gossip, oracle, "ladder")
    opts = {"overflow": dict(young=1, young_cap=3, young_list_cap=8, young_age=6, young_skip=1),
            "skip": dict(young=1, young_skip=1),
            "many_tiles": dict(young=1, young_age=12)}[case]
    eng = _engine(gossip, topo, f["ev"], f["t_cut"], gossip.F_TILE_PER_TICK, opts)
    try:
        eng.run()
        eng.sync()
        _, c = _check(gossip, eng, f["ev"], r, ("young", case))
        modes, slots = _reach_modes(c)
        assert c.young_launches > 0 and modes & RM_WS and slots, case
        if case == "overflow":
            assert c.young_fallback_rows > 0
        if case == "skip":
            assert c.young_skip_ticks > 0
        if case == "many_tiles":  # more write-sparse tiles than the LDS counter set holds: global atomics
            assert 2 in slots
        else:
            assert slots == {1}
    finally:
        eng.close()


# ---- folded rows: masked with the other frontier buffer and with the seen rows --------------------
@pytest.mark.parametrize("young", [0, 1])
def test_folded_rows(gossip, oracle, young):
    topo, ev, t_cut, r = _gnp(gossip, oracle, 4096, 16.0, 24, 4, 301)
    eng = _engine(gossip, topo, ev, t_cut, gossip.F_TILE_PER_TICK, dict(dense_rows=1, seen_fold=1, young=young))
    try:
        # tick by tick: the ledger shows, per launch, which mask sources k_reach used
        seen = set()
        while eng.current_tick < eng.end_tick:
            eng.run(eng.current_tick + 1)
            for rec in eng.launches():
                if rec.kernel == gossip.K_REACH and rec.arg >= 16:
                    seen.add(rec.arg & (RM_FOLDF | RM_FOLDS))
        eng.sync()
        _, c = _check(gossip, eng, ev, r, ("fold", young))
        assert c.pull_fold_rows > 0
        modes, _ = _reach_modes(c)
        # a tile's first folded tick is masked with its seen rows, the following ones with the other
        # buffer.  Without young tiles a tile stays folded for several ticks: both sources occur, in one
        # launch or another.  With them (young_age 5) a tile reaches k_pull at hop 6 of this 4-hop graph
        # and is folded for one tick only: the seen-row mask alone.  So the other-buffer mask is covered
        # by the young = 0 case only; the young = 1 case adds the seen-row mask beside write-sparse tiles.
        assert modes & RM_FOLDS, modes
        if not young:
            assert modes & RM_FOLDF, modes
        assert seen - {0} and all(m in (0, RM_FOLDS, RM_FOLDF, RM_FOLDS | RM_FOLDF) for m in seen), seen
    finally:
        eng.close()


# ---- id groups: several generations of one id, compared per share_id ------------------------------------
@pytest.mark.parametrize("young", [0, 1])
@pytest.mark.parametrize("name", ["ladder_collide", "components_collide"])
def test_id_groups(gossip, oracle, name, young):
    f, topo, r = _family(gossip, oracle, name)
    assert not f["unique"]
    eng = _engine(gossip, topo, f["ev"], f["t_cut"], gossip.F_TILE_PER_TICK if young else 0, dict(young=young))
    try:
        eng.run()
        eng.sync()
        table, _ = _check(gossip, eng, f["ev"], r, (name, young))
        assert (table.sum(axis=1) == 0).any()  # generations of an id their node had processed: all-zero rows
    finally:
        eng.close()


# ---- the hop clamp ----------------------------------------------------------------------------------
@pytest.mark.parametrize("hops", [32, 256])
def test_hop_clamp(gossip, oracle, hops):
    f, topo, r = _family(gossip, oracle, "long_ring")  # floods of 160 hops
    eng = _engine(gossip, topo, f["ev"], f["t_cut"], gossip.F_TILE_PER_TICK, dict(reach_hops=hops))
    try:
        eng.run()
        eng.sync()
        table, _ = _check(gossip, eng, f["ev"], r, ("clamp", hops), hops=hops)
        oh = np.asarray(r.trace[3], np.int64)
        assert oh.max() >= 159
        if hops == 32:
            assert int(table[:, 31].sum()) == int((oh >= 31).sum()) > 0
        else:
            assert table[:, 161:].sum() == 0 and int(table[:, 160].sum()) == int((oh == 160).sum())
            assert np.array_equal(table.astype(np.int64).sum(axis=0)[:161], np.bincount(oh, minlength=161)[:161])
    finally:
        eng.close()


# ---- DENSE mode: fused and three-kernel -------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("name", ["dense_sparse", "dense_tail[1025]"])
def test_dense_mode(gossip, oracle, name, fused):
    f, topo, r = _family(gossip, oracle, name)
    eng = _engine(gossip, topo, f["ev"], f["t_cut"], 0, dict(dense_fused=fused), mode=gossip.MODE_DENSE)
    try:
        eng.run()
        eng.sync()
        _, c = _check(gossip, eng, f["ev"], r, (name, fused))
        assert eng.mode == gossip.MODE_DENSE
        assert (c.dense_fused_launches == c.pull_launches) if fused else c.dense_fused_launches == 0
    finally:
        eng.close()


# ---- fidelity layers -----------------------------------------------------------------------------------
@pytest.mark.parametrize("link", [None, "5mbps"])
def test_hop_batch(gossip, oracle, link):
    n = 512
    topo = gossip.Topology.gnp(n, 0.02, 22, gossip.TOPO_EXACT)
    t_cut = gossip.seconds_to_ns(7.902)
    ev = gossip.make_schedule(n, 23, T0, t_cut)
    lt = gossip.LINK_5MBPS if link else None
    r = _oracle(oracle, topo, ev, t_cut, link_timing=lt)
    eng = _engine(gossip, topo, ev, t_cut, gossip.F_HOP_BATCH, link=lt)
    try:
        eng.run()
        eng.sync()
        _check(gossip, eng, ev, r, ("hop_batch", link))
    finally:
        eng.close()


def test_handshake_lost_births(gossip, oracle):
    n = 300
    topo = gossip.Topology.gnp(n, 0.03, 41, gossip.TOPO_EXACT)
    ev = S.events(n, 10, 6, 42)  # births from tick 0: ticks 0 and 1 are lost behind REGISTER
    t_cut = S.t_cut_for(10)
    r = _oracle(oracle, topo, ev, t_cut, handshake=(2 * L, 3 * L))
    eng = _engine(gossip, topo, ev, t_cut, gossip.F_HANDSHAKE)
    try:
        eng.run()
        eng.sync()
        table, _ = _check(gossip, eng, ev, r, "handshake")
        early = ev["ns"] < T0 + 2 * L
        sums = table.sum(axis=1)
        lost = early & (sums > 0)  # (a generation at a node without connector-side peers is not counted)
        assert lost.sum() > 0 and np.all(table[lost, 0] == 1) and np.all(sums[lost] == 1)
        # births once the sockets are ESTABLISHED, with ticks to spare before the cut, do flood
        mid = (ev["ns"] >= T0 + 2 * L) & (ev["ns"] < T0 + 6 * L) & (sums > 0)
        assert mid.sum() > 0 and np.all(sums[mid] > 1)
    finally:
        eng.close()


# ---- sums over engines ---------------------------------------------------------------------------------
@pytest.mark.parametrize("by_tick", [0, 1])
def test_share_shards_sum(gossip, oracle, by_tick):
    topo, ev, t_cut, r = _gnp(gossip, oracle, 4001, 16.0, 20, 2, 310 + 4001)
    fl = gossip.F_TILE_PER_TICK | (gossip.F_SHARD_BY_TICK if by_tick else 0)
    one = _engine(gossip, topo, ev, t_cut, fl, trace=False)
    parts = [_engine(gossip, topo, ev, t_cut, fl, trace=False, shard_rank=k, shard_count=2) for k in range(2)]
    try:
        for e in [one] + parts:
            e.run()
            e.sync()
        want = one.reach()
        tabs = [e.reach() for e in parts]
        owner = gossip.shard_events(topo, ev, 2, L if by_tick else 0)
        for k in range(2):  # a shard's table is zero for the events it does not own
            assert tabs[k][owner != k].sum() == 0 and tabs[k][owner == k].sum() > 0
        assert np.array_equal(tabs[0] + tabs[1], want)
        assert np.array_equal(parts[0].reach_totals() + parts[1].reach_totals(), one.reach_totals())
        ids = np.unique(ev["share_id"])
        assert np.array_equal(_by_id(ids, ev, want), _hist(ids, r.trace[1], r.trace[3], 32))
    finally:
        for e in [one] + parts:
            e.close()


def test_row_partition_sum(gossip, oracle):
    n = 1500
    topo = gossip.Topology.gnp(n, 0.01, 31, gossip.TOPO_EXACT)
    t_cut = gossip.seconds_to_ns(7.3)
    ev = gossip.make_schedule(n, 32, T0, t_cut)
    r = _oracle(oracle, topo, ev, t_cut)
    one = _engine(gossip, topo, ev, t_cut, mode=gossip.MODE_CSR)
    ranks = [_engine(gossip, topo, ev, t_cut, mode=gossip.MODE_CSR, trace=False, part=(k, 2)) for k in range(2)]
    try:
        one.run()
        one.sync()
        want, _ = _check(gossip, one, ev, r, "row partition, one engine")
        gossip.group_run(ranks)
        for e in ranks:
            e.sync()
        tabs = [e.reach() for e in ranks]
        assert tabs[0].sum() > 0 and tabs[1].sum() > 0
        assert np.array_equal(tabs[0] + tabs[1], want)
        # a rank counts its own rows: the hop-0 bin of an event is on the rank that owns its node
        own0 = ev["node"] < 1024
        assert np.array_equal(tabs[0][:, 0] > 0, own0 & (want[:, 0] > 0))
    finally:
        for e in [one] + ranks:
            e.close()


# ---- unique ids: the BFS layer sizes, a reference independent of ORACLE A -------------------------------
@pytest.mark.parametrize("name", ["tail[129]", "ladder"])
def test_bfs_closed_form(gossip, oracle, name):
    f, topo, r = _family(gossip, oracle, name)
    assert f["unique"]
    eng = _engine(gossip, topo, f["ev"], f["t_cut"])
    try:
        eng.run()
        eng.sync()
        table, _ = _check(gossip, eng, f["ev"], r, name)  # ORACLE A: never skipped
    finally:
        eng.close()
    try:
        import scipy  # noqa: F401  (bfs_reference needs it)
    except ImportError:
        return  # only the closed-form comparison is left out
    b = S.bfs_reference(f["n"], f["a"], f["b"], f["ev"], L, f["t_cut"])
    ids = np.unique(f["ev"]["share_id"])
    assert np.array_equal(_by_id(ids, f["ev"], table), _hist(ids, b["trace"][1], b["trace"][3], 32))


# ---- ABI errors ----------------------------------------------------------------------------------------
def test_abi_errors(gossip):
    n = 64
    topo = gossip.Topology.gnp(n, 0.1, 5, gossip.TOPO_EXACT)
    ev = S.events(n, 4, 2, 6)
    t_cut = S.t_cut_for(4)

    def expect(code, fn):
        with pytest.raises(gossip.GossipError) as e:
            fn()
        assert e.value.code == code, (e.value.code, str(e.value))

    off = gossip.Engine(n, L, T0, t_cut)  # without the flag
    try:
        off.set_topology(topo)
        off.set_schedule(ev)
        off.run()
        off.sync()
        expect(gossip.E_STATE, off.reach)
        expect(gossip.E_STATE, off.reach_totals)
        assert not [r for r in off.launches() if r.kernel == gossip.K_REACH]
        assert off.counters().reach_launches == 0
    finally:
        off.close()
    on = gossip.Engine(n, L, T0, t_cut, flags=gossip.F_REACH)
    try:
        for name, bad in (("reach_hops", 1), ("reach_hops", 1025), ("reach_shares", 2), ("reach_flush", 0), ("reach_flush", 256)):
            expect(gossip.E_INVAL, lambda: on.set_option(name, bad))
        on.set_option("reach_hops", 8)
        on.set_topology(topo)
        expect(gossip.E_STATE, on.reach_totals)  # before the schedule
        on.set_schedule(ev)
        expect(gossip.E_STATE, lambda: on.set_option("reach_hops", 16))
        expect(gossip.E_STATE, lambda: on.set_option("reach_shares", 0))
        on.run()
        on.sync()
        assert on.reach().shape == (len(ev), 8) and on.reach(len(ev), 0).shape == (0, 8)
        expect(gossip.E_INVAL, lambda: on.reach(0, len(ev) + 1))
        expect(gossip.E_INVAL, lambda: on.reach(len(ev), 1))
        expect(gossip.E_INVAL, lambda: on.reach(len(ev) + 1, 0))
        import ctypes as C
        lib = gossip.load_library()
        short = np.zeros(7, np.uint64)
        h = C.c_uint32()
        assert lib.gossip_engine_get_reach_totals(on._h, 7, C.c_void_p(short.ctypes.data), C.byref(h)) == gossip.E_INVAL
        assert h.value == 8 and short.sum() == 0
        assert [r for r in on.launches() if r.kernel == gossip.K_REACH]
    finally:
        on.close()
    os.environ["GOSSIP_REACH"] = "1"  # the environment default sets the flag at creation
    try:
        envd = gossip.Engine(n, L, T0, t_cut)
    finally:
        del os.environ["GOSSIP_REACH"]
    try:
        envd.set_topology(topo)
        envd.set_schedule(ev)
        envd.run()
        envd.sync()
        assert int(envd.reach().sum()) == int(envd.stats().processed.sum()) > 0
    finally:
        envd.close()
    tot = gossip.Engine(n, L, T0, t_cut, flags=gossip.F_REACH)  # totals only
    try:
        tot.set_option("reach_shares", 0)
        tot.set_topology(topo)
        tot.set_schedule(ev)
        tot.run()
        tot.sync()
        expect(gossip.E_STATE, tot.reach)
        assert int(tot.reach_totals().sum()) == int(tot.stats().processed.sum()) > 0
    finally:
        tot.close()


# ---- Python front end and the command-line tool ------------------------------------------------------
def test_simulation_keeps_the_profile_summed_over_shards(gossip):
    sims = []
    for shards in (1, 2):
        s = gossip.P2PGossipNetworkSimulation(64, topo_seed=3, node_seed=1003, shards=shards)
        s.CreateRandomTopology(0.1, 5.0)
        s.Start(9.0, reach=True)
        sims.append(s)
    assert sims[0].reach.shape == (len(sims[0].events), 32) and sims[0].reach.sum() == sims[0].stats.processed.sum()
    assert np.array_equal(sims[0].reach, sims[1].reach) and sims[1].shards_used == 2
    plain = gossip.P2PGossipNetworkSimulation(64, topo_seed=3, node_seed=1003)
    plain.CreateRandomTopology(0.1, 5.0)
    plain.Start(9.0)
    assert plain.reach is None


@pytest.mark.parametrize("extra", [(), ("--shards=2",), ("--hopBatch",), ("--linkTiming",), ("--handshake",)])
def test_cli_reach_file(gossip, tmp_path, extra):
    exe = os.path.join(PKG, "lib", "gossip_sim")
    base = [exe, "--numNodes=64", "--connectionProb=0.1", "--simTime=9", "--Latency=5", "--seed=3", "--nodeSeed=1003"]
    out = str(tmp_path / "reach.txt")
    a = subprocess.run(base + list(extra), capture_output=True, text=True, timeout=120)
    b = subprocess.run(base + list(extra) + ["--reach", out], capture_output=True, text=True, timeout=120)
    assert a.returncode == 0 and b.returncode == 0, a.stderr[-2000:] + b.stderr[-2000:]
    assert a.stdout == b.stdout  # the report does not change by one byte
    t_cut = gossip.seconds_to_ns(9.0 - 0.1)
    topo = gossip.Topology.gnp(64, 0.1, 3, gossip.TOPO_EXACT)
    ev = gossip.make_schedule(64, 1003, T0, t_cut)
    fl = {"--hopBatch": gossip.F_HOP_BATCH, "--linkTiming": gossip.F_HOP_BATCH, "--handshake": gossip.F_HANDSHAKE}
    eng = _engine(gossip, topo, ev, t_cut, sum(fl.get(x, 0) for x in extra), trace=False,
                  link=gossip.LINK_5MBPS if "--linkTiming" in extra else None)
    try:
        eng.run()
        eng.sync()
        table = eng.reach().astype(np.int64)
    finally:
        eng.close()
    lines = open(out).read().splitlines()
    assert len(lines) == len(ev) > 0
    h50, h90 = gossip.coverage_hops(table, 0.5), gossip.coverage_hops(table, 0.9)
    for k, line in enumerate(lines):
        x = [int(v) for v in line.split()]
        row = table[k]
        last = int(np.flatnonzero(row).max()) if row.any() else -1
        assert x[:3] == [int(ev["ns"][k]), int(ev["node"][k]), int(ev["share_id"][k])], k
        assert x[3:7] == [int(row.sum()), int(h50[k]), int(h90[k]), last], (k, line)
        assert x[7:] == row[:last + 1].tolist(), (k, line)
    assert table.sum() > len(ev)
