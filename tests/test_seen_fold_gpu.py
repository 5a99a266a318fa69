"""Seen bits carried in dense frontier rows (option seen_fold, tmask TM_FOLDW / TM_SEENF) against ORACLE A.

A sealed tile (not open, every member of its id instances born) that k_pull reads as dense rows and
writes whole keeps its seen bits in the F_next row (seen | new) and writes no seen row; the next tick
reads the seen pair back from the node's own F_cur row, and the tick the tile stops being written
whole, nodes still unsaturated in it store the pair once.  Peers read folded rows: the old bits in
them change nothing a peer takes, so the seven per-node counters and the
first-contact trace must stay bit-exact.

Every case runs with dense_rows = 1 (every listed tile at hop >= 1 is written whole, so tiny graphs
have dense-row ticks) and a fresh tile per tick (F_TILE_PER_TICK: tiles seal the tick after they
open, and the window is wider than 64 words -- the one-peer-walk kernels that keep saturation bits),
compares with ORACLE A and asserts from pull_fold_rows that rows really were folded.
"""
import functools

import numpy as np
import pytest

import structured as S
from cases import L, T0

pytestmark = pytest.mark.gpu

STATS = ("gen", "recv", "fwd", "sent", "processed", "peers", "sockets")


def _run(gossip, topo, ev, t_cut, opts=(), mid=None, trace=True, lat=L):
    """One engine, dense_rows = 1 and a fresh tile per tick: (stats, counters, trace, mid counters).
    mid = (k, fn): the run stops after k ticks, reads the counters and calls fn(engine)."""
    fl = gossip.F_TILE_PER_TICK | (gossip.F_TRACE if trace else 0)
    eng = gossip.Engine(topo.num_nodes, lat, T0, t_cut, flags=fl)
    try:
        eng.set_option("dense_rows", 1)
        for k, v in dict(opts).items():
            eng.set_option(k, v)
        eng.set_topology(topo)
        eng.set_schedule(ev)
        midc = None
        if mid is not None:
            eng.run(eng.first_tick + mid[0])
            eng.sync()
            midc = eng.counters()
            mid[1](eng)
        eng.run()
        eng.sync()
        return eng.stats(), eng.counters(), eng.trace() if trace else None, midc
    finally:
        eng.close()


def _oracle(oracle, topo, ev, t_cut, lat=L):
    a, b = topo.links()
    return oracle.run_replay(topo.num_nodes, lat, T0, t_cut, a, b, ev["ns"], ev["node"], ev["share_id"], trace=True)


def _parity(st, tr, r, what, lat=L):
    for k in STATS:
        got, want = getattr(st, k), getattr(r, k)
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{what}: {k} differs at {len(bad)} nodes, first {bad[:8].tolist()}: "
                                 f"engine {got[bad[:8]].tolist()} oracle {want[bad[:8]].tolist()}")
    node, sid, tick, hop, via = S.sorted_trace(tr)
    tn, ti, tt, th, tv = S.sorted_trace(r.trace)
    assert np.array_equal(node, tn) and np.array_equal(sid, ti), what
    assert np.array_equal(tick, tt // lat), what
    assert np.array_equal(hop, th), what
    assert np.array_equal(via, tv), what
    assert int(r.recv.sum()) > 0


def _same_stats(x, y, what):
    for k in STATS:
        assert np.array_equal(getattr(x, k), getattr(y, k)), (what, k)


@functools.lru_cache(maxsize=None)
def _gnp(gossip, oracle, n, deg, ticks, per_tick, seed):
    """G(n, p) with mean degree `deg`, per_tick births in each of `ticks` ticks and a cut inside the tick
    after the last birth tick (floods still running: the last tick has keep masks), with ORACLE A's run."""
    topo = gossip.Topology.gnp(n, deg / (n - 1), seed, gossip.TOPO_SKIP)
    ev = S.events(n, ticks, per_tick, seed + 1)
    t_cut = S.t_cut_for(ticks)
    return topo, ev, t_cut, _oracle(oracle, topo, ev, t_cut)


# ---- base parity and byte check ----------------------------------------------------------------
@pytest.mark.parametrize("pull_nt", [0, 1])
@pytest.mark.parametrize("young", [0, 5])
def test_base_parity_and_bytes(gossip, oracle, young, pull_nt):
    topo, ev, t_cut, r = _gnp(gossip, oracle, 4096, 16.0, 24, 4, 301)
    yo = dict(young=1, young_age=young) if young else dict(young=0)
    opts = dict(yo, pull_nt=pull_nt)
    st1, c1, tr1, _ = _run(gossip, topo, ev, t_cut, dict(opts, seen_fold=1))
    what = ("base", young, pull_nt)
    _parity(st1, tr1, r, what)
    st0, c0, _, _ = _run(gossip, topo, ev, t_cut, dict(opts, seen_fold=0), trace=False)
    _same_stats(st0, st1, what)
    assert c1.pull_nt == pull_nt and c1.pull_lpw == 32 and c1.words_hw > 64, what
    assert c1.young_launches > 0 if young else c1.young_launches == 0, what
    print(f"{what}: fold rows {c1.pull_fold_rows}, seen writes {c0.pull_seen_writes} -> {c1.pull_seen_writes}, "
          f"seen reads {c0.pull_seen_reads} -> {c1.pull_seen_reads}, F writes {c0.pull_f_writes} -> {c1.pull_f_writes}")
    assert c1.pull_fold_rows > 0 and c0.pull_fold_rows == 0, what
    # Fewer seen pairs written.  With young_age = 5 there is none to save on this graph: 16^3 already
    # equals n, so no node is six hops from a source, k_pull's first tick on a tile (hop 6) brings nothing
    # new and k_pull writes no seen pair at all, folded or not (measured: 0 and 0; young off: 961,837
    # and 801,551 pairs) -- "lower" can only be asked where the unfolded run writes some.
    assert c1.pull_seen_writes < c0.pull_seen_writes or c0.pull_seen_writes == 0, what
    assert young or c0.pull_seen_writes > 0, what
    # the seen pair is read from one place or the other, the rows written whole are the same rows
    assert c1.pull_seen_reads == c0.pull_seen_reads and c1.pull_f_writes == c0.pull_f_writes, what
    assert c1.pull_pair_edges <= c0.pull_pair_edges, what  # (old bits in a row only cover more)


# ---- node-count tails ---------------------------------------------------------------------------
@pytest.mark.parametrize("gate", [1, 0])
@pytest.mark.parametrize("n", [4001, 130])
def test_node_count_tails(gossip, oracle, n, gate):
    # 4001 = 62 x 64 + 33 and 130 = 2 x 64 + 2: ragged last 64-node chunks; pull_gate 0 runs the kernel
    # that takes its saturation bits and fold flags at run time
    topo, ev, t_cut, r = _gnp(gossip, oracle, n, 16.0 if n > 1000 else 6.0, 20, 2, 310 + n)
    st, c, tr, _ = _run(gossip, topo, ev, t_cut, dict(seen_fold=1, young=0, pull_gate=gate))
    _parity(st, tr, r, ("tail", n, gate))
    assert c.pull_fold_rows > 0 and c.pull_sat == 1 and c.words_hw > 64, (n, gate)


# ---- hubs above one lane group's peers ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _family(gossip, oracle, name):
    f = S.family(name)
    topo = gossip.Topology.from_links(f["n"], f["a"], f["b"])
    return f, topo, _oracle(oracle, topo, f["ev"], f["t_cut"])


@pytest.mark.parametrize("young", [0, 1])
def test_hub_ladder(gossip, oracle, young):
    # hubs of degree 33 .. 257: the extra peer chunks of k_pull<32, 1>, beside degree-2..4 leaves
    f, topo, r = _family(gossip, oracle, "ladder")
    st, c, tr, _ = _run(gossip, topo, f["ev"], f["t_cut"], dict(seen_fold=1, young=young))
    _parity(st, tr, r, ("ladder", young))
    assert c.pull_fold_rows > 0 and c.pull_lpw == 32, young


# ---- colliding ids ------------------------------------------------------------------------------
def _collide_events(n, late):
    """Ticks 0 and 1: 12 births each over 6 ids (id groups of 4, two members per tick), and a unique id
    per tick; ticks 2 .. 11: one unique id per tick (the window stays wide, tiles keep sealing).
    late: one more member of id 3 is born at tick 6, six ticks after the group's first."""
    rng = np.random.default_rng(77)
    nodes = rng.permutation(n)  # every event at a node of its own
    phase = 1 + rng.permutation(n).astype(np.int64) * ((L - 2) // n)  # distinct phases in [1, L)
    rows, k = [], 0
    for t in range(12):
        ids = [1 + j % 6 for j in range(12)] if t < 2 else []
        ids.append(1000 + t)
        if late and t == 6:
            ids.append(3)
        for i in ids:
            v = int(nodes[k])
            k += 1
            rows.append((T0 + t * L + int(phase[v]), v, i))
    rows.sort()
    ev = np.empty(len(rows), S.GEN_EVENT_DTYPE)
    ev["ns"], ev["node"], ev["share_id"] = zip(*rows)
    return ev


@pytest.mark.parametrize("late", [False, True], ids=["all_born_early", "late_member"])
def test_colliding_ids(gossip, oracle, late):
    # early: the group tiles of ticks 0 and 1 seal at tick 2 and fold with WF_GROUP words (group_fix
    # reads the seen pair out of the F_cur row).  late: the tick-0 tile holds an instance with an unborn
    # member until tick 6 and must not fold before it; the other tiles fold meanwhile.
    n = 2000
    topo = gossip.Topology.gnp(n, 6.0 / (n - 1), 320, gossip.TOPO_SKIP)
    ev = _collide_events(n, late)
    t_cut = T0 + 30 * L
    r = _oracle(oracle, topo, ev, t_cut)
    st, c, tr, _ = _run(gossip, topo, ev, t_cut, dict(seen_fold=1, young=0))
    _parity(st, tr, r, ("collide", late))
    assert c.pull_fold_rows > 0 and c.words_hw > 64, late
    st0, c0, _, _ = _run(gossip, topo, ev, t_cut, dict(seen_fold=0, young=0), trace=False)
    _same_stats(st0, st, ("collide", late))
    if late:  # the tile that waits for its late member folds on fewer ticks
        early = _run(gossip, topo, _collide_events(n, False), t_cut, dict(seen_fold=1, young=0), trace=False)[1]
        assert c.pull_fold_rows < early.pull_fold_rows, (c.pull_fold_rows, early.pull_fold_rows)


# ---- leaving the folded state -------------------------------------------------------------------
def test_exit_with_unsaturated_nodes(gossip, oracle):
    # dense_rows off in the middle of the floods: the next tick no tile is written whole, so every
    # folded tile exits at once, most of its nodes still unsaturated -- each stores its seen pair
    topo, ev, t_cut, r = _gnp(gossip, oracle, 4096, 16.0, 24, 4, 301)
    st, c, tr, mid = _run(gossip, topo, ev, t_cut, dict(seen_fold=1, young=0),
                          mid=(12, lambda eng: eng.set_option("dense_rows", 0)))
    _parity(st, tr, r, "exit")
    assert mid.pull_fold_rows > 0 and c.pull_fold_rows == mid.pull_fold_rows  # (no folding after the switch)
    # seen_fold off mid-run is an exit tick as well
    st, c, tr, mid = _run(gossip, topo, ev, t_cut, dict(seen_fold=1, young=0),
                          mid=(9, lambda eng: eng.set_option("seen_fold", 0)))
    _parity(st, tr, r, "exit by option")
    assert mid.pull_fold_rows > 0 and c.pull_fold_rows == mid.pull_fold_rows


def test_cut_tick_after_folded_ticks(gossip, oracle):
    # the cut falls inside the floods' last tick: keep masks on tiles folded the tick before (they exit
    # there, every node storing its seen pair: a keep tick leaves no tile saturated)
    topo, ev, t_cut, r = _gnp(gossip, oracle, 4096, 16.0, 24, 4, 301)
    st, c, tr, mid = _run(gossip, topo, ev, t_cut, dict(seen_fold=1, young=0), mid=(24, lambda eng: None))
    _parity(st, tr, r, "cut")
    assert c.ticks == mid.ticks + 1 and mid.pull_fold_rows > 0  # (the cut tick is the last one)
    assert c.pull_fold_rows == mid.pull_fold_rows  # the cut tick folds nothing


# ---- a window above one k_pull launch -------------------------------------------------------------
def test_wide_window_two_launches(gossip, oracle):
    # 160-hop floods on a ring, a fresh tile per tick: above 2,048 words (two launches per tick, three
    # occupancy words, the rows widened mid-run with folded tiles alive)
    f, topo, r = _family(gossip, oracle, "long_ring")
    st, c, tr, _ = _run(gossip, topo, f["ev"], f["t_cut"], dict(seen_fold=1, young=0))
    _parity(st, tr, r, "long_ring")
    assert c.words_hw > 2048 and c.pull_fold_rows > 0 and c.pull_lpw == 32


# ---- options that would strand the folded state ---------------------------------------------------
def test_option_guard(gossip, oracle):
    topo, ev, t_cut, r = _gnp(gossip, oracle, 4096, 16.0, 24, 4, 301)
    eng = gossip.Engine(topo.num_nodes, L, T0, t_cut, flags=gossip.F_TILE_PER_TICK)
    try:
        assert eng.get_option("seen_fold") == -1  # auto
        eng.set_option("dense_rows", 1)
        eng.set_option("young", 0)
        eng.set_option("pull_sat", 0)  # before the first tick: settable as ever
        eng.set_option("pull_sat", 1)
        for bad in (-2, 2):
            with pytest.raises(gossip.GossipError) as ei:
                eng.set_option("seen_fold", bad)
            assert ei.value.code == gossip.E_INVAL
        eng.set_topology(topo)
        eng.set_schedule(ev)
        eng.set_option("pull_tiles", 0)
        eng.set_option("pull_tiles", 1)
        eng.run(eng.first_tick + 10)
        eng.sync()
        assert eng.counters().pull_fold_rows > 0
        for name in ("pull_sat", "pull_tiles"):
            with pytest.raises(gossip.GossipError) as ei:
                eng.set_option(name, 0)
            assert ei.value.code == gossip.E_INVAL and "fold" in str(ei.value), name
            eng.set_option(name, 1)  # (what it holds already)
        eng.run()
        eng.sync()
        _same_stats(eng.stats(), r, "guard")
    finally:
        eng.close()
