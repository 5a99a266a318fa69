"""Degree-ordered peer lists (option peer_order) and k_pull's batch schedule on exit-likely passes
(option pull_batch) against ORACLE A.

Neither option may change a result: peer_order only permutes the rows of the engine's CSR (which
peer rows k_pull reads before the bottom-up early exit fires), pull_batch only changes how many
peer rows a batch holds (when the exit is tested).  Every combination is compared bit for bit with
ORACLE A -- the seven per-node counters and the first-contact trace -- on the late-exit workload
(id groups, a cut inside a tick, young tiles on and off), on the degree ladder (degree ties, rows of
more than 32 peers, multiplicity in `sent`) and on node counts that leave a ragged last 64-node
chunk; on a 200,000-node graph the two options together must read strictly fewer peer rows.
"""
import numpy as np
import pytest

import structured as S
from cases import L, T0

pytestmark = pytest.mark.gpu

STATS = ("gen", "recv", "fwd", "sent", "processed", "peers", "sockets")
COMBOS = [(0, 0), (0, 1), (1, 0), (1, 1)]  # (peer_order, pull_batch)


def _engine(gossip, n, lat, t_cut, ev, opts, flags, topo=None, graph=None):
    eng = gossip.Engine(n, lat, T0, t_cut, flags=flags)
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        if graph is not None:
            eng.set_graph(*graph)
        else:
            eng.set_topology(topo)
        eng.set_schedule(ev)
        eng.run()
        eng.sync()
        tr = eng.trace() if flags & gossip.F_TRACE else None
        return eng.stats(), eng.counters(), tr
    finally:
        eng.close()


def _assert_parity(st, tr, r, lat, what):
    for k in STATS:
        got, want = getattr(st, k), getattr(r, k)
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{what}: {k} differs at {len(bad)} nodes, first {bad[:8].tolist()}: "
                                 f"engine {got[bad[:8]].tolist()} oracle {want[bad[:8]].tolist()}")
    node, sid, tick, hop, via = S.sorted_trace(tr)
    tn, ti, tt, th, tv = S.sorted_trace(r.trace)
    assert np.array_equal(node, tn) and np.array_equal(sid, ti), what
    assert np.array_equal(tick, tt // lat) and np.array_equal(hop, th), what
    assert np.array_equal(via, tv), what
    assert int(r.recv.sum()) > 0, what


# ---- 1. the late-exit workload (test_late_exit_gpu.py::late_case) ---------------------------------
@pytest.fixture(scope="module")
def late_case(gossip, oracle):
    n = 6000
    topo = gossip.Topology.gnp(n, 16.0 / (n - 1), 91, gossip.TOPO_SKIP)
    lat = gossip.milliseconds_to_ns(5.0)
    t_cut = gossip.seconds_to_ns(6.37)  # a cut inside a tick: keep masks on late words
    ev = gossip.make_schedule(n, 92, T0, t_cut, id_mask=0x3FFF)  # id groups
    a, b = topo.links()
    r = oracle.run_replay(n, lat, T0, t_cut, a, b, ev["ns"], ev["node"], ev["share_id"], trace=True)
    return topo, lat, t_cut, ev, r


@pytest.mark.parametrize("young", [1, 0])
@pytest.mark.parametrize("peer_order,pull_batch", COMBOS)
def test_late_case_matches_oracle(gossip, late_case, peer_order, pull_batch, young):
    topo, lat, t_cut, ev, r = late_case
    # a fresh tile per tick: a window wider than 64 words, the one-peer-walk-per-node k_pull<32, 1>
    yo = dict(young=1, young_age=2) if young else dict(young=0)
    opts = dict(yo, peer_order=peer_order, pull_batch=pull_batch)
    st, c, tr = _engine(gossip, topo.num_nodes, lat, t_cut, ev, opts, gossip.F_TRACE | gossip.F_TILE_PER_TICK,
                        topo=topo)
    assert c.words_hw > 64 and c.pull_lpw == 32
    assert (c.young_launches > 0) == bool(young)
    _assert_parity(st, tr, r, lat, ("late_case", peer_order, pull_batch, young))


# ---- 2. the degree ladder: ties, rows of more than 32 peers, multiplicity -------------------------
@pytest.mark.parametrize("peer_order,pull_batch", [(1, 1), (1, 0), (0, 1)])
@pytest.mark.parametrize("name", ["ladder", "ladder_parallel", "ladder_collide"])
def test_ladder_matches_oracle(gossip, oracle, name, peer_order, pull_batch):
    f = S.family(name)
    topo = gossip.Topology.from_links(f["n"], f["a"], f["b"])
    r = oracle.run_replay(f["n"], L, T0, f["t_cut"], f["a"], f["b"], f["ev"]["ns"], f["ev"]["node"],
                          f["ev"]["share_id"], trace=True)
    opts = dict(peer_order=peer_order, pull_batch=pull_batch)
    st, c, tr = _engine(gossip, f["n"], L, f["t_cut"], f["ev"], opts, gossip.F_TRACE | gossip.F_TILE_PER_TICK,
                        topo=topo)
    assert c.words_hw > 64 and c.pull_lpw == 32
    if name == "ladder_parallel":
        assert (st.peers > st.sockets).any()  # multiplicity: sent counts every copy
    _assert_parity(st, tr, r, L, (name, peer_order, pull_batch))


# ---- 3. node-count tails: steps of the last 64-node chunk that lie wholly past n ------------------
@pytest.mark.parametrize("pull_push", [0, 1])
@pytest.mark.parametrize("n", [193, 223, 254])  # n % 64 = 1, 31, 62
def test_node_count_tails(gossip, oracle, n, pull_push):
    assert n % 64 in (1, 31, 62)
    _, a, b = S.ring_chords(n, 7)
    ev = S.events(n, 12, 2, 100 + n)
    t_cut = S.t_cut_for(12)
    topo = gossip.Topology.from_links(n, a, b)
    r = oracle.run_replay(n, L, T0, t_cut, a, b, ev["ns"], ev["node"], ev["share_id"], trace=True)
    for pull_batch in (0, 1):
        opts = dict(pull_push=pull_push, pull_batch=pull_batch)
        st, c, tr = _engine(gossip, n, L, t_cut, ev, opts, gossip.F_TRACE | gossip.F_TILE_PER_TICK, topo=topo)
        assert c.words_hw > 64 and c.pull_lpw == 32 and c.pull_sat == 1  # the tile-list k_pull<32, 1>
        if pull_push == 0:  # the instantiation without push marks: it runs every step of a chunk
            assert c.pull_push_tiles == 0 and c.pull_pushw_tiles == 0 and c.pull_marks == 0
        _assert_parity(st, tr, r, L, ("tail", n, pull_push, pull_batch))


# ---- 4. fewer peer rows ---------------------------------------------------------------------------
def test_reads_fewer_rows(gossip):
    # the workload of test_late_exit_reads_fewer_rows: 200k nodes, degree 16, a fresh tile per tick
    n = 200_000
    topo = gossip.Topology.gnp(n, 16.0 / (n - 1), 93, gossip.TOPO_SKIP, threads=16)
    lat = gossip.milliseconds_to_ns(5.0)
    t_cut = gossip.seconds_to_ns(5.4)
    ev = gossip.make_schedule(n, 94, T0, t_cut)
    runs = {}
    for po, pb in COMBOS:
        st, c, _ = _engine(gossip, n, lat, t_cut, ev, dict(peer_order=po, pull_batch=pb, young=0),
                           gossip.F_TILE_PER_TICK, topo=topo)
        runs[po, pb] = (st, c.pull_pair_edges)
    base = runs[0, 0][1]
    for k in COMBOS:
        print(f"peer_order={k[0]} pull_batch={k[1]}: pull_pair_edges {runs[k][1]} "
              f"ratio to (0, 0) {runs[k][1] / base:.4f}")
    for k in STATS:
        assert np.array_equal(getattr(runs[0, 0][0], k), getattr(runs[1, 1][0], k)), k
    assert runs[1, 1][1] < base


# ---- 5. option handling ---------------------------------------------------------------------------
def test_peer_order_only_before_the_graph(gossip):
    topo = gossip.Topology.gnp(100, 0.1, 5, gossip.TOPO_EXACT)
    eng = gossip.Engine(100, L, T0, T0 + 10 * L)
    try:
        assert eng.get_option("peer_order") == 1 and eng.get_option("pull_batch") in (0, 1)
        eng.set_option("peer_order", 0)
        assert eng.get_option("peer_order") == 0
        eng.set_option("peer_order", 1)
        for bad in (-1, 2):
            with pytest.raises(gossip.GossipError) as ei:
                eng.set_option("peer_order", bad)
            assert ei.value.code == gossip.E_INVAL
        eng.set_topology(topo)
        with pytest.raises(gossip.GossipError) as ei:
            eng.set_option("peer_order", 0)
        assert ei.value.code == gossip.E_STATE
        assert eng.get_option("peer_order") == 1
        eng.set_option("pull_batch", 1)  # a launch option: any time
        assert eng.get_option("pull_batch") == 1
    finally:
        eng.close()


# ---- 6. the caller's order is irrelevant ------------------------------------------------------------
def test_callers_row_order_is_irrelevant(gossip, late_case):
    topo, lat, t_cut, ev, r = late_case
    rp, col, mult = topo.csr()
    asc_c, asc_m, shuf_c, shuf_m = col.copy(), mult.copy(), col.copy(), mult.copy()
    rng = np.random.default_rng(7)
    for v in range(topo.num_nodes):
        lo, hi = int(rp[v]), int(rp[v + 1])
        o = np.argsort(col[lo:hi], kind="stable")
        asc_c[lo:hi], asc_m[lo:hi] = col[lo:hi][o], mult[lo:hi][o]
        p = rng.permutation(hi - lo)
        shuf_c[lo:hi], shuf_m[lo:hi] = col[lo:hi][p], mult[lo:hi][p]
    assert not np.array_equal(asc_c, shuf_c)
    fl = gossip.F_TILE_PER_TICK
    opts = dict(young=0, pull_batch=1)
    asc = _engine(gossip, topo.num_nodes, lat, t_cut, ev, opts, fl, graph=(rp, asc_c, asc_m))
    shuf = _engine(gossip, topo.num_nodes, lat, t_cut, ev, opts, fl, graph=(rp, shuf_c, shuf_m))
    for k in STATS:
        assert np.array_equal(getattr(asc[0], k), getattr(shuf[0], k)), k
        assert np.array_equal(getattr(asc[0], k), getattr(r, k)), k
    # ordered rows: the same peer rows are read whatever order the caller gave
    assert asc[1].pull_pair_edges == shuf[1].pull_pair_edges
    # the caller's order kept: still the same results
    keep = _engine(gossip, topo.num_nodes, lat, t_cut, ev, dict(opts, peer_order=0), fl, graph=(rp, shuf_c, shuf_m))
    for k in STATS:
        assert np.array_equal(getattr(keep[0], k), getattr(asc[0], k)), k
