"""C3 at its stated configuration -- sparse G(n,p), 1,000,000 nodes, average degree 16, 60 s of
simulated time on one MI355X -- and the bench's warm-start slice pinned to the continuous run.

* slice == continuous: the bench times ticks [2005, 2025) of a schedule that replays only the
  generations of the LIFE_TICKS ticks before t = 10 s (plus every earlier generation of the ids
  that recur there; gossip/workloads.py).  That is exact only if every flood older than
  LIFE_TICKS has died out by then.  Here the continuous run (every generation from t = 5 s) and
  the slice replay must give bit-identical per-node counter DELTAS over the timed ticks.
* the full 60 s run (~15.6M shares, 10,980 ticks) against the reference's counter invariants
  (p2pnode.cc:115-120,155-165; forwarded == received, sent == |peers| x (gen + recv)).
* colliding share ids at full size: GenerateUniqueShareId (p2pnode.cc:201-209) repeats ids above
  128,849 nodes; the C3 schedule's own colliding pairs closest in time (floods of one id that
  meet mid-way, p2pnode.cc:189) and one pair whose later generation finds its id already
  processed (counted and sent, not processed: p2pnode.cc:115-120), replayed on the 1M-node graph
  against ORACLE A bit for bit.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATS = ("gen", "recv", "fwd", "sent", "processed", "peers", "sockets")
DELTA = ("gen", "recv", "fwd", "sent", "processed")


def _w():
    import gossip.workloads as W
    return W


@pytest.fixture(scope="module")
def c3(gossip):
    W = _w()
    topo = W.topology("C3")
    ev = gossip.make_schedule(topo.num_nodes, W.CONFIGS["C3"]["node_seed"], W.T0_NS, W.T_CUT_NS, threads=16)
    return topo, ev


def _stats_at(gossip, topo, ev, ticks, t_start_ns=None, **kw):
    """Per-node stats after each tick boundary in `ticks` (one engine run, stepped)."""
    W = _w()
    eng = gossip.Engine(topo.num_nodes, W.L_NS, W.T0_NS if t_start_ns is None else t_start_ns, W.T_CUT_NS, **kw)
    eng.set_topology(topo)
    eng.set_schedule(ev)
    out = []
    for t in ticks:
        eng.run(t)
        eng.sync()
        out.append((eng.stats(), eng.counters().edge_events))
    eng.close()
    return out


def test_c3_slice_equals_continuous_run(gossip, c3):
    W = _w()
    topo, ev = c3
    n = topo.num_nodes
    warm, steps = 5, 20  # the bench's default window shape: ticks [2005, 2025)
    t0 = W.SLICE_NS // W.L_NS + warm
    t1 = t0 + steps
    cont = ev[ev["ns"] < t1 * W.L_NS]
    sl, info = W.slice_schedule(n, W.CONFIGS["C3"]["node_seed"], W.SLICE_NS, t1 * W.L_NS)
    assert info["earlier_same_id"] > 0 and len(sl) < len(cont) // 2
    (a0, e0), (a1, e1) = _stats_at(gossip, topo, cont, [t0, t1])
    (b0, f0), (b1, f1) = _stats_at(gossip, topo, sl, [t0, t1])
    for k in DELTA:
        da = getattr(a1, k).astype(np.int64) - getattr(a0, k).astype(np.int64)
        db = getattr(b1, k).astype(np.int64) - getattr(b0, k).astype(np.int64)
        assert np.array_equal(da, db), (k, int(np.count_nonzero(da != db)))
    assert e1 - e0 == f1 - f0 > 0
    # the slice's ticks before the window are NOT the continuous run's (fewer floods in flight)
    assert int(b0.recv.sum()) < int(a0.recv.sum())
    # the bench's compressed ramp (workloads.compress_ramp: the earlier generations of recurring
    # ids moved next to the slice, the engine started there): every counter of the slice replay,
    # at both ends of the timed window, not only the deltas
    cs, t_start = W.compress_ramp(sl, info["t_lo_ns"])
    assert t_start > W.T0_NS + 900 * W.L_NS and not np.array_equal(cs["ns"], sl["ns"])
    (c0, g0), (c1, g1) = _stats_at(gossip, topo, cs, [t0, t1], t_start_ns=t_start)
    assert (g0, g1) == (f0, f1)
    for k in STATS:
        assert np.array_equal(getattr(c0, k), getattr(b0, k)), k
        assert np.array_equal(getattr(c1, k), getattr(b1, k)), k


def test_c3_full_60s_invariants(gossip, c3):
    W = _w()
    topo, ev = c3
    n = topo.num_nodes
    (st, edges), = _stats_at(gossip, topo, ev, [W.T_CUT_NS // W.L_NS + 1])
    assert np.array_equal(st.fwd, st.recv)  # p2pnode.cc:157,163
    assert np.array_equal(st.sent, st.peers.astype(np.uint64) * (st.gen + st.recv).astype(np.uint64))
    assert np.array_equal(st.gen, np.bincount(ev["node"], minlength=n).astype(np.uint32))
    assert edges == int(st.sent.sum())
    # colliding ids (21k shares at C3): a later generation of an id the node has seen counts as
    # generated but not as processed (p2pnode.cc:115-120)
    lost = st.gen.astype(np.int64) + st.recv - st.processed
    assert np.all(lost >= 0) and int(lost.sum()) > 0
    # ~every share floods its component: receptions per share close to n
    assert int(st.recv.sum()) > 0.9 * len(ev) * n
    assert len(ev) > 15_000_000


def test_c3_colliding_ids_vs_oracle_a(gossip, oracle, c3):
    W = _w()
    topo, ev = c3
    n = topo.num_nodes
    L = W.L_NS
    ids, first, cnt = np.unique(ev["share_id"], return_index=True, return_counts=True)
    dup = ids[cnt == 2]
    assert len(dup) > 5000  # 21,357 colliding shares at 1M nodes
    pos = np.flatnonzero(np.isin(ev["share_id"], dup))
    pe = ev[pos]
    order = np.lexsort((pe["ns"], pe["share_id"]))
    pe = pe[order].reshape(-1, 2)  # (earlier, later) generation of each colliding id
    # The 4 pairs closest in time (0.8 ms to 25 ms apart for this schedule: the two floods of
    # one id are both under way and meet), and one pair 12-40 ticks apart (the later generation
    # finds its id already processed everywhere); whole floods, 8 hops past the last generation.
    gap = pe[:, 1]["ns"] - pe[:, 0]["ns"]
    close = np.argsort(gap, kind="stable")[:4]
    late = np.flatnonzero((gap > 12 * L) & (gap < 40 * L))[:1]
    assert gap[close].max() < 8 * L and len(late) == 1
    pick = pe[np.concatenate([close, late])].reshape(-1)
    pick = pick[np.lexsort((pick["node"], pick["ns"]))]
    t_cut = int(pick["ns"].max()) + 8 * L + L // 3
    from concurrent.futures import ThreadPoolExecutor

    a, b = topo.links()
    with ThreadPoolExecutor(1) as pool:  # ORACLE A on the CPU beside the GPU run
        fut = pool.submit(oracle.run_replay, n, L, W.T0_NS, t_cut, a, b, pick["ns"], pick["node"],
                          pick["share_id"])
        eng = gossip.Engine(n, L, W.T0_NS, t_cut)
        eng.set_topology(topo)
        eng.set_schedule(pick)
        eng.run()
        eng.sync()
        st = eng.stats()
        eng.close()
        ref = fut.result()
    del a, b
    for k in STATS:
        x, y = getattr(st, k), getattr(ref, k)
        assert np.array_equal(x, y), (k, int(np.count_nonzero(x != y)))
    # generations of ids their node had already received: generated and sent, not processed
    assert int((ref.gen + ref.recv - ref.processed).sum()) >= 1
    assert ref.edge_events > 50_000_000
