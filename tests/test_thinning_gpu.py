"""The per-tick thinned peer lists on the device (k_fanout_kth, the four k_fanout_count* kernels, the scan and
k_fanout_compact, csrc/fanout_kernel.h) against the model (thinning_ref.py), entry by entry: after every one of
the first 8 ticks the engine's (rowptr_t, col_t) and, in exact mode, its bound table are read back
(Engine.thinned_lists) and must EQUAL the model's -- every row pointer, every row's sorted peers, every bound of a
node with k[u] > 0 -- and so must the tick's share of the kernels' own totals (selected_in, selected_out,
lost_copies, down_copies, down_node_ticks).  No share enters the lists, so idle senders and receivers that have
seen everything are checked like the others.  Engines run with flags = 0 (no F_REACH, no F_TRACE): the
configuration of the benchmarks.  The inputs are shown not to be vacuous by test_thinning_cpu.py, which also
holds the case table.
"""
import numpy as np
import pytest

import fanout_exact_ref as X
import fanout_ref as F
import faults_ref as R
import rounds_ref as M
import thinning_ref as TH
from cases import L, T0
from test_thinning_cpu import FIRST, GRAPHS, TICKS, config, events_of, grids_of, modes_of, thinning, topology

pytestmark = pytest.mark.gpu

T_CUT = T0 + TICKS * L + L // 3  # inside the tick after the compared ones: the run ends one tick later


def _engine(gossip, topo, ev, c, grid):
    eng = gossip.Engine(topo.num_nodes, L, T0, T_CUT, flags=0)
    try:
        eng.set_option("fanout_grid", grid)
        eng.set_topology(topo)
        if c["fanout"] is not None:
            eng.set_fanout(c["fanout"], c["seed"])
        elif c["thr"] is not None:
            eng.set_forward_thresholds(c["thr"], c["seed"])
        elif c["k"] is not None:
            eng.set_fanout_counts(c["k"], c["seed"])
        if len(c["outages"]):
            o = np.array(c["outages"], np.int64).reshape(-1, 3)
            eng.set_outages(o[:, 0], o[:, 1], o[:, 2])
        if c["loss_thr"]:
            eng.set_link_loss(int(c["loss_thr"]), c["loss_seed"])
        if c["rounds"] > 1:
            eng.set_rounds(c["rounds"])
        eng.set_schedule(ev)
    except BaseException:
        eng.close()
        raise
    return eng


_MODEL = {}


def _model(gossip, graph, mode):
    """The existing model's run of the whole flood: per-node sent and recv at the end."""
    if (graph, mode) not in _MODEL:
        topo = topology(gossip, graph)
        n = topo.num_nodes
        a, b = topo.links()
        c, ev = config(mode, n, topo.degrees()[0]), events_of(n)
        fa = dict(outages=c["outages"], loss_thr=c["loss_thr"], loss_seed=c["loss_seed"])
        if c["rounds"] > 1:
            m = M.run(n, a, b, ev, L, T_CUT, c["rounds"], k=c["k"], seed=c["seed"], **fa)
        elif c["k"] is not None:
            m = X.run(n, a, b, ev, L, T_CUT, c["k"], c["seed"], **fa)
        elif c["outages"] or c["loss_thr"]:
            m = R.run(n, a, b, ev, L, T_CUT, np.full(n, 0xFFFFFFFF, np.uint32) if c["thr"] is None else c["thr"], c["seed"], **fa)
        else:
            m = F.run(n, a, b, ev, L, T_CUT, c["thr"], c["seed"])
        _MODEL[graph, mode] = m
    return _MODEL[graph, mode]


def _totals(eng):
    f, x = eng.fanout_counters(), eng.fault_counters()
    return dict(selected_in=f.selected_in, selected_out=f.selected_out, lost_copies=x.lost_copies, down_copies=x.down_copies,
                down_node_ticks=x.down_node_ticks)


def _first_difference(got, want):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    return [(int(i), int(got[i]), int(want[i])) for i in bad[:6]]


CASES = [(g, m, grid) for g in GRAPHS for m in modes_of(g) for grid in grids_of(g)]


@pytest.mark.parametrize("graph,mode,grid", CASES, ids=[f"{g}-{m}-grid{x}" for g, m, x in CASES])
def test_lists_entry_by_entry(gossip, graph, mode, grid):
    topo = topology(gossip, graph)
    n = topo.num_nodes
    c, ev, th = config(mode, n, topo.degrees()[0]), events_of(n), thinning(gossip, graph, mode)
    exact = c["k"] is not None
    eng = _engine(gossip, topo, ev, c, grid)
    try:
        assert eng.first_tick == FIRST and eng.end_tick == FIRST + TICKS + 1
        before = _totals(eng)
        for t in range(FIRST, FIRST + TICKS):
            what = (graph, mode, grid, t - FIRST)
            eng.run(t + 1)
            got = eng.thinned_lists(bound=exact)
            want = th.tick(t)
            assert got[0] == t, what
            row_ptr, col = got[1], got[2]
            assert row_ptr.shape == (n + 1,) and np.array_equal(row_ptr, want["row_ptr"]), \
                (what, "row_ptr (node, engine, model)", _first_difference(row_ptr, want["row_ptr"]))
            assert col.shape == want["col"].shape
            rows = TH.rows_of(row_ptr, col)
            assert np.array_equal(rows, want["col"]), (what, "col (flat position, engine, model)", _first_difference(rows, want["col"]))
            if exact:
                m = want["bound_mask"]
                assert np.array_equal(got[3][m], want["bound"][m]), \
                    (what, "bound (index among the nodes with k > 0, engine, model)", _first_difference(got[3][m], want["bound"][m]))
            now = _totals(eng)
            delta = {k: now[k] - before[k] for k in now}
            assert delta == {k: want[k] for k in now}, (what, delta)
            before = now
        eng.run()
        eng.sync()
        st = eng.stats()
        fl, fc = eng.fanout_counters(), eng.fault_counters()
        strided = {r.arg: r.strided for r in eng.launches() if r.kernel == gossip.K_FANOUT}
    finally:
        eng.close()
    want = _model(gossip, graph, mode)
    assert np.array_equal(st.sent, want["sent"]), (graph, mode, grid, "sent", _first_difference(st.sent, want["sent"]))
    assert np.array_equal(st.recv, want["recv"]), (graph, mode, grid, "recv", _first_difference(st.recv, want["recv"]))
    assert fl.launches == TICKS + 1 and fc.dropped_generations == want.get("dropped", 0)
    if grid == 1 and n > 256:  # one block of four waves strides the chunks of 64 nodes
        assert strided and all(s == TICKS + 1 for s in strided.values()), strided
    if mode == "c_all_lost":
        assert not st.recv.any()


def test_rounds_do_not_enter_the_selection(gossip):
    # mode h is g with set_rounds(3): compared with g's model tick for tick above; here the two engines directly
    for graph in ("ladder", "gaps"):
        topo = topology(gossip, graph)
        n = topo.num_nodes
        got = {}
        for mode in ("g", "h"):
            eng = _engine(gossip, topo, events_of(n), config(mode, n, topo.degrees()[0]), 0)
            try:
                got[mode] = []
                for t in range(FIRST, FIRST + TICKS):
                    eng.run(t + 1)
                    got[mode].append(eng.thinned_lists(bound=True))
            finally:
                eng.close()
        for x, y in zip(got["g"], got["h"]):
            assert x[0] == y[0] and all(np.array_equal(p, q) for p, q in zip(x[1:], y[1:])), (graph, x[0])


def test_refusals_and_the_short_buffer(gossip):
    import ctypes as C
    topo = topology(gossip, "tail[65]")
    n = topo.num_nodes
    ev = events_of(n)
    lib = gossip.load_library()

    def refused(code, match, fn):
        with pytest.raises(gossip.GossipError, match=match) as e:
            fn()
        assert e.value.code == code

    plain = gossip.Engine(n, L, T0, T_CUT)
    try:  # no thinning mode: before and after ticks
        plain.set_topology(topo)
        refused(gossip.E_STATE, "thins no peer lists", plain.thinned_lists)
        plain.set_schedule(ev)
        plain.run(FIRST + 2)
        refused(gossip.E_STATE, "thins no peer lists", plain.thinned_lists)
    finally:
        plain.close()
    eng = gossip.Engine(n, L, T0, T_CUT)
    try:
        eng.set_topology(topo)
        eng.set_fanout(1, 3)
        refused(gossip.E_STATE, "no tick has finished", eng.thinned_lists)
        eng.set_schedule(ev)
        refused(gossip.E_STATE, "no tick has finished", eng.thinned_lists)  # before the first tick
        eng.run(FIRST + 3)
        refused(gossip.E_INVAL, "exact-k mode only", lambda: eng.thinned_lists(bound=True))
        eng.sync()
        ledger = [(r.key, r.launches, r.strided) for r in eng.launches()]
        c0, f0 = eng.counters(), eng.fanout_counters()
        tick, row_ptr, col = eng.thinned_lists()
        assert tick == FIRST + 2 and 0 < row_ptr[n] == col.size
        # a short col_cap: GOSSIP_EINVAL, and num_entries is written all the same
        t, total = C.c_int64(-1), C.c_uint64(0)
        short = np.full(col.size, -7, np.int32)
        rc = lib.gossip_engine_get_thinned_lists(eng._h, C.byref(t), None, C.c_void_p(short.ctypes.data), col.size - 1, C.byref(total), None)
        assert rc == gossip.E_INVAL and total.value == col.size and t.value == tick and np.all(short == -7)
        assert str(col.size - 1) in lib.gossip_last_error().decode()
        # the query form: no buffers at all
        total.value = 0
        assert lib.gossip_engine_get_thinned_lists(eng._h, C.byref(t), None, None, 0, C.byref(total), None) == 0 and total.value == col.size
        # the call launched nothing, allocated nothing, counted nothing
        c1, f1 = eng.counters(), eng.fanout_counters()
        assert [(r.key, r.launches, r.strided) for r in eng.launches()] == ledger
        assert c1.device_bytes == c0.device_bytes and c1.ticks == c0.ticks == 3 and c1.edge_events == c0.edge_events
        assert (f1.launches, f1.selected_in, f1.selected_out, f1.entries, f1.bytes) == (f0.launches, f0.selected_in, f0.selected_out, f0.entries, f0.bytes)
        # and a second read gives the same lists
        again = eng.thinned_lists()
        assert again[0] == tick and np.array_equal(again[1], row_ptr) and np.array_equal(again[2], col)
    finally:
        eng.close()
