"""Multi-round push on the device (k_rounds, csrc/rounds_kernel.h) against the model (rounds_ref.py): engine and
model agree EXACTLY on per-node gen, recv, fwd, sent and processed and on edge_events, and with
F_TRACE | F_REACH on the (node, share, hop, via) set, the ticks and the reach table; the re-sent bits the
kernel counts are the model's.  The model is pinned to the fault and exact-k models at r = 1, to the closed
form of a flood and to hand cases by test_rounds_cpu.py.
"""
import functools
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
import thinning_ref as TH
from cases import L, T0

pytestmark = pytest.mark.gpu

ALWAYS = 0xFFFFFFFF
FIRST = T0 // L
FOREVER = np.iinfo(np.int64).max
FAR = T0 + 60 * L
STAT_KEYS = ("gen", "recv", "fwd", "sent", "processed")


@functools.lru_cache(maxsize=None)
def _base(gossip):  # the base inputs of test_fanout_gpu.py
    topo = gossip.Topology.gnp(1000, 8.0 / 999.0, 7, gossip.TOPO_SKIP)
    return topo, S.events(1000, 6, 8, 8)


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
    return gossip.Topology.from_links(n, a, b), ev, T0 + 200 * L


def _silent_counts():
    kk = np.full(1000, 2, np.uint32)
    kk[np.random.default_rng(5).choice(1000, 150, replace=False)] = 0  # silent nodes
    kk[::11] = 5
    return kk


_MODEL = {}


def _model(topo, ev, t_cut, r, thr=None, k=None, seed=1, outages=(), loss_thr=0, loss_seed=1):
    key = (id(topo), ev.tobytes(), t_cut, r, None if thr is None else np.asarray(thr).tobytes(),
           None if k is None else np.asarray(k).tobytes(), seed, tuple(outages), loss_thr, loss_seed)
    if key not in _MODEL:
        a, b = topo.links()
        m = M.run(topo.num_nodes, a, b, ev, L, t_cut, r, thr=thr, k=k, seed=seed, outages=outages, loss_thr=loss_thr,
                  loss_seed=loss_seed)
        assert np.array_equal(m["peers"], topo.degrees()[0])
        _MODEL[key] = m
    return _MODEL[key]


def _engine(gossip, topo, ev, t_cut, r, mode=None, seed=1, outages=(), loss_thr=0, loss_seed=1, flags=0, opts=(), snaps=(),
            trace=True, rounds_first=False, **kw):
    """mode: None (a flood), ("binomial", k), ("exact", k) or ("counts", k per node).  r None: set_rounds is not called."""
    fl = gossip.F_REACH | (gossip.F_TRACE if trace else 0) | flags
    eng = gossip.Engine(topo.num_nodes, L, T0, t_cut, flags=fl, **kw)
    try:
        for name, v in dict(opts).items():
            eng.set_option(name, v)
        eng.set_topology(topo)
        if r is not None and rounds_first:
            eng.set_rounds(r)
        if mode is not None:
            {"binomial": eng.set_fanout, "exact": eng.set_fanout_exact, "counts": eng.set_fanout_counts}[mode[0]](mode[1], seed)
        if len(outages):
            o = np.array(outages, np.int64).reshape(-1, 3)
            eng.set_outages(o[:, 0], o[:, 1], o[:, 2])
        if loss_thr:
            eng.set_link_loss(int(loss_thr), loss_seed)
        if r is not None and not rounds_first:
            eng.set_rounds(r)
        for t in snaps:
            eng.add_snapshot(t)
        eng.set_schedule(ev)
    except BaseException:
        eng.close()
        raise
    return eng


def _result(eng, trace=True):
    eng.sync()
    st, c = eng.stats(), eng.counters()
    out = dict(gen=st.gen, recv=st.recv, fwd=st.fwd, sent=st.sent, processed=st.processed, peers=st.peers,
               edge_events=int(c.edge_events), reach=eng.reach(), counters=c, launches=eng.launches(),
               fanout=eng.fanout_counters(), faults=eng.fault_counters(), rounds=eng.rounds_counters(),
               ticks=(eng.first_tick, eng.end_tick))
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


def _rounds_records(res, gossip):
    return [x for x in res["launches"] if x.kernel == gossip.K_ROUNDS]


def _model_kw(topo, mode):
    if mode is None:
        return {}
    if mode[0] == "binomial":
        return dict(thr=F.thresholds(mode[1], topo.degrees()[0]))
    return dict(k=mode[1])


def _run(gossip, topo, ev, t_cut, r, what, mode=None, seed=1, outages=(), loss_thr=0, loss_seed=1, trace=True, **kw):
    """One engine run compared with the model, the kernel's own counters included; returns (engine result, model)."""
    eng = _engine(gossip, topo, ev, t_cut, r, mode=mode, seed=seed, outages=outages, loss_thr=loss_thr, loss_seed=loss_seed,
                  trace=trace, **kw)
    try:
        eng.run()
        got = _result(eng, trace)
    finally:
        eng.close()
    want = _model(topo, ev, t_cut, r, seed=seed, outages=tuple(outages), loss_thr=loss_thr, loss_seed=loss_seed,
                  **_model_kw(topo, mode))
    _same(got, want, what, trace)
    rc, rec = got["rounds"], _rounds_records(got, gossip)
    assert rc.resent_bits == want["resent"], (what, rc.resent_bits, want["resent"])
    assert len(rec) == 1 and rec[0].arg == M.planes(r) and rec[0].launches == rc.launches > 0, what
    assert rc.rows_visited > 0 and rc.bytes >= 16 * rc.rows_visited, what
    assert got["faults"].dropped_generations == want["dropped"], what
    # the totals of the thinning passes: the model of the thinned lists (rounds do not enter the selection)
    first, fo, fa = got["ticks"][0], got["fanout"], got["faults"]
    tot = TH.of_topology(topo, seed=seed, outages=tuple(outages), loss_thr=loss_thr, loss_seed=loss_seed,
                         **_model_kw(topo, mode)).totals(range(first, first + int(got["counters"].ticks)))
    assert fo.launches == got["counters"].ticks, what
    assert (fo.selected_in, fo.selected_out) == (tot["selected_in"], tot["selected_out"]), (what, tot)
    assert (fa.lost_copies, fa.down_copies, fa.down_node_ticks) == (tot["lost_copies"], tot["down_copies"], tot["down_node_ticks"]), what
    return got, want


# ---- the modes, r from one plane to four ---------------------------------------------------------------
MODES = {"binomial3": ("binomial", 3), "exact2": ("exact", 2), "counts_silent": ("counts", None), "flood_loss": None}


@pytest.mark.parametrize("r", [2, 3, 5, 16])
@pytest.mark.parametrize("name", list(MODES))
def test_modes(gossip, name, r):
    topo, ev = _base(gossip)
    mode = ("counts", _silent_counts()) if name == "counts_silent" else MODES[name]
    loss = gossip.loss_threshold(0.3) if name == "flood_loss" else 0
    got, want = _run(gossip, topo, ev, FAR, r, (name, r), mode=mode, loss_thr=loss, loss_seed=3)
    one = _model(topo, ev, FAR, 1, loss_thr=loss, loss_seed=3, **_model_kw(topo, mode))
    assert want["resent"] > 0 and int(want["sent"].sum()) > int(one["sent"].sum())
    if name == "counts_silent":
        silent = mode[1] == 0
        assert not got["sent"][silent].any() and got["recv"][silent].any()


# ---- outages and loss together ----------------------------------------------------------------------------
def _sender_down_in_a_later_round(want, outages, n, r):
    node, _, tick, _, _ = want["trace"]
    for x in range(1, r):
        for t in np.unique(tick):
            dn = R.down_mask(n, outages, int(t) + x)
            if dn[node[tick == t]].any():
                return True
    return False


def _exact_fault_counts(topo, k, seed, outages, loss_thr, loss_seed, ticks):
    """faults_ref.fault_counts with the exact row rule in place of the binomial selection."""
    n = topo.num_nodes
    a, b = topo.links()
    u, v, c, _ = F.copies(n, a, b)
    rp = np.concatenate([[0], np.cumsum(np.bincount(u, minlength=n))])
    kk = np.broadcast_to(np.asarray(k, np.int64), (n,))
    dnt = lc = dc = 0
    for t in ticks:
        made, dn = X.made(seed, u, v, c, rp, kk, t), R.down_mask(n, outages, t + 1)
        lost = R.lost(loss_seed, u, v, c, t, loss_thr)
        dnt += int(dn.sum())
        dc += int((made & dn[v]).sum())
        lc += int((made & ~dn[v] & lost).sum())
    return dnt, lc, dc


@pytest.mark.parametrize("kind", ["exact", "binomial"])
def test_outages_and_loss_on_the_ladder(gossip, kind):
    topo, ev, t_cut = _ladder(gossip)
    n = topo.num_nodes
    peers, sockets = topo.degrees()
    assert (peers > sockets).any()  # parallel links: two copies, two draws
    outages = tuple((v, FIRST + 2 + v % 5, FIRST + 3 + v % 5 + v % 4) for v in range(0, n, 3))
    loss = gossip.loss_threshold(0.2)
    mode = (kind, 2 if kind == "exact" else 3)
    got, want = _run(gossip, topo, ev, t_cut, 3, ("ladder", kind), mode=mode, seed=4, outages=outages, loss_thr=loss, loss_seed=9,
                     opts=dict(fanout_grid=1, rounds_grid=1))
    assert _sender_down_in_a_later_round(want, outages, n, 3)
    f, (first, end) = got["faults"], got["ticks"]
    assert f.down_copies > 0  # a receiver down at a delivery
    clean = _model(topo, ev, t_cut, 3, seed=4, loss_thr=loss, loss_seed=9, **_model_kw(topo, mode))
    assert not np.array_equal(clean["recv"], want["recv"])
    if kind == "exact":
        counts = _exact_fault_counts(topo, 2, 4, outages, loss, 9, range(first, end))
        assert counts[0] == R.fault_counts(n, *topo.links(), np.full(n, ALWAYS, np.uint32), 4, outages, loss, 9, range(first, end))[0]
    else:
        counts = R.fault_counts(n, *topo.links(), F.thresholds(3, peers), 4, outages, loss, 9, range(first, end))
    assert (f.down_node_ticks, f.lost_copies, f.down_copies) == counts


# ---- r = 1 is the engine without the call -------------------------------------------------------------------
def _ledger(res):
    return sorted((x.kernel, x.lpw, x.epn, x.flags, x.arg, x.launches, x.strided) for x in res["launches"])


def test_one_round_is_off(gossip):
    topo, ev = _base(gossip)
    t_cut = S.t_cut_for(6)

    def go(setup):
        eng = gossip.Engine(topo.num_nodes, L, T0, t_cut, flags=gossip.F_REACH | gossip.F_TRACE)
        try:
            eng.set_topology(topo)
            setup(eng)
            eng.set_schedule(ev)
            eng.run()
            return _result(eng)
        finally:
            eng.close()

    def thin(eng):
        eng.set_link_loss(0)

    def on_off(eng):
        eng.set_link_loss(0)
        eng.set_rounds(3)
        eng.set_rounds(1)

    pairs = ((go(lambda e: None), go(lambda e: e.set_rounds(1))),  # never on: a no-op, thinning stays off
             (go(thin), go(on_off)))                              # switched on and off again: thinning as it was
    for plain, off in pairs:
        for k in STAT_KEYS + ("peers", "reach"):
            assert np.array_equal(plain[k], off[k]), k
        assert plain["edge_events"] == off["edge_events"]
        for x, y in zip(S.sorted_trace(plain["trace"]), S.sorted_trace(off["trace"])):
            assert np.array_equal(x, y)
        assert _ledger(plain) == _ledger(off) and not _rounds_records(off, gossip)
        assert plain["counters"].device_bytes == off["counters"].device_bytes
        rc = off["rounds"]
        assert (rc.launches, rc.resent_bits, rc.rows_visited, rc.bytes, rc.ms) == (0, 0, 0, 0, 0.0)
    assert not [x for x in pairs[0][1]["launches"] if x.kernel == gossip.K_FANOUT]
    assert [x for x in pairs[1][1]["launches"] if x.kernel == gossip.K_FANOUT]


# ---- option invariance at r = 3 ---------------------------------------------------------------------------------
INVARIANTS = [("pull_sat", dict(pull_sat=0), 0), ("pull_gate", dict(pull_gate=0), 0), ("pull_nt", dict(pull_nt=1), 0),
              ("pull_tile_order", dict(pull_tile_order=0), 0), ("late_age", dict(late_age=0), 0),
              ("peer_order", dict(peer_order=0), 0), ("grids", dict(fanout_grid=1, rounds_grid=1), 0),
              ("tile_per_tick", {}, "F_TILE_PER_TICK"), ("rounds_first", {}, 0),
              # without tile lists k_pull writes whole occupancy words itself (no zeroing before the pull)
              ("pull_tiles", dict(pull_tiles=0), 0), ("noskip", {}, "F_NOSKIP")]


@pytest.mark.parametrize("name,opts,flags", INVARIANTS, ids=[i[0] for i in INVARIANTS])
def test_option_invariance(gossip, name, opts, flags):
    topo, ev = _base(gossip)
    flags = getattr(gossip, flags) if flags else 0
    outages = tuple((v, FIRST + 3, FIRST + 6) for v in range(0, 1000, 7))
    kw = dict(mode=("exact", 2), outages=outages, loss_thr=gossip.loss_threshold(0.2), loss_seed=9)
    ref, _ = _run(gossip, topo, ev, S.t_cut_for(6), 3, "default", **kw)
    got, _ = _run(gossip, topo, ev, S.t_cut_for(6), 3, ("option", name), opts=opts, flags=flags,
                  rounds_first=name == "rounds_first", **kw)
    for k in STAT_KEYS + ("reach",):
        assert np.array_equal(got[k], ref[k]), k
    assert got["rounds"].resent_bits == ref["rounds"].resent_bits
    if name == "grids":  # one block of k_rounds loops over the 63 groups of 16 rows
        assert _rounds_records(got, gossip)[0].strided == got["rounds"].launches
        assert _rounds_records(ref, gossip)[0].strided == 0
        assert all(x.strided > 0 for x in got["launches"] if x.kernel == gossip.K_FANOUT)


def test_many_sparse_tiles_several_occupancy_words(gossip):
    # a birth tick = a tile (F_TILE_PER_TICK) on a ring whose floods last longer than 64 ticks: more than 64
    # tiles live at once, so the rows' gate words span several occupancy words
    n, a, b = S.ring_chords(513, 0)
    topo, ev, t_cut = gossip.Topology.from_links(n, a, b), S.events(n, 100, 1, 14), T0 + 420 * L
    got, want = _run(gossip, topo, ev, t_cut, 3, "ring513", loss_thr=gossip.loss_threshold(0.2), loss_seed=2, trace=False,
                     flags=gossip.F_TILE_PER_TICK)
    print(f"  window high water {got['counters'].words_hw} words, longest flood {int(want['trace'][3].max())} hops")
    assert got["counters"].words_hw > 1024 and int(want["trace"][3].max()) > 150


@pytest.mark.parametrize("count,by_tick", [(2, 0), (2, 1)])
def test_share_shards_add_up(gossip, count, by_tick):
    topo, ev = _base(gossip)
    fl = gossip.F_SHARD_BY_TICK if by_tick else 0
    kw = dict(mode=("exact", 2), loss_thr=gossip.loss_threshold(0.2), loss_seed=9)
    want = _model(topo, ev, FAR, 3, k=2, loss_thr=kw["loss_thr"], loss_seed=9)
    parts = []
    for rank in range(count):
        eng = _engine(gossip, topo, ev, FAR, 3, flags=fl, trace=False, shard_rank=rank, shard_count=count, **kw)
        try:
            eng.run()
            parts.append(_result(eng, trace=False))
        finally:
            eng.close()
    assert sum(int(p["gen"].sum()) > 0 for p in parts) >= 2  # the shares really are split
    tot = {k: sum(p[k].astype(np.uint64) for p in parts) for k in STAT_KEYS + ("reach",)}
    tot["edge_events"] = sum(p["edge_events"] for p in parts)
    _same(tot, want, ("shards", count, by_tick), trace=False)
    assert sum(p["rounds"].resent_bits for p in parts) == want["resent"]


# ---- the cut: rounds cut mid-way, snapshots ------------------------------------------------------------------------
def test_cut_and_snapshots(gossip):
    topo, ev = _base(gossip)
    t_cut = S.t_cut_for(6)
    snaps = (T0 + 3 * L + L // 2, T0 + 5 * L + 7)
    kw = dict(mode=("binomial", 3), loss_thr=gossip.loss_threshold(0.2), loss_seed=9)
    eng = _engine(gossip, topo, ev, t_cut, 4, snaps=snaps, **kw)
    try:
        eng.run()
        got = _result(eng)
        snap = [eng.snapshot(i) for i in range(2)]
    finally:
        eng.close()
    want = _model(topo, ev, t_cut, 4, thr=F.thresholds(3, topo.degrees()[0]), loss_thr=kw["loss_thr"], loss_seed=9)
    _same(got, want, "cut")
    assert got["rounds"].resent_bits == want["resent"]
    far = _model(topo, ev, FAR, 4, thr=F.thresholds(3, topo.degrees()[0]), loss_thr=kw["loss_thr"], loss_seed=9)
    assert int(want["sent"].sum()) < int(far["sent"].sum()) and want["resent"] < far["resent"]  # rounds were cut
    for i, ts in enumerate(snaps):
        assert snap[i][0] == ts and snap[i][2] == M.snapshot_total(want, ev, ts), i
        assert snap[i][1] == int(np.sum((ev["ns"] < ts) & want["counted"])), i


# ---- window reuse and growth ------------------------------------------------------------------------------------------
def test_words_retire_and_are_reused(gossip):
    topo = gossip.Topology.gnp(200, 6.0 / 199.0, 3, gossip.TOPO_SKIP)
    ev = S.events(200, 110, 20, 21)
    t_cut = S.t_cut_for(110)
    got, want = _run(gossip, topo, ev, t_cut, 3, "reuse", mode=("exact", 2), loss_thr=gossip.loss_threshold(0.2), loss_seed=6,
                     trace=False, max_words=32)
    c = got["counters"]
    print(f"  window {c.words_hw} of {c.words_cap} words for {len(ev)} events")
    assert c.words_cap * 64 < len(ev)  # columns were handed out more than once


def test_window_grows_after_the_setter(gossip):
    n, a, b = S.ring_chords(65, 0)
    topo, ev, t_cut = gossip.Topology.from_links(n, a, b), S.events(65, 50, 1, 22), T0 + 200 * L
    kw = dict(loss_thr=gossip.loss_threshold(0.3), loss_seed=2, flags=gossip.F_TILE_PER_TICK, trace=False)
    eng = _engine(gossip, topo, ev, t_cut, 3, **kw)
    try:
        cap0, bytes0 = eng.counters().words_cap, eng.counters().device_bytes
        eng.run()
        got = _result(eng, trace=False)
    finally:
        eng.close()
    want = _model(topo, ev, t_cut, 3, loss_thr=kw["loss_thr"], loss_seed=2)
    _same(got, want, "growth", trace=False)
    c = got["counters"]
    print(f"  window {cap0} -> {c.words_cap} words, high water {c.words_hw}")
    assert c.words_hw > cap0 and c.words_cap > cap0 and c.device_bytes > bytes0
    assert got["rounds"].resent_bits == want["resent"]


# ---- a re-send, and nothing else, delivers --------------------------------------------------------------------------------
def test_ring_of_65_under_loss(gossip):
    topo, ev, t_cut = _ring65(gossip)
    loss = 1 << 31
    one = _model(topo, ev, t_cut, 1, loss_thr=loss, loss_seed=4)
    assert 0 < int(one["recv"].sum()) < 64  # r = 1: the flood stops where a loss hits, in both directions
    eng = _engine(gossip, topo, ev, t_cut, None, loss_thr=loss, loss_seed=4)
    try:
        eng.run()
        _same(_result(eng), one, "ring r = 1")
    finally:
        eng.close()
    got, want = _run(gossip, topo, ev, t_cut, 4, "ring r = 4", loss_thr=loss, loss_seed=4)
    assert int(want["recv"].sum()) > int(one["recv"].sum())
    assert int(want["trace"][3].max()) > int(one["trace"][3].max())


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

    for kw, match in [(dict(flags=gossip.F_HOP_BATCH), "HOP_BATCH"), (dict(flags=gossip.F_HANDSHAKE), "HANDSHAKE"),
                      (dict(part=(0, 2)), "row partition"), (dict(mode=gossip.MODE_DENSE), "DENSE"),
                      (dict(opts=dict(dense_rows=1)), "dense_rows")]:
        eng = make(**kw)
        try:
            _refused(gossip, gossip.E_INVAL, match, lambda: eng.set_rounds(3))
        finally:
            eng.close()
    eng = make(graph=False)
    try:
        _refused(gossip, gossip.E_STATE, "graph", lambda: eng.set_rounds(3))
        eng.set_topology(topo)
        _refused(gossip, gossip.E_INVAL, "rounds: 1 .. 16", lambda: eng.set_rounds(0))
        _refused(gossip, gossip.E_INVAL, "rounds: 1 .. 16", lambda: eng.set_rounds(17))
        # a refused call left the engine as it was: not in the thinning mode, where forcing young on is refused
        eng.set_option("young", 1)
        eng.set_option("young", -1)
        eng.set_rounds(16)
        assert eng.mode == gossip.MODE_CSR
        _refused(gossip, gossip.E_INVAL, "young", lambda: eng.set_option("young", 1))
        _refused(gossip, gossip.E_INVAL, "dense_rows", lambda: eng.set_option("dense_rows", 1))  # forcing it on afterwards
        eng.set_rounds(1)
        eng.set_option("dense_rows", 1)  # off again: the option is free
        eng.set_option("dense_rows", -1)
        eng.set_rounds(2)
        eng.set_schedule(ev)
        _refused(gossip, gossip.E_STATE, "before the schedule", lambda: eng.set_rounds(3))
    finally:
        eng.close()


# ---- the command-line tool -----------------------------------------------------------------------------------------------
def test_cli_rounds(gossip):
    from conftest import PKG
    sim = os.path.join(PKG, "lib", "gossip_sim")
    n, p, lat = 200, 0.04, 5_000_000
    t0, t_cut = gossip.seconds_to_ns(5.0), gossip.seconds_to_ns(8.9)
    topo = gossip.Topology.gnp(n, p, 5, gossip.TOPO_EXACT)
    ev = gossip.unique_ids(gossip.make_schedule(n, 6, t0, t_cut))
    eng = gossip.Engine(n, lat, t0, t_cut)
    try:
        eng.set_topology(topo)
        eng.set_fanout_exact(2, 1)
        eng.set_link_loss(0.3, 1)
        eng.set_rounds(3)
        eng.set_schedule(ev)
        eng.run()
        eng.sync()
        st, edge_events, resent = eng.stats(), int(eng.counters().edge_events), eng.rounds_counters().resent_bits
    finally:
        eng.close()
    assert resent > 0 and 0 < edge_events < 1 << 32
    args = [sim, f"--numNodes={n}", f"--connectionProb={p}", "--simTime=9", "--seed=5", "--nodeSeed=6", "--uniqueIds",
            "--rounds", "3", "--fanoutExact", "2", "--loss", "0.3"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert gossip.format_statistics(st) in r.stdout
    assert int(re.search(r"Total shares sent: (\d+)", r.stdout).group(1)) == edge_events == int(st.sent.sum())
    # the library's refusal, in the library's words
    r = subprocess.run(args[:7] + ["--rounds", "17"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "rounds: 1 .. 16" in r.stderr
    r = subprocess.run([x for x in args if x != "--uniqueIds"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--uniqueIds" in r.stderr
