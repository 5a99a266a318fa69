"""Fanout-limited gossip on the device (k_fanout_count / k_fanout_compact, csrc/fanout_kernel.h) against
the model (fanout_ref.py): engine and model agree EXACTLY on per-node gen, recv, fwd, sent and
processed and on edge_events, and with F_TRACE | F_REACH on the (node, share, hop) set and the reach
table.  The model equals the closed form of a flood at probability 1 (test_fanout_cpu.py), which
existing tests pin to ORACLE A.

Figures of the base inputs (G(1000, mean degree 8), topology seed 7, events(1000, 6, 8, 8): 48 shares,
cut 60 ticks out, selection seed 1), from the model: mean coverage 0.67 / 0.88 / 0.96 and 6 / 3 / 1 shares
under 5 % coverage at fanout 2 / 3 / 4, floods of up to 23 / 17 / 12 hops, 0.16 / 0.32 / 0.46 of the flood's
sends (BASE_FIGURES below; the test re-derives and asserts them).

The long-window case as the issue states it (ring of 513, every 7th node at 2^31) has short floods: a
node forwards once, so a flood passes k half-probability nodes with probability 2^-k and the window
stays a few hundred words (model: floods of at most 47 hops; 192 words).  It runs as stated; a second
variant with those nodes at 255/256 and a birth in each of 135 ticks keeps 135 tiles alive at once (floods
of up to 395 hops, asserted on the model), so the window spans several k_pull launches.
"""
import functools

import numpy as np
import pytest

import fanout_ref as F
import structured as S
import thinning_ref as TH
from cases import L, T0

pytestmark = pytest.mark.gpu

ALWAYS = 0xFFFFFFFF
FAR = T0 + 60 * L
# fanout -> (mean coverage, shares under 5 % coverage) of the base inputs, cut 60 ticks out
BASE_FIGURES = {2: (0.6707, 6), 3: (0.8803, 3), 4: (0.9608, 1)}
WORDCTL_BYTES, BIRTH_BYTES, RING = 40, 40, 4


@functools.lru_cache(maxsize=None)
def _base(gossip):
    topo = gossip.Topology.gnp(1000, 8.0 / 999.0, 7, gossip.TOPO_SKIP)
    return topo, S.events(1000, 6, 8, 8)


@functools.lru_cache(maxsize=None)
def _links(gossip, name):
    if name == "ladder":
        n, a, b = S.ladder(seed=11, parallel=True)
        ev = S.events(n, 10, 6, 12, must_include=range(len(S.LADDER_DEGS)))
        t_cut = T0 + 40 * L
    elif name.startswith("tail"):
        n = int(name[4:])
        n, a, b = S.ring_chords(n, 7)
        ev, t_cut = S.events(n, 12, min(2, n), 100 + n), S.t_cut_for(12)
    elif name == "ring513":
        n, a, b = S.ring_chords(513, 0)
        ev, t_cut = S.events(n, 12, 2, 14), T0 + 330 * L
    elif name == "ring513_long":  # a birth tick = a tile (F_TILE_PER_TICK): 135 tiles live at once
        n, a, b = S.ring_chords(513, 0)
        ev, t_cut = S.events(n, 135, 1, 14), T0 + 400 * L
    else:
        raise KeyError(name)
    return gossip.Topology.from_links(n, a, b), ev, t_cut


_MODEL = {}


def _model(topo, ev, t_cut, thr, seed):
    thr = np.ascontiguousarray(thr, np.uint32)
    key = (id(topo), ev.tobytes(), t_cut, thr.tobytes(), seed)
    if key not in _MODEL:
        a, b = topo.links()
        m = F.run(topo.num_nodes, a, b, ev, L, t_cut, thr, seed)
        assert np.array_equal(m["peers"], topo.degrees()[0])
        _MODEL[key] = m
    return _MODEL[key]


def _thr(topo, k):
    return F.thresholds(k, topo.degrees()[0])


def _engine(gossip, topo, ev, t_cut, k=None, thr=None, seed=1, flags=0, opts=(), snaps=(), trace=True, **kw):
    fl = gossip.F_REACH | (gossip.F_TRACE if trace else 0) | flags
    eng = gossip.Engine(topo.num_nodes, L, T0, t_cut, flags=fl, **kw)
    for name, v in dict(opts).items():
        eng.set_option(name, v)
    eng.set_topology(topo)
    if k is not None:
        eng.set_fanout(k, seed)
    elif thr is not None:
        eng.set_forward_thresholds(thr, seed)
    for t in snaps:
        eng.add_snapshot(t)
    eng.set_schedule(ev)
    return eng


def _result(eng, trace=True):
    eng.sync()
    st = eng.stats()
    c = eng.counters()
    out = dict(gen=st.gen, recv=st.recv, fwd=st.fwd, sent=st.sent, processed=st.processed, peers=st.peers,
               edge_events=int(c.edge_events), reach=eng.reach(), counters=c, launches=eng.launches(),
               fanout=eng.fanout_counters())
    if trace:
        out["trace"] = eng.trace()
    return out


def _hops_set(trace):
    node, sid, _tick, hop, via = (np.asarray(x, np.int64) for x in trace)
    o = np.lexsort((sid, node))
    return node[o], sid[o], hop[o], via[o]


def _same(got, want, what, trace=True):
    for k in ("gen", "recv", "fwd", "sent", "processed"):
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


def _run(gossip, topo, ev, t_cut, what, k=None, thr=None, seed=1, trace=True, **kw):
    """One engine run compared with the model; returns the engine's result."""
    eng = _engine(gossip, topo, ev, t_cut, k=k, thr=thr, seed=seed, trace=trace, **kw)
    try:
        eng.run()
        got = _result(eng, trace)
    finally:
        eng.close()
    want = _model(topo, ev, t_cut, _thr(topo, k) if k is not None else thr, seed)
    _same(got, want, what, trace)
    f, c = got["fanout"], got["counters"]
    assert f.launches == c.ticks > 0 and f.entries == c.ticks * int(topo.csr()[0][-1]), what
    assert f.bytes > 0, what
    _same_totals(got, topo, what, thr=_thr(topo, k) if k is not None else thr, seed=seed)
    return got


def _same_totals(got, topo, what, **config):
    """The kernels' own totals against the model of the thinned lists (thinning_ref.py), summed over the ticks the
    run executed: every tick thins every list, whether or not a share is on it."""
    first = T0 // L  # gossip_engine_first_tick of every engine here
    want = TH.of_topology(topo, **config).totals(range(first, first + int(got["counters"].ticks)))
    f = got["fanout"]
    assert (f.selected_in, f.selected_out) == (want["selected_in"], want["selected_out"]), (what, want)
    if "faults" in got:
        x = got["faults"]
        assert (x.lost_copies, x.down_copies, x.down_node_ticks) == (want["lost_copies"], want["down_copies"], want["down_node_ticks"]), (what, want)


def _pull_keys(res, gossip):
    return {r.key for r in res["launches"] if r.kernel == gossip.K_PULL}


def _fanout_records(res, gossip):
    return {r.arg: r for r in res["launches"] if r.kernel == gossip.K_FANOUT}


# ---- base --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 4])
def test_base_floods_die_by_themselves(gossip, k):
    topo, ev = _base(gossip)
    snaps = (T0 + 3 * L + L // 2, T0 + 5 * L + 7)
    eng = _engine(gossip, topo, ev, FAR, k=k, snaps=snaps)
    try:
        eng.run()
        got = _result(eng)
        snap = [eng.snapshot(i) for i in range(2)]
    finally:
        eng.close()
    want = _model(topo, ev, FAR, _thr(topo, k), 1)
    # the inputs are non-trivial (asserted on the model): partial coverage, and die-outs at fanout 2
    cov = want["reach"].sum(axis=1) / topo.num_nodes
    print(f"fanout {k}: mean coverage {cov.mean():.4f}, under 5 %: {int((cov < 0.05).sum())}, "
          f"hops up to {int(want['trace'][3].max())}, sends {int(want['sent'].sum())}")
    assert 0.3 < cov.mean() < 0.99
    assert (round(float(cov.mean()), 4), int((cov < 0.05).sum())) == BASE_FIGURES[k]
    if k == 2:
        assert (cov < 0.05).any()
    _same(got, want, ("base", k))
    for i, ts in enumerate(snaps):
        assert snap[i][0] == ts and snap[i][2] == F.snapshot_total(want, ev, want["peers"], ts), ("snapshot", k, i)
        assert 0 < snap[i][2] < int(want["processed"].sum())  # inside the floods
    rec = _fanout_records(got, gossip)
    assert set(rec) == {1, 2} and rec[1].launches == rec[2].launches == got["counters"].ticks
    assert got["fanout"].selected_in > 0 and got["fanout"].selected_in <= got["fanout"].selected_out


@pytest.mark.parametrize("k", [2, 3, 4])
def test_base_cut_inside_floods(gossip, k):
    topo, ev = _base(gossip)
    got = _run(gossip, topo, ev, S.t_cut_for(6), ("cut", k), k=k)
    far = _model(topo, ev, FAR, _thr(topo, k), 1)
    assert 0 < int(got["recv"].sum()) < int(far["recv"].sum())  # the keep masks dropped receptions


# ---- degree and tail boundaries ----------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 64])
def test_ladder_degrees_and_parallel_links(gossip, k):
    topo, ev, t_cut = _links(gossip, "ladder")
    peers, sockets = topo.degrees()
    assert set(S.LADDER_DEGS) <= set(int(x) for x in sockets) and (peers > sockets).any()  # degrees 0 .. 257, multiplicity 2
    # (set_fanout's thresholds: the model's are floor(k 2^32 / peers) with peers the sum of multiplicities,
    #  which differs from the distinct-peer count at every second hub link -- exact agreement pins both)
    got = _run(gossip, topo, ev, t_cut, ("ladder", k), k=k, opts=dict(fanout_grid=1))
    rec = _fanout_records(got, gossip)
    assert rec[1].strided == rec[1].launches > 0 and rec[2].strided == rec[2].launches  # 633 nodes on 4 waves
    if k == 64:  # every node of degree <= 64 floods; the hubs above it do not
        assert int(got["sent"].sum()) < int((peers.astype(np.uint64) * got["processed"]).sum())


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("n", S.TAIL_N)
def test_tails(gossip, n, k):
    topo, ev, t_cut = _links(gossip, f"tail{n}")
    got = _run(gossip, topo, ev, t_cut, ("tail", n, k), k=k, opts=dict(fanout_grid=1))
    rec = _fanout_records(got, gossip)
    assert (rec[1].strided > 0) == (n > 256)  # one block = 4 waves = 256 nodes


# ---- long, wide window ---------------------------------------------------------------------------------
@pytest.mark.parametrize("gate", [1 << 31, 0xFF000000])
def test_long_window_many_pull_launches(gossip, gate):
    topo, ev, t_cut = _links(gossip, "ring513" if gate == 1 << 31 else "ring513_long")
    thr = np.full(513, ALWAYS, np.uint32)
    thr[::7] = gate
    want = _model(topo, ev, t_cut, thr, 5)
    hops = int(want["trace"][3].max())
    print(f"gate {gate:#x}: longest flood {hops} hops, receptions {int(want['recv'].sum())}")
    got = _run(gossip, topo, ev, t_cut, ("ring513", gate), thr=thr, seed=5, trace=False, flags=gossip.F_TILE_PER_TICK)
    pulls = sum(r.launches for r in got["launches"] if r.kernel == gossip.K_PULL)
    print(f"  window high water {got['counters'].words_hw} words, {pulls} k_pull launches in {got['counters'].ticks} ticks")
    if gate != 1 << 31:
        assert hops >= 300 and 0 < int(want["recv"].sum()) < 135 * 512  # long floods, some cut short at a gate
        assert got["counters"].words_hw > 2048 and pulls > got["counters"].ticks


# ---- probability 1 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["base", "ladder"])
def test_probability_one_is_the_plain_engine(gossip, name):
    if name == "base":
        (topo, ev), t_cut = _base(gossip), S.t_cut_for(6)
    else:
        topo, ev, t_cut = _links(gossip, "ladder")
    res = []
    for fan in (False, True):
        eng = _engine(gossip, topo, ev, t_cut, thr=np.full(topo.num_nodes, ALWAYS, np.uint32) if fan else None)
        try:
            eng.run()
            res.append(_result(eng))
        finally:
            eng.close()
    plain, fan = res
    for k in ("gen", "recv", "fwd", "sent", "processed", "peers", "reach"):
        assert np.array_equal(plain[k], fan[k]), (name, k)
    assert plain["edge_events"] == fan["edge_events"]
    for x, y in zip(S.sorted_trace(plain["trace"]), S.sorted_trace(fan["trace"])):
        assert np.array_equal(x, y), name
    rec = _fanout_records(fan, gossip)
    assert rec[1].launches == fan["counters"].ticks == plain["counters"].ticks
    assert not _fanout_records(plain, gossip)


# ---- arbitrary thresholds ------------------------------------------------------------------------------
def test_arbitrary_thresholds(gossip):
    topo, ev = _base(gossip)
    rng = np.random.default_rng(21)
    thr = rng.integers(1 << 29, 1 << 32, size=1000, dtype=np.uint64).astype(np.uint32)
    thr[rng.choice(1000, 150, replace=False)] = 0       # silent nodes
    thr[rng.choice(1000, 150, replace=False)] = ALWAYS
    thr[int(ev["node"][0])] = 0                         # a source that never sends
    got = _run(gossip, topo, ev, FAR, "thresholds", thr=thr, seed=9)
    assert np.all(got["sent"][thr == 0] == 0) and int(got["recv"].sum()) > 0


# ---- option invariance -----------------------------------------------------------------------------------
# ("seen_fold" 0 is vacuous by design: fanout mode resolves folded rows to off, since a folded row would
#  deliver seen | new and with it shares the sender withheld; the case only shows the option stays legal.
#  seen_fold 1 -- "the same as auto" -- is the other legal value and resolves to off as well.)
OPTIONS = [("default", {}), ("seen_fold_1", dict(seen_fold=1)), ("dense_rows", dict(dense_rows=1)), ("seen_fold", dict(seen_fold=0)), ("pull_sat", dict(pull_sat=0)),
           ("late_age", dict(late_age=0)), ("pull_tiles", dict(pull_tiles=0)), ("peer_order", dict(peer_order=0)),
           ("pull_batch", dict(pull_batch=1)), ("pull_nt", dict(pull_nt=1)), ("pull_grid", dict(pull_grid=1))]
@pytest.mark.parametrize("name,opts", OPTIONS, ids=[o[0] for o in OPTIONS])
@pytest.mark.parametrize("flags", [0, 32], ids=["window", "tile_per_tick"])
def test_option_invariance(gossip, name, opts, flags):
    topo, ev = _base(gossip)
    got = _run(gossip, topo, ev, S.t_cut_for(6), ("option", name, flags), k=3, flags=flags, opts=opts)
    keys = _pull_keys(got, gossip)
    assert keys
    if name == "pull_tiles":
        assert not any(k[3] & gossip.PULL_SP for k in keys)
    if name == "pull_grid":
        assert all(r.strided == r.launches for r in got["launches"] if r.kernel == gossip.K_PULL)


def test_option_runs_use_different_pull_kernels(gossip):
    # the invariance above is over different compiled kernels: the lane shapes of a growing window, the
    # tile-mask (SP) instantiation and, without tile lists, the plain one
    topo, ev = _base(gossip)
    union = set()
    for opts in ({}, dict(pull_tiles=0)):
        got = _run(gossip, topo, ev, S.t_cut_for(6), ("kernels", tuple(opts)), k=3, flags=gossip.F_TILE_PER_TICK, opts=opts,
                   trace=False)
        union |= _pull_keys(got, gossip)
    print(sorted(union))
    assert len(union) >= 3
    assert any(k[3] & gossip.PULL_SP for k in union) and any(not k[3] & gossip.PULL_SP for k in union)


# ---- shards ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count,by_tick", [(2, 0), (3, 0), (2, 1), (3, 1)])
def test_share_shards_add_up(gossip, count, by_tick):
    topo, ev = _base(gossip)
    fl = gossip.F_SHARD_BY_TICK if by_tick else 0
    want = _model(topo, ev, FAR, _thr(topo, 3), 1)
    parts = []
    for r in range(count):
        eng = _engine(gossip, topo, ev, FAR, k=3, flags=fl, trace=False, shard_rank=r, shard_count=count)
        try:
            eng.run()
            parts.append(_result(eng, trace=False))
        finally:
            eng.close()
    assert sum(int(p["gen"].sum()) > 0 for p in parts) >= 2  # the shares really are split
    tot = {k: sum(p[k].astype(np.uint64) for p in parts) for k in ("gen", "recv", "fwd", "sent", "processed", "reach")}
    tot["edge_events"] = sum(p["edge_events"] for p in parts)
    _same(tot, want, ("shards", count, by_tick), trace=False)


# ---- stepping, seeds ---------------------------------------------------------------------------------------
def test_stepping(gossip):
    topo, ev = _base(gossip)
    eng = _engine(gossip, topo, ev, FAR, k=3)
    try:
        first = eng.first_tick
        eng.run(first + 3)
        mid = eng.stats()
        eng.run(first + 9)
        eng.run()
        got = _result(eng)
    finally:
        eng.close()
    want = _model(topo, ev, FAR, _thr(topo, 3), 1)
    _same(got, want, "stepping")
    # after 3 ticks: the sends of the generations and receptions of ticks first .. first + 2
    part = _model(topo, ev[ev["ns"] < T0 + 3 * L], T0 + 3 * L, _thr(topo, 3), 1)
    assert np.array_equal(mid.sent, part["sent"]) and np.array_equal(mid.recv, part["recv"])


def test_seeds(gossip):
    topo, ev = _base(gossip)
    runs = {}
    for tag, seed in (("a", 1), ("b", 1), ("two", 2), ("high", (1 << 32) + 1)):
        runs[tag] = _run(gossip, topo, ev, FAR, ("seed", tag), k=3, seed=seed, trace=False)
    for k in ("recv", "sent", "reach"):
        assert np.array_equal(runs["a"][k], runs["b"][k])
    assert not np.array_equal(runs["a"]["recv"], runs["two"]["recv"])
    assert not np.array_equal(runs["a"]["recv"], runs["high"]["recv"])


# ---- refusals ----------------------------------------------------------------------------------------------
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

    cases = [(dict(flags=gossip.F_HOP_BATCH), "HOP_BATCH"), (dict(flags=gossip.F_HANDSHAKE), "HANDSHAKE"),
             (dict(part=(0, 2)), "row partition"), (dict(mode=gossip.MODE_DENSE), "DENSE"),
             (dict(opts=dict(young=1)), "young"), (dict(opts=dict(pull_push=1)), "pull_push"),
             (dict(opts=dict(young_skip=1)), "young_skip"), (dict(opts=dict(young_idle=1)), "young_idle")]
    for kw, match in cases:
        eng = make(**kw)
        try:
            _refused(gossip, gossip.E_INVAL, match, lambda: eng.set_fanout(3, 1))
            _refused(gossip, gossip.E_INVAL, match, lambda: eng.set_forward_thresholds(np.zeros(n, np.uint32), 1))
        finally:
            eng.close()
    eng = make(graph=False)
    try:
        _refused(gossip, gossip.E_STATE, "graph", lambda: eng.set_fanout(3, 1))
        eng.set_topology(topo)
        _refused(gossip, gossip.E_INVAL, "fanout >= 1", lambda: eng.set_fanout(0, 1))
        eng.set_fanout(3, 1)
        assert eng.mode == gossip.MODE_CSR
        for name in ("young", "pull_push", "young_skip", "young_idle"):  # forcing one on afterwards
            _refused(gossip, gossip.E_INVAL, name, lambda: eng.set_option(name, 1))
            eng.set_option(name, 0)
        # colliding ids: the first collision is named
        bad = ev.copy()
        bad["share_id"][5] = bad["share_id"][2]
        _refused(gossip, gossip.E_INVAL, f"unique share ids: id {int(bad['share_id'][5])} of node {int(bad['node'][5])}",
                 lambda: eng.set_schedule(bad))
        eng.set_schedule(gossip.unique_ids(bad))
        _refused(gossip, gossip.E_STATE, "before the schedule", lambda: eng.set_fanout(3, 1))
        _refused(gossip, gossip.E_STATE, "before the schedule", lambda: eng.set_forward_thresholds(np.zeros(n, np.uint32), 1))
    finally:
        eng.close()
    # AUTO on a graph dense enough for DENSE mode resolves to CSR once fanout is set
    dn = 2048
    dtopo = gossip.Topology.gnp(dn, 0.08, 3, gossip.TOPO_SKIP)
    eng = gossip.Engine(dn, L, T0, FAR)
    try:
        eng.set_topology(dtopo)
        assert eng.mode == gossip.MODE_DENSE
        eng.set_fanout(4, 1)
        assert eng.mode == gossip.MODE_CSR
    finally:
        eng.close()
    # ticks beyond 32 bits (the draw's counter word): a 1 ns latency puts t_start at tick 5 x 10^9
    eng = gossip.Engine(n, 1, T0, T0 + 1000)
    try:
        eng.set_topology(topo)
        _refused(gossip, gossip.E_INVAL, "32 bits", lambda: eng.set_fanout(3, 1))
        _refused(gossip, gossip.E_INVAL, "32 bits", lambda: eng.set_forward_thresholds(np.zeros(n, np.uint32), 1))
    finally:
        eng.close()


def test_auto_dense_graph_runs_the_csr_pull(gossip):
    # an engine whose AUTO mode had resolved to DENSE at the graph, switched to CSR by the setter,
    # against the model (mean degree 164: thresholds of about 4 / 164)
    dn = 2048
    dtopo = gossip.Topology.gnp(dn, 0.08, 3, gossip.TOPO_SKIP)
    ev = S.events(dn, 3, 4, 5)
    probe = gossip.Engine(dn, L, T0, FAR)
    try:
        probe.set_topology(dtopo)
        assert probe.mode == gossip.MODE_DENSE
    finally:
        probe.close()
    got = _run(gossip, dtopo, ev, T0 + 30 * L, "auto dense", k=4, trace=False)
    assert not [r for r in got["launches"] if r.kernel in (gossip.K_DENSE_BITS, gossip.K_DENSE_DEDUP)]
    assert int(got["recv"].sum()) > dn


# ---- off means off -------------------------------------------------------------------------------------------
def test_off_means_off(gossip):
    topo, ev = _base(gossip)
    t_cut = S.t_cut_for(6)
    plain = gossip.Engine(topo.num_nodes, L, T0, t_cut)
    fan = gossip.Engine(topo.num_nodes, L, T0, t_cut)
    try:
        for e in (plain, fan):
            e.set_topology(topo)
        fan.set_fanout(3, 1)
        before = fan.counters().device_bytes
        for e in (plain, fan):
            e.set_schedule(ev)
            e.run()
            e.sync()
        assert not [r for r in plain.launches() if r.kernel == gossip.K_FANOUT]
        f = plain.fanout_counters()
        assert (f.launches, f.selected_in, f.selected_out, f.entries, f.ms, f.bytes) == (0, 0, 0, 0, 0.0, 0)
        # the engine's device memory by the recipe that held before fanout mode existed: three bitmaps,
        # occupancy x 2 + saturation words, counters, graph, liveness, the staging ring
        c = plain.counters()
        n, nnz, stride = topo.num_nodes, int(topo.csr()[0][-1]), c.words_cap
        ntw = (stride + 1023) // 1024
        bcap = int(np.bincount((ev["ns"] // L).astype(np.int64) - T0 // L).max())
        recipe = (3 * n * stride * 8 + 24 * n * ntw + n * 20 + nnz * 4 + (n + 1) * 8 + 2 * stride * 8 +
                  RING * (stride * WORDCTL_BYTES + bcap * BIRTH_BYTES + 4))
        print(f"device_bytes plain {c.device_bytes} recipe {recipe} fanout {fan.counters().device_bytes} (setter: {before})")
        assert c.device_bytes == recipe
        # and what the setter allocated is what the fanout engine holds on top
        assert before > 0 and fan.counters().device_bytes == recipe + before
        assert before >= nnz * 9 + (n + 1) * 32
    finally:
        plain.close()
        fan.close()


# ---- the command-line tool -----------------------------------------------------------------------------------
def test_cli_fanout_with_reach(gossip, tmp_path):
    import os
    import re
    import subprocess

    from conftest import PKG
    sim = os.path.join(PKG, "lib", "gossip_sim")
    n, p, lat = 300, 0.03, 5_000_000
    t0, t_cut = gossip.seconds_to_ns(5.0), gossip.seconds_to_ns(8.9)
    topo = gossip.Topology.gnp(n, p, 5, gossip.TOPO_EXACT)
    ev = gossip.make_schedule(n, 6, t0, t_cut)
    a, b = topo.links()
    want = F.run(n, a, b, ev, lat, t_cut, F.thresholds(3, topo.degrees()[0]), (1 << 33) + 5)
    assert 0 < int(want["recv"].sum()) and int(want["sent"].sum()) < int((want["peers"].astype(np.uint64) * want["processed"]).sum())
    reach = str(tmp_path / "reach.txt")
    r = subprocess.run([sim, f"--numNodes={n}", f"--connectionProb={p}", "--simTime=9", "--seed=5", "--nodeSeed=6", "--fanout=3",
                        f"--fanoutSeed={(1 << 33) + 5}", f"--reach={reach}", "--shards=2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    st = gossip.Stats(want["gen"], want["recv"], want["fwd"], want["sent"], want["processed"], *topo.degrees())
    assert gossip.format_statistics(st) in r.stdout  # the report format is unchanged
    rows = [line.split() for line in open(reach)]
    assert len(rows) == len(ev)
    assert [int(x[3]) for x in rows] == want["reach"].sum(axis=1).tolist()
    # colliding ids: the error names --uniqueIds, and --uniqueIds runs
    evf = str(tmp_path / "ev.txt")
    with open(evf, "w") as f:
        for k in range(len(ev)):
            f.write(f"{int(ev['ns'][k])} {int(ev['node'][k])} {int(ev['share_id'][k]) & 7}\n")
    args = [sim, f"--numNodes={n}", f"--connectionProb={p}", "--simTime=9", "--seed=5", f"--events={evf}", "--fanout=3",
            f"--fanoutSeed={(1 << 33) + 5}", "--quiet"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--uniqueIds" in r.stderr and "unique share ids" in r.stderr
    r = subprocess.run(args + ["--uniqueIds"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert re.search(rf"Total shares sent: {int(want['sent'].sum())}\b", r.stdout)
