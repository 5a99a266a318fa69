"""Exact-k fanout on the device (k_fanout_kth and the exact count passes, csrc/fanout_kernel.h) against
the model (fanout_exact_ref.py): engine and model agree EXACTLY on per-node gen, recv, fwd, sent and
processed and on edge_events, and with F_TRACE | F_REACH on the (node, share, hop) set, the ticks and the
reach table.  The model equals the closed form of a flood at k >= degree (test_fanout_exact_cpu.py).  The
inputs are those of test_fanout_gpu.py.

Figures of the base inputs (G(1000, mean degree 8), topology seed 7, events(1000, 6, 8, 8): 48 shares, cut
60 ticks out, selection seed 1), from the model: mean coverage 0.0092 / 0.7645 / 0.9408 / 0.9823 at k = 1 /
2 / 3 / 4 and 48 / 0 / 0 / 0 shares under 5 % coverage (binomial fanout: 0.6707 / 0.8803 / 0.9608 and 6 / 3 / 1
at 2 / 3 / 4); sends 441 / 73,352 / 135,178 / 187,124 (binomial: 64,535 / 127,367 / 183,207).  BASE_FIGURES
below; the test re-derives and asserts them.
"""
import numpy as np
import pytest

import fanout_exact_ref as X
import fanout_ref as F
import faults_ref as R
import structured as S
from cases import L, T0
from test_fanout_gpu import FAR, OPTIONS, _base, _fanout_records, _links, _pull_keys, _refused, _result, _same, _same_totals

pytestmark = pytest.mark.gpu

FIRST = T0 // L
# k -> (mean coverage, shares under 5 % coverage) of the base inputs, cut 60 ticks out
BASE_FIGURES = {1: (0.0092, 48), 2: (0.7645, 0), 3: (0.9408, 0), 4: (0.9823, 0)}

_MODEL = {}


def _model(topo, ev, t_cut, k, seed=1, outages=(), loss_thr=0, loss_seed=1):
    k = np.ascontiguousarray(np.broadcast_to(np.asarray(k, np.uint32), (topo.num_nodes,)))
    key = (id(topo), ev.tobytes(), t_cut, k.tobytes(), seed, tuple(outages), loss_thr, loss_seed)
    if key not in _MODEL:
        a, b = topo.links()
        m = X.run(topo.num_nodes, a, b, ev, L, t_cut, k, seed, outages=outages, loss_thr=loss_thr, loss_seed=loss_seed)
        assert np.array_equal(m["peers"], topo.degrees()[0])
        _MODEL[key] = m
    return _MODEL[key]


def _engine(gossip, topo, ev, t_cut, k=None, seed=1, setup=None, flags=0, opts=(), snaps=(), trace=True, **kw):
    """k: an int (set_fanout_exact), an array (set_fanout_counts) or None; setup(eng): further setters."""
    fl = gossip.F_REACH | (gossip.F_TRACE if trace else 0) | flags
    eng = gossip.Engine(topo.num_nodes, L, T0, t_cut, flags=fl, **kw)
    try:
        for name, v in dict(opts).items():
            eng.set_option(name, v)
        eng.set_topology(topo)
        if isinstance(k, (int, np.integer)):
            eng.set_fanout_exact(int(k), seed)
        elif k is not None:
            eng.set_fanout_counts(k, seed)
        if setup:
            setup(eng)
        for t in snaps:
            eng.add_snapshot(t)
        eng.set_schedule(ev)
    except BaseException:
        eng.close()
        raise
    return eng


def _invariant(got, k, what):
    want = np.minimum(np.asarray(k, np.uint64), got["peers"].astype(np.uint64)) * got["processed"].astype(np.uint64)
    assert np.array_equal(got["sent"].astype(np.uint64), want), what


def _run(gossip, topo, ev, t_cut, what, k, seed=1, trace=True, faults=None, **kw):
    """One engine run compared with the model; returns the engine's result.  faults: dict(outages=, loss_thr=,
    loss_seed=) for the model, applied to the engine by the setup in kw."""
    eng = _engine(gossip, topo, ev, t_cut, k=k, seed=seed, trace=trace, **kw)
    try:
        eng.run()
        got = _result(eng, trace)
        got["faults"] = eng.fault_counters()
    finally:
        eng.close()
    want = _model(topo, ev, t_cut, k, seed, **(faults or {}))
    _same(got, want, what, trace)
    _invariant(got, k, what)
    f, c = got["fanout"], got["counters"]
    assert f.launches == c.ticks > 0 and f.entries == c.ticks * int(topo.csr()[0][-1]), what
    assert f.bytes > 0, what
    _same_totals(got, topo, what, k=k, seed=seed, **(faults or {}))
    rec = _fanout_records(got, gossip)
    assert set(rec) == ({4, 6, 2} if faults else {4, 5, 2}), (what, sorted(rec))  # args 1 and 3 are absent
    assert all(r.launches == c.ticks for r in rec.values()), what
    return got


# ---- base --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_base_far_cut_figures_and_snapshots(gossip, k):
    topo, ev = _base(gossip)
    snaps = (T0 + 3 * L + L // 2, T0 + 5 * L + 7)
    eng = _engine(gossip, topo, ev, FAR, k=k, snaps=snaps)
    try:
        eng.run()
        got = _result(eng)
        snap = [eng.snapshot(i) for i in range(2)]
    finally:
        eng.close()
    want = _model(topo, ev, FAR, k)
    cov = want["reach"].sum(axis=1) / topo.num_nodes
    print(f"exact fanout {k}: mean coverage {cov.mean():.4f}, under 5 %: {int((cov < 0.05).sum())}, "
          f"hops up to {int(want['trace'][3].max())}, sends {int(want['sent'].sum())}")
    assert (round(float(cov.mean()), 4), int((cov < 0.05).sum())) == BASE_FIGURES[k]
    _same(got, want, ("base", k))
    _invariant(got, k, ("base", k))
    for i, ts in enumerate(snaps):
        assert snap[i][0] == ts and snap[i][2] == X.snapshot_total(want, ev, ts), ("snapshot", k, i)
        assert 0 < snap[i][2] < int(want["processed"].sum())  # inside the floods
    rec = _fanout_records(got, gossip)
    assert set(rec) == {4, 5, 2} and rec[4].launches == rec[5].launches == rec[2].launches == got["counters"].ticks
    f = got["fanout"]
    assert 0 < f.selected_in <= f.selected_out
    # every node selects k of its copies in every tick (degrees 1 .. 21, no ties): the counted out side
    assert f.selected_out == f.launches * int(np.minimum(k, want["peers"]).sum())


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_base_cut_inside_floods(gossip, k):
    topo, ev = _base(gossip)
    got = _run(gossip, topo, ev, S.t_cut_for(6), ("cut", k), k=k)
    far = _model(topo, ev, FAR, k)
    assert 0 < int(got["recv"].sum()) < int(far["recv"].sum())  # the keep masks dropped receptions


# ---- degree and tail boundaries ----------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 32])
def test_ladder_degrees_and_parallel_links(gossip, k):
    topo, ev, t_cut = _links(gossip, "ladder")
    peers, sockets = topo.degrees()
    assert set(S.LADDER_DEGS) <= set(int(x) for x in sockets) and (peers > sockets).any()  # degrees 0 .. 257, multiplicity 2
    assert (peers < k).any() and (peers > k).any() and (peers > 64).any() and (peers > 256).any()  # rows shorter / longer than k, 64, 256
    got = _run(gossip, topo, ev, t_cut, ("ladder", k), k=k, opts=dict(fanout_grid=1))
    rec = _fanout_records(got, gossip)
    for arg in (4, 5, 2):  # 633 nodes on 4 waves: the strided loop of both passes
        assert rec[arg].strided == rec[arg].launches > 0, arg
    assert int(got["sent"].sum()) < int((peers.astype(np.uint64) * got["processed"]).sum())


def test_ladder_counts_at_and_next_to_the_row_length(gossip):
    # k[u] = D - 1, D, D + 1 by u mod 3 at every node of up to 33 peer copies (the ladder's peer counts skip 2
    # and 32, so a uniform k meets D = k only at k = 1), 32 at the hubs
    topo, ev, t_cut = _links(gossip, "ladder")
    peers = topo.degrees()[0].astype(np.int64)
    kk = np.where(peers <= 33, np.clip(peers + np.arange(len(peers)) % 3 - 1, 0, 32), 32).astype(np.uint32)
    assert ((kk == peers) & (peers > 1)).any() and ((kk == peers - 1) & (peers > 1)).any() and (kk > peers).any()
    got = _run(gossip, topo, ev, t_cut, "ladder counts", k=kk, seed=6, opts=dict(fanout_grid=1))
    assert int(got["recv"].sum()) > 0


def test_ladder_k_above_the_limit_is_refused(gossip):
    topo, ev, t_cut = _links(gossip, "ladder")
    peers = topo.degrees()[0]
    eng = gossip.Engine(topo.num_nodes, L, T0, t_cut)
    try:
        eng.set_topology(topo)
        hub = int(np.flatnonzero(peers > 33)[0])
        _refused(gossip, gossip.E_INVAL, rf"node {hub} has {int(peers[hub])} peer copies", lambda: eng.set_fanout_exact(33, 1))
        kk = np.full(topo.num_nodes, 2, np.uint32)
        kk[peers <= 40] = 40  # above 32 where nothing is selected: allowed
        eng.set_fanout_counts(kk, 1)
        kk[hub] = 33
        _refused(gossip, gossip.E_INVAL, rf"node {hub} ", lambda: eng.set_fanout_counts(kk, 1))
    finally:
        eng.close()


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("n", S.TAIL_N)
def test_tails(gossip, n, k):
    topo, ev, t_cut = _links(gossip, f"tail{n}")
    got = _run(gossip, topo, ev, t_cut, ("tail", n, k), k=k, opts=dict(fanout_grid=1))
    rec = _fanout_records(got, gossip)
    assert (rec[4].strided > 0) == (rec[5].strided > 0) == (n > 256)  # one block = 4 waves = 256 nodes


# ---- per-node counts -----------------------------------------------------------------------------------
def test_per_node_counts_and_silent_nodes(gossip):
    topo, ev = _base(gossip)
    rng = np.random.default_rng(23)
    kk = rng.integers(1, 7, size=1000).astype(np.uint32)
    kk[rng.choice(1000, 150, replace=False)] = 0  # silent nodes
    kk[int(ev["node"][0])] = 0                    # a source that never sends
    got = _run(gossip, topo, ev, FAR, "counts", k=kk, seed=9)
    assert 140 <= int((kk == 0).sum()) <= 160
    assert np.all(got["sent"][kk == 0] == 0) and int(got["processed"][kk == 0].sum()) > 0 and int(got["recv"].sum()) > 0


# ---- k >= every degree -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["base", "ladder"])
def test_k_above_every_degree_is_the_plain_engine(gossip, name):
    if name == "base":
        (topo, ev), t_cut = _base(gossip), S.t_cut_for(6)
    else:
        topo, ev, t_cut = _links(gossip, "ladder")
    k = int(topo.degrees()[0].max())
    res = []
    for fan in (False, True):
        eng = _engine(gossip, topo, ev, t_cut, k=k if fan else None)
        try:
            eng.run()
            res.append(_result(eng))
        finally:
            eng.close()
    plain, fan = res
    for key in ("gen", "recv", "fwd", "sent", "processed", "peers", "reach"):
        assert np.array_equal(plain[key], fan[key]), (name, key)
    assert plain["edge_events"] == fan["edge_events"]
    for x, y in zip(S.sorted_trace(plain["trace"]), S.sorted_trace(fan["trace"])):
        assert np.array_equal(x, y), name
    assert _fanout_records(fan, gossip)[4].launches == fan["counters"].ticks == plain["counters"].ticks
    assert not _fanout_records(plain, gossip)


# ---- option invariance -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,opts", OPTIONS, ids=[o[0] for o in OPTIONS])
@pytest.mark.parametrize("flags", [0, 32], ids=["window", "tile_per_tick"])
def test_option_invariance(gossip, name, opts, flags):
    topo, ev = _base(gossip)
    got = _run(gossip, topo, ev, S.t_cut_for(6), ("option", name, flags), k=3, flags=flags, opts=opts)
    assert _pull_keys(got, gossip)


# ---- shards ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count,by_tick", [(2, 0), (3, 0), (2, 1), (3, 1)])
def test_share_shards_add_up(gossip, count, by_tick):
    topo, ev = _base(gossip)
    fl = gossip.F_SHARD_BY_TICK if by_tick else 0
    want = _model(topo, ev, FAR, 3)
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
    _same(got, _model(topo, ev, FAR, 3), "stepping")
    part = _model(topo, ev[ev["ns"] < T0 + 3 * L], T0 + 3 * L, 3)
    assert np.array_equal(mid.sent, part["sent"]) and np.array_equal(mid.recv, part["recv"])


def test_seeds(gossip):
    topo, ev = _base(gossip)
    runs = {}
    for tag, seed in (("a", 1), ("b", 1), ("two", 2), ("high", (1 << 32) + 1)):
        runs[tag] = _run(gossip, topo, ev, FAR, ("seed", tag), k=3, seed=seed, trace=False)
    for key in ("recv", "sent", "reach"):
        assert np.array_equal(runs["a"][key], runs["b"][key])
    assert not np.array_equal(runs["a"]["recv"], runs["two"]["recv"])
    assert not np.array_equal(runs["a"]["recv"], runs["high"]["recv"])
    assert not np.array_equal(runs["two"]["recv"], runs["high"]["recv"])


# ---- faults ------------------------------------------------------------------------------------------------
def _down(n, seed=3):
    rng = np.random.default_rng(seed)
    return tuple((int(v), FIRST + 2, FIRST + 6) for v in np.sort(rng.choice(n, n // 10, replace=False)))


LOSS = 0x1999999A  # 0.1


@pytest.mark.parametrize("case", ["outages", "loss", "both", "both_setters_first"])
def test_with_faults(gossip, case):
    topo, ev = _base(gossip)
    outages = _down(topo.num_nodes) if case != "loss" else ()
    loss = LOSS if case != "outages" else 0
    o = np.array(outages, np.int64).reshape(-1, 3)

    def setup(eng):
        if len(o):
            eng.set_outages(o[:, 0], o[:, 1], o[:, 2])
        if loss:
            eng.set_link_loss(loss, 77)

    faults = dict(outages=outages, loss_thr=loss, loss_seed=77)
    if case == "both_setters_first":  # the fault setters, then the exact setter: either order composes
        eng = _engine(gossip, topo, ev, FAR, k=None, setup=lambda e: (setup(e), e.set_fanout_exact(3, 1)))
        try:
            eng.run()
            got = _result(eng)
            got["faults"] = eng.fault_counters()
        finally:
            eng.close()
        _same(got, _model(topo, ev, FAR, 3, 1, **faults), case)
        assert set(_fanout_records(got, gossip)) == {4, 6, 2}
    else:
        got = _run(gossip, topo, ev, FAR, case, k=3, faults=faults, setup=setup)
    want = _model(topo, ev, FAR, 3, 1, **faults)
    clean = _model(topo, ev, FAR, 3)
    assert int(want["recv"].sum()) < int(clean["recv"].sum())  # the faults bite
    fc = got["faults"]
    assert fc.launches == got["counters"].ticks
    assert (fc.lost_copies > 0) == bool(loss) and (fc.down_node_ticks > 0) == bool(len(o))


def test_loss_draws_are_those_of_the_binomial_run(gossip):
    # the loss key and seed are untouched: the exact model and the binomial model lose the same copies in the
    # same ticks under one loss seed (and the engine equals either model: test_with_faults, test_faults_gpu.py)
    topo, ev = _base(gossip)
    a, b = topo.links()
    ex = _model(topo, ev, FAR, 3, 1, loss_thr=LOSS, loss_seed=77)
    bi = R.run(topo.num_nodes, a, b, ev, L, FAR, F.thresholds(3, topo.degrees()[0]), 1, loss_thr=LOSS, loss_seed=77)
    common = sorted(set(ex["lost_by_tick"]) & set(bi["lost_by_tick"]))
    assert len(common) >= 10
    for t in common:
        assert np.array_equal(ex["lost_by_tick"][t], bi["lost_by_tick"][t]), t
    assert not np.array_equal(ex["recv"], bi["recv"])  # while the selections differ
    # and on the device: both engines' lost copies come from those draws -- each equals its model
    got = _run(gossip, topo, ev, FAR, "loss draws", k=3, faults=dict(loss_thr=LOSS, loss_seed=77), trace=False,
               setup=lambda e: e.set_link_loss(LOSS, 77))
    eng = _engine(gossip, topo, ev, FAR, trace=False, setup=lambda e: (e.set_fanout(3, 1), e.set_link_loss(LOSS, 77)))
    try:
        eng.run()
        _same(_result(eng, False), bi, "binomial with loss", trace=False)
    finally:
        eng.close()
    assert got["faults"].lost_copies > 0


# ---- the four setters: the last one wins -------------------------------------------------------------------
def test_last_setter_wins(gossip):
    topo, ev = _base(gossip)
    a, b = topo.links()
    exact = _model(topo, ev, FAR, 3)
    binom = F.run(topo.num_nodes, a, b, ev, L, FAR, F.thresholds(3, topo.degrees()[0]), 1)
    assert not np.array_equal(exact["recv"], binom["recv"])
    orders = [(lambda e: (e.set_fanout(3, 1), e.set_fanout_exact(3, 1)), exact, {4, 5, 2}),
              (lambda e: (e.set_fanout_exact(3, 1), e.set_fanout(3, 1)), binom, {1, 2}),
              (lambda e: (e.set_fanout_exact(2, 5), e.set_fanout_counts(np.full(1000, 3, np.uint32), 1)), exact, {4, 5, 2}),
              (lambda e: (e.set_fanout_exact(3, 1), e.set_forward_thresholds(F.thresholds(3, topo.degrees()[0]), 1)), binom, {1, 2})]
    for i, (setup, want, args) in enumerate(orders):
        eng = _engine(gossip, topo, ev, FAR, setup=setup, trace=False)
        try:
            eng.run()
            got = _result(eng, False)
        finally:
            eng.close()
        _same(got, want, ("order", i), trace=False)
        assert set(_fanout_records(got, gossip)) == args, i


# ---- off means off -----------------------------------------------------------------------------------------
def test_allocations_are_the_setters(gossip):
    topo, ev = _base(gossip)
    n = topo.num_nodes
    binom = gossip.Engine(n, L, T0, FAR)
    exact = gossip.Engine(n, L, T0, FAR)
    try:
        for e in (binom, exact):
            e.set_topology(topo)
        base = exact.counters().device_bytes
        binom.set_fanout(3, 1)
        exact.set_fanout_exact(3, 1)
        # the binomial setter's allocations are what they were; the exact setter adds its three tables
        assert exact.counters().device_bytes - binom.counters().device_bytes == (n + 1) * 16
        exact.set_fanout_exact(4, 2)  # a second call re-fills them
        assert exact.counters().device_bytes - binom.counters().device_bytes == (n + 1) * 16
        assert binom.counters().device_bytes > base
    finally:
        binom.close()
        exact.close()


# ---- refusals ----------------------------------------------------------------------------------------------
def test_refusals(gossip):
    topo, ev = _base(gossip)
    n = topo.num_nodes
    kk = np.full(n, 3, np.uint32)

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
            _refused(gossip, gossip.E_INVAL, match, lambda: eng.set_fanout_exact(3, 1))
            _refused(gossip, gossip.E_INVAL, match, lambda: eng.set_fanout_counts(kk, 1))
        finally:
            eng.close()
    eng = make(graph=False)
    try:
        _refused(gossip, gossip.E_STATE, "graph", lambda: eng.set_fanout_exact(3, 1))
        _refused(gossip, gossip.E_STATE, "graph", lambda: eng.set_fanout_counts(kk, 1))
        eng.set_topology(topo)
        _refused(gossip, gossip.E_INVAL, "fanout >= 1", lambda: eng.set_fanout_exact(0, 1))
        _refused(gossip, gossip.E_INVAL, "one count per node", lambda: eng.set_fanout_counts(kk[:-1], 1))
        eng.set_fanout_exact(3, 1)
        assert eng.mode == gossip.MODE_CSR
        for name in ("young", "pull_push", "young_skip", "young_idle"):  # forcing one on afterwards
            _refused(gossip, gossip.E_INVAL, name, lambda: eng.set_option(name, 1))
            eng.set_option(name, 0)
        bad = ev.copy()
        bad["share_id"][5] = bad["share_id"][2]
        _refused(gossip, gossip.E_INVAL, f"unique share ids: id {int(bad['share_id'][5])} of node {int(bad['node'][5])}",
                 lambda: eng.set_schedule(bad))
        eng.set_schedule(gossip.unique_ids(bad))
        _refused(gossip, gossip.E_STATE, "before the schedule", lambda: eng.set_fanout_exact(3, 1))
        _refused(gossip, gossip.E_STATE, "before the schedule", lambda: eng.set_fanout_counts(kk, 1))
    finally:
        eng.close()
    # AUTO on a graph dense enough for DENSE mode resolves to CSR once exact fanout is set
    dn = 2048
    dtopo = gossip.Topology.gnp(dn, 0.08, 3, gossip.TOPO_SKIP)
    eng = gossip.Engine(dn, L, T0, FAR)
    try:
        eng.set_topology(dtopo)
        assert eng.mode == gossip.MODE_DENSE
        eng.set_fanout_exact(4, 1)
        assert eng.mode == gossip.MODE_CSR
    finally:
        eng.close()
    # ticks beyond 32 bits (the draw's counter word)
    eng = gossip.Engine(n, 1, T0, T0 + 1000)
    try:
        eng.set_topology(topo)
        _refused(gossip, gossip.E_INVAL, "32 bits", lambda: eng.set_fanout_exact(3, 1))
        _refused(gossip, gossip.E_INVAL, "32 bits", lambda: eng.set_fanout_counts(kk, 1))
    finally:
        eng.close()


# ---- the command-line tool -----------------------------------------------------------------------------------
def test_cli_fanout_exact_with_reach(gossip, tmp_path):
    import os
    import subprocess

    from conftest import PKG
    sim = os.path.join(PKG, "lib", "gossip_sim")
    n, p, lat = 300, 0.03, 5_000_000
    t0, t_cut = gossip.seconds_to_ns(5.0), gossip.seconds_to_ns(8.9)
    topo = gossip.Topology.gnp(n, p, 5, gossip.TOPO_EXACT)
    ev = gossip.make_schedule(n, 6, t0, t_cut)
    a, b = topo.links()
    seed = (1 << 33) + 5
    want = X.run(n, a, b, ev, lat, t_cut, 3, seed)
    assert 0 < int(want["recv"].sum()) and int(want["sent"].sum()) < int((want["peers"].astype(np.uint64) * want["processed"]).sum())
    reach = str(tmp_path / "reach.txt")
    common = [sim, f"--numNodes={n}", f"--connectionProb={p}", "--simTime=9", "--seed=5"]
    r = subprocess.run(common + ["--nodeSeed=6", "--fanoutExact=3", f"--fanoutSeed={seed}", f"--reach={reach}", "--shards=2"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    st = gossip.Stats(want["gen"], want["recv"], want["fwd"], want["sent"], want["processed"], *topo.degrees())
    assert gossip.format_statistics(st) in r.stdout
    rows = [line.split() for line in open(reach)]
    assert len(rows) == len(ev)
    assert [int(x[3]) for x in rows] == want["reach"].sum(axis=1).tolist()
    # --fanout together with --fanoutExact is an error
    r = subprocess.run(common + ["--fanout=3", "--fanoutExact=3", "--quiet"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--fanoutExact" in r.stderr
    # colliding ids: the same --uniqueIds hint
    evf = str(tmp_path / "ev.txt")
    with open(evf, "w") as f:
        for k in range(len(ev)):
            f.write(f"{int(ev['ns'][k])} {int(ev['node'][k])} {int(ev['share_id'][k]) & 7}\n")
    args = common + [f"--events={evf}", "--fanoutExact=3", f"--fanoutSeed={seed}", "--quiet"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--uniqueIds" in r.stderr and "unique share ids" in r.stderr
    r = subprocess.run(args + ["--uniqueIds"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
