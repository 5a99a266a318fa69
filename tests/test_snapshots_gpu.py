"""Periodic snapshots (gossip_engine_add_snapshot / get_snapshot) inside a tick, against ORACLE A.

A snapshot at T with T % latency != 0 gives every word of its tick a column mask (ctl.snap: the
columns whose phase is below T's), and each kernel that finds new bits adds popcount(new & mask) to
the snapshot's partial: k_pull in all its instantiations, k_pull_young, k_dense_dedup, k_dense_fused,
k_births (one per effective birth, minus one where an own generation cancels an arrival the pull has
counted), and k_snap_count with per-column masks in hop-batched runs.  A tick-aligned snapshot takes
none of that code (base sums only).

Every run here adds the snapshot set of snapshot_ref.times -- in-tick times in the first ticks, mid
run, in the last tick and in the cut tick, one aligned, one before the run, one after the cut -- and
compares every snapshot with snapshot_ref.expected (the events of ORACLE A's trace with t < T), and
the seven per-node counters with ORACLE A's.  test_snapshot_ref.py pins that reference against ORACLE
A's own periodic rows and shows that the snapshot ticks hold events on both sides of T.  One engine per
(case, path); the path's own counters show that it ran.
"""
import numpy as np
import pytest

import snapshot_ref as R
import structured as S
import test_structured_gpu as TS
from cases import CASES, L, T0

pytestmark = pytest.mark.gpu

STATS = TS.STATS
SUM = ("gen", "recv", "fwd", "sent", "processed")
TPT = TS.TPT

# the CSR paths of test_structured_gpu.py and four more
NEW_PATHS = {
    "seen_fold": ((TPT,), (("dense_rows", 1), ("seen_fold", 1))),
    "seen_fold_young": ((TPT,), (("dense_rows", 1), ("seen_fold", 1), ("young", 1))),
    "short_batch": ((TPT,), (("pull_batch", 1), ("dense_rows", 1))),
    # The ladder's hubs put every node within four hops of every other (ORACLE A's largest hop count): at
    # the default young_age (5) and at young_tight's 6 a flood is over before its tile leaves the young
    # set, k_pull_young counts every arrival and k_pull none.  Two hops: both kernels add to the one
    # partial of a tick.
    "young_age2": ((TPT,), (("young", 1), ("young_age", 2))),
}
PATHS = dict(TS.PATHS, **NEW_PATHS)
FOLD_PATHS = ("seen_fold", "seen_fold_young")


def _make(gossip, name, lat, ts, flags=(), opts=(), mode=None, max_words=0, link=None, part=None, shard=(0, 1)):
    """An engine over the family's inputs with the snapshots ts, ready to run."""
    f = TS._family(name)
    fl = 0
    for x in flags:
        fl |= getattr(gossip, x)
    eng = gossip.Engine(f["n"], lat, T0, f["t_cut"], flags=fl, mode=gossip.MODE_AUTO if mode is None else mode,
                        max_words=max_words, shard_rank=shard[0], shard_count=shard[1])
    try:
        for k, v in opts:
            eng.set_option(k, v)
        if part is not None:
            eng.set_row_partition(*part)
        eng.set_topology(TS._topo(gossip, name))
        if link is not None:
            eng.set_link_timing(*link)
        for T in ts:
            eng.add_snapshot(T)
        eng.set_schedule(f["ev"])
    except Exception:
        eng.close()
        raise
    return eng


def _run(gossip, name, lat, ts, **kw):
    """(stats, counters, snapshots) of one complete run."""
    eng = _make(gossip, name, lat, ts, **kw)
    try:
        eng.run()
        eng.sync()
        return eng.stats(), TS.counters_with_ledger(eng), [eng.snapshot(k) for k in range(len(ts))]
    finally:
        eng.close()


def _assert_stats(st, r, what, keys=STATS):
    for k in keys:
        got, want = np.asarray(getattr(st, k)), getattr(r, k)
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{what}: {k} differs at {len(bad)} nodes, first {bad[:8].tolist()}: "
                                 f"engine {got[bad[:8]].tolist()} oracle {want[bad[:8]].tolist()}")
    assert int(r.recv.sum()) > 0


def _assert_snaps(snaps, r, lat, ts, what):
    want = [R.expected(r, T) for T in ts]
    bad = [f"T = tick0 {T // lat - T0 // lat:+d} + {T % lat} ns: engine (gen, processed) {got[1:]}, oracle {w[1:]}, "
           f"(arrivals, generations) of the tick before | after T {R.splits(r, lat, T)}"
           for T, got, w in zip(ts, snaps, want) if tuple(got) != w]
    assert not bad, f"{what}: {len(bad)} of {len(ts)} snapshots differ:\n  " + "\n  ".join(bad)


def _ran_new(path, c, name):
    what = (name, path)
    assert c.pull_launches > 0 and c.ticks > 0, what
    if name == "ladder":
        assert c.pull_lpw == 32 and c.words_hw > 64, what
    # (a tile is folded only once every member of its id groups is born: ladder_collide's 64 ids recur
    #  through all 40 birth ticks, so none of its tiles is sealed while it is read dense -- the fold
    #  paths run there as dense-row paths with seen_fold on and fold no row)
    if path in FOLD_PATHS and name != "ladder_collide":
        assert c.pull_fold_rows > 0, what
    if path in ("seen_fold_young", "young_age2"):
        assert c.young_launches > 0 and c.young_slot_lines > 0, what
    else:
        assert c.young_launches == 0, what


def _csr(gossip, oracle, name, path, lat=L, which="A", flags=None, **kw):
    f = TS._family(name)
    pf, opts = PATHS[path]
    ts = R.family_times(f, lat, which)
    st, c, snaps = _run(gossip, name, lat, ts, flags=pf if flags is None else flags, opts=opts, **kw)
    r = R.replay(oracle, f, lat)
    what = (name, path, lat, which)
    _assert_snaps(snaps, r, lat, ts, what)
    _assert_stats(st, r, what)
    if path in TS.PATHS:
        TS._ran(path, c, name)
        if name == "ladder":
            TS._ran_ladder(path, c, name)
    else:
        _ran_new(path, c, name)
    return c


# ---- CSR paths ------------------------------------------------------------------------------------
@pytest.mark.parametrize("lat", [L, S.L_ODD], ids=["5ms", "2.3ms"])
@pytest.mark.parametrize("path", list(PATHS))
def test_ladder(gossip, oracle, path, lat):
    _csr(gossip, oracle, "ladder", path, lat)


@pytest.mark.parametrize("lat", [L, S.L_ODD], ids=["5ms", "2.3ms"])
@pytest.mark.parametrize("path", ["default", "wide_nt_push", "young_tight", "seen_fold"])
def test_ladder_set_b(gossip, oracle, path, lat):
    # T = t_cut itself (the snapshot mask equals the keep mask), r = 1 (an empty mask) and r = lat - 1
    _csr(gossip, oracle, "ladder", path, lat, which="B")


@pytest.mark.parametrize("path", TS.COLLIDE_PATHS + FOLD_PATHS)
@pytest.mark.parametrize("name", ["ladder_collide", "components_collide"])
def test_colliding_ids(gossip, oracle, name, path):
    # id groups; components_collide's tick +18 holds an own generation that cancels a counted arrival
    _csr(gossip, oracle, name, path)


@pytest.mark.parametrize("path", ["default", "wide_nt_push", "young", "young_tight"])
@pytest.mark.parametrize("name", ["tail[65]", "tail[513]"])
def test_tails(gossip, oracle, name, path):
    _csr(gossip, oracle, name, path)


@pytest.mark.parametrize("path", ["wide", "young", "seen_fold"])
def test_long_ring(gossip, oracle, path):
    # a window above 2,048 words: a tick is several k_pull launches, each adds to the one partial
    c = _csr(gossip, oracle, "long_ring", path, flags=tuple(set(PATHS[path][0]) | {TPT}))
    assert c.words_hw > 2048, c.words_hw


def test_window_grows_between_snapshots(gossip, oracle):
    c = _csr(gossip, oracle, "ladder", "wide", max_words=16)
    assert c.words_cap > 16 and c.words_hw > 16


# ---- hand cases: closed-form values -----------------------------------------------------------------
HAND_PATHS = {
    "default": ((), ()),
    "dense_rows": ((), (("dense_rows", 1),)),
    "young": ((TPT,), (("young", 1),)),  # k_births' slot branch
}


@pytest.mark.parametrize("path", list(HAND_PATHS))
@pytest.mark.parametrize("name", list(R.HAND))
def test_hand_cases(gossip, name, path):
    c = next(x for x in CASES if x["name"] == name)
    topo = gossip.Topology.from_links(c["n"], [x for x, _ in c["links"]], [y for _, y in c["links"]])
    ev = np.array(c["events"], np.int64)
    ev = gossip.events_from_arrays(ev[:, 0], ev[:, 1], ev[:, 2])
    flags, opts = HAND_PATHS[path]
    fl = 0
    for x in flags:
        fl |= getattr(gossip, x)
    for ph, want in R.HAND[name]:
        # tick +1 after node 1's arrival (phase 123,457), node 2's tick at phase ph, tick +3 aligned
        ts = [T0 + L + L // 2, T0 + R.HAND_TICK * L + ph, T0 + 3 * L]
        eng = gossip.Engine(c["n"], L, T0, c["t_cut"], flags=fl)
        try:
            for k, v in opts:
                eng.set_option(k, v)
            eng.set_topology(topo)
            for T in ts:
                eng.add_snapshot(T)
            eng.set_schedule(ev)
            eng.run()
            eng.sync()
            st, cn = eng.stats(), eng.counters()
            got = [eng.snapshot(k) for k in range(len(ts))]
        finally:
            eng.close()
        assert got == [(ts[0], 1, 2), (ts[1],) + want, (ts[2], 2, 3)], (name, path, ph)
        for k, w in c["expect"].items():
            assert getattr(st, k).tolist() == w, (name, path, ph, k)
        if path == "young":
            assert cn.young_launches > 0, (name, path)
        else:
            assert cn.young_launches == 0, (name, path)


# ---- DENSE mode -------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("name,lat", [("ladder", L), ("dense_tail[1025]", L), ("dense_sparse", L), ("ladder_collide", L),
                                      ("dense_tail[1025]", S.L_ODD)])
def test_dense(gossip, oracle, name, lat, fused):
    f = TS._family(name)
    ts = R.family_times(f, lat)
    st, c, snaps = _run(gossip, name, lat, ts, opts=(("dense_fused", fused),), mode=gossip.MODE_DENSE)
    r = R.replay(oracle, f, lat)
    what = (name, lat, "dense", fused)
    _assert_snaps(snaps, r, lat, ts, what)
    _assert_stats(st, r, what)
    assert c.dense_ops > 0 and c.pull_launches > 0, what
    if not fused:
        assert c.dense_fused_launches == 0, what
    elif name == "ladder_collide":  # ticks whose window holds a group word leave the fused kernel
        assert 0 < c.dense_fused_launches < c.pull_launches, what
    elif lat == L:  # unique ids: every tick fused, the snapshot ticks among them
        assert c.dense_fused_launches == c.pull_launches, what
    else:
        assert c.dense_fused_launches > 0, what


# ---- hop batch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("link", [None, "5mbps"])
@pytest.mark.parametrize("mode", ["csr", "dense"])
def test_hop_batch(gossip, oracle, mode, link):
    # every share runs from its own batched tick; k_snap_count takes per-column masks from the real times
    f = TS._family("ladder")
    ts = R.family_times(f, L)
    eng = _make(gossip, "ladder", L, ts, flags=("F_HOP_BATCH",), link=gossip.LINK_5MBPS if link else None,
                mode=gossip.MODE_DENSE if mode == "dense" else gossip.MODE_CSR)
    try:
        eng.run()
        eng.sync()
        st, c = eng.stats(), eng.counters()
        snaps = [eng.snapshot(k) for k in range(len(ts))]  # (after the complete run)
    finally:
        eng.close()
    r = R.replay(oracle, f, L, "link" if link else "plain")
    what = ("ladder", "hop batch", mode, link)
    _assert_snaps(snaps, r, L, ts, what)
    _assert_stats(st, r, what)
    assert c.pull_launches > 0 and (c.dense_ops > 0) == (mode == "dense"), what


# ---- handshake window -----------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["default", "wide"])
@pytest.mark.parametrize("name", ["ladder", "tail[65]"])
def test_handshake(gossip, oracle, name, path):
    # the snapshots in ticks +0 and +1 fall inside the lost-share window: a share generated there floods
    # nothing, but its id is in processedShares from its generation on
    f = TS._family(name)
    ts = R.family_times(f, L)
    st, c, snaps = _run(gossip, name, L, ts, flags=PATHS[path][0] + ("F_HANDSHAKE",), mode=gossip.MODE_CSR)
    r = R.replay(oracle, f, L, "handshake")
    tick0 = T0 // L
    lost = [R.splits(r, L, T) for T in ts if T // L - tick0 in (0, 1) and T % L]
    assert len(lost) == 2 and all(s[0] == s[1] == 0 for s in lost) and sum(s[2] for s in lost) > 0, lost
    what = (name, "handshake", path)
    _assert_snaps(snaps, r, L, ts, what)
    _assert_stats(st, r, what)
    assert c.pull_launches > 0, what


# ---- row partition ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["csr", "dense", "dense3"])
@pytest.mark.parametrize("name,R_", [("ladder", 2), ("dense_sparse", 3)])
def test_row_partition(gossip, oracle, name, R_, mode):
    # ladder: 633 nodes, blocks of 512 and 121 rows.  Every rank knows the whole schedule (total_gen);
    # it counts the processed ids of its own rows only
    f = TS._family(name)
    ts = R.family_times(f, L)
    opts = () if mode == "csr" else (("dense_fused", 1 if mode == "dense" else 0),)
    m = gossip.MODE_CSR if mode == "csr" else gossip.MODE_DENSE
    ranks = []
    try:
        for k in range(R_):
            ranks.append(_make(gossip, name, L, ts, opts=opts, mode=m, part=(k, R_)))
        gossip.group_run(ranks)
        for e in ranks:
            e.sync()
        got = [e.stats() for e in ranks]
        cs = [e.counters() for e in ranks]
        snaps = [[e.snapshot(k) for k in range(len(ts))] for e in ranks]
    finally:
        for e in ranks:
            e.close()
    r = R.replay(oracle, f, L)
    what = (name, mode, R_)
    want = [R.expected(r, T) for T in ts]
    for k, w in enumerate(want):
        parts = [s[k] for s in snaps]
        assert all(p[0] == w[0] and p[1] == w[1] for p in parts), (what, k, parts, w)
        assert sum(p[2] for p in parts) == w[2], (what, k, parts, w, R.splits(r, L, ts[k]))
    tot = {k: sum(getattr(g, k).astype(np.uint64) for g in got) for k in SUM}
    for k in SUM:
        assert np.array_equal(tot[k], getattr(r, k).astype(np.uint64)), (what, k)
    for k in ("peers", "sockets"):
        assert np.array_equal(getattr(got[0], k), getattr(r, k)), (what, k)
    assert sum(1 for g in got if g.recv.any()) == R_, what  # every rank owns rows that received
    for c in cs:
        assert c.pull_launches > 0, what
        if mode == "dense":
            assert c.dense_fused_launches == c.pull_launches and c.exchange_bytes_sent > 0, what
        if mode == "dense3":
            assert c.dense_fused_launches == 0 and c.dense_ops > 0, what


# ---- share shards -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["hash", "birth_tick"])
def test_share_shards(gossip, oracle, rule):
    f = TS._family("ladder_collide")
    ts = R.family_times(f, L)
    flags = () if rule == "hash" else ("F_SHARD_BY_TICK", TPT)
    parts = [_run(gossip, "ladder_collide", L, ts, flags=flags, shard=(s, 3)) for s in range(3)]
    r = R.replay(oracle, f, L)
    what = ("ladder_collide", "shards", rule)
    for k, w in enumerate(R.expected(r, T) for T in ts):
        got = [p[2][k] for p in parts]
        assert all(g[0] == w[0] for g in got), (what, k)
        assert (sum(g[1] for g in got), sum(g[2] for g in got)) == w[1:], (what, k, got, w)
    for k in SUM:
        total = sum(getattr(p[0], k).astype(np.uint64) for p in parts)
        assert np.array_equal(total, getattr(r, k).astype(np.uint64)), (what, k)
    assert all(int(p[0].gen.sum()) > 0 and p[1].pull_launches > 0 for p in parts), what  # no empty shard


# ---- call rules ---------------------------------------------------------------------------------------------
def test_call_rules(gossip, oracle):
    f = TS._family("ladder")
    ts = R.family_times(f, L)
    tick0 = T0 // L
    mid = next(k for k, T in enumerate(ts) if T // L - tick0 == 3)
    late = next(k for k, T in enumerate(ts) if T // L - tick0 == 20)
    after = next(k for k, T in enumerate(ts) if T > f["t_cut"])
    eng = _make(gossip, "ladder", L, ts)
    try:
        with pytest.raises(gossip.GossipError) as ei:
            eng.add_snapshot(T0)  # (after the schedule)
        assert ei.value.code == gossip.E_STATE
        eng.run(eng.first_tick + 3)  # ticks +0 .. +2 done: tick +3's snapshot is not there yet
        eng.sync()
        for k in (mid, late, after):
            with pytest.raises(gossip.GossipError) as ei:
                eng.snapshot(k)
            assert ei.value.code == gossip.E_STATE, k
        eng.run(eng.first_tick + 4)
        eng.sync()
        early = eng.snapshot(mid)  # its tick has passed: final
        with pytest.raises(gossip.GossipError) as ei:
            eng.snapshot(late)
        assert ei.value.code == gossip.E_STATE
        eng.run()
        eng.sync()
        snaps = [eng.snapshot(k) for k in range(len(ts))]
    finally:
        eng.close()
    assert early == snaps[mid]
    _assert_snaps(snaps, R.replay(oracle, f, L), L, ts, "ladder, read in three steps")
    eng = gossip.Engine(f["n"], L, T0, f["t_cut"])
    try:
        eng.add_snapshot(T0 + 3 * L + 7)
        with pytest.raises(gossip.GossipError) as ei:
            eng.add_snapshot(T0 + 3 * L + L - 1)  # a second one in tick +3
        assert ei.value.code == gossip.E_INVAL
        eng.add_snapshot(T0 + 4 * L)
    finally:
        eng.close()
