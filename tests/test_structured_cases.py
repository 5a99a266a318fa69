"""The structured families (structured.py) on the CPU: ORACLE A pinned against the closed-form BFS
count on every unique-id family, ORACLE B against ORACLE A, the builders' determinism and the
ladder's hub degrees.  The device tests (test_structured_gpu.py) then compare the engine with
ORACLE A on exactly these inputs."""
import numpy as np
import pytest

import structured as S
from cases import L, T0

STATS = ("gen", "recv", "fwd", "sent", "processed", "peers")


def _oracle_a(oracle, f, lat=L):
    return oracle.run_replay(f["n"], lat, T0, f["t_cut"], f["a"], f["b"], f["ev"]["ns"], f["ev"]["node"],
                             f["ev"]["share_id"], trace=True)


# (one variant per family at the 2.3 ms latency: ticks that no birth time is aligned to)
@pytest.mark.parametrize("name", S.UNIQUE_FAMILIES + [f + "@2.3ms" for f in S.UNIQUE_FAMILIES
                                                       if f in S.ODD_LATENCY_FAMILIES])
def test_oracle_a_equals_closed_form(oracle, name):
    name, _, odd = name.partition("@")
    lat = S.L_ODD if odd else L
    f = S.family(name)
    assert f["unique"]
    r = _oracle_a(oracle, f, lat)
    want = S.bfs_reference(f["n"], f["a"], f["b"], f["ev"], lat, f["t_cut"])
    for k in STATS:
        assert np.array_equal(getattr(r, k), want[k]), k
    assert int(r.recv.sum()) > 0 and int(r.gen.sum()) > 0
    tn, ti, tt, th, tv = S.sorted_trace(r.trace)
    wn, wi, wt, wh, wv = S.sorted_trace(want["trace"])
    assert np.array_equal(tn, wn) and np.array_equal(ti, wi)
    assert np.array_equal(tt // lat, wt) and np.array_equal(th, wh) and np.array_equal(tv, wv)


def test_cut_falls_inside_running_floods(oracle):
    # the cut of every family drops arrivals that a later cut would count: the keep masks are at work
    for name in ("tail[65]", "ladder", "long_ring", "dense_sparse"):
        f = S.family(name)
        cut = S.bfs_reference(f["n"], f["a"], f["b"], f["ev"], L, f["t_cut"])
        late = S.bfs_reference(f["n"], f["a"], f["b"], f["ev"], L, f["t_cut"] + 400 * L)
        assert int(cut["recv"].sum()) < int(late["recv"].sum()), name


@pytest.mark.parametrize("name", ["ladder", "ladder_parallel", "long_ring"])
def test_oracle_b_equals_oracle_a(oracle, name):
    f = S.family(name)
    ra = _oracle_a(oracle, f)
    rb = oracle.run_oracle_b(f["n"], L, f["t_cut"], f["a"], f["b"], f["ev"]["ns"], f["ev"]["node"],
                             f["ev"]["share_id"], threads=4)
    for k in STATS + ("sockets",):
        assert np.array_equal(getattr(ra, k), getattr(rb, k)), k


def test_builders_are_deterministic():
    for build in (lambda: S.ring_chords(257, 7), lambda: S.ladder(seed=11), lambda: S.ladder(seed=11, parallel=True),
                  S.components):
        (n1, a1, b1), (n2, a2, b2) = build(), build()
        assert n1 == n2 and np.array_equal(a1, a2) and np.array_equal(b1, b2)
        assert a1.dtype == np.uint32 and np.all(a1 != b1) and int(max(a1.max(), b1.max())) < n1
    assert not np.array_equal(S.ladder(seed=11)[2], S.ladder(seed=12)[2])
    e1, e2 = S.events(633, 40, 6, 12, must_include=range(33)), S.events(633, 40, 6, 12, must_include=range(33))
    assert np.array_equal(e1, e2) and not np.array_equal(e1, S.events(633, 40, 6, 13, must_include=range(33)))


def test_ring_chords_shape():
    assert [x.tolist() for x in S.ring_chords(2, 7)[1:]] == [[0], [1]]
    n, a, b = S.ring_chords(5, 7)           # n <= 2 * chord: the bare ring
    assert sorted(zip(a.tolist(), b.tolist())) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0)]
    n, a, b = S.ring_chords(20, 7)
    assert len(a) == 20 + 7 and (18, 5) in set(zip(a.tolist(), b.tolist()))
    assert len(set(zip(a.tolist(), b.tolist())) | set(zip(b.tolist(), a.tolist()))) == 2 * len(a)  # no parallel keys


def test_events_shape():
    f = S.family("ladder")
    ev = f["ev"]
    assert len(ev) == 40 * 6 and f["unique"]
    assert np.all(np.diff(ev["ns"]) >= 0) and ev["ns"].min() > T0 and ev["ns"].max() < f["t_cut"]
    tick = (ev["ns"] - T0) // L
    assert np.array_equal(np.bincount(tick), np.full(40, 6))
    # at most one birth per node and tick (the engine relies on it), at the finer 2.3 ms ticks too
    for lat in (L, S.L_ODD):
        key = (ev["ns"] // lat) * f["n"] + ev["node"]
        assert len(np.unique(key)) == len(ev)
    assert set(range(len(S.LADDER_DEGS))) <= set(ev["node"].tolist())  # every hub generates
    phase = (ev["ns"] - T0) % L
    by_node = {}
    for v, p in zip(ev["node"].tolist(), phase.tolist()):
        assert by_node.setdefault(v, p) == p and 1 <= p < L
    assert len(set(by_node.values())) == len(by_node)  # distinct phases


@pytest.mark.parametrize("parallel", [False, True])
def test_ladder_hub_degrees(gossip, parallel):
    n, a, b = S.ladder(seed=11, parallel=parallel)
    assert n == len(S.LADDER_DEGS) + S.LADDER_POOL
    topo = gossip.Topology.from_links(n, a, b)
    rp, col, mult = topo.csr()
    peers, sockets = topo.degrees()
    h = len(S.LADDER_DEGS)
    for k, d in enumerate(S.LADDER_DEGS):
        row = col[rp[k]:rp[k + 1]]
        assert len(row) == d and len(np.unique(row)) == d and (d == 0 or row.min() >= h), k
        extra = int((mult[rp[k]:rp[k + 1]] == 2).sum())
        assert peers[k] == d + extra
    hub_links = sum(S.LADDER_DEGS)
    doubled = int((mult[:rp[h]] == 2).sum())
    assert doubled == (hub_links // 2 if parallel else 0)
    # leaves: ring + chords (2..4) plus their hubs
    assert int((rp[h + 1:] - rp[h:-1]).min()) >= 2


@pytest.mark.parametrize("name", S.COLLIDING_FAMILIES)
def test_colliding_families_invariants(oracle, name):
    f = S.family(name)
    ev = f["ev"]
    ids, cnt = np.unique(ev["share_id"], return_counts=True)
    assert not f["unique"] and cnt.max() >= 2 and cnt.max() <= 16  # far below 64 generations per id
    r = _oracle_a(oracle, f)
    assert np.array_equal(r.fwd, r.recv)
    assert np.all(r.processed <= r.gen + r.recv) and np.any(r.processed < r.gen + r.recv)
    assert int(r.recv.sum()) > 0
    if name == "components_collide":
        iso = np.arange(f["n"] - 3, f["n"])
        assert set(iso.tolist()) <= set(ev["node"].tolist())   # generations at peerless nodes ...
        assert not r.gen[iso].any() and not r.processed[iso].any()  # ... are not counted
        # the same id born in both components stays two instances: each flood covers its own ring only
        comp = np.where(ev["node"] < 130, 0, np.where(ev["node"] < 200, 1, 2))
        both = [i for i in ids if {0, 1} <= set(comp[ev["share_id"] == i].tolist())]
        assert both
        tn, ti = r.trace[0], r.trace[1]
        for i in both[:4]:
            nodes = tn[ti == i]
            assert (nodes < 130).any() and ((nodes >= 130) & (nodes < 200)).any()
