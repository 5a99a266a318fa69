"""Structured graphs for the parity tests: chosen degrees, node-count tails and long floods.

G(n,p) graphs have Poisson degrees, a diameter of 8-10 hops and whatever tails their n happens to
leave.  The builders here put nodes on the degree boundaries of the kernels (a ladder of hubs of
degree 0 .. 257 beside degree-2..4 leaves), node counts on the 64 / 256 / 1,024-node boundaries, and
floods of 160 and 280 hops (ring graphs) that widen the live window past one k_pull launch's tiles
and past the fused DENSE kernel's.  Everything is deterministic from a seed; the CPU tests
(test_structured_cases.py) pin ORACLE A on these inputs against a closed-form BFS count, the device
tests (test_structured_gpu.py) compare the engine with ORACLE A.

Plain helpers: link keys (n, a, b) for Topology.from_links, generation events, the closed form.
"""
import numpy as np

from cases import L, T0

GEN_EVENT_DTYPE = np.dtype([("ns", "<i8"), ("node", "<u4"), ("share_id", "<u4")])
L_ODD = 2_300_000  # the 2.3 ms latency of the odd-latency variants: ticks no event time is aligned to

LADDER_DEGS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 23, 24, 25, 31, 32, 33, 47, 48, 49, 63, 64, 65, 71, 72, 73,
               127, 128, 129, 191, 192, 193, 255, 256, 257]
LADDER_POOL = 600
TAIL_N = (2, 63, 64, 65, 127, 129, 257, 513)
DENSE_TAIL_N = (2, 65, 513, 1023, 1025, 2049)


def _keys(pairs):
    k = np.array(pairs, dtype=np.uint32).reshape(-1, 2)
    assert np.all(k[:, 0] != k[:, 1])  # no self-loops
    return k[:, 0].copy(), k[:, 1].copy()


def ring_chords(n, chord):
    """A ring 0-1-...-(n-1)-0 (a single link for n = 2) with a chord (i, i + chord) at every third node."""
    pairs = [(i, i + 1) for i in range(n - 1)]
    if n > 2:
        pairs.append((n - 1, 0))
    if chord > 0 and n > 2 * chord:
        pairs += [(i, (i + chord) % n) for i in range(0, n, 3)]
    a, b = _keys(pairs)
    return n, a, b


def ladder(degs=LADDER_DEGS, pool=LADDER_POOL, seed=1, parallel=False):
    """Hubs 0 .. len(degs)-1, hub k linked to exactly degs[k] distinct leaves of the `pool` leaves
    behind them; the leaves form ring_chords(pool, 41).  parallel: every second hub link is added
    reversed as well (multiplicity 2 on both ends: counted by the degree, not by the distinct-peer CSR)."""
    rng = np.random.default_rng(seed)
    h = len(degs)
    pairs = []
    k = 0
    for hub, d in enumerate(degs):
        for leaf in np.sort(rng.choice(pool, size=d, replace=False)):
            pairs.append((hub, h + int(leaf)))
            if parallel and k % 2 == 1:
                pairs.append((h + int(leaf), hub))
            k += 1
    _, ra, rb = ring_chords(pool, 41)
    a, b = _keys(pairs) if pairs else (np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    return h + pool, np.concatenate([a, ra + h]).astype(np.uint32), np.concatenate([b, rb + h]).astype(np.uint32)


def components(n1=130, n2=70, isolated=3):
    """Two rings with chords of different size side by side, then `isolated` peerless nodes."""
    _, a1, b1 = ring_chords(n1, 7)
    _, a2, b2 = ring_chords(n2, 7)
    return (n1 + n2 + isolated, np.concatenate([a1, a2 + n1]).astype(np.uint32),
            np.concatenate([b1, b2 + n1]).astype(np.uint32))


def gaps(n1=100, empty=130, n2=103):
    """ring_chords(n1, 7), then `empty` peerless nodes, then ring_chords(n2, 7): n = 333.  For the kernels that
    walk 64-node chunks of the flat entry range: the chunk of nodes 128 .. 191 has no entries and starts inside
    a 64-entry word (rowptr & 63 != 0), chunk 64 .. 127 ends in empty rows and chunk 192 .. 255 begins with them."""
    _, a1, b1 = ring_chords(n1, 7)
    _, a2, b2 = ring_chords(n2, 7)
    off = n1 + empty
    return (off + n2, np.concatenate([a1, a2 + off]).astype(np.uint32), np.concatenate([b1, b2 + off]).astype(np.uint32))


# ring_chords(n, 0) at these n: every node has degree 2, so every 64-node chunk starts on a 64-entry word
# boundary (rowptr & 63 == 0) and only the last word of the flat entry range is covered in part
ALIGNED_RING_N = (129, 513)


def aligned_ring(n):
    assert n in ALIGNED_RING_N
    return ring_chords(n, 0)


def events(n, ticks, per_tick, seed, id_mask=0, must_include=()):
    """per_tick distinct nodes generate in each of `ticks` ticks of L = 5 ms after T0 (a node has at
    most one birth per tick), node v always at its own phase in [1, L), all phases distinct; sorted
    by (ns, node); the k-th event's id is (k+1)*7919 mod 2^31 (unique), ANDed with id_mask if given.
    must_include: nodes forced into the first ticks, so that each generates at least once."""
    assert 0 < per_tick <= n < L - 2
    rng = np.random.default_rng(seed)
    stride = (L - 2) // n
    phase = 1 + rng.permutation(n).astype(np.int64) * stride + rng.integers(0, stride, size=n)
    assert phase.min() >= 1 and phase.max() < L and len(np.unique(phase)) == n
    forced = [int(v) for v in must_include]
    assert len(forced) <= ticks * per_tick and len(set(forced)) == len(forced)
    ns, node = [], []
    for t in range(ticks):
        take, forced = forced[:per_tick], forced[per_tick:]
        if len(take) < per_tick:
            rest = np.setdiff1d(np.arange(n), take)
            take = take + [int(v) for v in rng.choice(rest, size=per_tick - len(take), replace=False)]
        for v in take:
            ns.append(T0 + t * L + int(phase[v]))
            node.append(v)
    ns, node = np.array(ns, np.int64), np.array(node, np.uint32)
    o = np.lexsort((node, ns))
    ev = np.empty(len(o), GEN_EVENT_DTYPE)
    ev["ns"], ev["node"] = ns[o], node[o]
    ids = ((np.arange(len(o), dtype=np.int64) + 1) * 7919) % (1 << 31)
    ev["share_id"] = ids & id_mask if id_mask else ids
    return ev


def t_cut_for(ticks):
    """A cut inside the tick after the last birth tick, floods still running: keep masks at work."""
    return T0 + ticks * L + L // 3


def bfs_reference(n, a, b, ev, lat, t_cut):
    """Closed form for unique ids: a share born at (t, s) reaches v != s at t + d(s,v) * lat, and is
    counted there iff that is before t_cut; every first arrival forwards to every peer."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import shortest_path

    assert len(np.unique(ev["share_id"])) == len(ev)
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    peers = (np.bincount(a, minlength=n) + np.bincount(b, minlength=n)).astype(np.uint32)
    adj = coo_matrix((np.ones(2 * len(a), np.int8), (np.concatenate([a, b]), np.concatenate([b, a]))),
                     shape=(n, n)).tocsr()
    srcs, inv = np.unique(ev["node"], return_inverse=True)
    dist = shortest_path(adj, unweighted=True, indices=srcs).reshape(len(srcs), n)
    gen = np.zeros(n, np.uint32)
    recv = np.zeros(n, np.uint32)
    tn, ti, tt, th, tv = [], [], [], [], []
    for k in range(len(ev)):
        t, s, sid = int(ev["ns"][k]), int(ev["node"][k]), int(ev["share_id"][k])
        assert t < t_cut
        if peers[s] == 0:
            continue  # "has no peers to send shares to": not counted, nothing sent
        gen[s] += 1
        tn.append([s]), ti.append([sid]), tt.append([t // lat]), th.append([0]), tv.append([0])
        d = dist[inv[k]]
        v = np.flatnonzero(np.isfinite(d) & (d > 0))
        dv = d[v].astype(np.int64)
        keep = t + dv * lat < t_cut
        v, dv = v[keep], dv[keep]
        recv[v] += 1
        tn.append(v), ti.append(np.full(len(v), sid)), tt.append((t + dv * lat) // lat), th.append(dv)
        tv.append(np.ones(len(v), np.int64))
    cat = lambda xs, dt: np.concatenate([np.asarray(x, np.int64) for x in xs]).astype(dt) if xs else np.zeros(0, dt)
    trace = (cat(tn, np.uint32), cat(ti, np.uint32), cat(tt, np.int64), cat(th, np.uint32), cat(tv, np.uint8))
    return dict(gen=gen, recv=recv, fwd=recv.copy(), processed=gen + recv,
                sent=peers.astype(np.uint64) * (gen + recv).astype(np.uint64), peers=peers, trace=trace)


def sorted_trace(trace):
    """(node, id, tick-or-ns, hop, via) in (node, id) order."""
    node, sid = trace[0], trace[1]
    o = np.lexsort((sid, node))
    return tuple(np.asarray(x)[o] for x in trace)


def family(name):
    """The inputs of one family: dict(n, a, b, ev, t_cut, unique).  Sizes are the smallest that
    still reach the boundary the family exists for."""
    hubs = range(len(LADDER_DEGS))
    if name.startswith("tail[") or name.startswith("dense_tail["):
        n = int(name[name.index("[") + 1:-1])
        g, ev, ticks = ring_chords(n, 7), events(n, 12, min(2, n), 100 + n), 12
    elif name in ("ladder", "ladder_parallel", "ladder_collide"):
        g = ladder(seed=11, parallel=name == "ladder_parallel")
        ev = events(g[0], 40, 6, 12, id_mask=0x3F if name == "ladder_collide" else 0, must_include=hubs)
        ticks = 40
    elif name == "components_collide":
        g = components()
        ev, ticks = events(g[0], 30, 4, 13, id_mask=0x1F, must_include=range(g[0] - 3, g[0])), 30
    elif name == "long_ring":      # 160 hops: with a fresh tile per tick, a window above 2,048 words
        g, ev, ticks = ring_chords(320, 0), events(320, 200, 2, 14), 200
    elif name == "dense_long_ring":  # 280 hops: above the fused DENSE kernel's 4,096 words
        g, ev, ticks = ring_chords(560, 0), events(560, 300, 2, 15), 300
    elif name == "dense_sparse":   # 3 K stages of 1,024 nodes, floods that sit in one or two of them
        g, ev, ticks = ring_chords(2500, 97), events(2500, 30, 4, 16), 30
    else:
        raise KeyError(name)
    n, a, b = g
    t_cut = T0 + 60 * L if name == "ladder_collide" else t_cut_for(ticks)
    return dict(name=name, n=n, a=a, b=b, ev=ev, t_cut=t_cut, unique=len(np.unique(ev["share_id"])) == len(ev))


UNIQUE_FAMILIES = ([f"tail[{n}]" for n in TAIL_N] + ["ladder", "ladder_parallel", "long_ring", "dense_long_ring"] +
                   [f"dense_tail[{n}]" for n in DENSE_TAIL_N if n not in TAIL_N] + ["dense_sparse"])
COLLIDING_FAMILIES = ["ladder_collide", "components_collide"]
# one variant per family runs at the 2.3 ms latency as well
ODD_LATENCY_FAMILIES = ["tail[65]", "tail[513]", "ladder", "ladder_parallel", "ladder_collide", "components_collide",
                        "long_ring", "dense_long_ring", "dense_tail[1025]", "dense_sparse"]
