"""The model of the per-tick thinned peer lists (thinning_ref.py), the parts that need no device: the model
against the library's own host rule functions (gossip.fanout_selected, gossip.fanout_exact_row,
gossip.fault_lost), and the inputs of test_thinning_gpu.py shown not to be vacuous -- on the model alone, per
(graph, mode) pair that file runs, over the ticks it steps.

The case table (GRAPHS, MODES, modes_of, config) is shared with test_thinning_gpu.py.
"""
import functools

import numpy as np
import pytest

import fanout_ref as F
import structured as S
import thinning_ref as TH
from cases import L, T0

FIRST = T0 // L
TICKS = 8                 # the ticks the device test steps and compares: FIRST .. FIRST + 7
ALWAYS = 0xFFFFFFFF
LOSS = 0x33333333         # floor(0.2 * 2^32)
SEED, LOSS_SEED = 44, 11
EXACT_KS = (1, 2, 8, 9, 32)

GRAPHS = ([f"tail[{n}]" for n in S.TAIL_N] + [f"aligned[{n}]" for n in S.ALIGNED_RING_N] + ["ladder", "gaps", "base"])
# every graph runs these; the ladder and gaps() run every mode
COMMON_MODES = ("a1", "d", "e2", "g")
MODES = ("a1", "a3", "b", "c", "c_all_lost", "d") + tuple(f"e{k}" for k in EXACT_KS) + ("f", "f_hubs", "g", "h")


def modes_of(graph):
    if graph == "ladder":
        return MODES
    if graph == "gaps":
        return tuple(m for m in MODES if m != "f_hubs")  # (counts next to the row length: the ladder's hubs)
    return COMMON_MODES


def grids_of(graph):
    """fanout_grid values: 1 (one block strides every chunk) and 0 (the default grid)."""
    return (0, 1) if graph.startswith("tail[") or graph in ("ladder", "gaps") else (0,)


@functools.lru_cache(maxsize=None)
def topology(gossip, graph):
    if graph == "base":
        return gossip.Topology.gnp(1000, 8.0 / 999.0, 7, gossip.TOPO_SKIP)
    if graph.startswith("tail["):
        n, a, b = S.ring_chords(int(graph[5:-1]), 7)
    elif graph.startswith("aligned["):
        n, a, b = S.aligned_ring(int(graph[8:-1]))
    elif graph == "ladder":
        n, a, b = S.ladder(seed=11, parallel=True)
    elif graph == "gaps":
        n, a, b = S.gaps()
    else:
        raise KeyError(graph)
    return gossip.Topology.from_links(n, a, b)


def events_of(n):
    """A three-tick schedule."""
    return S.events(n, 3, min(2, n), 200 + n)


def outages_of(n):
    """Every third node is down once: from FIRST + 1 .. 4 for 1 .. 3 ticks, inside the stepped ticks."""
    return tuple((v, FIRST + 1 + v % 4, FIRST + 2 + v % 4 + v % 3) for v in range(0, n, 3))


def config(mode, n, peers):
    """The configuration of a mode on a graph of n nodes with `peers` out-copies per node:
    dict(thr, k, seed, outages, loss_thr, loss_seed, rounds, fanout) -- thr / k as thinning_ref.Thinning takes
    them; fanout: the k of set_fanout where thr are its thresholds (the engine derives them itself)."""
    peers = np.asarray(peers, np.int64)
    c = dict(thr=None, k=None, seed=SEED, outages=(), loss_thr=0, loss_seed=LOSS_SEED, rounds=1, fanout=None)
    faults = dict(outages=outages_of(n), loss_thr=LOSS)
    if mode in ("a1", "a3", "d"):
        c["fanout"] = {"a1": 1, "a3": 3, "d": 3}[mode]
        c["thr"] = F.thresholds(c["fanout"], peers)
        if mode == "d":
            c.update(faults)
    elif mode == "b":
        vals = np.array([0, 1, 1 << 31, 0xFFFFFFFE, ALWAYS], np.uint32)
        c["thr"] = vals[np.random.default_rng(31).integers(0, 5, size=n)]
    elif mode == "c":
        c.update(faults)
    elif mode == "c_all_lost":
        c.update(outages=outages_of(n), loss_thr=ALWAYS)
    elif mode[0] == "e":
        c["k"] = np.full(n, int(mode[1:]), np.uint32)
    elif mode == "f":
        rng = np.random.default_rng(32)
        kk = rng.integers(1, 7, size=n).astype(np.uint32)
        kk[rng.choice(n, max(1, n // 7), replace=False)] = 0  # silent nodes
        c["k"] = kk
    elif mode == "f_hubs":
        # k[u] = D - 1, D, D + 1 by u mod 3 at every node of up to 33 out-copies (a node that must select takes at
        # most 32), 32 at the hubs above
        c["k"] = np.where(peers <= 33, np.clip(peers + np.arange(n) % 3 - 1, 0, 32), 32).astype(np.uint32)
    elif mode in ("g", "h"):
        c["k"] = np.full(n, 2, np.uint32)
        c.update(faults)
        c["rounds"] = 3 if mode == "h" else 1
    else:
        raise KeyError(mode)
    return c


@functools.lru_cache(maxsize=None)
def thinning(gossip, graph, mode):
    """The model of (graph, mode).  Mode h is g with rounds, which do not enter the selection: g's model."""
    if mode == "h":
        return thinning(gossip, graph, "g")
    topo = topology(gossip, graph)
    a, b = topo.links()
    c = config(mode, topo.num_nodes, topo.degrees()[0])
    th = TH.Thinning(topo.num_nodes, a, b, thr=c["thr"], k=c["k"], seed=c["seed"], outages=c["outages"], loss_thr=c["loss_thr"],
                     loss_seed=c["loss_seed"])
    assert np.array_equal(th.peers, topo.degrees()[0])
    return th


PAIRS = [(g, m) for g in GRAPHS for m in modes_of(g)]


# ---- the model against the library's host rule functions -----------------------------------------------
@pytest.mark.parametrize("graph", ["ladder", "gaps"])
@pytest.mark.parametrize("mode", ["b", "d", "e2", "e32", "f", "g"])
def test_reference_against_the_host_rule_functions(gossip, graph, mode):
    th = thinning(gossip, graph, mode)
    n, u, v, c = th.n, th.u, th.v, th.c
    if graph == "ladder":
        assert int(c.max()) == 1  # parallel links: copies 0 and 1
    for T in (FIRST, FIRST + 1, FIRST + 5):
        r = th.tick(T)
        if th.thr is not None:
            lib = np.array([gossip.fanout_selected(th.seed, int(u[i]), int(v[i]), int(c[i]), T, int(th.thr[u[i]])) for i in range(len(u))])
            assert np.array_equal(lib, r["made"]), (graph, mode, T)
        else:
            made = np.zeros(len(u), bool)
            for x in range(n):
                lo, hi = int(th.rp[x]), int(th.rp[x + 1])
                sel, w = gossip.fanout_exact_row(th.seed, x, v[lo:hi], c[lo:hi], int(th.k[x]), T, draws=True)
                made[lo:hi] = sel
                if th.k[x] > 0:  # the k-th smallest draw is the bound of a node that selects
                    want = np.sort(w)[th.k[x] - 1] if hi - lo > th.k[x] else TH.ALL
                    assert r["bound_mask"][x] and int(r["bound"][x]) == int(want), (graph, mode, T, x)
                else:
                    assert not r["bound_mask"][x]
            assert np.array_equal(made, r["made"]), (graph, mode, T)
        if th.loss_thr:
            lib = np.array([gossip.fault_lost(th.loss_seed, int(u[i]), int(v[i]), int(c[i]), T, th.loss_thr) for i in range(len(u))])
            assert np.array_equal(lib, r["lost"]), (graph, mode, T)
        # the lists follow from the three rules: entry by entry, in plain Python
        dn = {int(o[0]) for o in th.outages if o[1] <= T + 1 < o[2]}
        keep = sorted({(int(v[i]), int(u[i])) for i in range(len(u))
                       if r["made"][i] and not r["lost"][i] and int(v[i]) not in dn})
        rows = np.repeat(np.arange(n), np.diff(r["row_ptr"]))
        assert keep == list(zip(rows.tolist(), r["col"].tolist())), (graph, mode, T)
        assert r["selected_in"] == len(keep) and r["selected_out"] == int(r["made"].sum())


def test_fault_counts_are_those_of_faults_ref(gossip):
    import faults_ref as R
    for graph in ("ladder", "gaps"):
        for mode in ("c", "d"):
            th = thinning(gossip, graph, mode)
            topo = topology(gossip, graph)
            a, b = topo.links()
            thr = th.thr if th.thr is not None else np.full(th.n, ALWAYS, np.uint64)
            ticks = range(FIRST, FIRST + TICKS)
            want = R.fault_counts(th.n, a, b, thr, th.seed, th.outages, th.loss_thr, th.loss_seed, ticks)
            t = th.totals(ticks)
            assert (t["down_node_ticks"], t["lost_copies"], t["down_copies"]) == want, (graph, mode)


# ---- the inputs are not vacuous ---------------------------------------------------------------------------
def _row_outcomes(th, ticks):
    """Over the ticks: is some populated row kept whole, some emptied, some thinned in part?"""
    full = np.diff(th.full_row_ptr)
    whole = emptied = part = False
    for T in ticks:
        kept = np.diff(th.tick(T)["row_ptr"])
        pop = full > 0
        whole |= bool((pop & (kept == full)).any())
        emptied |= bool((pop & (kept == 0)).any())
        part |= bool(((kept > 0) & (kept < full)).any())
    return whole, emptied, part


def _can_drop(th):
    """Can the configuration drop a copy at all?  (Not where every sender sends every copy and nothing is lost.)"""
    if th.faults:
        return True
    if th.k is not None:
        return bool(((th.k == 0) | (np.diff(th.rp) > th.k)).any())
    return th.thr is not None and bool((th.thr != ALWAYS).any())


# the pairs that keep every list whole by construction: exact counts at or above every row length, no faults
FLOODS = {("aligned[129]", "e2"), ("aligned[513]", "e2"), ("tail[2]", "a1"), ("tail[2]", "e2"),
          ("gaps", "e8"), ("gaps", "e9"), ("gaps", "e32")}


# the pairs in which every populated row has a peer that sends every copy: at k = 3 the nodes of gaps() with up to
# three peers (all but the few where two chords meet) send to all of them; at k = 32 and in f_hubs only the ladder's
# hubs select, and every row has a leaf of the ring among its peers
NEVER_EMPTIED = {("gaps", "a3"), ("ladder", "e32"), ("ladder", "f_hubs")}


@pytest.mark.parametrize("graph,mode", PAIRS, ids=[f"{g}-{m}" for g, m in PAIRS])
def test_rows_whole_emptied_and_thinned_in_part(gossip, graph, mode):
    th = thinning(gossip, graph, mode)
    ticks = range(FIRST, FIRST + TICKS)
    assert (not _can_drop(th)) == ((graph, mode) in FLOODS), (graph, mode)
    whole, emptied, part = _row_outcomes(th, ticks)
    if (graph, mode) in FLOODS:
        assert whole and not emptied and not part
    elif mode == "c_all_lost":  # every list is empty: row_ptr all zeros
        assert all(not th.tick(T)["row_ptr"].any() for T in ticks) and emptied
    elif graph == "tail[2]":    # two rows of one entry: whole or emptied
        assert whole and emptied
    elif (graph, mode) in NEVER_EMPTIED:
        assert whole and part and not emptied
    else:
        assert whole and emptied and part, (graph, mode, whole, emptied, part)


def _hub_boundaries_differ(th, ticks):
    """Per hub of 65 or more distinct peers: is there a tick in which the two entries on either side of one of the
    row's 64-entry word boundaries (flat positions j - 1 and j, j % 64 == 0, in the model's own CSR: rows in order,
    peers ascending) differ in outcome?"""
    rp = th.full_row_ptr
    hubs = np.flatnonzero(np.diff(rp) >= 65)
    ok = np.zeros(len(hubs), bool)
    for T in ticks:
        s = th.tick(T)["survives"]
        for i, h in enumerate(hubs):
            j = np.arange((rp[h] // 64 + 1) * 64, rp[h + 1], 64)
            j = j[j > rp[h]]
            ok[i] |= bool((s[j - 1] != s[j]).any())
    return hubs, ok


# What a hub's row keeps is decided by its peers, the leaves (3 .. 20 out-copies, most of them 5 .. 12).  The modes
# below are on the ladder for the out side -- the hubs' own selection: k_fanout_kth at 8, 9 and 32 slots, counts next
# to the row length, the bounds -- and their leaves drop little or nothing:
#   e32      no leaf selects: the hubs' rows stay whole
#   e8, e9   only the leaves of 9 / 10 or more out-copies select, and drop one copy in nine or so: the hubs of two or
#            more word boundaries (127 peers and up) are asked for
#   f_hubs   a leaf sends D - 1, D or D + 1 of its D copies: some hub is asked for
SPARSE_HUB_MODES = {"e8": 127, "e9": 127, "f_hubs": None, "e32": None}


@pytest.mark.parametrize("mode", modes_of("ladder"))
def test_ladder_hub_rows_differ_across_word_boundaries(gossip, mode):
    th = thinning(gossip, "ladder", mode)
    hubs, ok = _hub_boundaries_differ(th, range(FIRST, FIRST + TICKS))
    width = np.diff(th.full_row_ptr)[hubs]
    assert width.tolist() == [d for d in S.LADDER_DEGS if d >= 65]
    if mode == "c_all_lost":
        assert not ok.any()
    elif mode == "e32":
        D = np.diff(th.rp)
        leaves = np.arange(len(S.LADDER_DEGS), th.n)
        assert (D[leaves] <= th.k[leaves]).all() and not ok.any()
    elif mode in SPARSE_HUB_MODES:
        at_least = SPARSE_HUB_MODES[mode]
        assert ok.any() and (at_least is None or ok[width >= at_least].all()), (mode, hubs[~ok].tolist())
    else:
        assert ok.all(), (mode, hubs[~ok].tolist())


def test_exact_counts_have_selecting_nodes(gossip):
    for k in EXACT_KS:
        th = thinning(gossip, "ladder", f"e{k}")
        D = np.diff(th.rp)
        sel = np.flatnonzero(D > k)
        assert len(sel) > 0, k
        if k == 32:  # the hubs of 33 or more peers, and no leaf
            assert sel.max() < len(S.LADDER_DEGS) and {int(x) for x in D[sel]} >= {49, 257 + 128}
    th = thinning(gossip, "ladder", "f_hubs")
    D = np.diff(th.rp)
    for d in (-1, 0, 1):
        assert ((th.k == D + d) & (D > 1)).any(), d
    assert ((th.k == 32) & (D > 64)).any()
    for graph in ("ladder", "gaps"):
        th = thinning(gossip, graph, "f")
        D = np.diff(th.rp)
        assert ((th.k == 0) & (D > 0)).any() and ((th.k > 0) & (D > th.k)).any() and ((th.k > 0) & (D <= th.k) & (D > 0)).any()
    for graph in GRAPHS:  # k = 2 selects on every graph but the degree-2 rings and the single link
        th = thinning(gossip, graph, "g")
        assert (np.diff(th.rp) > 2).any() == (not graph.startswith("aligned[") and graph != "tail[2]"), graph


@pytest.mark.parametrize("graph", GRAPHS)
def test_faults_drop_by_loss_alone_and_by_outage_alone(gossip, graph):
    ticks = range(FIRST, FIRST + TICKS)
    for mode in [m for m in ("c", "d", "g") if m in modes_of(graph)]:
        th = thinning(gossip, graph, mode)
        by_loss = by_outage = False
        for T in ticks:
            r = th.tick(T)
            key = th.v.astype(np.int64) * th.n + th.u  # the entry (row v, peer u) of a copy
            down_v = r["down"][th.v]
            # by the outage alone: a copy that was made and not lost, into a row that is down in T + 1
            by_outage |= bool((r["made"] & ~r["lost"] & down_v).any())
            # by loss alone: an entry of an up row with a made copy, every made copy of it lost
            by_loss |= len(np.setdiff1d(np.unique(key[r["made"] & ~down_v]), np.unique(key[r["arrives"]]))) > 0
        assert by_loss and by_outage, (graph, mode)
    n = topology(gossip, graph).num_nodes
    out = outages_of(n)
    assert all(FIRST < o[1] < o[2] <= FIRST + TICKS for o in out)  # every outage begins and ends inside the stepped ticks
    th = thinning(gossip, graph, "g")
    mid = np.any([th.down(T) for T in range(FIRST + 1, FIRST + TICKS)], axis=0)
    assert (mid & ~th.down(FIRST) & ~th.down(FIRST + TICKS)).any()  # some node goes down and comes back


def test_structured_row_pointers(gossip):
    # gaps(): chunk 128 .. 191 has no entries and starts inside a word; chunk 64 .. 127 ends in empty rows, chunk
    # 192 .. 255 begins with them
    th = thinning(gossip, "gaps", "a1")
    rp, csr = th.full_row_ptr, topology(gossip, "gaps").csr()[0]
    assert np.array_equal(rp, np.asarray(csr, np.int64))  # the engine's row pointers are these
    assert th.n == 333 and rp[128] == rp[192] and rp[128] & 63 != 0
    assert rp[127] == rp[128] and rp[64] < rp[100] == rp[128]          # ends in empty rows
    assert rp[192] == rp[193] and rp[230] == rp[192] and rp[231] > rp[230] and rp[256] > rp[192]  # begins with them
    # the aligned rings: degree 2 everywhere, every chunk starts on a word boundary
    for n in S.ALIGNED_RING_N:
        th = thinning(gossip, f"aligned[{n}]", "a1")
        rp = th.full_row_ptr
        assert np.array_equal(rp, np.asarray(topology(gossip, f"aligned[{n}]").csr()[0], np.int64))
        assert np.all(np.diff(rp) == 2) and np.all(rp[0:n:64] & 63 == 0) and rp[n] & 63 != 0
    # the tails with chords are not aligned: some chunk starts inside a word
    th = thinning(gossip, "tail[513]", "a1")
    assert (th.full_row_ptr[0:513:64] & 63 != 0).any()
