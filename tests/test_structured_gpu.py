"""Parity of the HIP engine with ORACLE A on the structured families of structured.py: nodes on the
kernels' degree boundaries (ladder), node counts on the 64 / 256 / 1,024-node boundaries (tails),
floods of 160 and 280 hops (windows above one k_pull launch's 2,048 words and above the fused DENSE
kernel's 4,096), a DENSE run with empty 1,024-node stages, colliding ids beside overflowed hubs.

Every run compares the seven per-node counters and the first-contact trace (node, id, tick, hop,
via) with ORACLE A bit for bit, one engine per (case, path), and asserts from the engine's counters
that the path it names really ran.  test_structured_cases.py pins ORACLE A on the same inputs
against the closed-form BFS count.
"""
import functools

import numpy as np
import pytest

import structured as S
from cases import L, T0

pytestmark = pytest.mark.gpu

STATS = ("gen", "recv", "fwd", "sent", "processed", "peers", "sockets")
TPT = "F_TILE_PER_TICK"
# the launch ledger's kernel ids and k_pull template flags (include/gossip.h)
K_PULL, K_PULL_YOUNG = 0, 1
PULL_NT, PULL_SP, PULL_PUSH = 1, 2, 4

# CSR paths: (flag names, options)
PATHS = {
    "default": ((), ()),
    "wide": ((TPT,), ()),
    "wide_nt_push": ((TPT,), (("pull_nt", 1), ("pull_push", 1))),
    "push_off": ((TPT,), (("pull_push", 0), ("pull_nt", 1))),  # the non-PUSH SP kernel, ragged last chunk
    "no_tile_lists": ((), (("pull_tiles", 0),)),
    "dense_rows": ((), (("dense_rows", 1),)),
    "dense_rows_nosat": ((), (("dense_rows", 1), ("pull_sat", 0))),
    "noskip": (("F_NOSKIP",), ()),
    "young": ((TPT,), (("young", 1), ("young_nt", 1), ("young_skip", 1))),
    "young_tight": ((TPT,), (("young", 1), ("young_cap", 3), ("young_list_cap", 8), ("young_age", 6),
                             ("young_skip", 1))),
    # every host heuristic decides from a BFS layer model that is wrong for these graphs
    "young_auto": ((), (("young", 1), ("young_skip", -1), ("pull_push", -1), ("dense_rows", -1))),
}
COLLIDE_PATHS = ("default", "wide_nt_push", "young", "young_tight", "dense_rows")


@functools.lru_cache(maxsize=None)
def _family(name):
    return S.family(name)


_topos = {}


def _topo(gossip, name):
    if name not in _topos:
        f = _family(name)
        _topos[name] = gossip.Topology.from_links(f["n"], f["a"], f["b"])
    return _topos[name]


def counters_with_ledger(eng):
    """The engine's counters with its launch ledger riding along as .launches (what _ran reads)."""
    c = eng.counters()
    c.launches = eng.launches()
    return c


def _engine_run(gossip, name, flags=(), opts=(), lat=L, mode=None, graph="topology", probe=None):
    """One engine over the family's inputs: (stats, counters, trace); with probe = k the run stops after
    k ticks and reads the counters there as well (the "last tick" counters while floods still run)."""
    f = _family(name)
    fl = gossip.F_TRACE
    for x in flags:
        fl |= getattr(gossip, x)
    eng = gossip.Engine(f["n"], lat, T0, f["t_cut"], flags=fl, mode=gossip.MODE_AUTO if mode is None else mode)
    try:
        for k, v in opts:
            eng.set_option(k, v)
        if graph == "topology":
            eng.set_topology(_topo(gossip, name))
        else:
            eng.set_graph(*graph)
        eng.set_schedule(f["ev"])
        if probe is not None:
            eng.run(eng.first_tick + probe)
            eng.sync()
            mid = eng.counters()
        eng.run()
        eng.sync()
        out = eng.stats(), counters_with_ledger(eng), eng.trace()
        return out if probe is None else out + (mid,)
    finally:
        eng.close()


def _assert_parity(oracle, name, lat, st, tr, what):
    assert_parity_inputs(oracle, _family(name), lat, st, tr, what)


def assert_parity_inputs(oracle, f, lat, st, tr, what):
    """The engine's counters and first-contact trace against ORACLE A on the inputs f (n, a, b, ev, t_cut)."""
    r = oracle.run_replay(f["n"], lat, T0, f["t_cut"], f["a"], f["b"], f["ev"]["ns"], f["ev"]["node"],
                          f["ev"]["share_id"], trace=True)
    for k in STATS:
        got, want = getattr(st, k), getattr(r, k)
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{what}: {k} differs at {len(bad)} nodes, first {bad[:8].tolist()}: "
                                 f"engine {got[bad[:8]].tolist()} oracle {want[bad[:8]].tolist()}")
    node, sid, tick, hop, via = S.sorted_trace(tr)
    tn, ti, tt, th, tv = S.sorted_trace(r.trace)
    assert np.array_equal(node, tn) and np.array_equal(sid, ti), what
    assert np.array_equal(tick, tt // lat), what   # first-contact tick
    assert np.array_equal(hop, th), what           # first-arrival hop count
    assert np.array_equal(via, tv), what
    assert int(r.recv.sum()) > 0


def _csr(gossip, oracle, name, path, lat=L):
    flags, opts = PATHS[path]
    st, c, tr = _engine_run(gossip, name, flags, opts, lat)
    _assert_parity(oracle, name, lat, st, tr, (name, path, lat))
    _ran(path, c, name)
    return c


def _ran(path, c, name):
    """The path's own switches took effect in the launches (what every case of the path must show)."""
    what = (name, path)
    assert c.pull_launches > 0 and c.ticks > 0, what
    if path in ("default", "wide", "dense_rows", "dense_rows_nosat"):
        assert c.pull_tiles == 1 and c.pull_nt == 0, what
        assert c.pull_sat == (0 if path == "dense_rows_nosat" else 1), what
    if path in ("wide_nt_push", "push_off"):
        assert c.pull_nt == 1 and c.pull_tiles == 1, what
    if path == "push_off":
        assert c.pull_push_tiles == 0 and c.pull_pushw_tiles == 0 and c.pull_marks == 0, what
    if path in ("no_tile_lists", "noskip"):  # passes over consecutive words: no lists, no saturation bits
        assert c.pull_tiles == 0 and c.pull_sat == 0 and c.pull_sat_skips == 0, what
    if path.startswith("young"):
        assert c.young_launches > 0 and c.young_slot_lines > 0, what
    if path in ("young", "young_tight"):
        assert c.young_skip_ticks > 0, what
    else:
        assert path.startswith("young") or c.young_launches == 0, what
    # ... and in the launch ledger: the k_pull instantiations that ran, from their launch sites
    pulls = [r for r in c.launches if r.kernel == K_PULL]
    assert pulls and sum(r.launches for r in pulls) >= c.pull_launches, what  # (pull_launches: since reset)
    sp = [r for r in pulls if r.flags & PULL_SP]
    assert all((r.lpw, r.epn) == (32, 1) for r in sp), what
    if path in ("default", "wide", "dense_rows", "dense_rows_nosat"):
        assert not any(r.flags & PULL_NT for r in pulls), what
    if path in ("wide_nt_push", "push_off"):  # pull_nt 1: every kernel that has a non-temporal form ran it
        assert all(r.flags & PULL_NT for r in pulls if r.epn == 1 and r.lpw >= 16), what
    if path == "push_off":  # "the non-PUSH SP kernel": an SP instantiation ran, and none with push marks
        assert sp and not any(r.flags & PULL_PUSH for r in pulls), what
    if path in ("no_tile_lists", "noskip", "dense_rows_nosat"):  # no saturation words: no SP instantiation
        assert not sp, what
    young = [r for r in c.launches if r.kernel == K_PULL_YOUNG]
    assert sum(r.launches for r in young) >= c.young_launches and bool(young) == path.startswith("young"), what


def _ran_ladder(path, c, name, dense_tiles=None):
    what = (name, path)
    if path == "wide":
        assert c.words_hw > 64 and c.pull_lpw == 32, what
    if path == "wide_nt_push":
        assert c.pull_lpw == 32 and c.pull_marks > 0 and c.pull_push_tiles > 0, what
    if path == "push_off":
        assert c.words_hw > 64 and c.pull_lpw == 32, what
    if path in ("dense_rows", "dense_rows_nosat"):
        assert (c.pull_dense_tiles if dense_tiles is None else dense_tiles) > 0, what
    if path in ("young", "young_tight"):
        assert c.young_idle_ticks > 0, what
    if path == "young_tight":  # overflowed slots and lists at hubs beside roomy leaves
        assert c.young_fallback_rows > 0 and c.young_seen_reads > 0, what


# ---- the degree ladder -------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
def test_ladder(gossip, oracle, path):
    _ran_ladder(path, _csr(gossip, oracle, "ladder", path), "ladder")


@pytest.mark.parametrize("path", list(PATHS))
def test_ladder_odd_latency(gossip, oracle, path):
    # 2.3 ms ticks: more ticks per flood, and a cut that falls inside a tick for every birth phase
    _ran_ladder(path, _csr(gossip, oracle, "ladder", path, lat=S.L_ODD), "ladder@2.3ms")


@pytest.mark.parametrize("path", COLLIDE_PATHS)
@pytest.mark.parametrize("name", ["ladder_parallel", "ladder_collide", "components_collide"])
def test_ladder_variants_and_components(gossip, oracle, name, path):
    if name == "ladder_collide" and path == "dense_rows":
        # the cut at T0 + 60 L comes 20 ticks after the last birth: the floods are over, and the last
        # tick reads no tile at all -- the dense-row tiles of a tick are read after 20 of the 40 birth ticks
        flags, opts = PATHS[path]
        st, c, tr, mid = _engine_run(gossip, name, flags, opts, probe=20)
        _assert_parity(oracle, name, L, st, tr, (name, path, "two runs"))
        _ran(path, c, name)
        _ran_ladder(path, c, name, dense_tiles=mid.pull_dense_tiles)
        return
    c = _csr(gossip, oracle, name, path)
    if name != "components_collide":
        _ran_ladder(path, c, name)


@pytest.mark.parametrize("name,path", [("ladder_parallel", "dense_rows"), ("ladder_collide", "wide_nt_push"),
                                       ("components_collide", "young_tight"), ("tail[65]", "push_off"),
                                       ("tail[513]", "young"), ("long_ring", "wide")])
def test_odd_latency_variants(gossip, oracle, name, path):
    # one variant per family at 2.3 ms ticks (the ladder's: test_ladder_odd_latency)
    c = _csr(gossip, oracle, name, path, lat=S.L_ODD)
    if name.startswith("ladder"):
        _ran_ladder(path, c, name)


# ---- node-count tails --------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
def test_tails(gossip, oracle, path):
    seen = {}
    for n in S.TAIL_N:
        c = _csr(gossip, oracle, f"tail[{n}]", path)
        seen[n] = (c.words_hw, c.pull_lpw)
    if path in ("wide", "wide_nt_push", "push_off"):
        # A fresh 16-word tile per tick.  n >= 63: floods of 5 hops and more hold 12 tiles, a window of
        # 192 words, and k_pull<32, 1> (the wide-window kernel) serves it.  n = 2: a flood is one hop, the
        # window stops at 3 tiles = 48 words and never reaches 64 -- 32 word-lanes cover it in one pass,
        # which is what pull_lpw == 32 says there.
        for n, (hw, lpw) in seen.items():
            assert lpw == 32 and (hw > 64 if n > 2 else 16 < hw <= 64), (path, n, hw, lpw)
    if path in ("default", "no_tile_lists", "dense_rows", "dense_rows_nosat", "noskip", "young_auto"):
        assert all(hw == 16 and lpw == 8 for hw, lpw in seen.values()), (path, seen)  # one packed tile


# ---- long floods: windows above one k_pull launch ------------------------------------------------
@pytest.mark.parametrize("path", ["wide", "wide_nt_push", "no_tile_lists", "young"])
def test_long_ring(gossip, oracle, path):
    # 160 hops, a fresh tile every tick: 200 ticks x 2 births (final values) hold a window above
    # 2,048 words, so a tick is several k_pull launches (wb > 0, pt_off[li]) and ntw >= 3
    flags, opts = PATHS[path]
    flags = tuple(set(flags) | {TPT})
    st, c, tr = _engine_run(gossip, "long_ring", flags, opts)
    _assert_parity(oracle, "long_ring", L, st, tr, ("long_ring", path))
    _ran(path, c, "long_ring")
    assert c.words_hw > 2048, c.words_hw  # (a tick launches k_pull once per 2,048 words of the window)
    if path in ("wide", "wide_nt_push"):
        assert c.pull_lpw == 32
    if path == "wide_nt_push":
        assert c.pull_marks > 0 and c.pull_push_tiles > 0
    if path == "young":
        assert c.young_idle_ticks > 0


# ---- DENSE mode --------------------------------------------------------------------------------
def _dense(gossip, oracle, name, fused, flags=(), lat=L):
    st, c, tr = _engine_run(gossip, name, flags, (("dense_fused", 1 if fused else 0),), lat, mode=gossip.MODE_DENSE)
    _assert_parity(oracle, name, lat, st, tr, (name, "dense", fused))
    assert c.dense_ops > 0 and c.pull_launches > 0, name
    if not fused:
        assert c.dense_fused_launches == 0, name
    return st, c, tr


def _same(x, y, what):
    (sx, _, tx), (sy, _, ty) = x, y
    for k in STATS:
        assert np.array_equal(getattr(sx, k), getattr(sy, k)), (what, k)
    for p, q in zip(S.sorted_trace(tx), S.sorted_trace(ty)):
        assert np.array_equal(p, q), what


@pytest.mark.parametrize("fused", [1, 0])
def test_dense_tails(gossip, oracle, fused):
    for n in S.DENSE_TAIL_N:
        st, c, tr = _dense(gossip, oracle, f"dense_tail[{n}]", fused)
        if fused:  # unique ids, one tile: every tick fused
            assert c.dense_fused_launches == c.pull_launches, n


@pytest.mark.parametrize("rounds", [None, "0"])
@pytest.mark.parametrize("fused", [1, 0])
def test_dense_sparse(gossip, oracle, monkeypatch, fused, rounds):
    # ring_chords(2500, 97): 3 K stages of 1,024 nodes, and floods that sit in one or two of them for
    # their first hops -- the stage masks skip the empty ones (G(n,p) leaves none empty after hop 1)
    if rounds is not None:
        monkeypatch.setenv("GOSSIP_DENSE_ROUNDS", rounds)  # every live tile through the split-tile tail
    st, c, tr = _dense(gossip, oracle, "dense_sparse", fused)
    # n_pad = 3,072: 12 row blocks of 256 nodes, 3 K stages.  dense_ops counts (row block, column tile,
    # stage) units computed; a live 256-share column tile costs all 12 x 3 units unless a stage is skipped.
    mb, nst = 12, 3
    units, rem = divmod(c.dense_ops, 2 * 256 * 256 * 1024)
    assert rem == 0 and units > 0 and c.words_hw == 16
    if fused:
        # k_dense_fused reports the column tiles it computes nothing for, 12 row blocks each; every tick
        # covers the one packed tile's 4 column tiles (words_hw 16 from the first launch on)
        assert c.dense_fused_launches == c.pull_launches
        dead, rem = divmod(c.dense_tiles_skipped, mb)
        assert rem == 0
        live = 4 * c.pull_launches - dead
        assert 0 < units < mb * nst * live, (units, live)  # the stage masks skipped empty stages
    else:
        # k_dense_bits skips the stages whose frontier columns it finds empty: without any skipped the
        # units of a run are a multiple of 12 x 3
        assert units % (mb * nst) != 0, units


@pytest.mark.parametrize("name", ["dense_tail[1025]", "dense_sparse", "dense_long_ring"])
def test_dense_odd_latency_variants(gossip, oracle, name):
    flags = (TPT,) if name == "dense_long_ring" else ()
    f = _dense(gossip, oracle, name, 1, flags=flags, lat=S.L_ODD)
    u = _dense(gossip, oracle, name, 0, flags=flags, lat=S.L_ODD)
    assert f[1].dense_fused_launches > 0
    _same(f, u, (name, "2.3 ms, fused vs three-kernel"))


@pytest.mark.parametrize("fused", [1, 0])
def test_dense_ladder(gossip, oracle, fused):
    st, c, tr = _dense(gossip, oracle, "ladder", fused)
    if fused:
        assert c.dense_fused_launches == c.pull_launches


def test_dense_ladder_collide(gossip, oracle):
    # id groups: ticks whose window holds a group word leave the fused kernel
    f = _dense(gossip, oracle, "ladder_collide", 1)
    u = _dense(gossip, oracle, "ladder_collide", 0)
    assert 0 < f[1].dense_fused_launches < f[1].pull_launches
    _same(f, u, "ladder_collide fused vs three-kernel")


def test_dense_long_ring(gossip, oracle):
    # 280 hops, a fresh tile per tick, 300 ticks x 2 births (final values): the run starts fused and
    # leaves the fused kernel when the window outgrows its 4,096 words, then comes back to it
    f = _dense(gossip, oracle, "dense_long_ring", 1, flags=(TPT,))
    u = _dense(gossip, oracle, "dense_long_ring", 0, flags=(TPT,))
    assert f[1].words_hw > 4096 and u[1].words_hw > 4096
    assert 0 < f[1].dense_fused_launches < f[1].pull_launches
    _same(f, u, "dense_long_ring fused vs three-kernel")


# ---- gossip_engine_set_graph: a symmetric CSR runs, an asymmetric one is refused ------------------
def test_set_graph_symmetric_csr_equals_topology(gossip, oracle):
    rp, col, mult = _topo(gossip, "ladder_parallel").csr()
    assert (mult == 2).any()
    a = _engine_run(gossip, "ladder_parallel")
    b = _engine_run(gossip, "ladder_parallel", graph=(rp, col, mult))
    _same(a, b, "set_graph vs set_topology")
    _assert_parity(oracle, "ladder_parallel", L, b[0], b[2], "set_graph")


def test_set_graph_refuses_asymmetric_csr(gossip):
    f = _family("ladder_parallel")
    rp, col, mult = _topo(gossip, "ladder_parallel").csr()
    hub = len(S.LADDER_DEGS) - 1          # the degree-257 hub loses its first peer; the peer keeps the hub
    j = int(rp[hub])
    leaf = int(col[j])
    rp2 = rp.copy()
    rp2[hub + 1:] -= 1
    eng = gossip.Engine(f["n"], L, T0, f["t_cut"])
    try:
        with pytest.raises(gossip.GossipError) as ei:
            eng.set_graph(rp2, np.delete(col, j), np.delete(mult, j))
        assert ei.value.code == gossip.E_INVAL
        # rows are scanned in order: the first entry without a reverse is the leaf's entry for the hub
        assert f"row {leaf}, col {hub}" in str(ei.value) and "asymmetric" in str(ei.value)
        eng.set_graph(rp, col, mult)      # the refusal left the engine without a graph: the whole CSR is taken
    finally:
        eng.close()
