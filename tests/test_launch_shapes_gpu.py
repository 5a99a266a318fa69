"""Every k_pull instantiation, the grid-stride loops and the DENSE K split at small n, each named from
the engine's launch ledger (gossip.h, gossip_engine_get_launches: what was launched, counted at the
launch sites) and compared with ORACLE A bit for bit: the seven per-node counters and the first-contact
trace.

The shape rule, restated here (csrc/pull_plan.h has it; tests/pull_plan pins it): hw, the high-water
count of 64-share words of the live window, gives the word-lanes -- hw <= 16: lpw 8, hw <= 32: lpw 16,
hw <= 64: lpw 32, above that lpw 32 "wide" with epn 1 -- and below the wide window the edge-lanes epn
double while lpw * epn * 2 <= 64 and epn * 8 < avg_deg, avg_deg = CSR entries (distinct neighbours) / n.
hw is 16 words per 1,024-share tile in use and only grows: with unique ids a burst of B births in the
first tick and none later pins the window for the run (B <= 1,024: hw 16; <= 2,048: 32; <= 3,072: 48),
and GOSSIP_F_TILE_PER_TICK with floods of several hops gives a wide one.

k_young_idle's block cap is a constant 16,384, so it cannot stride below 4.19 M nodes: its launches
are in the ledger, its stride loop is covered only by the C4-scale tests (test_scale_gpu.py).
"""
import numpy as np
import pytest

import structured as S
from cases import L, T0
from test_structured_gpu import STATS, assert_parity_inputs

pytestmark = pytest.mark.gpu

K_PULL, K_PULL_YOUNG, K_YOUNG_IDLE, K_DENSE_BITS, K_DENSE_DEDUP = range(5)
NT, SP, PUSH, SHORT, FOLD = 1, 2, 4, 8, 16

# ---- inputs --------------------------------------------------------------------------------------
# name -> (n, average degree, graph seed, birth ticks, births per tick, cut in ticks after T0, ...); G(n,p)
# of the skip kind: Poisson degrees, so peer lists that are no multiple of the edge-lanes and shorter
# than them.  The cut falls inside a tick (keep masks on the last one) and early enough that ORACLE A's
# event loop stays at a few million edge events (each input: under 5 s of ORACLE A, once per session).
INPUTS = {
    # bursts: every birth in the first tick, hw pinned for the run
    "b700_d5": (700, 5, 71, 1, 700, 6), "b700_d12": (700, 12, 72, 1, 700, 3),
    "b700_d24": (700, 24, 73, 1, 700, 2), "b700_d48": (700, 48, 74, 1, 700, 2),
    "b1500_d5": (1500, 5, 75, 1, 1500, 4), "b1500_d12": (1500, 12, 76, 1, 1500, 2),
    "b1500_d24": (1500, 24, 77, 1, 1500, 2),
    "b2600_d5": (2600, 5, 78, 1, 2600, 3), "b2600_d12": (2600, 12, 79, 1, 2600, 2),
    # n = 3,000: 47 chunks of 64 nodes, the last of 56, a natural grid of 12 blocks
    "b3000_d12": (3000, 12, 80, 1, 3000, 2), "b1000of3000_d5": (3000, 5, 81, 1, 1000, 4),
    # a fresh tile per birth tick (flag), floods of ~8 hops: a wide window (6 tiles) holding tiles of
    # six ages.  200 births in the first tick, 4 in each later one (the 7th entry: births kept per tick
    # after the first): the engine's BFS layer model then expects 32 bits and more per row on two
    # consecutive hops of the first tile (0.60 and 0.21 of the nodes at hops 4 and 5 of a degree-8.2
    # graph), which is what makes a tile dense-row and then folded under the auto settings, beside
    # early and late tiles that push
    "wide": (3000, 8, 82, 6, 200, 14, 4),
    # DENSE mode: n_pad 9,216 (9 K stages, ragged last row block, more rows than the dedup grid's 8,192
    # waves) and 5,120 (5 stages); two dozen shares over six ticks
    "dense8300": (8300, 80, 83, 6, 4, 6), "dense5000": (5000, 80, 84, 6, 4, 6),
    "dense5000_collide": (5000, 80, 84, 6, 4, 6),
}
_inputs_memo = {}


def _inputs(gossip, name):
    if name not in _inputs_memo:
        n, deg, seed, ticks, per_tick, cut = INPUTS[name][:6]
        topo = gossip.Topology.gnp(n, deg / (n - 1), seed, gossip.TOPO_SKIP)
        a, b = topo.links()
        ev = S.events(n, ticks, per_tick, seed + 100, id_mask=0xF if name.endswith("_collide") else 0)
        if len(INPUTS[name]) > 6:  # thin the later ticks (a subset: the ids stay unique)
            tick = (ev["ns"] - T0) // L
            rank = np.arange(len(ev)) - np.searchsorted(tick, tick)
            ev = ev[(tick == 0) | (rank < INPUTS[name][6])]
        rp, _, _ = topo.csr()
        _inputs_memo[name] = dict(name=name, n=n, a=a, b=b, ev=ev, t_cut=T0 + cut * L + L // 3, topo=topo,
                                  avg_deg=float(rp[-1]) / n)
    return _inputs_memo[name]


def _run(gossip, f, flags=(), opts=(), lat=L, mode=None):
    """One engine over the inputs: (stats, counters, trace, ledger as {(kernel, lpw, epn, flags, arg): record})."""
    eng = _engine(gossip, f, flags, opts, lat, mode)
    try:
        eng.run()
        eng.sync()
        return _results(eng)
    finally:
        eng.close()


def _engine(gossip, f, flags, opts, lat, mode, part=None):
    fl = 0 if part else gossip.F_TRACE  # (a row rank: counters only)
    for x in flags:
        fl |= getattr(gossip, x)
    eng = gossip.Engine(f["n"], lat, T0, f["t_cut"], flags=fl, mode=gossip.MODE_CSR if mode is None else mode)
    try:
        if part:
            eng.set_row_partition(*part)
        for k, v in opts:
            eng.set_option(k, v)
        eng.set_topology(f["topo"])
        eng.set_schedule(f["ev"])
    except Exception:
        eng.close()
        raise
    return eng


def _results(eng, trace=True):
    led = {r.key: r for r in eng.launches()}
    return eng.stats(), eng.counters(), eng.trace() if trace else None, led


def _pull(led, lpw, epn, flags):
    """The ledger's record of k_pull<lpw, epn, flags> (None: never launched)."""
    return led.get((K_PULL, lpw, epn, flags, 0))


def _pull_keys(led):
    return {(k[1], k[2], k[3]) for k in led if k[0] == K_PULL}


def _same(x, y, what):
    for k in STATS:
        assert np.array_equal(getattr(x[0], k), getattr(y[0], k)), (what, k)
    for p, q in zip(S.sorted_trace(x[2]), S.sorted_trace(y[2])):
        assert np.array_equal(p, q), what


def _show(what, c, led):
    print(what, "words_hw", c.words_hw, "pull_grid", c.pull_grid, "young_grid", c.young_grid, "ledger",
          sorted((k, r.launches, r.strided) for k, r in led.items()))


# ---- the ledger's ABI on a live engine -----------------------------------------------------------------
def test_ledger_is_cumulative_and_caller_sized(gossip):
    import ctypes as C
    f = _inputs(gossip, "b700_d5")
    eng = _engine(gossip, f, (), (), L, None)
    try:
        assert eng.launches() == []  # nothing launched yet
        eng.run(eng.first_tick + 2)
        eng.sync()
        mid = {r.key: r.launches for r in eng.launches()}
        assert mid and sum(mid.values()) == eng.counters().pull_launches  # one window: one k_pull per tick
        eng.reset_timing()
        assert eng.counters().pull_launches == 0
        assert {r.key: r.launches for r in eng.launches()} == mid  # reset_timing leaves the ledger
        eng.run()
        eng.sync()
        end = {r.key: r.launches for r in eng.launches()}
        assert all(end[k] >= v for k, v in mid.items()) and sum(end.values()) > sum(mid.values())
        # NULL sizes; an array too short is refused and left alone
        lib, cnt = gossip.load_library(), C.c_uint32(0)
        assert lib.gossip_engine_get_launches(eng._h, None, 0, C.byref(cnt)) == 0 and cnt.value == len(end)
        arr = (gossip.gossip_launch_record * 1)()
        if len(end) > 1:
            assert lib.gossip_engine_get_launches(eng._h, arr, 1, C.byref(cnt)) == gossip.E_INVAL
            assert cnt.value == len(end) and arr[0].launches == 0
        assert lib.gossip_engine_get_launches(eng._h, arr, 1, None) == gossip.E_INVAL
    finally:
        eng.close()


# ---- B. one case per k_pull instantiation ----------------------------------------------------------
TPT = ("F_TILE_PER_TICK",)
# (lpw, epn, flags) -> (input, engine flags, options, words_hw).  The key follows the shape rule of the
# module docstring from the input's window and degree band (<= 8: epn 1, <= 16: 2, <= 32: 4, above: 8,
# capped by 64 / lpw), and from the options: pull_nt 1 takes the non-temporal form where one exists
# (lpw 16 and 32 at epn 1); 32 x 1 lanes over tile lists with saturation words run the SP instantiations,
# which pull_sat 0 or pull_tiles 0 defeat.
SHAPES = {
    (8, 1, 0): ("b700_d5", (), (), 16),
    (8, 2, 0): ("b700_d12", (), (), 16),
    (8, 4, 0): ("b700_d24", (), (), 16),
    (8, 8, 0): ("b700_d48", (), (), 16),
    (16, 1, 0): ("b1500_d5", (), (), 32),
    (16, 2, 0): ("b1500_d12", (), (), 32),
    (16, 4, 0): ("b1500_d24", (), (), 32),
    (32, 1, 0): ("b2600_d5", (), (("pull_sat", 0),), 48),
    (32, 2, 0): ("b2600_d12", (), (), 48),
    (16, 1, NT): ("b1500_d5", (), (("pull_nt", 1),), 32),
    (32, 1, NT): ("b2600_d5", (), (("pull_nt", 1), ("pull_tiles", 0)), 48),
}
# the sixteen SP kernels on the wide window: NT from pull_nt, PUSH from pull_push 1 (every listed tile
# that is not dense-row marks; the layer model's dense-row tiles in the middle of a flood leave the early
# and late tiles of the window to push), SHORT from pull_batch 1, FOLD from seen_fold -1 (auto: the
# dense-row tiles fold) against 0
for _f in range(16):
    _nt, _push, _short, _fold = _f & 1, (_f >> 1) & 1, (_f >> 2) & 1, (_f >> 3) & 1
    SHAPES[(32, 1, SP | NT * _nt | PUSH * _push | SHORT * _short | FOLD * _fold)] = (
        "wide", TPT, (("pull_nt", _nt), ("pull_push", _push), ("pull_batch", _short), ("seen_fold", -1 if _fold else 0)),
        None)
# instantiations no input of this file reaches, each with its reason (at most two, SP with PUSH and FOLD)
NOT_REACHED = {}

_reached = {}  # key -> the k_pull keys its case launched (the completeness test reads it)


def _shape_id(key):
    lpw, epn, fl = key
    return f"{lpw}x{epn}" + "".join("_" + s for s, b in (("nt", NT), ("sp", SP), ("push", PUSH), ("short", SHORT),
                                                         ("fold", FOLD)) if fl & b)


def _shape_case(gossip, oracle, key):
    name, flags, opts, hw = SHAPES[key]
    f = _inputs(gossip, name)
    st, c, tr, led = _run(gossip, f, flags, opts)
    _show((key, name, opts), c, led)
    _reached[key] = _pull_keys(led)
    assert_parity_inputs(oracle, f, L, st, tr, (key, name, opts))
    return f, c, led


@pytest.mark.parametrize("key", [k for k in SHAPES if k not in NOT_REACHED], ids=_shape_id)
def test_pull_instantiation(gossip, oracle, key):
    f, c, led = _shape_case(gossip, oracle, key)
    lpw, epn, fl = key
    hw = SHAPES[key][3]
    # the degree band the table's key assumes
    band = 1 if f["avg_deg"] <= 8 else 2 if f["avg_deg"] <= 16 else 4 if f["avg_deg"] <= 32 else 8
    if hw is None:
        assert c.words_hw > 64, c.words_hw
    else:
        assert c.words_hw == hw and epn == min(band, 64 // lpw), (c.words_hw, f["avg_deg"])
    r = _pull(led, lpw, epn, fl)
    assert r is not None and r.launches > 0, (key, sorted(_pull_keys(led)))
    assert c.pull_lpw == lpw and c.pull_nt == (1 if fl & NT else 0)


if NOT_REACHED:  # (an empty parameter list would leave a skipped test behind)
    @pytest.mark.parametrize("key", list(NOT_REACHED), ids=_shape_id)
    @pytest.mark.xfail(strict=True, reason="no input of this file reaches the instantiation (NOT_REACHED)")
    def test_pull_instantiation_not_reached(gossip, oracle, key):
        _, _, led = _shape_case(gossip, oracle, key)
        r = _pull(led, *key)
        assert r is not None and r.launches > 0, NOT_REACHED[key]


def test_pull_matrix_is_complete(gossip):
    # the cases above record what they launched; a case that did not run in this session runs here
    for key, (name, flags, opts, _) in SHAPES.items():
        if key not in _reached:
            _reached[key] = _pull_keys(_run(gossip, _inputs(gossip, name), flags, opts)[3])
    listed = {(r.lpw, r.epn, r.flags) for r in gossip.pull_instantiations()}
    assert len(listed) == 27 and set(SHAPES) == listed
    assert len(NOT_REACHED) <= 2 and all(k[2] & SP and k[2] & PUSH and k[2] & FOLD and why for k, why in NOT_REACHED.items())
    reached = {k for k in SHAPES if k not in NOT_REACHED and k in _reached.get(k, ())}
    assert reached | set(NOT_REACHED) == listed, sorted(listed - reached - set(NOT_REACHED))
    assert not any(k in _reached.get(k, ()) for k in NOT_REACHED)


# ---- C. grid-stride loops ----------------------------------------------------------------------------
# one representative per kernel family on n = 3,000 (47 chunks): (key, input, flags, options)
STRIDE = {
    "epn2": ((32, 2, 0), "b3000_d12", (), ()),
    "tile_masks_8x1": ((8, 1, 0), "b1000of3000_d5", (), ()),
    "no_tile_lists": ((8, 1, 0), "b1000of3000_d5", (), (("pull_tiles", 0),)),
    "sp_push": ((32, 1, SP | PUSH), "wide", TPT, (("pull_push", 1), ("seen_fold", 0))),
    "sp_fold": ((32, 1, SP | FOLD), "wide", TPT, (("pull_push", 0),)),
    "sp_short": ((32, 1, SP | SHORT), "wide", TPT, (("pull_batch", 1), ("pull_push", 0), ("seen_fold", 0))),
}


@pytest.mark.parametrize("fam", list(STRIDE))
def test_pull_grid_stride(gossip, oracle, fam):
    key, name, flags, opts = STRIDE[fam]
    f = _inputs(gossip, name)
    assert f["n"] == 3000
    nat = _run(gossip, f, flags, opts)
    _show((fam, "natural grid"), nat[1], nat[3])
    assert_parity_inputs(oracle, f, L, nat[0], nat[2], (fam, "natural grid"))
    r = _pull(nat[3], *key)
    assert r is not None and r.launches > 0 and nat[1].pull_grid == 12
    assert all(x.strided == 0 for k, x in nat[3].items() if k[0] == K_PULL)  # 48 waves, 47 chunks
    if fam == "no_tile_lists":
        assert nat[1].pull_tiles == 0
    for grid in (1, 3):
        got = _run(gossip, f, flags, opts + (("pull_grid", grid),))
        _show((fam, grid), got[1], got[3])
        assert_parity_inputs(oracle, f, L, got[0], got[2], (fam, grid))
        _same(got, nat, (fam, grid, "vs natural grid"))
        r = _pull(got[3], *key)
        assert r is not None and r.strided > 0 and r.strided == r.launches, (fam, grid)
        assert got[1].pull_grid == grid
        assert _pull_keys(got[3]) == _pull_keys(nat[3])  # the grid changes no dispatch


YOUNG = {
    "overlap": (("young", 1), ("young_overlap", 1), ("young_skip", 1)),
    "serial": (("young", 1), ("young_overlap", 0), ("young_skip", 1)),
    "overflow": (("young", 1), ("young_cap", 3), ("young_list_cap", 8), ("young_age", 6), ("young_skip", 1)),
    "no_skip": (("young", 1), ("young_skip", 0)),
}


@pytest.mark.parametrize("fam", list(YOUNG))
def test_young_grid_stride(gossip, oracle, fam):
    f = _inputs(gossip, "wide")
    opts = YOUNG[fam]
    nat = _run(gossip, f, TPT, opts)
    _show((fam, "natural grid"), nat[1], nat[3])
    assert_parity_inputs(oracle, f, L, nat[0], nat[2], (fam, "natural grid"))
    assert nat[1].young_launches > 0 and nat[1].young_grid == 750  # ceil(3,000 / 4) blocks
    assert all(x.strided == 0 for k, x in nat[3].items() if k[0] in (K_PULL_YOUNG, K_YOUNG_IDLE))
    if fam == "overflow":
        assert nat[1].young_fallback_rows > 0
    # the instantiation of the sparse ticks with empty-slot skipping, the other one without
    arg = 0 if fam == "no_skip" else 1
    for grid in (1, 5):
        got = _run(gossip, f, TPT, opts + (("young_grid", grid),))
        _show((fam, grid), got[1], got[3])
        assert_parity_inputs(oracle, f, L, got[0], got[2], (fam, grid))
        _same(got, nat, (fam, grid, "vs natural grid"))
        young = {k[4]: x for k, x in got[3].items() if k[0] == K_PULL_YOUNG}
        assert young and all(x.strided == x.launches > 0 for x in young.values()), (fam, grid)
        assert arg in young, (fam, grid, sorted(young))
        assert got[1].young_grid == grid
        idle = got[3].get((K_YOUNG_IDLE, 0, 0, 0, 0))
        assert idle is None or idle.strided == 0  # (its own grid: the module docstring)


# ---- D. DENSE three-kernel path: K split and dedup stride --------------------------------------------
def _dense(gossip, oracle, name, opts, lat=L, fused=0):
    f = _inputs(gossip, name)
    got = _run(gossip, f, (), (("dense_fused", fused),) + opts, lat=lat, mode=gossip.MODE_DENSE)
    _show((name, opts, lat), got[1], got[3])
    assert_parity_inputs(oracle, f, lat, got[0], got[2], (name, opts, lat))
    assert got[1].dense_ops > 0 and got[1].words_hw == 16
    if not fused:
        assert got[1].dense_fused_launches == 0
    return got


def _ksplits(led):
    return {k[4]: r for k, r in led.items() if k[0] == K_DENSE_BITS}


@pytest.mark.parametrize("min_tiles", [1, 512, 1 << 20])
def test_dense_ksplit_8300(gossip, oracle, min_tiles):
    # n_pad 9,216: 36 row blocks x 4 column tiles = 144 block tiles, 9 stages.  dense_min_tiles 1 leaves
    # K whole; the default 512 and 2^20 both split it in 4 (a split keeps at least 2 stages): splits of
    # ceil(9 / 4) = 3 stages, the fourth empty
    st, c, tr, led = _dense(gossip, oracle, "dense8300", (("dense_min_tiles", min_tiles),))
    ks = _ksplits(led)
    assert set(ks) == ({1} if min_tiles == 1 else {4}), sorted(ks)
    if min_tiles == 1:
        assert ks[1].launches > 0 and ks[1].strided == 0
    else:
        assert ks[4].strided == ks[4].launches > 0
    dd = led[(K_DENSE_DEDUP, 0, 0, 0, 0)]
    assert dd.strided == dd.launches > 0  # 8,300 rows, 512 blocks of 16 waves


@pytest.mark.parametrize("lat", [L, S.L_ODD])
def test_dense_ksplit_5000(gossip, oracle, lat):
    # n_pad 5,120: 20 x 4 block tiles, 5 stages: the default splits K in 2, stages 3 + 2; the 2.3 ms
    # latency brings keep masks into the dedup
    st, c, tr, led = _dense(gossip, oracle, "dense5000", (), lat=lat)
    ks = _ksplits(led)
    assert set(ks) == {2} and ks[2].strided == ks[2].launches > 0, sorted(ks)
    dd = led[(K_DENSE_DEDUP, 0, 0, 0, 0)]
    assert dd.launches > 0 and dd.strided == 0  # 5,000 rows: one per wave


def test_dense_ksplit_row_partition(gossip, oracle):
    # two row ranks (lockstep backend) of 4,608 and 3,692 rows: rank 1 starts at row block 18 (mb0 > 0),
    # each rank contracts its row chunks with the K split
    f = _inputs(gossip, "dense8300")
    whole = _run(gossip, f, (), (("dense_fused", 0),), mode=gossip.MODE_DENSE)
    assert_parity_inputs(oracle, f, L, whole[0], whole[2], "dense8300 single engine")
    ranks = [_engine(gossip, f, (), (("dense_fused", 0),), L, gossip.MODE_DENSE, part=(r, 2)) for r in range(2)]
    try:
        gossip.group_run(ranks)
        for e in ranks:
            e.sync()
        got = [_results(e, trace=False) for e in ranks]
    finally:
        for e in ranks:
            e.close()
    for k in ("gen", "recv", "fwd", "sent", "processed"):
        total = sum(getattr(g[0], k).astype(np.uint64) for g in got)
        assert np.array_equal(total, getattr(whole[0], k).astype(np.uint64)), k
    for r, g in enumerate(got):
        _show(("dense8300 rank", r), g[1], g[3])
        own = np.flatnonzero(g[0].recv)
        assert own.size and (own.max() < 4608 if r == 0 else own.min() >= 4608), r
        ks = _ksplits(g[3])
        assert ks and all(k > 1 and x.launches > 0 for k, x in ks.items()), (r, sorted(ks))
        assert g[1].dense_fused_launches == 0


def test_dense_ksplit_colliding_ids(gossip, oracle):
    # id groups: a tick whose window holds a group word leaves the fused kernel for the three-kernel path
    st, c, tr, led = _dense(gossip, oracle, "dense5000_collide", (), fused=1)
    assert len(np.unique(_inputs(gossip, "dense5000_collide")["ev"]["share_id"])) < 24
    assert c.dense_fused_launches < c.pull_launches
    ks = _ksplits(led)
    assert set(ks) == {2} and ks[2].strided == ks[2].launches > 0, sorted(ks)
