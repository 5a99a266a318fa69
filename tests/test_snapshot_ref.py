"""The reference of test_snapshots_gpu.py, checked on the CPU.

snapshot_ref.expected derives a periodic snapshot's totals from ORACLE A's trace (events with t < T).
Here it is pinned against ORACLE A's own PrintPeriodicStats rows, and against closed-form hand cases;
and for every oracle run the device tests compare with, the snapshot times are shown to fall where they
can fail: inside ticks that hold arrivals, and generations, on both sides of the snapshot.
"""
import functools

import numpy as np
import pytest

import snapshot_ref as R
import structured as S
from cases import CASES, L, T0


# ---- expected() against ORACLE A's own periodic rows ---------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(num_nodes=60, connection_prob=0.1, sim_time_s=20.05, latency_ms=3.7, topo_seed=6, node_seed=6000),  # n60_lat37
    dict(num_nodes=300, connection_prob=0.05, sim_time_s=20.05, latency_ms=2.3, topo_seed=5, node_seed=5000, id_mask=0xFF),
    dict(num_nodes=400, connection_prob=0.01, sim_time_s=30.05, latency_ms=2.3, topo_seed=73, node_seed=74, id_mask=0x3FF),
], ids=["n60_lat37", "n300_idFF", "n400_id3FF"])
def test_expected_equals_oracle_periodic_rows(oracle, kw):
    r = oracle.run_reference(trace=True, **kw)
    lat = oracle.milliseconds_to_ns(kw["latency_ms"])
    t_cut = oracle.seconds_to_ns(kw["sim_time_s"] - 0.1)
    assert len(r.periodic) >= 2
    assert any(t % lat != 0 and t < t_cut for t, _, _, _ in r.periodic)  # inside a tick, before the cut
    assert r.periodic[-1][0] > t_cut                                     # and one after it: frozen totals
    for t, gen, proc, _sockets in r.periodic:
        assert R.expected(r, t) == (t, gen, proc)
    assert R.expected(r, t_cut)[1:] == (int(r.gen.sum()), int(r.processed.sum()))
    if kw.get("id_mask"):  # colliding ids: generations that are no new processed id
        assert len(np.unique(r.gen_events[2])) < len(r.gen_events[2])


# ---- the snapshot times ---------------------------------------------------------------------------
def test_times_recipe():
    a = R.times(L, T0 + 40 * L + L // 3)
    tick0 = T0 // L
    assert sorted(t // L - tick0 for t in a) == [-1, 0, 1, 2, 3, 20, 39, 40, 41]
    assert sorted(t % L for t in a if 0 <= t // L - tick0 < 40 and t // L - tick0 != 2) == sorted(
        [L // 3, L // 2, 2 * L // 3, L // 3, L // 2])
    assert (tick0 + 2) * L in a and T0 - L // 2 in a and T0 + 41 * L + L // 3 in a
    assert (tick0 + 40) * L + (L // 3) // 2 in a
    b = R.times(L, T0 + 40 * L + L // 3, which="B")
    assert set(a) - set(b) == {(tick0 + 3) * L + 2 * L // 3, (tick0 + 20) * L + L // 3, (tick0 + 40) * L + (L // 3) // 2}
    assert set(b) - set(a) == {(tick0 + 3) * L + 1, (tick0 + 20) * L + L - 1, T0 + 40 * L + L // 3}
    # 2.3 ms: T0 is inside tick0, which k = 0 holds -- the snapshot before the run moves one tick back
    lat = S.L_ODD
    o = R.times(lat, T0 + 40 * L + L // 3, extra=((9, 7),))
    assert len({t // lat for t in o}) == len(o) == 10 and (T0 // lat + 9) * lat + 7 in o
    assert min(o) == T0 - lat // 2 - lat and min(o) // lat == T0 // lat - 1
    with pytest.raises(AssertionError):
        R.times(L, T0 + 40 * L, extra=((3, 5),))  # two snapshots in one tick


@functools.lru_cache(maxsize=None)
def _family(name):
    return S.family(name)


@pytest.mark.parametrize("name,lat,kind", R.RUNS)
def test_set_a_splits_ticks(oracle, name, lat, kind):
    # what gives the device test teeth: a kernel that ignored its snapshot mask and counted every new
    # bit of the tick, or none, is wrong wherever the tick holds events on both sides of T
    f = _family(name)
    r = R.replay(oracle, f, lat, kind)
    ts = R.family_times(f, lat)
    sp = [R.splits(r, lat, T) for T in ts]
    arrivals = [(T, s[:2]) for T, s in zip(ts, sp) if s[0] > 0 and s[1] > 0]
    gens = [(T, s[2:]) for T, s in zip(ts, sp) if s[2] > 0 and s[3] > 0]
    print(name, lat, kind, "arrivals split", arrivals, "generations split", gens)
    assert len(arrivals) >= 3, (name, lat, kind, sp)
    assert len(gens) >= 1, (name, lat, kind, sp)
    want = [R.expected(r, T) for T in ts]
    assert want[-2][1:] == (0, 0)                                                  # before the run
    assert want[-1][1:] == (int(r.gen.sum()), int(r.processed.sum()))              # after the cut: frozen
    assert R.expected(r, f["t_cut"]) == (f["t_cut"],) + want[-1][1:]


def test_figures_of_three_ticks(oracle):
    # (the splits the choice of r around lat / 2 was made on)
    for name, k, want in (("ladder", 3, (2394, 928)), ("long_ring", 100, (218, 182)), ("dense_sparse", 15, (687, 610))):
        r = R.replay(oracle, _family(name), L)
        assert R.splits(r, L, T0 + k * L + L // 2)[:2] == want, name


def test_set_b_on_the_ladder(oracle):
    # r = 1: no event before T in its tick (phases are >= 1); r = lat - 1: every event before it;
    # T = t_cut: everything the run counts
    f = _family("ladder")
    for lat in (L, S.L_ODD):
        r = R.replay(oracle, f, lat)
        tick0 = T0 // lat
        for T in R.family_times(f, lat, "B"):
            s = R.splits(r, lat, T)
            if T % lat == 1:
                assert s[0] == 0 and s[2] == 0 and s[1] > 0, (lat, T, s)
            if T % lat == lat - 1:
                assert s[1] == 0 and s[3] == 0 and s[0] > 0, (lat, T, s)
        assert f["t_cut"] in R.family_times(f, lat, "B")
        assert sum(1 for T in R.family_times(f, lat, "B") if T % lat in (1, lat - 1) and T // lat > tick0) == 2


# ---- hand cases -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.HAND))
def test_hand_cases(oracle, name):
    c = next(x for x in CASES if x["name"] == name)
    a, b = [x for x, _ in c["links"]], [y for _, y in c["links"]]
    ev = np.array(c["events"], np.int64)
    assert ev[1, 0] // L - T0 // L == R.HAND_TICK and ev[1, 1] == 2
    r = oracle.run_replay(c["n"], L, T0, c["t_cut"], a, b, ev[:, 0], ev[:, 1], ev[:, 2], trace=True)
    for k, want in c["expect"].items():
        assert getattr(r, k).tolist() == want, (name, k)
    for ph, want in R.HAND[name]:
        T = T0 + R.HAND_TICK * L + ph
        assert R.expected(r, T) == (T,) + want, (name, ph)
    # the thresholds are the two events' own phases
    g, arr = int(ev[1, 0] % L), int((ev[0, 0] + 2 * L) % L)
    assert {ph for ph, _ in R.HAND[name]} >= {g, g + 1, arr, arr + 1}
    if name == "collide_same_tick_gen_first":
        assert R.gen_beats_arrival(r, (a, b), L) == [(2, 5, int(ev[1, 0]), int(ev[0, 0]) + 2 * L)]
    else:
        assert R.gen_beats_arrival(r, (a, b), L) == []


# ---- an own generation that beats a same-tick arrival, in the families -----------------------------
def test_components_collide_has_a_generation_that_beats_an_arrival(oracle):
    f = _family("components_collide")
    r = R.replay(oracle, f, L)
    found = R.gen_beats_arrival(r, (f["a"], f["b"]), L)
    assert found == [(118, 5, 5_090_766_484, 5_092_180_404)]
    node, sid, t_gen, t_arr = found[0]
    assert t_arr < f["t_cut"]
    (k, ph), = R.EXTRA[("components_collide", L)]
    T = (T0 // L + k) * L + ph
    assert T // L == t_gen // L == t_arr // L and t_gen < t_arr < T  # the snapshot lies past the arrival's phase
    assert T in R.family_times(f, L)
    # node 118's id 5 is one processed id there: its generation, not the arrival
    at = (r.trace[0] == node) & (r.trace[1] == sid)
    assert r.trace[2][at].tolist() == [t_gen] and r.trace[4][at].tolist() == [0]


def test_other_colliding_schedules_have_none(gossip, oracle):
    # (scanned over every tick; should a change of the schedules bring one, add a snapshot past its
    # arrival's phase to snapshot_ref.EXTRA)
    f = _family("ladder_collide")
    assert R.gen_beats_arrival(R.replay(oracle, f, L), (f["a"], f["b"]), L) == []
    n = 400  # test_young_gpu.py's test_young_collisions
    topo = gossip.Topology.gnp(n, 0.01, 73, gossip.TOPO_EXACT)
    t_cut = gossip.seconds_to_ns(14.9)
    ev = gossip.make_schedule(n, 74, T0, t_cut, id_mask=0x3FF)
    a, b = topo.links()
    r = oracle.run_replay(n, L, T0, t_cut, a, b, ev["ns"], ev["node"], ev["share_id"], trace=True)
    assert len(np.unique(ev["share_id"])) < len(ev)
    assert R.gen_beats_arrival(r, (a, b), L) == []
