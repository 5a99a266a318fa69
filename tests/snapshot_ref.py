"""Periodic-snapshot totals (PrintPeriodicStats, p2pnetwork.cc:231-250) from ORACLE A's trace.

A periodic event at T is scheduled before every event of its own nanosecond, so it sees exactly
the events with t < T:

    total_gen       = #{counted generations with ns < T}        (gen_events)
    total_processed = #{first-contact records with t_ns < T}    (trace; one per processedShares entry)

A record exists only for t_ns < t_cut, so both totals are frozen after the cut.
test_snapshot_ref.py pins this rule against ORACLE A's own on_periodic rows; test_snapshots_gpu.py
compares the engine's snapshots with it at times that fall inside a tick, where the kernels count a
partial through their per-word snapshot masks (a tick-aligned snapshot takes the base sums only).

Plain helpers, no GPU.
"""
import numpy as np

from cases import T0


def expected(result, T):
    """(T, total_gen, total_processed) of a snapshot at T from an OracleResult that has a trace."""
    assert result.trace is not None
    return (int(T), int(np.count_nonzero(result.gen_events[0] < T)), int(np.count_nonzero(result.trace[2] < T)))


def times(lat, t_cut, t0=T0, which="A", extra=()):
    """The snapshot times of one run, at most one per tick (the engine's rule).  With tick0 = t0 // lat
    and K = t_cut // lat - tick0:

    set A: ticks tick0 + k for k in (0, 1, 3, K // 2, K - 1) with r cycling through lat // 3, lat // 2
           and 2 * lat // 3; k = 2 with r = 0 (aligned: base sums only); the cut tick with
           r = (t_cut % lat) // 2 (keep and snapshot masks on one tick); t0 - lat // 2 (before the run:
           zeros); t_cut + lat (after the cut: frozen totals).
    set B: the same, but the cut-tick snapshot is t_cut itself and the two mid ticks k = 3 and K // 2
           take r = 1 (an empty mask: phases are >= 1) and r = lat - 1.

    extra: further (k, r) pairs, snapshots at (tick0 + k) * lat + r, for a run whose recipe ticks do not
    split enough events (EXTRA below).

    Where t0 is not a multiple of lat, t0 - lat // 2 can fall into tick0 itself, which k = 0 holds; it
    then moves back by whole ticks until its tick is free (still before the run)."""
    assert which in ("A", "B")
    tick0 = t0 // lat
    K = t_cut // lat - tick0
    assert K >= 8, K  # 0, 1, 2, 3, K // 2, K - 1 and K are seven different ticks
    rs = (lat // 3, lat // 2, 2 * lat // 3)
    out = []
    for i, k in enumerate((0, 1, 3, K // 2, K - 1)):
        r = rs[i % 3]
        if which == "B" and k == 3:
            r = 1
        if which == "B" and k == K // 2:
            r = lat - 1
        out.append((tick0 + k) * lat + r)
    out += [(tick0 + k) * lat + r for k, r in extra]
    out.append((tick0 + 2) * lat)
    out.append(t_cut if which == "B" else (tick0 + K) * lat + (t_cut % lat) // 2)
    before = t0 - lat // 2
    while before // lat >= tick0:
        before -= lat
    out.append(before)
    out.append(t_cut + lat)
    ticks = [t // lat for t in out]
    assert len(set(ticks)) == len(ticks), ticks
    return out


# (family, latency) -> extra (k, r) of set A, where the recipe's own ticks split too few events:
#  ladder_collide: 64 ids -- every node holds every id after 15 ticks, K // 2 = 30 and K - 1 = 59 are
#      empty; ticks 5, 8 and 11 are in the thick of the floods.
#  components_collide: node 118 generates id 5 at phase 766,484 of tick +18 while a peer's copy of id 5
#      is due there at phase 2,180,404: the pull counts that arrival and k_births takes it back; r lies
#      past the arrival's phase (test_snapshot_ref.py asserts the event from ORACLE A's trace).
#  dense_tail[1025] at 2.3 ms: two births per 5 ms leave few 2.3 ms ticks with two generations; tick +9
#      has them at phases 1,325,969 and 1,559,129.
EXTRA = {
    ("ladder_collide", 5_000_000): ((5, 5_000_000 // 3), (8, 5_000_000 // 2), (11, 2 * 5_000_000 // 3)),
    ("components_collide", 5_000_000): ((18, 2_181_404),),
    ("dense_tail[1025]", 2_300_000): ((9, 1_442_549),),
}


# The oracle runs test_snapshots_gpu.py compares with: (family, latency, kind), kind "plain", "link"
# (run_replay(link_timing=LINK_5MBPS), the hop-batched runs) or "handshake" (handshake=(2 lat, 3 lat)).
# test_snapshot_ref.py asserts for each that set A splits arrivals and generations inside a tick.
RUNS = [("ladder", 5_000_000, "plain"), ("ladder", 2_300_000, "plain"), ("ladder_collide", 5_000_000, "plain"),
        ("components_collide", 5_000_000, "plain"), ("tail[65]", 5_000_000, "plain"), ("tail[513]", 5_000_000, "plain"),
        ("long_ring", 5_000_000, "plain"), ("dense_tail[1025]", 5_000_000, "plain"),
        ("dense_tail[1025]", 2_300_000, "plain"), ("dense_sparse", 5_000_000, "plain"),
        ("ladder", 5_000_000, "link"), ("ladder", 5_000_000, "handshake"), ("tail[65]", 5_000_000, "handshake")]


def replay(oracle, f, lat, kind="plain"):
    """ORACLE A's run of a structured.py family (the run_replay arguments of test_structured_gpu.py, so a
    session's memoised oracle serves both files)."""
    kw = {}
    if kind == "link":
        kw["link_timing"] = oracle.LINK_5MBPS
    if kind == "handshake":
        kw["handshake"] = (2 * lat, 3 * lat)
    return oracle.run_replay(f["n"], lat, T0, f["t_cut"], f["a"], f["b"], f["ev"]["ns"], f["ev"]["node"],
                             f["ev"]["share_id"], trace=True, **kw)


# Hand cases on cases.py's path 0-1-2, id 5 generated at node 0 at phase 123,457 of tick +0 and again at
# node 2 in tick +2, where node 0's copy arrives at phase 123,457.  Before tick +2: node 0's generation
# and node 1's arrival, (gen, processed) = (1, 2).  A snapshot at phase r of tick +2 sees the events with
# phase < r:
#  collide_same_tick_gen_first (node 2 generates at phase 122,457; the arrival is a duplicate, dropped):
#      r <= 122,457: neither;  r in (122,457, 123,457]: the generation, a new processed id;
#      r > 123,457: the same -- an engine's pull has counted the arrival and k_births takes it back.
#  collide_same_tick_arrival_first (node 2 generates at phase 124,457, after the arrival):
#      r <= 123,457: neither;  r in (123,457, 124,457]: the arrival;  r > 124,457: the generation as
#      well, counted but not a new processed id.
HAND_TICK = 2
HAND = {
    "collide_same_tick_gen_first": [(1, (1, 2)), (122_457, (1, 2)), (122_458, (2, 3)), (123_457, (2, 3)),
                                    (123_458, (2, 3)), (4_999_999, (2, 3))],
    "collide_same_tick_arrival_first": [(1, (1, 2)), (123_457, (1, 2)), (123_458, (1, 3)), (124_457, (1, 3)),
                                        (124_458, (2, 3)), (4_999_999, (2, 3))],
}


def family_times(f, lat, which="A"):
    """times() for a family of structured.py (its dict), with the family's EXTRA ticks in set A."""
    extra = EXTRA.get((f["name"], lat), ()) if which == "A" else ()
    return times(lat, f["t_cut"], which=which, extra=extra)


def splits(result, lat, T):
    """For the tick that holds T: (arrivals before T, arrivals at or after T, generations before T,
    generations at or after T), counted over the first-contact records of that tick (via 1 / via 0)."""
    t, via = result.trace[2], result.trace[4]
    lo = (T // lat) * lat
    tick = (t >= lo) & (t < lo + lat)
    early = t < T
    return (int(np.count_nonzero(tick & early & (via == 1))), int(np.count_nonzero(tick & ~early & (via == 1))),
            int(np.count_nonzero(tick & early & (via == 0))), int(np.count_nonzero(tick & ~early & (via == 0))))


def gen_beats_arrival(result, links, lat):
    """The (node, id, t_gen, t_arrival) of every own generation that ORACLE A recorded as a first
    contact (via 0) while a peer's copy of the same id was in flight to that node and due later in the
    same tick: t_gen <= t_arrival, t_gen // lat == t_arrival // lat.  (Whoever first holds an id sends it
    to every peer, so the arrival time at v is the peer's first-contact time + lat.  The dropped arrival
    itself leaves no record.)  An engine's pull counts such an arrival and k_births takes it back."""
    node, sid, t, _hop, via = result.trace
    first = {(int(n), int(i)): int(x) for n, i, x in zip(node, sid, t)}
    peers = {}
    for a, b in zip(*links):
        peers.setdefault(int(a), set()).add(int(b))
        peers.setdefault(int(b), set()).add(int(a))
    out = []
    for n, i, x in zip(node[via == 0], sid[via == 0], t[via == 0]):
        n, i, x = int(n), int(i), int(x)
        for u in peers.get(n, ()):
            tu = first.get((u, i))
            if tu is not None and tu + lat >= x and (tu + lat) // lat == x // lat:
                out.append((n, i, x, tu + lat))
    return sorted(set(out))
