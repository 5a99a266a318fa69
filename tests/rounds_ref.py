"""Multi-round push, the model: a numpy restatement of the semantics in include/gossip.h
(gossip_engine_set_rounds), level-synchronous per share and per tick.  It reuses only the rule functions of
the other models: the directed copies and the binomial selection (fanout_ref), the exact row rule
(fanout_exact_ref.made), the loss draw and the outage test (faults_ref).  The independent checker of the
engine's rounds mode.  Test infrastructure only.

A node that first contacts a share in tick T (its generation, or a first reception) makes Sends of it in the
ticks T .. T + r - 1, each with that tick's selection, loss draw and receiver outage test (for tick + 1).
A column is alive in tick X iff g + (X - g // lat) * lat < t_cut; Sends of a dead column are not made.  A
sender that is down in X makes no Sends in X (none counted); its rounds elapse all the same.  A down node has
no first contacts.  r = 1 is faults_ref.run / fanout_exact_ref.run.
"""
import numpy as np

import fanout_exact_ref as X
import fanout_ref as F
import faults_ref as R

ALWAYS = 0xFFFFFFFF


def planes(r):
    """Counter planes of r rounds: bit_length(r - 1)."""
    return int(r - 1).bit_length()


def run(n, a, b, ev, lat, t_cut, r, thr=None, k=None, seed=1, outages=(), loss_thr=0, loss_seed=1, hops=32):
    """The model's run.  thr: per-node forward thresholds (binomial fanout; None with k None: a flood), or
    k: per-node exact fanout counts (a scalar broadcasts).  Returns faults_ref.run's dictionary plus resent:
    the (node, share, tick) Send-set members that were re-sends."""
    assert len(np.unique(ev["share_id"])) == len(ev) and r >= 1
    assert thr is None or k is None
    u, v, c, peers = F.copies(n, a, b)
    rp = np.concatenate([[0], np.cumsum(np.bincount(u, minlength=n))])
    outages = [tuple(int(x) for x in o) for o in outages]
    if k is not None:
        k = np.broadcast_to(np.asarray(k, np.int64), (n,))
    else:
        thr = np.full(n, ALWAYS, np.uint64) if thr is None else np.asarray(thr, np.uint64)
    made_c, lost_c, down_c = {}, {}, {}

    def made_of(tick):
        if tick not in made_c:
            made_c[tick] = X.made(seed, u, v, c, rp, k, tick) if k is not None else F.selected(seed, u, v, c, tick, thr[u])
        return made_c[tick]

    def lost_of(tick):
        if tick not in lost_c:
            lost_c[tick] = R.lost(loss_seed, u, v, c, tick, loss_thr) if loss_thr else np.zeros(len(u), bool)
        return lost_c[tick]

    def down_of(tick):
        if tick not in down_c:
            down_c[tick] = R.down_mask(n, outages, tick)
        return down_c[tick]

    gen = np.zeros(n, np.uint32)
    recv = np.zeros(n, np.uint32)
    sent = np.zeros(n, np.uint64)
    reach = np.zeros((len(ev), hops), np.uint32)
    counted = np.zeros(len(ev), bool)
    tn, ti, tt, th, tv, arr = [], [], [], [], [], []
    dropped = resent = 0
    for e in range(len(ev)):
        t, s, sid = int(ev["ns"][e]), int(ev["node"][e]), int(ev["share_id"][e])
        assert t < t_cut
        tick0 = t // lat
        if down_of(tick0)[s]:
            dropped += 1
            continue
        if peers[s] == 0:
            continue
        counted[e] = True
        gen[s] += 1
        tn.append([s]), ti.append([sid]), tt.append([tick0]), th.append([0]), tv.append([0])
        reach[e, 0] += 1
        contact = np.full(n, -1, np.int64)  # the tick of the first contact
        contact[s] = tick0
        last = tick0                        # the latest first contact so far
        tick = tick0
        while tick <= last + r - 1 and t + (tick - tick0) * lat < t_cut:  # someone has a round left; the column is alive
            has = (contact >= 0) & (contact > tick - r)
            senders = np.flatnonzero(has & ~down_of(tick))
            resent += int(np.sum(contact[senders] < tick))
            if len(senders):
                is_sender = np.zeros(n, bool)
                is_sender[senders] = True
                idx = np.flatnonzero(is_sender[u] & made_of(tick))  # the out-copies of the senders that are made
                np.add.at(sent, u[idx], 1)  # made and counted, whatever becomes of it
                idx = idx[~lost_of(tick)[idx] & ~down_of(tick + 1)[v[idx]]]
                h = tick + 1 - tick0
                at = t + h * lat
                new = np.unique(v[idx])
                new = new[contact[new] < 0]
                if at < t_cut and len(new):
                    contact[new] = tick + 1
                    last = tick + 1
                    recv[new] += 1
                    reach[e, min(h, hops - 1)] += len(new)
                    tn.append(new), ti.append(np.full(len(new), sid)), tt.append(np.full(len(new), at // lat))
                    th.append(np.full(len(new), h)), tv.append(np.ones(len(new), np.int64))
                    arr.append(np.full(len(new), at))
            tick += 1
    cat = lambda xs, dt: np.concatenate([np.asarray(x, np.int64) for x in xs]).astype(dt) if xs else np.zeros(0, dt)
    trace = (cat(tn, np.uint32), cat(ti, np.uint32), cat(tt, np.int64), cat(th, np.uint32), cat(tv, np.uint8))
    return dict(gen=gen, recv=recv, fwd=recv.copy(), processed=gen + recv, sent=sent, peers=peers, trace=trace,
                reach=reach, arrivals=cat(arr, np.int64), dropped=dropped, counted=counted, lost_by_tick=dict(lost_c),
                resent=resent)


def snapshot_total(res, ev, t_ns):
    """Total processed at a snapshot time: the generations that happened and the first receptions before t_ns."""
    return int(np.sum((ev["ns"] < t_ns) & res["counted"])) + int(np.sum(res["arrivals"] < t_ns))
