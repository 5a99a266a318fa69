"""Fault injection, the model: a numpy restatement of the semantics in include/gossip.h
(gossip_engine_set_outages / gossip_engine_set_link_loss), level-synchronous per share, on top of the
fanout model (fanout_ref.py: the copies, the selection rule) with Philox from philox_ref.py.  The
independent checker of the engine's fault mode.  Test infrastructure only.

Ticks: a share generated at g is sent in tick g // lat; a first arrival at hop h happens in tick
g // lat + h and forwards in that tick; Sends made in tick T are pulled in tick T + 1.
  outages   (node, tick_from, tick_to) triples, half-open, absolute ticks, in any order, overlapping or
            not (the model never merges them: a node is down in t iff some interval holds t).  A
            generation in a down tick of its node does not happen.  A Send u -> v made in T delivers only
            if v is up in T + 1; it is made and counted in sent either way.
  loss      a Send u -> v, copy c, made in tick T is lost iff
                y = Philox4x32-10((min(u,v), max(u,v), T, c), (seed & 0xffffffff, (seed >> 32) ^ 0x4C4F5353))
                w = y[0] if u < v else y[1];  lost = loss_thr == 0xffffffff or w < loss_thr
            made and counted, delivers nothing.
  fanout    decides whether a Send is made (fanout_ref.selected); faults whether a made Send arrives.
"""
import numpy as np

import fanout_ref as F
from philox_ref import philox4x32_10

ALWAYS = 0xFFFFFFFF
LOSS_KEY1 = 0x4C4F5353


def lost(seed, u, v, c, tick, thr):
    """The loss rule on arrays (broadcast): bool array."""
    u, v, c, tick, thr = np.broadcast_arrays(*(np.asarray(x, np.uint64) for x in (u, v, c, tick, thr)))
    ctr = np.stack([np.minimum(u, v), np.maximum(u, v), tick & np.uint64(0xFFFFFFFF), c], -1)
    key = np.empty(u.shape + (2,), np.uint64)
    key[..., 0] = int(seed) & 0xFFFFFFFF
    key[..., 1] = ((int(seed) >> 32) & 0xFFFFFFFF) ^ LOSS_KEY1
    y = philox4x32_10(ctr, key)
    w = np.where(u < v, y[..., 0], y[..., 1])
    return (thr == np.uint64(ALWAYS)) | (w < thr)


def down_mask(n, outages, tick):
    """bool[n]: the nodes down in `tick`."""
    d = np.zeros(n, bool)
    for node, t0, t1 in outages:
        if int(t0) <= tick < int(t1):
            d[int(node)] = True
    return d


class _Draws:
    """Per tick and directed copy: made (fanout), lost, receiver down in tick + 1 -- shared by all shares."""

    def __init__(self, n, u, v, c, thr, seed, outages, loss_thr, loss_seed):
        self.n, self.u, self.v, self.c = n, u, v, c
        self.thr, self.seed, self.outages = thr, seed, [tuple(int(x) for x in o) for o in outages]
        self.loss_thr, self.loss_seed = int(loss_thr), loss_seed
        self._made, self._lost, self._down = {}, {}, {}

    def made(self, tick):
        if tick not in self._made:
            self._made[tick] = F.selected(self.seed, self.u, self.v, self.c, tick, self.thr[self.u])
        return self._made[tick]

    def lost(self, tick):
        if tick not in self._lost:
            self._lost[tick] = (lost(self.loss_seed, self.u, self.v, self.c, tick, self.loss_thr) if self.loss_thr
                                else np.zeros(len(self.u), bool))
        return self._lost[tick]

    def down(self, tick):
        if tick not in self._down:
            self._down[tick] = down_mask(self.n, self.outages, tick)
        return self._down[tick]


def run(n, a, b, ev, lat, t_cut, thr, seed, outages=(), loss_thr=0, loss_seed=1, hops=32):
    """The model's run.  fanout_ref.run's dictionary (gen, recv, fwd, sent, processed, peers, trace, reach,
    arrivals) plus dropped (generations in a down tick of their node), counted (bool per event: it
    happened) and lost_by_tick (tick -> the loss draw of every directed copy, for the ticks a share was
    sent in)."""
    assert len(np.unique(ev["share_id"])) == len(ev)
    thr = np.asarray(thr, np.uint64)
    u, v, c, peers = F.copies(n, a, b)
    rp = np.concatenate([[0], np.cumsum(np.bincount(u, minlength=n))])
    dr = _Draws(n, u, v, c, thr, seed, outages, loss_thr, loss_seed)
    gen = np.zeros(n, np.uint32)
    recv = np.zeros(n, np.uint32)
    sent = np.zeros(n, np.uint64)
    reach = np.zeros((len(ev), hops), np.uint32)
    counted = np.zeros(len(ev), bool)
    tn, ti, tt, th, tv, arr = [], [], [], [], [], []
    dropped = 0
    for k in range(len(ev)):
        t, s, sid = int(ev["ns"][k]), int(ev["node"][k]), int(ev["share_id"][k])
        assert t < t_cut
        tick0 = t // lat
        if dr.down(tick0)[s]:
            dropped += 1
            continue  # down in its generation tick: does not happen
        if peers[s] == 0:
            continue  # no peers: not counted, nothing sent
        counted[k] = True
        gen[s] += 1
        tn.append([s]), ti.append([sid]), tt.append([tick0]), th.append([0]), tv.append([0])
        reach[k, 0] += 1
        seen = np.zeros(n, bool)
        seen[s] = True
        front = np.array([s], np.int64)
        h = 0
        while len(front):
            tick = tick0 + h
            idx = np.concatenate([np.arange(rp[x], rp[x + 1]) for x in front])
            idx = idx[dr.made(tick)[idx]]
            np.add.at(sent, u[idx], 1)  # made and counted, whatever becomes of it
            idx = idx[~dr.lost(tick)[idx] & ~dr.down(tick + 1)[v[idx]]]
            h += 1
            at = t + h * lat
            new = np.unique(v[idx])
            new = new[~seen[new]]
            if at >= t_cut or not len(new):
                break
            seen[new] = True
            recv[new] += 1
            reach[k, min(h, hops - 1)] += len(new)
            tn.append(new), ti.append(np.full(len(new), sid)), tt.append(np.full(len(new), at // lat))
            th.append(np.full(len(new), h)), tv.append(np.ones(len(new), np.int64))
            arr.append(np.full(len(new), at))
            front = new
    cat = lambda xs, dt: np.concatenate([np.asarray(x, np.int64) for x in xs]).astype(dt) if xs else np.zeros(0, dt)
    trace = (cat(tn, np.uint32), cat(ti, np.uint32), cat(tt, np.int64), cat(th, np.uint32), cat(tv, np.uint8))
    return dict(gen=gen, recv=recv, fwd=recv.copy(), processed=gen + recv, sent=sent, peers=peers, trace=trace,
                reach=reach, arrivals=cat(arr, np.int64), dropped=dropped, counted=counted,
                lost_by_tick=dict(dr._lost))


def snapshot_total(res, ev, t_ns):
    """Total processed at a snapshot time: the generations that happened and the first receptions before t_ns."""
    return int(np.sum((ev["ns"] < t_ns) & res["counted"])) + int(np.sum(res["arrivals"] < t_ns))


def fault_counts(n, a, b, thr, seed, outages, loss_thr, loss_seed, ticks):
    """The engine's GPU-side fault counters over the thinned ticks `ticks` (every tick of the run thins every
    peer list, whether or not a share is on it): (down_node_ticks, lost_copies, down_copies)."""
    u, v, c, _ = F.copies(n, a, b)
    dr = _Draws(n, u, v, c, np.asarray(thr, np.uint64), seed, outages, loss_thr, loss_seed)
    dnt = lc = dc = 0
    for t in ticks:
        made, dn = dr.made(t), dr.down(t + 1)
        dnt += int(dn.sum())
        dc += int((made & dn[v]).sum())
        lc += int((made & ~dn[v] & dr.lost(t)).sum())
    return dnt, lc, dc
