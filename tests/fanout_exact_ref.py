"""Exact-k fanout, the model: a numpy restatement of the rule in include/gossip.h
(gossip_engine_set_fanout_exact / _set_fanout_counts), level-synchronous per share, with Philox from
philox_ref.py, the directed copies from fanout_ref.copies and q from a per-row sort.  The independent
checker of the engine's exact mode; it shares no code with the library.  Test infrastructure only.

Sender u with D out-copies (v, c), c < mult(u, v), and the fanout count k[u], in tick T:
    x = Philox4x32-10((min(u,v), max(u,v), T, c), (seed & 0xffffffff, (seed >> 32) ^ 0x46414E4B))
    w = x[0] << 32 | x[1] if u < v else x[2] << 32 | x[3]
    q = the k[u]-th smallest of u's D draws;  selected = k[u] > 0 and (D <= k[u] or w <= q)
Faults (optional) as in faults_ref.py: the rule decides whether a Send is made, outages and loss whether
a made Send arrives.
"""
import numpy as np

import fanout_ref as F
import faults_ref as R
from philox_ref import philox4x32_10

KEY1 = 0x46414E4B  # "FANK"


def draws(seed, u, v, c, tick):
    """w(u -> v, c, tick) on arrays (broadcast): uint64 array."""
    u, v, c, tick = np.broadcast_arrays(*(np.asarray(x, np.uint64) for x in (u, v, c, tick)))
    ctr = np.stack([np.minimum(u, v), np.maximum(u, v), tick & np.uint64(0xFFFFFFFF), c], -1)
    key = np.empty(u.shape + (2,), np.uint64)
    key[..., 0] = int(seed) & 0xFFFFFFFF
    key[..., 1] = ((int(seed) >> 32) & 0xFFFFFFFF) ^ KEY1
    x = philox4x32_10(ctr, key)
    s = np.uint64(32)
    return np.where(u < v, (x[..., 0] << s) | x[..., 1], (x[..., 2] << s) | x[..., 3])


def select_row(w, k):
    """One sender's draws w (uint64, D of them) and its count k: bool array of the selected copies."""
    w = np.asarray(w, np.uint64)
    if k == 0:
        return np.zeros(len(w), bool)
    if len(w) <= k:
        return np.ones(len(w), bool)
    return w <= np.sort(w)[k - 1]


def row(seed, sender, receiver, copy, k, tick):
    """(selected, draws) of one sender's out-copies."""
    w = draws(seed, np.full(len(receiver), sender, np.uint64), receiver, copy, tick)
    return select_row(w, int(k)), w


def made(seed, u, v, c, rp, k, tick):
    """The tick's selection of every directed copy (u sorted: row x is [rp[x], rp[x + 1]))."""
    w = draws(seed, u, v, c, tick)
    k = np.asarray(k, np.int64)
    ws = w[np.lexsort((w, u))]  # every row sorted by its draws
    D = np.diff(rp)
    need = (k > 0) & (D > k)
    q = np.zeros(len(D), np.uint64)
    q[need] = ws[rp[:-1][need] + k[need] - 1]
    return (k[u] > 0) & ((D[u] <= k[u]) | (w <= q[u]))


def run(n, a, b, ev, lat, t_cut, k, seed, outages=(), loss_thr=0, loss_seed=1, hops=32):
    """The model's run, in the shape of faults_ref.run: dict(gen, recv, fwd, sent, processed, peers, trace,
    reach, arrivals, dropped, counted, lost_by_tick).  k: one count per node (a scalar broadcasts)."""
    assert len(np.unique(ev["share_id"])) == len(ev)
    k = np.broadcast_to(np.asarray(k, np.int64), (n,))
    u, v, c, peers = F.copies(n, a, b)
    rp = np.concatenate([[0], np.cumsum(np.bincount(u, minlength=n))])
    outages = [tuple(int(x) for x in o) for o in outages]
    made_c, lost_c, down_c = {}, {}, {}

    def made_of(tick):
        if tick not in made_c:
            made_c[tick] = made(seed, u, v, c, rp, k, tick)
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
    dropped = 0
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
        seen = np.zeros(n, bool)
        seen[s] = True
        front = np.array([s], np.int64)
        h = 0
        while len(front):
            tick = tick0 + h
            idx = np.concatenate([np.arange(rp[x], rp[x + 1]) for x in front])
            idx = idx[made_of(tick)[idx]]
            np.add.at(sent, u[idx], 1)  # made and counted, whatever becomes of it
            idx = idx[~lost_of(tick)[idx] & ~down_of(tick + 1)[v[idx]]]
            h += 1
            at = t + h * lat
            new = np.unique(v[idx])
            new = new[~seen[new]]
            if at >= t_cut or not len(new):
                break
            seen[new] = True
            recv[new] += 1
            reach[e, min(h, hops - 1)] += len(new)
            tn.append(new), ti.append(np.full(len(new), sid)), tt.append(np.full(len(new), at // lat))
            th.append(np.full(len(new), h)), tv.append(np.ones(len(new), np.int64))
            arr.append(np.full(len(new), at))
            front = new
    cat = lambda xs, dt: np.concatenate([np.asarray(x, np.int64) for x in xs]).astype(dt) if xs else np.zeros(0, dt)
    trace = (cat(tn, np.uint32), cat(ti, np.uint32), cat(tt, np.int64), cat(th, np.uint32), cat(tv, np.uint8))
    return dict(gen=gen, recv=recv, fwd=recv.copy(), processed=gen + recv, sent=sent, peers=peers, trace=trace,
                reach=reach, arrivals=cat(arr, np.int64), dropped=dropped, counted=counted, lost_by_tick=dict(lost_c))


def snapshot_total(res, ev, t_ns):
    """Total processed at a snapshot time: the generations that happened and the first receptions before t_ns."""
    return int(np.sum((ev["ns"] < t_ns) & res["counted"])) + int(np.sum(res["arrivals"] < t_ns))
