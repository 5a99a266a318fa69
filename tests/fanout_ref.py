"""Fanout-limited gossip, the model: a numpy restatement of the semantics in include/gossip.h
(gossip_engine_set_fanout), level-synchronous per share, with Philox from philox_ref.py.  The
independent checker of the engine's fanout mode.  Test infrastructure only.

A Send u -> v, copy c < mult(u, v), made in tick T = floor(send time / lat) happens iff
    x = Philox4x32-10((min(u,v), max(u,v), T, c), (seed & 0xffffffff, (seed >> 32) ^ 0x46414E4F))
    w = x[0] if u < v else x[1];  selected = thr[u] == 0xffffffff or w < thr[u]
A share generated at g is sent in tick g // lat; a first arrival at hop h (time g + h * lat, counted
iff before t_cut) forwards in tick g // lat + h.  Unique share ids.
"""
import numpy as np

from philox_ref import philox4x32_10

ALWAYS = 0xFFFFFFFF
KEY1 = 0x46414E4F


def selected(seed, u, v, c, tick, thr):
    """The rule on arrays (broadcast): bool array."""
    u, v, c, tick, thr = np.broadcast_arrays(*(np.asarray(x, np.uint64) for x in (u, v, c, tick, thr)))
    ctr = np.stack([np.minimum(u, v), np.maximum(u, v), tick & np.uint64(0xFFFFFFFF), c], -1)
    key = np.empty(u.shape + (2,), np.uint64)
    key[..., 0] = int(seed) & 0xFFFFFFFF
    key[..., 1] = ((int(seed) >> 32) & 0xFFFFFFFF) ^ KEY1
    x = philox4x32_10(ctr, key)
    w = np.where(u < v, x[..., 0], x[..., 1])
    return (thr == np.uint64(ALWAYS)) | (w < thr)


def thresholds(k, deg):
    """gossip_engine_set_fanout's thresholds for peer counts deg (sum of multiplicities)."""
    deg = np.asarray(deg, np.uint64)
    with np.errstate(divide="ignore"):
        t = (np.uint64(k) << np.uint64(32)) // np.maximum(deg, np.uint64(1))
    return np.where(deg <= np.uint64(k), np.uint64(ALWAYS), t).astype(np.uint32)


def copies(n, a, b):
    """Directed copies (u, v, c) of the link keys: every key (a, b) is one copy each way; the copies
    of one ordered pair are numbered 0, 1, ...  Returns u, v, c sorted by u, and the peer counts."""
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    u = np.concatenate([a, b])
    v = np.concatenate([b, a])
    o = np.lexsort((v, u))
    u, v = u[o], v[o]
    first = np.ones(len(u), bool)
    first[1:] = (u[1:] != u[:-1]) | (v[1:] != v[:-1])
    start = np.maximum.accumulate(np.where(first, np.arange(len(u)), 0))
    c = np.arange(len(u)) - start
    return u, v, c, np.bincount(u, minlength=n).astype(np.uint32)


def run(n, a, b, ev, lat, t_cut, thr, seed, hops=32):
    """The model's run.  Returns dict(gen, recv, fwd, sent, processed, peers, trace, reach, arrivals):
    trace = (node, share_id, tick, hop, via) of every first contact; reach = (len(ev), hops) first
    contacts per event and hop (last bin: every later hop); arrivals = (time, ) of every counted
    first reception (for snapshot totals)."""
    assert len(np.unique(ev["share_id"])) == len(ev)
    thr = np.asarray(thr, np.uint64)
    u, v, c, peers = copies(n, a, b)
    rp = np.concatenate([[0], np.cumsum(np.bincount(u, minlength=n))])
    gen = np.zeros(n, np.uint32)
    recv = np.zeros(n, np.uint32)
    sent = np.zeros(n, np.uint64)
    reach = np.zeros((len(ev), hops), np.uint32)
    tn, ti, tt, th, tv, arr = [], [], [], [], [], []
    sel_cache = {}

    def sel_of(tick):  # the tick's draw of every directed copy: shared by all shares of the tick
        if tick not in sel_cache:
            sel_cache[tick] = selected(seed, u, v, c, tick, thr[u])
        return sel_cache[tick]

    for k in range(len(ev)):
        t, s, sid = int(ev["ns"][k]), int(ev["node"][k]), int(ev["share_id"][k])
        assert t < t_cut
        if peers[s] == 0:
            continue  # no peers: not counted, nothing sent
        gen[s] += 1
        tick0 = t // lat
        tn.append([s]), ti.append([sid]), tt.append([tick0]), th.append([0]), tv.append([0])
        reach[k, 0] += 1
        seen = np.zeros(n, bool)
        seen[s] = True
        front = np.array([s], np.int64)
        h = 0
        while len(front):
            sel = sel_of(tick0 + h)
            idx = np.concatenate([np.arange(rp[x], rp[x + 1]) for x in front])
            idx = idx[sel[idx]]
            np.add.at(sent, u[idx], 1)
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
                reach=reach, arrivals=cat(arr, np.int64))


def snapshot_total(res, ev, peers, t_ns):
    """Total processed at a snapshot time: counted generations and first receptions before t_ns."""
    g = int(np.sum((ev["ns"] < t_ns) & (peers[ev["node"]] > 0)))
    return g + int(np.sum(res["arrivals"] < t_ns))
