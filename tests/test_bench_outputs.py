"""bench.py --dump-outputs: the node sample is fixed by the node count alone, and the files are
float64 arrays of the sampled counters, summed over share shards, within 64 MB in all.  CPU only:
the bench module is loaded, nothing is launched."""
import importlib.util
import os

import numpy as np

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_output_nodes_are_a_fixed_sorted_sample():
    b = _bench()
    assert np.array_equal(b.output_nodes(1000), np.arange(1000))
    assert np.array_equal(b.output_nodes(b.OUTPUT_SAMPLE), np.arange(b.OUTPUT_SAMPLE))
    n = 10_000_000
    s = b.output_nodes(n)
    assert s.size == b.OUTPUT_SAMPLE and s[0] >= 0 and s[-1] < n
    assert np.all(np.diff(s) > 0)
    assert np.array_equal(s, b.output_nodes(n))
    assert s[-1] - s[0] > n // 2  # spread over the nodes, not a prefix


def test_compress_ramp_keeps_what_the_floods_depend_on(gossip):
    # workloads.compress_ramp: the slice itself untouched, every generation's node, id and phase
    # kept, per id every distance below the flood lifetime kept to the tick and every longer one
    # still at least that long, nothing before the new start or moved past t_lo - LIFE_TICKS
    import collections

    import gossip.workloads as W
    n = 3_000_000
    ev, info = W.slice_schedule(n, 77, W.SLICE_NS, W.SLICE_NS + 26 * W.L_NS, threads=8)
    assert info["earlier_same_id"] > 20
    t_lo = info["t_lo_ns"]
    cs, t_start = W.compress_ramp(ev, t_lo)
    assert W.T0_NS < t_start == (int(cs["ns"].min()) // W.L_NS - 1) * W.L_NS
    assert t_lo - t_start < 100 * W.L_NS
    assert np.array_equal(cs[cs["ns"] >= t_lo], ev[ev["ns"] >= t_lo])
    assert np.all(np.diff(cs["ns"]) >= 0)

    def key(e):
        return sorted(zip(e["node"].tolist(), e["share_id"].tolist(), (e["ns"] % W.L_NS).tolist()))
    assert key(cs) == key(ev)
    moved = np.sort(cs["ns"][cs["ns"] < t_lo]) - np.sort(ev["ns"][ev["ns"] < t_lo])
    assert int((cs["ns"] < t_lo).sum()) == info["earlier_same_id"] and moved.sum() > 0

    def ticks_by_id(e):
        d = collections.defaultdict(list)
        for t, sid in zip((e["ns"] // W.L_NS).tolist(), e["share_id"].tolist()):
            d[sid].append(t)
        return d
    early_ids = set(ev["share_id"][ev["ns"] < t_lo].tolist())
    a, b = ticks_by_id(ev), ticks_by_id(cs)
    lo_tick = t_lo // W.L_NS
    for sid in early_ids:
        ta, tb = a[sid], b[sid]  # ascending: both arrays are sorted by time
        assert len(ta) == len(tb)
        for i in range(len(ta)):
            assert tb[i] >= ta[i] and (tb[i] == ta[i] or tb[i] <= lo_tick - W.LIFE_TICKS)
        for i in range(len(ta) - 1):
            da, db = ta[i + 1] - ta[i], tb[i + 1] - tb[i]
            assert db == da if da < W.LIFE_TICKS else db >= W.LIFE_TICKS, (sid, ta, tb)


def test_dump_outputs_writes_float64_sums_within_the_size_limit(gossip, tmp_path):
    b = _bench()
    n = 3 * b.OUTPUT_SAMPLE
    nodes = b.output_nodes(n)
    rng = np.random.default_rng(7)
    shard = [gossip.Stats(*(rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint64 if k == "sent" else np.uint32)
                            for k in b.OUTPUT_NAMES)) for _ in range(2)]
    shard[1].peers[:] = shard[0].peers
    shard[1].sockets[:] = shard[0].sockets
    st = None
    for s in shard:
        st = b.add_stats(st, b.sample_stats(s, nodes))
    d = str(tmp_path / "out")
    b.dump_outputs(d, st, nodes)
    total = 0
    for k in b.OUTPUT_NAMES:
        a = np.load(os.path.join(d, f"{k}.npy"))
        total += os.path.getsize(os.path.join(d, f"{k}.npy"))
        assert a.dtype == np.float64 and a.shape == nodes.shape
        want = getattr(shard[0], k)[nodes].astype(np.float64)
        if k not in ("peers", "sockets"):  # (u32 + u32 must not wrap)
            want = want + getattr(shard[1], k)[nodes].astype(np.float64)
        assert np.array_equal(a, want), k
    assert np.array_equal(np.load(os.path.join(d, "sample_nodes.npy")), nodes.astype(np.float64))
    total += os.path.getsize(os.path.join(d, "sample_nodes.npy"))
    assert total <= 64 * 10**6
