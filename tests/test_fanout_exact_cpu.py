"""Exact-k fanout, the parts that need no device: the rule of libgossip.so (gossip_fanout_exact_row)
against the model (fanout_exact_ref.py) on rows at every boundary, its uniformity over 4,000 ticks, the
model against the closed form of a flood at k >= degree, the invariant sent == min(k, peers) x processed,
csrc/fanout_kernel.h as pure host code (a stand-alone program with its own main,
tests/fanout_exact/fanout_exact_check.cpp, compiled with -fsanitize=address,undefined and run), and the
ABI mirror."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import fanout_exact_ref as X
import structured as S
from cases import L, T0
from conftest import PKG, ROOT

SEEDS = (1, 2, 0xFFFFFFFF, 0x1_0000_0001, 0x8000_0000_0000_0001, 0xFFFF_FFFF_FFFF_FFFF, 0xDEADBEEF_00000000)
TICKS = (0, 1, 1000, 12345678, 0xFFFFFFFE, 0xFFFFFFFF)
SENDERS = (9, 0, 0xFFFFFFFF, 0xFFFFFFFE, 0x80000000, 123456)
U64 = (1 << 64) - 1


def _rows():
    """(seed, sender, k, tick, receiver[], copy[]) rows: D in {1, k - 1, k, k + 1, 64, 65, 257} for k in
    {0, 1, 3, 8, 32}, every row of two or more copies with copies 0 and 1 of one peer, node ids near
    2^32 - 1, ticks up to 2^32 - 1, seeds with high bits set."""
    rng = np.random.default_rng(91)
    pool = np.concatenate([rng.choice(1 << 20, 300, replace=False) + 1000,
                           [1, 2, 0xFFFFFFFD, 0xFFFFFFFC, 0x7FFFFFFF, 0x80000001]]).astype(np.uint64)
    out = []
    i = 0
    for k in (0, 1, 3, 8, 32):
        for D in sorted({1, k - 1, k, k + 1, 64, 65, 257} - {0, -1}):
            for rep in range(3):
                sender = SENDERS[i % len(SENDERS)]
                recv = rng.choice(pool, D, replace=False)
                copy = np.zeros(D, np.uint64)
                if D >= 2:
                    recv[-1], copy[-1] = recv[-2], 1  # a parallel link: copies 0 and 1 of one peer
                out.append((SEEDS[i % len(SEEDS)], sender, k, TICKS[(i // 2) % len(TICKS)], recv, copy))
                i += 1
    return out


def test_library_row_equals_model(gossip):
    rows = _rows()
    assert len(rows) >= 90
    seen_d = set()
    for seed, sender, k, tick, recv, copy in rows:
        want_sel, want_w = X.row(seed, sender, recv, copy, k, tick)
        got_sel, got_w = gossip.fanout_exact_row(seed, sender, recv, copy, k, tick, draws=True)
        what = (hex(seed), sender, k, tick, len(recv))
        assert np.array_equal(got_w, want_w), what
        assert np.array_equal(got_sel, want_sel), what
        assert int(got_sel.sum()) == min(k, len(recv)), what  # exactly min(k, D): no tie in these rows
        assert np.array_equal(gossip.fanout_exact_row(seed, sender, recv, copy, k, tick), got_sel)  # draws=NULL
        seen_d.add((k, len(recv)))
    assert {(32, 31), (32, 32), (32, 33), (1, 1), (1, 2), (0, 257), (32, 257), (3, 65)} <= seen_d
    # one Philox call serves both directions, from different words: w(u -> v) != w(v -> u)
    a = gossip.fanout_exact_row(5, 3, [9], [0], 1, 7, draws=True)[1][0]
    b = gossip.fanout_exact_row(5, 9, [3], [0], 1, 7, draws=True)[1][0]
    assert int(a) != int(b)
    # an empty row
    assert gossip.fanout_exact_row(1, 3, [], [], 2, 0).size == 0


def test_uniformity(gossip):
    # sender 9, seven out-copies (two of them the copies of one peer), k = 3, ticks 0 .. 3999: a uniform
    # 3-subset takes every copy with probability 3/7 (sd over 4,000 ticks 0.0078) and every pair with 1/7
    # (sd 0.0055); the bounds are 5 sd
    recv = np.array([2, 5, 11, 11, 40, 77, 100000], np.uint32)
    copy = np.array([0, 0, 0, 1, 0, 0, 0], np.uint32)
    sel = np.array([gossip.fanout_exact_row(11, 9, recv, copy, 3, t) for t in range(4000)])
    assert np.all(sel.sum(axis=1) == 3)
    freq = sel.mean(axis=0)
    pairs = {(i, j): float((sel[:, i] & sel[:, j]).mean()) for i, j in itertools.combinations(range(7), 2)}
    print("copy frequencies", np.round(freq, 4), "worst", float(np.abs(freq - 3 / 7).max()))
    print("pair frequencies: worst deviation", max(abs(p - 1 / 7) for p in pairs.values()))
    assert np.all(np.abs(freq - 3 / 7) < 0.04)
    assert all(abs(p - 1 / 7) < 0.03 for p in pairs.values())


def _gnp(n=300, seed=5):
    rng = np.random.default_rng(seed)
    iu = np.triu_indices(n, 1)
    m = rng.random(len(iu[0])) < 6.0 / n
    return n, iu[0][m].astype(np.uint32), iu[1][m].astype(np.uint32), S.events(n, 6, 8, 9), S.t_cut_for(6)


def _inputs(name):
    if name == "ladder_parallel":
        f = S.family(name)
        return f["n"], f["a"], f["b"], f["ev"], f["t_cut"]
    return _gnp()


@pytest.mark.parametrize("name", ["ladder_parallel", "gnp"])
def test_model_is_the_flood_at_k_above_every_degree(name):
    # bfs_reference is pinned to ORACLE A by test_structured_cases.py
    n, a, b, ev, t_cut = _inputs(name)
    want = S.bfs_reference(n, a, b, ev, L, t_cut)
    kmax = int(want["peers"].max())
    for k in (kmax, kmax + 7):
        got = X.run(n, a, b, ev, L, t_cut, k, seed=3)
        for key in ("gen", "recv", "fwd", "sent", "processed", "peers"):
            assert np.array_equal(got[key], want[key]), (name, k, key)
        for x, y in zip(S.sorted_trace(got["trace"]), S.sorted_trace(want["trace"])):
            assert np.array_equal(x, y), name
    thin = X.run(n, a, b, ev, L, t_cut, 2, seed=3)
    assert thin["sent"].sum() < want["sent"].sum() and np.all(thin["recv"] <= want["recv"])
    assert np.array_equal(thin["gen"], want["gen"])


@pytest.mark.parametrize("name", ["ladder_parallel", "gnp"])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_model_invariant_sent_is_min_k_peers_times_processed(name, k):
    n, a, b, ev, t_cut = _inputs(name)
    for cut in (t_cut, T0 + 3 * L + 1, T0 + 60 * L):
        e = ev[ev["ns"] < cut]
        m = X.run(n, a, b, e, L, cut, k, seed=4)
        assert int(m["processed"].sum()) > len(e)
        assert np.array_equal(m["sent"], np.minimum(k, m["peers"]).astype(np.uint64) * m["processed"]), (name, k, cut)
    # per-node counts, zeros included
    kk = np.random.default_rng(2).integers(0, 5, n)
    m = X.run(n, a, b, ev, L, t_cut, kk, seed=4)
    assert np.array_equal(m["sent"], np.minimum(kk, m["peers"]).astype(np.uint64) * m["processed"])


def _bound_cases():
    """Hand-made draws for fanout_exact_bound: (k, draws, bound, count)."""
    top = U64
    return [
        (2, [5, 9, 9, 9, 30], 9, 4),                # ties at the k-th value: all tied draws pass, the count says so
        (3, [7, 7, 7, 7, 7, 7], 7, 6),              # every draw tied
        (2, [9, 30, 9, 5, 9], 9, 4),                # the same ties met in another order
        (3, [50, 40, 40, 30, 40, 20, 10], 30, 3),   # ties above the bound: evicted, not counted
        (2, [40, 40, 50, 30, 20], 30, 2),           # a tie evicted with its maximum
        (1, [0, 0, 4], 0, 2),                       # the draw 0, tied
        (1, [3, 0, 4], 0, 1),
        (2, [top, top, top], top, 3),               # 2^64 - 1 at the bound: all pass
        (2, [top, 1, top - 1, top], top - 1, 2),    # 2^64 - 1 above the bound 2^64 - 2
        (1, [top, 0], 0, 1),
        (3, [4, 2, 9], top, 3),                     # D = k: no selection, every copy
        (32, list(range(100, 132)), top, 32),       # D = k = 32
        (32, list(range(200, 100, -1)), 132, 32),   # k = 32 of 100, descending: every draw replaces the largest
        (8, [3] * 5 + [1, 2] + [3] * 5, 3, 12),
        (0, [1, 2, 3], top, 0),                     # k = 0: nothing is sent
        (0, [], top, 0),
        (5, [], top, 0),
    ]


def test_fanout_exact_check_asan_ubsan(tmp_path):
    rows = _rows()
    lines = []
    for seed, sender, k, tick, recv, copy in rows:
        sel, w = X.row(seed, sender, recv, copy, k, tick)
        lines.append(f"{seed} {sender} {k} {tick} {len(recv)}\n")
        lines += [f"{int(r)} {int(c)} {int(x)} {int(s)}\n" for r, c, x, s in zip(recv, copy, w, sel)]
    rfile = tmp_path / "rows.txt"
    rfile.write_text("".join(lines))
    cases = _bound_cases()
    for k, w, bound, count in cases:  # the expectations themselves, by the definition
        if k and len(w) > k:
            assert bound == sorted(w)[k - 1] and count == sum(x <= bound for x in w)
    bfile = tmp_path / "bounds.txt"
    bfile.write_text("".join(f"{k} {len(w)} " + " ".join(str(x) for x in w) + f" {bound} {count}\n" for k, w, bound, count in cases))
    exe = str(tmp_path / "fanout_exact_check")
    src = os.path.join(ROOT, "tests", "fanout_exact", "fanout_exact_check.cpp")
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                        "-I" + os.path.join(PKG, "csrc"), src, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    r = subprocess.run([exe, str(rfile), str(bfile)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert f"{len(rows)} rows" in r.stdout and f"{len(cases)} bounds: checks passed" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_fanout_exact_abi_mirror(gossip):
    lib = gossip.load_library()
    # the new symbols refuse NULL without a device
    assert lib.gossip_engine_set_fanout_exact(None, 3, 1) == gossip.E_INVAL
    assert lib.gossip_engine_set_fanout_counts(None, None, 1) == gossip.E_INVAL
    assert lib.gossip_fanout_exact_row(1, 0, 3, None, None, 1, 0, None, None) == gossip.E_INVAL
    assert lib.gossip_fanout_exact_row(1, 0, 0, None, None, 1, 0, None, None) == 0  # an empty row needs no arrays
    hdr = open(os.path.join(ROOT, "include", "gossip.h")).read()
    for name in ("gossip_engine_set_fanout_exact", "gossip_engine_set_fanout_counts", "gossip_fanout_exact_row"):
        assert re.search(rf"\bint {name}\(", hdr), name
    assert "0x46414E4B" in hdr
    # nothing existing is extended: the ledger constants and the struct sizes
    assert gossip.K_FANOUT == 6 and "#define GOSSIP_K_FANOUT 6" in hdr
    ledger = open(os.path.join(PKG, "csrc", "launch_ledger.h")).read()
    assert "LK_FANOUT = 6" in ledger and "kLaunchKernels = 7" in ledger
    assert C.sizeof(gossip.gossip_fanout_counters) == 48
    assert [f[0] for f in gossip.gossip_fanout_counters._fields_] == ["launches", "selected_in", "selected_out", "entries", "ms",
                                                                      "bytes"]
    assert [f[0] for f in gossip.gossip_counters._fields_][-4:] == ["reach_launches", "reach_ms", "reach_bytes",
                                                                   "reach_slots_ms"]
    kernel = open(os.path.join(PKG, "csrc", "fanout_kernel.h")).read()
    assert "kFanoutExactMax = 32" in kernel and "kFanoutExactKey1 = 0x46414E4Bu" in kernel
