"""The thinned peer lists of one tick, the model: what k_fanout_kth, the count pass, the scan and
k_fanout_compact (csrc/fanout_kernel.h) must leave in (rowptr_t, col_t) and, in exact mode, in the bound
table -- entry by entry, from the rule functions of the other models alone (fanout_ref.selected,
fanout_exact_ref.draws / made, faults_ref.lost / down_mask) on fanout_ref.copies.  No share enters: the
lists are a function of (graph, seeds, thresholds or counts, outages, loss, tick).  It shares no code with
the library.  Test infrastructure only.

Entry (row v, distinct peer u) of tick T:
    survives = any over c < mult(u -> v) of made(u -> v, c, T) and not lost(u -> v, c, T) and not down(v, T + 1)
made: the binomial rule with per-node thresholds (thr), the exact row rule (k), or always (neither).
"""
import numpy as np

import fanout_exact_ref as X
import fanout_ref as F
import faults_ref as R

ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


class Thinning:
    """The model of one engine configuration.  thr: per-node thresholds (binomial), k: per-node counts or a
    scalar (exact); neither: every Send is made (a faults-only flood)."""

    def __init__(self, n, a, b, thr=None, k=None, seed=1, outages=(), loss_thr=0, loss_seed=1):
        assert thr is None or k is None
        self.n, self.seed = int(n), seed
        self.u, self.v, self.c, self.peers = F.copies(n, a, b)
        self.rp = np.concatenate([[0], np.cumsum(np.bincount(self.u, minlength=n))]).astype(np.int64)
        self.thr = None if thr is None else np.asarray(thr, np.uint64)
        self.k = None if k is None else np.broadcast_to(np.asarray(k, np.int64), (n,)).copy()
        self.outages = [tuple(int(x) for x in o) for o in outages]
        self.loss_thr, self.loss_seed = int(loss_thr), loss_seed
        self.faults = bool(self.outages) or self.loss_thr != 0
        # the full lists: distinct (row v, peer u) pairs, rows in order, a row's peers ascending
        self.pair = np.unique(self.v.astype(np.int64) * n + self.u.astype(np.int64))
        self.full_row_ptr = np.concatenate([[0], np.cumsum(np.bincount(self.pair // n, minlength=n))]).astype(np.int64)
        self._ticks, self._counts = {}, {}

    # ---- the three rules, per directed copy ------------------------------------------------------------
    def made(self, T):
        if self.k is not None:
            return X.made(self.seed, self.u, self.v, self.c, self.rp, self.k, T)
        if self.thr is not None:
            return F.selected(self.seed, self.u, self.v, self.c, T, self.thr[self.u])
        return np.ones(len(self.u), bool)

    def lost(self, T):
        if not self.loss_thr:
            return np.zeros(len(self.u), bool)
        return R.lost(self.loss_seed, self.u, self.v, self.c, T, self.loss_thr)

    def down(self, T):
        """bool[n]: the nodes down in tick T."""
        return R.down_mask(self.n, self.outages, T)

    def bound(self, T):
        """(bound, mask) of exact mode: the k[u]-th smallest of u's D draws where D > k[u] >= 1, 2^64 - 1 where
        D <= k[u]; mask is False where k[u] = 0 (the bound means nothing there)."""
        w = X.draws(self.seed, self.u, self.v, self.c, T)
        D = np.diff(self.rp)
        out = np.full(self.n, ALL, np.uint64)
        for x in np.flatnonzero((self.k > 0) & (D > self.k)):
            out[x] = np.sort(w[self.rp[x]:self.rp[x + 1]])[self.k[x] - 1]
        return out, self.k > 0

    # ---- one tick ----------------------------------------------------------------------------------------
    def _compute(self, T):
        n = self.n
        made, lost, dn = self.made(T), self.lost(T), self.down(T + 1)
        arrives = made & ~lost & ~dn[self.v]
        keys = np.unique(self.v[arrives].astype(np.int64) * n + self.u[arrives].astype(np.int64))
        rows, col = keys // n, (keys % n).astype(np.int32)
        row_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
        res = dict(tick=T, made=made, lost=lost, down=dn, arrives=arrives, row_ptr=row_ptr, col=col,
                   survives=np.isin(self.pair, keys),  # per entry of the full lists (self.pair)
                   selected_in=len(keys), selected_out=int(made.sum()),
                   # the fault counters as faults_ref.fault_counts counts them
                   down_node_ticks=int(dn.sum()) if self.faults else 0,
                   down_copies=int((made & dn[self.v]).sum()),
                   lost_copies=int((made & ~dn[self.v] & lost).sum()))
        if self.k is not None:
            res["bound"], res["bound_mask"] = self.bound(T)
        return res

    def tick(self, T):
        """The expected lists of tick T: dict(row_ptr, col (rows concatenated, each ascending), survives,
        selected_in, selected_out, lost_copies, down_copies, down_node_ticks, made, lost, down, arrives[,
        bound, bound_mask])."""
        T = int(T)
        if T not in self._ticks:
            self._ticks[T] = self._compute(T)
        return self._ticks[T]

    COUNT_KEYS = ("selected_in", "selected_out", "lost_copies", "down_copies", "down_node_ticks")

    def counts(self, T):
        """The five totals of tick T (COUNT_KEYS), without keeping the tick's arrays."""
        T = int(T)
        if T not in self._counts:
            r = self._ticks[T] if T in self._ticks else self._compute(T)
            self._counts[T] = tuple(r[k] for k in self.COUNT_KEYS)
        return self._counts[T]

    def totals(self, ticks):
        """COUNT_KEYS summed over the ticks: dict."""
        s = np.zeros(len(self.COUNT_KEYS), np.int64)
        for T in ticks:
            s += np.array(self.counts(T), np.int64)
        return dict(zip(self.COUNT_KEYS, (int(x) for x in s)))


def rows_of(row_ptr, col):
    """(row_ptr, col) with every row's peers sorted: the engine may order a row its own way."""
    row_ptr = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)
    row = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    return col[np.lexsort((col, row))].astype(np.int32)


_CACHE = {}


def of_topology(topo, thr=None, k=None, seed=1, outages=(), loss_thr=0, loss_seed=1):
    """The model of an engine on `topo` (gossip.Topology), cached per configuration: parametrised tests that
    vary only engine options over one configuration draw every tick once."""
    n = topo.num_nodes
    kb = None if k is None else np.ascontiguousarray(np.broadcast_to(np.asarray(k, np.int64), (n,))).tobytes()
    tb = None if thr is None else np.ascontiguousarray(thr, np.uint32).tobytes()
    key = (id(topo), tb, kb, seed, tuple(tuple(int(x) for x in o) for o in outages), int(loss_thr), loss_seed)
    if key not in _CACHE:
        a, b = topo.links()
        _CACHE[key] = (topo, Thinning(n, a, b, thr=thr, k=k, seed=seed, outages=outages, loss_thr=loss_thr, loss_seed=loss_seed))
    return _CACHE[key][1]
