#!/usr/bin/env python3
"""bench.py's workload under fanout-limited gossip: the cost figures of DESIGN section 6.

    python tools/bench_fanout.py [--fanout 2,4,8] [--fanout-seed 1] [--exact] [--out FILE.json]
                                 [-- bench.py arguments, default: --gpus 1 --steps 20 --warmup 5]

bench.py runs unchanged, once per fanout (a fanout of 0 in the list runs the plain flood the same way:
the figures to compare against).  Engine.set_schedule is wrapped: it calls
set_fanout(k, seed) -- with --exact, set_fanout_exact(k, seed): exactly k Sends per node and tick, with
k_fanout_kth in the measured passes -- first (after the graph, before the schedule, as the mode requires) and renumbers
the share ids with gossip.unique_ids -- bench.py's synthetic schedule reuses ids above 128,849 nodes,
and fanout mode needs them unique.  Reach profiles are switched on through the environment
(GOSSIP_REACH=1), as tools/bench_reach.py does.  Engine.counters() is wrapped to print, at each read,
a line "FANOUT_PROBE {json}" on stderr: bench.py reads counters() before reset_timing and after its
timed ticks (run_shards), so a shard's line read after its reset_timing holds the timed ticks alone (each probe says
which engine it read, its place among that engine's reads and whether reset_timing came before) -- fanout ms /
launches = k_fanout per tick (count pass + scan + compact pass, HIP events, GOSSIP_F_TIMING), bytes
its traffic model, pull_phase_ms and pull_bytes_moved the pull phase over the thinned lists, col_ids
the peer ids k_pull loaded (4 B each: the peer-list part of its bytes; a flood loads every entry), and
reach_totals the first contacts by hop so far.  With --out, the timed probes of every fanout go to one
JSON file.  The bench value printed by bench.py is the fanout run's, not the flagship's.
"""
import json
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["GOSSIP_REACH"] = "1"
sys.path.insert(0, os.path.join(ROOT, "p2p-gossip-simulation-ns3_amd"))
import gossip  # noqa: E402

_counters = gossip.Engine.counters
_set_schedule = gossip.Engine.set_schedule
_reset_timing = gossip.Engine.reset_timing
_state = dict(k=0, seed=1, exact=False, probes=[], engines=0)


def _set_schedule_fanout(self, ev):
    if _state["k"]:  # (--fanout 0: the flood over the same renumbered schedule, for comparison)
        (self.set_fanout_exact if _state["exact"] else self.set_fanout)(_state["k"], _state["seed"])
    _set_schedule(self, gossip.unique_ids(ev))


def _counters_probe(self):
    c = _counters(self)
    f = self.fanout_counters()
    # (the read's place in this engine's life: bench.py's run_shards reads once before reset_timing and
    #  once after the timed ticks; other paths of bench.py may order their reads differently)
    self._fanout_reads = getattr(self, "_fanout_reads", 0) + 1
    if self._fanout_reads == 1:
        self._fanout_engine = _state["engines"]
        _state["engines"] += 1
    p = dict(fanout=_state["k"], exact=_state["exact"], engine=self._fanout_engine, read=self._fanout_reads - 1,
             after_reset=bool(getattr(self, "_fanout_reset", False)), ticks=c.ticks, fanout_launches=f.launches, fanout_ms=f.ms, fanout_bytes=f.bytes,
             fanout_entries=f.entries, selected_in=f.selected_in, selected_out=f.selected_out,
             fanout_ms_per_tick=f.ms / f.launches if f.launches else None,
             pull_phase_ms=c.pull_phase_ms, pull_ms=c.pull_ms, pull_launches=c.pull_launches,
             pull_bytes_moved=c.pull_bytes_moved, pull_col_ids=c.pull_col_ids, edge_events=c.edge_events,
             words_hw=c.words_hw, device_bytes=c.device_bytes,
             reach_totals=[int(x) for x in self.reach_totals()],
             fanout_ledger=[(r.arg, r.launches, r.strided) for r in self.launches() if r.kernel == gossip.K_FANOUT])
    _state["probes"].append(p)
    print("FANOUT_PROBE " + json.dumps(p), file=sys.stderr, flush=True)
    return c


def _reset_timing_probe(self):
    self._fanout_reset = True
    _reset_timing(self)


def main():
    argv = sys.argv[1:]
    rest = []
    if "--" in argv:
        argv, rest = argv[:argv.index("--")], argv[argv.index("--") + 1:]
    ks, seed, out = [2, 4, 8], 1, None
    i = 0
    while i < len(argv):
        if argv[i] == "--exact":
            _state["exact"] = True
            i += 1
            continue
        if argv[i] == "--fanout":
            ks = [int(x) for x in argv[i + 1].split(",")]
        elif argv[i] == "--fanout-seed":
            seed = int(argv[i + 1], 0)
        elif argv[i] == "--out":
            out = argv[i + 1]
        else:
            raise SystemExit(__doc__)
        i += 2
    gossip.Engine.counters = _counters_probe
    gossip.Engine.set_schedule = _set_schedule_fanout
    gossip.Engine.reset_timing = _reset_timing_probe
    runs = []
    for k in ks:
        _state.update(k=k, seed=seed, probes=[], engines=0)
        sys.argv = ["bench.py"] + (rest or ["--gpus", "1", "--steps", "20", "--warmup", "5"])
        try:
            runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
        except SystemExit as e:
            if e.code not in (0, None):
                raise
        # per engine: the last read after its reset_timing holds the timed ticks alone, the last one
        # before it the ramp (every probe carries its engine and its place in that engine's reads)
        last = {}
        for p in _state["probes"]:
            last[(p["engine"], p["after_reset"])] = p
        runs.append(dict(fanout=k, seed=seed, exact=_state["exact"], timed=[p for (e, a), p in sorted(last.items()) if a],
                         ramp=[p for (e, a), p in sorted(last.items()) if not a]))
    if out:
        with open(out, "w") as f:
            json.dump(dict(bench_args=rest or ["--gpus", "1", "--steps", "20", "--warmup", "5"], runs=runs), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
