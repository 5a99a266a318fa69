#!/usr/bin/env python3
"""bench.py's workload with reach profiles on (GOSSIP_F_REACH): the cost figures of DESIGN section 6.

    python tools/bench_reach.py [bench.py arguments, default: --gpus 1 --steps 20 --warmup 5]
    rocprofv3 --pmc <counters> -d DIR -o run --output-format csv -- python tools/bench_reach.py

bench.py runs unchanged.  The flag is switched on through the environment (GOSSIP_REACH=1, read by
gossip_engine_create), so nothing about how bench.py creates its engines matters.  bench.py's JSON
line has no reach counters, so this wrapper also wraps Engine.counters() to print, at each read, a
line "REACH_PROBE {json}" on stderr with them beside the pull phase's.  That part depends on
bench.py reading counters() through gossip.Engine before reset_timing and after its timed ticks (as
run_shards does): the second line of each shard then holds the timed ticks alone -- reach_ms / steps
= the pass per tick, reach_slots_ms its k_reach_slots part, reach_bytes / reach_ms the rate it
loaded at.  Without those reads the run still measures the flag-on bench value; only the probe
lines are missing.
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


def _counters_probe(self):
    c = _counters(self)
    print("REACH_PROBE " + json.dumps(dict(
        ticks=c.ticks, reach_launches=c.reach_launches, reach_ms=c.reach_ms, reach_slots_ms=c.reach_slots_ms,
        reach_bytes=c.reach_bytes, pull_phase_ms=c.pull_phase_ms, pull_ms=c.pull_ms, young_ms=c.young_ms,
        pull_launches=c.pull_launches, words_hw=c.words_hw,
        reach_ledger=[(r.arg, r.launches) for r in self.launches() if r.kernel == gossip.K_REACH])),
        file=sys.stderr, flush=True)
    return c


def main():
    gossip.Engine.counters = _counters_probe
    sys.argv = ["bench.py"] + (sys.argv[1:] or ["--gpus", "1", "--steps", "20", "--warmup", "5"])
    runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")


if __name__ == "__main__":
    main()
