#!/usr/bin/env python3
"""bench.py's workload under fault injection: the cost of the count pass with faults.

    python tools/bench_faults.py [--fanout 8] [--down 0.1] [--loss 0.1] [--seed 1] [--configs fanout,down,loss,both]
                                 [--out FILE.json] [-- bench.py arguments, default: --gpus 1 --steps 20 --warmup 5]

bench.py runs unchanged, once per configuration, all in one run of one build:
    fanout   the thinning passes with fanout only (k_fanout_count: what tools/bench_fanout.py measures)
    down     the same with a random --down fraction of the nodes down for the whole run
    loss     the same with message loss --loss
    both     outages and loss
Engine.set_schedule is wrapped as in tools/bench_fanout.py: it calls set_fanout, then the fault setters
(after the graph, before the schedule), and renumbers the share ids with gossip.unique_ids.  Reach
profiles are on (GOSSIP_REACH=1), as there.  Engine.counters() is wrapped to print, at each read, a line
"FAULTS_PROBE {json}" on stderr; a shard's line read after its reset_timing holds the timed ticks alone:
fanout_ms / fanout_launches = the thinning per tick (count pass + scan + compact pass, HIP events,
GOSSIP_F_TIMING), and the fault counters of those ticks.  With --out the timed probes of every
configuration go to one JSON file, with ms per tick summed over the run's shards and its ratio to the
fanout-only run of the same build.  With nodes down bench.py ends in its own check "shard coverage broken"
after the timed ticks: its shards did not generate every event of the slice, which is what an outage
does (dropped generations); the probes are complete by then and the message is kept as bench_exit.
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
_state = dict(config="fanout", k=8, down=0.1, loss=0.1, seed=1, probes=[], engines=0)


def _set_schedule_faults(self, ev):
    cfg = _state["config"]
    self.set_fanout(_state["k"], _state["seed"])
    if cfg in ("down", "both"):
        self.set_outages(*gossip.crash_outages(self.n, _state["down"], 0, seed=_state["seed"]))
    if cfg in ("loss", "both"):
        self.set_link_loss(float(_state["loss"]), _state["seed"] + 1)
    _set_schedule(self, gossip.unique_ids(ev))


def _counters_probe(self):
    c = _counters(self)
    f, x = self.fanout_counters(), self.fault_counters()
    self._faults_reads = getattr(self, "_faults_reads", 0) + 1
    if self._faults_reads == 1:
        self._faults_engine = _state["engines"]
        _state["engines"] += 1
    p = dict(config=_state["config"], engine=self._faults_engine, read=self._faults_reads - 1,
             after_reset=bool(getattr(self, "_faults_reset", False)), ticks=c.ticks, fanout_launches=f.launches, fanout_ms=f.ms,
             fanout_bytes=f.bytes, fanout_entries=f.entries, selected_in=f.selected_in, selected_out=f.selected_out,
             fanout_ms_per_tick=f.ms / f.launches if f.launches else None,
             fault_launches=x.launches, down_node_ticks=x.down_node_ticks, lost_copies=x.lost_copies, down_copies=x.down_copies,
             dropped_generations=x.dropped_generations,
             pull_phase_ms=c.pull_phase_ms, pull_bytes_moved=c.pull_bytes_moved, edge_events=c.edge_events, words_hw=c.words_hw,
             device_bytes=c.device_bytes,
             fanout_ledger=[(r.arg, r.launches, r.strided) for r in self.launches() if r.kernel == gossip.K_FANOUT])
    _state["probes"].append(p)
    print("FAULTS_PROBE " + json.dumps(p), file=sys.stderr, flush=True)
    return c


def _reset_timing_probe(self):
    self._faults_reset = True
    _reset_timing(self)


def main():
    argv = sys.argv[1:]
    rest = []
    if "--" in argv:
        argv, rest = argv[:argv.index("--")], argv[argv.index("--") + 1:]
    configs, out = ["fanout", "down", "loss", "both"], None
    i = 0
    while i < len(argv):
        if argv[i] == "--fanout":
            _state["k"] = int(argv[i + 1])
        elif argv[i] == "--down":
            _state["down"] = float(argv[i + 1])
        elif argv[i] == "--loss":
            _state["loss"] = float(argv[i + 1])
        elif argv[i] == "--seed":
            _state["seed"] = int(argv[i + 1], 0)
        elif argv[i] == "--configs":
            configs = argv[i + 1].split(",")
        elif argv[i] == "--out":
            out = argv[i + 1]
        else:
            raise SystemExit(__doc__)
        i += 2
    if not set(configs) <= {"fanout", "down", "loss", "both"}:
        raise SystemExit(__doc__)
    gossip.Engine.counters = _counters_probe
    gossip.Engine.set_schedule = _set_schedule_faults
    gossip.Engine.reset_timing = _reset_timing_probe
    bench_args = rest or ["--gpus", "1", "--steps", "20", "--warmup", "5"]
    runs = []
    for cfg in configs:
        _state.update(config=cfg, probes=[], engines=0)
        sys.argv = ["bench.py"] + bench_args
        bench_exit = None
        try:
            runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
        except SystemExit as e:
            # bench.py checks that its shards generated every event of the slice: with nodes down they do not,
            # by design (dropped generations), and it stops after the timed ticks -- the probes are complete
            if e.code not in (0, None) and not (cfg in ("down", "both") and any(p["after_reset"] for p in _state["probes"])):
                raise
            bench_exit = None if e.code in (0, None) else str(e.code)
        last = {}  # per engine: the last read after its reset_timing holds the timed ticks alone
        for p in _state["probes"]:
            last[(p["engine"], p["after_reset"])] = p
        timed = [p for (e, a), p in sorted(last.items()) if a]
        launches = sum(p["fanout_launches"] for p in timed)
        runs.append(dict(config=cfg, fanout=_state["k"], down=_state["down"] if cfg in ("down", "both") else 0.0,
                         loss=_state["loss"] if cfg in ("loss", "both") else 0.0, seed=_state["seed"], shards=len(timed),
                         thinning_ms_per_shard_tick=sum(p["fanout_ms"] for p in timed) / launches if launches else None,
                         bench_exit=bench_exit,
                         timed=timed))
    base = next((r["thinning_ms_per_shard_tick"] for r in runs if r["config"] == "fanout"), None)
    for r in runs:
        r["vs_fanout_only"] = r["thinning_ms_per_shard_tick"] / base if base and r["thinning_ms_per_shard_tick"] else None
        print(f"FAULTS_RESULT {r['config']}: {r['thinning_ms_per_shard_tick']} ms per shard-tick over {r['shards']} shard(s), "
              f"x{r['vs_fanout_only']} of fanout only", file=sys.stderr, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(dict(bench_args=bench_args, runs=runs), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
