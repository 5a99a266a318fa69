#!/usr/bin/env python3
"""bench.py's workload under multi-round push: the cost figures of DESIGN section 6.

    python tools/bench_rounds.py [--rounds 1,2,4] [--fanout-exact 4] [--loss 0,0.1] [--seed 1] [--out FILE.json]
                                 [-- bench.py arguments, default: --gpus 1 --steps 20 --warmup 5]

bench.py runs unchanged, once per (loss, rounds) pair, at one fixed exact fanout.  Engine.set_schedule is
wrapped: it calls set_fanout_exact(k, seed), set_link_loss(p, seed) where p > 0 and set_rounds(r) first (after
the graph, before the schedule, as the modes require; rounds 1 makes no set_rounds call: the figures to compare
against) and renumbers the share ids with gossip.unique_ids, as tools/bench_fanout.py does.  Reach profiles are
switched on through the environment (GOSSIP_REACH=1).  Engine.counters() is wrapped to print, at each read, a
line "ROUNDS_PROBE {json}" on stderr: bench.py reads counters() before reset_timing and after its timed ticks,
so a shard's line read after its reset_timing holds the timed ticks alone -- rounds_ms / rounds_launches =
k_rounds per tick (HIP events, GOSSIP_F_TIMING), rounds_bytes the bytes the kernel counted, rounds_gbps the two
divided, fanout_ms the thinning passes, pull_phase_ms the pull phase, and reach_totals the first contacts by
hop so far (coverage = their sum / (generations x nodes)).  With --out, the timed probes of every run go to
one JSON file.  The bench value printed by bench.py is the run's own, not the flagship's.
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
_state = dict(r=1, k=4, loss=0.0, seed=1, probes=[], engines=0)


def _set_schedule_rounds(self, ev):
    self.set_fanout_exact(_state["k"], _state["seed"])
    if _state["loss"] > 0.0:
        self.set_link_loss(float(_state["loss"]), _state["seed"])
    if _state["r"] > 1:
        self.set_rounds(_state["r"])
    _set_schedule(self, gossip.unique_ids(ev))


def _counters_probe(self):
    c = _counters(self)
    f, rc = self.fanout_counters(), self.rounds_counters()
    self._rounds_reads = getattr(self, "_rounds_reads", 0) + 1
    if self._rounds_reads == 1:
        self._rounds_engine = _state["engines"]
        _state["engines"] += 1
    tot = [int(x) for x in self.reach_totals()]
    p = dict(rounds=_state["r"], fanout_exact=_state["k"], loss=_state["loss"], engine=self._rounds_engine,
             read=self._rounds_reads - 1, after_reset=bool(getattr(self, "_rounds_reset", False)), ticks=c.ticks, nodes=self.n,
             rounds_launches=rc.launches, rounds_ms=rc.ms, rounds_bytes=rc.bytes, resent_bits=rc.resent_bits,
             rows_visited=rc.rows_visited,
             rounds_ms_per_tick=rc.ms / rc.launches if rc.launches else None,
             rounds_gbps=rc.bytes / rc.ms / 1e6 if rc.ms else None,
             fanout_launches=f.launches, fanout_ms=f.ms, fanout_ms_per_tick=f.ms / f.launches if f.launches else None,
             pull_phase_ms=c.pull_phase_ms, pull_ms=c.pull_ms, pull_launches=c.pull_launches,
             pull_bytes_moved=c.pull_bytes_moved, edge_events=c.edge_events, generations=c.generations,
             receptions=c.receptions, words_hw=c.words_hw, words_cap=c.words_cap, device_bytes=c.device_bytes,
             reach_totals=tot,
             rounds_ledger=[(x.arg, x.launches, x.strided) for x in self.launches() if x.kernel == gossip.K_ROUNDS])
    _state["probes"].append(p)
    print("ROUNDS_PROBE " + json.dumps(p), file=sys.stderr, flush=True)
    return c


def _reset_timing_probe(self):
    self._rounds_reset = True
    _reset_timing(self)


def main():
    argv = sys.argv[1:]
    rest = []
    if "--" in argv:
        argv, rest = argv[:argv.index("--")], argv[argv.index("--") + 1:]
    rs, losses, out = [1, 2, 4], [0.0, 0.1], None
    i = 0
    while i < len(argv):
        if argv[i] == "--rounds":
            rs = [int(x) for x in argv[i + 1].split(",")]
        elif argv[i] == "--fanout-exact":
            _state["k"] = int(argv[i + 1])
        elif argv[i] == "--loss":
            losses = [float(x) for x in argv[i + 1].split(",")]
        elif argv[i] == "--seed":
            _state["seed"] = int(argv[i + 1], 0)
        elif argv[i] == "--out":
            out = argv[i + 1]
        else:
            raise SystemExit(__doc__)
        i += 2
    gossip.Engine.counters = _counters_probe
    gossip.Engine.set_schedule = _set_schedule_rounds
    gossip.Engine.reset_timing = _reset_timing_probe
    bench_args = rest or ["--gpus", "1", "--steps", "20", "--warmup", "5"]
    runs = []
    for loss in losses:
        for r in rs:
            _state.update(r=r, loss=loss, probes=[], engines=0)
            sys.argv = ["bench.py"] + bench_args
            try:
                runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
            except SystemExit as e:
                if e.code not in (0, None):
                    raise
            except gossip.GossipError as e:  # (a run that does not fit: kept in the file, the others go on)
                print("ROUNDS_RUN " + json.dumps(dict(rounds=r, loss=loss, error=str(e))), file=sys.stderr, flush=True)
                runs.append(dict(summary=dict(rounds=r, loss=loss, fanout_exact=_state["k"], error=str(e))))
                continue
            # per engine: the last read after its reset_timing holds the timed ticks alone, the last one before
            # it the ramp
            last = {}
            for p in _state["probes"]:
                last[(p["engine"], p["after_reset"])] = p
            timed = [p for (e, a), p in sorted(last.items()) if a]
            ramp = [p for (e, a), p in sorted(last.items()) if not a]
            # one line per run: ms per tick of the timed ticks summed over the shards (bench.py runs a GPU's
            # shards one after another), the k_rounds part, and the coverage so far (first contacts / (generations x nodes), floods still running included)
            ticks = max((p["fanout_launches"] for p in timed), default=0)  # (a thinning pass per tick, since reset_timing)
            ms = dict(pull=sum(p["pull_phase_ms"] for p in timed), fanout=sum(p["fanout_ms"] for p in timed),
                      rounds=sum(p["rounds_ms"] for p in timed))
            rbytes = sum(p["rounds_bytes"] for p in timed)
            gens = sum(p["generations"] for p in timed)
            reached = sum(sum(p["reach_totals"]) for p in timed)
            line = dict(rounds=r, loss=loss, fanout_exact=_state["k"], shards=len(timed), timed_ticks=ticks,
                        ms_per_tick={k: v / ticks if ticks else None for k, v in ms.items()},
                        rounds_share=ms["rounds"] / sum(ms.values()) if sum(ms.values()) else None,
                        rounds_bytes_per_tick=rbytes / ticks if ticks else None,
                        rounds_gbps=rbytes / ms["rounds"] / 1e6 if ms["rounds"] else None,
                        coverage=reached / (gens * timed[0]["nodes"]) if gens and timed else None)
            print("ROUNDS_RUN " + json.dumps(line), file=sys.stderr, flush=True)
            runs.append(dict(summary=line, timed=timed, ramp=ramp))
    if out:
        with open(out, "w") as f:
            json.dump(dict(bench_args=bench_args, runs=runs), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
