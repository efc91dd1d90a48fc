"""An N-player round robin two ways, on the same box: one league arena against one two-network arena per pairing.

    python scripts/bench_league.py            # 8 players: 28 pairings x 100 games, ResNet-128x20 fp16, 200 sims, K = 4

  league       engine.LeagueEngine: every pairing's games in one arena, each simulation step's leaf rows routed
               to their tree's network (spmcts_league_route), one trunk launch per network per step.
  sequential   what 28 calls of SelfPlayScheduler.compare_models() run, one after another: a two-network
               SelfPlayEngine of `games` slots per pairing, built as the scheduler builds it (evaluate mode, no
               Move records, leaf dedup and the evaluation cache at their defaults).

Both wall times include building the engines (packing the weights, allocating the arena): a user waits for both.
Rows per trunk launch = network rows / trunk launches, a launch being one network's evaluation of one step
(simulation steps and the end-of-ply expansions).  The gfx clock is sampled over each timed region
(bench.GfxClock).  Writes profiles/league/round_robin.json and prints the same JSON line.  No threshold: this is
a measurement.
"""
import argparse
import itertools
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench import GfxClock
from self_play_reinforcement_learning_amd.engine import LeagueEngine, SelfPlayEngine
from self_play_reinforcement_learning_amd.modules import ResidualTower

ap = argparse.ArgumentParser()
ap.add_argument("--players", type=int, default=8)
ap.add_argument("--games", type=int, default=100, help="games per pairing")
ap.add_argument("--blocks", type=int, default=20)
ap.add_argument("--filter-factor", type=int, default=32, help="channels / 4")
ap.add_argument("--sims", type=int, default=200)
ap.add_argument("--threads", type=int, default=4)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--out", default=os.path.join("profiles", "league", "round_robin.json"))
args = ap.parse_args()
dev = torch.device("cuda:0")

nets = []
for s in range(args.players):
    torch.manual_seed(1000 + s)
    nets.append(ResidualTower(7, 6, 7, num_blocks=args.blocks, filter_factor=args.filter_factor).to(dev).eval())
pairings = list(itertools.combinations(range(args.players), 2))


def timed(fn):
    torch.cuda.synchronize()
    clk = GfxClock(dev)
    clk.start()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    clk.stop()
    c = clk.report().get("clock_ghz")
    return out, wall, round(c, 3) if c else None


def tally(breakdowns):
    return [[b[s][k] for s in ("first", "second") for k in ("wins", "draws", "losses")] for b in breakdowns]


def league():
    eng = LeagueEngine("connect4", [dict(network=n, iterations=args.sims) for n in nets], pairings,
                       games_per_pairing=args.games, seed=args.seed, search_threads=args.threads, dtype=torch.float16)
    res = eng.play()
    c = eng.counters()
    out = dict(games=c["games_finished"], plies=eng.plies, nn_rows=c["nn_rows"], trunk_launches=eng.launches,
               results=tally(res))
    eng.close()
    return out


def sequential():
    out = dict(games=0, plies=0, nn_rows=0, trunk_launches=0, results=[])
    for p, (i, j) in enumerate(pairings):
        eng = SelfPlayEngine("connect4", nets[i], n_games=args.games, iterations=args.sims, evaluate=True,
                             seed=args.seed + p, opponent=nets[j], record=False, search_threads=args.threads,
                             max_games=args.games, dtype=torch.float16)
        eng.run(games=args.games)
        eng.check()
        c = eng.counters()
        out["games"] += c["games_finished"]
        out["plies"] += eng.plies
        out["nn_rows"] += c["nn_rows"]
        out["trunk_launches"] += 2 * eng.plies * (eng.select_steps + 1)  # both networks, every step of every ply
        out["results"].append([x for side in c["results"] for x in side])
        eng.arena.close()
        print(f"sequential pairing {p + 1}/{len(pairings)} done", flush=True)
    return out


report = dict(players=args.players, pairings=len(pairings), games_per_pairing=args.games, blocks=args.blocks,
              channels=4 * args.filter_factor, sims=args.sims, search_threads=args.threads, dtype="fp16",
              device=torch.cuda.get_device_name(0))
for name, fn in (("league", league), ("sequential", sequential)):
    out, wall, clock = timed(fn)
    out.update(wall_s=round(wall, 2), clock_ghz=clock,
               rows_per_trunk_launch=round(out["nn_rows"] / max(1, out["trunk_launches"]), 1))
    report[name] = out
    print(f"{name}: {wall:.1f} s", flush=True)
report["speedup"] = round(report["sequential"]["wall_s"] / report["league"]["wall_s"], 2)
report["note"] = ("the sequential engines run with leaf dedup and the evaluation cache (their defaults), the league "
                  "evaluates every leaf on its own; the two play different games (different seeds and row sharing), "
                  "so the results differ game by game")
os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
with open(args.out, "w") as f:
    f.write(json.dumps(report) + "\n")
print(json.dumps(report))
