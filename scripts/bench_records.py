"""Game records (csrc/records.h, records.py): what the game log costs a self-play run, and how fast finished games
are graded.

log      two LanedEngines of the bench's configuration (bench.py: connect4, --games slots, --sims simulations, a
         --blocks-block net, 2 lanes, 4 sims in flight, fp16), one with record_games=True and one without, same
         seed; --warmup plies each, then --rounds rounds of --plies timed plies, the two engines alternating within
         every round (off then on, then on then off): positions/s per round and engine, the medians, the spread
         and the ratio on / off of every round.
grade    --grade-games finished 7x6 games (random legal playouts, seeded) graded by grade_games at --max-empty
         empty cells: seconds (one warm-up call, then --repeats timed calls with a fresh table), graded positions per
         second, and the solver's node counts (sum, max per position).

    python scripts/bench_records.py [--out profiles/records/bench.json]   -> one JSON line
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def playouts(n, seed):
    """n finished 7x6 games of uniformly random legal moves."""
    from self_play_reinforcement_learning_amd.envs import Connect4Env

    rng = np.random.default_rng(seed)
    env = Connect4Env()
    games = []
    for _ in range(n):
        env.reset()
        moves, done = [], False
        while not done:
            a = int(rng.choice(np.flatnonzero(env.valid_moves())))
            _, _, done, _ = env.step(a, 1 if len(moves) % 2 == 0 else -1)
            moves.append(a)
        games.append(moves)
    return games


def bench_log(args):
    import torch

    from self_play_reinforcement_learning_amd.engine import LanedEngine
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    torch.manual_seed(0)
    net = ResidualTower(7, 6, 7, num_blocks=args.blocks, filter_factor=32).cuda().eval()
    n0 = int(round(args.games * 0.48))  # bench.py's lane split under cross-lane dedup
    engines = {}
    for name, rec in (("off", False), ("on", True)):
        engines[name] = LanedEngine("connect4", net, n_games=args.games, lanes=2, lane_sizes=[n0, args.games - n0],
                                    iterations=args.sims, seed=1234, dtype=torch.float16, search_threads=4, eval_cache=1,
                                    record_games=rec)
        for _ in range(args.warmup):
            engines[name].ply()
    rates = {"off": [], "on": []}
    for r in range(args.rounds):
        for name in (("off", "on") if r % 2 == 0 else ("on", "off")):
            eng = engines[name]
            torch.cuda.synchronize()
            p0, t0 = eng.positions, time.perf_counter()
            for _ in range(args.plies):
                eng.ply()
            torch.cuda.synchronize()
            rates[name].append((eng.positions - p0) / (time.perf_counter() - t0))
    for eng in engines.values():
        eng.check()
    records = engines["on"].game_records()
    ratio = [a / b for a, b in zip(rates["on"], rates["off"])]
    return dict(games=args.games, sims=args.sims, blocks=args.blocks, warmup=args.warmup, rounds=args.rounds,
                plies=args.plies, positions_per_s={k: [round(x, 1) for x in v] for k, v in rates.items()},
                median={k: round(statistics.median(v), 1) for k, v in rates.items()},
                ratio_on_off=[round(x, 4) for x in ratio], ratio_median=round(statistics.median(ratio), 4),
                ratio_min=round(min(ratio), 4), ratio_max=round(max(ratio), 4), records_kept=len(records),
                games_finished_on=engines["on"].games_done)


def bench_grade(args):
    import torch

    from self_play_reinforcement_learning_amd.records import from_moves, grade_games
    from self_play_reinforcement_learning_amd.solve import SolveTable

    records = from_moves("connect4", playouts(args.grade_games, 7))
    out, secs = None, []
    for i in range(args.repeats + 1):
        table = SolveTable("connect4")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = grade_games("connect4", records, max_empty=args.max_empty, table=table)
        torch.cuda.synchronize()
        if i:  # the first call warms up
            secs.append(time.perf_counter() - t0)
    nodes = out["nodes"]
    tier = int(out["n_graded"]) + int(out["n_unsolved"])
    return dict(games=len(records), max_empty=args.max_empty, rows=out["n_rows"], exact_tier_rows=tier,
                graded=out["n_graded"], unsolved=out["n_unsolved"], strong=out["n_strong"], weak=out["n_weak"],
                blunders=out["n_blunders"], seconds=[round(s, 4) for s in secs],
                seconds_median=round(statistics.median(secs), 4),
                graded_per_s=round(out["n_graded"] / statistics.median(secs), 1), nodes_sum=int(nodes.sum()),
                nodes_max=int(nodes.max()) if nodes.numel() else 0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--plies", type=int, default=8)
    ap.add_argument("--grade-games", type=int, default=4096)
    ap.add_argument("--max-empty", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip", choices=["log", "grade"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {}
    if args.skip != "log":
        res["log"] = bench_log(args)
    if args.skip != "grade":
        res["grade"] = bench_grade(args)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
