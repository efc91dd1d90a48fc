"""The exact depth-limited negamax on the device (csrc/negamax.h): solver rate and arena cost.

solver   --positions positions reached by random 8-ply openings on 7x6 (seeded; a playout that ended is drawn
         again), solved at each of --depths: time per batch from device events (one warm-up batch, then --repeats
         timed ones: median and min), nodes (moves made, from the kernel's own counts) and nodes/s; beside it the
         host twin's nodes/s on one core over the first --host-positions positions.
arena    a --games-game evaluation arena (2-block net, --sims sims, K = 4) against "lookahead", Negamax(4) and
         Negamax(6): device time of spmcts_games_end_ply (the launch that holds the negamax kernel) per ply, from
         events around it, over plies 2 .. --plies; the difference to "lookahead" is what a negamax side adds to a
         ply (the negamax side moves in half of the games each ply).

    python scripts/bench_negamax.py [--out profiles/negamax/bench.json]   -> one JSON line
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def openings(n, plies, seed):
    """n unfinished 7x6 positions after `plies` random moves: (boards int8 [n, 7, 6], players int8 [n])."""
    from self_play_reinforcement_learning_amd.envs import Connect4Env

    rng = np.random.default_rng(seed)
    env = Connect4Env()
    boards, drawn = [], 0
    while len(boards) < n:
        drawn += 1
        env.reset()
        done = False
        for p in range(plies):
            a = int(rng.choice(np.flatnonzero(env.valid_moves())))
            _, _, done, _ = env.step(a, 1 if p % 2 == 0 else -1)
            if done:
                break
        if not done:
            boards.append(env.board.astype(np.int8).copy())
    players = np.full(n, 1 if plies % 2 == 0 else -1, dtype=np.int8)
    return np.stack(boards), players, drawn


def solver(args):
    import torch

    from self_play_reinforcement_learning_amd import solve_positions
    from self_play_reinforcement_learning_amd.hardcoded_players import negamax_host

    boards, players, drawn = openings(args.positions, 8, args.seed)
    b, p = torch.as_tensor(boards).cuda(), torch.as_tensor(players).cuda()
    out = []
    for depth in args.depths:
        nodes = int(solve_positions("connect4", boards=b, players=p, depth=depth)["nodes"].sum())  # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            solve_positions("connect4", boards=b, players=p, depth=depth)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        host_nodes = sum(negamax_host("connect4", boards[i], int(players[i]), depth)[1]
                         for i in range(min(args.host_positions, args.positions)))
        host_s = time.perf_counter() - t0
        med = statistics.median(ms)
        print(f"depth {depth}: {nodes} nodes, {med:.3f} ms per batch", file=sys.stderr, flush=True)
        out.append(dict(depth=depth, positions=args.positions, nodes=nodes, batch_ms_median=med, batch_ms_min=min(ms),
                        batch_ms=ms, device_nodes_per_s=nodes / (med * 1e-3), host_nodes=host_nodes,
                        host_nodes_per_s_one_core=host_nodes / host_s,
                        worst_case_nodes=args.positions * sum(7 ** k for k in range(1, depth + 1))))
    return dict(openings_drawn=drawn, runs=out)


def arena(args):
    import torch

    from self_play_reinforcement_learning_amd.engine import SelfPlayEngine
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    torch.manual_seed(0)
    net = ResidualTower(7, 6, 7, num_blocks=2, filter_factor=32).cuda().eval()
    out = {}
    for name, kw in (("lookahead", dict(opponent="lookahead")), ("negamax4", dict(opponent="negamax", opponent_depth=4)),
                     ("negamax6", dict(opponent="negamax", opponent_depth=6))):
        eng = SelfPlayEngine("connect4", network=net, n_games=args.games, iterations=args.sims, seed=1, evaluate=True,
                             record=False, search_threads=4, **kw)
        a = eng.arena
        spans = []
        for method in ("games_end_ply_async", "games_end_ply"):
            inner = getattr(a, method)

            def timed(inner=inner):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = inner()
                e1.record()
                spans.append((e0, e1))
                return r

            setattr(a, method, timed)
        for _ in range(args.plies):
            eng.ply()  # finished games are refilled: every ply has --games active games
        torch.cuda.synchronize()
        eng.check()
        ms = [e0.elapsed_time(e1) for e0, e1 in spans][2:]  # plies 0 and 1 warm the kernels up
        out[name] = dict(end_ply_ms_mean=statistics.mean(ms), end_ply_ms_median=statistics.median(ms),
                         end_ply_ms_max=max(ms), plies=len(ms))
        eng.arena.close()
    for name in ("negamax4", "negamax6"):
        out[name]["added_ms_per_ply_mean"] = out[name]["end_ply_ms_mean"] - out["lookahead"]["end_ply_ms_mean"]
        out[name]["added_ms_per_ply_max"] = out[name]["end_ply_ms_max"] - out["lookahead"]["end_ply_ms_median"]
    out["scale_mcts_ply_ms"] = 142.5  # README: the 4,096-game, 200-sim ResNet-128x20 ply
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--positions", type=int, default=4096)
    ap.add_argument("--depths", type=int, nargs="*", default=[6, 8])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-positions", type=int, default=16)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=8)
    ap.add_argument("--plies", type=int, default=14)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--skip-arena", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_negamax.py measures on the GPU; none is available")
    res = dict(device=torch.cuda.get_device_name(0), solver=solver(args))
    if not args.skip_arena:
        res["arena"] = arena(args)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
