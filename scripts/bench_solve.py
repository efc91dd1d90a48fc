"""The exact solver to the end of the game on the device (csrc/solve.h): batch time, node rate, launches and tail.

sets     --positions unfinished 7x6 positions after random 24-ply and 20-ply playouts (seeded; a playout that
         ended is drawn again).  Each set: one warm-up batch, then --repeats timed batches from device events, the
         table cleared before every batch (median and min); nodes from the kernels' own counts, nodes/s, the
         kernel launches a batch took and the time per launch (the tail: the last launches hold the hardest
         position's lanes alone), the positions not solved within --max-nodes.  Beside it the host twin on one core
         over the same positions, on one table cleared once.
yardstick  --positions positions with 8 empty cells (34 plies), solved to the end and by the full-width
         spmcts_negamax_batch at depth 8; the codes must agree.

    python scripts/bench_solve.py [--out profiles/solve/bench.json]   -> one JSON line
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def playouts(n, plies, seed):
    """n unfinished 7x6 positions after `plies` random moves: (boards int8 [n, 7, 6], players int8 [n], drawn)."""
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
    return np.stack(boards), np.full(n, 1 if plies % 2 == 0 else -1, dtype=np.int8), drawn


def timed(f, repeats, before):
    import torch

    ms = []
    for _ in range(repeats):
        before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = f()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms, out


def one_set(args, plies, table, host_table):
    import torch

    from self_play_reinforcement_learning_amd import solve_to_end
    from self_play_reinforcement_learning_amd.solve import solve_host

    boards, players, drawn = playouts(args.positions, plies, args.seed + plies)
    b, p = torch.as_tensor(boards).cuda(), torch.as_tensor(players).cuda()

    def run():
        return solve_to_end("connect4", boards=b, players=p, max_nodes=args.max_nodes, table=table,
                            launch_nodes=args.launch_nodes)

    table.clear()
    run()  # warm-up
    ms, out = timed(run, args.repeats, table.clear)
    nodes = out["nodes"].cpu().numpy()
    med = statistics.median(ms)
    res = dict(plies=plies, positions=args.positions, playouts_drawn=drawn, batch_ms_median=med, batch_ms_min=min(ms),
               batch_ms=ms, nodes=int(nodes.sum()), nodes_mean=float(nodes.mean()), nodes_max=int(nodes.max()),
               device_nodes_per_s=float(nodes.sum()) / (med * 1e-3), launches=out["launches"],
               ms_per_launch=med / max(out["launches"], 1), unsolved=int((~out["solved"]).sum()),
               outcomes={k: int((out["outcome"][out["solved"]] == v).sum()) for k, v in (("win", 1), ("draw", 0), ("loss", -1))})
    print(f"{plies} plies: {res['nodes']} nodes, {med:.1f} ms per batch, {out['launches']} launches", file=sys.stderr, flush=True)
    host_table.clear()
    m = min(args.host_positions, args.positions)
    t0 = time.perf_counter()
    host = [solve_host("connect4", boards[i], int(players[i]), host_table, max_nodes=args.max_nodes) for i in range(m)]
    host_s = time.perf_counter() - t0
    score = out["score"].cpu().numpy()
    solved = out["solved"].cpu().numpy()
    agree = all(host[i][0].tolist() == score[i].tolist() for i in range(m) if solved[i] and not (host[i][0] == -127).any())
    res.update(host_positions=m, host_nodes=int(sum(h[1] for h in host)), host_s=host_s,
               host_nodes_per_s_one_core=sum(h[1] for h in host) / host_s, host_codes_agree=bool(agree))
    return res


def yardstick(args, table):
    import torch

    from self_play_reinforcement_learning_amd import solve_positions, solve_to_end

    boards, players, drawn = playouts(args.positions, 34, args.seed + 34)
    b, p = torch.as_tensor(boards).cuda(), torch.as_tensor(players).cuda()
    full = lambda: solve_positions("connect4", boards=b, players=p, depth=8)  # noqa: E731
    end = lambda: solve_to_end("connect4", boards=b, players=p, max_nodes=args.max_nodes, table=table)  # noqa: E731
    full(), table.clear(), end()
    ms_full, out_full = timed(full, args.repeats, lambda: None)
    ms_end, out_end = timed(end, args.repeats, table.clear)
    return dict(empties=8, positions=args.positions, playouts_drawn=drawn, codes_agree=bool(torch.equal(out_full["score"], out_end["score"])),
                full_width_ms_median=statistics.median(ms_full), full_width_nodes=int(out_full["nodes"].sum()),
                solve_ms_median=statistics.median(ms_end), solve_nodes=int(out_end["nodes"].sum()), solve_launches=out_end["launches"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--positions", type=int, default=4096)
    ap.add_argument("--plies", type=int, nargs="*", default=[24, 20])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-positions", type=int, default=4096)
    ap.add_argument("--max-nodes", type=int, default=1 << 24)
    ap.add_argument("--launch-nodes", type=int, default=0)
    ap.add_argument("--table-entries", type=int, default=1 << 22)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_solve.py measures on the GPU; none is available")
    from self_play_reinforcement_learning_amd import SolveTable
    from self_play_reinforcement_learning_amd.solve import HostSolveTable

    table = SolveTable("connect4", entries=args.table_entries)
    host_table = HostSolveTable("connect4", entries=args.table_entries)
    res = dict(device=torch.cuda.get_device_name(0), table_entries=args.table_entries, max_nodes=args.max_nodes,
               launch_nodes=args.launch_nodes, sets=[one_set(args, plies, table, host_table) for plies in args.plies],
               yardstick=yardstick(args, table))
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
