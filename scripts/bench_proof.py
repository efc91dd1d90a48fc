"""What proving from the search trees costs (csrc/arena_tree.h k_tree_bounds): Arena.bounds_batch over --trees
Connect4 trees after one --sims-simulation search (--threads sims in flight, the table net) at mid-game positions
(--plies random plies that leave the game open; --positions distinct ones, tree t searches position t mod
--positions on its own random stream).

bounds_batch writes into buffers allocated once and is timed with device events: one warm-up call, then --repeats
timed calls, the median reported (every call's time listed).  The comparison is the route the library offered before
the kernel: Arena.export_subtrees(min_visits=0) sized to the trees' counts, the host copies (TreeView.from_export)
and the host walk (TreeView.score_bounds), wall-clock time on the first --sample trees, scaled to all of them (the
sample's results are checked against the kernel's on the way).  Beside the times: the share of trees that are open,
bounded on one side (a win, a loss, at least or at most a draw, not yet exact) and solved (lo == hi), and the mean
number of expanded nodes walked.

    python scripts/bench_proof.py [--out profiles/proof/bench.json]   -> one JSON line
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def midgame_positions(count, plies, seed):
    """`count` distinct move lists of `plies` random legal plies from the empty 7x6 board, the game still on."""
    import numpy as np

    from self_play_reinforcement_learning_amd.envs import Connect4Env

    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        env, moves, player = Connect4Env(), [], 1
        for _ in range(plies):
            legal = np.flatnonzero(env.valid_moves())
            a = int(legal[rng.integers(len(legal))])
            _, _, done, _ = env.step(a, player)
            moves.append(a)
            player = -player
            if done:
                moves = None
                break
        if moves is not None and moves not in out:
            out.append(moves)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trees", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=200)
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--plies", type=int, default=20)
    ap.add_argument("--positions", type=int, default=64)
    ap.add_argument("--sample", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from self_play_reinforcement_learning_amd import TreeView
    from self_play_reinforcement_learning_amd._lib import call, ptr
    from self_play_reinforcement_learning_amd.arena import Arena, _stream, table_net_eval

    game, T, K = "connect4", args.trees, args.threads
    seqs = midgame_positions(args.positions, args.plies, seed=5)
    a = Arena(game, n_trees=T, iterations=args.sims, seed=11, leaf_format="f32", leaf_layout="nchw", search_threads=K)
    ids = list(range(T))

    def step(n):
        if n:
            p, v = table_net_eval(game, a.leaves(n), a.leaf_format, a.leaf_layout)
            a.expand(p, v)

    a.tree_reset(ids, [1] * T)
    for i in range(args.plies):
        step(a.play_action(ids, [seqs[t % len(seqs)][i] for t in ids]))
    a.search_begin(ids)
    for _ in range(-(-args.sims // K)):
        step(a.select())
    a.check()
    t = a._dev_i32(ids)
    out = a.bounds_batch(t)

    def run():
        call("spmcts_tree_bounds_batch", a.h, ptr(t), T, *[ptr(out[k]) for k in Arena.BOUNDS_FIELDS], _stream())

    run()  # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    a.check()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    lo, hi = host["lo"].astype(int), host["hi"].astype(int)
    solved = lo == hi
    one_side = ~solved & ((lo >= 0) | (hi <= 0))
    res = dict(game=game, trees=T, sims=args.sims, threads=K, plies=args.plies, positions=len(seqs),
               repeats=args.repeats,
               bounds_batch=dict(us=[round(1e3 * x, 1) for x in ms], us_median=round(1e3 * statistics.median(ms), 1),
                                 ns_per_tree=round(1e6 * statistics.median(ms) / T, 1)),
               share=dict(open=round(float((~solved & ~one_side).mean()), 4), one_side=round(float(one_side.mean()), 4),
                          solved=round(float(solved.mean()), 4)),
               nodes=dict(mean=round(float(host["nodes"].mean()), 1), max=int(host["nodes"].max())))

    # the route without the kernel, on a sample
    S = min(args.sample, T)
    sample = ids[:S]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    count = a.export_subtrees(sample, 1, min_visits=0)["count"]
    ex = a.export_subtrees(sample, int(count.max()), min_visits=0)
    rs = {k: v.cpu().numpy() for k, v in a.root_stats_batch(sample).items()}
    t1 = time.perf_counter()
    views = [TreeView.from_export(ex, i) for i in range(S)]
    t2 = time.perf_counter()
    twin = [views[i].score_bounds(game, rs["board"][i], int(rs["root_player"][i])) for i in range(S)]
    t3 = time.perf_counter()
    for i, w in enumerate(twin):
        got = {k: (host[k][i].tolist() if host[k].ndim > 1 else int(host[k][i])) for k in Arena.BOUNDS_FIELDS}
        assert got == w, (i, got, w)
    per_tree = (t3 - t0) / S
    res["host_route"] = dict(sample=S, export_ms=round(1e3 * (t1 - t0), 2), copy_ms=round(1e3 * (t2 - t1), 2),
                             walk_ms=round(1e3 * (t3 - t2), 2), us_per_tree=round(1e6 * per_tree, 1),
                             scaled_ms_all_trees=round(1e3 * per_tree * T, 1))
    res["speedup_over_host_route"] = round(per_tree * T * 1e3 / statistics.median(ms), 1)
    a.close()
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
