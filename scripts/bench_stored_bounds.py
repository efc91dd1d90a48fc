"""What keeping the score bounds in the nodes costs and buys (csrc/arena_solver.h, Arena.set_stored_bounds), on one
GPU.  A SelfPlayEngine of --games Connect4 games (--sims simulations, --threads in flight, a random-init
ResNet-128x20 through the fused trunk), one lane, one seed:

cost      ms per ply over --plies plies in four modes: off; stored bounds; proof play (the verdict walks); proof play
          on stored bounds (the verdict reads the root's block).  Wall clock around a synchronised run, after one
          warm-up ply; network rows per finished game and the sims alongside (off and stored must agree: the search
          does not read the bounds).
verdict   the verdict pass alone, --warm plies in: Arena.proof_moves_batch over the active games' mover trees, from
          the stored block and by the walk, device events, one warm-up and --repeats timed calls each.
stop      proof_stop_every = each of --strides with stored bounds, --plies plies each.

    python scripts/bench_stored_bounds.py [--out profiles/solver/stored_bounds.json]   -> one JSON line
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.bench_proof_play import timed, tower  # noqa: E402


def engine(net, args, stored, proof, stride=0):
    from self_play_reinforcement_learning_amd.engine import SelfPlayEngine

    return SelfPlayEngine("connect4", net, n_games=args.games, iterations=args.sims, seed=11,
                          search_threads=args.threads, proof_play=proof, proof_stop_every=stride, stored_bounds=stored)


def run_plies(eng, plies):
    import torch

    eng.ply()  # the first ply's allocations
    torch.cuda.synchronize()
    c0, t0 = eng.counters(), time.perf_counter()
    for _ in range(plies):
        eng.ply()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    eng.check()
    c1 = eng.counters()
    games = c1["games_finished"] - c0["games_finished"]
    return dict(plies=plies, ms_per_ply=round(1e3 * dt / plies, 2), games_finished=games,
                nn_rows=c1["nn_rows"] - c0["nn_rows"],
                nn_rows_per_game=round((c1["nn_rows"] - c0["nn_rows"]) / max(games, 1), 1),
                sims=c1["sims"] - c0["sims"], leaked_sims=c1["leaked_sims"] - c0["leaked_sims"])


def bench_cost(net, args):
    rows = []
    for name, stored, proof in (("off", False, False), ("stored", True, False), ("proof_play", False, True),
                                ("proof_play+stored", True, True)):
        eng = engine(net, args, stored, proof)
        row = dict(mode=name, **run_plies(eng, args.plies))
        if proof:
            row["proof_stats"] = eng.arena.proof_stats()
        rows.append(row)
        eng.arena.close()
    return rows


def bench_verdict(net, args):
    out = {}
    for name, stored in (("walk", False), ("stored", True)):
        eng = engine(net, args, stored, True)
        for _ in range(args.warm):
            eng.ply()
        a = eng.arena
        st = a.games_state()
        movers = [2 * g + ((int(st["ply"][g]) + int(st["swap"][g])) & 1) for g in range(args.games)
                  if st["state"][g] == 1]
        t = a._dev_i32(movers)
        us = [1e3 * x for x in timed(lambda: a.proof_moves_batch(t), args.repeats)]
        got = {k: v.cpu().numpy() for k, v in a.proof_moves_batch(t).items()}
        eng.check()
        out[name] = dict(trees=len(movers), us=[round(x, 1) for x in us], us_median=round(statistics.median(us), 1),
                         solved_share=round(float((got["lo"] == got["hi"]).mean()), 4),
                         keep_sum=int((got["keep"].astype("int64") & 0xffffffff).sum()))
        a.close()
    out["same_verdicts"] = out["walk"]["keep_sum"] == out["stored"]["keep_sum"]
    return out


def bench_stop(net, args):
    rows = []
    for stride in args.strides:
        eng = engine(net, args, True, True, stride=stride)
        row = dict(stride=stride, **run_plies(eng, args.plies))
        stats = eng.arena.proof_stats()
        row.update(trees_stopped=stats["trees_stopped"], sims_skipped=stats["sims_skipped"])
        rows.append(row)
        eng.arena.close()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=200)
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--warm", type=int, default=16, help="verdict: plies played before the timed calls")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--strides", type=int, nargs="*", default=[0, 1, 4, 16])
    ap.add_argument("--plies", type=int, default=40)
    ap.add_argument("--parts", nargs="*", default=["cost", "verdict", "stop"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    res = dict(game="connect4", games=args.games, sims=args.sims, threads=args.threads,
               net=f"ResidualTower(filter_factor=32, num_blocks={args.blocks}), random init, fp16 fused trunk",
               repeats=args.repeats)
    net = tower(args.blocks)
    if "cost" in args.parts:
        res["cost"] = bench_cost(net, args)
    if "verdict" in args.parts:
        res["verdict"] = bench_verdict(net, args)
    if "stop" in args.parts:
        res["stop"] = bench_stop(net, args)
    line = json.dumps(res, default=lambda o: o.tolist() if hasattr(o, "tolist") else str(o))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
