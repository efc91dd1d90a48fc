"""What searching with the stored score bounds costs and buys (csrc/arena_solver.h sb_refuted / sb_proved,
Arena.set_solver_rules), on one GPU.  The workload of bench_stored_bounds.py: a SelfPlayEngine of --games Connect4
games (--sims simulations, --threads in flight, a random-init ResNet-128x20 through the fused trunk), one lane, one
seed.  Numbers are recorded, no threshold is set; the feature stays off by default whatever they say.

cost      ms per ply over --plies plies in six modes: off; stored bounds only; refute; proved; both rules; both rules
          plus proof play.  Wall clock around a synchronised run after one warm-up ply; network rows per finished
          game, sims, leaks and the two statistics of the rules alongside.
kernels   the mean device time of k_expand_vl / k_select_vl per mode: one child process per mode under
          `rocprofv3 --kernel-trace --stats` (a run of its own, no counters in it), --trace-plies plies each.
strength  Elo.compare_models of one random-init ResNet-128x4 against itself with and without solver_search, --sims
          simulations, openings "all:2", and Elo.grade(max_empty=12) of both sides (the experiment of "Proof-guided
          play", scripts/bench_proof_play.py).

    python scripts/bench_solver_search.py [--out profiles/solver/solver_search.json]   -> one JSON line
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_proof_play import tower  # noqa: E402
from scripts.bench_stored_bounds import run_plies  # noqa: E402

# mode -> (stored_bounds, solver_search, proof_play)
MODES = {"off": (False, False, False), "stored": (True, False, False), "refute": (True, "refute", False),
         "proved": (True, "proved", False), "both": (True, True, False), "both+proof_play": (True, True, True)}


def engine(net, args, mode):
    from self_play_reinforcement_learning_amd.engine import SelfPlayEngine

    stored, solver, proof = MODES[mode]
    return SelfPlayEngine("connect4", net, n_games=args.games, iterations=args.sims, seed=11,
                          search_threads=args.threads, proof_play=proof, stored_bounds=stored, solver_search=solver)


def run_mode(net, args, mode, plies):
    eng = engine(net, args, mode)
    row = dict(mode=mode, **run_plies(eng, plies), **eng.arena.solver_stats())
    if MODES[mode][2]:
        row["proof_stats"] = eng.arena.proof_stats()
    eng.arena.close()
    return row


def kernel_times(args):
    """Per mode: {kernel family: mean device time in us, calls} from rocprofv3's kernel statistics of a child run."""
    out = {}
    for mode in args.modes:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "-o", "run", "--", sys.executable,
                   os.path.abspath(__file__), "--only-mode", mode, "--plies", str(args.trace_plies), "--games",
                   str(args.games), "--sims", str(args.sims), "--threads", str(args.threads), "--blocks", str(args.blocks)]
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=args.trace_timeout)
            files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if not files:
                raise RuntimeError(f"rocprofv3 left no kernel statistics for mode {mode}")
            fam = {}
            with open(files[0]) as f:
                for r in csv.DictReader(f):
                    for key in ("k_expand_vl", "k_select_vl"):
                        if key in r["Name"]:
                            calls, total = fam.get(key, (0, 0.0))
                            fam[key] = (calls + int(r["Calls"]), total + float(r["TotalDurationNs"]))
            out[mode] = {k: dict(calls=c, mean_us=round(t / c / 1e3, 2)) for k, (c, t) in fam.items()}
    return out


def bench_strength(args):
    from self_play_reinforcement_learning_amd import Elo, ModelDatabase
    from self_play_reinforcement_learning_amd.base_model import ModelContainer
    from self_play_reinforcement_learning_amd.envs import Connect4Env

    net = tower(args.strength_blocks, seed=1)
    with tempfile.TemporaryDirectory() as d:
        db = ModelDatabase(d, Connect4Env)
        db.add_model("plain", ModelContainer("MCTreeSearch", policy_kwargs=dict(network=net, iterations=args.sims)))
        db.add_model("solver", ModelContainer("MCTreeSearch", policy_kwargs=dict(network=net, iterations=args.sims,
                                                                                  solver_search=True)))
        elo = Elo(db, seed=3, search_threads=args.threads)
        counts = elo.compare_models("plain", "solver", num_games=args.strength_games, openings="all:2",
                                    record_games=True)
        grade = elo.grade("plain", "solver", max_empty=12)
    return dict(net=f"ResidualTower(filter_factor=32, num_blocks={args.strength_blocks}), random init", sims=args.sims,
                openings="all:2", games=args.strength_games, counts=counts, grade_max_empty_12=grade)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=200)
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--plies", type=int, default=40)
    ap.add_argument("--trace-plies", type=int, default=12)
    ap.add_argument("--trace-timeout", type=int, default=240)
    ap.add_argument("--modes", nargs="*", default=list(MODES))
    ap.add_argument("--strength-games", type=int, default=98)
    ap.add_argument("--strength-blocks", type=int, default=4)
    ap.add_argument("--parts", nargs="*", default=["cost", "kernels", "strength"])
    ap.add_argument("--only-mode", default=None, help="(the kernels part's child run: one mode, nothing written)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    if args.only_mode:
        run_mode(tower(args.blocks), args, args.only_mode, args.plies)
        return
    res = dict(game="connect4", games=args.games, sims=args.sims, threads=args.threads,
               net=f"ResidualTower(filter_factor=32, num_blocks={args.blocks}), random init, fp16 fused trunk")
    if "kernels" in args.parts:  # first: the children run while this process holds no GPU memory
        res["kernels"] = dict(plies=args.trace_plies, **kernel_times(args))
    if "cost" in args.parts:
        net = tower(args.blocks)
        res["cost"] = [run_mode(net, args, mode, args.plies) for mode in args.modes]
    if "strength" in args.parts:
        res["strength"] = bench_strength(args)
    line = json.dumps(res, default=lambda o: o.tolist() if hasattr(o, "tolist") else str(o))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
