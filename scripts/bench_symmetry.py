"""What the boards' mirror symmetry costs and buys (csrc/board.h canonical_pair behind the SYM = true kernels,
Arena.set_symmetry), on one GPU.  Numbers are recorded, no threshold is set; the feature stays off by default
whatever they say.

lanes     the bench's workload (bench.py): a LanedEngine of --games Connect4 games in two lanes (0.48 / 0.52), --sims
          simulations, --threads in flight, a random-init ResNet-128x20 through the fused fp16 trunk, leaf dedup,
          cross-lane dedup, cache window 1; modes off and mirror.  Per mode positions/s, ms per ply, nn_rows,
          nn_leaves, cache_rows and rows per leaf over the bench's window (5 warm-up plies, 20 timed) and over a
          steady-state window (45 warm-up plies, 20 timed).
league    the same two modes in a LeagueEngine of one net against itself with openings "all:2" (98 slots): rows per
          leaf and ms per ply over the whole match.
kernels   the mean device time of k_expand_vl / k_encode / k_dedup_insert per mode: one child process per mode under
          `rocprofv3 --kernel-trace --stats` (a run of its own, no counters in it), --trace-plies plies each.

    python scripts/bench_symmetry.py [--out profiles/symmetry/symmetry.json]   -> one JSON line
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_proof_play import tower  # noqa: E402

MODES = {"off": None, "mirror": "mirror"}
KERNELS = ("k_expand_vl", "k_encode", "k_dedup_insert")


def engine(net, args, mode):
    import torch

    from self_play_reinforcement_learning_amd.engine import LanedEngine

    n0 = int(round(args.games * 0.48))  # bench.py's lane split under cross-lane dedup
    return LanedEngine("connect4", net, n_games=args.games, lanes=2, lane_sizes=[n0, args.games - n0],
                       iterations=args.sims, seed=1234, search_threads=args.threads, dtype=torch.float16, eval_cache=1,
                       symmetry=MODES[mode])


def window(eng, warmup, plies):
    """Counters and wall clock over `plies` plies after `warmup` more warm-up plies of the running engine."""
    import torch

    for _ in range(warmup):
        eng.ply()
    torch.cuda.synchronize()
    c0, p0, t0 = eng.counters(), eng.positions, time.perf_counter()
    for _ in range(plies):
        eng.ply()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    eng.check()
    c1 = eng.counters()
    d = {k: c1[k] - c0[k] for k in ("nn_rows", "nn_leaves", "cache_rows", "sims")}
    return dict(warmup=warmup, plies=plies, positions_per_s=round((eng.positions - p0) / dt, 1),
                ms_per_ply=round(1e3 * dt / plies, 2), rows_per_leaf=round(d["nn_rows"] / max(d["nn_leaves"], 1), 4), **d)


def run_mode(net, args, mode, trace_plies=None):
    eng = engine(net, args, mode)
    assert eng.cross_dedup and eng.leaf_dedup and eng.symmetry == MODES[mode]
    if trace_plies is not None:
        row = dict(mode=mode, trace=window(eng, 1, trace_plies))
    else:  # the bench's window, then on to the steady state: 5 + 20 + 20 = 45 plies before the second window
        row = dict(mode=mode, bench_window=window(eng, args.warmup, args.plies))
        row["steady_window"] = window(eng, args.steady_warmup - args.warmup - args.plies, args.plies)
    for e in eng.lanes:
        e.arena.close()
    return row


def run_league(args, mode):
    import torch

    from self_play_reinforcement_learning_amd.engine import LeagueEngine
    from self_play_reinforcement_learning_amd.openings import parse_openings

    net = tower(args.blocks)
    book = parse_openings("all:2", "connect4")
    players = [dict(network=net, iterations=args.sims, name="a"), dict(network=net, iterations=args.sims, name="b")]
    lg = LeagueEngine("connect4", players, [(0, 1)], games_per_pairing=2 * len(book), seed=3,
                      search_threads=args.threads, dtype=torch.float16, openings=book, symmetry=MODES[mode])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lg.play()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    lg.check()
    c = lg.counters()
    lg.close()
    return dict(mode=mode, openings="all:2", games=2 * len(book), plies=lg.plies, ms_per_ply=round(1e3 * dt / max(lg.plies, 1), 2),
                nn_rows=c["nn_rows"], nn_leaves=c["nn_leaves"], cache_rows=c["cache_rows"],
                rows_per_leaf=round(c["nn_rows"] / max(c["nn_leaves"], 1), 4),
                note="a league arena runs without leaf dedup: one row per leaf in either mode")


def kernel_times(args):
    """Per mode: {kernel: mean device time in us, calls} from rocprofv3's kernel statistics of a child run."""
    out = {}
    for mode in args.modes:
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "-o", "run", "--", sys.executable,
                   os.path.abspath(__file__), "--only-mode", mode, "--trace-plies", str(args.trace_plies), "--games",
                   str(args.games), "--sims", str(args.sims), "--threads", str(args.threads), "--blocks", str(args.blocks)]
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=args.trace_timeout)
            files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if not files:
                raise RuntimeError(f"rocprofv3 left no kernel statistics for mode {mode}")
            fam = {}
            with open(files[0]) as f:
                for r in csv.DictReader(f):
                    for key in KERNELS:
                        if key in r["Name"]:
                            calls, total = fam.get(key, (0, 0.0))
                            fam[key] = (calls + int(r["Calls"]), total + float(r["TotalDurationNs"]))
            out[mode] = {k: dict(calls=c, mean_us=round(t / c / 1e3, 2)) for k, (c, t) in fam.items()}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=200)
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--plies", type=int, default=20)
    ap.add_argument("--steady-warmup", type=int, default=45)
    ap.add_argument("--trace-plies", type=int, default=8)
    ap.add_argument("--trace-timeout", type=int, default=240)
    ap.add_argument("--modes", nargs="*", default=list(MODES))
    ap.add_argument("--parts", nargs="*", default=["kernels", "lanes", "league"])
    ap.add_argument("--only-mode", default=None, help="(the kernels part's child run: one mode, nothing written)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    if args.only_mode:
        run_mode(tower(args.blocks), args, args.only_mode, trace_plies=args.trace_plies)
        return
    res = dict(game="connect4", games=args.games, sims=args.sims, threads=args.threads,
               net=f"ResidualTower(filter_factor=32, num_blocks={args.blocks}), random init, fp16 fused trunk",
               engine="LanedEngine, 2 lanes (0.48 / 0.52), leaf dedup, cross-lane dedup, cache window 1")
    if "kernels" in args.parts:  # first: the children run while this process holds no GPU memory
        res["kernels"] = dict(plies=args.trace_plies, **kernel_times(args))
    if "lanes" in args.parts:
        net = tower(args.blocks)
        res["lanes"] = [run_mode(net, args, mode) for mode in args.modes]
    if "league" in args.parts:
        res["league"] = [run_league(args, mode) for mode in args.modes]
    line = json.dumps(res, default=lambda o: o.tolist() if hasattr(o, "tolist") else str(o))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
