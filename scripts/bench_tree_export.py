"""What reading the trees costs (csrc/arena_tree.h): spmcts_tree_pv_batch and spmcts_tree_export_batch(min_visits=1)
over --trees trees after one --sims-simulation search (--threads sims in flight, the table net, Connect4 from the
empty board), with spmcts_root_stats_batch on the same arena in the same run as the yardstick.

Each entry point writes into buffers allocated once and is timed alone with device events: one warm-up call, then
--repeats timed calls, the median reported (every call's time listed).  The export's rows hold --max-nodes entries
(default: simulations + 8, enough for every node of one search); `nodes` is the trees' node counts, `bytes` what the
export's kernel writes per call (output fields and work words of the listed nodes).

    python scripts/bench_tree_export.py [--out profiles/tree_export/bench.json]   -> one JSON line
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, repeats):
    import torch

    fn()  # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(us=[round(1e3 * x, 1) for x in ms], us_median=round(1e3 * statistics.median(ms), 1))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trees", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=200)
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--max-nodes", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from self_play_reinforcement_learning_amd.arena import Arena, _stream, table_net_eval
    from self_play_reinforcement_learning_amd._lib import call, ptr

    game, T, K = "connect4", args.trees, args.threads
    M = args.max_nodes or args.sims + 8
    a = Arena(game, n_trees=T, iterations=args.sims, seed=11, leaf_format="f32", leaf_layout="nchw", search_threads=K)
    ids = list(range(T))
    a.tree_reset(ids, [1] * T)
    a.search_begin(ids)
    for _ in range(-(-args.sims // K)):
        n = a.select()
        if n:
            p, v = table_net_eval(game, a.leaves(n), a.leaf_format, a.leaf_layout)
            a.expand(p, v)
    a.check()
    dev, L = a.device, a.cells
    t = a._dev_i32(ids)

    rs = a.root_stats_batch(t)
    pv = a.pv_batch(t)
    ex = a.export_subtrees(t, M)
    nbytes = ctypes.c_uint64()
    call("spmcts_tree_export_work_bytes", a.h, T, M, ctypes.byref(nbytes))
    work = torch.empty(nbytes.value // 8, dtype=torch.int64, device=dev)

    def run_rs():
        call("spmcts_root_stats_batch", a.h, ptr(t), T, ptr(rs["child_n"]), ptr(rs["child_w"]), ptr(rs["child_p"]),
             ptr(rs["root_n"]), ptr(rs["root_w"]), ptr(rs["root_player"]), ptr(rs["board"]), _stream())

    def run_pv():
        call("spmcts_tree_pv_batch", a.h, ptr(t), T, L, 1, ptr(pv["pv"]), ptr(pv["pv_n"]), ptr(pv["pv_vl"]),
             ptr(pv["pv_w"]), ptr(pv["pv_p"]), ptr(pv["pv_len"]), ptr(pv["pv_end"]), ptr(pv["end_board"]), _stream())

    def run_ex():
        call("spmcts_tree_export_batch", a.h, ptr(t), T, M, 1, -1, *[ptr(ex[k]) for k, _, _ in Arena.EXPORT_FIELDS],
             ptr(ex["count"]), ptr(work), nbytes.value, _stream())

    res = dict(game=game, trees=T, sims=args.sims, threads=K, max_nodes=M, repeats=args.repeats,
               root_stats_batch=timed(run_rs, args.repeats), pv_batch=timed(run_pv, args.repeats),
               export_subtrees=timed(run_ex, args.repeats))
    a.check()
    count = ex["count"].cpu().numpy()
    plen = pv["pv_len"].cpu().numpy()
    listed = int(count.clip(max=M).sum())
    per_node = 4 + 1 + 2 + 4 + 4 + 8 + 4 + 1 + 1 + 24  # the nine output fields and three work words
    res["nodes"] = dict(sum=int(count.sum()), min=int(count.min()), median=float(statistics.median(count.tolist())),
                        max=int(count.max()), truncated=int((count > M).sum()))
    res["pv_len"] = dict(min=int(plen.min()), median=float(statistics.median(plen.tolist())), max=int(plen.max()))
    res["export_subtrees"]["bytes"] = listed * per_node
    res["export_subtrees"]["ns_per_node"] = round(1e3 * res["export_subtrees"]["us_median"] / max(listed, 1), 3)
    res["export_subtrees"]["ns_per_tree"] = round(1e3 * res["export_subtrees"]["us_median"] / T, 1)
    res["pv_batch"]["ns_per_tree"] = round(1e3 * res["pv_batch"]["us_median"] / T, 1)
    res["root_stats_batch"]["ns_per_tree"] = round(1e3 * res["root_stats_batch"]["us_median"] / T, 1)
    a.close()
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
