"""Generate the fixtures of the Connect4 variant boards (6x5 "connect4_6_5", 8x7 "connect4_8_7") by running
the REFERENCE itself, with make_golden.py's conventions: the reference is imported by path through
tests/golden/refshims, nothing of it is copied, and only inputs and the outputs it produced are written.
Where the reference is absent the script says so and writes nothing.

    python tests/golden/make_variant_golden.py

Per board (tag c4_6x5 / c4_8x7):
  env_kat_<tag>.npz         Connect4Env(W, H).step known answers, env_kat_c4.npz's record layout (ValueError and
                            GameOver rows included); coverage is asserted before writing: a win in each of the
                            four directions, wins whose run touches column 0, the last column, row 0 and the top
                            row, and a full-board draw (from games whose movers avoid winning moves)
  mcts_search_<tag>.json    as gen_mcts_search: 24 cases at 25 sims, 6 at 200 sims (2 of them strong_play)
  selfplay_games_<tag>.json as gen_selfplay_games at 25 sims: 4 self-play games, 2 evaluate-mode games
  arena_games_<tag>.json    as gen_arena_games at 25 sims: 2 games against OneStepLookahead
Every file is held to the size of the smallest G1 / G2 / G3 fixture (env_kat_ttt.npz).
"""
import functools
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (sets up sys.path for the reference, the shims and the repository)
from oracle.table_net import TableNet  # noqa: E402

BOARDS = [("c4_6x5", "connect4_6_5", 6, 5), ("c4_8x7", "connect4_8_7", 8, 7)]
MAX_BYTES = os.path.getsize(os.path.join(HERE, "env_kat_ttt.npz"))


# ----------------------------------------------------------------------------- env KATs
def _win_facts(board, x, y, p):
    """Directions ("h", "v", "d1", "d2") in which the stone at (x, y) completes a run of >= 4 of p, and which
    board edges those runs touch."""
    W, H = board.shape
    dirs, touch = set(), set()
    for name, (dx, dy) in {"h": (1, 0), "v": (0, 1), "d1": (1, 1), "d2": (1, -1)}.items():
        cells = [(x, y)]
        for s in (1, -1):
            cx, cy = x + s * dx, y + s * dy
            while 0 <= cx < W and 0 <= cy < H and board[cx, cy] == p:
                cells.append((cx, cy))
                cx, cy = cx + s * dx, cy + s * dy
        if len(cells) >= 4:
            dirs.add(name)
            for cx, cy in cells:
                if cx == 0:
                    touch.add("col0")
                if cx == W - 1:
                    touch.add("colW")
                if cy == 0:
                    touch.add("row0")
                if cy == H - 1:
                    touch.add("rowH")
    return dirs, touch


def gen_env_kat(Connect4Env, GameOver, W, H, n_games=300, seed=4321):
    rng = random.Random(seed + 100 * W + H)
    cols = {k: [] for k in ("before", "after", "action", "player", "reward", "done", "valid", "status", "game_id",
                            "ply")}
    cover = {k: 0 for k in ("h", "v", "d1", "d2", "col0", "colW", "row0", "rowH", "draw")}

    def row(b0, b1, a, p, r, d, valid, st, g, k):
        for key, v in zip(cols, (b0.astype(np.int8), b1.astype(np.int8), a, p, r, bool(d), valid.astype(np.bool_), st,
                                 g, k)):
            cols[key].append(v)

    def winning(env, a, p):
        e2 = Connect4Env(W, H)
        e2.reset()
        e2.set_state(env.board.copy())
        _, r, _, _ = e2.step(a, p)
        return r != 0

    def play(g, avoid_wins):
        """One game; avoid_wins: the mover picks among the moves that do not win, while there is one."""
        env = Connect4Env(W, H)
        env.reset()
        p = 1 if g % 2 == 0 else -1
        k = 0
        rows = []
        while True:
            legal = [i for i, m in enumerate(env.valid_moves()) if m]
            if avoid_wins:
                quiet = [a for a in legal if not winning(env, a, p)]
                legal = quiet or legal
            a = rng.choice(legal)
            b0 = env.board.copy()
            s, r, d, _ = env.step(a, p)
            rows.append((b0, s.copy(), a, p, r, d, env.valid_moves(), 0, g, k))
            k += 1
            if d:
                b1 = env.board.copy()  # a step after the game is over raises GameOver
                try:
                    env.step(a, -p)
                    st = 0
                except GameOver:
                    st = 2
                except ValueError:
                    st = 1
                rows.append((b1, env.board.copy(), a, -p, 0, True, env.valid_moves(), st, g, k))
                facts = (_win_facts(s, a, int(np.sum(np.abs(s[a]))) - 1, p) if r else (set(), set()), r == 0)
                return rows, facts
            p = -p

    def keep(rows, facts):
        for r_ in rows:
            row(*r_)
        (dirs, touch), draw = facts
        for k in list(dirs) + list(touch):
            cover[k] += 1
        cover["draw"] += int(draw)

    for g in range(n_games):
        keep(*play(g, False))
        if g % 10 == 0:  # the full-column error path on a fresh env
            env2 = Connect4Env(W, H)
            env2.reset()
            col = rng.randrange(W)
            q = 1
            for _ in range(H):
                env2.step(col, q)  # alternating pieces: no vertical four
                q = -q
            b0 = env2.board.copy()
            try:
                env2.step(col, 1)
                st = 0
            except ValueError:
                st = 1
            row(b0, env2.board.copy(), col, 1, 0, False, env2.valid_moves(), st, -1, -1)
    # whatever random play left uncovered (a full-board draw on 8x7, typically): games whose movers avoid winning
    # moves, kept only when they add coverage
    g = n_games
    for _ in range(20000):
        if all(cover.values()):
            break
        rows, facts = play(g, True)
        (dirs, touch), draw = facts
        if any(cover[k] == 0 for k in list(dirs) + list(touch)) or (draw and not cover["draw"]):
            keep(rows, facts)
            g += 1
    assert all(cover.values()), f"{W}x{H}: coverage incomplete {cover}"
    st = np.array(cols["status"], np.int8)
    assert (st == 1).any() and (st == 2).any(), "ValueError / GameOver rows"
    print(f"  {W}x{H}: {g} games, {len(st)} rows, coverage {cover}")
    return dict(
        before=np.stack(cols["before"]), after=np.stack(cols["after"]), action=np.array(cols["action"], np.int8),
        player=np.array(cols["player"], np.int8), reward=np.array(cols["reward"], np.int8),
        done=np.array(cols["done"]), valid=np.stack(cols["valid"]), status=st,
        game_id=np.array(cols["game_id"], np.int32), ply=np.array(cols["ply"], np.int16),
    )


# ----------------------------------------------------------------------------- searches
def gen_searches(ref_mcts, EnvCls, game, A, W, H):
    MCTreeSearch = ref_mcts.MCTreeSearch
    plan = [(25, 24, W + H - 1, False), (200, 4, W + H + 1, False), (200, 2, 2 * W + H, True)]
    cases = []
    cid = 0
    for sims, count, max_open, strong in plan:
        for k in range(count):
            rng = random.Random(1000 * sims + k + (7 if strong else 0) + 100000 * W + 10000 * H)
            opening = mg._random_opening(EnvCls, rng, max_open)
            seed = 30_000 + 1000 * W + cid
            salt = (cid + 1) * 7919 + W
            net = TableNet(A, salt=salt)
            np.random.seed(seed)
            tree = MCTreeSearch(network=net, env=EnvCls, iterations=sims, strong_play=strong)
            for a in opening:
                tree.play_action(a, None)
            root_player = int(tree.root_node.player)
            tree.train(False)
            tree.evaluate(False)
            action = tree()
            root = tree.root_node
            mv = tree.temp_memory[-1] if tree.temp_memory else None
            kids = root.children
            cases.append(dict(
                id=cid, game=game, sims=sims, seed=seed, salt=salt, strong_play=strong, opening=opening,
                root_player=root_player, action=int(action), child_n=[int(c.n) for c in kids],
                child_w=[float(c.w) for c in kids], root_n=int(root.n), root_w=float(root.w), recorded=mv is not None,
                state=(mv.state.numpy().astype(int).reshape(-1).tolist() if mv else None),
                tree_probs=(mv.tree_probs.numpy().astype(float).tolist() if mv else None),
                q=(float(mv.q) if mv else None), net_calls=net.calls,
            ))
            cid += 1
    return cases


# ----------------------------------------------------------------------------- whole games
def gen_selfplay(ref_mcts, SelfPlayer, EnvCls, game, A, W):
    MCTreeSearch = ref_mcts.MCTreeSearch
    orig_play = MCTreeSearch._play
    log = []

    def spy_play(self, temp=0.05):
        root = self.root_node
        pre = dict(tree=getattr(self, "_golden_tree", -1), child_n=[int(c.n) for c in root.children],
                   child_w=[float(c.w) for c in root.children], root_n=int(root.n), root_w=float(root.w))
        a = orig_play(self, temp)
        pre["action"] = int(a)
        mv = self.temp_memory[-1] if self.temp_memory else None
        pre["tree_probs"] = mv.tree_probs.numpy().astype(float).tolist() if mv else None
        pre["q"] = float(mv.q) if mv else None
        log.append(pre)
        return a

    MCTreeSearch._play = spy_play
    games = []
    gid = 0
    sims = 25
    try:
        for count, evaluate in ((4, False), (2, True)):
            for k in range(count):
                seed = 40_000 + 100 * W + gid
                swap = bool(k % 2)
                salt_p = 3 * gid + 1 + 1000 * W
                salt_o = salt_p if not evaluate else salt_p + 1
                np.random.seed(seed)
                mq, rq = mg._ListQueue(), mg._ListQueue()
                net_p = TableNet(A, salt=salt_p)
                net_o = net_p if not evaluate else TableNet(A, salt=salt_o)
                pol = MCTreeSearch(network=net_p, env=EnvCls, memory_queue=mq, iterations=sims)
                pol.train(False)
                opp = MCTreeSearch(network=net_o, env=EnvCls, memory_queue=mq, iterations=sims)
                opp.env = EnvCls()
                opp.train(False)
                pol.evaluate(evaluate)
                opp.evaluate(evaluate)
                pol._golden_tree = 0
                opp._golden_tree = 1
                sp = SelfPlayer(pol, opp, EnvCls(), rq)
                del log[:]
                _, r = sp.play_episode(swap_sides=swap, update=not evaluate)
                moves = [dict(state=m.state.numpy().astype(int).reshape(-1).tolist(), actual_val=float(m.actual_val),
                              tree_probs=m.tree_probs.numpy().astype(float).tolist(), q=float(m.q)) for m in mq.items]
                games.append(dict(
                    id=gid, game=game, sims=sims, seed=seed, swap_sides=swap, evaluate=evaluate, salt_policy=salt_p,
                    salt_opponent=salt_o, result=int(r),
                    results_queue=[dict(reward=int(x["reward"]), swap_sides=bool(x["swap_sides"])) for x in rq.items],
                    plies=[dict(x) for x in log], moves=moves,
                ))
                gid += 1
    finally:
        MCTreeSearch._play = orig_play
    return games


def gen_lookahead(ref_mcts, SelfPlayer, EnvCls, game, A, W):
    from games.general import hardcoded_players as hp

    MCTreeSearch = ref_mcts.MCTreeSearch
    orig_play, orig_random = MCTreeSearch._play, hp.random
    log, choices = [], []

    def spy_play(self, temp=0.05):
        root = self.root_node
        pre = dict(tree=getattr(self, "_golden_tree", -1), child_n=[int(c.n) for c in root.children],
                   child_w=[float(c.w) for c in root.children], root_n=int(root.n), root_w=float(root.w))
        a = orig_play(self, temp)
        pre["action"] = int(a)
        log.append(pre)
        return a

    MCTreeSearch._play = spy_play
    hp.random = mg._ChoiceSpy(choices)
    games = []
    sims = 25
    try:
        for gid in range(2):
            seed = 60_000 + 100 * W + gid
            swap = bool(gid % 2)
            salt_p, salt_o = 5 * gid + 1 + 1000 * W, 5 * gid + 2 + 1000 * W
            np.random.seed(seed)
            random.seed(seed)
            rq = mg._ListQueue()
            pol = MCTreeSearch(network=TableNet(A, salt=salt_p), env=EnvCls, memory_queue=None, iterations=sims)
            pol.train(False)
            opp = hp.OneStepLookahead(env=EnvCls)
            opp.env = EnvCls()
            opp.train(False)
            pol.evaluate(True)
            opp.evaluate(True)
            pol._golden_tree = 0
            sp = SelfPlayer(pol, opp, EnvCls(), rq)
            del log[:]
            del choices[:]
            states, r = sp.play_episode(swap_sides=swap, update=False)
            games.append(dict(
                id=gid, game=game, sims=sims, opponent="lookahead", opponent_sims=0, seed=seed, policy_kwargs={},
                opponent_kwargs={}, swap_sides=swap, salt_policy=salt_p, salt_opponent=salt_o, result=int(r),
                results_queue=[dict(reward=int(x["reward"]), swap_sides=bool(x["swap_sides"])) for x in rq.items],
                plies=[dict(x) for x in log], choices=[list(c) for c in choices],
                final_board=np.asarray(states[-1]).astype(int).reshape(-1).tolist(),
            ))
    finally:
        MCTreeSearch._play = orig_play
        hp.random = orig_random
    return games


def _write_json(name, obj):
    path = os.path.join(HERE, name)
    with open(path, "w") as f:
        json.dump(obj, f, separators=(",", ":"))
    _check_size(path)


def _check_size(path):
    n = os.path.getsize(path)
    assert n <= MAX_BYTES, f"{os.path.basename(path)}: {n} bytes > {MAX_BYTES}"
    print(f"  {os.path.basename(path)}: {n} bytes")


def main():
    if not os.path.isdir(mg.REF):
        print(f"reference not found at {mg.REF}: nothing written")
        return
    ref_mcts, SelfPlayer, Connect4Env, _, GameOver, _ = mg._ref_imports()
    for tag, game, W, H in BOARDS:
        EnvCls = functools.partial(Connect4Env, W, H)
        assert EnvCls().variant_string() == game
        print(f"{game}: env KAT ...", flush=True)
        path = os.path.join(HERE, f"env_kat_{tag}.npz")
        np.savez_compressed(path, **gen_env_kat(Connect4Env, GameOver, W, H))
        _check_size(path)
        print(f"{game}: searches ...", flush=True)
        _write_json(f"mcts_search_{tag}.json", gen_searches(ref_mcts, EnvCls, game, W, W, H))
        print(f"{game}: whole games ...", flush=True)
        _write_json(f"selfplay_games_{tag}.json", gen_selfplay(ref_mcts, SelfPlayer, EnvCls, game, W, W))
        _write_json(f"arena_games_{tag}.json", gen_lookahead(ref_mcts, SelfPlayer, EnvCls, game, W, W))
    print("done")


if __name__ == "__main__":
    main()
