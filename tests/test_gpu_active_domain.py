"""The packed launch domain of a games-mode simulation step (csrc/spmcts.hip launch_rows): the per-slot
kernels -- dedup, scan, alias, encode, peer push, cache fill, the threaded expand -- run over the pending
slots of the searching trees (the active list) instead of all T = 2 G trees.  Nothing a search sees may
change: whole games against the oracle's threaded episodes at list sizes that leave a partly filled wave,
holes in the list and idle list entries; the row order; and flags left over from a tree's last search.
"""
import numpy as np
import pytest
import torch

from tests.parity_helpers import A_OF, NumpyRNG, RecordingRNG, TableNet, load_json, play_episode, run_g3_group

pytestmark = pytest.mark.gpu

K = 4
SIMS = 16


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from self_play_reinforcement_learning_amd import _lib

    _lib.lib()


# ----------------------------------------------------------------------------- ragged and holed lists
def _games(G):
    """G self-play games of 16 sims (game i in slot i: swap_sides = i odd, as the arena numbers them)."""
    return [dict(game="connect4", sims=SIMS, seed=31000 + 7 * i, swap_sides=bool(i & 1), evaluate=False,
                 salt_policy=1 + i % 3, salt_opponent=1 + i % 3) for i in range(G)]


@pytest.fixture(scope="module")
def counting_oracle():
    """The oracle's trees, also counting the terminal _set_node expansions (play_action on the move that
    ends the game): the arena drops both trees with the finished game instead (k_games_end_ply), so those
    are not among its terminal_leaves."""
    import oracle.selfplay as osp

    base = osp.OracleTree

    class CountingTree(base):
        def play_action(self, action):
            before = self.stats["terminal_leaves"]
            super().play_action(action)
            self.stats["set_node_terminal"] = (self.stats.get("set_node_terminal", 0)
                                               + self.stats["terminal_leaves"] - before)

    osp.OracleTree = CountingTree
    yield
    osp.OracleTree = base


_ORACLE = {}


def _oracle_game(g):
    """The oracle's threaded episode of game g, computed once: (result, Moves, the two trees' counters)."""
    if g["seed"] not in _ORACLE:
        net = TableNet(A_OF[g["game"]], g["salt_policy"])
        np.random.seed(g["seed"])
        base = NumpyRNG()
        r, moves, _, (pol, opp, _) = play_episode(g["game"], net, net, RecordingRNG(base), RecordingRNG(base), g["sims"],
                                                  swap_sides=g["swap_sides"], update=True, evaluate=False, threads=K)
        _ORACLE[g["seed"]] = (r, moves, [dict(pol.stats), dict(opp.stats)])
    return _ORACLE[g["seed"]]


@pytest.mark.parametrize("G,bpt", [(1, 0), (5, 0), (13, 0), (5, 4 * SIMS + 32)],
                         ids=["G1", "G5", "G13", "G5-recycled"])
def test_ragged_lists_match_oracle(counting_oracle, G, bpt):
    """Games mode, K = 4, 16 sims, no refill, played to the end: G = 1 (one lane group of one wave), 5 (a
    partly filled wave) and 13 (two expand waves; 52 slots, no multiple of the 256- and 512-thread
    blocks); list entries fall idle at the front, middle and end as games finish.  Move records and
    counters equal the oracle's threaded episodes bit for bit -- also with a node store of four searches'
    worth of blocks (k_compact over the same list)."""
    games = _games(G)
    moves, c = run_g3_group(games, search_threads=K, blocks_per_tree=bpt)
    oracle = [_oracle_game(g) for g in games]
    stats = [s for _, _, trees in oracle for s in trees]
    exp = dict(sims=sum(s["sims"] for s in stats), nn_leaves=sum(s["nn_evals"] - 1 for s in stats),  # - reset()'s
               terminal_leaves=sum(s["terminal_leaves"] - s.get("set_node_terminal", 0) for s in stats),
               depth_sum=sum(s["depth_sum"] for s in stats), leaked_sims=sum(s["leaks"] for s in stats))
    print({k: (c[k], v) for k, v in exp.items()}, "compactions", c["compactions"])
    assert c["error_flags"] == 0 and c["games_finished"] == G
    assert (c["compactions"] > 0) == (bpt > 0)
    exp_results = np.zeros((2, 3), dtype=np.int64)
    by_game = {}
    for i in range(len(moves["z"])):
        by_game.setdefault(int(moves["game"][i]), []).append(i)
    for gi, (g, (r, exp_moves, _)) in enumerate(zip(games, oracle)):
        exp_results[int(g["swap_sides"])][{1: 0, 0: 1, -1: 2}[r]] += 1
        rows = by_game.get(gi, [])
        assert len(rows) == len(exp_moves), gi
        for i, M in zip(rows, exp_moves):
            assert moves["state"][i].astype(int).tolist() == M["state"].reshape(-1).astype(int).tolist(), (gi, i)
            assert float(moves["z"][i]) == float(M["actual_val"]), (gi, i)
            assert moves["tree_probs"][i].astype(float).tolist() == M["tree_probs"].astype(float).tolist(), (gi, i)
            q = np.float64(moves["q"][i]) if moves["q_f64"][i] else np.float32(moves["q"][i])
            assert float(q) == float(M["q"]), (gi, i)
    assert np.array_equal(np.array(c["results"]), exp_results)
    for k, v in exp.items():
        assert c[k] == v, k


# ----------------------------------------------------------------------------- idle sides, two segments
def _g5_first(opponent, n=5):
    """The first n games of the Connect4 evaluation fixture against `opponent` with default kwargs (game i
    keeps slot i, so swap_sides stays the arena's)."""
    games = [g for g in load_json("arena_games.json")
             if g["game"] == "connect4" and g["opponent"] == opponent and not g.get("policy_kwargs")
             and not g.get("opponent_kwargs")]
    key = (games[0]["sims"], games[0]["opponent_sims"])
    games = [g for g in games if (g["sims"], g["opponent_sims"]) == key][:n]
    assert len(games) == n and all(g["swap_sides"] == bool(i & 1) for i, g in enumerate(games))
    return games


@pytest.mark.parametrize("opponent,k0,k1", [("lookahead", K, None), ("mcts", K, 1)], ids=["lookahead", "mcts-K4v1"])
def test_evaluation_arena_matches_oracle(opponent, k0, k1):
    """An evaluation arena of 5 games: against OneStepLookahead the list entry of a game is empty (-1) on
    the plies its hard-coded side moves; against a second network the searching trees send rows to both
    segments, the policy with 4 sims in flight and the opponent with 1.  Bit-identical to the oracle."""
    from tests.parity_helpers import run_g5_group

    games = _g5_first(opponent)
    moves, c, oracle, rows = run_g5_group(games, search_threads=k0, opponent_threads=k1)
    assert c["error_flags"] == 0 and c["games_finished"] == len(games)
    if opponent == "mcts":
        assert rows[0] > 0 and rows[1] > 0
    by_game = {}
    for i in range(len(moves["z"])):
        by_game.setdefault(int(moves["game"][i]), []).append(i)
    exp = np.zeros((2, 3), dtype=np.int64)
    for gi, (g, (r, omoves, _, _)) in enumerate(zip(games, oracle)):
        exp[int(g["swap_sides"])][{1: 0, 0: 1, -1: 2}[r]] += 1
        got = by_game.get(gi, [])
        assert len(got) == len(omoves), gi
        for i, M in zip(got, omoves):
            assert moves["state"][i].astype(int).tolist() == M["state"].reshape(-1).astype(int).tolist(), (gi, i)
            assert float(moves["z"][i]) == float(M["actual_val"]), (gi, i)
            assert moves["tree_probs"][i].astype(float).tolist() == M["tree_probs"].astype(float).tolist(), (gi, i)
            q = np.float64(moves["q"][i]) if moves["q_f64"][i] else np.float32(moves["q"][i])
            assert float(q) == float(M["q"]), (gi, i)
    assert np.array_equal(np.array(c["results"]), exp)


# ----------------------------------------------------------------------------- row order
def _row_slots(arena, n):
    """Pending slot (tree * K + j) of each of the first n leaf rows."""
    from self_play_reinforcement_learning_amd._lib import call, ptr
    from self_play_reinforcement_learning_amd.arena import _stream

    out = torch.empty(arena.n_trees * arena.search_threads, dtype=torch.int32, device=arena.device)
    call("spmcts_leaf_trees", arena.h, ptr(out), _stream())
    return out[:n].cpu().numpy().astype(int)


def _table_step(arena, n):
    from self_play_reinforcement_learning_amd.arena import table_net_eval

    p, v = table_net_eval(arena.game, arena.leaves(n), arena.leaf_format, arena.leaf_layout, salt=5)
    arena.expand(p, v)


def test_rows_in_slot_order_games_mode():
    """Games mode, G = 13: the rows of every simulation step are the pending slots in ascending order (one
    network segment), all of searching trees -- at the first step exactly the K slots of each game's mover,
    list order = tree order -- and leaf_trees gives their trees, non-decreasing."""
    from self_play_reinforcement_learning_amd.arena import Arena

    G = 13
    arena = Arena("connect4", n_trees=2 * G, n_games=G, iterations=SIMS, seed=3, search_threads=K)
    arena.games_set_limit(G)
    arena.games_start(list(range(G)))
    for ply in range(3):
        # game g's mover: tree 2 g + ((ply + swap) & 1), swap = g odd
        movers = [2 * g + ((ply + (g & 1)) & 1) for g in range(G)]
        arena.games_begin_ply()
        for step in range(SIMS // K):
            n = arena.select()
            slots = _row_slots(arena, n)
            trees = arena.leaf_trees(n).cpu().numpy().astype(int)
            assert n > 0 and (np.diff(slots) > 0).all(), (ply, step, slots)
            assert trees.tolist() == (slots // K).tolist() and (np.diff(trees) >= 0).all()
            assert set(trees.tolist()) <= set(movers), (ply, step)
            if step == 0:  # every slot of every mover is pending: nothing is terminal this early
                assert slots.tolist() == [t * K + j for t in movers for j in range(K)], ply
            _table_step(arena, n)
        n = arena.games_end_ply()
        if n:
            _table_step(arena, n)
        arena.games_finish_ply(refill=False)
    arena.check()
    arena.close()


def test_rows_in_tree_order_for_a_permuted_search_list():
    """spmcts_search_begin with trees 5, 2, 7 of an 8-tree arena: the rows come out in tree order 2, 5, 7
    (K slots each at the first step), whatever the order of the caller's list."""
    from self_play_reinforcement_learning_amd.arena import Arena

    arena = Arena("connect4", n_trees=8, iterations=SIMS, seed=3, search_threads=K)
    arena.tree_reset(list(range(8)), [1] * 8)
    arena.search_begin([5, 2, 7])
    for step in range(SIMS // K):
        n = arena.select()
        slots = _row_slots(arena, n)
        assert (np.diff(slots) > 0).all() and set((slots // K).tolist()) <= {2, 5, 7}, (step, slots)
        if step == 0:
            assert arena.leaf_trees(n).cpu().numpy().tolist() == [2] * K + [5] * K + [7] * K
        _table_step(arena, n)
    arena.search_end(1.0)
    arena.check()
    arena.close()


# ----------------------------------------------------------------------------- stale flags across plies
def test_flags_of_idle_trees_do_not_leak_across_plies():
    """Two lanes of 11 + 13 games with cross-lane dedup and an evaluation cache of window 1, 28 plies with
    refill: every tree searches on one ply and idles on the next, keeping the owner / served flags
    (down, xpeer, xc, dent, srow) of its last search while the other tree of its game searches.  The same
    seeds with the cache, cross-lane dedup and leaf dedup off give the same Move records and counters."""
    from self_play_reinforcement_learning_amd.engine import LanedEngine
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    torch.manual_seed(0)
    net = ResidualTower(7, 6, 7, num_blocks=2, filter_factor=32).cuda().eval()
    out = []
    for on in (False, True):
        eng = LanedEngine("connect4", net, n_games=24, lanes=2, lane_sizes=[11, 13], iterations=SIMS, seed=7,
                          search_threads=K, max_games=96, cross_dedup=on, leaf_dedup=on, eval_cache=1 if on else 0)
        assert eng.cross_dedup == on and eng.leaf_dedup == on and eng.eval_cache == (1 if on else 0)
        got = []
        eng.run(plies=28, on_moves=lambda m: got.append({k: v.cpu().numpy() for k, v in m.items()}))
        eng.check()
        out.append(({k: np.concatenate([g[k] for g in got]) for k in got[0]}, eng.counters()))
    (m0, c0), (m1, c1) = out
    assert len(m0["z"]) > 0 and c0["games_finished"] > 0
    for k in m0:
        np.testing.assert_array_equal(m0[k], m1[k], err_msg=k)
    for k in ("sims", "leaked_sims", "moves", "nn_leaves", "terminal_leaves", "depth_sum", "games_finished",
              "positions_exported", "results"):
        assert c0[k] == c1[k], k
    assert c0["nn_rows"] == c0["nn_leaves"] and c0["cache_rows"] == 0
    assert c1["cache_rows"] > 0 and c1["nn_rows"] + c1["cache_rows"] < c1["nn_leaves"]
