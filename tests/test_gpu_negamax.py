"""GPU: the negamax kernels (csrc/negamax.h) against their host twin, solve_positions, the arena player replayed on
the host, and the engines' wiring."""
import ctypes

import numpy as np
import pytest
import torch

from self_play_reinforcement_learning_amd import _lib
from self_play_reinforcement_learning_amd.arena import GAMES
from tests import negamax_helpers as nh
from tests.variant_helpers import variant_oracle  # noqa: F401

pytestmark = pytest.mark.gpu
X = nh.X
_HOST = {}


def host(game, index, depth):
    """(codes, nodes) of position `index` of the generator from the host twin, computed once."""
    key = (game, index, depth)
    if key not in _HOST:
        board, player = nh.positions(game)[index]
        codes, nodes = nh.host_codes(game, board, player, depth)
        _HOST[key] = (codes.copy(), nodes)
    return _HOST[key]


def device_batch(game, indices, depth, want_nodes=True):
    """spmcts_negamax_batch over the listed positions of the generator -> (codes [n, A], nodes [n])."""
    gid, W, H, A = GAMES[game]
    pos = nh.positions(game)
    n = len(indices)
    boards = torch.as_tensor(np.stack([pos[i][0] for i in indices]) if n else np.zeros((0, W, H), np.int8)).cuda()
    players = torch.as_tensor(np.array([pos[i][1] for i in indices], dtype=np.int8)).cuda()
    score = torch.full((max(n, 1), A), 77, dtype=torch.int8, device="cuda")
    nodes = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
    _lib.call("spmcts_negamax_batch", gid, W, H, _lib.ptr(boards), _lib.ptr(players), n, depth, _lib.ptr(score),
              _lib.ptr(nodes) if want_nodes else None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return score.cpu().numpy(), nodes.cpu().numpy()


@pytest.mark.parametrize("game", nh.BOARDS)
def test_device_matches_host_twin(game):
    """Batches of 0, 1, 2, 65 and 257 positions (a position's A * A items inside one wave, across two, over many
    blocks) at depths 1, 2 (no grandchild search), 3, 6 and 7 (odd and even horizons), bit-equal to the host twin,
    node counts included and the same in a second run."""
    pos = nh.positions(game)
    for depth in (1, 2, 3, 6, 7):
        # the deep horizons run on every third position (random playouts and carved boards alike)
        pool = list(range(len(pos))) if depth <= 3 else list(range(0, len(pos), 3))
        for n in (0, 1, 2, 65, 257):
            idx = [pool[(5 * n + k) % len(pool)] for k in range(n)]
            score, nodes = device_batch(game, idx, depth)
            if n == 0:
                assert (score == 77).all() and (nodes == -1).all()  # a no-op
                continue
            for k, i in enumerate(idx):
                codes, made = host(game, i, depth)
                assert score[k].tolist() == codes.tolist(), (game, depth, n, k, i)
                assert nodes[k] == made and made > 0, (game, depth, n, k, i)
            if n == 65:
                score2, nodes2 = device_batch(game, idx, depth)
                assert (score2 == score).all() and (nodes2 == nodes).all()
                score3, nodes3 = device_batch(game, idx, depth, want_nodes=False)
                assert (score3 == score).all() and (nodes3 == -1).all()


@pytest.mark.parametrize("game", nh.BOARDS)
def test_device_at_the_depth_cap(game):
    gid, W, H, A = GAMES[game]
    cap = _lib.lib().spmcts_negamax_max_depth(gid, W, H)
    idx = [3, 11, 29, len(nh.positions(game)) - 1]
    score, nodes = device_batch(game, idx, cap)
    for k, i in enumerate(idx):
        codes, made = host(game, i, cap)
        assert score[k].tolist() == codes.tolist() and nodes[k] == made, (game, i)


def test_a_batch_split_into_launches_equals_its_pieces():
    """TicTacToe at depth 9: the launch bound (positions * sum 9^k) admits fewer than half of 65 positions, so
    the batch takes several launches; the result is that of each piece solved on its own, and the host twin's."""
    game = "tictactoe"
    gid, W, H, A = GAMES[game]
    per = _lib.lib().spmcts_negamax_launch_positions(gid, W, H, 9)
    pool = list(range(len(nh.positions(game))))
    idx = [pool[(7 * k) % len(pool)] for k in range(65)]
    assert 1 <= per < len(idx) / 2
    score, nodes = device_batch(game, idx, 9)
    for lo in range(0, len(idx), per):
        piece = idx[lo:lo + per]
        s, m = device_batch(game, piece, 9)
        assert (s == score[lo:lo + len(piece)]).all() and (m == nodes[lo:lo + len(piece)]).all()
    for k, i in enumerate(idx):
        codes, made = host(game, i, 9)
        assert score[k].tolist() == codes.tolist() and nodes[k] == made


def test_solve_positions_known_answers():
    from self_play_reinforcement_learning_amd import solve_positions

    for game in nh.BOARDS:
        rows = [(moves, D, codes) for g, moves, depths, codes in nh.KNOWN if g == game for D in depths]
        for D in sorted({r[1] for r in rows}):
            sel = [r for r in rows if r[1] == D]
            out = solve_positions(game, positions=[r[0] for r in sel], depth=D)
            score = out["score"].cpu().numpy()
            assert out["score"].dtype == torch.int8 and out["value"].dtype == torch.int8
            assert out["best"].dtype == torch.bool and out["nodes"].dtype == torch.int64
            for k, (moves, _, codes) in enumerate(sel):
                assert score[k].tolist() == codes, (game, moves, D)
                legal = [c for c in codes if c != X]
                value = max(legal, key=nh.rank)
                assert int(out["value"][k]) == value
                assert out["best"][k].tolist() == [c == value for c in codes]
                assert int(out["nodes"][k]) > 0
                if not moves and (game, D) in nh.FULL_WIDTH:
                    assert int(out["nodes"][k]) == nh.FULL_WIDTH[(game, D)]
    # boards= with players= is the same solver
    pos = nh.positions("connect4")
    out = solve_positions("connect4", boards=np.stack([b for b, _ in pos]), players=[p for _, p in pos], depth=4)
    for k in range(len(pos)):
        assert out["score"][k].cpu().tolist() == host("connect4", k, 4)[0].tolist()
    assert solve_positions("connect4", positions=[], depth=3)["score"].shape == (0, 7)
    for bad in (0, 9, 2.0):
        with pytest.raises(ValueError):
            solve_positions("connect4", positions=[[]], depth=bad)


def _league_replay(game, seed):
    """negamax(2) v random, negamax(4) v lookahead, negamax(3) v negamax(5): 32 slots each, tape RNG, no network;
    every slot's result and ply count against the host replay on the same tapes."""
    from self_play_reinforcement_learning_amd.engine import LeagueEngine

    players = [dict(kind="negamax", depth=2), dict(kind="random"), dict(kind="negamax", depth=4),
               dict(kind="lookahead"), dict(kind="negamax", depth=3), dict(kind="negamax", depth=5)]
    pairings = [(0, 1), (2, 3), (4, 5)]
    eng = LeagueEngine(game, players, pairings, games_per_pairing=32, rng="tape")
    cells = eng.arena.cells
    rng = np.random.default_rng(seed)
    tapes = [rng.random(cells).tolist() for _ in range(2 * eng.n_slots)]
    eng.arena.set_tapes(tapes)
    eng.play()
    c = eng.counters()
    r = eng.arena.games_results()
    eng.close()
    assert c["error_flags"] == 0 and c["games_finished"] == 96 and c["sims"] == 0
    assert (r["state"] != 1).all()
    seen = set()
    for first, i, j in eng.schedule:
        for s in range(first, first + eng.g):
            swap = bool(s & 1)
            assert bool(r["swap"][s]) == swap
            res, ply = nh.replay_game(game, players[i], players[j], tapes[2 * s], tapes[2 * s + 1], swap)
            assert (int(r["result"][s]), int(r["ply"][s])) == (res, ply), (game, s, i, j)
            seen.add(res)
    assert len(seen) >= 2  # the games are not all one result


def test_arena_player_replays_on_the_host():
    _league_replay("connect4", 5)


def test_arena_player_replays_on_the_host_6x5(variant_oracle):  # noqa: F811
    _league_replay("connect4_6_5", 6)


def test_set_tree_players_depth_limits():
    from self_play_reinforcement_learning_amd.arena import Arena

    a = Arena("connect4", n_trees=4, n_games=2, iterations=4)
    kinds = [_lib.PLAYER_NEGAMAX, _lib.PLAYER_RANDOM] * 2
    for budgets in (None, [0, 0, 1, 0], [7, 0, 1, 0], [-1, 0, 1, 0]):
        with pytest.raises(_lib.SpmctsError, match="depth"):
            a.set_tree_players(kinds=kinds, budgets=budgets)
    a.set_tree_players(kinds=kinds, budgets=[6, 0, 1, 0])
    with pytest.raises(_lib.SpmctsError, match="unknown player kind"):
        a.set_tree_players(kinds=[4, 0, 0, 0], budgets=[1, 1, 1, 1])
    a.close()


def test_engine_with_a_negamax_opponent():
    """test_hardcoded_opponents_on_device's assertions with opponent="negamax"."""
    from self_play_reinforcement_learning_amd.engine import SelfPlayEngine
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    torch.manual_seed(0)
    net = ResidualTower(7, 6, 7, num_blocks=2, filter_factor=32).cuda().eval()
    eng = SelfPlayEngine("connect4", network=net, opponent="negamax", opponent_depth=3, n_games=64, iterations=8,
                         seed=2, max_games=64, evaluate=True)
    got = []
    eng.run(games=64, on_moves=lambda m: got.append({k: v.cpu().numpy() for k, v in m.items()}))
    eng.check()
    moves = {k: np.concatenate([g[k] for g in got]) for k in got[0]}
    c = eng.counters()
    assert c["games_finished"] == 64 and c["error_flags"] == 0
    assert np.array(c["results"]).sum() == 64
    # only the policy's moves are recorded; the policy's tree searched every one of its plies
    assert c["moves"] == moves["z"].shape[0] == c["positions_exported"]
    for gid in np.unique(moves["game"]):
        assert len(np.unique(moves["z"][moves["game"] == gid])) == 1
    eng.arena.close()
    for bad in (0, 7):
        with pytest.raises(ValueError):
            SelfPlayEngine("connect4", network=net, opponent="negamax", opponent_depth=bad, n_games=4, iterations=4)


def test_elo_rates_negamax_rungs(tmp_path):
    from self_play_reinforcement_learning_amd import Elo, ModelContainer, ModelDatabase, Negamax, Random
    from self_play_reinforcement_learning_amd.envs import Connect4Env

    db = ModelDatabase(tmp_path, Connect4Env)
    db.add_model("random", ModelContainer(Random))
    db.add_model("nm2", ModelContainer(Negamax, policy_kwargs=dict(depth=2)))
    db.add_model("nm4", ModelContainer(Negamax, policy_kwargs=dict(depth=4)))
    elo = Elo(db, seed=3)
    new = elo.compare_models("random", "nm2", "nm4", num_games=32)
    assert set(new) == set(db.results()) == {"random__nm2", "random__nm4", "nm4__nm2"}
    assert all(sum(r.values()) == 32 for r in db.results().values())
    ratings = elo.calculate_elo()
    assert ratings["random"] == 0 and set(ratings) == {"random", "nm2", "nm4"}
