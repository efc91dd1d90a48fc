"""CPU: the exact depth-limited negamax's host twin (spmcts_negamax_host, the kernel's search core compiled for the
host) against the known answers and an independent brute force; tactical_report; the host Negamax player; the ABI.
"""
import ctypes
import random

import numpy as np
import pytest

from self_play_reinforcement_learning_amd import _lib
from self_play_reinforcement_learning_amd.arena import GAMES
from tests import negamax_helpers as nh

X = nh.X


@pytest.mark.parametrize("game,moves,depths,codes", nh.KNOWN, ids=[f"{k[0]}-{k[1]}" for k in nh.KNOWN])
def test_known_answers(game, moves, depths, codes):
    board, player = nh.after(game, moves)
    for D in depths:
        got, nodes = nh.host_codes(game, board, player, D)
        assert got.tolist() == codes, (game, moves, D)
        if not moves and (game, D) in nh.FULL_WIDTH:  # the search is full width: the plain recursion's count
            assert nodes == nh.FULL_WIDTH[(game, D)]


@pytest.mark.parametrize("game", nh.BOARDS)
def test_host_twin_matches_brute_force(game):
    """Depths 1 to 4 on every position of the generator, 5 on the first four; illegal codes and full-board draws
    inside the horizon must occur (the carved boards give them)."""
    brute = nh.brute(game)
    pos = nh.positions(game)
    assert len(pos) >= 30
    illegal = draws = decided = 0
    for i, (board, player) in enumerate(pos):
        for D in (1, 2, 3, 4) + ((5,) if i < 4 else ()):
            got, nodes = nh.host_codes(game, board, player, D)
            exp = brute(board, player, D)
            assert got.tolist() == exp.tolist(), (game, i, D, board.tolist(), player)
            assert nodes >= int((got != X).sum())
            illegal += int((got == X).any())
            decided += int(((got != X) & (got != 0)).any())
        empties = int((board == 0).sum())
        if empties <= 2:  # the board fills inside a horizon of 4: the search must stop there, with code 0 unless won
            draws += 1
    assert illegal and draws >= 3 and decided


def test_tictactoe_full_solve_after_two_plies():
    brute = nh.brute("tictactoe")
    n = 0
    for a in range(9):
        for b in range(9):
            if a == b:
                continue
            board, player = nh.after("tictactoe", [a, b])
            got, _ = nh.host_codes("tictactoe", board, player, 9)
            assert got.tolist() == brute(board, player, 9).tolist(), (a, b)
            n += 1
    assert n == 72


def test_a_board_holding_a_line_is_searched_on():
    """The documented behaviour on a finished position: step's rule, a move whose row, column or diagonal holds
    a run wins for whoever makes it."""
    board = np.zeros((7, 6), dtype=np.int8)
    board[0:4, 0] = 1  # +1 already has the bottom row
    board[0:3, 1] = -1
    for player in (1, -1):
        got, _ = nh.host_codes("connect4", board, player, 2)
        assert got.tolist() == nh.brute("connect4")(board, player, 2).tolist()


def test_tactical_report_classes():
    import torch

    from self_play_reinforcement_learning_amd import tactical_report

    score = torch.tensor([[3, 0, -2, X, 0, 0, 0],      # a win exists, the move chosen draws: missed_win
                          [1, 3, 0, 0, 0, 0, 0],       # wins, but in 3 where 1 was there: slower_win
                          [0, -2, 0, 0, 0, 0, X],      # walks into a forced loss: blunder
                          [-2, -4, -2, X, X, X, X],    # every move loses: forced_loss
                          [0, 0, 0, 0, 0, 0, 0],       # nothing decided: ok
                          [1, 3, 0, 0, 0, 0, 0],       # the fastest win: ok
                          [5, 0, -2, 0, 0, 0, 0]],     # a win exists, the move chosen loses: missed_win first
                         dtype=torch.int8)
    action = torch.tensor([1, 1, 1, 1, 3, 0, 2])
    rep = tactical_report(score, action)
    assert rep["label"] == ["missed_win", "slower_win", "blunder", "forced_loss", "ok", "ok", "missed_win"]
    assert rep["counts"] == dict(missed_win=2, slower_win=1, blunder=1, forced_loss=1, ok=2)
    assert rep["chosen"].tolist() == [0, 3, -2, -4, 0, 1, -2]
    with pytest.raises(ValueError):
        tactical_report(score, torch.tensor([3, 0, 0, 0, 0, 0, 0]))  # an illegal move chosen


@pytest.mark.parametrize("game", ["connect4", "tictactoe"])
def test_host_player(game):
    from self_play_reinforcement_learning_amd.envs import Connect4Env, TicTacToeEnv
    from self_play_reinforcement_learning_amd.hardcoded_players import Negamax, negamax_rank

    Env = Connect4Env if game == "connect4" else TicTacToeEnv
    depth = 4 if game == "connect4" else 5
    rng = np.random.default_rng(11)
    for case in range(40):
        me = 1 if case % 2 else -1
        p = Negamax(env=Env, depth=depth, player=me)
        p.reset(me)
        ref = nh.make_env(game)
        ref.reset()
        player, done = 1, False
        for _ in range(2 * int(rng.integers(0, 5 if game == "connect4" else 3)) + (0 if me == 1 else 1)):
            a = int(rng.choice(np.flatnonzero(ref.valid_moves())))
            _, _, done, _ = ref.step(a, player)
            if done:
                break
            p.play_action(a, player)
            player = -player
        if done:
            continue
        assert p.mover() == player == me
        codes, _ = nh.host_codes(game, ref.board, me, depth)
        value = max(nh.rank(c) for c in codes if c != X)
        random.seed(case)
        a = p(None)
        assert codes[a] != X and nh.rank(codes[a]) == value
        assert int(negamax_rank(codes).max()) == value
        random.seed(case)
        assert p(None) == a


def test_host_player_depth_errors():
    from self_play_reinforcement_learning_amd.envs import Connect4Env, TicTacToeEnv
    from self_play_reinforcement_learning_amd.hardcoded_players import Negamax

    assert Negamax(env=Connect4Env).depth == 2
    Negamax(env=Connect4Env, depth=8)
    Negamax(env=TicTacToeEnv, depth=9)
    for Env, depth in ((Connect4Env, 0), (Connect4Env, 9), (TicTacToeEnv, 10), (Connect4Env, -1), (Connect4Env, "deep"),
                       (Connect4Env, 2.5), (Connect4Env, None)):
        with pytest.raises(ValueError):
            Negamax(env=Env, depth=depth)


def test_model_database_round_trips_depth(tmp_path):
    from self_play_reinforcement_learning_amd import ModelContainer, ModelDatabase, Negamax
    from self_play_reinforcement_learning_amd.elo import POLICIES, Elo
    from self_play_reinforcement_learning_amd.envs import Connect4Env
    from self_play_reinforcement_learning_amd.hardcoded_players import Random

    assert "Negamax" in POLICIES
    db = ModelDatabase(str(tmp_path / "db"), Connect4Env)
    db.add_model("random", ModelContainer(Random))
    db.add_model("nm4", ModelContainer(Negamax, policy_kwargs=dict(depth=4)))
    db.add_model("nm", ModelContainer(Negamax))
    db2 = ModelDatabase(str(tmp_path / "db"), Connect4Env)
    assert db2.models()["nm4"] == {"policy": "Negamax", "net": None, "policy_kwargs": {"depth": 4}}
    c = db2.get_model("nm4")
    assert c.policy_gen is Negamax and c.policy_kwargs["depth"] == 4
    assert c.policy_gen(**c.policy_kwargs).depth == 4
    assert Elo(db2).players(["random", "nm4", "nm"]) == [dict(kind="random"), dict(kind="negamax", depth=4),
                                                        dict(kind="negamax", depth=2)]


def test_scheduler_accepts_negamax_as_evaluation_policy():
    """SelfPlayScheduler._opponent maps a Negamax container to the device player and its depth."""
    from self_play_reinforcement_learning_amd import ModelContainer, Negamax
    from self_play_reinforcement_learning_amd.self_play_parallel import SelfPlayScheduler

    sp = SelfPlayScheduler.__new__(SelfPlayScheduler)
    sp.evaluation_policy_container = ModelContainer(Negamax, policy_kwargs=dict(depth=3))
    assert sp._opponent() == ("negamax", {"opponent_depth": 3})
    sp.evaluation_policy_container = ModelContainer(Negamax)
    assert sp._opponent() == ("negamax", {"opponent_depth": 2})


def test_abi_depth_limits():
    L = _lib.lib()
    for game, (gid, W, H, A) in GAMES.items():
        cap = L.spmcts_negamax_max_depth(gid, W, H)
        assert cap >= (9 if game == "tictactoe" else 8)
        board = np.zeros((W, H), dtype=np.int8)
        codes = np.zeros(A, dtype=np.int8)
        nodes = ctypes.c_uint64()
        args = (board.ctypes.data_as(ctypes.c_void_p), 1)
        out = (codes.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nodes))
        assert L.spmcts_negamax_host(gid, W, H, *args, 1, *out) == 0
        for bad in (0, cap + 1, -3):
            assert L.spmcts_negamax_host(gid, W, H, *args, bad, *out) == -3
            assert b"depth" in L.spmcts_last_error()
            assert L.spmcts_negamax_batch(gid, W, H, None, None, 0, bad, None, None, None) == -3
        assert L.spmcts_negamax_batch(gid, W, H, None, None, 0, 1, None, None, None) == 0  # n = 0: a no-op, no GPU
        # launches: positions * sum_{k <= D} A^k stays below one constant at every depth
        bounds = []
        for D in range(1, cap + 1):
            per = L.spmcts_negamax_launch_positions(gid, W, H, D)
            assert per >= 1
            bounds.append(per * sum(A ** k for k in range(1, D + 1)))
        assert max(bounds) <= 8.0e9
    assert L.spmcts_negamax_max_depth(0, 5, 5) == -2
    assert _lib.PLAYER_NEGAMAX == 3
