"""CPU: game records (records.py) -- log_positions' host twin against a replay through the Python envs, the
GameRecords container, and grade_games(device="cpu") against known games and position-by-position solves."""
import numpy as np
import pytest
import torch

from self_play_reinforcement_learning_amd.mcts import TACTICAL_CLASSES
from self_play_reinforcement_learning_amd.records import GameRecords, from_moves, grade_games, log_positions
from self_play_reinforcement_learning_amd.solve import perfect_report, solve_host
from tests.record_helpers import (ALL_GAMES, BOARD_OF, FULL_GAME, TTT_DRAW, expected_positions, games_of_every_length,
                                  pack, random_game, replay)


def _same(got, exp, n):
    for k in ("boards", "players", "row_record", "row_ply", "offsets"):
        assert np.array_equal(got[k].numpy(), exp[k]), k
        assert got[k].numpy().dtype == exp[k].dtype, k
    assert got["status"].numpy().tolist() == [0] * n


# ----------------------------------------------------------------------------- 1. log_positions_host
@pytest.mark.parametrize("game", ALL_GAMES)
def test_log_positions_host_matches_replay(game):
    W, H = BOARD_OF[game]
    cells = W * H
    lists = games_of_every_length(game, np.random.default_rng(11))
    lens = {len(m) for m in lists}
    assert lens == set(range(1, cells + 1))  # every length from 1 to CELLS
    assert len(lists) > cells + cells // 2  # random games beside the full-board draw's prefixes
    b, rew, done = replay(game, FULL_GAME[game])
    assert len(FULL_GAME[game]) == cells and done and rew == 0  # a full-board draw
    assert not replay(game, FULL_GAME[game][:-1])[2]  # which does not end before its last move
    moves, plies = pack(game, lists)
    for first_ply in (0, 5, max(lens), cells + 3):
        got = log_positions(game, moves, plies, first_ply=first_ply, device="cpu")
        exp = expected_positions(game, lists, first_ply)
        _same(got, exp, len(lists))
        if first_ply >= max(lens):
            assert got["boards"].shape[0] == 0 and not got["offsets"].any()
    # rows in (record, ply) order, both maps
    got = log_positions(game, moves, plies, device="cpu")
    key = got["row_record"].long() * 1000 + got["row_ply"].long()
    assert bool((key[1:] > key[:-1]).all())
    assert got["players"].tolist() == [1 if p % 2 == 0 else -1 for p in got["row_ply"].tolist()]


def test_log_positions_host_empty_batch():
    got = log_positions("connect4", np.zeros((0, 42), dtype=np.uint8), np.zeros(0, dtype=np.int32), device="cpu")
    assert got["boards"].shape == (0, 7, 6) and got["status"].shape == (0,) and got["offsets"].tolist() == [0]


BAD = [  # (game, moves, plies or None = len(moves), status)
    ("connect4", [0] * 7, None, 1),                      # a full column
    ("connect4", [7], None, 1),                          # outside the action range
    ("tictactoe", [4, 4], None, 1),                      # an occupied cell
    ("connect4", [0, 1, 0, 1, 0, 1, 0, 2], None, 2),     # a move after the winning move
    ("tictactoe", [0, 3, 1, 4, 2, 5], None, 2),
    ("connect4", [3], 43, 3),                            # plies > CELLS
    ("tictactoe", [4], -1, 3),
]


@pytest.mark.parametrize("game,bad,plies,status", BAD)
def test_log_positions_host_status_of_a_bad_record(game, bad, plies, status):
    good = [random_game(game, np.random.default_rng(s)) for s in (1, 2)]
    lists = [good[0], bad, good[1]]
    moves, pl = pack(game, lists)
    if plies is not None:
        pl[1] = plies
    got = log_positions(game, moves, pl, first_ply=1, device="cpu")
    assert got["status"].tolist() == [0, status, 0]
    exp = expected_positions(game, lists, 1, bad={1})  # the bad record contributes no rows
    for k in ("boards", "players", "row_record", "row_ply", "offsets"):
        assert np.array_equal(got[k].numpy(), exp[k]), k
    assert 1 not in got["row_record"].tolist()


# ----------------------------------------------------------------------------- 2. GameRecords
RENDER = """game 0: X side 0, O side 1, 3 plies, draw
ply 0: X (side 0) plays 3
.......
.......
.......
.......
.......
...X...
ply 1: O (side 1) plays 3
.......
.......
.......
.......
...O...
...X...
ply 2: X (side 0) plays 0
.......
.......
.......
.......
...O...
X..X..."""


def test_game_records_container(tmp_path):
    lists = [[3, 3, 0], [0, 1, 0, 1, 0, 1, 0], [0, 1, 0, 1, 2, 1, 3, 1]]
    r = from_moves("connect4", lists)
    assert len(r) == 3 and r.ids.tolist() == [0, 1, 2] and r.swap.tolist() == [0, 0, 0]
    assert r.result.tolist() == [0, 1, -1]  # unfinished, the first mover's win, the second mover's win
    assert [r.moves_of(i) for i in range(3)] == lists
    assert not r.moves[0, 3:].any()
    assert r.as_openings(2) == [[3, 3], [0, 1], [0, 1]]
    assert r.render(0) == RENDER
    path = tmp_path / "games.json"
    r.names[1] = ["a", "b"]
    r.save(path)
    q = GameRecords.load(path)
    for k in GameRecords._ARRAYS:
        assert np.array_equal(getattr(q, k), getattr(r, k)) and getattr(q, k).dtype == getattr(r, k).dtype, k
    assert q.names == r.names and q.game == r.game
    assert "a wins" in q.render(1) and "O (b) plays 1" in q.render(1)
    q.extend(r)
    assert len(q) == 6 and q.moves_of(5) == lists[2] and q.names[4] == ["a", "b"]
    with pytest.raises(ValueError, match="game 1 is not a legal game: illegal move"):
        from_moves("connect4", [[0], [0] * 7])
    with pytest.raises(ValueError):
        q.extend(from_moves("tictactoe", [[4]]))


# ----------------------------------------------------------------------------- 3. grade_games on the host
def test_grade_a_perfect_tictactoe_draw():
    g = grade_games("tictactoe", from_moves("tictactoe", [TTT_DRAW]), max_empty=9, device="cpu")
    assert g["n_rows"] == 9 and g["n_graded"] == 9 and g["n_unsolved"] == 0 and g["n_horizon"] == 0
    assert g["per_side"]["graded"].tolist() == [[5, 4]]
    assert g["per_side"]["strong"].tolist() == [[5, 4]] and g["per_side"]["weak"].tolist() == [[5, 4]]
    assert g["per_side"]["blunders"].tolist() == [[0, 0]] and g["per_side"]["first_blunder"].tolist() == [[-1, -1]]
    assert g["value"].tolist() == [0] * 9 and g["chosen"].tolist() == [0] * 9
    assert g["side"].tolist() == [0, 1] * 4 + [0]


def test_grade_finds_the_blunder_and_the_forced_losses():
    """X takes a corner, O answers on the adjacent edge (the one losing reply of four kinds), X wins by force."""
    r = from_moves("tictactoe", [[0, 1, 4, 2, 8]])
    r.swap[0] = 1  # tree 2g + 1 moved first: O is side 0
    g = grade_games("tictactoe", r, max_empty=9, device="cpu")
    assert g["n_unsolved"] == 0 and g["n_graded"] == 5
    assert g["blunder"].tolist() == [False, True, False, False, False]
    assert g["side"].tolist() == [1, 0, 1, 0, 1]
    assert g["per_side"]["blunders"].tolist() == [[1, 0]] and g["per_side"]["first_blunder"].tolist() == [[1, -1]]
    cls = [TACTICAL_CLASSES[c] for c in g["class"].tolist()]
    assert cls[1] == "blunder" and cls[3] == "forced_loss"  # every later move of the loser is forced
    assert g["weak"].tolist() == [True, False, True, True, True]
    assert g["strong"].tolist()[2] and g["strong"].tolist()[4]  # X takes the fastest win each time
    assert g["value"].tolist()[1] == 0 and g["chosen"].tolist()[1] < 0


def test_grade_equals_position_by_position_solves_6x5():
    game = "connect4_6_5"
    rng = np.random.default_rng(5)
    lists = [random_game(game, rng) for _ in range(6)]
    lists = [m for m in lists if len(m) >= 22][:3] or lists[:2]
    r = from_moves(game, lists)
    g = grade_games(game, r, max_empty=10, device="cpu")
    assert g["n_unsolved"] == 0  # the default budget of 2^22 moves solves every position of 10 empty cells
    pos = log_positions(game, r.moves, r.plies, device="cpu")
    n_tier = 0
    for i in range(g["n_rows"]):
        b = pos["boards"][i].numpy()
        rec, ply = int(pos["row_record"][i]), int(pos["row_ply"][i])
        if (b == 0).sum() > 10:
            assert not bool(g["exact"][i]) and int(g["class"][i]) == -1
            continue
        n_tier += 1
        codes, nodes = solve_host(game, b, int(pos["players"][i]))
        assert nodes < 1 << 22
        rep = perfect_report(torch.as_tensor(codes)[None], [lists[rec][ply]])
        assert bool(g["exact"][i])
        assert (bool(g["strong"][i]), bool(g["weak"][i])) == (bool(rep["strong"][0]), bool(rep["weak"][0])), i
        assert int(g["chosen"][i]) == int(codes[lists[rec][ply]])
    assert n_tier == g["n_graded"] > 0
    assert g["n_strong"] == int(g["per_side"]["strong"].sum()) <= g["n_weak"] <= g["n_graded"]
    assert g["n_blunders"] == g["n_graded"] - g["n_weak"]
    # the horizon tier takes the other rows and counts none of them as exact
    h = grade_games(game, r, max_empty=10, depth=2, device="cpu")
    assert h["n_horizon"] == h["n_rows"] - n_tier and h["n_graded"] == n_tier
    assert not bool((h["horizon"] & h["exact"]).any()) and bool((h["class"][h["horizon"]] >= 0).all())
    assert not bool(h["strong"][h["horizon"]].any()) and not bool(h["weak"][h["horizon"]].any())


def test_grade_leaves_unsolved_rows_out():
    """A budget of one move cannot solve the empty TicTacToe board: the row is counted as unsolved, in no ratio."""
    r = from_moves("tictactoe", [TTT_DRAW])
    g = grade_games("tictactoe", r, max_empty=9, max_nodes=1, device="cpu")
    assert g["n_unsolved"] > 0 and g["n_graded"] + g["n_unsolved"] == 9
    assert not bool(g["exact"][0]) and int(g["class"][0]) == -1
    assert not bool(g["strong"][0]) and not bool(g["weak"][0]) and not bool(g["blunder"][0])
    assert int(g["per_side"]["graded"].sum()) == g["n_graded"] and g["n_strong"] <= g["n_graded"]


def test_names_are_exported():
    import self_play_reinforcement_learning_amd as pkg

    assert pkg.GameRecords is GameRecords and pkg.grade_games is grade_games
