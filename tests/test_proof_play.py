"""CPU: the keep set of proof-guided play -- tree.proof_move_set, the host twin of k_proof_verdict's rule
(csrc/arena_proof.h) -- on hand-made bounds, and on the oracle's trees at late positions against the exact
solver's host twin (solve.solve_host): where a win is secured or the root is solved, what is kept is exact."""
import numpy as np
import pytest

from self_play_reinforcement_learning_amd import _lib
from self_play_reinforcement_learning_amd.solve import solve_host
from self_play_reinforcement_learning_amd.tree import describe_proof_moves, proof_move_set
from tests.bounds_helpers import code_to_value, late_positions, oracle_bounds, searched_tree

pytestmark = pytest.mark.filterwarnings("ignore::DeprecationWarning")

X = -128  # an illegal move


def kept(lo, hi, move_lo, move_hi):
    mask = proof_move_set(lo, hi, move_lo, move_hi)
    return [a for a in range(len(move_lo)) if (mask >> a) & 1]


def test_entry_points_and_exports():
    import self_play_reinforcement_learning_amd as pkg

    L = _lib.lib()
    names = ("spmcts_set_proof_play", "spmcts_tree_proof_moves_batch", "spmcts_proof_last", "spmcts_get_proof_stats",
             "spmcts_proof_stop")
    assert all(n in _lib.HEADER_SYMBOLS for n in names)
    assert L.spmcts_set_proof_play(None, None) == -1
    assert L.spmcts_tree_proof_moves_batch(None, None, 0, None, None, None, None) == -1
    assert L.spmcts_proof_last(None, None, None, None, None) == -1
    assert L.spmcts_get_proof_stats(None, None) == -1
    assert L.spmcts_proof_stop(None, None) == -1
    assert pkg.proof_move_set is proof_move_set
    for name in ("set_proof_play", "proof_moves_batch", "proof_last", "proof_stats", "proof_stop"):
        assert hasattr(pkg.Arena, name), name
    assert hasattr(pkg.MCTreeSearch, "proof_moves")


def test_a_secured_but_unsolved_win_keeps_only_the_moves_that_reach_it():
    # lo = 5 from move 2; move 4 might win faster (hi 9) but is not proved to reach 5; move 0 is a proved draw
    assert kept(5, 9, [0, -7, 5, X, -8, 5, -3], [0, 8, 7, X, 9, 5, -3]) == [2, 5]


def test_a_solved_win_keeps_the_fastest_wins():
    assert kept(6, 6, [6, 4, -3, 6], [6, 4, -3, 6]) == [0, 3]


def test_a_solved_loss_keeps_only_the_slowest_losses():
    # every move loses; -2 is the longest resistance (the value of a loss is minus the cells left when it falls)
    assert kept(-2, -2, [-4, -2, X, -6, -2], [-4, -2, X, -6, -2]) == [1, 4]


def test_a_secured_draw_with_open_alternatives_keeps_them_and_drops_proved_losses():
    # move 1 secures the draw, moves 0 and 5 may still win, moves 2 and 3 are proved losses, move 4 at most a draw
    assert kept(0, 6, [-7, 0, -5, -3, -7, -7], [6, 0, -5, -1, 0, 4]) == [0, 1, 4, 5]


def test_a_solved_draw_keeps_the_drawing_moves():
    assert kept(0, 0, [0, -3, X, 0], [0, -3, X, 0]) == [0, 3]


def test_all_moves_open_keeps_every_legal_move():
    assert kept(-7, 6, [-7] * 4 + [X] + [-7] * 2, [6] * 4 + [X] + [6] * 2) == [0, 1, 2, 3, 5, 6]
    # an open root below zero whose moves are partly bounded: nothing is proved worse than lo
    assert kept(-5, 6, [-7, -5, X], [6, -1, X]) == [0, 1]


def test_an_illegal_move_is_never_kept_and_the_set_is_never_empty():
    """Every consistent small case: lo / hi are the maxima of the moves' bounds (as k_tree_bounds defines them)."""
    rng = np.random.default_rng(0)
    for _ in range(2000):
        A = int(rng.integers(1, 8))
        mlo = rng.integers(-6, 7, A)
        mhi = mlo + rng.integers(0, 5, A) * (rng.random(A) < 0.6)
        illegal = rng.random(A) < 0.3
        illegal[int(rng.integers(A))] = False
        mlo[illegal] = mhi[illegal] = X
        lo, hi = int(mlo.max()), int(mhi.max())
        mask = proof_move_set(lo, hi, mlo, mhi)
        assert mask != 0 and mask < (1 << A)
        for a in range(A):
            if illegal[a]:
                assert not (mask >> a) & 1
        secure = int(np.argmax(mlo == lo))
        assert (mask >> secure) & 1  # the move that secures lo


def test_batched_arguments_and_the_text():
    lo, hi = np.array([5, -2, 0], dtype=np.int8), np.array([9, -2, 6], dtype=np.int8)
    mlo = np.array([[0, 5, X, 5], [-4, -2, X, -2], [-7, 0, -5, -7]], dtype=np.int8)
    mhi = np.array([[0, 7, X, 5], [-4, -2, X, -2], [6, 0, -5, -1]], dtype=np.int8)
    got = proof_move_set(lo, hi, mlo, mhi)
    assert got.shape == (3,) and got.tolist() == [0b1010, 0b1010, 0b0011]
    assert [proof_move_set(int(lo[i]), int(hi[i]), mlo[i], mhi[i]) for i in range(3)] == got.tolist()
    assert isinstance(proof_move_set(5, 9, [0, 5], [0, 7]), int)
    assert describe_proof_moves(0b1010) == "keeps 1 3"


# (game, empty cells, simulations, positions): late positions of random playouts (tests/bounds_helpers.py), seeds
# chosen on the CPU so that the floors below hold
LATE = [("tictactoe", 6, 50, 12), ("tictactoe", 4, 200, 12), ("connect4", 8, 100, 24), ("connect4", 6, 200, 24)]


def test_kept_moves_are_exact_against_the_solver():
    """On the oracle's trees: where lo > 0 every kept move's exact score is >= lo; where lo == hi every kept move's
    exact score is the root's; a kept set always holds the move that secures lo.  The set holds at least 8 roots
    with a secured or solved win, 4 solved losses and 4 unsolved roots that lose a legal move."""
    wins = losses = cut = 0
    for game, empty, sims, count in LATE:
        for i, moves in enumerate(late_positions(game, count, empty, seed=empty)):
            t = searched_tree(game, moves, sims, salt=i + 1, seed=i)
            w = oracle_bounds(t)
            lo, hi, e = w["lo"], w["hi"], w["empty"]
            mask = proof_move_set(lo, hi, w["move_lo"], w["move_hi"])
            legal = [a for a in range(t.A) if w["move_lo"][a] != X]
            keep = [a for a in range(t.A) if (mask >> a) & 1]
            assert keep and set(keep) <= set(legal) and w["best"] in keep, (game, moves)
            codes, _ = solve_host(game, t.root.state, t.root.player)
            value = {a: code_to_value(codes[a], e) for a in legal}
            root = max(value.values())
            if lo > 0:
                assert all(value[a] >= lo for a in keep), (game, moves, keep, value, w)
            if lo == hi:
                assert lo == root and all(value[a] == root for a in keep), (game, moves, keep, value, w)
            wins += lo > 0
            losses += lo == hi and lo < 0
            cut += lo != hi and len(keep) < len(legal)
    assert wins >= 8 and losses >= 4 and cut >= 4, (wins, losses, cut)
