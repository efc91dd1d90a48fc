"""CPU: the host side of the stored bounds -- TreeView.node_bounds (score_bounds' recursion returned for every
node) on the oracle's trees, held at every node to the independent walker of tests/bounds_helpers.py (oracle_bounds
started at that node: written from the definitions, on the oracle's own nodes and envs), every root move's interval
held to the exact solver's host twin, and the optional move_lo / move_hi columns of a TreeView."""
from types import SimpleNamespace

import numpy as np
import pytest

from self_play_reinforcement_learning_amd import TreeView
from self_play_reinforcement_learning_amd.solve import solve_host
from tests.bounds_helpers import code_to_value, late_positions, oracle_bounds, searched_tree
from tests.parity_helpers import load_json
from tests.tree_helpers import bfs_arrays, g2_tree, g3_trees, oracle_bfs
from tests.variant_helpers import searches
from tests.variant_helpers import variant_oracle  # noqa: F401  (fixture)

pytestmark = pytest.mark.filterwarnings("ignore::DeprecationWarning")


def oracle_node_bounds(t):
    """The reference, one (move_lo, move_hi) per node in oracle_bfs(min_visits=0) order: (-128, -128) for the root;
    every other listed node is a child of an expanded node X, and its entry is what oracle_bounds gives for that move
    when its walk is started at X (X as the root of its own subtree)."""
    out = [(-128, -128)]
    queue = [t.root]
    e = 0
    while e < len(queue):
        node = queue[e]
        e += 1
        if not node.children:
            continue
        b = oracle_bounds(SimpleNamespace(root=node, game=t.game, A=t.A))
        for a, c in enumerate(node.children):
            out.append((b["move_lo"][a], b["move_hi"][a]))
            queue.append(c)
    return out


def check_tree(t, what):
    """node_bounds of the tree's full listing equals the reference at every node; returns (nodes, root bounds)."""
    view = TreeView.from_arrays(**bfs_arrays(oracle_bfs(t, min_visits=0)))
    got = view.node_bounds(t.game, t.root.state, t.root.player)
    want = oracle_node_bounds(t)
    assert len(got) == len(view.nodes) == len(want), what
    assert got == want, (what, [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w][:4])
    return len(got), oracle_bounds(t)


def _g2_cases(name, sims):
    cs = searches("c4_6x5") if name == "connect4_6_5" else [c for c in load_json("mcts_search.json") if c["game"] == name]
    return [c for c in cs if c["sims"] == sims][:6]


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("name,sims", [("tictactoe", 25), ("tictactoe", 200), ("connect4", 25), ("connect4", 200),
                                       ("connect4_6_5", 25)])
def test_every_node_on_search_cases(request, name, sims, K):
    """G2 search cases of the three boards, 25 and 200 simulations, sequential and four in flight."""
    if name == "connect4_6_5":
        request.getfixturevalue("variant_oracle")
    cases = _g2_cases(name, sims)
    assert len(cases) >= 4
    nodes = [check_tree(g2_tree(c, K)[0], c["id"])[0] for c in cases]
    assert max(nodes) > sims  # whole searches' worth of nodes


def test_every_node_and_soundness_on_late_connect4_positions():
    """36 late Connect4 positions (12, 10 and 8 empty cells, K = 1 and 4): every node's entry is the reference's, and
    every root move's interval contains the exact value of the move (solve.solve_host) -- over a set that holds
    solved trees, trees with a move ruled out and open trees."""
    solved = cut = opened = 0
    for empty, sims, K in ((12, 15, 1), (10, 60, 4), (8, 100, 1)):
        for i, moves in enumerate(late_positions("connect4", 12, empty, seed=empty)):
            t = searched_tree("connect4", moves, sims, salt=2, seed=i, threads=K)
            _, b = check_tree(t, ("late", empty, i))
            codes, _ = solve_host("connect4", t.root.state, t.root.player)
            values = []
            for a in range(t.A):
                if codes[a] == -128:
                    assert b["move_lo"][a] == b["move_hi"][a] == -128
                    continue
                v = code_to_value(codes[a], empty)
                assert b["move_lo"][a] <= v <= b["move_hi"][a], (moves, a, v, b)
                values.append(v)
            assert b["lo"] <= max(values) <= b["hi"]
            solved += b["lo"] == b["hi"]
            cut += any(hi < b["lo"] for hi in b["move_hi"] if hi != -128)
            opened += b["lo"] < 0 < b["hi"]
    assert solved >= 4 and cut >= 4 and opened >= 4, (solved, cut, opened)


@pytest.mark.parametrize("game,plies", [("connect4", 6), ("connect4", 9), ("tictactoe", 4), ("tictactoe", 5)])
def test_every_node_on_game_trees(game, plies):
    """Both trees of self-play games several plies in: roots that moved, subtrees kept from earlier searches."""
    games = [g for g in load_json("selfplay_games.json") if g["game"] == game and g["sims"] == 25
             and not g["evaluate"] and len(g["moves"]) > plies + 1][:3]
    assert len(games) >= 3
    for g in games:
        for t in g3_trees(g, plies):
            check_tree(t, g["id"])


def test_a_view_carries_the_stored_columns():
    t = searched_tree("tictactoe", [4, 0, 8, 2], 60, salt=1, seed=0)
    arrays = bfs_arrays(oracle_bfs(t, min_visits=0))
    plain = TreeView.from_arrays(**arrays)
    assert not plain.has_bounds and plain.root.move_lo is None and "move_lo" not in plain.to_dict()["nodes"][0]
    nb = plain.node_bounds("tictactoe", t.root.state, t.root.player)
    assert plain.score_bounds("tictactoe", t.root.state, t.root.player) == oracle_bounds(t)
    cols = dict(move_lo=np.array([x for x, _ in nb], dtype=np.int8), move_hi=np.array([y for _, y in nb], dtype=np.int8))
    view = TreeView.from_arrays(**arrays, **cols)
    assert view.has_bounds and [(nd.move_lo, nd.move_hi) for nd in view.nodes] == nb
    back = TreeView.from_dict(view.to_dict())
    assert back.has_bounds and [(nd.move_lo, nd.move_hi) for nd in back.nodes] == nb
    assert not TreeView.from_dict(plain.to_dict()).has_bounds
    with pytest.raises(ValueError):
        TreeView.from_arrays(**arrays, move_lo=cols["move_lo"])
    with pytest.raises(ValueError):
        TreeView.from_arrays(**arrays, move_lo=cols["move_lo"][:3], move_hi=cols["move_hi"][:3])
