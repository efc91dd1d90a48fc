"""CPU: the host side of reading the search trees -- the two entry points' argument checks, tree.TreeView on
hand-written arrays, and the oracle-side walkers of tests/tree_helpers.py on the G2 fixture (with the coverage the
GPU tests of tests/test_gpu_tree_export.py rely on, so that they cannot pass vacuously)."""
import json

import numpy as np
import pytest

from self_play_reinforcement_learning_amd import TreeView, _lib
from tests.parity_helpers import load_json
from tests.tree_helpers import (END_CUT, END_GAME, END_NO_CHILD, EXPANDED, TERMINAL, VALID, bfs_arrays, g2_tree,
                                oracle_bfs, oracle_pv)


def test_entry_points_refuse_a_null_handle():
    L = _lib.lib()
    assert L.spmcts_tree_pv_batch(None, None, 0, 1, 1, None, None, None, None, None, None, None, None, None) == -1
    assert L.spmcts_tree_export_batch(None, None, 0, 1, 1, -1, None, None, None, None, None, None, None, None, None,
                                      None, None, 0, None) == -1
    assert L.spmcts_tree_export_work_bytes(None, 1, 1, None) == -1
    for name in ("spmcts_tree_pv_batch", "spmcts_tree_export_batch", "spmcts_tree_export_work_bytes"):
        assert name in _lib.HEADER_SYMBOLS


# A hand-written tree (export order).  Root (player 1) with children a=1 (n 5), a=3 (n 5: a tie, a=1 first),
# a=4 (n 1); under a=1: a=0 (n 2, vl 1) and a=6 (n 2: tie again); under a=3: a=2 (n 4, terminal); under 1-0: a=5.
ARRAYS = dict(
    parent=[-1, 0, 0, 0, 1, 1, 2, 4],
    action=[-1, 1, 3, 4, 0, 6, 2, 5],
    depth=[0, 1, 1, 1, 2, 2, 2, 3],
    node_n=[12, 5, 5, 1, 2, 2, 4, 1],
    node_vl=[0, 0, 0, 0, 1, 0, 0, 0],
    node_w=[1.5, -2.0, 2.5, 0.25, 1.0, -0.5, 4.0, 0.125],
    node_p=[0.0, 0.3, 0.4, 0.1, 0.5, 0.25, 0.9, 0.2],
    player=[1, -1, -1, -1, 1, 1, 1, -1],
    flags=[EXPANDED | VALID, EXPANDED | VALID, EXPANDED | VALID, VALID, EXPANDED | VALID, VALID,
           VALID | TERMINAL, VALID],
)


def test_tree_view_wiring_and_fields():
    v = TreeView.from_arrays(**ARRAYS)
    assert len(v) == 8 and v.count == 8 and not v.truncated
    r = v.root
    assert r.parent is None and r.action == -1 and r.depth == 0 and r.moves == []
    assert [c.action for c in r.children] == [1, 3, 4]
    a1, a3, a4 = r.children
    assert a1.parent is r and [c.action for c in a1.children] == [0, 6] and a4.children == ()
    leaf = a1.children[0].children[0]
    assert leaf.moves == [1, 0, 5] and leaf.depth == 3 and leaf.player == -1 and leaf.parent.parent is a1
    assert a3.children[0].terminal and not a3.terminal and a3.expanded and not a4.expanded and a4.valid
    assert (a1.n, a1.vl, a1.w, a1.p) == (5, 0, -2.0, 0.3)
    # q = (w - vl) / (n + vl), mcts.py:59-62
    assert a1.q == -2.0 / 5 and a1.children[0].q == (1.0 - 1) / (2 + 1) and r.q == 1.5 / 12
    zero = TreeView.from_arrays(**{k: [x[0]] if k != "node_n" else [0] for k, x in ARRAYS.items()})
    assert zero.root.q == 0 and zero.root.children == ()


def test_tree_view_principal_variation_takes_the_lowest_action_on_ties():
    v = TreeView.from_arrays(**ARRAYS)
    assert v.principal_variation() == [(1, 5, -0.4), (0, 2, 0.0), (5, 1, 0.125)]
    assert v.principal_variation(min_visits=2) == [(1, 5, -0.4), (0, 2, 0.0)]
    assert v.principal_variation(min_visits=6) == []


def test_tree_view_render_filters():
    v = TreeView.from_arrays(**ARRAYS)
    full = v.render().splitlines()
    assert len(full) == 8 and full[0].startswith("root n=12")
    assert full[1].startswith("├── a=1 n=5 q=-0.400 p=0.300") and full[2].startswith("│   ├── a=0 n=2")
    assert full[3].startswith("│   │   └── a=5 n=1") and full[-1].startswith("└── a=4 n=1")
    assert [ln.endswith("#") for ln in full] == [False] * 6 + [True, False]  # a=3 / a=2 ended the game
    d1 = v.render(max_depth=1).splitlines()
    assert len(d1) == 4 and all("a=" in ln for ln in d1[1:])
    n2 = v.render(min_visits=2).splitlines()
    assert len(n2) == 6 and not any("n=1 " in ln for ln in n2)
    assert v.render(max_depth=0) == full[0]


def test_tree_view_to_dict_round_trips_through_json():
    v = TreeView.from_arrays(count=11, max_nodes=8, **ARRAYS)
    assert v.truncated and v.count == 11
    d = json.loads(json.dumps(v.to_dict()))
    assert d["truncated"] is True and d["count"] == 11 and len(d["nodes"]) == 8
    w = TreeView.from_dict(d)
    assert w.to_dict() == v.to_dict() and w.render() == v.render() and w.truncated
    assert not TreeView.from_arrays(count=8, max_nodes=8, **ARRAYS).truncated
    # a count below the room: only `count` entries are nodes, the rest is padding
    assert len(TreeView.from_arrays(count=4, **ARRAYS)) == 4


def test_tree_view_refuses_children_before_parents():
    bad = dict(ARRAYS, parent=[-1, 2, 0, 0, 1, 1, 2, 4])
    with pytest.raises(ValueError):
        TreeView.from_arrays(**bad)


# ----------------------------------------------------------------------------- the oracle walkers
def tree_cases():
    """The G2 cases the GPU tests run at 25 simulations: the fixture's first 40 Connect4 cases."""
    return [c for c in load_json("mcts_search.json") if c["game"] == "connect4" and c["sims"] == 25][:40]


@pytest.mark.parametrize("K", [1, 4])
def test_oracle_walkers_cover_the_interesting_trees(K):
    cases = tree_cases()
    assert len(cases) == 40
    lens, ties, ends, revisited_terminal = [], 0, 0, 0
    for c in cases:
        t, _ = g2_tree(c, K)
        pv = oracle_pv(t, 42)
        rows = oracle_bfs(t)
        # the walkers agree with each other and with the fixture's root
        ns = [ch.n for ch in t.root.children]
        if K == 1:
            assert ns == c["child_n"] and pv["moves"][0] == int(np.argmax(c["child_n"]))
        arr = bfs_arrays(rows)
        view = TreeView.from_arrays(**arr)
        assert [m for m, _, _ in view.principal_variation()] == pv["moves"]
        assert [n for _, n, _ in view.principal_variation()] == pv["n"]
        assert arr["parent"][0] == -1 and (arr["parent"][1:] < np.arange(1, len(rows))).all()
        assert (np.diff(arr["depth"]) >= 0).all() and (arr["node_n"][1:] >= 1).all()
        assert (arr["player"] == t.root.player * (-1) ** arr["depth"].astype(int)).all()
        d1 = [r for r in rows if r["depth"] == 1]
        assert [r["action"] for r in d1] == [a for a, n in enumerate(ns) if n >= 1]
        assert rows == oracle_bfs(t, min_visits=1, max_depth=None)
        assert oracle_bfs(t, max_depth=1) == rows[:1 + len(d1)]
        every = oracle_bfs(t, min_visits=0)
        assert len(every) == 1 + t.A * sum(1 for r in every if r["flags"] & EXPANDED)
        assert pv["end"] in (END_NO_CHILD, END_GAME)
        assert oracle_pv(t, 1)["end"] == (END_GAME if len(pv["moves"]) == 1 and pv["end"] == END_GAME else END_CUT)
        lens.append(len(pv["moves"]))
        ties += pv["ties"] > 0
        ends += pv["end"] == END_GAME
        revisited_terminal += any(r["flags"] & TERMINAL and r["n"] > 1 for r in rows)
        assert 11 <= len(rows) <= 27
    assert min(lens) >= 1 and max(lens) >= 3
    assert ties >= 1 and ends >= 1 and revisited_terminal >= 1
