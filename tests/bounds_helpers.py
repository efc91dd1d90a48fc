"""Oracle-side helpers of the score-bound tests: an independent recursive walker over an OracleTree, written from
the definitions of the bounds and not from the code it checks (csrc/arena_tree.h k_tree_bounds, tree.py
TreeView.score_bounds), plus late positions and the solver's codes as values.

Definitions.  e(X): the empty cells of node X's position.  s(X): the exact solver's score, the maximum over the
legal moves of e(X) if the move wins, 0 if it fills the board, -s(child) otherwise.  The bounds of a legal move at
X: [e(X), e(X)] for a win and [0, 0] for a full board, whether or not the child was ever visited; [-hi(child),
-lo(child)] for a child with children; [-(e(X) - 1), e(X) - 2] for any other.  lo(X) / hi(X): the maxima over the
legal moves.  The board is carried along with the oracle's own envs: "the move ended the game" is the env's `done`,
win or draw its reward.
"""
import numpy as np

import oracle.mcts as om
from oracle.mcts import NumpyRNG, OracleTree
from oracle.table_net import TableNet

ILLEGAL = -128
KEYS = ("lo", "hi", "move_lo", "move_hi", "best", "empty", "nodes")


def _env_at(game, state):
    env = om.make_env(game)  # (the module's name: the variant boards patch it, tests/variant_helpers.py)
    env.set_state(np.array(state, copy=True))
    return env


def oracle_bounds(t):
    """dict(lo, hi, move_lo [A], move_hi [A], best, empty, nodes) of an OracleTree's active root."""
    entered = 0

    def walk(node, state, player):
        nonlocal entered
        entered += bool(node.children)
        e = int(np.sum(state == 0))
        legal = _env_at(t.game, state).valid_moves()
        lo, hi = [ILLEGAL] * t.A, [ILLEGAL] * t.A
        for a in range(t.A):
            if not legal[a]:
                continue
            s, reward, done, _ = _env_at(t.game, state).step(a, player=player)
            if done:
                lo[a] = hi[a] = e if reward else 0
            elif node.children and node.children[a].children:
                _, _, clo, chi = walk(node.children[a], s, -player)
                lo[a], hi[a] = -max(chi), -max(clo)
            else:
                lo[a], hi[a] = -(e - 1), e - 2
        return e, player, lo, hi

    e, _, mlo, mhi = walk(t.root, t.root.state, t.root.player)
    lo, hi = max(mlo), max(mhi)
    return dict(lo=lo, hi=hi, move_lo=mlo, move_hi=mhi, best=mlo.index(lo), empty=e, nodes=entered)


def late_positions(game, count, empty, seed):
    """`count` distinct move lists from the empty board, player 1 first, each a random legal playout that leaves
    exactly `empty` empty cells with the game still on (playouts that end sooner are drawn again)."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        env = om.make_env(game)
        cells = env.width * env.height
        moves, player = [], 1
        while cells - len(moves) > empty:
            legal = np.flatnonzero(env.valid_moves())
            a = int(legal[rng.integers(len(legal))])
            _, _, done, _ = env.step(a, player=player)
            moves.append(a)
            player = -player
            if done:
                moves = None
                break
        if moves is not None and moves not in out:
            out.append(moves)
    return out


def searched_tree(game, moves, sims, salt=1, seed=0, threads=1):
    """An OracleTree (table net `salt`) taken to the position after `moves` by play_action and searched once."""
    from tests.parity_helpers import A_OF

    np.random.seed(seed)
    t = OracleTree(game, TableNet(A_OF[game], salt=salt), NumpyRNG(), sims, threads=threads)
    for a in moves:
        t.play_action(a)
    t.search()
    return t


def code_to_value(code, empty):
    """A solver's move code at a root of `empty` empty cells as the value of the move: +k -> e + 1 - k, -k ->
    -(e + 1 - k), 0 -> 0 (the inverse of tree.bounds_to_codes)."""
    code = int(code)
    return empty + 1 - code if code > 0 else (-(empty + 1 + code) if code < 0 else 0)
