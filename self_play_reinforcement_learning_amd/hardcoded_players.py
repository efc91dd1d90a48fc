"""Hard-coded opponents with the reference API (games/general/hardcoded_players.py:8-56).

`OneStepLookahead` and `Random` keep the reference's BasePlayer surface for
interactive play on the host envs (`__call__(s) -> action`, `reset(player)`,
`play_action(action, player)`).  Passed as the `policy_gen` of an
`evaluation_policy_container`, they make `SelfPlayScheduler.compare_models` /
evaluation games run them ON THE DEVICE as arena players
(`SPMCTS_PLAYER_LOOKAHEAD` / `SPMCTS_PLAYER_RANDOM`, csrc/arena_games.h
`hardcoded_move`) against the policy's trees.

`Negamax` has no reference form: it looks `depth` plies ahead exactly (the host twin of the device solver,
csrc/negamax.h), a player whose strength is fixed by construction; on the device it is
`SPMCTS_PLAYER_NEGAMAX`.
"""
import ctypes
import random

import numpy as np

from . import _lib
from .base_model import BasePlayer


class OneStepLookahead(BasePlayer):
    """Win if a move ends the game for `player`, else block one that ends it for `-player`,
    else a random valid move (hardcoded_players.py:18-33; `done` includes a full board)."""

    def __init__(self, env, player=-1, **kwargs):
        self.env = env()
        self.env_gen = env
        self.player = player

    def __call__(self, s):
        state = self.env.get_state()[0].copy()
        possible_moves = [i for i, ok in enumerate(self.env.valid_moves()) if ok]
        test_env = self.env_gen()
        for who in (self.player, -self.player):
            for a in possible_moves:
                test_env.set_state(state.copy())
                _, _, done, _ = test_env.step(a, who)
                if done:
                    return a
        return random.choice(possible_moves)

    def reset(self, player=None):
        self.player = player
        self.env.reset()

    def play_action(self, action, player):
        self.env.step(action, player)


ILLEGAL = -128  # the code of an illegal move (include/spmcts.h "exact depth-limited negamax")


def negamax_max_depth(game):
    """The deepest horizon of the negamax solver on an arena game name (9 for TicTacToe, 8 for Connect4)."""
    from .arena import GAMES

    gid, W, H, _ = GAMES[game]
    return int(_lib.lib().spmcts_negamax_max_depth(gid, W, H))


def negamax_host(game, board, player, depth):
    """The host twin of the device solver (spmcts_negamax_host; no GPU) on one position: `board` [W, H] of +-1
    stones, `player` the side to move.  Returns (codes int8 [A], nodes): +k a forced win in k plies, -k a forced
    loss delayed to ply k, 0 undecided within `depth` plies, -128 illegal.  ValueError for a depth outside
    [1, negamax_max_depth(game)]."""
    from .arena import GAMES

    gid, W, H, A = GAMES[game]
    cap = negamax_max_depth(game)
    if not isinstance(depth, (int, np.integer)) or isinstance(depth, bool) or not 1 <= depth <= cap:
        raise ValueError(f"negamax depth must be an integer in [1, {cap}] on {game}, got {depth!r}")
    b = np.ascontiguousarray(np.asarray(board).reshape(W, H), dtype=np.int8)
    codes = np.zeros(A, dtype=np.int8)
    nodes = ctypes.c_uint64()
    _lib.call("spmcts_negamax_host", gid, W, H, b.ctypes.data_as(ctypes.c_void_p), int(player), int(depth),
              codes.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nodes))
    return codes, int(nodes.value)


def negamax_rank(codes):
    """The preference order +1 > +3 > ... > 0 > ... > -4 > -2 as integers (larger is better; illegal moves
    lowest).  Works on numpy arrays and torch tensors alike."""
    c = codes.astype(np.int64) if isinstance(codes, np.ndarray) else codes.long()
    return (c > 0) * (256 - c) + (c < 0) * (-256 - c) + (c == ILLEGAL) * -1024


class Negamax(BasePlayer):
    """Looks `depth` plies ahead, perfectly: a move with the best code of the exact depth-limited negamax
    (negamax_host), chosen with random.choice among the best.  No reference form; on the device it is the arena
    player SPMCTS_PLAYER_NEGAMAX (csrc/negamax.h), whose strength is fixed by construction.

    The side to move is read off the board: the side with fewer stones, and `player` (the sign given to the
    constructor or to reset) where the counts are equal.  That holds both for play with true signs and under
    SelfPlayer's protocol, where an opposing player's own stones are +1 whatever sign reset() was given."""

    def __init__(self, env, depth=2, player=-1, **kwargs):
        from .arena import game_of_env

        self.env = env()
        self.env_gen = env
        self.player = player
        self.game = game_of_env(self.env)
        negamax_host(self.game, self.env.get_state()[0], 1, depth)  # ValueError for a depth out of range
        self.depth = int(depth)

    def mover(self):
        s = int(np.sum(self.env.get_state()[0]))
        return -1 if s > 0 else (1 if s < 0 else (self.player or 1))

    def scores(self):
        """(codes, nodes) of the env's position for the side to move."""
        return negamax_host(self.game, self.env.get_state()[0], self.mover(), self.depth)

    def __call__(self, s):
        codes, _ = self.scores()
        rank = negamax_rank(codes)
        return random.choice([int(a) for a in np.flatnonzero((rank == rank.max()) & (codes != ILLEGAL))])

    def reset(self, player=None):
        self.player = player
        self.env.reset()

    def play_action(self, action, player):
        self.env.step(action, player)


class Random(BasePlayer):
    """A uniformly random valid move (hardcoded_players.py:36-56)."""

    def __init__(self, env, player=-1, **kwargs):
        self.env = env()
        self.env_gen = env
        self.player = player

    def __call__(self, s):
        return random.choice([i for i, ok in enumerate(self.env.valid_moves()) if ok])

    def reset(self, player=None):
        self.env.reset()

    def play_action(self, action, player):
        self.env.step(action, player)
