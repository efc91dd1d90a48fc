"""Opening books: positions given as move sequences from the empty board.

An opening is a list of actions `m[0..L)`; `m[0]` is played by whoever moves first in the game.  Every move is
legal where it is played and none ends the game (include/spmcts.h spmcts_games_set_openings).  The arena plays
opening `((id mod period) >> 1) mod n` in game `id`, so ids 2k and 2k + 1 play one opening once per colour.

`enumerate_openings` builds a suite, `validate_openings` checks one with the package's own envs (the same
bitboard rules as the kernels, compiled for the host) and reports the first fault with the library's wording,
and `parse_openings` reads the command-line forms `all:N` and a JSON file of move lists.
"""
import json

import numpy as np

from . import _lib

MAX_OPENINGS = 65536  # include/spmcts.h spmcts_games_set_openings


def _game_name(env_or_game):
    if isinstance(env_or_game, str):
        return env_or_game
    from .arena import game_of_env

    return game_of_env(env_or_game)


def make_env(env_or_game):
    """A fresh env (envs.py) of an arena game name, or of a reference-style env class / instance."""
    from .arena import GAMES
    from .envs import Connect4Env, TicTacToeEnv

    game = _game_name(env_or_game)
    gid, W, H, _ = GAMES[game]
    env = Connect4Env(W, H) if gid == _lib.CONNECT4 else TicTacToeEnv()
    env.reset()
    return env


def _fault(env, seq):
    """(ply, reason) of the first move of `seq` that is illegal or ends the game, or None."""
    env.reset()
    player = 1  # legality and the game's end do not depend on who moves first
    for p, a in enumerate(seq):
        a = int(a)
        if a < 0 or a >= env.action_space.n or not env.valid_moves()[a]:
            return p, f"illegal move {a}"
        _, _, done, _ = env.step(a, player)
        if done:
            return p, f"move {a} ends the game"
        player = -player
    return None


def validate_openings(game, openings):
    """Raise ValueError("opening I ply P: ...") for the first sequence with an illegal or game-ending move: the
    index, ply and wording of the library's own check (spmcts_openings_validate).  Returns the openings as a list
    of int lists."""
    env = make_env(game)
    out = [[int(a) for a in seq] for seq in openings]
    if len(out) > MAX_OPENINGS:
        raise ValueError(f"openings: 0 .. {MAX_OPENINGS} sequences")
    cells = env.width * env.height
    for i, seq in enumerate(out):
        if len(seq) >= cells:
            raise ValueError(f"opening {i}: length {len(seq)} is not below width * height = {cells}")
        f = _fault(env, seq)
        if f is not None:
            raise ValueError(f"opening {i} ply {f[0]}: {f[1]}")
    return out


def enumerate_openings(env_or_game, plies, unique_positions=False):
    """Every legal, non-terminal move sequence of `plies` moves from the empty board, in lexicographic order.
    unique_positions=True keeps the first sequence that reaches each position."""
    env = make_env(env_or_game)
    n = env.action_space.n
    out, seen = [], set()

    def walk(seq, board, player):
        if len(seq) == plies:
            if unique_positions:
                key = board.tobytes()
                if key in seen:
                    return
                seen.add(key)
            out.append(list(seq))
            return
        env.set_state(board.copy())
        env.episode_over = False
        valid = env.valid_moves()
        for a in range(n):
            if not valid[a]:
                continue
            env.set_state(board.copy())
            env.episode_over = False
            b, _, done, _ = env.step(a, player)
            if done:
                continue
            walk(seq + [a], b.copy(), -player)

    walk([], env.reset().copy(), 1)
    return out


def pack_openings(openings):
    """(moves uint8 [n, max_len], lens int32 [n], max_len): the host arrays of spmcts_games_set_openings."""
    seqs = [[int(a) for a in s] for s in openings]
    for i, s in enumerate(seqs):
        for p, a in enumerate(s):
            if a < 0 or a > 255:
                raise ValueError(f"opening {i} ply {p}: illegal move {a}")
    max_len = max([len(s) for s in seqs], default=0)
    moves = np.zeros((max(len(seqs), 1), max(max_len, 1)), dtype=np.uint8)
    for i, s in enumerate(seqs):
        moves[i, :len(s)] = s
    # rows of max_len bytes (the table's stride), also when max_len is 0
    moves = np.ascontiguousarray(moves[:, :max_len]) if max_len else np.zeros((max(len(seqs), 1), 1), dtype=np.uint8)
    return moves, np.asarray([len(s) for s in seqs], dtype=np.int32).reshape(-1), max_len


def library_validate(game, openings):
    """The library's host-side check of a book (no arena, no GPU): raises SpmctsError with its message."""
    from .arena import GAMES

    gid, W, H, _ = GAMES[_game_name(game)]
    moves, lens, max_len = pack_openings(openings)
    _lib.call("spmcts_openings_validate", gid, W, H, moves.ctypes.data_as(_lib.ctypes.c_void_p),
              lens.ctypes.data_as(_lib.ctypes.c_void_p), len(lens), max_len)


def parse_openings(spec, game):
    """The command-line forms of a book: None / "" (no book), "all:N" (every N-ply opening), else the path of a
    JSON file holding a list of move lists; a list of move lists passes through.  The result is validated."""
    if spec is None or spec == "":
        return None
    if isinstance(spec, str):
        kind, _, arg = spec.partition(":")
        if kind == "all" and arg.isdigit():
            spec = enumerate_openings(game, int(arg))
        else:
            with open(spec) as f:
                spec = json.load(f)
    return validate_openings(game, spec)
