"""Helpers of the end-of-game solver's tests (tests/test_solve.py, tests/test_gpu_solve.py): the position sets and
the host twin's answers, computed once and shared.

Sets, per board:
  late(game)    seeded random playouts of a fixed length, redrawn until LATE_COUNT are unfinished (most random
                playouts of that length have ended: the draws used are recorded in DRAWS); 6 to 12 empty cells
  deep(game)    the same with 14 to 22 empty cells (12 to 20 on 6x5), kept where the host twin needs at most
                DEEP_MAX_NODES moves on a cleared table
  carved(game)  negamax_helpers.drawn_board with 1 to 12 cells taken off the top of one to four columns: no line
                by construction; both players to move, a single open column, one and two stones from full
  TicTacToe     negamax_helpers.positions("tictactoe")
The independent truth is negamax_helpers.brute at D = the number of empty cells.
"""
import numpy as np

from tests import negamax_helpers as nh

X = nh.X
UNKNOWN = -127
GRAVITY = ["connect4", "connect4_6_5", "connect4_8_7"]
# plies of the playouts: late leaves 6 .. 12 empties, deep 14 .. 22 (6x5: 12 .. 20)
LATE_PLIES = {"connect4": (30, 32, 34, 36), "connect4_6_5": (18, 20, 22, 24), "connect4_8_7": (44, 46, 48, 50)}
DEEP_PLIES = {"connect4": (20, 23, 26, 28), "connect4_6_5": (10, 13, 16, 18), "connect4_8_7": (34, 37, 40, 42)}
LATE_COUNT = 3   # per length
DEEP_COUNT = 4   # per length, before the node filter
DEEP_MAX_NODES = 300_000
DRAWS = {}       # (game, plies, seed) -> playouts drawn to get the unfinished ones
_CACHE = {}


def empties(board):
    return int((np.asarray(board) == 0).sum())


def playouts(game, plies, count, seed):
    """`count` unfinished positions after `plies` random plies: [(board int8 [W, H], player)]."""
    rng = np.random.default_rng(seed)
    out, draws = [], 0
    while len(out) < count:
        assert draws < 4000, (game, plies)
        draws += 1
        env = nh.make_env(game)
        env.reset()
        player, done = 1, False
        for _ in range(plies):
            a = int(rng.choice(np.flatnonzero(env.valid_moves())))
            _, _, done, _ = env.step(a, player)
            if done:
                break
            player = -player
        if not done:
            out.append((env.board.astype(np.int8), player))
    DRAWS[(game, plies, seed)] = draws
    return out


def move_lists(game, plies, count, seed):
    """`count` unfinished playouts of `plies` random plies as move lists from the empty board."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(4000):
        env = nh.make_env(game)
        env.reset()
        player, done, moves = 1, False, []
        for _ in range(plies):
            a = int(rng.choice(np.flatnonzero(env.valid_moves())))
            _, _, done, _ = env.step(a, player)
            moves.append(a)
            if done:
                break
            player = -player
        if not done:
            out.append(moves)
            if len(out) == count:
                return out
    raise AssertionError((game, plies))


def late(game):
    key = ("late", game)
    if key not in _CACHE:
        out = []
        for plies in LATE_PLIES[game]:
            out += playouts(game, plies, LATE_COUNT, seed=plies)
        assert all(6 <= empties(b) <= 12 for b, _ in out)
        _CACHE[key] = out
    return _CACHE[key]


def carved(game):
    """Boards carved from the drawn full board: (cells taken per column, player)."""
    key = ("carved", game)
    if key not in _CACHE:
        w, h = nh.SIZES[game]
        full = nh.drawn_board(game)
        specs = [([1] + [0] * (w - 1), 1), ([0] * (w - 1) + [1], -1),          # one stone from full
                 ([1, 1] + [0] * (w - 2), 1), ([2] + [0] * (w - 1), -1),        # two stones from full
                 ([0, 0, min(h, 5)] + [0] * (w - 3), 1), ([min(h, 5)] + [0] * (w - 1), -1),  # a single open column
                 ([3, 2] + [0] * (w - 2), 1), ([0, 2, 3, 1] + [0] * (w - 4), -1),
                 ([0] * (w - 3) + [2, 3, 3], 1), ([3, 3, 3, 3] + [0] * (w - 4), -1),
                 ([1, 4, 0, 4] + [0] * (w - 4), 1), ([2, 0, 3] + [0] * (w - 4) + [4], -1),
                 ([0, 3, 4, 3, 2] + [0] * (w - 5), 1)]
        out = []
        for cells, player in specs:
            assert len(cells) == w and 1 <= sum(cells) <= 12 and 1 <= sum(1 for k in cells if k) <= 4
            b = full.copy()
            for x, k in enumerate(cells):
                if k:
                    b[x, h - k:] = 0
            assert not nh.has_line(game, b)
            out.append((b, player))
        _CACHE[key] = out
    return _CACHE[key]


def small(game):
    """The positions the brute force reaches: (a) late and (b) carved on the gravity boards, (c) on TicTacToe."""
    if game == "tictactoe":
        return nh.positions("tictactoe")
    return late(game) + carved(game)


def host_table(game, entries=1 << 20):
    from self_play_reinforcement_learning_amd.solve import HostSolveTable

    return HostSolveTable(game, entries)


def host_solve(game, board, player, table=None, max_nodes=1 << 26):
    from self_play_reinforcement_learning_amd.solve import solve_host

    return solve_host(game, board, player, table=table, max_nodes=max_nodes)


def deep(game):
    """[(board, player, codes, nodes)]: the deep playouts the host twin solves in at most DEEP_MAX_NODES moves, each
    on a cleared table of 2^20 entries (so `nodes` is the position's own count)."""
    key = ("deep", game)
    if key not in _CACHE:
        table = host_table(game)
        out = []
        for plies in DEEP_PLIES[game]:
            for board, player in playouts(game, plies, DEEP_COUNT, seed=1000 + plies):
                table.clear()
                codes, nodes = host_solve(game, board, player, table, max_nodes=DEEP_MAX_NODES)
                if not (codes == UNKNOWN).any():
                    out.append((board, player, codes, nodes))
        assert out, game
        lo, hi = (12, 20) if game == "connect4_6_5" else (14, 22)
        assert all(lo <= empties(b) <= hi for b, _, _, _ in out)
        _CACHE[key] = out
    return _CACHE[key]


def small_solved(game):
    """[(board, player, codes, nodes)] of small(game), the host twin's answers on one warm table."""
    key = ("small_solved", game)
    if key not in _CACHE:
        table = host_table(game, 1 << 16)
        _CACHE[key] = [(b, p) + host_solve(game, b, p, table) for b, p in small(game)]
    return _CACHE[key]


def pool(game):
    """The GPU tests' pool: small(game) and, on the gravity boards, deep(game), with the host twin's codes."""
    return small_solved(game) + (deep(game) if game != "tictactoe" else [])


def step(game, board, player, action):
    """(child board, reward, done) of `player` playing `action` (the oracle env)."""
    env = nh.make_env(game)
    env.set_state(np.asarray(board, dtype=np.int64).copy())
    env.episode_over = False
    b, r, done, _ = env.step(int(action), player)
    return b.astype(np.int8), int(r), bool(done)


def value_of(codes):
    """The best code of a row (by the preference order) and the moves that carry it."""
    legal = [a for a in range(len(codes)) if codes[a] not in (X, UNKNOWN)]
    top = max(nh.rank(codes[a]) for a in legal)
    best = [a for a in legal if nh.rank(codes[a]) == top]
    return int(codes[best[0]]), best
