"""The exact solver to the end of the game (include/spmcts.h "exact solver to the end of the game",
csrc/solve.h): an alpha-beta search with a transposition table on the device, for a batch of positions.

    SolveTable      a zeroed device table bound to one board, kept across calls
    solve_to_end    the codes of a batch of positions, every line run to the end of the game
    solve_host      the host twin on one position (no GPU)
    perfect_report  a chosen move held against the codes: strong- and weak-correct

The codes are solve_positions' (mcts.py) at a horizon that reaches the end of the game: +k a forced win in k
plies, -k a forced loss delayed to ply k, 0 a draw under best play, -128 an illegal move, and -127 (UNKNOWN) a
legal move whose search gave up at the node budget.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .arena import GAMES, game_of_env
from .hardcoded_players import negamax_rank

ILLEGAL = -128
UNKNOWN = -127
MIN_TABLE_ENTRIES = 1 << 16
DEFAULT_MAX_NODES = 1 << 24  # a position's budget of moves: a 7x6 position after 20 random plies needs 2e5 on average


def _game(game):
    game = game if isinstance(game, str) else game_of_env(game)
    if game not in GAMES:
        raise ValueError(f"unknown game {game!r}")
    return game


def _check_entries(entries):
    if isinstance(entries, bool) or not isinstance(entries, int) or entries < MIN_TABLE_ENTRIES or entries & (entries - 1):
        raise ValueError(f"a solve table holds a power-of-two number of entries, at least 2^16, got {entries!r}")
    return entries


def _check_max_nodes(max_nodes):
    if isinstance(max_nodes, bool) or not isinstance(max_nodes, int) or max_nodes < 1:
        raise ValueError(f"max_nodes must be an integer >= 1, got {max_nodes!r}")
    return max_nodes


def has_line(game, boards):
    """bool [n]: the board holds a line of L (3 on TicTacToe, 4 on the Connect4 boards) of either side.
    boards: int8 [n, W, H] (numpy)."""
    b = np.asarray(boards)
    n, W, H = b.shape
    L = 3 if game == "tictactoe" else 4
    out = np.zeros(n, dtype=bool)
    for side in (1, -1):
        m = b == side
        for dx, dy in ((1, 0), (0, 1), (1, 1), (1, -1)):
            w, h = W - (L - 1) * dx, H - (L - 1) * abs(dy)
            if w <= 0 or h <= 0:
                continue
            y0 = (L - 1) if dy < 0 else 0
            run = np.ones((n, w, h), dtype=bool)
            for k in range(L):
                run &= m[:, k * dx:k * dx + w, y0 + k * dy:y0 + k * dy + h]
            out |= run.any(axis=(1, 2))
    return out


def check_unfinished(game, boards):
    """ValueError unless every board int8 [n, W, H] is unfinished: not full, no line of either side."""
    b = np.asarray(boards)
    full = (b != 0).all(axis=(1, 2))
    line = has_line(game, b)
    bad = np.flatnonzero(full | line)
    if len(bad):
        i = int(bad[0])
        raise ValueError(f"position {i} is finished ({'the board is full' if full[i] else 'the board holds a line'}): "
                         f"the solver takes unfinished positions only")


class HostSolveTable:
    """A zeroed host table of the host twin (solve_host), bound to one board."""

    def __init__(self, game, entries=1 << 20):
        self.game = _game(game)
        self.entries = _check_entries(entries)
        self.data = np.zeros(entries, dtype=np.uint64)

    def clear(self):
        self.data[:] = 0


def solve_host(game, board, player, table=None, max_nodes=DEFAULT_MAX_NODES):
    """The host twin (spmcts_solve_host; no GPU) on one position: board [W, H] of +-1 stones, player = the side
    to move.  table: a HostSolveTable of the board (a fresh one of 2^20 entries if None).  Returns (codes int8
    [A], nodes).  ValueError for a finished position or a table of another board."""
    game = _game(game)
    gid, W, H, A = GAMES[game]
    table = table if table is not None else HostSolveTable(game)
    if not isinstance(table, HostSolveTable) or table.game != game:
        raise ValueError(f"the table is not a HostSolveTable of {game}")
    b = np.ascontiguousarray(np.asarray(board).reshape(W, H), dtype=np.int8)
    check_unfinished(game, b[None])
    codes = np.full(A, ILLEGAL, dtype=np.int8)
    nodes = ctypes.c_uint64()
    _lib.call("spmcts_solve_host", gid, W, H, b.ctypes.data_as(ctypes.c_void_p), int(player),
              table.data.ctypes.data_as(ctypes.c_void_p), table.entries, _check_max_nodes(max_nodes),
              codes.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nodes))
    return codes, int(nodes.value)


def positions_to_boards(game, positions):
    """Move lists from the empty board (validated like an opening book: legal, not ending the game), player 1
    first -> (boards int8 [n, W, H], players int8 [n]: 1 after an even number of moves, -1 after an odd one)."""
    from .envs import Connect4Env, TicTacToeEnv
    from .openings import validate_openings

    game = _game(game)
    _, W, H, _ = GAMES[game]
    seqs = validate_openings(game, positions)
    env = TicTacToeEnv() if game == "tictactoe" else Connect4Env(W, H)
    bs = np.zeros((len(seqs), W, H), dtype=np.int8)
    for i, seq in enumerate(seqs):
        env.reset()
        for p, a in enumerate(seq):
            env.step(a, 1 if p % 2 == 0 else -1)
        bs[i] = env.board
    return bs, np.array([1 if len(s) % 2 == 0 else -1 for s in seqs], dtype=np.int8)


class SolveTable:
    """A zeroed device transposition table bound to one board (the entries of two boards would collide), kept
    across solve_to_end calls: what one batch proved serves the next."""

    def __init__(self, game, entries=1 << 22, device=None):
        self.game = _game(game)
        self.entries = _check_entries(entries)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.data = torch.zeros(entries, dtype=torch.int64, device=self.device)

    def clear(self):
        self.data.zero_()


def solve_to_end(game, positions=None, boards=None, players=None, max_nodes=DEFAULT_MAX_NODES, table=None, device=None,
                 launch_nodes=0):
    """The truth about a batch of positions, to the end of the game (spmcts_solve_batch; no network, no arena).

    positions / boards / players: as solve_positions takes them; every position must be unfinished (not full, no
    line of either side): ValueError otherwise.  max_nodes: a position's budget of moves; a position that reaches
    it stops, and the moves it has not finished carry -127.  table: a SolveTable of this board (a fresh one if
    None).  launch_nodes: the steps a lane takes per kernel launch (0: the library's default).

    Returns device tensors: score int8 [n, A] (the codes at the top of this file); solved bool [n]: no move carries
    -127; value int8 [n], best bool [n, A]: the best code and the moves that carry it, over the moves that are
    known; outcome int8 [n]: +1 / 0 / -1 for the mover under best play (valid where solved); nodes int64 [n];
    and launches, the kernel launches the batch took (an int)."""
    from .arena import _stream

    game = _game(game)
    gid, W, H, A = GAMES[game]
    max_nodes = _check_max_nodes(max_nodes)
    if isinstance(launch_nodes, bool) or not isinstance(launch_nodes, int) or not (launch_nodes == 0 or 4 <= launch_nodes < 1 << 32):
        raise ValueError(f"launch_nodes must be 0 (the default) or an integer >= 4, got {launch_nodes!r}")
    dev = torch.device(device) if device is not None else (
        table.device if table is not None else torch.device("cuda", torch.cuda.current_device()))
    if (positions is None) == (boards is None):
        raise ValueError("solve_to_end takes either positions= (move lists) or boards= with players=")
    if positions is not None:
        bs, pls = positions_to_boards(game, positions)
    else:
        if players is None:
            raise ValueError("boards= needs players= (the side to move of each board)")
        bs = torch.as_tensor(boards).to("cpu", torch.int8).reshape(-1, W, H).numpy()
        pls = torch.as_tensor(players).to("cpu", torch.int8).reshape(-1).numpy()
    n = bs.shape[0]
    if pls.shape[0] != n:
        raise ValueError(f"{n} boards but {pls.shape[0]} players")
    if n and not (np.isin(bs, (-1, 0, 1)).all() and np.isin(pls, (-1, 1)).all()):
        raise ValueError("boards hold -1, 0 and 1, players -1 and 1")
    check_unfinished(game, bs)
    if table is None:
        table = SolveTable(game, device=dev)
    if not isinstance(table, SolveTable) or table.game != game:
        raise ValueError(f"the table is not a SolveTable of {game}")
    if table.device != dev:
        raise ValueError(f"the table lives on {table.device}, the batch on {dev}")
    b = torch.as_tensor(np.ascontiguousarray(bs)).to(dev)
    pl = torch.as_tensor(np.ascontiguousarray(pls)).to(dev)
    score = torch.full((n, A), ILLEGAL, dtype=torch.int8, device=dev)
    nodes = torch.zeros(n, dtype=torch.int64, device=dev)
    launches = 0
    if n:
        size = ctypes.c_uint64()
        _lib.call("spmcts_solve_work_bytes", gid, W, H, n, ctypes.byref(size))
        work = torch.empty(int(size.value), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.call("spmcts_solve_batch", gid, W, H, _lib.ptr(b), _lib.ptr(pl), n, _lib.ptr(table.data), table.entries,
                      _lib.ptr(work), max_nodes, launch_nodes, _lib.ptr(score), _lib.ptr(nodes), _stream())
            launches = int(_lib.lib().spmcts_solve_launches())
    out = summarise(score)
    out.update(nodes=nodes, launches=launches)
    return out


def summarise(score):
    """score int8 [n, A] -> dict(score, solved, value, best, outcome) (solve_to_end's; pure torch)."""
    score = torch.as_tensor(score)
    n = score.shape[0]
    known = (score != ILLEGAL) & (score != UNKNOWN)
    solved = ~(score == UNKNOWN).any(dim=1)
    rank = torch.where(known, negamax_rank(score), torch.full_like(score, -(1 << 20), dtype=torch.int64))
    top = rank.max(dim=1, keepdim=True).values if n else rank[:, :1]
    best = (rank == top) & known
    value = torch.where(known.any(dim=1), (score.long() * best).sum(dim=1) // best.sum(dim=1).clamp(min=1),
                        torch.zeros(n, dtype=torch.int64, device=score.device)).to(torch.int8)
    return dict(score=score, solved=solved, value=value, best=best, outcome=torch.sign(value).to(torch.int8))


def perfect_report(score, action, solved=None):
    """Each position's chosen move held against the exact codes of solve_to_end (score int8 [n, A], action [n],
    solved bool [n]; None: the rows without a -127).  Pure torch.  Over the solved rows only:
        strong   the chosen move carries the best code (the fastest win, the slowest loss)
        weak     the chosen move's code has the sign of the position's value: it keeps the win, the draw or
                 the loss
    Returns {"strong": bool [n], "weak": bool [n] (False on unsolved rows), "solved": bool [n], "n_solved",
    "n_strong", "n_weak", "n_unsolved"}.  ValueError if a chosen move of a solved row is illegal."""
    score = torch.as_tensor(score)
    n = score.shape[0]
    action = torch.as_tensor(action).to(score.device, torch.int64).reshape(-1)
    if action.shape[0] != n:
        raise ValueError(f"{n} score rows but {action.shape[0]} actions")
    s = summarise(score)
    solved = s["solved"] if solved is None else torch.as_tensor(solved).to(score.device, torch.bool).reshape(-1) & s["solved"]
    chosen = score.long().gather(1, action.reshape(-1, 1)).reshape(-1) if n else score.long().reshape(-1)[:0]
    if bool(((chosen == ILLEGAL) & solved).any()):
        raise ValueError("a chosen move is illegal (code -128)")
    strong = s["best"].gather(1, action.reshape(-1, 1)).reshape(-1) & solved if n else solved
    weak = (torch.sign(chosen) == torch.sign(s["value"].long())) & solved
    return {"strong": strong, "weak": weak, "solved": solved, "n_solved": int(solved.sum()),
            "n_strong": int(strong.sum()), "n_weak": int(weak.sum()), "n_unsolved": int(n - int(solved.sum()))}
