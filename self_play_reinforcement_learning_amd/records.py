"""Game records and their exact grading (include/spmcts.h spmcts_games_set_log, spmcts_export_games,
spmcts_log_positions; csrc/records.h).

    GameRecords     the move lists of finished games with their ids, results and (league games) player names
    log_positions   records -> the position before every move, on the device or through the host twin
    grade_games     every move of the records' endgames held against the exact solver (solve.py), the rest against
                    the depth-limited negamax (mcts.solve_positions) if a depth is given

A record's moves are played from the empty board, the first mover's stones +1 ("X").  `swap` says which tree
moved first: side 0 is tree 2g (a league pairing's first player, an evaluation's policy), side 1 tree 2g + 1, and
the mover of ply p is side (p + swap) & 1.  `result` is the game's outcome in side 0's view.
"""
import json

import numpy as np
import torch

from . import _lib
from .arena import GAMES, game_of_env
from .solve import ILLEGAL

STATUS = ("legal", "illegal move", "move after the end of the game", "plies out of range")


def _game(game):
    game = game if isinstance(game, str) else game_of_env(game)
    if game not in GAMES:
        raise ValueError(f"unknown game {game!r}")
    return game


def _env(game):
    from .envs import Connect4Env, TicTacToeEnv

    _, W, H, _ = GAMES[game]
    return TicTacToeEnv() if game == "tictactoe" else Connect4Env(W, H)


def _board_text(board):
    """A board int [W, H] as text rows, the top row first: X the first mover's stones, O the other side's."""
    W, H = board.shape
    sym = {0: ".", 1: "X", -1: "O"}
    return ["".join(sym[int(board[x, y])] for x in range(W)) for y in reversed(range(H))]


class GameRecords:
    """The records of finished games as host arrays: ids int64 [n], slot int32 [n], result int8 [n] (side 0's
    view), swap uint8 [n], plies int32 [n], opening int32 [n] (-1: none), moves uint8 [n, W*H] (bytes past plies
    zero); for league games also names (a [side 0, side 1] pair of player names per record) and pairing int32 [n]
    (the schedule's pairing, -1: none)."""

    def __init__(self, game):
        self.game = _game(game)
        _, W, H, A = GAMES[self.game]
        self.W, self.H, self.A, self.cells = W, H, A, W * H
        self.ids = np.zeros(0, dtype=np.int64)
        self.slot = np.zeros(0, dtype=np.int32)
        self.result = np.zeros(0, dtype=np.int8)
        self.swap = np.zeros(0, dtype=np.uint8)
        self.plies = np.zeros(0, dtype=np.int32)
        self.opening = np.zeros(0, dtype=np.int32)
        self.moves = np.zeros((0, self.cells), dtype=np.uint8)
        self.pairing = np.zeros(0, dtype=np.int32)
        self.names = []

    def __len__(self):
        return int(self.ids.shape[0])

    _ARRAYS = ("ids", "slot", "result", "swap", "plies", "opening", "moves", "pairing")

    def append_arrays(self, ids, slot, result, swap, plies, opening, moves, pairing=None, names=None):
        n = len(ids)
        new = dict(ids=ids, slot=slot, result=result, swap=swap, plies=plies, opening=opening,
                   moves=np.asarray(moves).reshape(n, self.cells),
                   pairing=np.full(n, -1, dtype=np.int32) if pairing is None else pairing)
        for k in self._ARRAYS:
            cur = getattr(self, k)
            setattr(self, k, np.concatenate([cur, np.asarray(new[k]).astype(cur.dtype)]))
        self.names += [None] * n if names is None else [None if x is None else [str(x[0]), str(x[1])] for x in names]
        return self

    def append_export(self, export, id_offset=0, pairing=None, names=None):
        """Append what Arena.export_games returned (device tensors); id_offset is added to the ids."""
        h = {k: v.cpu().numpy() for k, v in export.items()}
        return self.append_arrays(h["id"] + id_offset, h["slot"], h["result"], h["swap"], h["plies"], h["opening"],
                                  h["moves"], pairing, names)

    def extend(self, other):
        if other.game != self.game:
            raise ValueError(f"records of {other.game} cannot extend records of {self.game}")
        return self.append_arrays(*[getattr(other, k) for k in self._ARRAYS], names=other.names)

    def moves_of(self, i):
        return [int(a) for a in self.moves[i, :int(self.plies[i])]]

    def as_openings(self, plies):
        """The first `plies` moves of every record, in the form openings= takes (a list of move lists)."""
        return [self.moves_of(i)[:int(plies)] for i in range(len(self))]

    # ------------------------------------------------------------------ files: JSON, data only
    def to_json(self):
        return dict(game=self.game, ids=self.ids.tolist(), slot=self.slot.tolist(), result=self.result.tolist(),
                    swap=self.swap.tolist(), opening=self.opening.tolist(), pairing=self.pairing.tolist(),
                    names=self.names, moves=[self.moves_of(i) for i in range(len(self))])

    @classmethod
    def from_json(cls, obj):
        r = cls(obj["game"])
        n = len(obj["ids"])
        moves = np.zeros((n, r.cells), dtype=np.uint8)
        for i, m in enumerate(obj["moves"]):
            if len(m) > r.cells:
                raise ValueError(f"record {i} has {len(m)} moves, the board {r.cells} cells")
            moves[i, :len(m)] = m
        return r.append_arrays(np.asarray(obj["ids"], dtype=np.int64), obj["slot"], obj["result"], obj["swap"],
                               [len(m) for m in obj["moves"]], obj["opening"], moves,
                               np.asarray(obj["pairing"], dtype=np.int32), obj["names"])

    def save(self, path):
        with open(path, "w") as f:
            json.dump(self.to_json(), f)

    @classmethod
    def load(cls, path):
        with open(path) as f:
            return cls.from_json(json.load(f))

    # ------------------------------------------------------------------ text
    def render(self, i):
        """Game i as text: a header, then for every ply the mover and its move and the board after it."""
        names = self.names[i] or ["side 0", "side 1"]
        swap = int(self.swap[i])
        res = {1: f"{names[0]} wins", 0: "draw", -1: f"{names[1]} wins"}[int(np.sign(self.result[i]))]
        out = [f"game {int(self.ids[i])}: X {names[swap]}, O {names[1 - swap]}, {int(self.plies[i])} plies, {res}"]
        env = _env(self.game)
        env.reset()
        for p, a in enumerate(self.moves_of(i)):
            env.step(a, 1 if p % 2 == 0 else -1)
            out.append(f"ply {p}: {'XO'[p & 1]} ({names[(p + swap) & 1]}) plays {a}")
            out += _board_text(env.board)
        return "\n".join(out)


def from_moves(game, move_lists):
    """Records of games typed in or read from a file: move lists from the empty board.  Ids 0 .. n - 1, no swap
    (side 0 moves first), the result filled in by replay (0 for a game that is not finished).  ValueError for a move
    list that is not a legal game."""
    r = GameRecords(game)
    n = len(move_lists)
    moves = np.zeros((n, r.cells), dtype=np.uint8)
    plies = np.zeros(n, dtype=np.int32)
    for i, m in enumerate(move_lists):
        m = [int(a) for a in m]
        if len(m) > r.cells or any(not 0 <= a < 256 for a in m):
            raise ValueError(f"game {i}: {len(m)} moves on a board of {r.cells} cells, or a move outside 0 .. 255")
        moves[i, :len(m)] = m
        plies[i] = len(m)
    st = log_positions(game, moves, plies, first_ply=r.cells, device="cpu")["status"].numpy()
    if st.any():
        i = int(np.flatnonzero(st)[0])
        raise ValueError(f"game {i} is not a legal game: {STATUS[st[i]]}")
    result = np.zeros(n, dtype=np.int8)
    env = _env(r.game)
    for i in range(n):
        env.reset()
        for p in range(plies[i]):
            _, rew, _, _ = env.step(int(moves[i, p]), 1 if p % 2 == 0 else -1)
            if rew:
                result[i] = 1 if p % 2 == 0 else -1
    return r.append_arrays(np.arange(n, dtype=np.int64), np.full(n, -1), result, np.zeros(n), plies, np.full(n, -1), moves)


def log_positions(game, moves, plies, first_ply=0, device=None):
    """The position before every move p >= first_ply of every legal record (spmcts_log_positions; device="cpu": its
    host twin, no GPU).  moves uint8 [n, W*H], plies int32 [n].  Returns tensors on `device`: boards int8 [N, W, H]
    (the first mover's stones +1), players int8 [N] (+1 on even plies), row_record and row_ply int32 [N] in (record,
    ply) order, status uint8 [n] (0 legal, 1 an illegal move, 2 a move after the game's end, 3 plies out of range; a
    record with a non-zero status has no rows) and offsets int32 [n + 1] (each record's first row; [n] = N)."""
    game = _game(game)
    gid, W, H, A = GAMES[game]
    cells = W * H
    if isinstance(first_ply, bool) or not isinstance(first_ply, (int, np.integer)) or first_ply < 0:
        raise ValueError(f"first_ply must be an integer >= 0, got {first_ply!r}")
    mv = np.ascontiguousarray(torch.as_tensor(moves).cpu().numpy().astype(np.uint8, copy=False)).reshape(-1, cells)
    pl = np.ascontiguousarray(torch.as_tensor(plies).cpu().numpy().astype(np.int32, copy=False)).reshape(-1)
    n = mv.shape[0]
    if pl.shape[0] != n:
        raise ValueError(f"{n} move rows but {pl.shape[0]} ply counts")
    cap = int(np.clip(np.clip(pl, 0, cells) - int(first_ply), 0, None).sum())  # enough for every legal record
    host = torch.device(device if device is not None else "cuda").type == "cpu"
    dev = torch.device("cpu") if host else (torch.device(device) if device is not None else
                                            torch.device("cuda", torch.cuda.current_device()))
    out = dict(boards=torch.zeros((cap, W, H), dtype=torch.int8, device=dev),
               players=torch.zeros(cap, dtype=torch.int8, device=dev),
               row_record=torch.zeros(cap, dtype=torch.int32, device=dev),
               row_ply=torch.zeros(cap, dtype=torch.int32, device=dev),
               status=torch.zeros(n, dtype=torch.uint8, device=dev),
               offsets=torch.zeros(n + 1, dtype=torch.int32, device=dev))
    if n == 0:
        return out
    m, p = torch.as_tensor(mv).to(dev), torch.as_tensor(pl).to(dev)
    args = [gid, W, H, _lib.ptr(m), _lib.ptr(p), n, int(first_ply), cap] + \
           [_lib.ptr(out[k]) for k in ("boards", "players", "row_record", "row_ply", "status", "offsets")]
    if host:
        _lib.call("spmcts_log_positions_host", *args)
    else:
        from .arena import _stream

        with torch.cuda.device(dev):
            _lib.call("spmcts_log_positions", *args, _stream())
    N = int(out["offsets"][n])
    for k in ("boards", "players", "row_record", "row_ply"):
        out[k] = out[k][:N]
    return out


def _exact_codes(game, boards, players, max_nodes, table, host):
    """(score int8 [n, A], nodes int64 [n]) of the exact solver, on the device or through its host twin."""
    from .solve import HostSolveTable, SolveTable, solve_host, solve_to_end

    n, A = boards.shape[0], GAMES[game][3]
    if not host:
        table = table if table is not None else SolveTable(game, device=boards.device)
        s = solve_to_end(game, boards=boards, players=players, max_nodes=max_nodes, table=table)
        return s["score"], s["nodes"]
    table = table if table is not None else HostSolveTable(game)
    score = torch.full((n, A), ILLEGAL, dtype=torch.int8)
    nodes = torch.zeros(n, dtype=torch.int64)
    for i in range(n):
        c, k = solve_host(game, boards[i].numpy(), int(players[i]), table=table, max_nodes=max_nodes)
        score[i] = torch.as_tensor(c)
        nodes[i] = k
    return score, nodes


def _horizon_codes(game, boards, players, depth, host):
    from .hardcoded_players import negamax_host
    from .mcts import solve_positions

    if not host:
        return solve_positions(game, boards=boards, players=players, depth=depth, device=boards.device)["score"]
    score = torch.zeros((boards.shape[0], GAMES[game][3]), dtype=torch.int8)
    for i in range(boards.shape[0]):
        score[i] = torch.as_tensor(negamax_host(game, boards[i].numpy(), int(players[i]), depth)[0])
    return score


def grade_games(game, records, max_empty=12, depth=0, first_ply=0, max_nodes=1 << 22, table=None, device=None):
    """Every move of `records` (a GameRecords) from ply first_ply on, held against the truth.

    The positions come from log_positions.  Exact tier: a position with at most max_empty empty cells goes to the
    exact solver (solve.solve_to_end; table: a SolveTable kept across calls) and its move is graded with
    solve.perfect_report (strong, weak) and mcts.tactical_report (the class).  Horizon tier: with depth > 0 every
    other position goes to the depth-limited negamax (mcts.solve_positions) and gets tactical_report's class only;
    it is never counted as exact.  A position of the exact tier that does not solve within max_nodes moves (a move
    of its carries -127) is counted in n_unsolved and appears in no ratio.  device="cpu" runs the same through the
    host twins (no GPU; a solve.HostSolveTable as table).

    Returns a dict.  Per row (tensors on the device, rows in (record, ply) order): record, ply int32; side int8 (0:
    tree 2g's move, 1: tree 2g + 1's, (ply + swap) & 1); action int64; chosen int8 (the played move's code) and
    value int8 (the position's best code), 0 where the row is in no tier or unsolved; exact bool (exact tier and
    solved); horizon bool; strong, weak, blunder bool (exact rows only; a blunder changes the exact outcome for
    the worse); class int64 (index into mcts.TACTICAL_CLASSES, -1 where not graded); nodes int64 (exact tier).
    Aggregates: per_side {graded, strong, weak, blunders: int64 [n records, 2], first_blunder: int32 [n records, 2]
    (the ply, -1: none)}; players {name: {graded, strong, weak, blunders}} where the records name players; status
    uint8 [n records] (log_positions'); n_rows, n_graded (exact), n_strong, n_weak, n_blunders, n_unsolved,
    n_horizon, and classes {name: count} over the graded rows of both tiers."""
    from .mcts import TACTICAL_CLASSES, tactical_report
    from .solve import perfect_report, summarise

    game = _game(game)
    if records.game != game:
        raise ValueError(f"records of {records.game} graded as {game}")
    _, W, H, A = GAMES[game]
    if isinstance(max_empty, bool) or not isinstance(max_empty, int) or max_empty < 0:
        raise ValueError(f"max_empty must be an integer >= 0, got {max_empty!r}")
    if isinstance(depth, bool) or not isinstance(depth, int) or depth < 0:
        raise ValueError(f"depth must be an integer >= 0, got {depth!r}")
    pos = log_positions(game, records.moves, records.plies, first_ply, device)
    dev = pos["boards"].device
    host = dev.type == "cpu"
    n, N = len(records), pos["boards"].shape[0]
    rec, ply = pos["row_record"].long(), pos["row_ply"].long()
    swap = torch.as_tensor(records.swap.astype(np.int64)).to(dev)
    moves = torch.as_tensor(records.moves.astype(np.int64)).to(dev)
    side = (ply + swap[rec]) & 1 if N else ply
    action = moves[rec, ply] if N else ply
    empty = (pos["boards"] == 0).sum(dim=(1, 2)) if N else ply
    tier1 = empty <= max_empty
    chosen = torch.zeros(N, dtype=torch.int8, device=dev)
    value = torch.zeros(N, dtype=torch.int8, device=dev)
    exact = torch.zeros(N, dtype=torch.bool, device=dev)
    strong, weak = exact.clone(), exact.clone()
    cls = torch.full((N,), -1, dtype=torch.int64, device=dev)
    nodes = torch.zeros(N, dtype=torch.int64, device=dev)
    n_unsolved = 0
    i1 = torch.nonzero(tier1).reshape(-1)
    if i1.numel():
        score, nd = _exact_codes(game, pos["boards"][i1].contiguous(), pos["players"][i1].contiguous(), max_nodes,
                                 table, host)
        nodes[i1] = nd.to(dev)
        rep = perfect_report(score, action[i1])
        ok = rep["solved"]
        n_unsolved = int(rep["n_unsolved"])
        rows, sc, act = i1[ok], score[ok], action[i1][ok]
        if rows.numel():
            exact[rows] = True
            strong[rows], weak[rows] = rep["strong"][ok], rep["weak"][ok]
            tr = tactical_report(sc, act)
            chosen[rows], cls[rows] = tr["chosen"], tr["class"]
            value[rows] = summarise(sc)["value"]
    horizon = torch.zeros(N, dtype=torch.bool, device=dev)
    i2 = torch.nonzero(~tier1).reshape(-1)
    if depth > 0 and i2.numel():
        score = _horizon_codes(game, pos["boards"][i2].contiguous(), pos["players"][i2].contiguous(), depth, host).to(dev)
        tr = tactical_report(score, action[i2])
        horizon[i2] = True
        chosen[i2], cls[i2] = tr["chosen"], tr["class"]
        value[i2] = summarise(score)["value"]
    blunder = exact & ~weak
    # aggregates per (record, side) over the exact rows
    key = rec * 2 + side

    def per(mask):
        return torch.zeros(2 * n, dtype=torch.int64, device=dev).index_add_(0, key, mask.long()).reshape(n, 2)

    first = torch.full((2 * n,), 1 << 30, dtype=torch.int64, device=dev)
    if N:
        first = first.scatter_reduce(0, key[blunder], ply[blunder], reduce="amin")
    first = torch.where(first == 1 << 30, torch.full_like(first, -1), first).to(torch.int32).reshape(n, 2)
    per_side = dict(graded=per(exact), strong=per(strong), weak=per(weak), blunders=per(blunder), first_blunder=first)
    players = {}
    host_side = {k: per_side[k].cpu().numpy() for k in ("graded", "strong", "weak", "blunders")}
    for r, nm in enumerate(records.names):
        for s in range(2):
            if nm is not None:
                p = players.setdefault(nm[s], dict(graded=0, strong=0, weak=0, blunders=0))
                for k in p:
                    p[k] += int(host_side[k][r, s])
    graded = exact | horizon
    labels = cls[graded].cpu().tolist()
    return {"record": pos["row_record"], "ply": pos["row_ply"], "side": side.to(torch.int8), "action": action,
            "chosen": chosen, "value": value, "exact": exact, "horizon": horizon, "strong": strong, "weak": weak,
            "blunder": blunder, "class": cls, "nodes": nodes, "per_side": per_side, "players": players,
            "status": pos["status"], "n_rows": N, "n_graded": int(exact.sum()), "n_strong": int(strong.sum()),
            "n_weak": int(weak.sum()), "n_blunders": int(blunder.sum()), "n_unsolved": n_unsolved,
            "n_horizon": int(horizon.sum()),
            "classes": {name: labels.count(i) for i, name in enumerate(TACTICAL_CLASSES)}}
