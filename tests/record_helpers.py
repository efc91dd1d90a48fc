"""Helpers of the game-record tests (tests/test_game_records.py, tests/test_gpu_game_records.py).

Host side: a replay of move lists through the oracle's Python envs (oracle/envs.py, the numpy restatement of the
reference's rules; independent of csrc/board.h), random legal games, and the expected output of log_positions
built from that replay.  GPU side: the loops of parity_helpers.run_g3_group / run_g5_group with the arena's game
log switched on or off and the finished-game ring drained every ply.
"""
import numpy as np

from tests.parity_helpers import _eval_table, empty_prior, g3_tapes, g5_tapes

BOARD_OF = {"connect4": (7, 6), "tictactoe": (3, 3), "connect4_6_5": (6, 5), "connect4_8_7": (8, 7)}
ALL_GAMES = sorted(BOARD_OF)


def _full_board(height, pairs, lone=()):
    """A full-board Connect4 draw.  Each column alternates colours from the bottom, X first in the columns that come
    first in `pairs` and in `lone`, O first in the others.  A pair (a, b) is filled by a, b, b, a over and over (X
    moves on even plies, so X gets a's even rows and b's odd ones; with an odd height the top cells are a for X, b for
    O), a lone column by alternate moves, which hands the move back to X only if the height is even."""
    moves = []
    for a, b in pairs:
        moves += [a, b, b, a] * (height // 2) + [a, b] * (height % 2)
    for c in lone:
        assert height % 2 == 0
        moves += [c] * height
    return moves


# One full-board draw per board.  Cell (c, r) ends X where r + [column c began with O] is even: columns alternate, a
# row repeats its columns' bottom colours or their inverse (XXXOOOX, XXXOOO, XXOOXXOO: no four alike), and a
# diagonal changes colour at every step but those where the bottom colour changes, so it holds runs of two at most.
C4_DRAW = _full_board(6, [(0, 3), (1, 4), (2, 5)], lone=[6])
FULL_GAME = {"connect4": C4_DRAW, "connect4_6_5": _full_board(5, [(0, 3), (1, 4), (2, 5)]),
             "connect4_8_7": _full_board(7, [(0, 2), (1, 3), (4, 6), (5, 7)])}
TTT_DRAW = FULL_GAME["tictactoe"] = [4, 0, 2, 6, 3, 5, 7, 1, 8]


def make_env(game):
    from oracle.envs import Connect4Env, TicTacToeEnv

    return TicTacToeEnv() if game == "tictactoe" else Connect4Env(*BOARD_OF[game])


def replay(game, moves):
    """Play a legal move list on the oracle env, the first mover +1.  Returns (boards before every move int8
    [len, W, H], reward of the last move for its mover, done after the last move)."""
    env = make_env(game)
    boards, rew, done = [], 0, False
    for p, a in enumerate(moves):
        boards.append(env.board.astype(np.int8).copy())
        _, rew, done, _ = env.step(int(a), 1 if p % 2 == 0 else -1)
    W, H = BOARD_OF[game]
    return np.array(boards, dtype=np.int8).reshape(len(moves), W, H), int(rew), bool(done)


def result_of(game, moves, swap):
    """The result in side 0's view (tree 2g's) of a finished legal game."""
    _, rew, done = replay(game, moves)
    assert done
    last_side = (len(moves) - 1 + int(swap)) & 1
    return rew * (1 if last_side == 0 else -1)


def random_game(game, rng, length=None):
    """A random legal game: played to its end, or cut after `length` plies if it lasts that long."""
    env = make_env(game)
    moves, done = [], False
    while not done and (length is None or len(moves) < length):
        a = int(rng.choice(np.flatnonzero(env.valid_moves())))
        _, _, done, _ = env.step(a, 1 if len(moves) % 2 == 0 else -1)
        moves.append(a)
    return moves


def long_games(game, rng, n, spare=8):
    """n random legal games that end with at most `spare` empty cells (random play rarely lasts that long on the
    larger boards: most draws are thrown away)."""
    W, H = BOARD_OF[game]
    out = []
    for _ in range(4000):
        m = random_game(game, rng)
        if len(m) >= W * H - spare:
            out.append(m)
            if len(out) == n:
                return out
    raise AssertionError(f"random play gave {len(out)} of {n} long games")


def full_game_prefixes(game):
    """The board's full-board draw cut after 1, 2, ... CELLS plies: a legal game of every length."""
    full = FULL_GAME[game]
    return [full[:n] for n in range(1, len(full) + 1)]


def games_of_every_length(game, rng):
    """Legal games of every length from 1 to CELLS: a random game of each length that random play reaches (cut games
    included), and every prefix of the board's full-board draw, so that no length is missing."""
    W, H = BOARD_OF[game]
    out = full_game_prefixes(game)
    for length in range(1, W * H + 1):
        for _ in range(40):  # a game that random play ends sooner is drawn again
            m = random_game(game, rng, length)
            if len(m) == length:
                out.append(m)
                break
    return out


def pack(game, move_lists):
    W, H = BOARD_OF[game]
    moves = np.zeros((len(move_lists), W * H), dtype=np.uint8)
    for i, m in enumerate(move_lists):
        moves[i, :len(m)] = m
    return moves, np.array([len(m) for m in move_lists], dtype=np.int32)


def expected_positions(game, move_lists, first_ply, bad=()):
    """What log_positions must give for legal move lists (the indices in `bad` excepted: no rows), from replay."""
    W, H = BOARD_OF[game]
    boards, players, rec, ply, offsets = [], [], [], [], []
    for r, m in enumerate(move_lists):
        offsets.append(len(rec))
        if r in bad:
            continue
        b, _, _ = replay(game, m)
        for p in range(first_ply, len(m)):
            boards.append(b[p])
            players.append(1 if p % 2 == 0 else -1)
            rec.append(r)
            ply.append(p)
    offsets.append(len(rec))
    return dict(boards=np.array(boards, dtype=np.int8).reshape(len(rec), W, H), players=np.array(players, dtype=np.int8),
                row_record=np.array(rec, dtype=np.int32), row_ply=np.array(ply, dtype=np.int32),
                offsets=np.array(offsets, dtype=np.int32))


# ----------------------------------------------------------------------------- GPU side
def _drain(arena, records):
    ex = arena.export_games()
    if ex["id"].numel():
        records.append({k: v.cpu().numpy() for k, v in ex.items()})


def _merge(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]} if parts else None


def run_g3_logged(games, log=True, search_threads=1):
    """parity_helpers.run_g3_group's loop with the game log on (or off).  Returns (Move rows, counters, game
    records or None, games_results of the slots)."""
    import torch

    from self_play_reinforcement_learning_amd.arena import Arena

    game, sims, evaluate = games[0]["game"], games[0]["sims"], games[0]["evaluate"]
    G = len(games)
    arena = Arena(game, n_trees=2 * G, n_games=G, iterations=sims, rng="tape", evaluate=evaluate,
                  leaf_format="f32", leaf_layout="nchw", search_threads=search_threads)
    if log:
        arena.games_set_log(True)
    tapes, salts = [], []
    for g in games:
        tp, to, _ = g3_tapes(g, search_threads)
        tapes += [tp, to]
        salts += [g["salt_policy"], g["salt_opponent"]]
    arena.set_tapes(tapes)
    salts_by_tree = torch.tensor(salts, dtype=torch.int64, device=arena.device)
    priors = np.stack([np.stack([empty_prior(game, g["salt_policy"]), empty_prior(game, g["salt_opponent"])])
                       for g in games])
    arena.games_set_limit(G)
    arena.games_start(list(range(G)), priors=priors)
    rows, records = [], []

    def step(count):
        if count:
            p, v = _eval_table(arena, salts_by_tree, count)
            arena.expand(p, v)

    for _ in range(64):
        arena.games_begin_ply()
        for _ in range(-(-sims // search_threads)):
            step(arena.select())
        step(arena.games_end_ply())
        fin, ring = arena.games_finish_ply(refill=False)
        if ring:
            rows.append({k: v.cpu().numpy() for k, v in arena.export_moves(ring).items()})
        if log:
            _drain(arena, records)
        if not (arena.games_state()["state"] == 1).any():
            break
    arena.check()
    counters, results = arena.counters(), arena.games_results()
    arena.close()
    return _merge(rows), counters, _merge(records), results


def run_g5_logged(games, log=True, search_threads=1, opponent_threads=None):
    """parity_helpers.run_g5_group's loop with the game log on (or off).  Returns (Move rows, counters, the
    oracle's episodes, game records or None, games_results of the slots)."""
    import torch

    from self_play_reinforcement_learning_amd import _lib
    from self_play_reinforcement_learning_amd.arena import Arena, table_net_eval

    g0 = games[0]
    game, sims, opp, opp_sims = g0["game"], g0["sims"], g0["opponent"], g0["opponent_sims"]
    G = len(games)
    kind = {"mcts": _lib.PLAYER_MCTS, "lookahead": _lib.PLAYER_LOOKAHEAD, "random": _lib.PLAYER_RANDOM}[opp]
    k0 = search_threads
    k1 = search_threads if opponent_threads is None or opp != "mcts" else opponent_threads
    pkw, okw = g0.get("policy_kwargs") or {}, g0.get("opponent_kwargs") or {}
    arena = Arena(game, n_trees=2 * G, n_games=G, iterations=max(sims, opp_sims), rng="tape", evaluate=True,
                  search_threads=max(k0, k1), strong_play=pkw.get("strong_play", False))
    arena.set_tree_players(nets=[0, 1 if opp == "mcts" else 0] * G, kinds=[_lib.PLAYER_MCTS, kind] * G,
                           budgets=[sims, opp_sims if opp == "mcts" else 0] * G)
    arena.set_tree_search(alpha=[pkw.get("alpha", 1), okw.get("alpha", 1)] * G,
                          strong_play=[pkw.get("strong_play", False), okw.get("strong_play", False)] * G,
                          search_threads=[k0, k1] * G)
    if log:
        arena.games_set_log(True)
    tapes, oracle, salts = [], [], []
    for g in games:
        tp, to, out = g5_tapes(g, search_threads, opponent_threads=k1 if opp == "mcts" else None)
        tapes += [tp, to]
        oracle.append(out)
        salts += [g["salt_policy"], g["salt_opponent"]]
    arena.set_tapes(tapes)
    salts_by_tree = torch.tensor(salts, dtype=torch.int64, device=arena.device)
    priors = np.stack([np.stack([empty_prior(game, g["salt_policy"]), empty_prior(game, g["salt_opponent"])])
                       for g in games])
    arena.games_set_limit(G)
    arena.games_start(list(range(G)), priors=priors)
    rows, records = [], []

    def seg_eval(row0, n, trees_all):
        if n == 0:
            return torch.zeros((1, arena.A), device=arena.device), torch.zeros(1, device=arena.device)
        trees = trees_all[row0:row0 + n].long()
        return table_net_eval(game, arena.leaves_from(row0, n), arena.leaf_format, arena.leaf_layout,
                              salts=salts_by_tree[trees].contiguous())

    def step(count):
        if not count:
            return
        n0, n1 = arena.segment_counts()
        trees_all = arena.leaf_trees(arena.max_rows)
        p0, v0 = seg_eval(0, n0, trees_all)
        p1, v1 = seg_eval(arena.seg1, n1, trees_all)
        arena.expand2(p0, v0, p1, v1)

    for _ in range(64):
        arena.games_begin_ply()
        for _ in range(max(-(-sims // k0), -(-opp_sims // k1))):
            step(arena.select())
        step(arena.games_end_ply())
        fin, ring = arena.games_finish_ply(refill=False)
        if ring:
            rows.append({k: v.cpu().numpy() for k, v in arena.export_moves(ring).items()})
        if log:
            _drain(arena, records)
        if not (arena.games_state()["state"] == 1).any():
            break
    arena.check()
    counters, results = arena.counters(), arena.games_results()
    arena.close()
    return _merge(rows), counters, oracle, _merge(records), results


def check_records(records, results, expected):
    """records (merged export) against `expected`: per slot (moves, result in tree 2g's view, swap); slot = game id
    here (one game per slot, started in slot order)."""
    assert records is not None and len(records["id"]) == len(expected)
    assert sorted(records["id"].tolist()) == list(range(len(expected)))
    for i in range(len(records["id"])):
        g = int(records["id"][i])
        moves, result, swap = expected[g]
        n = int(records["plies"][i])
        assert int(records["slot"][i]) == g
        assert records["moves"][i, :n].tolist() == list(moves), g
        assert not records["moves"][i, n:].any(), g
        assert (n, int(records["result"][i]), int(records["swap"][i])) == (len(moves), result, int(swap)), g
        assert int(records["opening"][i]) == -1
        # the ring's copy of what games_results keeps per slot
        assert (int(results["result"][g]), int(results["swap"][g]), int(results["ply"][g])) == (result, int(swap), n)
