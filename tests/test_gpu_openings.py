"""GPU: opening books in the game kernels (include/spmcts.h spmcts_games_set_openings / spmcts_games_openings),
batched root statistics (spmcts_root_stats_batch), and what is built on them: SelfPlayEngine / LanedEngine /
LeagueEngine(openings=), Elo.compare_models(openings=), analyse_positions, MCTreeSearch.set_position."""
import itertools

import numpy as np
import pytest
import torch

from tests.opening_helpers import BOOK, book_specs, check_book_group, run_book_group
from tests.parity_helpers import load_json

pytestmark = pytest.mark.gpu

# [3, 3] plays an occupied cell in TicTacToe (no legal move there: tests/test_openings.py), so its book takes
# [3, 4] in that place: the same lengths, so the same plies mix book games and searching games
BOOKS = {"connect4": BOOK, "tictactoe": [[], [3], [3, 4], [0, 6, 3]]}


# ----------------------------------------------------------------------------- tape mode, table net, bit-exact
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("game", ["connect4", "tictactoe"])
def test_book_selfplay_matches_oracle(game, K):
    """8 slots, no refill, 16 sims, a book of lengths 0..3: Move records, per-game results and the counters equal
    the forced-opening oracle episodes bit for bit, on tapes that hold no draw for a book ply."""
    specs = book_specs(game, book=BOOKS[game])
    moves, counters, results = run_book_group(specs, BOOKS[game], search_threads=K)
    check_book_group(specs, moves, counters, results, search_threads=K)


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("opponent", ["lookahead", "random"])
@pytest.mark.parametrize("game", ["connect4", "tictactoe"])
def test_book_evaluation_games_match_oracle(game, opponent, K):
    """Evaluate mode against the hard-coded players: a book move replaces the player's own move and leaves its
    RNG stream untouched (its tape holds exactly the draws of its own moves)."""
    specs = book_specs(game, book=BOOKS[game], opponent=opponent)
    moves, counters, results = run_book_group(specs, BOOKS[game], search_threads=K, evaluate=True)
    check_book_group(specs, moves, counters, results, search_threads=K, evaluate=True)


def test_book_period_restarts_the_suite():
    """id_period 4 over a 4-opening book: ids 4..7 play openings 0, 0, 1, 1 again."""
    specs = book_specs("connect4", book=BOOK, period=4)
    assert [g["opening_index"] for g in specs] == [0, 0, 1, 1, 0, 0, 1, 1]
    moves, counters, results = run_book_group(specs, BOOK, search_threads=4, period=4)
    check_book_group(specs, moves, counters, results, search_threads=4)


SAME = ("sims", "nn_leaves", "terminal_leaves", "depth_sum", "set_node_expansions", "moves", "games_finished",
        "positions_exported", "results", "leaked_sims", "nn_rows", "error_flags")


@pytest.mark.parametrize("K", [1, 4])
def test_empty_book_changes_nothing(K):
    """An arena given an empty book, or a book of one empty opening, records the Moves and counters of an arena
    that never made the call."""
    specs = book_specs("connect4", book=None)
    base = run_book_group(specs, None, search_threads=K)
    check_book_group(specs, *base, search_threads=K)
    for book in ([], [[]]):
        moves, counters, results = run_book_group(specs, book, search_threads=K)
        assert results == base[2]
        for k in base[0]:
            np.testing.assert_array_equal(moves[k], base[0][k], err_msg=k)
        for k in SAME:
            assert counters[k] == base[1][k], k


def test_set_openings_refusals():
    """The library's message names opening and ply; an odd period, a book on a tree-only arena and a change while
    games are active are refused; the refused call leaves the book as it was."""
    from self_play_reinforcement_learning_amd._lib import SpmctsError
    from self_play_reinforcement_learning_amd.arena import Arena

    a = Arena("connect4", n_trees=8, n_games=4, iterations=4, leaf_format="f32", leaf_layout="nchw")
    for book, msg in (([[3, 3], [3] * 7], "opening 1 ply 6: illegal move 3"),
                      ([[0, 1, 0, 1, 0, 1, 0]], "opening 0 ply 6: move 0 ends the game"),
                      ([[], [7]], "opening 1 ply 0: illegal move 7")):
        with pytest.raises(SpmctsError) as e:
            a.games_set_openings(book)
        assert str(e.value).endswith("(-3): " + msg)
    with pytest.raises(SpmctsError, match="even"):
        a.games_set_openings(BOOK, id_period=3)
    assert a.games_openings().tolist() == [-1] * 4
    a.games_set_openings(BOOK, id_period=2)
    a.games_set_limit(4)
    a.games_start([0, 1, 2, 3])
    assert a.games_openings().tolist() == [0, 0, 0, 0]  # ids mod 2
    with pytest.raises(SpmctsError, match="active"):
        a.games_set_openings([])
    a.check()
    a.close()
    t = Arena("connect4", n_trees=2, iterations=4, leaf_format="f32", leaf_layout="nchw")
    with pytest.raises(SpmctsError, match="no game slots"):
        t.games_set_openings(BOOK)
    t.close()


# ----------------------------------------------------------------------------- Philox
def _position(game, seq, first):
    """The board after `seq` from the empty board, the first mover's stones as `first`."""
    from self_play_reinforcement_learning_amd.openings import make_env

    env = make_env(game)
    p = first
    for a in seq:
        env.step(a, p)
        p = -p
    return env.board.astype(np.int8)


def test_refill_assigns_openings_by_game_id():
    """4 slots play 12 games of a 3-opening book of length 2 with refill: after every ply each slot's opening is
    (id >> 1) % 3, a game's trees stand at its opening's position after two plies (root_stats_batch), and every
    opening ends with as many swap as non-swap games."""
    from self_play_reinforcement_learning_amd.arena import Arena, table_net_eval

    game, book, sims, K = "connect4", [[3, 3], [0, 6], [2, 4]], 8, 4
    a = Arena(game, n_trees=8, n_games=4, iterations=sims, seed=11, leaf_format="f32", leaf_layout="nchw",
              search_threads=K)
    a.games_set_openings(book)
    a.games_set_limit(12)
    a.games_start([0, 1, 2, 3])
    seen, at_book_end, done = {}, 0, 0

    def step(n):
        if n:
            p, v = table_net_eval(game, a.leaves(n), a.leaf_format, a.leaf_layout)
            a.expand(p, v)

    for _ in range(200):
        st = a.games_state()
        op = a.games_openings()
        for g in range(4):
            if st["state"][g] == 1:
                gid = int(st["game_id"][g])
                assert op[g] == (gid >> 1) % 3, (g, gid)
                assert int(st["swap"][g]) == (gid & 1)
                seen[gid] = (int(op[g]), int(st["swap"][g]))
            else:
                assert op[g] == -1
        slots = [g for g in range(4) if st["state"][g] == 1 and st["ply"][g] == 2]
        if slots:
            rs = a.root_stats_batch([2 * g + s for g in slots for s in (0, 1)])
            boards = rs["board"].cpu().numpy().reshape(len(slots), 2, a.W, a.H)
            players = rs["root_player"].cpu().numpy().reshape(len(slots), 2)
            for i, g in enumerate(slots):
                first = -1 if st["swap"][g] else 1  # tree 2g's sign of the first mover's stones; 2g + 1 the other
                np.testing.assert_array_equal(boards[i, 0], _position(game, book[op[g]], first))
                np.testing.assert_array_equal(boards[i, 1], _position(game, book[op[g]], -first))
                assert players[i].tolist() == [first, -first]  # two plies on, the first mover moves again
            at_book_end += len(slots)
        if not (st["state"] == 1).any():
            break
        a.games_begin_ply()
        for _ in range(-(-sims // K)):
            step(a.select())
        step(a.games_end_ply())
        fin, _ = a.games_finish_ply(refill=True)
        a.export_moves(4096)
        done += fin
    a.check()
    c = a.counters()
    a.close()
    assert done == 12 == c["games_finished"] and at_book_end == 12 and sorted(seen) == list(range(12))
    for o in range(3):
        swaps = [s for op_, s in seen.values() if op_ == o]
        assert len(swaps) == 4 and sum(swaps) == 2
    # two book plies per game: no search, no Move
    assert c["sims"] + c["leaked_sims"] == sims * c["moves"]


def test_laned_engine_book_with_and_without_row_reuse():
    """LanedEngine with a book on a 2-block C = 128 net, 128 games, K = 4: cross-lane dedup and the evaluation
    cache on give the Moves of a run with every reuse off, bit for bit; no Move is a book position."""
    from self_play_reinforcement_learning_amd.engine import LanedEngine
    from self_play_reinforcement_learning_amd.modules import ResidualTower
    from self_play_reinforcement_learning_amd.openings import enumerate_openings

    torch.manual_seed(0)
    net = ResidualTower(3, 3, 9, num_blocks=2, filter_factor=32).cuda().eval()
    book = enumerate_openings("tictactoe", 2)
    out = []
    for kw in (dict(cross_dedup=True, eval_cache=2), dict(cross_dedup=False, eval_cache=0, leaf_dedup=False)):
        eng = LanedEngine("tictactoe", net, n_games=128, lanes=2, iterations=16, seed=7, search_threads=4,
                          max_games=512, openings=book, **kw)
        assert eng.cross_dedup == kw["cross_dedup"] and eng.eval_cache == kw["eval_cache"]
        got = []
        eng.run(plies=10, on_moves=lambda m: got.append({k: v.cpu().numpy() for k, v in m.items()}))
        eng.check()
        out.append(({k: np.concatenate([g[k] for g in got]) for k in got[0]}, eng.counters()))
    (m0, c0), (m1, c1) = out
    assert len(m0["z"]) > 128
    for k in m0:
        np.testing.assert_array_equal(m0[k], m1[k], err_msg=k)
    for k in ("sims", "leaked_sims", "moves", "nn_leaves", "terminal_leaves", "depth_sum", "games_finished", "results"):
        assert c0[k] == c1[k], k
    assert c0["nn_rows"] < c1["nn_rows"] == c1["nn_leaves"]
    assert (np.abs(m0["state"]).sum(axis=1) >= 2).all()  # every recorded position is past its two book plies


def _tower(seed, game="tictactoe", blocks=2, ff=32):
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    torch.manual_seed(seed)
    shape = (7, 6, 7) if game == "connect4" else (3, 3, 9)
    return ResidualTower(*shape, num_blocks=blocks, filter_factor=ff).cuda().eval()


def test_league_walks_the_suite_per_pairing(tmp_path):
    """Two 2-block nets and `random` play all:2 on TicTacToe, 144 games per pairing: every pairing plays each of
    the 72 openings once per side, the per-opening breakdown sums to the totals, the two book plies launch no
    network, and Elo.compare_models(openings=) adds exactly g games per pairing to results.json."""
    from self_play_reinforcement_learning_amd import Elo, ModelDatabase
    from self_play_reinforcement_learning_amd.base_model import ModelContainer
    from self_play_reinforcement_learning_amd.engine import LeagueEngine
    from self_play_reinforcement_learning_amd.envs import TicTacToeEnv
    from self_play_reinforcement_learning_amd.openings import enumerate_openings

    book = enumerate_openings("tictactoe", 2)
    assert len(book) == 72
    players = [dict(network=_tower(0), iterations=8), dict(kind="random"), dict(network=_tower(1), iterations=8)]
    pairings = list(itertools.combinations(range(3), 2))
    lg = LeagueEngine("tictactoe", players, pairings, games_per_pairing=144, seed=4, search_threads=4, openings=book)
    assert lg.g == 144 and lg.book_plies == 2
    lg.ply()
    op = lg.arena.games_openings()
    st = lg.arena.games_state()
    for p in range(3):
        assert op[p * 144:(p + 1) * 144].tolist() == [k // 2 for k in range(144)]  # from the first opening on
        assert st["swap"][p * 144:(p + 1) * 144].tolist() == [0, 1] * 72
    lg.ply()
    # two book plies: no search step and no network launch of one; only each ply's _set_node rows went to the two
    # networks (a searched ply launches select_steps + 1 times per network)
    assert lg.device_count and lg.select_steps == 2
    assert lg.launches == 2 * lg.n_nets and lg.counters()["sims"] == 0
    rs = lg.arena.root_stats_batch([2 * s for s in range(lg.n_slots)])
    boards = rs["board"].cpu().numpy()
    for s in (0, 1, 143, 144, 287):  # pairings 0 and 1: tree 2s is a network's (pairing 2's is `random`: no tree)
        np.testing.assert_array_equal(boards[s], _position("tictactoe", book[(s % 144) >> 1], -1 if s & 1 else 1))
    assert not boards[288:].any()
    out = lg.play()
    assert lg.launches > 0
    r = lg.arena.games_results()
    for p, b in enumerate(out):
        assert sorted(b["openings"]) == list(range(72))
        for side in ("first", "second"):
            assert all(sum(o[side].values()) == 1 for o in b["openings"].values())  # once per side
            for k in ("wins", "draws", "losses"):
                assert sum(o[side][k] for o in b["openings"].values()) == b[side][k]
        assert sum(b["first"].values()) == sum(b["second"].values()) == 72
        assert (r["ply"][p * 144:(p + 1) * 144] >= 5).all()  # no game ended inside its book
    lg.close()

    db = ModelDatabase(tmp_path, TicTacToeEnv)
    db.add_model("random", ModelContainer("Random"))
    for name, seed in (("a", 0), ("b", 1)):
        db.add_model(name, ModelContainer("MCTreeSearch", policy_kwargs=dict(network=_tower(seed), iterations=8)))
    elo = Elo(db, seed=4)
    new = elo.compare_models("a", "random", "b", num_games=144, openings="all:2")
    assert set(new) == {"random__a", "random__b", "b__a"}
    assert all(sum(v.values()) == 144 for v in db.results().values())
    elo.compare_all(num_games=144, openings=book)
    assert all(sum(v.values()) == 288 for v in db.results().values())


# ----------------------------------------------------------------------------- analysis
@pytest.mark.parametrize("game,K", [("connect4", 4), ("tictactoe", 1)])
def test_root_stats_batch_equals_root_stats(game, K):
    """64 trees at different depths, mid-search (after 3 of 8 steps): the batch call returns root_stats(t) of
    every tree bit for bit, in the order asked for, unexpanded roots and repeated ids included."""
    from self_play_reinforcement_learning_amd.arena import Arena, table_net_eval

    T = 64
    a = Arena(game, n_trees=T + 1, iterations=8 * K, seed=5, leaf_format="f32", leaf_layout="nchw", search_threads=K)

    def step(n):
        if n:
            p, v = table_net_eval(game, a.leaves(n), a.leaf_format, a.leaf_layout)
            a.expand(p, v)

    a.tree_reset(list(range(T + 1)), [1 if t % 3 else -1 for t in range(T + 1)])
    seqs = [BOOKS[game][t % 4] for t in range(T)]
    for i in range(3):
        on = [t for t in range(T) if i < len(seqs[t])]
        step(a.play_action(on, [seqs[t][i] for t in on]))
    a.search_begin(list(range(T)))  # tree T stays as reset
    for _ in range(3):
        step(a.select())
    order = list(range(T, -1, -1)) + [5, 5]
    got = {k: v.cpu().numpy() for k, v in a.root_stats_batch(order).items()}
    assert got["child_w"].dtype == np.float64 and got["child_p"].dtype == np.float32
    for i, t in enumerate(order):
        want = a.root_stats(t)
        assert got["child_n"][i].tolist() == want["child_n"], t
        assert got["child_w"][i].tolist() == want["child_w"], t
        assert got["child_p"][i].tolist() == want["child_p"], t
        assert int(got["root_n"][i]) == want["root_n"] and float(got["root_w"][i]) == want["root_w"], t
        assert int(got["root_player"][i]) == want["root_player"], t
        np.testing.assert_array_equal(got["board"][i], want["board"])
    assert got["root_n"][1:T + 1].max() > 0 and got["child_n"][0].sum() == 0
    a.check()
    a.close()


def _g2_positions(game, n=12):
    return [c["opening"] for c in load_json("mcts_search.json") if c["game"] == game][:n]


@pytest.mark.parametrize("game,K", [("connect4", 4), ("tictactoe", 1)])
def test_analyse_positions_equals_arena_calls(game, K):
    """analyse_positions over the G2 fixtures' opening sequences = the same Arena calls made by hand with the
    same seed (reset, play_action per ply, one search, root_stats per tree)."""
    from self_play_reinforcement_learning_amd import DeviceTableNet, analyse_positions
    from self_play_reinforcement_learning_amd.arena import Arena
    from self_play_reinforcement_learning_amd.evaluator import make_evaluator

    seqs = _g2_positions(game)
    assert len(seqs) >= 4 and len({len(s) for s in seqs}) > 1
    sims, seed = 24, 9
    net = DeviceTableNet(game, salt=3)
    out = {k: v.cpu().numpy() for k, v in analyse_positions(game, net, seqs, sims, search_threads=K, seed=seed).items()}
    ev = make_evaluator(net, game, dtype=torch.float16)
    n = len(seqs)
    a = Arena(game, n_trees=n, iterations=sims, seed=seed, leaf_format=ev.leaf_format, leaf_layout=ev.leaf_layout,
              search_threads=K)

    def step(count):
        if count:
            p, v = ev(a.leaves(count))
            a.expand(p, v)

    p0, _ = ev(ev.empty_root_input(a.W, a.H, a.device))
    a.set_root_prior(p0[0])
    a.tree_reset(list(range(n)), [1] * n)
    for i in range(max(len(s) for s in seqs)):
        on = [t for t in range(n) if i < len(seqs[t])]
        step(a.play_action(on, [seqs[t][i] for t in on]))
    a.search_begin(list(range(n)))
    for _ in range(-(-sims // K)):
        step(a.select())
    for t in range(n):
        want = a.root_stats(t)
        assert out["child_n"][t].tolist() == want["child_n"] and sum(want["child_n"]) > 0, t
        assert out["child_w"][t].tolist() == want["child_w"], t
        assert out["child_p"][t].tolist() == want["child_p"], t
        assert int(out["root_n"][t]) == want["root_n"] and float(out["root_w"][t]) == want["root_w"], t
        assert float(out["root_q"][t]) == (want["root_w"] / want["root_n"] if want["root_n"] else 0.0), t
        assert int(out["action"][t]) == int(np.argmax(want["child_n"])), t
        np.testing.assert_array_equal(out["board"][t], want["board"])
        np.testing.assert_array_equal(out["board"][t], _position(game, seqs[t], 1))
    a.check()
    a.close()


def test_set_position_equals_play_action_loop():
    """MCTreeSearch.set_position(moves) = reset + a play_action loop: the same root, then the same search."""
    from self_play_reinforcement_learning_amd import DeviceTableNet, MCTreeSearch
    from self_play_reinforcement_learning_amd.envs import Connect4Env

    seq = [3, 3, 2, 4, 0]
    views = []
    for use in (True, False):
        t = MCTreeSearch(network=DeviceTableNet("connect4", salt=1), env=Connect4Env, iterations=20, seed=13)
        if use:
            board = t.set_position(seq, player=-1)
            np.testing.assert_array_equal(board, _position("connect4", seq, -1))
        else:
            t.reset(-1)
            for a in seq:
                t.play_action(a)
        before = t.root_node
        action = t()
        t.play_action(action)
        views.append((before, action, t.root_node))
    (b0, a0, r0), (b1, a1, r1) = views
    assert a0 == a1
    for x, y in ((b0, b1), (r0, r1)):
        assert (x.n, x.w, x.player) == (y.n, y.w, y.player)
        np.testing.assert_array_equal(x.state, y.state)
        assert [(c.n, c.w, c.p) for c in x.children] == [(c.n, c.w, c.p) for c in y.children]
    with pytest.raises(ValueError, match="opening 0 ply 6"):
        t.set_position([3] * 7)


# ----------------------------------------------------------------------------- the engine keyword, the scheduler, the CLI
def test_selfplay_engine_openings_and_period():
    """SelfPlayEngine(openings=, opening_period=) called directly: 6 slots, 18 games, a 3-opening book with id
    period 4, so only openings 0 and 1 are ever played; every slot follows ((id % 4) >> 1) % 3 through the
    refills, and no Move holds a position from inside its game's book."""
    from self_play_reinforcement_learning_amd import DeviceTableNet
    from self_play_reinforcement_learning_amd.engine import SelfPlayEngine

    book = [[3, 3, 2], [0], [6, 6]]
    eng = SelfPlayEngine("connect4", DeviceTableNet("connect4", salt=2), n_games=6, iterations=8, seed=3,
                         max_games=18, search_threads=4, openings=book, opening_period=4)
    assert eng.openings == book
    seen, got = {}, []

    def on_ply(e):
        st, op = e.arena.games_state(), e.arena.games_openings()
        for g in range(6):
            if st["state"][g] == 1:
                gid = int(st["game_id"][g])
                assert op[g] == ((gid % 4) >> 1) % 3, (g, gid)
                seen[gid] = int(op[g])

    eng.start()
    on_ply(eng)
    while eng.games_done < 18:
        eng.ply(on_moves=lambda m: got.append({k: v.cpu().numpy() for k, v in m.items()}))
        on_ply(eng)
    eng.check()
    assert sorted(seen) == list(range(18)) and set(seen.values()) == {0, 1}
    moves = {k: np.concatenate([g[k] for g in got]) for k in got[0]}
    stones = np.abs(moves["state"]).sum(axis=1)
    for gid, o in seen.items():
        assert (stones[moves["game"] == gid] >= len(book[o])).all(), gid
    c = eng.counters()
    assert c["sims"] + c["leaked_sims"] == 8 * c["moves"] and c["moves"] == len(stones)
    eng.arena.close()


def test_scheduler_compare_models_openings(tmp_path, monkeypatch):
    """SelfPlayScheduler.compare_models(openings=): the book reaches the evaluation engine (a second network, and a
    hard-coded player), game i of the comparison plays opening (i >> 1) % n, and the totals still cover
    epoch_length games."""
    from self_play_reinforcement_learning_amd import (MCTreeSearch, ModelContainer, OneStepLookahead,
                                                      SelfPlayScheduler, TicTacToeEnv)

    a, b = _tower(0), _tower(1)
    for ev, spec in ((ModelContainer(policy_gen=MCTreeSearch, policy_kwargs=dict(iterations=6, env=TicTacToeEnv)), "all:1"),
                     (ModelContainer(policy_gen=OneStepLookahead, policy_kwargs=dict(env=TicTacToeEnv)), [[4], [0, 8]])):
        container = ModelContainer(policy_gen=MCTreeSearch, policy_kwargs=dict(iterations=8, env=TicTacToeEnv))
        sp = SelfPlayScheduler(policy_container=container, env=TicTacToeEnv, network=a, evaluation_policy_container=ev,
                               evaluation_network=b, epoch_length=36, save_dir=str(tmp_path), n_games=12)
        book = [[k] for k in range(9)] if spec == "all:1" else spec
        seen, engines = {}, []
        make = sp._evaluation_engine

        def recording(n_games, openings=None, make=make, seen=seen, engines=engines):
            eng, per_rank = make(n_games, openings)
            engines.append(eng)
            play = eng.play_games

            def on_ply(e):
                st, op = e.arena.games_state(), e.arena.games_openings()
                for g in np.flatnonzero(st["state"] == 1):
                    seen[int(st["game_id"][g])] = int(op[g])

            eng.play_games = lambda n: play(n, on_ply=on_ply)  # a game stays active for five plies at least
            return eng, per_rank

        monkeypatch.setattr(sp, "_evaluation_engine", recording)
        total, breakdown = sp.compare_models(openings=spec)
        assert engines[0].openings == book
        assert sum(breakdown[s][k] for s in ("first", "second") for k in ("wins", "draws", "losses")) == 36
        assert sum(breakdown["first"].values()) == 18
        assert sorted(seen) == list(range(36))
        assert all(o == (gid >> 1) % len(book) for gid, o in seen.items())


def test_elo_cli_openings_flag(tmp_path, monkeypatch, capsys):
    """python -m ....elo compare_models --openings all:2: the flag reaches the league engine as the parsed suite
    and results.json gains exactly g games per pairing."""
    import json

    from self_play_reinforcement_learning_amd import ModelDatabase, elo, engine
    from self_play_reinforcement_learning_amd.base_model import ModelContainer
    from self_play_reinforcement_learning_amd.envs import TicTacToeEnv
    from self_play_reinforcement_learning_amd.openings import enumerate_openings

    db = ModelDatabase(tmp_path, TicTacToeEnv)
    db.add_model("random", ModelContainer("Random"))
    db.add_model("a", ModelContainer("MCTreeSearch", policy_kwargs=dict(network=_tower(0), iterations=8)))
    given = []

    class Recording(engine.LeagueEngine):
        def __init__(self, *args, **kw):
            given.append(kw.get("openings"))
            super().__init__(*args, **kw)

    monkeypatch.setattr(engine, "LeagueEngine", Recording)
    elo.main(["compare_models", "--dir", str(tmp_path), "--g", "tictactoe", "--games", "144", "--openings", "all:2"])
    assert given == [enumerate_openings("tictactoe", 2)]
    printed = json.loads(capsys.readouterr().out)
    assert printed == db.results() and sum(printed["random__a"].values()) == 144
    elo.main(["compare_models", "--dir", str(tmp_path), "--g", "tictactoe", "--games", "4", "--p", "a", "random"])
    assert given[1] is None and sum(db.results()["random__a"].values()) == 148
