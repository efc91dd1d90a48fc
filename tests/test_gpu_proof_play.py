"""GPU: proof-guided play -- k_proof_verdict and k_proof_stop (csrc/arena_proof.h).  The verdict against the host
twin tree.proof_move_set applied to Arena.bounds_batch, element for element; whole games with the feature on and
off; the moves it plays against the exact solver; per-player switching in a league; the early stop; argument
handling.  Every network is the table net."""
import numpy as np
import pytest
import torch

from self_play_reinforcement_learning_amd import _lib
from self_play_reinforcement_learning_amd.arena import Arena, _stream, table_net_eval
from self_play_reinforcement_learning_amd.tree import proof_move_set
from tests.bounds_helpers import code_to_value, late_positions
from tests.parity_helpers import load_json
from tests.tree_helpers import G3Run
from tests.variant_helpers import variant_oracle  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::DeprecationWarning")]

ALL = 0xffffffff


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    _lib.lib()


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _mask(keep):
    """Arena's int32 keep words as unsigned masks (int64)."""
    return np.asarray(keep).astype(np.int64) & ALL


def _legal(b):
    """The legal moves of bounds_batch rows as masks."""
    ok = (b["move_lo"] != -128).astype(np.int64)
    return (ok << np.arange(ok.shape[1], dtype=np.int64)).sum(axis=1)


def _check_twin(arena, ids, what):
    """proof_moves_batch of the listed trees equals the twin on bounds_batch's rows; returns (masks, bounds)."""
    got, b = _host(arena.proof_moves_batch(ids)), _host(arena.bounds_batch(ids))
    assert got["keep"].dtype == np.int32 and got["lo"].dtype == np.int8 and got["hi"].dtype == np.int8
    want = proof_move_set(b["lo"], b["hi"], b["move_lo"], b["move_hi"])
    keep = _mask(got["keep"])
    assert keep.tolist() == np.asarray(want).tolist(), what
    assert got["lo"].tolist() == b["lo"].tolist() and got["hi"].tolist() == b["hi"].tolist(), what
    legal = _legal(b)
    assert ((keep & ~legal) == 0).all() and (keep != 0).all(), what
    return keep, b


class Searched:
    """A tree-mode arena of one tree per position (move lists from the empty board), table net `salt`, Philox: the
    trees taken to their positions by play_action.  search() runs the simulations and leaves the arena before
    search_end."""

    def __init__(self, game, seqs, sims, K, seed=5, salt=3, blocks_per_tree=0):
        self.game, self.seqs, self.sims, self.salt = game, seqs, sims, salt
        n = len(seqs)
        self.ids = list(range(n))
        self.arena = a = Arena(game, n_trees=n, iterations=sims, rng="philox", seed=seed, leaf_format="f32",
                               leaf_layout="nchw", search_threads=K, blocks_per_tree=blocks_per_tree)
        a.tree_reset(self.ids, [1] * n)
        for i in range(max(len(s) for s in seqs)):
            on = [t for t in self.ids if i < len(seqs[t])]
            self.step(a.play_action(on, [seqs[t][i] for t in on]))

    def step(self, count):
        if count:
            a = self.arena
            p, v = table_net_eval(self.game, a.leaves(count), a.leaf_format, a.leaf_layout, salt=self.salt)
            a.expand(p, v)

    def search(self, between=None):
        a = self.arena
        a.search_begin(self.ids)
        for s in range(-(-self.sims // a.search_threads)):
            self.step(a.select())
            if between is not None:
                between(s)


# board -> empty cells of the positions: late enough for 60 simulations to prove something
MID = {"tictactoe": 5, "connect4": 12, "connect4_6_5": 10}


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("game", ["tictactoe", "connect4", "connect4_6_5"])
def test_verdict_equals_the_twin(request, game, K):
    """13 trees (A = 9 / P = 16: four groups a block, A = 7 and 6 / P = 8: eight; a partial last block either way),
    60 simulations, sequential and four in flight: before the search, between two simulation steps and after it the
    verdict is the twin's on every tree."""
    if game == "connect4_6_5":
        request.getfixturevalue("variant_oracle")
    seqs = late_positions(game, 13, MID[game], seed=3)
    run = Searched(game, seqs, 60, K)
    a = run.arena
    _check_twin(a, run.ids, (game, K, "before"))
    run.search(lambda s: _check_twin(a, run.ids, (game, K, "step", s)) if s in (0, 3) else None)
    keep, b = _check_twin(a, run.ids, (game, K, "after"))
    if game == "tictactoe":  # 5 empty cells, 60 simulations: most trees have proved their position
        assert (b["lo"] == b["hi"]).any() and (keep != _legal(b)).any()
    order = [12, 0, 7, 7, 3]  # a shuffled list with a repeat: row i is tree order[i]
    part = _mask(_host(a.proof_moves_batch(order))["keep"])
    assert part.tolist() == [int(keep[t]) for t in order]
    a.check()
    a.close()


def _g3_games(game, n):
    games = [g for g in load_json("selfplay_games.json") if g["game"] == game and g["sims"] == 25
             and not g["evaluate"]][:n]
    assert len(games) == n
    return games


def _g3_ply(run, ids, reads):
    """tests/tree_helpers.py G3Run.ply, reading the verdict of every tree after the first simulation step and after
    the ply when `reads` (checked against the twin there)."""
    a = run.arena
    a.games_begin_ply()
    for s in range(-(-run.sims // run.K)):
        run._step(a.select())
        if reads and s == 0:
            _check_twin(a, ids, "mid-ply")
    run._step(a.games_end_ply())
    _, ring = a.games_finish_ply(refill=False)
    if ring:
        run.records.append({k: v.cpu().numpy() for k, v in a.export_moves(ring).items()})
    if reads:
        _check_twin(a, ids, "after the ply")
    return bool((a.games_state()["state"] == 1).any())


def test_reading_the_verdict_mid_ply_changes_nothing():
    """A G3 TicTacToe group (tape mode) to the end twice, K = 4, once reading every tree's verdict between two
    simulation steps of every search and between the plies, each read equal to the twin: Move records, results and
    counters are bit-identical."""
    games = _g3_games("tictactoe", 8)
    outs = []
    for reads in (False, True):
        run = G3Run(games, K=4, blocks_per_tree=3 * 25 + 16)
        ids = list(range(2 * len(games)))
        for _ in range(16):
            more = _g3_ply(run, ids, reads)
            if not more:
                break
        assert not more
        run.arena.check()
        res = run.arena.games_results()
        outs.append((run.merged(), run.arena.counters(), {k: np.asarray(v).tolist() for k, v in res.items()}))
        run.arena.close()
    (m0, c0, r0), (m1, c1, r1) = outs
    assert c0 == c1 and r0 == r1 and c0["games_finished"] == len(games)
    assert sorted(m0) == sorted(m1)
    for k in m0:
        assert m0[k].tobytes() == m1[k].tobytes(), k


def test_a_compacted_arena():
    """6 plies of the G3 Connect4 games in a store small enough to be compacted (moved roots, renumbered blocks)."""
    games = _g3_games("connect4", 8)
    run = G3Run(games, blocks_per_tree=2 * 25 + 8)
    for _ in range(6):
        assert run.ply()
    assert run.arena.counters()["compactions"] > 0
    _check_twin(run.arena, list(range(2 * len(games))), "compacted")
    run.arena.check()
    run.arena.close()


# ----------------------------------------------------------------------------- whole games, on and off
class Games:
    """G Connect4 6x5 self-play games in one arena (table net, Philox, K sims in flight, no refill), a ply at a time,
    with the game log on.  Per ply it keeps, for every active game: its mover tree, that tree's bounds and visit
    counts just before the move, and (proof play on) the verdict the move was chosen with."""

    def __init__(self, game, G, sims, K, seed, proof, salt=2):
        self.game, self.G, self.sims, self.K, self.salt, self.proof = game, G, sims, K, salt, proof
        self.arena = a = Arena(game, n_trees=2 * G, n_games=G, iterations=sims, rng="philox", seed=seed,
                               leaf_format="f32", leaf_layout="nchw", search_threads=K)
        if proof:
            a.set_proof_play(True)
        a.games_set_log(True)
        a.games_set_limit(G)
        a.games_start(list(range(G)))
        self.plies, self.moves, self.finished = [], [], {}
        self._merged, self._rows = None, {}  # rows(): valid once every game has finished

    def _step(self, count):
        if count:
            a = self.arena
            p, v = table_net_eval(self.game, a.leaves(count), a.leaf_format, a.leaf_layout, salt=self.salt)
            a.expand(p, v)

    def ply(self):
        a = self.arena
        st = a.games_state()
        on = [g for g in range(self.G) if st["state"][g] == 1]
        movers = [2 * g + ((int(st["ply"][g]) + int(st["swap"][g])) & 1) for g in on]
        a.games_begin_ply()
        for _ in range(-(-self.sims // self.K)):
            self._step(a.select())
        b, rs = _host(a.bounds_batch(movers)), _host(a.root_stats_batch(movers))
        self._step(a.games_end_ply())
        rec = dict(games=on, movers=movers, ply=[int(st["ply"][g]) for g in on], bounds=b, child_n=rs["child_n"])
        if self.proof:
            last = _host(a.proof_last())
            rec.update(keep=_mask(last["keep"][movers]), lo=last["lo"][movers], hi=last["hi"][movers])
        self.plies.append(rec)
        _, ring = a.games_finish_ply(refill=False)
        if ring:
            self.moves.append(_host(a.export_moves(ring)))
        ex = _host(a.export_games())
        for k in range(len(ex["id"])):
            self.finished[int(ex["slot"][k])] = dict(id=int(ex["id"][k]), swap=int(ex["swap"][k]),
                                                     moves=ex["moves"][k, :int(ex["plies"][k])].tolist())
        return bool((a.games_state()["state"] == 1).any())

    def play(self):
        while self.ply():
            assert len(self.plies) <= self.arena.cells
        self.arena.check()
        return self

    def rows(self, slot):
        """The Move rows of the slot's game by ply: {ply: (state, tree_probs, q)}; a game's rows come side 0 first,
        each side's in ply order."""
        if slot in self._rows:
            return self._rows[slot]
        g = self.finished[slot]
        if self._merged is None:
            self._merged = {k: np.concatenate([r[k] for r in self.moves]) for k in self.moves[0]}
        m = self._merged
        idx = np.flatnonzero(m["game"] == g["id"])
        n = len(g["moves"])
        order = [p for side in (0, 1) for p in range(n) if (p + g["swap"]) % 2 == side]
        assert len(idx) == n
        self._rows[slot] = {p: (m["state"][i].tobytes(), m["tree_probs"][i], m["q"][i].tobytes())
                            for p, i in zip(order, idx)}
        return self._rows[slot]


def test_games_with_the_proof_on_and_off():
    """20 games, K = 4, 50 simulations, the same seed with proof play off and on.  Every action is in the verdict's
    keep set, the verdict is the twin's on the bounds read just before the move, and a game's actions and Move rows
    are those of the off run up to its first ply whose keep set is not the legal set.  Every recorded distribution is
    zero outside the keep set, sums to 1 and is the renormalised visit distribution over it (float64 from the visit
    counts, to 1e-6: float32 values of at most 1)."""
    game, G = "connect4_6_5", 20
    off, on = Games(game, G, 50, 4, 11, False).play(), Games(game, G, 50, 4, 11, True).play()
    assert len(on.finished) == len(off.finished) == G
    A = on.arena.A
    first = {}  # slot -> its game's first restricted ply
    for rec in on.plies:
        want = np.asarray(proof_move_set(rec["bounds"]["lo"], rec["bounds"]["hi"], rec["bounds"]["move_lo"],
                                         rec["bounds"]["move_hi"]))
        assert rec["keep"].tolist() == want.tolist()
        assert rec["lo"].tolist() == rec["bounds"]["lo"].tolist() and rec["hi"].tolist() == rec["bounds"]["hi"].tolist()
        legal = _legal(rec["bounds"])
        for k, g in enumerate(rec["games"]):
            p, keep = rec["ply"][k], int(rec["keep"][k])
            action = on.finished[g]["moves"][p]
            assert (keep >> action) & 1, (g, p, action, keep)
            if keep != int(legal[k]):
                first.setdefault(g, p)
            probs = on.rows(g)[p][1]
            sel = np.array([(keep >> a) & 1 for a in range(A)], dtype=np.float64)
            w = rec["child_n"][k].astype(np.float64) * sel
            w = sel if w.sum() == 0 else w
            assert probs.dtype == np.float32 and (probs[sel == 0] == 0).all(), (g, p)
            assert abs(float(probs.astype(np.float64).sum()) - 1) <= 1e-6
            assert np.abs(probs.astype(np.float64) - w / w.sum()).max() <= 1e-6, (g, p)
    assert len(first) >= G // 2  # most games reach a ply at which the proof rules a move out
    changed = 0
    for g in range(G):
        d = first.get(g, len(on.finished[g]["moves"]))
        mon, moff = on.finished[g]["moves"], off.finished[g]["moves"]
        assert mon[:d] == moff[:d], g
        ron, roff = on.rows(g), off.rows(g)
        for p in range(d):
            assert ron[p][0] == roff[p][0] and ron[p][1].tobytes() == roff[p][1].tobytes() and ron[p][2] == roff[p][2]
        changed += mon != moff
    assert changed > 0
    stats = on.arena.proof_stats()
    n_plies = sum(len(r["games"]) for r in on.plies)
    assert stats["plies"] == n_plies == on.arena.counters()["moves"]
    assert stats["restricted"] == sum(int((r["keep"] != _legal(r["bounds"])).sum()) for r in on.plies)
    assert stats["solved"] == sum(int((r["lo"] == r["hi"]).sum()) for r in on.plies)
    assert stats["secured_win"] == sum(int((r["lo"] > 0).sum()) for r in on.plies)
    assert stats["trees_stopped"] == 0 == stats["sims_skipped"]
    assert off.arena.proof_stats() == dict.fromkeys(Arena.PROOF_STATS, 0)
    with pytest.raises(_lib.SpmctsError):
        off.arena.proof_last()
    on.arena.close()
    off.arena.close()


# ----------------------------------------------------------------------------- the moves played, against the solver
# (game, empty cells, simulations, positions): at most 10 empty cells (tests/test_proof_play.py LATE's kind)
EXACT = [("tictactoe", 6, 50, 24), ("tictactoe", 4, 200, 12), ("connect4", 10, 60, 48), ("connect4", 8, 100, 48),
         ("connect4", 6, 200, 24)]


def test_the_move_played_is_exact_where_the_tree_has_proved_it():
    """Searches at late positions ended by search_end with proof play on, and the same searches (same seed) ended
    with it off.  Where lo > 0 the move played has an exact score >= lo; where lo == hi it has the root's exact
    score (solve_to_end).  The floors of tests/test_proof_play.py hold, and in at least one case the off run's move
    has an exact score below lo: the feature changed a real mistake."""
    from self_play_reinforcement_learning_amd import solve_to_end

    wins = losses = cut = fixed = 0
    for game, empty, sims, count in EXACT:
        seqs = late_positions(game, count, empty, seed=empty + 1)
        exact = solve_to_end(game, positions=seqs)
        assert bool(exact["solved"].all())
        codes = exact["score"].cpu().numpy()
        played = {}
        for proof in (False, True):
            run = Searched(game, seqs, sims, 4, seed=17)
            a = run.arena
            if proof:
                a.set_proof_play(True)
            run.search()
            keep, b = _check_twin(a, run.ids, (game, empty))
            out = _host(a.search_end(1.0))
            if proof:
                last = _host(a.proof_last())
                assert _mask(last["keep"]).tolist() == keep.tolist() and last["lo"].tolist() == b["lo"].tolist()
                outside = ((keep[:, None] >> np.arange(a.A)) & 1) == 0
                assert (out["tree_probs"][outside] == 0).all() and out["recorded"].all()
            a.check()
            played[proof] = (out["action"].tolist(), keep, b)
            a.close()
        (act_off, keep_off, b_off), (act_on, keep_on, b) = played[False], played[True]
        assert keep_off.tolist() == keep_on.tolist()  # the same searches
        legal = _legal(b)
        for i in range(len(seqs)):
            lo, hi, a_on, a_off = int(b["lo"][i]), int(b["hi"][i]), act_on[i], act_off[i]
            assert (int(keep_on[i]) >> a_on) & 1 and codes[i, a_on] != -128, (game, seqs[i])
            value = [code_to_value(c, empty) if c != -128 else None for c in codes[i]]
            root = max(v for v in value if v is not None)
            if lo > 0:
                assert value[a_on] >= lo, (game, seqs[i], a_on, value, lo)
            if lo == hi:
                assert lo == root and value[a_on] == root, (game, seqs[i], a_on, value, lo)
            wins += lo > 0
            losses += lo == hi and lo < 0
            cut += lo != hi and int(keep_on[i]) != int(legal[i])
            fixed += (lo > 0 or lo == hi) and value[a_off] < lo
    assert wins >= 8 and losses >= 4 and cut >= 4 and fixed >= 1, (wins, losses, cut, fixed)


def test_single_tree_search_and_analyse_positions():
    from self_play_reinforcement_learning_amd import DeviceTableNet, MCTreeSearch, analyse_positions
    from self_play_reinforcement_learning_amd.envs import TicTacToeEnv

    net = DeviceTableNet("tictactoe", salt=1)
    for proof in (False, True):
        mc = MCTreeSearch(network=net, env=TicTacToeEnv, iterations=200, seed=3, threading=True, thread_count=4,
                          proof_play=proof)
        mc.set_position([4, 0, 8, 2])  # +1 to move, 5 empty cells; -1 threatens 1 (0-1-2)
        mc.search()
        got, sb = mc.proof_moves(), mc.score_bounds()
        assert got["mask"] == proof_move_set(sb["lo"], sb["hi"], sb["move_lo"], sb["move_hi"])
        assert got["keep"] == [a for a in range(9) if (got["mask"] >> a) & 1] and (got["lo"], got["hi"]) == (sb["lo"], sb["hi"])
        action = mc._play(1)
        if proof:
            assert action in got["keep"]
            assert all(p == 0 for a, p in enumerate(mc.temp_memory[-1].tree_probs.tolist()) if a not in got["keep"])
    seqs = late_positions("tictactoe", 6, 5, seed=2)
    out = _host(analyse_positions("tictactoe", net, seqs, 60, search_threads=4, seed=9, bounds=True))
    want = proof_move_set(out["bound_lo"], out["bound_hi"], out["move_lo"], out["move_hi"])
    assert _mask(out["keep"]).tolist() == np.asarray(want).tolist()


# ----------------------------------------------------------------------------- league: per player
def test_league_switches_it_per_player():
    """One table net against itself, proof play on for the second player only, and a random and a negamax player
    that carry the key too: the stats count the plies of the one MCTS player's trees, the verdict rows of every other
    tree stay "no restriction", and the hard-coded players' games are those of a league without the key."""
    from self_play_reinforcement_learning_amd import DeviceTableNet
    from self_play_reinforcement_learning_amd.engine import LeagueEngine

    net = DeviceTableNet("connect4_6_5", salt=1)

    def league(proof):
        players = [dict(network=net, iterations=30, name="plain"),
                   dict(network=net, iterations=30, name="proof", proof_play=proof),
                   dict(kind="random", proof_play=proof), dict(kind="negamax", depth=2, proof_play=proof)]
        eng = LeagueEngine("connect4_6_5", players, [(0, 1), (2, 3)], games_per_pairing=6, seed=4, search_threads=4,
                           record_games=True)
        seen = []
        eng.start()
        while eng.games_done < eng.n_slots:
            st = eng.arena.games_state()
            movers = {2 * g + ((int(st["ply"][g]) + int(st["swap"][g])) & 1) for g in range(12) if st["state"][g] == 1}
            eng.ply()
            if proof:
                keep = _mask(_host(eng.arena.proof_last())["keep"])
                on_trees = [t for t in range(24) if t < 12 and t % 2 == 1]  # pairing (0, 1): slots 0..5, its second player
                assert all(keep[t] == ALL for t in range(24) if t not in on_trees)
                assert all(keep[t] != ALL for t in movers if t in on_trees)
                seen.append(len([t for t in movers if t in on_trees]))
        eng.check()
        r = eng.game_records()
        games = sorted((int(r.pairing[i]), int(r.ids[i]), tuple(r.moves_of(i))) for i in range(len(r.ids)))
        stats = eng.arena.proof_stats()
        eng.close()
        return games, stats, sum(seen)

    g_on, s_on, plies = league(True)
    g_off, s_off, _ = league(False)
    assert s_off == dict.fromkeys(Arena.PROOF_STATS, 0)
    assert s_on["plies"] == plies > 0
    assert [g for g in g_on if g[0] == 1] == [g for g in g_off if g[0] == 1]  # random against negamax: unaffected


# ----------------------------------------------------------------------------- early stop
@pytest.mark.parametrize("cap", [None, 8])
def test_a_solved_tree_stops_searching(cap):
    """32 Connect4 games from 16 late openings (12 empty cells), K = 4, 200 simulations, proof_stop every 4th
    simulation step, with the default sim cap and with the smallest (2 K): check() is clean, trees were stopped, sims
    + leaked_sims + sims_skipped == searches x iterations, every stopped tree's verdict at the end of its ply has
    lo == hi, and its move has the root's exact score (solve_to_end)."""
    from self_play_reinforcement_learning_amd import DeviceTableNet, solve_to_end
    from self_play_reinforcement_learning_amd.engine import SelfPlayEngine

    book = late_positions("connect4", 16, 12, seed=21)
    eng = SelfPlayEngine("connect4", DeviceTableNet("connect4", salt=2), n_games=32, iterations=200, seed=6,
                         max_games=32, search_threads=4, openings=book, record_games=True, proof_play=True,
                         proof_stop_every=4)
    a = eng.arena
    if cap is not None:
        a.set_sim_cap(cap)
    eng.start()
    stopped = []  # (game id, ply) of every search that was stopped
    before = a.proof_stopped().cpu().numpy()
    while eng.games_done < 32:
        st = a.games_state()
        eng.ply()
        now, last = a.proof_stopped().cpu().numpy(), _host(a.proof_last())
        for t in np.flatnonzero(now != before):
            g = int(t) // 2
            assert now[t] == before[t] + 1 and st["state"][g] == 1
            assert t == 2 * g + ((int(st["ply"][g]) + int(st["swap"][g])) & 1)  # the game's mover
            assert last["lo"][t] == last["hi"][t] != -128, (g, t)
            stopped.append((int(st["game_id"][g]), int(st["ply"][g])))
        before = now
    eng.check()
    c, stats = eng.counters(), a.proof_stats()
    assert stats["trees_stopped"] == len(stopped) > 0 and stats["sims_skipped"] > 0
    assert c["sims"] + c["leaked_sims"] + stats["sims_skipped"] == c["moves"] * 200
    assert stats["plies"] == c["moves"]
    r = eng.game_records()
    moves_of = {int(r.ids[i]): r.moves_of(i) for i in range(len(r.ids))}
    seqs = [moves_of[g][:p] for g, p in stopped]
    codes = solve_to_end("connect4", positions=seqs)["score"].cpu().numpy()
    for k, (g, p) in enumerate(stopped):
        action = moves_of[g][p]
        e = 42 - p
        values = [code_to_value(x, e) for x in codes[k] if x != -128]
        assert codes[k, action] != -128 and code_to_value(codes[k, action], e) == max(values), (g, p, action)
    a.close()


def test_proof_stop_refusals():
    from self_play_reinforcement_learning_amd import DeviceTableNet
    from self_play_reinforcement_learning_amd.engine import LeagueEngine, SelfPlayEngine

    L = _lib.lib()
    a1 = Arena("tictactoe", n_trees=2, iterations=8, search_threads=1)
    a1.set_proof_play(True)
    assert L.spmcts_proof_stop(a1.h, None) == -4  # a sequential arena
    with pytest.raises(_lib.SpmctsError):
        a1.proof_stop()
    a1.close()
    a4 = Arena("tictactoe", n_trees=2, iterations=8, search_threads=4)
    assert L.spmcts_proof_stop(a4.h, None) == -4  # proof play is off
    a4.set_proof_play([True, False])
    assert L.spmcts_proof_stop(a4.h, None) == 0  # nothing is searching: nothing stops
    a4.check()
    assert a4.proof_stats()["trees_stopped"] == 0
    a4.close()
    net = DeviceTableNet("tictactoe", salt=1)
    with pytest.raises(ValueError, match="proof_play"):
        SelfPlayEngine("tictactoe", net, n_games=2, iterations=8, search_threads=4, proof_stop_every=2)
    with pytest.raises(ValueError, match="search_threads"):
        SelfPlayEngine("tictactoe", net, n_games=2, iterations=8, search_threads=1, proof_play=True, proof_stop_every=2)
    with pytest.raises(ValueError, match="proof_play"):
        LeagueEngine("tictactoe", [dict(network=net), dict(kind="random")], [(0, 1)], games_per_pairing=2,
                     proof_stop_every=2)


# ----------------------------------------------------------------------------- argument handling
def _raw(arena, trees, fill, skip=None):
    """spmcts_tree_proof_moves_batch into sentinel-filled buffers of the caller; output `skip` is passed as NULL."""
    n, dev = len(trees), arena.device
    t = arena._dev_i32(trees)
    o = dict(keep=torch.full((n,), fill, dtype=torch.int32, device=dev),
             lo=torch.full((n,), fill, dtype=torch.int8, device=dev), hi=torch.full((n,), fill, dtype=torch.int8, device=dev))
    _lib.call("spmcts_tree_proof_moves_batch", arena.h, _lib.ptr(t), n,
              *[None if k == skip else _lib.ptr(o[k]) for k in ("keep", "lo", "hi")], _stream())
    torch.cuda.current_stream().synchronize()
    return _host(o)


def test_argument_handling():
    """Every output may be NULL in turn; n = 0 launches nothing; a tree id of -1 or T raises SPMCTS_ERR_STATE, leaves
    its row's sentinels untouched and every other row right; proof_last is refused while the feature is off."""
    run = Searched("connect4", late_positions("connect4", 6, 10, seed=5), 40, 4)
    a, T, fill = run.arena, 6, 77
    run.search()
    keep, b = _check_twin(a, run.ids, "args")
    order = [int(x) for x in np.random.default_rng(7).integers(0, T, 37)]
    full = _raw(a, order, fill)
    assert _mask(full["keep"]).tolist() == [int(keep[t]) for t in order]
    for skip in ("keep", "lo", "hi"):
        part = _raw(a, order, fill, skip)
        for k in ("keep", "lo", "hi"):
            assert (part[k] == fill).all() if k == skip else part[k].tobytes() == full[k].tobytes(), (skip, k)
    e0 = a.proof_moves_batch([])
    assert e0["keep"].shape == (0,) and e0["lo"].shape == (0,)
    L = _lib.lib()
    assert L.spmcts_tree_proof_moves_batch(a.h, None, 3, None, None, None, None) == -1
    assert L.spmcts_tree_proof_moves_batch(a.h, None, -1, None, None, None, None) == -3
    assert L.spmcts_proof_last(a.h, None, None, None, None) == -4
    a.check()
    bad = [0, -1, 3, T, 5]
    out = _raw(a, bad, fill)
    with pytest.raises(_lib.SpmctsError, match="inconsistent tree state"):
        a.check()
    for i, t in enumerate(bad):
        if 0 <= t < T:
            assert int(_mask(out["keep"][i])) == int(keep[t]) and out["lo"][i] == b["lo"][t] and out["hi"][i] == b["hi"][t]
        else:
            assert all(out[k][i] == fill for k in ("keep", "lo", "hi")), i
    a.close()
