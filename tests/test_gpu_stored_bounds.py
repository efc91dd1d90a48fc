"""GPU: score bounds kept in the nodes (Arena.set_stored_bounds; csrc/arena_solver.h and the SB = true kernels).
The invariant -- every stored entry of every block reachable from the active root equals the host recursion on the
tree as it stands (TreeView.node_bounds on the device's own full export), and the root's entries equal the
independent walk of bounds_batch -- after a search, between two simulation steps, mid-game, after a compaction and
with the smallest sim cap; that keeping them changes nothing the search computes; the proof kernels on the stored
block against the walk; refusals.  Every network is the table net."""
import pytest
import torch

from self_play_reinforcement_learning_amd import _lib
from self_play_reinforcement_learning_amd.arena import Arena, _stream
from tests.bounds_helpers import late_positions
from tests.stored_bounds_helpers import Trees, check_invariant, deep_expansions, host, play_games, same_bytes
from tests.variant_helpers import variant_oracle  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::DeprecationWarning")]


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    _lib.lib()


# board -> (empty cells of the positions, simulations): late enough for the trees to prove something
MID = {"tictactoe": (5, 60), "connect4": (12, 60), "connect4_6_5": (10, 60)}


@pytest.mark.parametrize("strong", [False, True])
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("game", ["tictactoe", "connect4", "connect4_6_5"])
def test_invariant_through_a_search(request, game, K, strong):
    """13 trees at late positions (A = 9 / P = 16: four groups a block; A = 7 and 6 / P = 8: eight; a partial last
    block either way), sequential and four sims in flight: the invariant holds before the search (the blocks of the
    play_action expansions), between two simulation steps (pending and locked leaves) and after it; the same run
    without stored bounds gives the same visit counts, values and counters, bit for bit."""
    if game == "connect4_6_5":
        request.getfixturevalue("variant_oracle")
    empty, sims = MID[game]
    seqs = late_positions(game, 13, empty, seed=3)
    run = Trees(game, seqs, sims, K, stored=True, strong=strong)
    a = run.arena
    check_invariant(a, run.ids, (game, K, "before"))
    run.search(lambda s: check_invariant(a, run.ids, (game, K, "step", s)) if s in (0, 3) else None)
    views, bb = check_invariant(a, run.ids, (game, K, "after"))
    assert sum(deep_expansions(v) for v in views) >= 13  # the walks went past the leaf's own entry
    if game == "tictactoe":  # 5 empty cells, 60 simulations: most trees have proved their position
        assert (bb["lo"] == bb["hi"]).any()
    a.check()
    plain = Trees(game, seqs, sims, K, stored=False, strong=strong)
    plain.search()
    rs0, rs1 = host(plain.arena.root_stats_batch(run.ids)), host(a.root_stats_batch(run.ids))
    same_bytes(rs0, rs1)
    assert plain.arena.counters() == a.counters()
    out0, out1 = host(plain.arena.search_end(1.0)), host(a.search_end(1.0))
    same_bytes(out0, out1)
    plain.arena.close()
    a.close()


@pytest.mark.parametrize("K,cap", [(1, None), (4, None), (4, 8)])
def test_invariant_mid_game_compacted_and_capped(K, cap):
    """8 Connect4 games from late openings in a store small enough to be compacted (moved roots, renumbered blocks,
    subtrees kept across moves), sequential, four in flight, and four in flight with the smallest sim cap (2 K:
    paused fills, stashed replies): the invariant holds on both trees of every game after every ply, and Move
    records, results and counters are those of the same games without stored bounds."""
    book = late_positions("connect4", 4, 22, seed=8)
    seen = []

    def on_ply(a, ply):
        views, _ = check_invariant(a, list(range(16)), ("games", K, cap, ply))
        seen.append(sum(deep_expansions(v) for v in views))

    kw = dict(book=book, blocks_per_tree=2 * 30 + 12, sim_cap=cap)
    a1, on = play_games("connect4", 8, 30, K, 13, True, on_ply=on_ply, **kw)
    a0, off = play_games("connect4", 8, 30, K, 13, False, **kw)
    assert on["counters"]["compactions"] > 0 and max(seen) > 0 and len(seen) >= 4, (on["counters"], seen)
    if cap is not None:
        assert a1.sim_pauses() > 0
    assert on["counters"] == off["counters"] and on["results"] == off["results"]
    same_bytes(on["moves"], off["moves"])
    a0.close()
    a1.close()


def test_proof_play_decides_the_same_from_the_stored_block():
    """12 Connect4 6x5 games with proof play on, K = 4, 50 simulations, the same seed with and without stored
    bounds: the verdict before every move (k_proof_verdict on the root's stored block, against the walk) restricts
    the same moves, so Move records, results, counters and the proof statistics are bit-identical -- and the proof
    did restrict moves."""
    a1, on = play_games("connect4_6_5", 12, 50, 4, 11, True, proof=True)
    a0, off = play_games("connect4_6_5", 12, 50, 4, 11, False, proof=True)
    assert on["proof"] == off["proof"] and on["proof"]["restricted"] > 0 and on["proof"]["solved"] > 0
    assert on["counters"] == off["counters"] and on["results"] == off["results"]
    same_bytes(on["moves"], off["moves"])
    last0, last1 = host(a0.proof_last()), host(a1.proof_last())
    same_bytes(last0, last1)
    a0.close()
    a1.close()


def test_proof_stop_stops_the_solved_trees():
    """13 TicTacToe trees at 5 empty cells, K = 4, proof play on, proof_stop after every simulation step, in two
    arenas of the same seed in lockstep, one with stored bounds (k_proof_stop reads the root's block) and one without
    (it walks).  Every call stops exactly the trees that are searching (started < the 60 simulations), not paused
    inside a fill by the sim cap (Arena.search_progress) and whose bounds_batch (the walk) gives lo == hi just before
    it -- no other tree, and every such tree -- and the two arenas stop the same trees."""
    seqs = late_positions("tictactoe", 13, 5, seed=3)
    runs = [Trees("tictactoe", seqs, 60, 4, stored=st) for st in (True, False)]
    for r in runs:
        r.arena.set_proof_play(True)
        r.arena.search_begin(r.ids)
    total = paused = 0
    for s in range(15):
        now = []
        for r in runs:
            a = r.arena
            r.step(a.select())
            before = a.proof_stopped().cpu().numpy()
            bb, prog = host(a.bounds_batch(r.ids)), host(a.search_progress())
            a.proof_stop()
            now.append(a.proof_stopped().cpu().numpy())
            due = (bb["lo"] == bb["hi"]) & (prog["started"] < 60) & ((prog["resume"] & 1) == 0)
            assert (now[-1] - before).tolist() == due.astype(int).tolist(), (s, prog)
            paused += int(((prog["resume"] & 1) != 0).sum())
            after = host(a.search_progress())["started"]
            assert (after[due] == 0x3fffffff).all() and (after[~due] == prog["started"][~due]).all()
        assert now[0].tolist() == now[1].tolist(), s
        total = int(now[0].sum())
    assert total > 0
    stats = [r.arena.proof_stats() for r in runs]
    assert stats[0] == stats[1] and stats[0]["trees_stopped"] == total
    same_bytes(host(runs[0].arena.root_stats_batch(runs[0].ids)), host(runs[1].arena.root_stats_batch(runs[1].ids)))
    for r in runs:
        r.arena.check()
        r.arena.close()


def test_refusals():
    """spmcts_set_solver_search: a null handle; a use flag that is on (NULL means every tree) is refused with -2 and
    starts nothing, since the search rules are not built; starting the maintenance after an expansion is refused with
    -4; a second call changes nothing.  The bounds export without stored bounds is refused and the plain export is
    untouched."""
    import ctypes

    import numpy as np

    L = _lib.lib()
    assert L.spmcts_set_solver_search(None, None) == -1
    seqs = late_positions("tictactoe", 2, 7, seed=1)
    late = Trees("tictactoe", seqs, 8, 1, stored=False)
    a = late.arena
    zeros = np.zeros(2, dtype=np.uint8).ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert L.spmcts_set_solver_search(a.h, zeros) == -4  # the play_action expansions made blocks
    with pytest.raises(_lib.SpmctsError):
        a.set_stored_bounds()
    assert not a.stored_bounds
    with pytest.raises(_lib.SpmctsError):
        a.export_subtrees([0], 16, min_visits=0, bounds=True)
    plain = a.export_subtrees([0, 1], 16, min_visits=0)
    assert "move_lo" not in plain and int(plain["count"].min()) > 1
    a.check()
    a.close()
    fresh = Arena("tictactoe", n_trees=2, iterations=8, rng="philox", seed=1, leaf_format="f32", leaf_layout="nchw")
    assert L.spmcts_set_solver_search(fresh.h, None) == -2  # NULL: every tree on
    for flags in (True, [False, True]):
        with pytest.raises(_lib.SpmctsError, match="not built"):
            fresh.set_solver_search(flags)
    assert not fresh.stored_bounds
    with pytest.raises(_lib.SpmctsError):  # the refused calls started nothing
        fresh.export_subtrees([0], 16, min_visits=0, bounds=True)
    fresh.set_solver_search([False, False])  # before any reset: nothing to stamp yet
    fresh.set_stored_bounds()
    with pytest.raises(_lib.SpmctsError, match="not built"):
        fresh.set_solver_search(True)
    assert fresh.stored_bounds
    fresh.tree_reset([0, 1], [1, -1])
    check_invariant(fresh, [0, 1], "fresh")
    ex = host(fresh.export_subtrees([0], 16, min_visits=0, bounds=True))
    assert ex["move_lo"][0, 1:10].tolist() == [-8] * 9 and ex["move_hi"][0, 1:10].tolist() == [7] * 9
    assert ex["move_lo"][0, 0] == -128 and (ex["move_lo"][0, 10:] == -128).all()
    t = fresh._dev_i32([0])
    assert L.spmcts_tree_export_bounds_batch(None, _lib.ptr(t), 1, 4, 0, -1, *[None] * 12, None, 0, _stream()) == -1
    assert L.spmcts_search_progress(None, None, None, _stream()) == -1
    fresh.check()
    fresh.close()


def test_bounds_contain_the_exact_scores_on_the_device_path(request):
    """analyse_positions(bounds=True, stored_bounds=True) on late positions against solve_to_end: every legal root
    move's interval contains its exact value and lo <= the best value <= hi; every output equals the run without
    stored bounds bit for bit; and the stored entries of the whole tree (tree=dict(bounds=True)) are the host
    recursion's.  The set holds solved trees and trees with a move ruled out."""
    from self_play_reinforcement_learning_amd import DeviceTableNet, TreeView, analyse_positions, solve_to_end
    from tests.bounds_helpers import code_to_value

    solved = cut = 0
    for game, empty, sims in (("tictactoe", 5, 100), ("connect4", 10, 60), ("connect4", 8, 100)):
        seqs = late_positions(game, 8, empty, seed=empty + 2)
        net = DeviceTableNet(game, salt=3)
        kw = dict(search_threads=4, seed=9, bounds=True)
        out = analyse_positions(game, net, seqs, sims, stored_bounds=True,
                                tree=dict(max_nodes=16 * sims, min_visits=0, bounds=True), **kw)
        plain = host(analyse_positions(game, net, seqs, sims, **kw))
        tree = out.pop("tree")
        out = host(out)
        same_bytes(out, plain)
        codes = solve_to_end(game, positions=seqs)["score"].cpu().numpy()
        for i in range(len(seqs)):
            view = TreeView.from_export(tree, i)
            assert view.has_bounds and not view.truncated
            want = view.node_bounds(game, out["board"][i], int(out["root_player"][i]))
            assert [(nd.move_lo, nd.move_hi) for nd in view.nodes] == want, (game, i)
            lo, hi, values = int(out["bound_lo"][i]), int(out["bound_hi"][i]), []
            for a in range(codes.shape[1]):
                mlo, mhi = int(out["move_lo"][i, a]), int(out["move_hi"][i, a])
                if codes[i, a] == -128:
                    assert mlo == mhi == -128
                    continue
                v = code_to_value(codes[i, a], empty)
                assert mlo <= v <= mhi, (game, seqs[i], a, v, mlo, mhi)
                values.append(v)
            assert lo <= max(values) <= hi
            solved += lo == hi
            cut += any(int(x) != -128 and int(x) < lo for x in out["move_hi"][i])
    assert solved >= 4 and cut >= 4, (solved, cut)


def test_a_league_keeps_them_too():
    """A league of one table net against itself (proof play on for the second player) and a random against a negamax
    player, with and without stored bounds: the same games and proof statistics, and the trees hold the invariant
    mid-league."""
    from self_play_reinforcement_learning_amd import DeviceTableNet
    from self_play_reinforcement_learning_amd.engine import LeagueEngine

    net = DeviceTableNet("connect4_6_5", salt=1)
    outs = []
    for stored in (True, False):
        players = [dict(network=net, iterations=30, name="plain"), dict(network=net, iterations=30, name="proof",
                                                                         proof_play=True),
                   dict(kind="random"), dict(kind="negamax", depth=2)]
        eng = LeagueEngine("connect4_6_5", players, [(0, 1), (2, 3)], games_per_pairing=6, seed=4, search_threads=4,
                           record_games=True, stored_bounds=stored)
        assert eng.arena.stored_bounds == stored
        eng.start()
        plies = 0
        while eng.games_done < eng.n_slots:
            eng.ply()
            plies += 1
            if stored and plies == 6:
                check_invariant(eng.arena, list(range(12)), "league")  # pairing (0, 1): the MCTS players' trees
        eng.check()
        r = eng.game_records()
        outs.append((sorted((int(r.pairing[i]), int(r.ids[i]), tuple(r.moves_of(i))) for i in range(len(r.ids))),
                     eng.arena.proof_stats()))
        eng.close()
    assert outs[0] == outs[1] and outs[0][1]["plies"] > 0


def test_engine_and_single_tree_search_carry_the_option():
    """SelfPlayEngine(stored_bounds=True) plays the games of the same engine without it (proof play and the early
    stop on, K = 4) and its trees hold the invariant; MCTreeSearch(stored_bounds=True).tree() carries the stored
    bounds on its nodes, equal to the view's own recursion."""
    from self_play_reinforcement_learning_amd import DeviceTableNet, MCTreeSearch
    from self_play_reinforcement_learning_amd.engine import SelfPlayEngine
    from self_play_reinforcement_learning_amd.envs import TicTacToeEnv

    book = late_positions("connect4", 8, 14, seed=21)
    outs = []
    for stored in (True, False):
        eng = SelfPlayEngine("connect4", DeviceTableNet("connect4", salt=2), n_games=16, iterations=60, seed=6,
                             max_games=16, search_threads=4, openings=book, record_games=True, proof_play=True,
                             proof_stop_every=2, stored_bounds=stored)
        assert eng.arena.stored_bounds == stored
        eng.start()
        for _ in range(3):
            eng.ply()
        if stored:
            check_invariant(eng.arena, list(range(32)), "engine")
        while eng.games_done < 16:
            eng.ply()
        eng.check()
        r = eng.game_records()
        games = sorted((int(r.ids[i]), tuple(r.moves_of(i))) for i in range(len(r.ids)))
        outs.append((games, eng.counters(), eng.arena.proof_stats()))
        eng.arena.close()
    assert outs[0] == outs[1] and outs[0][2]["trees_stopped"] > 0
    mc = MCTreeSearch(network=DeviceTableNet("tictactoe", salt=1), env=TicTacToeEnv, iterations=100, seed=3,
                      threading=True, thread_count=4, stored_bounds=True)
    mc.set_position([4, 0, 8, 2])
    mc.search()
    view, root = mc.tree(min_visits=0), mc.root_node
    assert view.has_bounds and not view.truncated
    assert [(nd.move_lo, nd.move_hi) for nd in view.nodes] == view.node_bounds("tictactoe", root.state, root.player)
    sb = mc.score_bounds()
    assert [c.move_lo for c in view.root.children] == sb["move_lo"]
    assert not MCTreeSearch(network=DeviceTableNet("tictactoe", salt=1), env=TicTacToeEnv, iterations=8,
                            seed=3).tree(min_visits=0).has_bounds
