"""GPU: solver-aware search (Arena.set_solver_rules; csrc/arena_solver.h sb_refuted / sb_proved behind the SB = true
k_select / sim_vl).  The arena on the host twin's tapes (tests/solver_search_helpers.py SolverOracleTree) equals
the twin bit for bit with both rules, each rule alone, sequential and four sims in flight, strong_play on and off;
trees without rule bits in the same arena are untouched; the stored-bounds invariant holds with the rules on;
whole games; the register copy of the root's block; refusals, defaults and the Python options.  Every network is
the table net."""
import ctypes

import numpy as np
import pytest
import torch

from self_play_reinforcement_learning_amd import _lib
from self_play_reinforcement_learning_amd.arena import Arena
from tests.bounds_helpers import late_positions
from tests.solver_search_helpers import (GROUPS, SolverOracleTree, assert_counters_equal, assert_tree_equal,
                                         group_positions, run_games, run_positions, twin_group, twin_search)
from tests.stored_bounds_helpers import check_invariant, host
from tests.variant_helpers import variant_oracle  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::DeprecationWarning")]


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    _lib.lib()


@pytest.mark.parametrize("rules", ["both", "refute", "proved"])
@pytest.mark.parametrize("strong", [False, True])
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("game", sorted(GROUPS))
def test_tape_parity_with_the_twin(request, game, K, strong, rules):
    """8 late positions per board (tictactoe 6 empty / 25 sims, P = 16; connect4 12 empty / 100 sims and connect4 6x5
    10 empty / 50 sims, P = 8): child_n, child_w, the root, action, tree_probs, q and its dtype flag, the counters
    (sims, depth sum, terminal leaves, leaks) and the two statistics equal the twin's, and no tape error is raised.
    The twin's rules fire in every group (tests/test_solver_search.py), and its visit counts differ from the plain
    oracle's, so this fails on kernels that do not apply them."""
    if game == "connect4_6_5":
        request.getfixturevalue("variant_oracle")
    runs = twin_group(game, K, strong, rules)
    exps = [e for _, e, _ in runs]
    assert sum(e["stats"]["proved"] + e["stats"]["refuted_levels"] for e in exps) > 0
    res, counters, stats, per_tree = run_positions(game, group_positions(game), GROUPS[game][1], K,
                                                   [t for t, _, _ in runs], rules, strong)
    assert_counters_equal(counters, stats, exps, (game, K, strong, rules))
    for i, (r, e) in enumerate(zip(res, exps)):
        assert_tree_equal(r, e, (game, K, strong, rules, i))
        assert per_tree[i].tolist() == [e["stats"]["proved"], e["stats"]["refuted_levels"]], i


@pytest.mark.parametrize("game,K", [("tictactoe", 4), ("connect4", 4), ("connect4", 1)])
def test_mixed_arena(game, K):
    """Odd trees with both rules, even trees with none, in one arena: the odd trees equal the twin, the even trees
    are byte-identical to the same arena run with stored bounds only (and to the plain oracle), and count nothing."""
    from oracle.mcts import OracleTree

    sims, seqs = GROUPS[game][1], group_positions(game)
    on = twin_group(game, K, False, "both")
    plain = [twin_search(game, m, sims, K, i, cls=OracleTree) for i, m in enumerate(seqs)]
    mixed = [on[i] if i % 2 else plain[i] for i in range(len(seqs))]
    tapes = [t for t, *_ in mixed]
    rules = ["both" if i % 2 else "off" for i in range(len(seqs))]
    res, counters, stats, per_tree = run_positions(game, seqs, sims, K, tapes, rules)
    exps = [m[1] for m in mixed]
    assert_counters_equal(counters, stats, exps, (game, K))
    for i, (r, e) in enumerate(zip(res, exps)):
        e = dict(e, q_f64=e.get("q_f64", r["q_f64"]))
        assert_tree_equal(r, e, (game, K, i))
    assert per_tree[0::2].sum() == 0 and per_tree[1::2].sum() > 0
    # the off trees against an arena that only stores the bounds: the same bytes (the on trees' tapes do not fit
    # that run, so only the even trees are run there, at their own ids' tapes)
    base, c0, s0, _ = run_positions(game, seqs[0::2], sims, K, tapes[0::2], "off")
    assert s0 == dict(proved=0, refuted_levels=0) and c0["error_flags"] == 0
    for b, r in zip(base, res[0::2]):
        assert sorted(b) == sorted(r)
        for k in b:
            assert np.asarray(b[k]).tobytes() == np.asarray(r[k]).tobytes(), k


@pytest.mark.parametrize("game", ["tictactoe", "connect4"])
def test_the_stored_bounds_invariant_holds_with_the_rules_on(game):
    """K = 4, both rules: stored_bounds_helpers.check_invariant between simulation steps (leaves pending and locked)
    and after the search; the twin's parity holds in the same run."""
    sims, seqs = GROUPS[game][1], group_positions(game)
    runs = twin_group(game, 4, False, "both")
    ids, seen = list(range(len(seqs))), []

    def between(arena, s):
        if s in (0, 2, 5, "end"):
            check_invariant(arena, ids, (game, s))
            seen.append(s)

    res, counters, stats, _ = run_positions(game, seqs, sims, 4, [t for t, _, _ in runs], "both", between=between)
    assert len(seen) == 4
    assert_counters_equal(counters, stats, [e for _, e, _ in runs], game)
    for i, (r, (_, e, _)) in enumerate(zip(res, runs)):
        assert_tree_equal(r, e, (game, i))


@pytest.mark.parametrize("game,sims,K,kw", [
    ("tictactoe", 20, 4, dict(sim_cap=8)),
    ("tictactoe", 20, 1, dict(blocks_per_tree=3 * 20 + 16)),
    ("connect4_6_5", 24, 4, dict(sim_cap=8)),
    ("connect4_6_5", 24, 4, dict(blocks_per_tree=4 * 24 + 40)),
])
def test_whole_games(request, game, sims, K, kw):
    """6 self-play games of two twins each (oracle.selfplay.play_episode with the twin patched in) on their tapes,
    with the smallest sim cap and with a node store small enough to compact: Move records and results equal the
    twin's, the statistics too, and every search_node call is accounted for."""
    if game == "connect4_6_5":
        request.getfixturevalue("variant_oracle")
    G = 6
    moves, counters, stats, eps = run_games(game, G, sims, K, "both", **kw)
    assert counters["error_flags"] == 0 and counters["games_finished"] == G
    if "blocks_per_tree" in kw:
        assert counters["compactions"] > 0
    exp_results = np.zeros((2, 3), dtype=np.int64)
    by_game = {}
    for i in range(len(moves["z"])):
        by_game.setdefault(int(moves["game"][i]), []).append(i)
    for gi, (_, _, r, exp_moves, _) in enumerate(eps):
        exp_results[gi % 2][{1: 0, 0: 1, -1: 2}[r]] += 1
        rows = by_game.get(gi, [])
        assert len(rows) == len(exp_moves), gi
        for i, M in zip(rows, exp_moves):
            assert moves["state"][i].astype(int).tolist() == M["state"].reshape(-1).astype(int).tolist(), (gi, i)
            assert float(moves["z"][i]) == float(M["actual_val"]), (gi, i)
            assert moves["tree_probs"][i].astype(float).tolist() == M["tree_probs"].astype(float).tolist(), (gi, i)
            q = np.float64(moves["q"][i]) if moves["q_f64"][i] else np.float32(moves["q"][i])
            assert float(q) == float(M["q"]), (gi, i)
    assert np.array_equal(np.array(counters["results"]), exp_results)
    tw = [s for e in eps for s in e[4]]
    assert stats["proved"] == sum(s["proved"] for s in tw) > 0
    assert stats["refuted_levels"] == sum(s["refuted_levels"] for s in tw) > 0
    assert counters["sims"] == sum(s["sims"] for s in tw) and counters["leaked_sims"] == sum(s["leaks"] for s in tw)
    assert counters["sims"] + counters["leaked_sims"] == counters["moves"] * sims


def _root_rule_changes(game, moves, sims, K, seed):
    """Replies of the twin's search after which solver_select at the root decides otherwise than before and a later
    select still runs: (count, the twin's tape and results)."""
    from self_play_reinforcement_learning_amd.tree import solver_select

    changes = []

    class Watch(SolverOracleTree):
        def _masks(self):
            mlo, mhi = self.move_bounds(self.root)
            r, p, _ = solver_select(mlo, mhi, expanded=[bool(c.children) for c in self.root.children])
            return r.tolist(), p.tolist()

        def _reply_threaded(self, *item):
            before = self._masks()
            super()._reply_threaded(*item)
            if self._masks() != before:
                changes.append(self.stats["sims"] + self.stats["leaks"])

    tape, exp, t = twin_search(game, moves, sims, K, seed, cls=Watch)
    selects = t.stats["sims"] + t.stats["leaks"]
    return sum(1 for c in changes if c < selects), tape, exp


def test_register_copy():
    """K = 4, tictactoe, 6 empty cells: in the twin, replies change what the two rules decide at the root itself (an
    sb_propagate that reaches the root's block on the device) and the fill right after such a reply -- the same
    launch, where the root's block sits in registers -- selects at the root again.  The device equals the twin on
    these cases, which it could not with a stale copy."""
    seqs = group_positions("tictactoe")
    runs = [_root_rule_changes("tictactoe", m, 25, 4, i) for i, m in enumerate(seqs)]
    assert sum(n for n, _, _ in runs) >= 8, [n for n, _, _ in runs]
    res, counters, stats, _ = run_positions("tictactoe", seqs, 25, 4, [t for _, t, _ in runs], "both")
    assert_counters_equal(counters, stats, [e for _, _, e in runs], "register copy")
    for i, (r, (_, _, e)) in enumerate(zip(res, runs)):
        assert_tree_equal(r, e, i)


def test_refusals_and_defaults():
    """spmcts_set_solver_rules: -1 for a null handle, -3 for a bit outside REFUTE | PROVED, -4 for an arena without
    stored bounds; the statistics are zero before use; NULL switches every rule off; rules switched off again give
    the stored-only search from that search on."""
    L = _lib.lib()
    u8 = lambda xs: np.asarray(xs, dtype=np.uint8).ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))  # noqa: E731
    out = (ctypes.c_int64 * 2)(7, 7)
    assert L.spmcts_set_solver_rules(None, None) == -1
    assert L.spmcts_get_solver_stats(None, out) == -1
    a = Arena("tictactoe", n_trees=2, iterations=8, rng="philox", seed=1, leaf_format="f32", leaf_layout="nchw")
    assert a.solver_rules.tolist() == [0, 0]  # never set
    assert L.spmcts_set_solver_rules(a.h, u8([1, 2])) == -4  # no stored bounds yet
    assert L.spmcts_set_solver_rules(a.h, u8([4, 0])) == -3
    assert L.spmcts_set_solver_rules(a.h, None) == -4
    assert a.solver_stats() == dict(proved=0, refuted_levels=0)
    assert a.solver_stats(per_tree=True).cpu().tolist() == [[0, 0], [0, 0]]
    a.set_stored_bounds()
    assert L.spmcts_set_solver_rules(a.h, u8([3, 8])) == -3
    assert L.spmcts_set_solver_rules(a.h, None) == 0 and L.spmcts_set_solver_rules(a.h, u8([0, 0])) == 0
    assert a.solver_stats() == dict(proved=0, refuted_levels=0)
    with pytest.raises(ValueError):
        a.set_solver_rules(refute=[True])
    a.set_solver_rules(refute=[True, False], proved=True)
    assert a.solver_rules.tolist() == [3, 2]
    with pytest.raises(_lib.SpmctsError, match="not built"):  # the maintenance switch keeps refusing use flags
        a.set_solver_search(True)
    a.check()
    a.close()
    b = Arena("tictactoe", n_trees=1, iterations=8, rng="philox", seed=1, leaf_format="f32", leaf_layout="nchw")
    b.set_solver_rules()  # switches the stored bounds on first
    assert b.stored_bounds and b.solver_rules.tolist() == [3]
    b.close()
    # on, then off again: from that search on the trees search like an arena that only stores the bounds
    from tests.stored_bounds_helpers import Trees, same_bytes

    seqs = late_positions("tictactoe", 6, 6, seed=3)
    runs = [Trees("tictactoe", seqs, 25, 4, stored=True, seed=5) for _ in range(2)]
    runs[0].arena.set_solver_rules(True, True)
    runs[0].arena.set_solver_rules(False, False)
    for r in runs:
        r.search()
    same_bytes(host(runs[0].arena.root_stats_batch(runs[0].ids)), host(runs[1].arena.root_stats_batch(runs[1].ids)))
    assert runs[0].arena.counters() == runs[1].arena.counters()
    assert runs[0].arena.solver_stats() == dict(proved=0, refuted_levels=0)
    # a search with the rules on, then off (the statistics stay allocated and non-zero, the rule bits go): the
    # second search equals the twin's second search with both rules off, and counts nothing more
    gp = group_positions("tictactoe")
    twins = [twin_search("tictactoe", m, 25, 4, i, "both", then_off=True) for i, m in enumerate(gp)]
    seen = {}

    def off_again(arena):
        seen["first"] = arena.solver_stats()
        arena.set_solver_rules(False, False)
        assert arena.solver_rules.tolist() == [0] * len(gp)

    res, counters, stats, _ = run_positions("tictactoe", gp, 25, 4, [t for t, _, _ in twins], "both",
                                            first_search=off_again)
    assert seen["first"] == stats and stats["proved"] == sum(e["first"]["proved"] for _, e, _ in twins) > 0
    assert stats["refuted_levels"] == sum(e["first"]["refuted_levels"] for _, e, _ in twins) > 0
    assert_counters_equal(counters, stats, [e for _, e, _ in twins], "on then off")
    for i, (r, (_, e, _)) in enumerate(zip(res, twins)):
        assert_tree_equal(r, e, ("on then off", i))
    # and switched on, the same trees search otherwise
    on = Trees("tictactoe", seqs, 25, 4, stored=True, seed=5)
    on.arena.set_solver_rules()
    on.search()
    st = on.arena.solver_stats()
    assert st["proved"] > 0 and st["refuted_levels"] > 0
    assert host(on.arena.root_stats_batch(on.ids))["child_n"].tolist() != \
        host(runs[1].arena.root_stats_batch(runs[1].ids))["child_n"].tolist()
    for r in runs + [on]:
        r.arena.check()
        r.arena.close()


def test_the_python_options_carry_it():
    """solver_search= on MCTreeSearch, SelfPlayEngine (one side only, too), a league with one player on, and
    analyse_positions, whose bounds still contain solve_to_end's values."""
    from self_play_reinforcement_learning_amd import DeviceTableNet, MCTreeSearch, analyse_positions, solve_to_end
    from self_play_reinforcement_learning_amd.engine import LeagueEngine, SelfPlayEngine
    from self_play_reinforcement_learning_amd.envs import TicTacToeEnv
    from tests.bounds_helpers import code_to_value

    mc = MCTreeSearch(network=DeviceTableNet("tictactoe", salt=1), env=TicTacToeEnv, iterations=60, seed=3,
                      threading=True, thread_count=4, solver_search=True)
    assert mc.stored_bounds and mc._arena.solver_rules.tolist() == [3]
    mc.set_position([4, 0, 8, 2])
    mc.search()
    assert mc._arena.solver_stats()["proved"] > 0
    one = MCTreeSearch(network=DeviceTableNet("tictactoe", salt=1), env=TicTacToeEnv, iterations=8, seed=3,
                       solver_search="refute")
    assert one._arena.solver_rules.tolist() == [1]
    with pytest.raises(ValueError):
        MCTreeSearch(network=DeviceTableNet("tictactoe", salt=1), env=TicTacToeEnv, iterations=8, solver_search="x")

    book = late_positions("connect4", 8, 14, seed=21)
    eng = SelfPlayEngine("connect4", DeviceTableNet("connect4", salt=2), n_games=8, iterations=40, seed=6, max_games=8,
                         search_threads=4, openings=book, solver_search=True, opponent_solver_search=False)
    assert eng.arena.stored_bounds and eng.arena.solver_rules.tolist() == [3, 0] * 8
    eng.start()
    while eng.games_done < 8:
        eng.ply()
    eng.check()
    per_tree = eng.arena.solver_stats(per_tree=True).cpu().numpy()
    assert per_tree[0::2].sum() > 0 and per_tree[1::2].sum() == 0
    c = eng.counters()
    eng.arena.close()
    assert c["error_flags"] == 0

    net = DeviceTableNet("connect4_6_5", salt=1)
    players = [dict(network=net, iterations=30, name="plain"),
               dict(network=net, iterations=30, name="solver", solver_search=True), dict(kind="random")]
    lg = LeagueEngine("connect4_6_5", players, [(0, 1), (1, 2)], games_per_pairing=4, seed=4, search_threads=4)
    assert lg.arena.stored_bounds and lg.solver_search
    rules = lg.arena.solver_rules.tolist()
    assert rules[:8] == [0, 3] * 4 and rules[8:] == [3, 0] * 4
    lg.play()
    lg.check()
    per_tree = lg.arena.solver_stats(per_tree=True).cpu().numpy()
    assert per_tree[np.array(rules) == 0].sum() == 0 and per_tree[np.array(rules) == 3].sum() > 0
    lg.close()

    for game, empty, sims in (("tictactoe", 5, 100), ("connect4", 10, 60)):
        seqs = late_positions(game, 8, empty, seed=empty + 2)
        out = analyse_positions(game, DeviceTableNet(game, salt=3), seqs, sims, search_threads=4, seed=9, bounds=True,
                                solver_search=True)
        st = out.pop("solver_stats")
        assert st["proved"] > 0 and st["refuted_levels"] > 0
        out = host(out)
        codes = solve_to_end(game, positions=seqs)["score"].cpu().numpy()
        for i in range(len(seqs)):
            values = []
            for a in range(codes.shape[1]):
                mlo, mhi = int(out["move_lo"][i, a]), int(out["move_hi"][i, a])
                if codes[i, a] == -128:
                    assert mlo == mhi == -128
                    continue
                v = code_to_value(codes[i, a], empty)
                assert mlo <= v <= mhi, (game, seqs[i], a, v, mlo, mhi)
                values.append(v)
            assert int(out["bound_lo"][i]) <= max(values) <= int(out["bound_hi"][i])


def test_model_containers_and_lanes_carry_it(tmp_path):
    """A ModelContainer's policy_kwargs through Elo: players() carries solver_search and stored_bounds, the league
    built from them sets the rule bits of that model's trees only, on late openings those trees count and the
    others do not, and compare_models plays; a LanedEngine hands the option to every lane's arena."""
    from self_play_reinforcement_learning_amd import Elo, ModelDatabase
    from self_play_reinforcement_learning_amd.base_model import ModelContainer
    from self_play_reinforcement_learning_amd.engine import LanedEngine, LeagueEngine
    from self_play_reinforcement_learning_amd.envs import Connect4Env
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    torch.manual_seed(0)
    net = ResidualTower(7, 6, 7, num_blocks=1, filter_factor=32).cuda().eval()
    db = ModelDatabase(tmp_path, Connect4Env)
    db.add_model("plain", ModelContainer("MCTreeSearch", policy_kwargs=dict(network=net, iterations=40)))
    db.add_model("solver", ModelContainer("MCTreeSearch", policy_kwargs=dict(network=net, iterations=40,
                                                                            solver_search="proved")))
    db.add_model("stored", ModelContainer("MCTreeSearch", policy_kwargs=dict(network=net, iterations=40,
                                                                            stored_bounds=True)))
    elo = Elo(db, seed=4)
    ps = elo.named_players(["plain", "solver", "stored"])
    assert [p["solver_search"] for p in ps] == [False, "proved", False]
    assert [p["stored_bounds"] for p in ps] == [False, False, True]
    book = late_positions("connect4", 4, 12, seed=3)
    lg = LeagueEngine("connect4", ps[:2], [(0, 1)], games_per_pairing=4, seed=4, search_threads=4, openings=book)
    rules = lg.arena.solver_rules
    assert lg.arena.stored_bounds and rules.tolist() == [0, 2] * 4
    lg.play()
    lg.check()
    per_tree = lg.arena.solver_stats(per_tree=True).cpu().numpy()
    assert per_tree[rules == 0].sum() == 0 and per_tree[rules == 2, 0].sum() > 0 and per_tree[:, 1].sum() == 0
    lg.close()
    plain = LeagueEngine("connect4", [ps[0], ps[2]], [(0, 1)], games_per_pairing=2, seed=4, search_threads=4,
                         stored_bounds=any(p["stored_bounds"] for p in ps))
    assert plain.arena.stored_bounds and not plain.solver_search
    plain.close()
    new = elo.compare_models("plain", "solver", num_games=4, openings=book)
    assert sum(new["solver__plain"].values()) == 4

    eng = LanedEngine("connect4", net, n_games=16, lanes=2, iterations=16, seed=7, search_threads=4, max_games=16,
                      solver_search=True, opponent_solver_search="refute")
    for lane in eng.lanes:
        assert lane.arena.stored_bounds and lane.arena.solver_rules.tolist() == [3, 1] * lane.n_games
    eng.run(plies=4)
    eng.check()
