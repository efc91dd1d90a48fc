"""Mirror symmetry on the GPU (include/spmcts.h spmcts_set_symmetry; csrc/board.h canonical_pair behind the SYM = true
kernels): tape parity with the host twin (oracle.mcts.OracleTree over symmetry.SymmetricNet of the table net), the
encoded rows of every leaf format, root equivariance, exact reuse across dedup / cache / lanes / the sim cap's stash /
compaction, engines against the twin evaluator, and the refusals."""
import numpy as np
import pytest
import torch

from self_play_reinforcement_learning_amd import _lib
from self_play_reinforcement_learning_amd.arena import Arena, table_net_eval
from self_play_reinforcement_learning_amd.symmetry import canonical, mirror_actions, mirror_moves
from tests.symmetry_helpers import (BOARDS, GROUPS, VARIANTS, MirrorTwinEvaluator, PureTableEvaluator,
                                    assert_tree_equal, positions, run_positions, twin_group)
from tests.variant_helpers import variant_oracle  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::DeprecationWarning")]


@pytest.fixture(scope="module", autouse=True)
def _device():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    _lib.lib()


# ----------------------------------------------------------------------------- tape parity
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("game", BOARDS)
def test_tape_parity_with_the_twin(request, game, K):
    """8 late positions per board (tictactoe 25 sims, P = 16; connect4 100; connect4 6x5 50; connect4 8x7 50: A ==
    APAD == 8, bit 63 in use, the byte-swap mirror): child_n, child_w, the root, action, tree_probs, q and its dtype
    flag and the counters (sims, depth sum, terminal leaves, leaks) equal the twin's, and no tape error is raised.
    The twin's visit counts differ from the plain oracle's on every group (tests/test_symmetry.py), so this fails on
    kernels that do not canonicalise."""
    if game in VARIANTS:
        request.getfixturevalue("variant_oracle")
    runs = twin_group(game, K)
    exps = [e for _, e, _ in runs]
    res, counters = run_positions(game, positions(game), GROUPS[game][1], K, [t for t, _, _ in runs])
    assert counters["error_flags"] == 0
    for key, name in (("sims", "sims"), ("depth_sum", "depth_sum"), ("terminal_leaves", "terminal_leaves"),
                      ("leaked_sims", "leaks")):
        assert counters[key] == sum(e["stats"][name] for e in exps), (game, K, key)
    for i, (r, e) in enumerate(zip(res, exps)):
        assert_tree_equal(r, e, (game, K, i))


# ----------------------------------------------------------------------------- encoding
def _pending_rows(game, fmt, layout, symmetry, dedup, seqs, K=4):
    """The rows of the second simulation step of one search per move list (Philox, so the same leaves whatever the
    leaf format), decoded to own - opp boards int64 [n, W, H]."""
    n = len(seqs)
    # (no root noise: the trees of a position and of its mirror image then search mirror images, so rows repeat)
    arena = Arena(game, n_trees=n, iterations=4 * K, rng="philox", seed=9, leaf_format=fmt, leaf_layout=layout,
                  search_threads=K, x_noise=0.0)
    arena.set_symmetry(symmetry)
    if dedup:
        arena.set_leaf_dedup(True)

    def step(count):
        if count:
            p, v = table_net_eval(game, arena.leaves(count), fmt, layout, salt=1)
            arena.expand(p, v)

    arena.tree_reset(list(range(n)), [1] * n)
    for i in range(max(len(s) for s in seqs)):
        on = [t for t in range(n) if i < len(seqs[t])]
        step(arena.play_action(on, [seqs[t][i] for t in on]))
    arena.search_begin(list(range(n)))
    step(arena.select())
    count = arena.select()
    rows = arena.leaf_rows()
    assert rows.shape[0] == count
    arena.check()
    if fmt == "board":
        out = rows.clone()
    else:
        planes = rows.float()
        assert torch.equal(planes.sum(dim=1), torch.ones_like(planes[:, 0]))  # one plane set per cell
        out = (planes[:, 1] - planes[:, 2]).to(torch.int64)
    arena.close()
    return out.cpu()


@pytest.mark.parametrize("dedup", [False, True])
def test_encoding(dedup):
    """The same pending leaves in arenas that differ only in leaf_format and layout: every format's rows decode to
    the board-format rows, every board-format row is its own canonical form, some row is the mirror image of what
    the arena without the mode writes, and with dedup the rows are pairwise distinct (and fewer)."""
    game = "connect4"
    seqs = positions(game)
    seqs = seqs + mirror_moves(game, seqs)
    ref = _pending_rows(game, "board", "nchw", "mirror", dedup, seqs)
    canon, flipped = canonical(game, ref.numpy(), np.ones(len(ref), dtype=np.int64))
    assert not flipped.any() and (canon == ref.numpy()).all()
    plain = _pending_rows(game, "board", "nchw", None, dedup, seqs)
    assert canonical(game, plain.numpy(), np.ones(len(plain), dtype=np.int64))[1].any()
    every = _pending_rows(game, "board", "nchw", "mirror", False, seqs) if dedup else ref
    if dedup:  # one row per distinct canonical input: the set of rows the arena without dedup writes
        assert len(torch.unique(ref.reshape(len(ref), -1), dim=0)) == len(ref) < len(every)
        assert torch.equal(torch.unique(ref.reshape(len(ref), -1), dim=0),
                           torch.unique(every.reshape(len(every), -1), dim=0))
    else:
        assert len(torch.unique(ref.reshape(len(ref), -1), dim=0)) < len(ref) <= len(seqs) * 4
    for fmt in ("f32", "f16", "bf16"):
        for layout in ("nchw", "nhwc"):
            got = _pending_rows(game, fmt, layout, "mirror", dedup, seqs)
            assert torch.equal(got, ref), (fmt, layout)


# ----------------------------------------------------------------------------- root equivariance
def test_root_equivariance():
    """analyse_positions on positions and their mirror images: with symmetry="mirror" the priors of each mirrored
    position are child_p[..., m] of its original bit for bit; without it they are not."""
    from self_play_reinforcement_learning_amd import DeviceTableNet, analyse_positions

    game = "connect4"
    seqs = positions(game)
    m = torch.as_tensor(mirror_actions(game)).cuda()
    both = seqs + mirror_moves(game, seqs)
    out = analyse_positions(game, DeviceTableNet(game, salt=1), both, iterations=1, symmetry="mirror")
    p = out["child_p"]
    assert torch.equal(p[len(seqs):], p[:len(seqs)][:, m])
    assert torch.equal(out["board"][len(seqs):], out["board"][:len(seqs)].flip(1))
    off = analyse_positions(game, DeviceTableNet(game, salt=1), both, iterations=1, symmetry=None)["child_p"]
    assert not torch.equal(off[len(seqs):], off[:len(seqs)][:, m])


# ----------------------------------------------------------------------------- exact reuse
def _by_game(moves, stride=None, lane_games=None):
    """Move rows grouped by game (a LanedEngine's lane-local ids mapped to the single arena's), each game's rows in
    their order."""
    ids = moves["game"].astype(np.int64)
    if stride is not None:
        ids = (ids // stride) * lane_games + ids % stride
    order = np.argsort(ids, kind="stable")
    return {k: (ids[order] if k == "game" else v[order]) for k, v in moves.items()}


def _collect(eng, games):
    got = []
    eng.run(games=games, on_moves=lambda m: got.append({k: v.cpu().numpy() for k, v in m.items()}))
    eng.check()
    return {k: np.concatenate([g[k] for g in got]) for k in got[0]}, eng.counters()


def test_exact_reuse():
    """128 games of connect4 to the end of a generation, 25 sims, 4 in flight, a 2-block tower through the fused fp16
    trunk, symmetry on: the Move records and the results are identical with dedup off, dedup on, dedup with a cache
    window, two lanes with cross-lane dedup and the shared table, a sim cap that pauses (the stash) and a node store
    that compacts; dedup buys fewer rows."""
    from self_play_reinforcement_learning_amd.engine import LanedEngine, SelfPlayEngine
    from self_play_reinforcement_learning_amd.evaluator import HipTowerEvaluator
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    torch.manual_seed(0)
    net = ResidualTower(7, 6, 7, num_blocks=2, filter_factor=32).cuda().eval()
    G = 128
    kw = dict(n_games=G, iterations=25, search_threads=4, symmetry="mirror", seed=3, max_games=G)
    runs = {}
    for name, extra in (("off", dict(leaf_dedup=False, eval_cache=0)), ("dedup", dict(leaf_dedup=True, eval_cache=0)),
                        ("cache", dict(leaf_dedup=True, eval_cache=1)), ("cap", dict(leaf_dedup=True, eval_cache=1)),
                        ("compact", dict(leaf_dedup=True, eval_cache=1, blocks_per_tree=6 * 25 + 64))):
        eng = SelfPlayEngine("connect4", net, **kw, **extra)
        assert isinstance(eng.evaluator, HipTowerEvaluator) and eng.arena.symmetry == "mirror"
        if name == "cap":
            eng.arena.set_sim_cap(8)
        moves, c = _collect(eng, G)
        runs[name] = (_by_game(moves), c, eng.arena.sim_pauses())
    lanes = LanedEngine("connect4", net, lanes=2, cross_dedup=True, eval_cache=1, **kw)
    assert lanes.cross_dedup and lanes.symmetry == "mirror"
    moves, c = _collect(lanes, G)
    runs["lanes"] = (_by_game(moves, LanedEngine.GAME_ID_STRIDE, G // 2), c, 0)
    m0, c0, _ = runs["off"]
    assert c0["games_finished"] == G and c0["nn_rows"] == c0["nn_leaves"]
    for name, (m, c, _) in runs.items():
        for k in m0:
            np.testing.assert_array_equal(m0[k], m[k], err_msg=f"{name}: {k}")
        for k in ("sims", "leaked_sims", "moves", "nn_leaves", "terminal_leaves", "depth_sum", "games_finished",
                  "results"):
            assert c0[k] == c[k], (name, k)
    assert runs["dedup"][1]["nn_rows"] < c0["nn_rows"]
    assert runs["cache"][1]["cache_rows"] > 0 and runs["cache"][1]["nn_rows"] < runs["dedup"][1]["nn_rows"]
    assert runs["lanes"][1]["nn_rows"] < c0["nn_rows"]
    assert runs["cap"][2] > 0
    assert runs["compact"][1]["compactions"] > 0 and c0["compactions"] == 0


# ----------------------------------------------------------------------------- engines against the twin evaluator
def _table(game, salt, fmt="f32"):
    from self_play_reinforcement_learning_amd import DeviceTableNet
    from self_play_reinforcement_learning_amd.evaluator import TableEvaluator

    net = DeviceTableNet(game, salt=salt)
    return TableEvaluator(net, "board") if fmt == "board" else net


@pytest.mark.parametrize("K", [1, 4])
def test_engine_against_the_twin_evaluator(K):
    """SelfPlayEngine(symmetry="mirror") on the table net plays the Move records of SelfPlayEngine(symmetry=None) on
    MirrorTwinEvaluator(table net): the kernels' canonical rows, un-permuted at the expand, are the twin's function."""
    from self_play_reinforcement_learning_amd.engine import SelfPlayEngine

    # (eval_cache=0: these evaluators take the host-synchronised loop, which skips the expand of a step without
    # network rows; the cache is for the device-count loop, where test_exact_reuse runs it)
    kw = dict(n_games=64, iterations=25, search_threads=K, seed=5, max_games=64, eval_cache=0)
    sym = SelfPlayEngine("connect4", _table("connect4", 1), symmetry="mirror", **kw)
    twin = SelfPlayEngine("connect4", MirrorTwinEvaluator(_table("connect4", 1, "board")), symmetry=None, **kw)
    plain = SelfPlayEngine("connect4", _table("connect4", 1), symmetry=None, **kw)
    (ms, cs), (mt, ct), (mp, _) = _collect(sym, 64), _collect(twin, 64), _collect(plain, 64)
    for k in ms:
        np.testing.assert_array_equal(ms[k], mt[k], err_msg=k)
    assert cs["results"] == ct["results"] and cs["sims"] == ct["sims"]
    assert ms["state"].shape != mp["state"].shape or not (ms["state"] == mp["state"]).all()  # other games than without


def test_two_network_arena_against_the_twin_evaluator():
    """An evaluate=True arena of two table nets of different salts, leaf dedup on: the same Move records and results
    as the twin evaluators' arena, so the two networks' rows never merge after canonicalisation."""
    from self_play_reinforcement_learning_amd.engine import SelfPlayEngine

    kw = dict(n_games=64, iterations=25, search_threads=4, seed=5, max_games=64, evaluate=True, eval_cache=0)
    sym = SelfPlayEngine("connect4", PureTableEvaluator(_table("connect4", 1)),
                         opponent=PureTableEvaluator(_table("connect4", 2)), symmetry="mirror", **kw)
    assert sym.leaf_dedup and sym.evaluator1 is not None
    twin = SelfPlayEngine("connect4", MirrorTwinEvaluator(_table("connect4", 1, "board")),
                          opponent=MirrorTwinEvaluator(_table("connect4", 2, "board")), symmetry=None, **kw)
    (ms, cs), (mt, ct) = _collect(sym, 64), _collect(twin, 64)
    for k in ms:
        np.testing.assert_array_equal(ms[k], mt[k], err_msg=k)
    assert cs["results"] == ct["results"]
    assert cs["nn_rows"] < cs["nn_leaves"]


def test_league_against_the_twin_evaluator():
    """A LeagueEngine of three table nets with record_games=True: the game records equal those of the league of
    their twin evaluators."""
    from self_play_reinforcement_learning_amd.engine import LeagueEngine

    recs = []
    for twin in (False, True):
        nets = [MirrorTwinEvaluator(_table("connect4", s, "board")) if twin else _table("connect4", s)
                for s in (1, 2, 3)]
        lg = LeagueEngine("connect4", [dict(network=n, iterations=25, name=f"n{i}") for i, n in enumerate(nets)],
                          [(0, 1), (0, 2), (1, 2)], games_per_pairing=8, seed=4, search_threads=4,
                          record_games=True, symmetry=None if twin else "mirror")
        assert lg.arena.symmetry == (None if twin else "mirror")
        lg.play()
        lg.check()
        r = lg.game_records()
        order = np.argsort(r.ids, kind="stable")
        recs.append({k: getattr(r, k)[order] for k in ("ids", "result", "swap", "plies", "moves", "pairing")})
        lg.close()
    assert len(recs[0]["ids"]) == 24
    for k in recs[0]:
        np.testing.assert_array_equal(recs[0][k], recs[1][k], err_msg=k)


# ----------------------------------------------------------------------------- refusals and defaults
def test_refusals_and_defaults(tmp_path):
    from self_play_reinforcement_learning_amd import Elo, ModelDatabase
    from self_play_reinforcement_learning_amd.base_model import ModelContainer
    from self_play_reinforcement_learning_amd.engine import SelfPlayEngine
    from self_play_reinforcement_learning_amd.envs import Connect4Env
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    L = _lib.lib()
    a = Arena("connect4", n_trees=2, iterations=8, search_threads=4)
    assert a.symmetry is None and L.spmcts_get_symmetry(a.h) == 0
    assert L.spmcts_set_symmetry(a.h, 7) == -3 and L.spmcts_get_symmetry(a.h) == 0
    with pytest.raises(ValueError):
        a.set_symmetry("rotate")
    a.set_symmetry("mirror")
    assert a.symmetry == "mirror" and L.spmcts_get_symmetry(a.h) == _lib.SYM_MIRROR
    a.set_symmetry(None)
    assert a.symmetry is None and L.spmcts_get_symmetry(a.h) == 0
    a.set_symmetry("mirror")
    # pairing lanes of different modes is refused; a paired arena's mode is fixed
    b = Arena("connect4", n_trees=2, iterations=8, search_threads=4)
    for x in (a, b):
        x.set_leaf_dedup(True)
    assert L.spmcts_set_leaf_peer(b.h, a.h) < 0 and b"symmetry" in L.spmcts_last_error()
    b.set_symmetry("mirror")
    b.set_leaf_peer(a)
    assert L.spmcts_set_symmetry(b.h, 0) == -2 and L.spmcts_set_symmetry(a.h, 0) == -2
    b.set_leaf_peer(None)
    b.close()
    # after a search the mode is fixed
    a.tree_reset([0, 1], [1, 1])
    a.search_begin([0, 1])
    n = a.select()
    p, v = table_net_eval("connect4", a.leaves(n), a.leaf_format, a.leaf_layout, salt=1)
    a.expand(p, v)
    assert L.spmcts_set_symmetry(a.h, 0) == -2 and b"before" in L.spmcts_last_error()
    assert L.spmcts_set_symmetry(a.h, 1) == 0  # (the mode it has)
    assert L.spmcts_get_symmetry(a.h) == 1
    a.close()

    # ModelContainers that disagree
    torch.manual_seed(0)
    net = ResidualTower(7, 6, 7, num_blocks=1, filter_factor=32).cuda().eval()
    db = ModelDatabase(tmp_path, Connect4Env)
    db.add_model("plain", ModelContainer("MCTreeSearch", policy_kwargs=dict(network=net, iterations=16)))
    db.add_model("mirror", ModelContainer("MCTreeSearch", policy_kwargs=dict(network=net, iterations=16,
                                                                            symmetry="mirror")))
    elo = Elo(db, seed=4)
    with pytest.raises(ValueError, match="symmetry"):
        elo.compare_models("plain", "mirror", num_games=2)
    assert elo.league_symmetry(["mirror"]) == "mirror" and elo.league_symmetry(["plain"]) is None
    new = elo.compare_models("plain", "mirror", num_games=2, symmetry="mirror")
    assert sum(new["plain__mirror"].values()) == 2

    # never set, and set to None: byte-identical games
    out = []
    for sym in ("unset", None):
        kw = {} if sym == "unset" else dict(symmetry=sym)
        eng = SelfPlayEngine("connect4", net, n_games=32, iterations=16, search_threads=4, seed=3, max_games=32, **kw)
        if sym is None:
            eng.arena.set_symmetry(None)
        out.append(_collect(eng, 32))
    for k in out[0][0]:
        assert out[0][0][k].tobytes() == out[1][0][k].tobytes(), k
    assert out[0][1] == out[1][1]
