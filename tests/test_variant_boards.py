"""CPU: the Connect4 variant boards 6x5 ("connect4_6_5") and 8x7 ("connect4_8_7").

The host-compiled bitboard rules and the oracle reproduce the reference's own outputs on the two boards
(fixtures of tests/golden/make_variant_golden.py), game_of_env names them, the host twins of the hard-coded
players agree with the oracle's, and the add-on library libspmcts_boards.so holds their fused trunks while the
product library does not.  8x7 is the board whose masks fill the 64 bits and whose lane group has no idle lane.
"""
import ctypes
import os
import random

import numpy as np
import pytest

from self_play_reinforcement_learning_amd import _lib
from tests.variant_helpers import BOARDS, TAGS, arena_games, searches, selfplay_games
from tests.variant_helpers import variant_oracle  # noqa: F401  (fixture)

pytestmark = pytest.mark.filterwarnings("ignore::DeprecationWarning")


def _kat(golden_dir, tag):
    return dict(np.load(os.path.join(golden_dir, f"env_kat_{tag}.npz")))


# ----------------------------------------------------------------------------- rules
@pytest.mark.parametrize("tag", TAGS)
def test_host_bitboard_step_matches_variant_kat(golden_dir, tag):
    _, W, H = BOARDS[tag]
    k = _kat(golden_dir, tag)
    L = _lib.lib()
    r, d = ctypes.c_int32(), ctypes.c_int32()
    valid = np.zeros(W, dtype=np.uint8)
    assert len(k["action"]) > 5000
    for i in range(len(k["action"])):
        if k["status"][i] == 2:
            continue  # GameOver is the env object's flag, not a board rule
        b = np.ascontiguousarray(k["before"][i].astype(np.int8))
        st = L.spmcts_env_step_host(_lib.CONNECT4, W, H, b.ctypes.data_as(ctypes.c_void_p), int(k["action"][i]),
                                    int(k["player"][i]), ctypes.byref(r), ctypes.byref(d))
        assert st == k["status"][i], i
        assert np.array_equal(b, k["after"][i]), i
        if st == 0:
            assert r.value == k["reward"][i] and bool(d.value) == bool(k["done"][i]), i
            L.spmcts_valid_moves_host(_lib.CONNECT4, W, H, b.ctypes.data_as(ctypes.c_void_p),
                                      valid.ctypes.data_as(ctypes.c_void_p))
            assert np.array_equal(valid.astype(bool), k["valid"][i]), i


@pytest.mark.parametrize("tag", TAGS)
def test_variant_kat_coverage(golden_dir, tag):
    """Each KAT holds a win in each direction, wins whose run touches each edge of the board (column 0, the last
    column, row 0, the top row: the bits next to the sentinels and, on 8x7, next to bit 63), a full-board draw,
    and the ValueError / GameOver rows."""
    _, W, H = BOARDS[tag]
    k = _kat(golden_dir, tag)
    seen = set()
    for i in np.nonzero((k["reward"] == 1) & (k["status"] == 0))[0]:
        b = k["after"][i].astype(int) * int(k["player"][i])
        for name, (dx, dy) in {"h": (1, 0), "v": (0, 1), "d1": (1, 1), "d2": (1, -1)}.items():
            for x in range(W):
                for y in range(H):
                    run = [(x + j * dx, y + j * dy) for j in range(4)]
                    if all(0 <= cx < W and 0 <= cy < H and b[cx, cy] == 1 for cx, cy in run):
                        seen.add(name)
                        seen |= {e for e, hit in (("col0", any(cx == 0 for cx, _ in run)),
                                                  ("colW", any(cx == W - 1 for cx, _ in run)),
                                                  ("row0", any(cy == 0 for _, cy in run)),
                                                  ("rowH", any(cy == H - 1 for _, cy in run))) if hit}
    assert seen == {"h", "v", "d1", "d2", "col0", "colW", "row0", "rowH"}
    draws = k["done"] & (k["reward"] == 0) & (k["status"] == 0)
    assert draws.any() and all(np.abs(k["after"][i]).sum() == W * H for i in np.nonzero(draws)[0])
    assert (k["status"] == 1).any() and (k["status"] == 2).any()


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_env_matches_variant_kat(golden_dir, tag):
    from oracle.envs import Connect4Env, GameOver

    _, W, H = BOARDS[tag]
    k = _kat(golden_dir, tag)
    for i in range(len(k["action"])):
        e = Connect4Env(W, H)
        e.set_state(k["before"][i].astype(np.int64))
        if k["status"][i] == 2:
            e.episode_over = True
        try:
            s, r, d, _ = e.step(int(k["action"][i]), int(k["player"][i]))
            st = 0
        except ValueError:
            st, s = 1, e.board
        except GameOver:
            st, s = 2, e.board
        assert st == k["status"][i], i
        assert np.array_equal(s, k["after"][i]), i
        if st == 0:
            assert r == k["reward"][i] and d == k["done"][i], i
            assert np.array_equal(e.valid_moves(), k["valid"][i]), i


@pytest.mark.parametrize("tag", TAGS)
def test_env_facade_replays_variant_kat_games(golden_dir, tag):
    """Connect4Env(W, H) of this package (host bitboard rules behind the reference API) replays the KAT's games:
    boards, rewards, done, valid moves, GameOver after the end, ValueError on a full column."""
    from self_play_reinforcement_learning_amd.envs import Connect4Env, GameOver

    game, W, H = BOARDS[tag]
    k = _kat(golden_dir, tag)
    env = Connect4Env(W, H)
    assert env.variant_string() == game and env.action_space.n == W and env.max_moves() == W * H
    played = 0
    for g in np.unique(k["game_id"][k["game_id"] >= 0])[:60]:
        env.reset()
        for i in np.nonzero(k["game_id"] == g)[0]:
            if k["status"][i] == 2:
                with pytest.raises(GameOver):
                    env.step(int(k["action"][i]), int(k["player"][i]))
                continue
            s, r, d, heights = env.step(int(k["action"][i]), int(k["player"][i]))
            assert np.array_equal(s, k["after"][i]) and r == k["reward"][i] and d == k["done"][i], i
            assert np.array_equal(env.valid_moves(), k["valid"][i]), i
            assert np.array_equal(heights, np.abs(k["after"][i]).sum(1))
            played += 1
    assert played > 500
    i = int(np.nonzero(k["status"] == 1)[0][0])
    env.reset()
    env.set_state(k["before"][i].astype(np.int64))
    with pytest.raises(ValueError):
        env.step(int(k["action"][i]), int(k["player"][i]))


# ----------------------------------------------------------------------------- the oracle on the new sizes
def _ids(tag, n):
    return [(tag, i) for i in range(n)]


@pytest.mark.parametrize("tag,idx", _ids("c4_6x5", 30) + _ids("c4_8x7", 30))
def test_oracle_search_matches_reference(variant_oracle, tag, idx):  # noqa: F811
    from oracle.mcts import NumpyRNG, OracleTree
    from oracle.table_net import TableNet
    from tests.parity_helpers import A_OF

    cases = searches(tag)
    assert len(cases) == 30
    assert sorted((c["sims"], c["strong_play"]) for c in cases) == [(25, False)] * 24 + [(200, False)] * 4 + [(200, True)] * 2
    c = cases[idx]
    assert c["game"] == BOARDS[tag][0]
    net = TableNet(A_OF[c["game"]], c["salt"])
    np.random.seed(c["seed"])
    t = OracleTree(c["game"], net, NumpyRNG(), c["sims"], strong_play=c["strong_play"])
    for a in c["opening"]:
        t.play_action(a)
    assert t.root.player == c["root_player"]
    a = t.move()
    st = t.root_stats()
    rec = t.temp_memory[-1]
    assert a == c["action"]
    assert st["child_n"] == c["child_n"] and st["child_w"] == c["child_w"]
    assert st["root_n"] == c["root_n"] and st["root_w"] == c["root_w"]
    assert rec["state"].reshape(-1).tolist() == c["state"]
    assert rec["tree_probs"].astype(float).tolist() == c["tree_probs"]
    assert float(rec["q"]) == c["q"]
    assert net.calls == c["net_calls"]


@pytest.mark.parametrize("tag,idx", _ids("c4_6x5", 6) + _ids("c4_8x7", 6))
def test_oracle_selfplay_games_match_reference(variant_oracle, tag, idx):  # noqa: F811
    from oracle.mcts import NumpyRNG
    from oracle.selfplay import play_episode
    from oracle.table_net import TableNet
    from tests.parity_helpers import A_OF

    games = selfplay_games(tag)
    assert [(g["evaluate"], g["swap_sides"]) for g in games] == [(False, False), (False, True), (False, False),
                                                                 (False, True), (True, False), (True, True)]
    g = games[idx]
    A = A_OF[g["game"]]
    net_p = TableNet(A, g["salt_policy"])
    net_o = net_p if not g["evaluate"] else TableNet(A, g["salt_opponent"])
    np.random.seed(g["seed"])
    rng = NumpyRNG()
    r, moves, log, _ = play_episode(g["game"], net_p, net_o, rng, rng, g["sims"], swap_sides=g["swap_sides"],
                                    update=not g["evaluate"], evaluate=g["evaluate"])
    assert r == g["result"]
    assert len(log) == len(g["plies"])
    for L, P in zip(log, g["plies"]):
        for k in ("tree", "action", "child_n", "child_w", "root_n", "root_w", "tree_probs", "q"):
            assert L[k] == P[k], k
    assert len(moves) == len(g["moves"])
    for m, M in zip(moves, g["moves"]):
        assert m["state"].reshape(-1).tolist() == M["state"]
        assert float(m["actual_val"]) == M["actual_val"]
        assert m["tree_probs"].astype(float).tolist() == M["tree_probs"]
        assert float(m["q"]) == M["q"]


@pytest.mark.parametrize("tag,idx", _ids("c4_6x5", 2) + _ids("c4_8x7", 2))
def test_oracle_lookahead_games_match_reference(variant_oracle, tag, idx):  # noqa: F811
    from oracle.hardcoded import PyRandomRNG
    from oracle.mcts import NumpyRNG
    from oracle.selfplay import play_episode
    from oracle.table_net import TableNet
    from tests.parity_helpers import A_OF

    games = arena_games(tag)
    assert [(g["opponent"], g["swap_sides"]) for g in games] == [("lookahead", False), ("lookahead", True)]
    g = games[idx]

    class Log(PyRandomRNG):
        def __init__(self, seed):
            super().__init__(seed)
            self.log = []

        def choice_index(self, n):
            k = super().choice_index(n)
            self.log.append([n, k])
            return k

    A = A_OF[g["game"]]
    np.random.seed(g["seed"])
    lg = Log(g["seed"])
    r, moves, log, (pol, opp, env) = play_episode(
        g["game"], TableNet(A, g["salt_policy"]), TableNet(A, g["salt_opponent"]), NumpyRNG(), lg, g["sims"],
        swap_sides=g["swap_sides"], update=False, evaluate=True, opponent="lookahead", opponent_iterations=None)
    assert r == g["result"] and moves == []
    searched = [L for L in log if "child_n" in L]
    assert len(searched) == len(g["plies"])
    for L, P in zip(searched, g["plies"]):
        for k in ("tree", "action", "child_n", "child_w", "root_n", "root_w"):
            assert L[k] == P[k], k
    assert env.board.reshape(-1).astype(int).tolist() == g["final_board"]
    assert lg.log == g["choices"]


def test_variant_oracle_patch_is_undone():
    """Outside the fixture the oracle and the helper tables know the default games only."""
    import oracle.mcts
    from tests import parity_helpers as ph

    assert sorted(ph.A_OF) == ["connect4", "tictactoe"] and sorted(ph.CELLS_OF) == ["connect4", "tictactoe"]
    with pytest.raises(KeyError):
        oracle.mcts.make_env("connect4_6_5")


# ----------------------------------------------------------------------------- Python surface
def test_game_of_env_names_the_instantiated_boards():
    import oracle.envs
    from self_play_reinforcement_learning_amd.arena import GAMES, game_of_env
    from self_play_reinforcement_learning_amd.envs import Connect4Env, TicTacToeEnv

    assert GAMES["connect4_6_5"] == (_lib.CONNECT4, 6, 5, 6) and GAMES["connect4_8_7"] == (_lib.CONNECT4, 8, 7, 8)
    for Env in (Connect4Env, oracle.envs.Connect4Env):
        assert game_of_env(Env(6, 5)) == "connect4_6_5"
        assert game_of_env(Env(8, 7)) == "connect4_8_7"
        assert game_of_env(Env()) == "connect4"
        assert game_of_env(Env) == "connect4"  # a class: its default size
        with pytest.raises(ValueError) as e:
            game_of_env(Env(5, 4))
        for board in ("7x6", "6x5", "8x7", "connect4_6_5", "connect4_8_7", "5x4"):
            assert board in str(e.value), str(e.value)
    assert game_of_env(TicTacToeEnv) == "tictactoe"
    for name, (gid, W, H, A) in GAMES.items():
        if gid == _lib.CONNECT4:
            assert Connect4Env(W, H).variant_string() == name


def test_arena_geometry_of_the_variant_boards():
    """spmcts_arena_bytes runs the library's (game, width, height) switch without a GPU: the four boards are
    accepted, another size is refused with an error that lists them."""
    L = _lib.lib()
    n = ctypes.c_uint64()
    for W, H, ok in ((7, 6, True), (6, 5, True), (8, 7, True), (5, 4, False), (8, 8, False)):
        cfg = _lib.Config()
        cfg.game, cfg.width, cfg.height = _lib.CONNECT4, W, H
        cfg.n_trees, cfg.n_games, cfg.iterations, cfg.search_threads = 8, 4, 16, 8  # K = 8 = 8x7's whole lane group
        rc = L.spmcts_arena_bytes(ctypes.byref(cfg), ctypes.byref(n))
        assert (rc == 0) == ok, (W, H, rc)
        if not ok:
            msg = L.spmcts_last_error().decode()
            for board in ("connect4 7x6", "connect4 6x5", "connect4 8x7", "tictactoe 3x3"):
                assert board in msg, msg


@pytest.mark.parametrize("tag", TAGS)
def test_host_hardcoded_players_match_oracle_on_variant_boards(variant_oracle, tag):  # noqa: F811
    """OneStepLookahead / Random on Connect4Env(W, H) vs oracle.hardcoded, 100 random positions per board."""
    from oracle.hardcoded import HardcodedPlayer, PyRandomRNG
    from self_play_reinforcement_learning_amd.envs import Connect4Env
    from self_play_reinforcement_learning_amd.hardcoded_players import OneStepLookahead, Random

    game, W, H = BOARDS[tag]
    rng = np.random.default_rng(3 + W)
    checked = case = 0
    while checked < 100:
        case += 1
        ref = variant_oracle(game)
        ref.reset()
        plays, player = [], 1
        for _ in range(int(rng.integers(0, W * H - 4))):
            a = int(rng.choice(np.flatnonzero(ref.valid_moves())))
            _, _, done, _ = ref.step(a, player)
            if done:
                break
            plays.append((a, player))
            player = -player
        if ref.episode_over:
            continue
        checked += 1
        for kind, Cls in (("lookahead", OneStepLookahead), ("random", Random)):
            look = 1 if case % 2 else -1
            host = Cls(env=Connect4Env(W, H))
            host.reset(look)
            orc = HardcodedPlayer(kind, game, PyRandomRNG(case))
            orc.reset(look)
            for a, p in plays:
                host.play_action(a, p)
                orc.play_action(a, p)
            random.seed(case)
            assert host(None) == orc.move(), (case, kind, plays)


# ----------------------------------------------------------------------------- the two libraries
def test_both_libraries_export_the_tower_entry_points():
    assert os.path.exists(_lib.BOARDS_LIB_PATH), "libspmcts_boards.so is built by `make all`"
    B = _lib.boards_lib()
    L = _lib.lib()
    assert len(_lib.TOWER_SYMBOLS) == 6
    for name in _lib.TOWER_SYMBOLS:
        assert hasattr(L, name) and hasattr(B, name), name


def test_tower_supported_by_library():
    L, B = _lib.lib(), _lib.boards_lib()
    for W, H in ((6, 5), (8, 7)):
        for C in (128, 256):
            assert L.spmcts_tower_supported(W, H, C) == 0
            assert B.spmcts_tower_supported(W, H, C) == 1
            assert B.spmcts_tower_weight_layout(W, H, C) == _lib.WLAYOUT_32X32
            assert _lib.tower_lib(W, H, C) is B
        assert B.spmcts_tower_supported(W, H, 64) == 0 and _lib.tower_lib(W, H, 64) is None
    for W, H in ((7, 6), (3, 3)):
        for C in (128, 256):
            assert B.spmcts_tower_supported(W, H, C) == 0 and L.spmcts_tower_supported(W, H, C) == 1
            assert _lib.tower_lib(W, H, C) is L
            assert B.spmcts_tower_weight_layout(W, H, C) == -2
    # a shape a library does not hold: -2 from every entry point, before anything is launched
    assert B.spmcts_tower_forward(7, 6, 128, 2, None, 1, None, None, None, 0, None) == -2
    assert B.spmcts_tower_heads(7, 6, 128, 7, None, 1, None, None, None, None, 0, None) == -2
    assert B.spmcts_tower_heads(6, 5, 128, 7, None, 1, None, None, None, None, 0, None) == -2  # A = 6 on 6x5
    assert L.spmcts_tower_forward(6, 5, 128, 2, None, 1, None, None, None, 0, None) == -2
    assert B.spmcts_tower_forward(6, 5, 128, 2, None, 0, None, None, None, 0, None) == 0  # empty batch: nothing to do


def test_add_on_library_holds_only_the_variant_trunk_kernels():
    """libspmcts_boards.so: the board-major 32x32x16 trunks of 6x5 and 8x7 at C = 128 / 256 in bf16 / fp16 (8
    k_tower, 8 k_tower_dyn) and their 8 k_heads_co; no 7x6 or 3x3 kernel."""
    import re

    from tests.test_native_lib import _kernel_handles

    names = _kernel_handles(_lib.BOARDS_LIB_PATH)
    dyn = [n for n in names if n.startswith("_ZN5tower11k_tower_dyn")]
    host = [n for n in names if n.startswith("_ZN5tower7k_tower")]
    assert len(dyn) == 8 and len(host) == 8, (len(dyn), len(host))
    cfgs = re.findall(r"(?:CfgI|NS1_I)Li(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", " ".join(dyn + host))
    assert {(c[0], c[2], c[3]) for c in cfgs} == {("128", "6", "5"), ("256", "6", "5"), ("128", "8", "7"),
                                                 ("256", "8", "7")}
    assert len([n for n in names if n.startswith("_ZN5tower10k_heads_co")]) == 8


def test_variant_nets_fall_back_without_the_add_on_library(monkeypatch):
    """With the add-on library absent, no library holds the variant shapes: HipTowerEvaluator.supported is
    False (make_evaluator then takes the PyTorch TowerEvaluator) and constructing it raises."""
    from self_play_reinforcement_learning_amd.evaluator import HipTowerEvaluator
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    net = ResidualTower(6, 5, 6, num_blocks=1, filter_factor=32)
    assert HipTowerEvaluator.supported(net)
    monkeypatch.setattr(_lib, "_boards", None)
    monkeypatch.setattr(_lib, "BOARDS_LIB_PATH", os.path.join(os.path.dirname(_lib.BOARDS_LIB_PATH), "absent.so"))
    assert _lib.boards_lib() is None and _lib.tower_lib(6, 5, 128) is None
    assert not HipTowerEvaluator.supported(net)
    assert HipTowerEvaluator.supported(ResidualTower(7, 6, 7, num_blocks=1, filter_factor=32))
    with pytest.raises(ValueError, match="not instantiated"):
        HipTowerEvaluator(net)
