"""The sim cap on the GPU (include/spmcts.h spmcts_set_sim_cap; csrc/arena_select.h "sim cap"): a tree pauses at a
sim boundary once it has started `cap` sims in a launch, and the next launch resumes its slot cycle there.  The
cap only moves work between launches, so every run with cap = 2 K must give exactly what the same run with the
cap off gives -- Move records and search counters bit for bit, no sticky error -- while the pause counter shows
that launches did pause.  Games are played to the end: the late plies are where the terminal-leaf streaks are.
(The schedule itself is restated and checked on the CPU: tests/test_sim_cap_schedule.py.)"""
import functools

import numpy as np
import pytest
import torch

from tests.parity_helpers import _eval_table, empty_prior, g3_tapes
from tests.test_sim_cap_schedule import GPU_TAPE_CASES, gpu_tape_game

pytestmark = pytest.mark.gpu

SEARCH_COUNTERS = ("sims", "leaked_sims", "nn_leaves", "terminal_leaves", "depth_sum")
GAME_COUNTERS = SEARCH_COUNTERS + ("moves", "games_finished", "positions_exported", "results", "set_node_expansions")


def _net(game, seed=0):
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    torch.manual_seed(seed)
    W, H, A = (7, 6, 7) if game == "connect4" else (3, 3, 9)
    return ResidualTower(W, H, A, num_blocks=2, filter_factor=32).cuda().eval()


def _collect(eng, arenas, cap):
    """Play every game of `eng` to the end with the given cap; (Move records, counters, pauses)."""
    for a in arenas:
        a.set_sim_cap(cap)
    got = []
    eng.run(plies=64, on_moves=lambda m: got.append({k: v.cpu().numpy() for k, v in m.items()}))
    eng.check()
    c = eng.counters()
    assert c["error_flags"] == 0
    return {k: np.concatenate([g[k] for g in got]) for k in got[0]}, c, sum(a.sim_pauses() for a in arenas)


def _assert_same(off, on, n_games):
    (m0, c0, p0), (m1, c1, p1) = off, on
    assert c0["games_finished"] == n_games and len(m0["z"]) > 0  # played to the end
    assert sorted(m0) == sorted(m1)
    for k in m0:  # state, tree_probs, q, z (and the game ids)
        np.testing.assert_array_equal(m0[k], m1[k], err_msg=k)
    for k in GAME_COUNTERS:
        assert c0[k] == c1[k], k
    assert p0 == 0 and p1 > 0, (p0, p1)


# ----------------------------------------------------------------------------- Philox, the engine's device-count path
@pytest.mark.parametrize("game,K,sims", [("connect4", 4, 64), ("connect4", 2, 64), ("tictactoe", 3, 32)])
def test_cap_changes_nothing_philox(game, K, sims):
    """64 games to the end on a 2-block net, the path the benchmark takes (one select per ply, then an expand per
    step on the device-side row count)."""
    from self_play_reinforcement_learning_amd.engine import SelfPlayEngine

    net = _net(game)
    out = []
    for cap in (0, 2 * K):
        eng = SelfPlayEngine(game, net, n_games=64, iterations=sims, seed=5, search_threads=K, max_games=64)
        out.append(_collect(eng, [eng.arena], cap))
    _assert_same(out[0], out[1], 64)


# ----------------------------------------------------------------------------- tape RNG, the host loop
@functools.lru_cache(maxsize=None)
def _tapes(case):
    """The oracle's per-tree tapes of the case's games (computed once: the CPU replay is the slow part)."""
    game, K, sims, seeds = GPU_TAPE_CASES[case]
    tapes = []
    for i in range(len(seeds)):
        tp, to, _ = g3_tapes(gpu_tape_game(case, i), K)
        tapes += [tp, to]
    return tapes


def _tape_games(case, cap):
    """The games of GPU_TAPE_CASES[case] as slots of one tape-mode arena with the table net, stepped by the host
    loop of the parity tests: a select before every step's rows, and no expand for a step without rows."""
    from self_play_reinforcement_learning_amd.arena import Arena

    game, K, sims, seeds = GPU_TAPE_CASES[case]
    G = len(seeds)
    arena = Arena(game, n_trees=2 * G, n_games=G, iterations=sims, rng="tape", search_threads=K)
    arena.set_sim_cap(cap)
    arena.set_tapes(_tapes(case))
    salts_by_tree = torch.full((2 * G,), 11, dtype=torch.int64, device=arena.device)
    priors = np.stack([np.stack([empty_prior(game, 11)] * 2)] * G)
    arena.games_set_limit(G)
    arena.games_start(list(range(G)), priors=priors)
    records = []

    def step(count):
        if count:
            p, v = _eval_table(arena, salts_by_tree, count)
            arena.expand(p, v)

    for _ in range(64):
        arena.games_begin_ply()
        for _ in range(-(-sims // K)):
            step(arena.select())
        step(arena.games_end_ply())
        _, ring = arena.games_finish_ply(refill=False)
        if ring:
            records.append({k: v.cpu().numpy() for k, v in arena.export_moves(ring).items()})
        if not (arena.games_state()["state"] == 1).any():
            break
    arena.check()
    c, pauses = arena.counters(), arena.sim_pauses()
    arena.close()
    assert c["error_flags"] == 0
    return {k: np.concatenate([r[k] for r in records]) for k in records[0]}, c, pauses


@pytest.fixture(scope="module")
def tape_runs():
    cache = {}

    def get(case, cap):
        if (case, cap) not in cache:
            cache[case, cap] = _tape_games(case, cap)
        return cache[case, cap]

    return get


@pytest.mark.parametrize("case", sorted(GPU_TAPE_CASES))
def test_cap_changes_nothing_tape(case, tape_runs):
    """Tape RNG: the oracle's own draws, so a reordered operation shows as a different game.  The seeds pause in
    the CPU restatement (test_sim_cap_schedule.test_gpu_tape_cases_pause)."""
    K, n = GPU_TAPE_CASES[case][1], len(GPU_TAPE_CASES[case][3])
    _assert_same(tape_runs(case, 0), tape_runs(case, 2 * K), n)


@pytest.mark.parametrize("case", sorted(GPU_TAPE_CASES))
def test_larger_caps_change_nothing_tape(case, tape_runs):
    """cap = 4 K (the other default that was measured) and a cap no launch reaches."""
    K, n = GPU_TAPE_CASES[case][1], len(GPU_TAPE_CASES[case][3])
    m0, c0, _ = tape_runs(case, 0)
    for cap in (4 * K, 1 << 20):
        m1, c1, p1 = _tape_games(case, cap)
        for k in m0:
            np.testing.assert_array_equal(m0[k], m1[k], err_msg=f"{k} cap {cap}")
        for k in GAME_COUNTERS:
            assert c0[k] == c1[k], (k, cap)
        assert cap < (1 << 20) or p1 == 0


# ----------------------------------------------------------------------------- two lanes, cross-lane dedup, cache
def test_cap_changes_nothing_two_lanes_dedup_cache():
    """128 + 128 games on two lanes with leaf dedup, cross-lane dedup and the evaluation cache on: a stashed slot
    has no row, so it must stay out of the dedup table, the owner flags, the peer push and the cache."""
    from self_play_reinforcement_learning_amd.engine import LanedEngine

    net = _net("connect4")
    K, out = 4, []
    for cap in (0, 2 * K):
        eng = LanedEngine("connect4", net, n_games=256, lanes=2, lane_sizes=[128, 128], iterations=64, seed=7,
                          search_threads=K, max_games=256, cross_dedup=True, leaf_dedup=True, eval_cache=1)
        assert eng.cross_dedup and eng.leaf_dedup and eng.eval_cache == 1
        out.append(_collect(eng, [e.arena for e in eng.lanes], cap))
        assert out[-1][1]["cache_rows"] > 0
    _assert_same(out[0], out[1], 256)


# ----------------------------------------------------------------------------- evaluate mode, two networks
def test_cap_changes_nothing_evaluate_mode_per_side_k():
    """Evaluation games between two networks, each side with its own sims in flight (4 and 2) and budget."""
    from self_play_reinforcement_learning_amd.engine import SelfPlayEngine

    net0, net1 = _net("connect4", 0), _net("connect4", 1)
    out = []
    for cap in (0, 8):
        eng = SelfPlayEngine("connect4", net0, n_games=64, iterations=64, seed=9, search_threads=4, max_games=64,
                             evaluate=True, opponent=net1, opponent_iterations=48, opponent_search_threads=2)
        assert eng.evaluator1 is not None and eng.search_threads == 4
        out.append(_collect(eng, [eng.arena], cap))
    _assert_same(out[0], out[1], 64)


# ----------------------------------------------------------------------------- the setter
def test_set_sim_cap_refuses_a_cap_below_2k():
    from self_play_reinforcement_learning_amd._lib import SpmctsError
    from self_play_reinforcement_learning_amd.arena import Arena

    arena = Arena("connect4", n_trees=4, iterations=16, search_threads=4)
    for cap in (1, 4, 7, -1):
        with pytest.raises(SpmctsError):
            arena.set_sim_cap(cap)
    for cap in (0, 8, 9, 16, 1 << 20):
        arena.set_sim_cap(cap)
    assert arena.sim_pauses() == 0
    arena.close()
