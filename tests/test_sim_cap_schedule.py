"""The sim cap's schedule, restated over the oracle (CPU): a tree that has started `cap` sims in one launch
pauses at a sim boundary and the next launch resumes its slot cycle there (csrc/arena_select.h "sim cap",
csrc/arena_expand.h expand_vl_body).  The cycle -- reply slot 0, fill slot 0, reply slot 1, ... -- is
OracleTree.search's, only cut into launches differently, so every episode output must equal the uncapped
oracle's, no search may need more launches than ceil(iterations / K) + 1, and the cases must actually pause.
"""
import hashlib
import pickle

import numpy as np
import pytest

import oracle.selfplay as oracle_selfplay
from oracle.mcts import NumpyRNG, OracleTree
from oracle.table_net import TableNet
from tests.parity_helpers import A_OF

EMPTY, ROW, STASH = 0, 1, 2  # a slot's state between launches (View::need)


class CappedTree(OracleTree):
    """OracleTree whose threaded search runs in launches, as the kernels do.

    launch(rows=False) is k_select_vl (no network outputs: a slot that waits for the network ends the walk),
    launch(rows=True) is k_expand_vl after a network launch (every ROW slot of its start was evaluated).  A
    launch walks the cycle once round from the resume slot: reply the slot if it holds a leaf, then fill it;
    `cap` sims started in the launch pause the tree before the next one, and the evaluated slots the launch
    has not replied yet go to the stash.  select_each_step: the host loops that select before every step's
    rows and skip the expand of a step without rows (tests/parity_helpers.py, MCTreeSearch.search)."""

    cap = 0
    select_each_step = False
    log = None  # shared: dict(pauses, launches, max_launches)

    def search(self):
        K, iters, cap = self.threads, self.iterations, self.cap
        assert K > 1 and (cap == 0 or cap >= 2 * K)
        self._add_noise(self.root)
        slots, state = [None] * K, [EMPTY] * K
        started, res, launches = 0, 0, 0

        def launch(rows):
            nonlocal started, res, launches
            launches += 1
            at_start = list(state)
            start, nst, paused = res, 0, False
            for i in range(K):
                j = (start + i) % K
                res = j
                if not rows and at_start[j] == ROW:
                    break  # not evaluated: the cycle goes on at this reply, in an expand
                if at_start[j] != EMPTY:
                    item, slots[j], state[j] = slots[j], None, EMPTY
                    self._reply_threaded(*item)
                while started < iters:
                    if cap and nst >= cap:
                        paused = True
                        break
                    started += 1
                    nst += 1
                    item = self._select_threaded()
                    if item is not None:
                        slots[j], state[j] = item, ROW
                        break
                if paused:
                    for k in range(i + 1, K):  # evaluated, not yet replied: the outputs go to the stash
                        q = (start + k) % K
                        if rows and at_start[q] == ROW:
                            state[q] = STASH
                    break
            else:
                res = start  # a complete cycle ends where it began
            self.log["pauses"] += int(paused)

        def busy():
            return started < iters or any(s != EMPTY for s in state)

        if self.select_each_step:
            steps = 0
            while busy():
                launch(False)
                if any(s == ROW for s in state):
                    launch(True)
                steps += 1
            self.log["max_steps"] = max(self.log["max_steps"], steps)
        else:
            launch(False)
            while busy():
                launch(True)
            self.log["max_launches"] = max(self.log["max_launches"], launches)
        for c in self.root.children:
            c.noise_active = False


def _episode(game, sims, K, seed, tree_cls):
    A = A_OF[game]
    np.random.seed(seed)
    rng = NumpyRNG()
    orig = oracle_selfplay.OracleTree
    oracle_selfplay.OracleTree = tree_cls
    try:
        r, moves, log, (pol, opp, _) = oracle_selfplay.play_episode(game, TableNet(A, 11), TableNet(A, 11), rng, rng,
                                                                   sims, swap_sides=bool(seed & 1), threads=K)
    finally:
        oracle_selfplay.OracleTree = orig
    return hashlib.sha256(pickle.dumps((r, moves, log))).hexdigest(), (r, moves, log), (pol.stats, opp.stats)


def capped_class(cap, select_each_step=False):
    log = dict(pauses=0, max_launches=0, max_steps=0)
    return type("Capped", (CappedTree,), dict(cap=cap, select_each_step=select_each_step, log=log)), log


# (game, sims, seeds): seeds for which the capped schedule pauses (asserted below)
CASES = {"connect4": (64, (1, 2)), "tictactoe": (32, (1, 2))}


@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("game", ["connect4", "tictactoe"])
def test_capped_schedule_equals_oracle_search(game, K):
    sims, seeds = CASES[game]
    for seed in seeds:
        h0, out0, stats0 = _episode(game, sims, K, seed, OracleTree)
        cls, log = capped_class(2 * K)
        h1, out1, stats1 = _episode(game, sims, K, seed, cls)
        assert h1 == h0 and stats1 == stats0, (game, K, seed)
        assert log["pauses"] > 0, (game, K, seed)
        assert log["max_launches"] <= -(-sims // K) + 1, (game, K, seed, log)
        # the host loops that select before every step and skip the expand of a step without rows
        cls, log = capped_class(2 * K, select_each_step=True)
        h2, _, stats2 = _episode(game, sims, K, seed, cls)
        assert h2 == h0 and stats2 == stats0, (game, K, seed)
        assert log["pauses"] > 0 and log["max_steps"] <= -(-sims // K), (game, K, seed, log)


# The tape-mode games of tests/test_gpu_sim_cap.py (game, K, sims, seeds; game i of a case plays seed seeds[i],
# swap_sides = i odd, table-net salts 11): the GPU test needs launches that pause, which is a condition of the
# test and not a measurement, so it is checked here, on the CPU.
GPU_TAPE_CASES = {
    "ttt_k3": ("tictactoe", 3, 32, tuple(range(100, 164))),
    "c4_k4": ("connect4", 4, 64, tuple(range(200, 212))),
    "c4_k2": ("connect4", 2, 64, tuple(range(300, 308))),  # cap 4: the tightest cap, the resume slot wraps most often
}


def gpu_tape_game(case, i):
    game, K, sims, seeds = GPU_TAPE_CASES[case]
    return dict(game=game, sims=sims, evaluate=False, salt_policy=11, salt_opponent=11, seed=seeds[i],
                swap_sides=bool(i & 1))


@pytest.mark.parametrize("case", sorted(GPU_TAPE_CASES))
def test_gpu_tape_cases_pause(case):
    game, K, sims, seeds = GPU_TAPE_CASES[case]
    cls, log = capped_class(2 * K, select_each_step=True)
    paused_games = 0
    for i, seed in enumerate(seeds):
        before = log["pauses"]
        g = gpu_tape_game(case, i)
        np.random.seed(seed)
        rng = NumpyRNG()
        orig = oracle_selfplay.OracleTree
        oracle_selfplay.OracleTree = cls
        try:
            oracle_selfplay.play_episode(game, TableNet(A_OF[game], 11), TableNet(A_OF[game], 11), rng, rng, sims,
                                         swap_sides=g["swap_sides"], threads=K)
        finally:
            oracle_selfplay.OracleTree = orig
        paused_games += log["pauses"] > before
    assert log["pauses"] > 0 and paused_games >= len(seeds) // 4, (case, log, paused_games)
    assert log["max_steps"] <= -(-sims // K), (case, log)


def test_cap_off_is_the_oracle_schedule():
    """cap 0: the launches are exactly OracleTree.search's rounds (one select, then one expand per round)."""
    cls, log = capped_class(0)
    h0, _, _ = _episode("tictactoe", 32, 4, 3, OracleTree)
    h1, _, _ = _episode("tictactoe", 32, 4, 3, cls)
    assert h0 == h1 and log["pauses"] == 0 and log["max_launches"] <= 32 // 4 + 1
