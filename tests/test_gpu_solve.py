"""GPU: the end-of-game solver's kernels (spmcts_solve_batch) against the host twin -- batch sizes, launch slicing,
a shared table under contention, the node budget -- and solve_to_end / SolveTable / PerfectEvaluator on top."""
import ctypes

import numpy as np
import pytest
import torch

from tests import negamax_helpers as nh
from tests import solve_helpers as sh

pytestmark = pytest.mark.gpu
X, U = sh.X, sh.UNKNOWN
BIG = 1 << 26


def batch(pool, n, start=0):
    """n positions cycling through the pool: boards [n, W, H], players [n], the host twin's codes [n, A]."""
    idx = [(start + i) % len(pool) for i in range(n)]
    return (np.stack([pool[i][0] for i in idx]), np.array([pool[i][1] for i in idx], dtype=np.int8),
            np.stack([pool[i][2] for i in idx]))


def solve(game, boards, players, table=None, **kw):
    from self_play_reinforcement_learning_amd import SolveTable, solve_to_end

    table = table if table is not None else SolveTable(game, entries=1 << 20)
    return solve_to_end(game, boards=boards, players=players, table=table, **kw)


@pytest.mark.parametrize("game", nh.BOARDS)
def test_device_matches_host_twin(game):
    """Batches of 1, 2, 65 and 257 positions: a position's items inside one wave, across two, over many blocks."""
    from self_play_reinforcement_learning_amd import SolveTable

    pool = sh.pool(game)
    assert len(pool) >= 25 and (game == "tictactoe" or len(sh.deep(game)) >= 4)
    table = SolveTable(game, entries=1 << 20)
    for n, start in ((1, 0), (1, len(pool) - 1), (2, 3), (65, 0), (257, 7)):
        boards, players, codes = batch(pool, n, start)
        out = solve(game, boards, players, table, max_nodes=BIG)
        assert out["score"].cpu().numpy().tolist() == codes.tolist(), (game, n)
        assert bool(out["solved"].all()) and bool((out["nodes"] > 0).all())
        again = solve(game, boards, players, table, max_nodes=BIG)  # the table is warm now
        assert torch.equal(again["score"], out["score"])


def test_empty_batch_leaves_outputs_untouched():
    from self_play_reinforcement_learning_amd import SolveTable, _lib
    from self_play_reinforcement_learning_amd.arena import GAMES

    gid, W, H, A = GAMES["connect4"]
    table = SolveTable("connect4", entries=1 << 16)
    score = torch.full((3, A), 77, dtype=torch.int8, device="cuda")
    nodes = torch.full((3,), 5, dtype=torch.int64, device="cuda")
    rc = _lib.lib().spmcts_solve_batch(gid, W, H, None, None, 0, _lib.ptr(table.data), table.entries, None, 1000, 0,
                                       _lib.ptr(score), _lib.ptr(nodes), None)
    torch.cuda.synchronize()
    assert rc == 0 and bool((score == 77).all()) and bool((nodes == 5).all()) and not bool(table.data.any())
    out = solve("connect4", np.zeros((0, W, H), np.int8), np.zeros(0, np.int8), table)
    assert out["score"].shape == (0, A) and out["solved"].shape == (0,) and out["launches"] == 0


def hard(game, least=2000):
    """The deep positions whose host search is long enough to be cut into many launches."""
    return [p for p in sh.deep(game) if p[3] >= least]


@pytest.mark.parametrize("game", sh.GRAVITY)
def test_launch_slicing(game):
    """Slices of 32 steps: a position of >= 2000 moves over at most 64 items takes many launches.  The codes are
    the default slice's and each position's alone; alone on a cleared table (one wave, no other writer) the node
    count is the single-slice run's."""
    from self_play_reinforcement_learning_amd import SolveTable

    pool = hard(game) + sh.pool(game)
    assert hard(game)
    boards, players, codes = batch(pool, 65)
    table = SolveTable(game, entries=1 << 18)
    sliced = solve(game, boards, players, table, max_nodes=BIG, launch_nodes=32)
    assert sliced["launches"] >= 3
    assert sliced["score"].cpu().numpy().tolist() == codes.tolist()
    table.clear()
    whole = solve(game, boards, players, table, max_nodes=BIG)
    assert torch.equal(whole["score"], sliced["score"]) and whole["launches"] < sliced["launches"]
    for i in range(min(65, len(pool))):  # each position of the batch alone, on the table the batch left
        alone = solve(game, boards[i:i + 1], players[i:i + 1], table, max_nodes=BIG, launch_nodes=32)
        assert alone["score"].cpu().numpy()[0].tolist() == codes[i].tolist(), (game, i)
    for board, player, code, nodes in hard(game)[:3]:
        table.clear()
        one = solve(game, board[None], np.array([player], np.int8), table, max_nodes=BIG)
        table.clear()
        cut = solve(game, board[None], np.array([player], np.int8), table, max_nodes=BIG, launch_nodes=32)
        assert cut["launches"] >= 3 and cut["launches"] > one["launches"]
        assert one["score"].cpu().numpy()[0].tolist() == code.tolist() == cut["score"].cpu().numpy()[0].tolist()
        assert int(one["nodes"][0]) == int(cut["nodes"][0]) > 0


@pytest.mark.parametrize("game", sh.GRAVITY)
def test_shared_table_under_contention(game):
    """257 copies of eight deep positions on a table of 2^16 entries: every copy gets the host twin's codes."""
    from self_play_reinforcement_learning_amd import SolveTable

    eight = sorted(sh.deep(game), key=lambda p: -p[3])[:8]
    assert len(eight) == 8
    boards, players, codes = batch(eight, 8 * 257)
    out = solve(game, boards, players, SolveTable(game, entries=1 << 16), max_nodes=BIG)
    assert bool(out["solved"].all())
    assert out["score"].cpu().numpy().tolist() == codes.tolist()


@pytest.mark.parametrize("game", sh.GRAVITY)
def test_budget(game):
    """A budget below the hardest position's count and above the others': exactly the hardest gives up (the call
    returns), with -127 on the moves it did not finish and nothing wrong on the rest.  The budget is an eighth of
    the hardest position's host count; the others are those the host solves in a thirty-second of it (the
    device's items share less than the host's sequential ones, so its counts run higher: the factor 4 is the
    margin for that, and the slices of 64 steps bound the overshoot to 64 moves per item)."""
    from self_play_reinforcement_learning_amd import SolveTable

    deep = sorted(sh.deep(game), key=lambda p: -p[3])
    hardest = deep[0]
    budget = hardest[3] // 8
    easy = [p for p in deep[1:] if p[3] * 32 <= hardest[3]]
    assert budget >= 1000 and len(easy) >= 3
    pool = easy[:5] + [hardest] + easy[5:10]
    boards, players, codes = batch(pool, len(pool))
    out = solve(game, boards, players, SolveTable(game, entries=1 << 20), max_nodes=budget, launch_nodes=64)
    k = min(5, len(easy))
    solved = out["solved"].cpu().numpy()
    score = out["score"].cpu().numpy()
    print("budget", budget, "host", [p[3] for p in pool], "device", out["nodes"].tolist())
    assert solved.tolist() == [i != k for i in range(len(pool))]
    assert (score[k] == U).any() and all(s in (c, U) for s, c in zip(score[k], codes[k]))
    assert np.delete(score, k, 0).tolist() == np.delete(codes, k, 0).tolist()
    assert int(out["nodes"][k]) >= budget


def test_solve_to_end_and_table():
    from self_play_reinforcement_learning_amd import SolveTable, solve_to_end

    from self_play_reinforcement_learning_amd.solve import positions_to_boards

    seqs = sh.move_lists("connect4", 28, 1, seed=2) + sh.move_lists("connect4", 31, 1, seed=3)
    table = SolveTable("connect4", entries=1 << 20)
    a = solve_to_end("connect4", positions=seqs, table=table)
    boards, players = positions_to_boards("connect4", seqs)
    assert players.tolist() == [1, -1]
    b = solve_to_end("connect4", boards=boards, players=players, table=table)
    for k, dtype, shape in (("score", torch.int8, (2, 7)), ("value", torch.int8, (2,)), ("best", torch.bool, (2, 7)),
                            ("nodes", torch.int64, (2,)), ("solved", torch.bool, (2,)), ("outcome", torch.int8, (2,))):
        assert a[k].dtype == dtype and tuple(a[k].shape) == shape and a[k].is_cuda, k
        if k != "nodes":
            assert torch.equal(a[k], b[k]), k
    for i in range(2):
        codes, _ = sh.host_solve("connect4", boards[i], int(players[i]))
        assert a["score"][i].cpu().numpy().tolist() == codes.tolist()
        v, best = sh.value_of(codes)
        assert int(a["value"][i]) == v and a["best"][i].nonzero().reshape(-1).tolist() == best
        assert int(a["outcome"][i]) == (v > 0) - (v < 0)
    with pytest.raises(ValueError):
        solve_to_end("connect4_6_5", boards=np.zeros((1, 6, 5), np.int8), players=[1], table=table)  # another board's
    with pytest.raises(ValueError):
        solve_to_end("connect4", positions=seqs, boards=boards, players=players)
    with pytest.raises(ValueError):
        solve_to_end("connect4", boards=boards)
    with pytest.raises(ValueError):
        solve_to_end("connect4", boards=nh.drawn_board("connect4")[None], players=[1])
    table.clear()
    assert not bool(table.data.any())
    # the C entry point refuses a finished position too
    from self_play_reinforcement_learning_amd import _lib
    from self_play_reinforcement_learning_amd.arena import GAMES

    gid, W, H, A = GAMES["connect4"]
    bad = torch.as_tensor(np.stack([boards[0], nh.drawn_board("connect4")])).cuda()
    pl = torch.ones(2, dtype=torch.int8, device="cuda")
    size = ctypes.c_uint64()
    _lib.call("spmcts_solve_work_bytes", gid, W, H, 2, ctypes.byref(size))
    work = torch.empty(size.value, dtype=torch.uint8, device="cuda")
    score = torch.zeros((2, A), dtype=torch.int8, device="cuda")
    rc = _lib.lib().spmcts_solve_batch(gid, W, H, _lib.ptr(bad), _lib.ptr(pl), 2, _lib.ptr(table.data), table.entries,
                                       _lib.ptr(work), 1000, 0, _lib.ptr(score), None, None)
    assert rc == -3 and b"position 1" in _lib.lib().spmcts_last_error()


def test_perfect_evaluator():
    """A 2-block net, 16 positions of 7x6 with at most 14 empty cells, 8 simulations: the counts are
    perfect_report's on analyse_positions and solve_to_end run separately; the base_network line is the raw
    policy's argmax."""
    from self_play_reinforcement_learning_amd import (MCTreeSearch, PerfectEvaluator, analyse_positions, perfect_report,
                                                      solve_to_end)
    from self_play_reinforcement_learning_amd.envs import Connect4Env
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    rng = np.random.default_rng(3)
    lines = []
    while len(lines) < 24:
        env = nh.make_env("connect4")
        env.reset()
        player, done, moves = 1, False, []
        for _ in range(int(rng.integers(28, 35))):
            a = int(rng.choice(np.flatnonzero(env.valid_moves())))
            _, _, done, _ = env.step(a, player)
            moves.append(a)
            if done:
                break
            player = -player
        if not done:
            lines.append("".join(str(a + 1) for a in moves) + " 0")
    torch.manual_seed(0)
    net = ResidualTower(7, 6, 7, num_blocks=2, filter_factor=32).cuda().eval()
    policy = MCTreeSearch(network=net, env=Connect4Env, iterations=8, seed=4, update_nn=False)
    ev = PerfectEvaluator(policy, lines, seed=11)
    res = ev.test(num_pos=16, base_network=True)
    assert [r["base_network"] for r in res] == [True, False]
    games = ev.last[False]["games"]
    assert len(games) == 16 and all(len(g) >= 28 for g in games)
    solved = solve_to_end("connect4", positions=games)
    assert bool(solved["solved"].all())
    search = analyse_positions("connect4", net, games, **ev._search_kwargs())
    rep = perfect_report(solved["score"], search["action"])
    assert (res[1]["total"], res[1]["n_solved"], res[1]["n_unsolved"]) == (rep["n_strong"], 16, 0)
    assert res[1]["line"] == f"{rep['n_strong']} correct moves out of 16: base_network = False"
    from self_play_reinforcement_learning_amd.solve import positions_to_boards

    boards, players = positions_to_boards("connect4", games)
    with torch.no_grad():
        probs = net.forward(torch.as_tensor(boards).long() * torch.as_tensor(players).long().reshape(-1, 1, 1))[0]
    raw = probs.argmax(dim=1)
    assert torch.equal(ev.last[True]["action"].cpu(), raw.cpu())
    legal = solved["score"].gather(1, raw.reshape(-1, 1).to(solved["score"].device)).reshape(-1) != X
    right = solved["best"].gather(1, raw.reshape(-1, 1).to(solved["score"].device)).reshape(-1) & legal
    assert res[0]["total"] == int(right.sum()) and res[0]["line"].startswith(f"{int(right.sum())} correct moves out of 16")
    weak = ev.test(num_pos=16, weak=True)
    assert weak[0]["total"] >= 0 and weak[0]["n_solved"] == 16
    assert ev.compare(lines[0].split(" ")[0]) in (0, 1)
