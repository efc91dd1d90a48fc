"""GPU: the batched self-play engine and the MCTreeSearch facade with real networks.

Properties that hold at any size: every exported Move is a legal position of
the owner's frame with a visit distribution over legal actions summing to 1,
z in {-1, 0, 1} with the two trees of a game holding opposite results, the
device counters balance (every simulation either reached the network or a
terminal leaf), and no device error flag is raised.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _legal(game, board):
    W, H = board.shape
    if game == "connect4":
        return (np.abs(board).sum(axis=1) < H)
    return board.reshape(-1) == 0


@pytest.mark.parametrize("game,n_games,sims,ff,blocks", [("connect4", 64, 16, 4, 1), ("tictactoe", 64, 25, 4, 1),
                                                         ("connect4", 512, 8, 8, 2)])
@pytest.mark.parametrize("threads", [1, 4])
def test_engine_selfplay_invariants(game, n_games, sims, ff, blocks, threads):
    from self_play_reinforcement_learning_amd.engine import SelfPlayEngine
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    torch.manual_seed(0)
    W, H, A = (7, 6, 7) if game == "connect4" else (3, 3, 9)
    net = ResidualTower(W, H, A, num_blocks=blocks, filter_factor=ff)
    eng = SelfPlayEngine(game, net, n_games=n_games, iterations=sims, seed=1, max_games=2 * n_games,
                         search_threads=threads)  # threads > 1: virtual-loss search (mcts.py:328-331)
    assert eng.select_steps == -(-sims // threads)
    got = []
    eng.run(games=2 * n_games, on_moves=lambda m: got.append({k: v.cpu().numpy() for k, v in m.items()}))
    eng.check()
    c = eng.counters()
    assert c["error_flags"] == 0
    assert c["games_finished"] == 2 * n_games
    assert c["sims"] > 0 and c["depth_sum"] >= c["sims"]
    # every search runs exactly `iterations` search_node calls: completed or leaked (mcts.py:349-354)
    assert c["sims"] + c["leaked_sims"] == sims * c["moves"]
    assert threads > 1 or c["leaked_sims"] == 0
    moves = {k: np.concatenate([g[k] for g in got]) for k in got[0]}
    assert len(moves["z"]) == c["positions_exported"] == c["moves"]
    assert set(np.unique(moves["z"]).tolist()) <= {-1.0, 0.0, 1.0}
    np.testing.assert_allclose(moves["tree_probs"].sum(1), 1.0, atol=1e-5)
    for i in range(len(moves["z"])):
        b = moves["state"][i].reshape(W, H).astype(int)
        legal = _legal(game, b)
        assert (moves["tree_probs"][i][~legal] == 0).all()
        # the owner is to move: equal piece counts (owner moved first) or one fewer
        assert (b == 1).sum() in ((b == -1).sum(), (b == -1).sum() - 1)
    # per game the two trees hold opposite results; a draw is 0 for both
    for gid in np.unique(moves["game"]):
        zs = np.unique(moves["z"][moves["game"] == gid])
        assert len(zs) <= 2 and (len(zs) == 1 and zs[0] == 0 or sorted(zs.tolist()) == [-1.0, 1.0] or len(zs) == 1)
    res = np.array(c["results"])
    assert res.sum() == 2 * n_games


def test_mcts_facade_matches_reference_search():
    """MCTreeSearch (one-tree arena) driven through the reference protocol, tape RNG + table net."""
    from oracle.table_net import TableNet  # noqa: F401  (checker only)
    from self_play_reinforcement_learning_amd.envs import Connect4Env
    from self_play_reinforcement_learning_amd.evaluator import DeviceTableNet
    from self_play_reinforcement_learning_amd.mcts import MCTreeSearch
    from tests.parity_helpers import g2_tape, load_json

    cases = [c for c in load_json("mcts_search.json") if c["game"] == "connect4" and c["sims"] == 25][:6]
    for c in cases:
        net = DeviceTableNet("connect4", salt=c["salt"])
        tree = MCTreeSearch(network=net, env_gen=Connect4Env, iterations=c["sims"], rng="tape", memory_queue=None)
        tree._arena.set_tapes([g2_tape(c)])
        tree.reset()
        for a in c["opening"]:
            tree.play_action(a, None)
        assert tree.root_node.player == c["root_player"]
        a = tree()
        root = tree.root_node
        assert a == c["action"]
        assert [ch.n for ch in root.children] == c["child_n"]
        assert [ch.w for ch in root.children] == c["child_w"]
        mv = tree.temp_memory[-1]
        assert mv.state.reshape(-1).tolist() == c["state"]
        assert mv.tree_probs.tolist() == c["tree_probs"]
        assert float(mv.q) == c["q"]


def test_mcts_facade_with_resnet_plays_full_game():
    from self_play_reinforcement_learning_amd.envs import Connect4Env
    from self_play_reinforcement_learning_amd.mcts import MCTreeSearch
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    torch.manual_seed(0)
    net = ResidualTower(7, 6, 7, num_blocks=1, filter_factor=4)

    class Q(list):
        def put(self, x):
            self.append(x)

    q = Q()
    p1 = MCTreeSearch(network=net, env=Connect4Env, iterations=20, memory_queue=q, seed=3)
    p2 = MCTreeSearch(network=net, env=Connect4Env, iterations=20, memory_queue=q, seed=4)
    env = Connect4Env()
    env.reset()
    p1.reset(1)
    p2.reset(-1)
    player, done, r = 1, False, 0
    while not done:
        pol = p1 if player == 1 else p2
        a = pol()
        p1.play_action(a, player)
        p2.play_action(a, -player)
        _, r, done, _ = env.step(a, player)
        r *= player
        player = -player
    p1.push_to_queue(done=True, r=r)
    p2.push_to_queue(done=True, r=-r)
    assert len(q) > 0 and all(m.state.shape == (7, 6) for m in q)


def test_mcts_search_after_update_uses_new_weights():
    """The reference searches with the updated network at once (its leaves call the module,
    mcts.py:316): after update_from_memory (or load_state_dict) the next search's leaf evaluations
    use the new weights, without waiting for a reset."""
    from self_play_reinforcement_learning_amd.envs import Connect4Env
    from self_play_reinforcement_learning_amd.evaluator import HipTowerEvaluator
    from self_play_reinforcement_learning_amd.mcts import MCTreeSearch, Move
    from self_play_reinforcement_learning_amd.memory import Memory
    from self_play_reinforcement_learning_amd.modules import ResidualTower, planes_from_boards

    torch.manual_seed(0)
    net = ResidualTower(7, 6, 7, num_blocks=2, filter_factor=32).cuda()
    optim = torch.optim.SGD(net.parameters(), lr=0.5)
    pol = MCTreeSearch(network=net, env=Connect4Env, iterations=16, optim=optim, batch_size=8, min_memory=8, seed=1)
    assert isinstance(pol._evaluator, HipTowerEvaluator)
    pol.reset(1)
    pol()
    x = planes_from_boards(torch.randint(-1, 2, (64, 7, 6)), 7, 6).cuda().to(torch.bfloat16)
    x = x.contiguous(memory_format=torch.channels_last)
    before, _ = pol._evaluator(x)
    pol.memory = Memory(100)
    for i in range(16):
        pol.memory.add(Move(torch.randint(-1, 2, (7, 6)), torch.tensor(1.0), torch.full((7,), 1 / 7), torch.tensor(0.0)))
    pol.update_from_memory()  # one SGD step changes the module's weights
    pol()  # no reset in between: the search must see them
    after, _ = pol._evaluator(x)
    fresh, _ = HipTowerEvaluator(net, dtype=pol._evaluator.dtype)(x)
    assert not torch.equal(before, after)
    assert torch.equal(after, fresh)


def test_trainer_steps_overlap_without_host_sync(tmp_path):
    """_Trainer.step() queues the SGD update on its own stream and returns a device tensor (no host
    synchronisation); after sync() the weights equal those of the same steps run synchronously."""
    from self_play_reinforcement_learning_amd.modules import ResidualTower
    from self_play_reinforcement_learning_amd.self_play_parallel import _Trainer

    rows = dict(state=torch.randint(-1, 2, (200, 42), dtype=torch.int8), tree_probs=torch.full((200, 7), 1 / 7),
                q=torch.zeros(200, dtype=torch.float64), z=torch.ones(200))
    out = []
    for overlap in (True, False):
        torch.manual_seed(0)
        net = ResidualTower(7, 6, 7, num_blocks=1, filter_factor=8).cuda()
        tr = _Trainer(net, torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.9), memory_size=1000, batch_size=16,
                      min_memory=0, q_average=True, device="cuda", overlap=overlap)
        tr.memory.add_moves(rows)
        torch.manual_seed(5)
        losses = [tr.step() for _ in range(4)]
        if overlap:
            assert tr.stream is not None and all(isinstance(x, torch.Tensor) for x in losses)
            tr.sync()
        assert tr.steps == 4
        torch.cuda.synchronize()
        out.append({k: v.clone() for k, v in net.state_dict().items()})
    for k in out[0]:  # same steps in the same order (backward kernels may differ in reduction order)
        torch.testing.assert_close(out[0][k], out[1][k], rtol=1e-4, atol=1e-6, msg=k)


@pytest.mark.parametrize("autocast", [False, True])
def test_trainer_graph_matches_eager_steps(autocast):
    """The captured-graph update (_Trainer(graph=True): forward, AZ loss, backward and the SGD step as
    one HIP graph replayed per step) gives the weights of the same updates run eagerly, step for step:
    3 eager warm-up steps, the capture, replays; a learning-rate change (ReduceLROnPlateau) re-captures
    and the new rate takes effect.  Eval-mode dropout (the masks' RNG is drawn differently inside a graph).
    With MIOpen's default algorithm choice two EAGER runs differ (atomics in the fp16 backward kernels:
    up to 5 % of an update, profiles/r04/trainer/determinism_default.json); with deterministic
    algorithms requested, eager, replayed and repeated runs are bit-identical
    (determinism_deterministic.json), so the test asks for them and compares bit for bit."""
    from self_play_reinforcement_learning_amd.modules import ResidualTower
    from self_play_reinforcement_learning_amd.self_play_parallel import _Trainer

    det = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        _graph_vs_eager(autocast, _Trainer, ResidualTower)
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = det


def _graph_vs_eager(autocast, _Trainer, ResidualTower):
    g = torch.Generator().manual_seed(7)
    rows = dict(state=torch.randint(-1, 2, (512, 42), dtype=torch.int8, generator=g),
                tree_probs=torch.softmax(torch.randn(512, 7, generator=g), 1),
                q=torch.rand(512, dtype=torch.float64, generator=g) - 0.5,
                z=torch.randint(-1, 2, (512,), generator=g).float())
    out, batches = [], None
    for graph in (False, True):
        torch.manual_seed(0)
        net = ResidualTower(7, 6, 7, num_blocks=2, filter_factor=16).cuda()
        opt = torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
        tr = _Trainer(net, opt, memory_size=1000, batch_size=64, min_memory=0, q_average=True, device="cuda",
                      overlap=False, autocast=autocast, train_mode=False, graph=graph)
        tr.memory.add_moves(rows)
        if batches is None:
            torch.manual_seed(11)
            batches = [tr.memory.sample_batch(64) for _ in range(10)]
        losses = []
        for i, b in enumerate(batches):
            if i == 6:
                opt.param_groups[0]["lr"] = 0.002  # as ReduceLROnPlateau does
            losses.append(float(tr._step_graphed(*b) if graph else tr._train_step(*b)))
        torch.cuda.synchronize()
        if graph:
            assert tr.graph_captures == 2  # steps 3 and 9 (after 3 eager steps each time)
        out.append(({k: v.clone() for k, v in net.state_dict().items()}, losses))
    (w0, l0), (w1, l1) = out
    assert all(math.isfinite(x) for x in l1)
    assert l0 == l1, (l0, l1)
    for k in w0:
        assert torch.equal(w0[k], w1[k]), k


def test_trainer_graph_train_mode_replays_run():
    """In train mode (dropout, BatchNorm batch statistics) every replay is a real update: the weights
    move on each step and BatchNorm's step counter counts every step, eager and replayed."""
    from self_play_reinforcement_learning_amd.modules import ResidualTower
    from self_play_reinforcement_learning_amd.self_play_parallel import _Trainer

    torch.manual_seed(0)
    net = ResidualTower(7, 6, 7, num_blocks=2, filter_factor=16).cuda()
    tr = _Trainer(net, torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.9), memory_size=1000, batch_size=64,
                  min_memory=0, q_average=True, device="cuda", overlap=True, autocast=True)
    g = torch.Generator().manual_seed(1)
    tr.memory.add_moves(dict(state=torch.randint(-1, 2, (256, 42), dtype=torch.int8, generator=g),
                             tree_probs=torch.full((256, 7), 1 / 7), q=torch.zeros(256, dtype=torch.float64),
                             z=torch.randint(-1, 2, (256,), generator=g).float()))
    prev = net.conv1.weight.detach().clone()
    losses, moved, nonfinite = [], [], []
    for i in range(8):
        loss = tr.step()
        tr.sync()
        torch.cuda.synchronize()
        losses.append(float(loss))
        moved.append(not torch.equal(prev, net.conv1.weight))
        nonfinite.append([n for n, p in net.named_parameters() if not torch.isfinite(p).all()][:3])
        prev = net.conv1.weight.detach().clone()
    assert all(math.isfinite(x) for x in losses) and not any(nonfinite), (losses, nonfinite)
    assert all(moved), moved
    assert tr.graph_captures == 1 and int(net.bn1.num_batches_tracked) == 8


def test_trainer_autocast_matches_fp32_steps():
    """_Trainer(autocast=True) runs the update under fp16 autocast as the reference's UpdateWorker
    (updateworker.py:147-149, no GradScaler), and the scheduler turns it on by default
    (train_autocast=True).  On one batch and the same starting weights (eval-mode dropout): the loss is
    within fp16 rounding of the fp32 loss, and the SGD update points the same way (cosine of the
    weight deltas)."""
    import inspect

    from self_play_reinforcement_learning_amd.modules import ResidualTower
    from self_play_reinforcement_learning_amd.self_play_parallel import SelfPlayScheduler, _Trainer

    assert inspect.signature(SelfPlayScheduler).parameters["train_autocast"].default is True
    g = torch.Generator().manual_seed(3)
    rows = dict(state=torch.randint(-1, 2, (256, 42), dtype=torch.int8, generator=g),
                tree_probs=torch.softmax(torch.randn(256, 7, generator=g), 1),
                q=torch.rand(256, dtype=torch.float64, generator=g) - 0.5,
                z=torch.randint(-1, 2, (256,), generator=g).float())
    loss, delta, batch = {}, {}, None
    for ac in (False, True):
        torch.manual_seed(0)
        net = ResidualTower(7, 6, 7, num_blocks=2, filter_factor=16).cuda()
        w0 = torch.cat([p.detach().reshape(-1).clone() for p in net.parameters()])
        tr = _Trainer(net, torch.optim.SGD(net.parameters(), lr=0.01, momentum=0.9), memory_size=1000, batch_size=64,
                      min_memory=0, q_average=True, device="cuda", overlap=False, autocast=ac,
                      train_mode=False)  # no dropout masks (their RNG differs between the dtypes)
        assert tr.autocast is ac
        tr.memory.add_moves(rows)
        if batch is None:
            batch = tr.memory.sample_batch(64)
        loss[ac] = tr.train_batch(*batch)
        delta[ac] = torch.cat([p.detach().reshape(-1) for p in net.parameters()]) - w0
    assert math.isfinite(loss[True]) and abs(loss[True] - loss[False]) < 5e-3 * abs(loss[False]), loss
    cos = torch.nn.functional.cosine_similarity(delta[True].double(), delta[False].double(), dim=0).item()
    assert cos > 0.99, cos


@pytest.mark.parametrize("lanes", [1, 2])
def test_scheduler_train_model_dropin(tmp_path, lanes):
    """run_self_play_connect4.py-style use (stale env_gen=/self_play= kwargs) trains and checkpoints,
    with one arena or two lanes (LanedEngine)."""
    from self_play_reinforcement_learning_amd import (Connect4Env, MCTreeSearch, ModelContainer, ResidualTower,
                                                      SelfPlayScheduler)

    torch.manual_seed(0)
    network = ResidualTower(width=7, height=6, action_size=7, num_blocks=1, filter_factor=4)
    policy_kwargs = dict(iterations=8, min_memory=64, memory_size=3000, env_gen=Connect4Env, batch_size=32)
    container = ModelContainer(policy_gen=MCTreeSearch, policy_kwargs=policy_kwargs)
    sp = SelfPlayScheduler(env=Connect4Env, network=network, policy_container=container,
                           evaluation_policy_container=None, initial_games=16, epoch_length=24, evaluation_games=0,
                           save_dir=str(tmp_path), self_play=True, stagger=True, stagger_mem_step=100, lr=0.005,
                           n_games=16, lanes=lanes)
    sp.train_model(2)
    assert len(getattr(sp.engine, "lanes", [sp.engine])) == lanes
    assert sp.engine.search_threads == 4  # inference_proxy=True: thread_count (default 4) sims in flight
    saves = sorted(p for p in (tmp_path / sp.start_time).iterdir() if p.name.startswith("model-"))
    assert len(saves) == 2
    ck = torch.load(saves[-1], weights_only=True)
    assert list(ck["model"].keys()) == list(network.state_dict().keys())
    assert len(sp.trainer.memory) > 0
    assert sp.engine.games_done == 16 + 2 * 24
    m = sp.trainer.memory.sample(4)
    assert m[0].state.shape == (7, 6) and m[0].tree_probs.shape == (7,) and m[0].actual_val.dtype == torch.float32


def test_scheduler_spawns_rank_processes(tmp_path, monkeypatch):
    """SelfPlayScheduler(gpus=2) outside torchrun starts its own two rank processes (the reference's
    scheduler starts its worker processes itself, self_play_parallel.py:95-171); rehearsed on the box's
    one GPU over gloo (RCCL refuses two ranks per GPU).  Both ranks play their share, rank 0 owns the
    replay and checkpoints, and the parent's network holds the final checkpoint afterwards; then
    compare_models shards its games over two ranks and returns the parent's parse_results."""
    from self_play_reinforcement_learning_amd import (Connect4Env, MCTreeSearch, ModelContainer, OneStepLookahead,
                                                      ResidualTower, SelfPlayScheduler)

    monkeypatch.setenv("SPMCTS_ALLOW_OVERSUBSCRIBE", "1")
    monkeypatch.setenv("SPMCTS_DIST_BACKEND", "gloo")
    torch.manual_seed(0)
    network = ResidualTower(width=7, height=6, action_size=7, num_blocks=1, filter_factor=4)
    before = {k: v.clone() for k, v in network.state_dict().items()}
    container = ModelContainer(policy_gen=MCTreeSearch, policy_kwargs=dict(iterations=8, min_memory=32, memory_size=3000,
                                                                           env=Connect4Env, batch_size=16))
    ev = ModelContainer(policy_gen=OneStepLookahead, policy_kwargs=dict(env=Connect4Env))
    sp = SelfPlayScheduler(env=Connect4Env, network=network, policy_container=container, evaluation_policy_container=ev,
                           initial_games=8, epoch_length=16, evaluation_games=0, save_dir=str(tmp_path), lr=0.005,
                           n_games=8, gpus=2)
    sp.train_model(1)
    saves = sorted(p for p in (tmp_path / sp.start_time).iterdir() if p.name.startswith("model-"))
    assert len(saves) == 1
    ck = torch.load(saves[-1], weights_only=True)
    for k, v in network.state_dict().items():
        assert torch.equal(v.cpu(), ck["model"][k].cpu()), k
    assert any(not torch.equal(before[k], v.cpu()) for k, v in network.state_dict().items())
    total, breakdown = sp.compare_models(gpus=2)
    assert sum(v for side in breakdown.values() for v in side.values()) == 16
    assert sum(breakdown["first"].values()) == 8 and sum(breakdown["second"].values()) == 8


def _tower(seed, blocks=2, ff=32):
    torch.manual_seed(seed)
    return ResidualTowerCls()(7, 6, 7, num_blocks=blocks, filter_factor=ff).cuda().eval()


def ResidualTowerCls():
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    return ResidualTower


def _run_engine(**kw):
    from self_play_reinforcement_learning_amd.engine import SelfPlayEngine

    async_device = kw.pop("async_device", True)
    eng = SelfPlayEngine("connect4", **kw)
    eng.async_device = async_device
    got = []
    eng.run(games=kw["max_games"], on_moves=lambda m: got.append({k: v.cpu().numpy() for k, v in m.items()}))
    eng.check()
    moves = {k: np.concatenate([g[k] for g in got]) for k in got[0]} if got else None
    return eng, moves, eng.counters()


@pytest.mark.parametrize("opp_iters", [12, 20])
def test_two_network_arena_async_matches_sync(opp_iters):
    """Evaluation games between two fused-tower networks (row segments per network, per-player
    iteration budgets): the device-count loop equals the host-synchronised loop exactly."""
    a, b = _tower(0), _tower(1)
    out = []
    for async_device in (True, False):
        eng, moves, c = _run_engine(network=a, opponent=b, opponent_iterations=opp_iters, n_games=40, iterations=12,
                                    seed=5, max_games=40, evaluate=True, async_device=async_device)
        assert eng.evaluator1 is not None and eng.arena.seg1 == 40
        out.append((moves, c))
    (m1, c1), (m2, c2) = out
    for k in m1:
        np.testing.assert_array_equal(m1[k], m2[k], err_msg=k)
    for k in ("sims", "moves", "nn_leaves", "terminal_leaves", "depth_sum", "games_finished", "results"):
        assert c1[k] == c2[k], k
    assert c1["games_finished"] == 40


def test_two_network_arena_uses_each_network():
    """Swapping in the same network as the opponent gives the self-play results; a different
    opponent network changes them."""
    a, b = _tower(0), _tower(1)
    _, m_self, c_self = _run_engine(network=a, n_games=32, iterations=10, seed=9, max_games=32)
    _, m_same, c_same = _run_engine(network=a, opponent=_tower(0), n_games=32, iterations=10, seed=9, max_games=32)
    _, m_diff, _ = _run_engine(network=a, opponent=b, n_games=32, iterations=10, seed=9, max_games=32)
    for k in m_self:
        np.testing.assert_array_equal(m_self[k], m_same[k], err_msg=k)
    assert c_self["results"] == c_same["results"]
    assert m_self["z"].shape != m_diff["z"].shape or not np.array_equal(m_self["tree_probs"], m_diff["tree_probs"])


@pytest.mark.parametrize("opponent", ["random", "lookahead"])
def test_hardcoded_opponents_on_device(opponent):
    a = _tower(0)
    eng, moves, c = _run_engine(network=a, opponent=opponent, n_games=64, iterations=8, seed=2, max_games=64,
                                evaluate=True)
    assert c["games_finished"] == 64 and c["error_flags"] == 0
    assert np.array(c["results"]).sum() == 64
    # only the policy's moves are recorded; the policy's tree searched every one of its plies
    assert c["moves"] == moves["z"].shape[0] == c["positions_exported"]
    for gid in np.unique(moves["game"]):
        assert len(np.unique(moves["z"][moves["game"] == gid])) == 1


def test_compare_models_dropin(tmp_path):
    """compare_models (self_play_parallel.py:355-379) with a second MCTreeSearch network and with a
    hard-coded evaluation player: (total_rewards, breakdown) over epoch_length games."""
    from self_play_reinforcement_learning_amd import (Connect4Env, MCTreeSearch, ModelContainer, OneStepLookahead,
                                                      SelfPlayScheduler)

    a, b = _tower(0), _tower(1)
    for ev in (ModelContainer(policy_gen=MCTreeSearch, policy_kwargs=dict(iterations=6, env=Connect4Env)),
               ModelContainer(policy_gen=OneStepLookahead, policy_kwargs=dict(env=Connect4Env))):
        container = ModelContainer(policy_gen=MCTreeSearch, policy_kwargs=dict(iterations=8, env=Connect4Env))
        sp = SelfPlayScheduler(policy_container=container, env=Connect4Env, network=a, evaluation_policy_container=ev,
                               evaluation_network=b, epoch_length=30, save_dir=str(tmp_path), n_games=16)
        total, breakdown = sp.compare_models()
        n = sum(v for side in breakdown.values() for v in side.values())
        assert n == 30
        assert total == sum(s["wins"] - s["losses"] for s in breakdown.values())
        assert sum(breakdown["first"].values()) == 15 and sum(breakdown["second"].values()) == 15


def test_compare_models_per_side_settings(tmp_path):
    """The evaluation MCTreeSearch keeps its own kwargs (selfplayworker.py:71-81 builds it from its own
    container): alpha, strong_play and thread_count reach the opponent's trees (spmcts_set_tree_search)
    instead of being overridden by the policy's; the search runs enough network steps for the side
    with fewer sims in flight."""
    from self_play_reinforcement_learning_amd import Connect4Env, MCTreeSearch, ModelContainer, SelfPlayScheduler

    a, b = _tower(0), _tower(1)
    ev = ModelContainer(policy_gen=MCTreeSearch, policy_kwargs=dict(iterations=9, env=Connect4Env, alpha=0.3,
                                                                    strong_play=True, thread_count=1))
    container = ModelContainer(policy_gen=MCTreeSearch, policy_kwargs=dict(iterations=8, env=Connect4Env))
    sp = SelfPlayScheduler(policy_container=container, env=Connect4Env, network=a, evaluation_policy_container=ev,
                           evaluation_network=b, epoch_length=20, save_dir=str(tmp_path), n_games=10)
    assert (sp._search_threads, sp._opponent_threads) == (4, 1)
    net, kw = sp._opponent()
    assert net is b and kw == dict(opponent_iterations=9, opponent_alpha=0.3, opponent_strong_play=True,
                                   opponent_search_threads=1)
    eng, _ = sp._evaluation_engine(20)
    assert eng.search_threads == 4 and eng.select_steps == max(-(-8 // 4), 9)
    eng.arena.close()
    total, breakdown = sp.compare_models()
    assert sum(v for side in breakdown.values() for v in side.values()) == 20


def test_device_errors_are_raised():
    """Sticky device error flags surface as SpmctsError: node-pool exhaustion, an illegal
    play_action, and an exhausted RNG tape (no silent fallbacks)."""
    from self_play_reinforcement_learning_amd import _lib
    from self_play_reinforcement_learning_amd.arena import Arena, table_net_eval

    def step(arena, count):
        if count:
            p, v = table_net_eval(arena.game, arena.leaves(count), arena.leaf_format, arena.leaf_layout, salt=5)
            arena.expand(p, v)

    # pool: 4 blocks per tree cannot hold a 25-simulation search
    a = Arena("connect4", n_trees=4, iterations=25, blocks_per_tree=4, leaf_format="f32")
    a.tree_reset([0, 1, 2, 3], [1] * 4)
    a.search_begin([0, 1, 2, 3])
    for _ in range(25):
        step(a, a.select())
    with pytest.raises(_lib.SpmctsError, match="node pool"):
        a.check()
    a.close()
    # illegal action: a full column
    a = Arena("connect4", n_trees=1, iterations=4, leaf_format="f32")
    a.tree_reset([0], [1])
    for _ in range(6):
        step(a, a.play_action([0], [3]))
    a.play_action([0], [3])
    with pytest.raises(_lib.SpmctsError, match="illegal action"):
        a.check()
    a.close()
    # tape: too few recorded doubles for a search
    a = Arena("connect4", n_trees=1, iterations=8, rng="tape", leaf_format="f32")
    a.set_tapes([[0.5] * 10])
    a.tree_reset([0], [1])
    a.search_begin([0])
    for _ in range(8):
        step(a, a.select())
    with pytest.raises(_lib.SpmctsError, match="tape"):
        a.check()
    a.close()


@pytest.mark.parametrize("stagger", [False, True])
def test_laned_engine_plays_like_its_lanes(stagger):
    """LanedEngine = independent lane arenas on their own streams: per-lane results equal those of a
    SelfPlayEngine with the same slots, seed and Philox subsequences, counters add up, and exported
    game ids are unique with the swap_sides parity preserved -- with the lanes in lock step and
    staggered (lane 1 half a ply behind lane 0; run() ends with drain())."""
    import numpy as np

    from self_play_reinforcement_learning_amd.engine import LanedEngine, SelfPlayEngine
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    torch.manual_seed(0)
    net = ResidualTower(7, 6, 7, num_blocks=1, filter_factor=32).cuda().eval()
    laned = LanedEngine("connect4", net, n_games=40, lanes=2, iterations=12, seed=3, stagger=stagger)
    got = []
    laned.run(plies=30, on_moves=lambda m: got.append({k: v.cpu().numpy() for k, v in m.items()}))
    laned.check()
    # lane 1 alone: 20 slots, trees 40..79 of the 40-game arena's Philox subsequences
    solo = SelfPlayEngine("connect4", net, n_games=20, iterations=12, seed=3, subsequence0=40)
    ref = []
    solo.run(plies=30, on_moves=lambda m: ref.append({k: v.cpu().numpy() for k, v in m.items()}))
    lane1 = [g for g in got if len(g["game"]) and g["game"][0] >= LanedEngine.GAME_ID_STRIDE]
    a = {k: np.concatenate([g[k] for g in lane1]) for k in lane1[0]}
    b = {k: np.concatenate([g[k] for g in ref]) for k in ref[0]}
    b["game"] = b["game"] + LanedEngine.GAME_ID_STRIDE
    for k in b:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    c = laned.counters()
    c0, c1 = laned.lanes[0].counters(), laned.lanes[1].counters()
    for k in ("sims", "moves", "nn_leaves", "games_finished"):
        assert c[k] == c0[k] + c1[k], k
    assert c["moves"] == 30 * 40
    ids = np.concatenate([g["game"] for g in got])
    firsts = {}
    for g in got:  # each game's records come in one batch: the policy's moves, then the opponent's
        for gid in np.unique(g["game"]):
            assert gid not in firsts
            firsts[gid] = True
    assert len(firsts) == c["games_finished"] and (ids >= 0).all()


def _gravity_ok(board):
    """Connect4 board [W, H] (row 0 = bottom): every column's pieces are contiguous from the bottom."""
    filled = board != 0
    return bool((filled[:, 1:] <= filled[:, :-1]).all())


def _full_size(G, sims, ff, blocks, plies, threads, lanes=2, blocks_per_tree=0, seed=11):
    """Size-independent properties of a full-size self-play run: exact simulation / move / leaf
    accounting, every exported Move a legal gravity-consistent position with a normalised,
    legal-only visit distribution, consistent per-game results, no device error flags."""
    from self_play_reinforcement_learning_amd.engine import LanedEngine
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    torch.manual_seed(0)
    net = ResidualTower(7, 6, 7, num_blocks=blocks, filter_factor=ff).cuda().eval()
    eng = LanedEngine("connect4", net, n_games=G, lanes=lanes, iterations=sims, seed=seed, search_threads=threads,
                      blocks_per_tree=blocks_per_tree)
    got = []
    eng.run(plies=plies, on_moves=lambda m: got.append({k: v.cpu().numpy() for k, v in m.items()}))
    eng.check()
    c = eng.counters()
    assert c["error_flags"] == 0
    # every slot searches every ply (finished slots refill): `sims` search_node calls per search,
    # each completed (network or terminal leaf) or leaked (threaded mode only, mcts.py:349-354)
    assert c["sims"] + c["leaked_sims"] == G * sims * plies
    assert threads > 1 or c["leaked_sims"] == 0
    assert c["moves"] == G * plies
    sim_nn = c["sims"] - c["terminal_leaves"]
    assert sim_nn <= c["nn_leaves"] <= sim_nn + c["set_node_expansions"]
    if got:
        moves = {k: np.concatenate([g[k] for g in got]) for k in got[0]}
        assert len(moves["z"]) == c["positions_exported"] > 0
        assert c["games_finished"] == len(np.unique(moves["game"]))
        assert set(np.unique(moves["z"]).tolist()) <= {-1.0, 0.0, 1.0}
        np.testing.assert_allclose(moves["tree_probs"].sum(1), 1.0, atol=1e-5)
        boards = moves["state"].reshape(-1, 7, 6).astype(int)
        for b, p in zip(boards, moves["tree_probs"]):
            assert _gravity_ok(b)
            assert (p[b[:, 5] != 0] == 0).all()  # full columns get no visits
            assert (b == 1).sum() in ((b == -1).sum(), (b == -1).sum() - 1)
        for gid in np.unique(moves["game"]):
            zs = moves["z"][moves["game"] == gid]
            assert (zs == 0).all() or sorted(np.unique(zs).tolist()) == [-1.0, 1.0]
    return c


def test_full_size_selfplay_properties():
    """BASELINE configs[1] at full size in the sequential search mode (K = 1): Connect4, 200 sims/move,
    4,096 games, ResNet-128x20 on the fused tower, two lanes with packed tiles, 12 plies."""
    _full_size(4096, 200, 32, 20, 12, threads=1)


def test_full_size_headline_bench_config():
    """The exact bench.py default: 4,096 games, 200 sims, ResNet-128x20, two lanes, 4 sims in flight
    per tree (the rolling threaded search), 12 plies."""
    c = _full_size(4096, 200, 32, 20, 12, threads=4)
    assert c["positions_exported"] > 0
    print(f"headline: blocks_in_use_max {c['blocks_in_use_max']} leaked_sims {c['leaked_sims']}")


def test_full_size_config3_recycled_store():
    """BASELINE configs[2] at full size: 16,384 games, 800 sims/move, ResNet-256x20, 4 sims in flight,
    two lanes — with a node store of 1,800 blocks per tree instead of the worst case 16,846
    (11.8 GB instead of 92 GB): subtrees above the active root are recycled (k_compact) and the
    high-water mark stays within the store.  6 plies: every policy tree searches 3 times, the third
    search after a compaction."""
    cap = 1800
    c = _full_size(16384, 800, 64, 20, 6, threads=4, blocks_per_tree=cap, seed=12)
    assert c["compactions"] > 0
    assert c["blocks_in_use_max"] <= cap
    print(f"config3: blocks_in_use_max {c['blocks_in_use_max']} of {cap}, compactions {c['compactions']}, "
          f"leaked_sims {c['leaked_sims']}")


def test_full_size_config5_arena():
    """BASELINE configs[4] at its per-GPU size: arena evaluation (elo.py:73-91 -> compare_models,
    self_play_parallel.py:355-379) of 8,192 games between two frozen ResNet-128x20 nets (seeds 0 and 1)
    on the fp16 fused trunk, 200 sims per move, evaluate mode (temp / 20, root noise on), 4 sims in flight
    per tree, two lanes, every game played to its end (a budget of 8,192 games: no slot refills).
    Size-independent accounting: every game finishes and is counted once in the results, half with the
    policy moving first (swap_sides = game id odd); every move of either side is one full search
    (sims + leaked = 200 x moves); no Move records in evaluate mode; network rows of the two nets never
    merge (rows <= leaves, each net's leaves in its own segment); no device error."""
    from self_play_reinforcement_learning_amd.engine import LanedEngine
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    G, sims = 8192, 200
    torch.manual_seed(0)
    a = ResidualTower(7, 6, 7, num_blocks=20, filter_factor=32).cuda().eval()
    torch.manual_seed(1)
    b = ResidualTower(7, 6, 7, num_blocks=20, filter_factor=32).cuda().eval()
    eng = LanedEngine("connect4", a, n_games=G, lanes=2, iterations=sims, seed=1234, opponent=b, dtype=torch.float16,
                      evaluate=True, record=False, search_threads=4, max_games=G)
    assert all(e.evaluator1 is not None for e in eng.lanes)
    got = []
    info = eng.run(games=G, on_moves=lambda m: got.append(int(m["z"].shape[0])))
    eng.check()
    c = eng.counters()
    assert c["error_flags"] == 0
    assert eng.games_done == c["games_finished"] == G
    r = c["results"]
    assert sum(map(sum, r)) == G
    assert sum(r[0]) == sum(r[1]) == G // 2  # each net moves first in half the games
    assert c["sims"] + c["leaked_sims"] == sims * c["moves"]
    assert 7 * G <= c["moves"] <= 42 * G  # Connect4 games last 7..42 plies
    assert c["positions_exported"] == 0 and sum(got) == 0
    assert 0 < c["nn_rows"] <= c["nn_leaves"]
    print(f"config5: {info['plies']} plies, results {r}, rows/leaf {c['nn_rows'] / c['nn_leaves']:.3f}, "
          f"leaked {c['leaked_sims']}")


def _run_moves(eng, games):
    got = []
    eng.run(games=games, on_moves=lambda m: got.append({k: v.cpu().numpy() for k, v in m.items()}))
    eng.check()
    return {k: np.concatenate([g[k] for g in got]) for k in got[0]}, eng.counters()


@pytest.mark.parametrize("game,n_games,sims,bpt", [("connect4", 512, 16, 0), ("tictactoe", 256, 24, 0),
                                                   ("connect4", 256, 16, 6 * 16 + 64)])
def test_leaf_dedup_is_exact(game, n_games, sims, bpt):
    """Batch leaf dedup (one row per distinct network input of a simulation step) changes nothing
    a search sees: the same Move records bit for bit and the same counters, with fewer network rows
    (games start from the empty board, so early steps are mostly duplicates); also beside subtree
    recycling (bpt > 0: a node store of 6 searches' worth of blocks)."""
    from self_play_reinforcement_learning_amd.engine import SelfPlayEngine
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    torch.manual_seed(0)
    W, H, A = (7, 6, 7) if game == "connect4" else (3, 3, 9)
    net = ResidualTower(W, H, A, num_blocks=2, filter_factor=32)
    out = []
    for dedup in (False, True):
        eng = SelfPlayEngine(game, net, n_games=n_games, iterations=sims, seed=3, max_games=2 * n_games,
                             search_threads=4, leaf_dedup=dedup, blocks_per_tree=bpt, eval_cache=0)
        assert eng.leaf_dedup == dedup and eng.evaluator.pure_planes
        out.append(_run_moves(eng, 2 * n_games))
    (m0, c0), (m1, c1) = out
    for k in m0:
        np.testing.assert_array_equal(m0[k], m1[k], err_msg=k)
    for k in ("sims", "leaked_sims", "moves", "nn_leaves", "terminal_leaves", "depth_sum", "games_finished",
              "positions_exported", "results"):
        assert c0[k] == c1[k], k
    assert c0["nn_rows"] == c0["nn_leaves"]
    assert c1["nn_rows"] < c1["nn_leaves"]
    assert (c1["compactions"] > 0) == (bpt > 0)  # with a small store: dedup beside subtree recycling


@pytest.mark.parametrize("lanes,n_games,sims,game,bpt,sizes", [(2, 512, 16, "connect4", 0, None),
                                                                (3, 384, 24, "connect4", 0, None),
                                                                (2, 256, 24, "tictactoe", 0, None),
                                                                (2, 256, 16, "connect4", 2 * 16 + 64, [118, 138])])
def test_cross_lane_dedup_is_exact(lanes, n_games, sims, game, bpt, sizes):
    """Cross-lane leaf dedup (LanedEngine cross_dedup, include/spmcts.h spmcts_set_leaf_peer): a follower lane's
    leaf whose network input lane 0 evaluates in the same simulation step takes lane 0's row.  Nothing a search
    sees changes: every lane's Move records bit for bit and the counters, with fewer network rows than
    per-lane dedup; leaf dedup switched off mid-run (bench.py's no-dedup twin) falls back to one row per leaf
    with the games still identical."""
    from self_play_reinforcement_learning_amd.engine import LanedEngine
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    torch.manual_seed(0)
    W, H, A = (7, 6, 7) if game == "connect4" else (3, 3, 9)
    net = ResidualTower(W, H, A, num_blocks=2, filter_factor=32).cuda().eval()
    out = []
    for cross in (False, True):
        # (TicTacToe; a recycled node store beside the pairing -- 96 blocks per tree: compacted within the 12
        # plies --; unequal lanes, as bench.py's 0.48 split)
        eng = LanedEngine(game, net, n_games=n_games, lanes=lanes, iterations=sims, seed=7, search_threads=4,
                          max_games=4 * n_games, cross_dedup=cross, blocks_per_tree=bpt, lane_sizes=sizes,
                          eval_cache=0)
        assert eng.cross_dedup == cross and eng.leaf_dedup
        got = []
        eng.run(plies=12, on_moves=lambda m: got.append({k: v.cpu().numpy() for k, v in m.items()}))
        eng.check()
        c_mid = eng.counters()
        for e in eng.lanes:  # the no-dedup twin's switch: every leaf its own row, the pairing idle
            e.arena.set_leaf_dedup(False)
        eng.run(plies=4, on_moves=lambda m: got.append({k: v.cpu().numpy() for k, v in m.items()}))
        eng.check()
        c = eng.counters()
        assert c["nn_rows"] - c_mid["nn_rows"] == c["nn_leaves"] - c_mid["nn_leaves"]
        out.append(({k: np.concatenate([g[k] for g in got]) for k in got[0]}, c_mid, c,
                    [e.counters()["nn_rows"] for e in eng.lanes]))
    (m0, c0, f0, r0), (m1, c1, f1, r1) = out
    for k in m0:
        np.testing.assert_array_equal(m0[k], m1[k], err_msg=k)
    for k in ("sims", "leaked_sims", "moves", "nn_leaves", "terminal_leaves", "depth_sum", "games_finished",
              "positions_exported", "results"):
        assert c0[k] == c1[k] and f0[k] == f1[k], k
    assert c1["nn_rows"] < c0["nn_rows"] < c0["nn_leaves"]
    assert r1[0] == r0[0] and all(b < a for a, b in zip(r0[1:], r1[1:]))  # lane 0's rows unchanged
    assert (c1["compactions"] > 0) == (bpt > 0)
    print(f"cross-lane dedup, {game} {lanes} lanes: rows/leaf {c0['nn_rows'] / c0['nn_leaves']:.4f} -> "
          f"{c1['nn_rows'] / c1['nn_leaves']:.4f}")


def test_cross_lane_dedup_pairing_rules():
    """spmcts_set_leaf_peer refuses pairings it cannot serve exactly (different search_threads, one-level
    lanes only), and a follower's expand after a leader-served step without spmcts_peer_push fails loudly."""
    from self_play_reinforcement_learning_amd import _lib
    from self_play_reinforcement_learning_amd.arena import Arena

    a = Arena("connect4", n_trees=64, iterations=8, search_threads=4, leaf_format="f32")
    b = Arena("connect4", n_trees=64, iterations=8, search_threads=4, leaf_format="f32")
    c = Arena("connect4", n_trees=64, iterations=8, search_threads=2, leaf_format="f32")
    with pytest.raises(_lib.SpmctsError, match="search_threads"):
        c.set_leaf_peer(a)
    b.set_leaf_peer(a)
    with pytest.raises(_lib.SpmctsError, match="leader cannot follow"):
        a.set_leaf_peer(c)
    for x in (a, b):
        x.set_leaf_dedup(True)
        x.tree_reset(list(range(64)), [1] * 64)
        x.search_begin(list(range(64)))
    n0 = a.select()
    p0 = torch.full((64 * 4, 7), 1 / 7, device="cuda")
    v0 = torch.zeros(64 * 4, device="cuda")
    a.expand(p0[:max(n0, 1)].contiguous(), v0[:max(n0, 1)].contiguous())
    b.select()  # every root is the same position: all of b's leaves are lane a's
    with pytest.raises(_lib.SpmctsError, match="peer_push"):
        b.expand(p0, v0)
    b.set_leaf_peer(None)
    for x in (a, b, c):
        x.close()


def test_leaf_dedup_two_networks_exact():
    """Evaluation arena (policy vs a second network, rows in two segments): dedup never merges rows
    of different networks, and the games come out identical."""
    from self_play_reinforcement_learning_amd.engine import SelfPlayEngine
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    torch.manual_seed(0)
    net = ResidualTower(7, 6, 7, num_blocks=2, filter_factor=32)
    torch.manual_seed(1)
    opp = ResidualTower(7, 6, 7, num_blocks=2, filter_factor=32)
    out = []
    for dedup in (False, True):
        eng = SelfPlayEngine("connect4", net, n_games=256, iterations=12, seed=5, max_games=512, opponent=opp,
                             evaluate=True, search_threads=4, leaf_dedup=dedup)
        eng.run(games=512)
        eng.check()
        out.append(eng.counters())
    c0, c1 = out
    for k in ("sims", "moves", "nn_leaves", "terminal_leaves", "depth_sum", "games_finished", "results"):
        assert c0[k] == c1[k], k
    assert c1["nn_rows"] < c1["nn_leaves"]


_SAME = ("sims", "leaked_sims", "moves", "nn_leaves", "terminal_leaves", "depth_sum", "games_finished",
         "positions_exported", "results")


@pytest.mark.parametrize("game,n_games,sims,bpt,window,cap", [("connect4", 512, 16, 0, 1, 0), ("connect4", 512, 16, 0, 3, 0),
                                                              ("tictactoe", 256, 24, 0, 2, 0),
                                                              ("connect4", 256, 16, 6 * 16 + 64, 2, 0),
                                                              ("connect4", 512, 16, 0, 4, 10)])
def test_eval_cache_is_exact(game, n_games, sims, bpt, window, cap):
    """Evaluation cache (include/spmcts.h spmcts_set_eval_cache): a leaf whose network input the arena evaluated
    in the last `window` plies takes those outputs instead of a row.  Nothing a search sees changes: the same
    Move records bit for bit and the same counters as per-step dedup alone, and every owner row of a step is
    either evaluated or cache-served (nn_rows + cache_rows = the dedup run's nn_rows); also beside subtree
    recycling, and with a 1,024-entry table (cap 10) whose inserts collide and run out of free entries."""
    from self_play_reinforcement_learning_amd.engine import SelfPlayEngine
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    torch.manual_seed(0)
    W, H, A = (7, 6, 7) if game == "connect4" else (3, 3, 9)
    net = ResidualTower(W, H, A, num_blocks=2, filter_factor=32)
    out = []
    for w in (0, window):
        eng = SelfPlayEngine(game, net, n_games=n_games, iterations=sims, seed=3, max_games=2 * n_games,
                             search_threads=4, blocks_per_tree=bpt, eval_cache=w)
        assert eng.leaf_dedup and eng.eval_cache == w
        if w and cap:
            eng.arena.set_eval_cache(w, cap)
        out.append(_run_moves(eng, 2 * n_games))
    (m0, c0), (m1, c1) = out
    for k in m0:
        np.testing.assert_array_equal(m0[k], m1[k], err_msg=k)
    for k in _SAME:
        assert c0[k] == c1[k], k
    assert c0["cache_rows"] == 0 and c1["cache_rows"] > 0
    assert c1["nn_rows"] + c1["cache_rows"] == c0["nn_rows"]
    assert (c1["compactions"] > 0) == (bpt > 0)
    print(f"eval cache, {game} window {window} cap {cap}: rows/leaf {c0['nn_rows'] / c0['nn_leaves']:.4f} -> "
          f"{c1['nn_rows'] / c1['nn_leaves']:.4f}")


@pytest.mark.parametrize("lanes,sizes", [(2, None), (3, None), (2, [118, 138])])
def test_eval_cache_with_cross_lane_dedup_is_exact(lanes, sizes):
    """The evaluation cache beside cross-lane dedup: paired lanes share the leader's table (a position either lane
    evaluated serves both; the follower looks there first, then in the leader's batch, taking only rows the
    leader's network evaluates), unpaired lanes keep one table each.  Every lane's Move records and the counters
    equal those of per-step dedup alone; fewer network rows than cross-lane dedup alone."""
    from self_play_reinforcement_learning_amd.engine import LanedEngine
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    torch.manual_seed(0)
    net = ResidualTower(7, 6, 7, num_blocks=2, filter_factor=32).cuda().eval()
    n_games = 256 if sizes else 128 * lanes
    out = []
    for cross, w in ((False, 0), (True, 0), (True, 2), (False, 2)):
        eng = LanedEngine("connect4", net, n_games=n_games, lanes=lanes, iterations=16, seed=7, search_threads=4,
                          max_games=4 * n_games, cross_dedup=cross, lane_sizes=sizes, eval_cache=w)
        assert eng.cross_dedup == cross and eng.eval_cache == w
        got = []
        eng.run(plies=12, on_moves=lambda m: got.append({k: v.cpu().numpy() for k, v in m.items()}))
        eng.check()
        out.append(({k: np.concatenate([g[k] for g in got]) for k in got[0]}, eng.counters()))
    (m0, c0), (m1, c1), (m2, c2), (m3, c3) = out
    for k in m0:
        for m in (m1, m2, m3):
            np.testing.assert_array_equal(m0[k], m[k], err_msg=k)
    for k in _SAME:
        assert c0[k] == c1[k] == c2[k] == c3[k], k
    assert c2["cache_rows"] > 0 and c2["nn_rows"] < c1["nn_rows"] < c0["nn_rows"]
    assert c3["cache_rows"] > 0 and c3["nn_rows"] < c0["nn_rows"]
    print(f"eval cache + cross-lane dedup, {lanes} lanes: rows/leaf {c1['nn_rows'] / c1['nn_leaves']:.4f} -> "
          f"{c2['nn_rows'] / c2['nn_leaves']:.4f}")


def test_eval_cache_two_networks_exact():
    """Evaluation arena (policy vs a second network, evaluate mode, rows in two segments): the cache keeps the two
    networks' keys apart and serves each segment's rows after its network rows; results and counters equal those of
    per-step dedup alone, with fewer network rows."""
    from self_play_reinforcement_learning_amd.engine import SelfPlayEngine
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    torch.manual_seed(0)
    net = ResidualTower(7, 6, 7, num_blocks=2, filter_factor=32)
    torch.manual_seed(1)
    opp = ResidualTower(7, 6, 7, num_blocks=2, filter_factor=32)
    out = []
    for w in (0, 2):
        eng = SelfPlayEngine("connect4", net, n_games=256, iterations=12, seed=5, max_games=512, opponent=opp,
                             evaluate=True, search_threads=4, eval_cache=w, record=False)
        assert eng.eval_cache == w and eng.evaluator1 is not None
        eng.run(games=512)
        eng.check()
        out.append(eng.counters())
    c0, c1 = out
    for k in ("sims", "leaked_sims", "moves", "nn_leaves", "terminal_leaves", "depth_sum", "games_finished", "results"):
        assert c0[k] == c1[k], k
    assert c1["cache_rows"] > 0 and c1["nn_rows"] + c1["cache_rows"] == c0["nn_rows"]
    print(f"eval cache, two networks: rows/leaf {c0['nn_rows'] / c0['nn_leaves']:.4f} -> {c1['nn_rows'] / c1['nn_leaves']:.4f}")


def test_eval_cache_cleared_on_new_weights():
    """refresh_network after the weights change clears the cache (spmcts_eval_cache_clear): the plies after the
    change see the new network's outputs only, exactly as the run without a cache does."""
    from self_play_reinforcement_learning_amd.engine import SelfPlayEngine
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    out = []
    for w in (0, 8):
        torch.manual_seed(0)
        net = ResidualTower(7, 6, 7, num_blocks=2, filter_factor=32).cuda().eval()
        torch.manual_seed(1)
        new = ResidualTower(7, 6, 7, num_blocks=2, filter_factor=32).cuda().eval()
        eng = SelfPlayEngine("connect4", net, n_games=256, iterations=16, seed=11, search_threads=4, eval_cache=w)
        got = []
        sink = lambda m: got.append({k: v.cpu().numpy() for k, v in m.items()})  # noqa: E731
        eng.run(plies=10, on_moves=sink)
        net.load_state_dict(new.state_dict())
        eng.refresh_network()
        eng.run(plies=10, on_moves=sink)
        eng.check()
        out.append(({k: np.concatenate([g[k] for g in got]) for k in got[0]}, eng.counters()))
    (m0, c0), (m1, c1) = out
    for k in m0:
        np.testing.assert_array_equal(m0[k], m1[k], err_msg=k)
    for k in _SAME:
        assert c0[k] == c1[k], k
    assert c1["cache_rows"] > 0


def test_eval_cache_rules():
    """spmcts_set_eval_cache refuses what it cannot serve exactly: search_threads 1 (no dedup rows) and a bad
    capacity; SelfPlayEngine refuses it without leaf dedup."""
    from self_play_reinforcement_learning_amd import _lib
    from self_play_reinforcement_learning_amd.arena import Arena
    from self_play_reinforcement_learning_amd.engine import SelfPlayEngine
    from self_play_reinforcement_learning_amd.modules import ResidualTower

    a = Arena("connect4", n_trees=64, iterations=8, search_threads=1, leaf_format="f32")
    with pytest.raises(_lib.SpmctsError, match="search_threads"):
        a.set_eval_cache(1)
    a.set_eval_cache(0)
    a.close()
    b = Arena("connect4", n_trees=64, iterations=8, search_threads=4, leaf_format="f32")
    with pytest.raises(_lib.SpmctsError, match="capacity"):
        b.set_eval_cache(1, 40)
    b.set_eval_cache(2, 12)
    b.eval_cache_clear()
    b.close()
    torch.manual_seed(0)
    net = ResidualTower(7, 6, 7, num_blocks=2, filter_factor=32)
    with pytest.raises(ValueError, match="eval_cache"):
        SelfPlayEngine("connect4", net, n_games=64, iterations=8, search_threads=4, leaf_dedup=False, eval_cache=1)


def test_bench_line_small_with_no_dedup_twin():
    """bench.py end to end on a small workload (subprocess, as the driver runs it): one JSON line with
    the contract keys, roofline and tree roofline, and the --twin-no-dedup plies (leaf dedup off on
    the same arenas: one network row per leaf), and with --secondary the bf16 trunk's line on a fresh
    engine."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--games", "512", "--sims", "16", "--blocks", "2",
           "--steps", "3", "--warmup", "2", "--full", "--no-cpu-baseline", "--twin-no-dedup", "2", "--secondary"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=root, check=True).stdout
    line = [l for l in out.splitlines() if l.startswith("{")]
    assert len(line) == 1
    d = json.loads(line[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "dtype", "data", "config", "roofline", "tree_roofline", "exchange"):
        assert k in d, k
    assert d["value"] > 0 and d["n_gpus"] == 1 and d["steps"] == 3 and d["exchange"]["backend"] is None
    assert 0 < d["roofline"]["frac"] < 1 and d["config"]["leaf_dedup"] is True and d["nn"]["rows_per_leaf"] <= 1.0
    tw = d["no_dedup_twin"]
    assert tw["plies"] == 2 and tw["value"] > 0 and tw["rows_per_leaf"] == 1.0
    # the default dtype is the reference's fp16; --secondary times the bf16 trunk on a fresh engine afterwards
    assert d["dtype"] == "fp16" and d["secondary_dtype"]["dtype"] == "bf16" and d["secondary_dtype"]["value"] > 0
    r = d["ranks"]
    assert r["world_size"] == 1 and len(r["per_rank"]) == 1
    assert r["positions_per_s_min"] == r["positions_per_s_max"] == r["per_rank"][0]["positions_per_s"]


def test_bench_line_small_with_eval_cache():
    """bench.py --eval-cache: the line names the window, counts the cache-served rows, and carries the
    no_cache_twin (the plies after the timed region with the cache off: per-step dedup alone, more rows)."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--games", "512", "--sims", "16", "--blocks", "2",
           "--steps", "3", "--warmup", "2", "--full", "--no-cpu-baseline", "--eval-cache", "2", "--twin-no-cache", "2",
           "--twin-no-dedup", "2"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=root, check=True).stdout
    d = json.loads([l for l in out.splitlines() if l.startswith("{")][0])
    assert d["config"]["eval_cache_plies"] == 2 and d["nn"]["cache_rows"] > 0
    tw, td = d["no_cache_twin"], d["no_dedup_twin"]
    assert tw["plies"] == 2 and tw["value"] > 0 and d["nn"]["rows_per_leaf"] < tw["rows_per_leaf"] < 1.0
    assert td["rows_per_leaf"] == 1.0


def test_bench_arena_line_with_eval_cache():
    """bench.py --mode arena (two networks, evaluate mode) runs the evaluation cache by default; its twins report
    the headline's unit (games/s)."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--mode", "arena", "--games", "256", "--sims", "16",
           "--blocks", "2", "--steps", "6", "--warmup", "6", "--full", "--no-cpu-baseline", "--twin-no-cache", "4",
           "--twin-no-dedup", "0"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=root, check=True).stdout
    d = json.loads([l for l in out.splitlines() if l.startswith("{")][0])
    assert d["unit"] == "games/s" and d["config"]["eval_cache_plies"] == 1 and d["nn"]["cache_rows"] > 0
    tw = d["no_cache_twin"]
    assert tw["unit"] == "games/s" and tw["value"] >= 0 and d["nn"]["rows_per_leaf"] < tw["rows_per_leaf"] <= 1.0


def test_bench_plain_line_and_dump_outputs(tmp_path):
    """A plain bench.py run (no --full) prints the headline line alone -- no CPU baseline, twins or secondary
    dtype -- with --steps timed plies and their ms_per_step, and --dump-outputs writes the last timed ply's
    outputs as float32 / float64 .npy files under 64 MB that a second run with the same arguments repeats
    value for value."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dumps = []
    for name in ("a", "b"):
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--games", "256", "--sims", "16",
               "--blocks", "2", "--steps", "3", "--warmup", "20", "--dump-outputs", str(tmp_path / name)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=root, check=True).stdout
        line = [l for l in out.splitlines() if l.startswith("{")]
        assert len(line) == 1
        d = json.loads(line[0])
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and d["dtype"] == "fp16"
        assert d["unit"] == "positions/s" and d["higher_is_better"] is True
        # --steps plies were timed: every game slot moves once per ply
        assert round(d["value"] * d["ms_per_step"] * 3 / 1e3) == 3 * 256
        assert d["cpu_baseline"] is None
        assert not {"no_cache_twin", "no_dedup_twin", "secondary_dtype"} & set(d)
        files = sorted(os.listdir(tmp_path / name))
        assert files == sorted(k + ".npy" for k in d["dumped_outputs"])
        dumps.append({f: np.load(tmp_path / name / f) for f in files})
    a, b = dumps
    assert {"ply_finished_exported.npy", "moves_state.npy", "moves_tree_probs.npy", "moves_z.npy", "slots_ply.npy",
            "slots_game_id.npy"} <= set(a)
    assert sum(v.nbytes for v in a.values()) <= 64 * 2 ** 20
    for f in a:
        assert a[f].dtype in (np.float32, np.float64), f
        assert a[f].shape == b[f].shape and np.array_equal(a[f], b[f]), f
    # after 20 + 3 plies some of the 256 games have ended: the last ply exported their Move records
    n = a["moves_z.npy"].shape[0]
    assert n > 0 and a["ply_finished_exported.npy"][1] == n and a["moves_state.npy"].shape == (n, 42)
    assert np.allclose(a["moves_tree_probs.npy"].sum(1), 1.0, atol=1e-5)
    assert a["slots_ply.npy"].shape == (256,) and a["slots_game_id.npy"].shape == (256,)
