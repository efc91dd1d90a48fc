"""`MCTreeSearch` with the reference policy protocol, backed by the HIP arena.

Drop-in for games/algos/mcts.py:116-394.  Same constructor (plus the stale
`env_gen=` / `evaluator=` aliases its own callers still pass,
run_self_play_connect4.py:29, c4_manual.py:24-31), same methods:
`__call__`, `reset`, `play_action`, `push_to_queue`, `pull_from_queue`,
`update_from_memory`, `loss`, `state_dict`, `load_state_dict`, `train`,
`evaluate`, `deduplicate`, attributes `memory`, `memory_queue`, `root_node`,
`env`, `network`, `strong_play`, `temp_memory`.

A single MCTreeSearch drives a one-tree arena (the object tree of mcts.py
becomes the device node store; `root_node` is a read-only view of it).  The
batched self-play path does not go through this class: SelfPlayScheduler
runs thousands of trees per arena (engine.py).
"""
import logging
import time
from collections import namedtuple

import numpy as np
import torch

from .arena import GAMES, Arena, game_of_env, solver_search_rules
from .base_model import Policy
from .evaluator import make_evaluator

Move = namedtuple("Move", ("state", "actual_val", "tree_probs", "q"))


class _ChildView:
    def __init__(self, n, w, p, player):
        self.n, self.w, self.p, self.player = n, w, p, player

    @property
    def q(self):
        return self.w / self.n if self.n else 0


class RootView:
    """Read-only snapshot of the active root (MCNode fields n, w, q, player, state, children)."""

    def __init__(self, stats):
        self.n = stats["root_n"]
        self.w = stats["root_w"]
        self.player = stats["root_player"]
        self.state = stats["board"].astype(np.int64)
        self.children = tuple(_ChildView(n, w, p, -self.player)
                              for n, w, p in zip(stats["child_n"], stats["child_w"], stats["child_p"]))

    @property
    def q(self):
        return self.w / self.n if self.n else 0


def az_loss(network, states, actual_val, tree_probs, q, q_average=True):
    """The AlphaZero loss of MCTreeSearch.loss (mcts.py:234-252) on stacked tensors:
    MSELossFlat(v, z [+ q]) (rl_utils/flat.py: float targets, mean over the batch) plus
    -sum(pi * log p) / B.  `states` int64 [B, W, H] in the Move frame (+1 = player to move).
    Shared by MCTreeSearch.loss and the scheduler's trainer (self_play_parallel._Trainer);
    pinned by tests/golden/trainer_step.npz (G8)."""
    dev = next(network.parameters()).device
    probs, value = network.forward(states.to(dev))
    z = actual_val.to(dev).float()
    if q_average:
        z = z + q.to(dev)
    value_loss = torch.mean((value.reshape(-1) - z.float().reshape(-1)) ** 2)
    prob_loss = -(probs.log() * tree_probs.to(dev)).sum() / probs.size()[0]
    return value_loss + prob_loss


class MCTreeSearch(Policy):
    def __init__(self, network=None, env=None, optim=None, memory_queue=None, iterations=100, temperature_cutoff=5,
                 batch_size=64, memory_size=200000, min_memory=20000, update_nn=True, starting_state_dict=None,
                 thread_count=4, strong_play=False, q_average=True, alpha=1, env_gen=None, evaluator=None,
                 seed=None, device=None, rng="philox", cpuct=4, x_noise=0.25, threading=False, proof_play=False,
                 stored_bounds=False, solver_search=False, symmetry=None):
        network = network if network is not None else evaluator
        env = env if env is not None else env_gen
        rules = solver_search_rules(solver_search)  # (a bad option raises before anything is built)
        if network is None or env is None:
            raise TypeError("MCTreeSearch needs `network` and `env` (or the legacy `evaluator` / `env_gen`)")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if isinstance(network, torch.nn.Module):
            network = network.to(self.device)
        self.network = network
        self.env_gen = env
        self.env = env() if callable(env) else env
        self.game = game_of_env(self.env)
        _, self.W, self.H, self.actions = GAMES[self.game]
        self.optim = optim
        self.iterations = iterations
        self.alpha = alpha
        self.cpuct, self.x_noise = cpuct, x_noise  # (read back by PerfectEvaluator's batch search)
        self.strong_play = strong_play
        self.q_average = q_average
        self.batch_size = batch_size
        self.min_memory = min_memory
        self.temperature_cutoff = temperature_cutoff
        self.update_nn = update_nn
        self.starting_state_dict = starting_state_dict
        self.thread_count = thread_count
        self.evaluating = False
        # threading=True: thread_count sims in flight with virtual loss, the reference's mode when its
        # network is an InferenceProxy (mcts.py:154, :328-331); False: its sequential mode
        self.threading = bool(threading)
        k = int(thread_count) if self.threading and thread_count and thread_count > 1 else 1
        # fp16 trunk: the reference's inference autocast dtype (inference_worker.py:114-119)
        self._evaluator = make_evaluator(network, self.game, device=self.device, dtype=torch.float16)
        if seed is None:
            seed = int(np.random.randint(0, 2**31 - 1))
        self._arena = Arena(self.game, n_trees=1, n_games=0, iterations=iterations, rng=rng, seed=seed,
                            strong_play=strong_play, leaf_format=self._evaluator.leaf_format,
                            leaf_layout=self._evaluator.leaf_layout, cpuct=cpuct, x_noise=x_noise, alpha=alpha,
                            device=self.device, search_threads=k)
        # symmetry="mirror": leaves are evaluated in canonical orientation (Arena.set_symmetry): the search runs
        # symmetry.SymmetricNet of the network, the same function on a position and on its mirror image
        self.symmetry = symmetry
        if symmetry is not None:
            self._arena.set_symmetry(symmetry)
        # proof_play=True: the move choice drops the moves the tree's own proof rules out (Arena.set_proof_play)
        self.proof_play = bool(proof_play)
        if self.proof_play:
            self._arena.set_proof_play(True)
        # stored_bounds=True: the tree keeps its score bounds in the nodes (Arena.set_stored_bounds); searches are
        # bit-identical, proof_moves() and the proof_play verdict read the root's block instead of walking the tree
        self.stored_bounds = bool(stored_bounds)
        if self.stored_bounds:
            self._arena.set_stored_bounds()
        # solver_search=True | "refute" | "proved": the selects read the stored bounds (Arena.set_solver_rules; it
        # switches stored bounds on): a refuted child draws no sims, a sim that reaches a solved child ends there
        self.solver_search = solver_search
        if any(rules):
            self._arena.set_solver_rules(*rules)
            self.stored_bounds = True
        self.temp_memory = []
        self.moves_played = 0
        # weights changed (update_from_memory / load_state_dict): the evaluator's folded / packed copy is
        # refreshed before the next leaf evaluation, the empty-board root prior at the next reset
        self._weights_stale = False
        self._root_prior_stale = True
        if starting_state_dict:
            self.load_state_dict(starting_state_dict)
        super().__init__(memory_queue=memory_queue, memory_size=memory_size)
        self.reset()

    # ------------------------------------------------------------------ search
    def _sync_weights(self):
        """The reference evaluates every leaf with the network as it is now (mcts.py:316): after an
        update the evaluator's packed weights are re-derived before the next evaluation."""
        if self._weights_stale:
            if hasattr(self._evaluator, "refresh"):
                self._evaluator.refresh()
            self._weights_stale = False

    def _refresh_root_prior(self):
        self._sync_weights()
        x = self._evaluator.empty_root_input(self.W, self.H, self.device)
        probs, _ = self._evaluator(x)
        self._arena.set_root_prior(probs[0])
        self._root_prior_stale = False

    def _eval_expand(self, n):
        if n:
            self._sync_weights()
            probs, values = self._evaluator(self._arena.leaves(n))
            self._arena.expand(probs, values)

    def reset(self, player=1):
        """mcts.py:166-174"""
        if self._root_prior_stale:
            self._refresh_root_prior()
        self._arena.tree_reset([0], [player])
        self.moves_played = 0
        self.temp_memory = []
        self._arena.check()
        return np.zeros([self.W, self.H], dtype=np.int64)

    def __call__(self, s=None):
        """Search `iterations` simulations from the root and pick a move (mcts.py:177-186)."""
        self.search()
        return self._play(1)

    def search(self):
        a = self._arena
        a.search_begin([0])
        for _ in range(-(-self.iterations // a.search_threads)):
            self._eval_expand(a.select())

    def _play(self, temp=1):
        if self.evaluating:
            temp = temp / 20  # mcts.py:273-274
        out = self._arena.search_end(temp)
        action = int(out["action"][0])
        if int(out["recorded"][0]):
            q = float(out["q"][0])
            qt = torch.tensor(q, dtype=torch.float64) if int(out["q_f64"][0]) else torch.tensor(q, dtype=torch.float32)
            self.temp_memory.append(Move(
                torch.as_tensor(out["state"][0].cpu().numpy().astype(np.int64).reshape(self.W, self.H)),
                None, out["tree_probs"][0].cpu().clone(), qt))
        else:
            logging.info("action exception: falling back to the most visited child")
        self.moves_played += 1
        self._arena.check()
        return action

    def play_action(self, action, player=None):
        """Advance the root; an unvisited child is expanded and backed up (mcts.py:188-209)."""
        self._eval_expand(self._arena.play_action([0], [int(action)]))

    def set_position(self, moves, player=1):
        """The tree of a position given as a move sequence from the empty board: reset(player), then
        play_action(m) for each move (the state the reference's MCTreeSearch is in after the same calls).  The
        single-tree form of analyse_positions' chain; the moves are validated first (openings.py)."""
        from .openings import validate_openings

        seq = validate_openings(self.game, [moves])[0]
        self.reset(player)
        for a in seq:
            self.play_action(a)
        return self.root_node.state

    @property
    def root_node(self):
        return RootView(self._arena.root_stats(0))

    def principal_variation(self, max_len=None, min_visits=1):
        """The line the search expects from the active root, [(action, n, q), ...]: at each node the most visited
        child, the lowest action on ties (the rule of _play's fallback, mcts.py:290-295), while it has at least
        max(min_visits, 1) visits, for at most max_len moves (Arena.pv_batch).  q is MCNode.q of the child."""
        out = {k: v[0].cpu().numpy() for k, v in self._arena.pv_batch([0], max_len, min_visits).items()}
        self._arena.check()
        pv = []
        for k in range(int(out["pv_len"])):
            n, vl, w = int(out["pv_n"][k]), int(out["pv_vl"][k]), float(out["pv_w"][k])
            pv.append((int(out["pv"][k]), n, (w - vl) / (n + vl) if n + vl else 0))
        return pv

    def tree(self, min_visits=1, max_depth=None):
        """The subtree under the active root as a tree.TreeView (the reference's root_node.children[a].children[b]
        walk and RenderTree, on a host copy): the nodes with at least min_visits visits, to max_depth.  Sized for
        one search's expansions first; a tree that does not fit is exported once more at its reported count."""
        from .tree import TreeView

        room = 2 + self.iterations * (self.actions if min_visits <= 0 else 1)
        sb = self.stored_bounds  # the nodes then carry their stored bounds (TreeNode.move_lo / .move_hi)
        view = TreeView.from_export(self._arena.export_subtrees([0], room, min_visits, max_depth, bounds=sb))
        if view.truncated:
            view = TreeView.from_export(self._arena.export_subtrees([0], view.count, min_visits, max_depth, bounds=sb))
        self._arena.check()
        return view

    def score_bounds(self):
        """What the tree under the active root has proved about its position (Arena.bounds_batch): lo <= s <= hi
        for the exact solver's score s (solve.py), per root move move_lo / move_hi (-128: illegal), best (the
        lowest action that secures lo), empty, nodes; status, tree.classify_bounds(lo, hi): "win", "loss", "draw",
        "not_lost", "not_won" or "open"; and the bounds as the solvers' move codes (tree.bounds_to_codes: +k a
        win in k plies, -k a loss at ply k): lo_code, hi_code, move_lo_code, move_hi_code.  Plain ints and lists."""
        from .tree import bounds_to_codes, classify_bounds

        raw = {k: v[0].cpu().numpy() for k, v in self._arena.bounds_batch([0]).items()}
        self._arena.check()
        out = {k: (v.tolist() if v.ndim else int(v)) for k, v in raw.items()}
        e = out["empty"]
        out["status"] = classify_bounds(out["lo"], out["hi"])
        out.update(lo_code=bounds_to_codes(out["lo"], e), hi_code=bounds_to_codes(out["hi"], e),
                   move_lo_code=bounds_to_codes(raw["move_lo"], e).tolist(),
                   move_hi_code=bounds_to_codes(raw["move_hi"], e).tolist())
        return out

    def proof_moves(self):
        """What proof-guided play would keep at the active root as the tree stands (Arena.proof_moves_batch; the
        tree is only read, proof_play on or off): dict(keep: the kept actions, a list; mask: the same as bits; lo,
        hi: the root's score bounds)."""
        out = {k: int(v[0]) for k, v in self._arena.proof_moves_batch([0]).items()}
        self._arena.check()
        mask = out["keep"] & 0xffffffff
        return dict(keep=[a for a in range(self.actions) if (mask >> a) & 1], mask=mask, lo=out["lo"], hi=out["hi"])

    # ------------------------------------------------------------------ memory / training
    def update(self, s, a, r, done, next_s):
        self.push_to_queue(s, a, r, done, next_s)
        self.pull_from_queue()
        if self.ready:
            self.update_from_memory()

    def pull_from_queue(self):
        while not self.memory_queue.empty():
            e = self.memory_queue.get()
            self.memory.add(Move(*[e[i].to(self.device) for i in range(4)]))

    def push_to_queue(self, s=None, a=None, r=None, done=None, next_s=None):
        """mcts.py:225-232: on `done`, stamp the owner's result on every buffered Move."""
        if done:
            for e in self.temp_memory:
                self.memory_queue.put(e._replace(actual_val=torch.tensor(r).float()))
            self.temp_memory = []

    def loss(self, batch):
        """AlphaZero loss (mcts.py:234-252): MSE(v, z [+ q]) - sum(pi * log p) / B."""
        s, actual_val, tree_probs, q = Move(*zip(*batch))
        return az_loss(self.network, torch.stack(s), torch.stack(actual_val), torch.stack(tree_probs),
                       torch.stack(q), self.q_average)

    def update_from_memory(self):
        if len(self.memory) < self.batch_size:
            time.sleep(1)
            return
        loss = self.loss(self.memory.sample(self.batch_size))
        self.optim.zero_grad()
        loss.backward()
        self.optim.step()
        self._weights_stale = True
        self._root_prior_stale = True

    @property
    def ready(self):
        return len(self.memory) >= self.min_memory and self.update_nn

    def load_state_dict(self, state_dict, target=False):
        self.network.load_state_dict(state_dict)
        self._weights_stale = True
        self._root_prior_stale = True

    def state_dict(self):
        return self.network.state_dict()

    def update_target_net(self):
        pass

    def deduplicate(self):
        self.memory.deduplicate("state", ["actual_val", "tree_probs"], Move)

    def train(self, train_state=True):
        if hasattr(self.network, "train"):
            return self.network.train(train_state)
        return self.network

    def evaluate(self, evaluate_state=False):
        """Evaluate mode plays with temp / 20 (mcts.py:273-274, :392-394)."""
        self.evaluating = evaluate_state


@torch.no_grad()
def analyse_positions(game, network, positions, iterations, search_threads=1, x_noise=0.25, seed=0, alpha=1.0,
                      strong_play=False, cpuct=4.0, player=1, device=None, dtype=torch.float16, rng="philox",
                      pv_len=0, tree=None, bounds=False, stored_bounds=False, solver_search=False, symmetry=None):
    """The search's answer for a batch of positions, each a move sequence from the empty board.

    One tree-mode arena of one tree per position: reset(player), one play_action step per ply (a tree whose
    sequence is shorter sits out), one search of `iterations` simulations (search_threads in flight per tree),
    then one Arena.root_stats_batch call.  Each tree is in the state MCTreeSearch.set_position(moves) followed by
    search() leaves it in; tree t draws from Philox subsequence t of `seed`.  Returns device tensors: child_n int32
    [n, A] (visit counts), child_w float64 [n, A], child_p float32 [n, A] (priors), root_n, root_w, root_q float64
    [n] (w / n of the root, 0 where n is 0), root_player int8 [n], action int64 [n] (the most visited child, the
    lowest index on ties), board int8 [n, W, H] (tree frame).

    pv_len > 0 adds each position's principal variation of at most pv_len moves (Arena.pv_batch): pv int8 [n,
    pv_len] (-1 past the end; pv[:, 0] is `action` wherever the root was searched), pv_len int32 [n], pv_n int32 and
    pv_w float64 [n, pv_len], pv_end uint8 [n].  A position's moves followed by its pv is a move list again.
    tree=dict(max_nodes=, min_visits=, max_depth=) adds Arena.export_subtrees' arrays of every position under
    "tree" (tree.TreeView.from_export(out["tree"], i) for position i).  bounds=True adds what each position's tree
    has proved (Arena.bounds_batch): bound_lo, bound_hi int8 [n] (lo <= s <= hi for the exact solver's score s),
    move_lo, move_hi int8 [n, A], bound_best int8 [n], bound_nodes int32 [n], and keep int32 [n], the moves
    proof-guided play would choose among (Arena.proof_moves_batch; bit a: move a).  None of them changes the other
    keys.  stored_bounds=True keeps the score bounds in the nodes (Arena.set_stored_bounds): the same outputs, `keep`
    read from the root's stored block, and tree=dict(..., bounds=True) lists the stored entries.
    solver_search=True | "refute" | "proved" searches with the stored bounds (Arena.set_solver_rules; stored bounds
    come with it): other visit counts, still sound bounds; out["solver_stats"] then holds Arena.solver_stats().
    symmetry="mirror" searches symmetry.SymmetricNet of the network (Arena.set_symmetry): a position and its mirror
    image then get mirrored answers, priors bit for bit."""
    from .openings import validate_openings

    game = game if isinstance(game, str) else game_of_env(game)
    seqs = validate_openings(game, positions)
    rules = solver_search_rules(solver_search)  # (a bad option raises before anything is built)
    n = len(seqs)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if isinstance(network, torch.nn.Module):
        network = network.to(dev)
    ev = make_evaluator(network, game, device=dev, dtype=dtype)
    arena = Arena(game, n_trees=max(n, 1), n_games=0, iterations=iterations, rng=rng, seed=seed,
                  strong_play=strong_play, leaf_format=ev.leaf_format, leaf_layout=ev.leaf_layout, cpuct=cpuct,
                  x_noise=x_noise, alpha=alpha, device=dev, search_threads=search_threads)
    try:
        if symmetry is not None:
            arena.set_symmetry(symmetry)
        if stored_bounds:
            arena.set_stored_bounds()
        if any(rules):
            arena.set_solver_rules(*rules)

        def eval_expand(count):
            if count:
                probs, values = ev(arena.leaves(count))
                arena.expand(probs, values)

        probs, _ = ev(ev.empty_root_input(arena.W, arena.H, dev))
        arena.set_root_prior(probs[0])
        trees = list(range(n))
        if n:
            arena.tree_reset(trees, [player] * n)
            for i in range(max(len(s) for s in seqs)):
                on = [t for t in trees if i < len(seqs[t])]
                eval_expand(arena.play_action(on, [seqs[t][i] for t in on]))
            arena.search_begin(trees)
            for _ in range(-(-iterations // arena.search_threads)):
                eval_expand(arena.select())
        out = arena.root_stats_batch(trees)
        rn = out["root_n"].to(torch.float64)
        out["root_q"] = torch.where(rn > 0, out["root_w"] / rn.clamp(min=1), torch.zeros_like(rn))
        out["action"] = out["child_n"].argmax(dim=1) if n else torch.zeros(0, dtype=torch.int64, device=dev)
        if pv_len > 0:
            pv = arena.pv_batch(trees, pv_len)
            out.update(pv=pv["pv"], pv_len=pv["pv_len"], pv_n=pv["pv_n"], pv_w=pv["pv_w"], pv_end=pv["pv_end"])
        if tree is not None:
            out["tree"] = arena.export_subtrees(trees, **tree)
        if bounds:
            b = arena.bounds_batch(trees)
            out.update(bound_lo=b["lo"], bound_hi=b["hi"], move_lo=b["move_lo"], move_hi=b["move_hi"],
                       bound_best=b["best"], bound_nodes=b["nodes"], keep=arena.proof_moves_batch(trees)["keep"])
        if any(rules):
            out["solver_stats"] = arena.solver_stats()
        arena.check()
    finally:
        arena.close()
    return out


SOLVE_ILLEGAL = -128  # the code of an illegal move (include/spmcts.h "exact depth-limited negamax")


def solve_positions(game, positions=None, boards=None, players=None, depth=6, device=None):
    """The truth about a batch of positions, to a horizon: the exact depth-limited negamax on the device
    (include/spmcts.h spmcts_negamax_batch; no network, no arena).

    positions: move lists from the empty board (validated like an opening book: legal, not ending the game),
    player 1 first, so the mover is 1 after an even number of moves and -1 after an odd one.  Or boards int8
    [n, W, H] of +-1 stones with players [n], the side to move of each; a board is assumed not to be finished
    (one that already holds a line is searched as if play went on).  depth: 1 .. 8 on the Connect4 boards, 1 .. 9
    on TicTacToe (a full solve).

    Returns device tensors: score int8 [n, A], one code per action -- +k (k odd): playing it forces a win within
    k plies and not sooner (the move itself is ply 1); -k (k even): every line loses, k the latest ply the loss can
    be delayed to; 0: not decided within `depth` plies (a full-board draw too); -128: illegal.  The better move has
    the higher place in +1 > +3 > ... > 0 > ... > -4 > -2.  value int8 [n]: the best code over the legal moves (0
    where there is none); best bool [n, A]: the legal moves that carry it; nodes int64 [n]: moves the search made.

    The search's own answer held against it (tactical_report below):
        tactical_report(solve_positions(game, seqs)["score"], analyse_positions(game, net, seqs, 200)["action"])"""
    from . import _lib
    from .arena import GAMES, _stream
    from .hardcoded_players import negamax_max_depth, negamax_rank
    from .openings import validate_openings

    game = game if isinstance(game, str) else game_of_env(game)
    gid, W, H, A = GAMES[game]
    cap = negamax_max_depth(game)
    if isinstance(depth, bool) or not isinstance(depth, int) or not 1 <= depth <= cap:
        raise ValueError(f"depth must be an integer in [1, {cap}] on {game}, got {depth!r}")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if (positions is None) == (boards is None):
        raise ValueError("solve_positions takes either positions= (move lists) or boards= with players=")
    if positions is not None:
        from .envs import Connect4Env, TicTacToeEnv

        seqs = validate_openings(game, positions)
        env = TicTacToeEnv() if game == "tictactoe" else Connect4Env(W, H)
        bs = np.zeros((len(seqs), W, H), dtype=np.int8)
        for i, seq in enumerate(seqs):
            env.reset()
            for p, a in enumerate(seq):
                env.step(a, 1 if p % 2 == 0 else -1)
            bs[i] = env.board
        boards = torch.as_tensor(bs)
        players = torch.as_tensor(np.array([1 if len(s) % 2 == 0 else -1 for s in seqs], dtype=np.int8))
    elif players is None:
        raise ValueError("boards= needs players= (the side to move of each board)")
    b = torch.as_tensor(boards).to(dev, torch.int8).reshape(-1, W, H).contiguous()
    pl = torch.as_tensor(players).to(dev, torch.int8).reshape(-1).contiguous()
    n = b.shape[0]
    if pl.shape[0] != n:
        raise ValueError(f"{n} boards but {pl.shape[0]} players")
    score = torch.full((n, A), SOLVE_ILLEGAL, dtype=torch.int8, device=dev)
    nodes = torch.zeros(n, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.call("spmcts_negamax_batch", gid, W, H, _lib.ptr(b), _lib.ptr(pl), n, depth, _lib.ptr(score),
                  _lib.ptr(nodes), _stream())
    rank = negamax_rank(score)
    top = rank.max(dim=1, keepdim=True).values if n else rank[:, :1]
    legal = score != SOLVE_ILLEGAL
    best = (rank == top) & legal
    value = torch.where(legal.any(dim=1), (score.long() * best).sum(dim=1) // best.sum(dim=1).clamp(min=1),
                        torch.zeros(n, dtype=torch.int64, device=dev)).to(torch.int8)
    return dict(score=score, value=value, best=best, nodes=nodes)


TACTICAL_CLASSES = ("missed_win", "slower_win", "blunder", "forced_loss", "ok")


def tactical_report(score, action):
    """Each position's chosen move held against its exact codes (solve_positions(...)["score"], int8 [n, A];
    action [n]).  Pure torch.  One class per position, the first that applies:
        missed_win   a +k existed and the chosen code is <= 0
        slower_win   the chosen move wins, but a faster win existed
        blunder      the chosen code is < 0 while a code >= 0 existed
        forced_loss  every legal code is < 0
        ok           anything else
    Returns {"label": [n names], "class": int64 [n] (index into TACTICAL_CLASSES), "chosen": int8 [n] (the chosen
    moves' codes), "counts": {name: count}}.  ValueError if a chosen move is illegal."""
    score = torch.as_tensor(score)
    action = torch.as_tensor(action).to(score.device, torch.int64).reshape(-1)
    n = score.shape[0]
    if action.shape[0] != n:
        raise ValueError(f"{n} score rows but {action.shape[0]} actions")
    s = score.long()
    chosen = s.gather(1, action.reshape(-1, 1)).reshape(-1) if n else s.reshape(-1)[:0]
    if bool((chosen == SOLVE_ILLEGAL).any()):
        raise ValueError("a chosen move is illegal (code -128)")
    legal = s != SOLVE_ILLEGAL
    big = torch.full_like(s, 1 << 20)
    fastest = torch.where(s > 0, s, big).min(dim=1).values if n else chosen  # the smallest +k (1 << 20: none)
    has_win = fastest < (1 << 20)
    safe = ((s >= 0) & legal).any(dim=1) if n else chosen > 0
    cls = torch.full((n,), TACTICAL_CLASSES.index("ok"), dtype=torch.int64, device=score.device)
    # assigned from the last rule to the first, so the first that applies stands
    cls[~safe] = TACTICAL_CLASSES.index("forced_loss")
    cls[(chosen < 0) & safe] = TACTICAL_CLASSES.index("blunder")
    cls[has_win & (chosen > fastest)] = TACTICAL_CLASSES.index("slower_win")
    cls[has_win & (chosen <= 0)] = TACTICAL_CLASSES.index("missed_win")
    label = [TACTICAL_CLASSES[i] for i in cls.tolist()]
    return {"label": label, "class": cls, "chosen": chosen.to(torch.int8),
            "counts": {name: label.count(name) for name in TACTICAL_CLASSES}}
