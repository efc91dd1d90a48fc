"""Python handle on one device arena (include/spmcts.h) — torch tensors in, torch tensors out.

All buffers handed to the library are torch tensors on the arena's device; the
library launches on `torch.cuda.current_stream()` of that device, so the
network that consumes the leaf rows runs on the same stream with no extra
synchronisation.  The only host round trip per simulation is reading the
number of leaf rows (`select()` returns it as a Python int).

Instantiated boards (`GAMES`): "connect4" (7x6), "connect4_6_5" (6x5), "connect4_8_7" (8x7) and "tictactoe"
(3x3), all in libspmcts.so.  The fused trunk of the 7x6 and 3x3 nets is in libspmcts.so too; that of the 6x5
and 8x7 nets is in the add-on library libspmcts_boards.so (`_lib.tower_lib`).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr

# name -> (game id, width, height, actions): the boards csrc/spmcts.hip with_game instantiates.  The Connect4
# variants carry the reference's variant_string() names (Connect4Env(6, 5) / Connect4Env(8, 7)).
GAMES = {"connect4": (_lib.CONNECT4, 7, 6, 7), "tictactoe": (_lib.TICTACTOE, 3, 3, 9),
         "connect4_6_5": (_lib.CONNECT4, 6, 5, 6), "connect4_8_7": (_lib.CONNECT4, 8, 7, 8)}
LEAF_FORMATS = {"f32": _lib.LEAF_F32, "f16": _lib.LEAF_F16, "bf16": _lib.LEAF_BF16, "board": _lib.LEAF_BOARD_I64}
_LEAF_DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "board": torch.int64}


def game_of_env(env):
    """Map a reference-style env (class or instance) to an arena game name.

    Accepts this package's envs and the reference's Connect4Env / TicTacToeEnv
    (games/connect4/connect4env.py, games/tictactoe/tictactoe_env.py) by shape.
    A Connect4 env of an instantiated size maps to its variant_string() name: "connect4" (7x6),
    "connect4_6_5", "connect4_8_7"; any other size raises a ValueError that lists the instantiated boards.
    """
    e = env() if isinstance(env, type) else env
    name = type(e).__name__.lower()
    w, h = getattr(e, "width", None), getattr(e, "height", None)
    n = e.action_space.n if hasattr(e, "action_space") else getattr(e, "n_actions", None)
    if "connect4" in name or (w, h, n) == (7, 6, 7):
        gid = _lib.CONNECT4
    elif "tictactoe" in name or (w, h, n) == (3, 3, 9):
        gid = _lib.TICTACTOE
    else:
        raise ValueError(f"unsupported environment {type(e).__name__}")
    for game, (g, W, H, A) in GAMES.items():
        if g == gid and (w, h) == (W, H):
            return game
    kind = "connect4" if gid == _lib.CONNECT4 else "tictactoe"
    built = ", ".join(f"{W}x{H} ({game})" for game, (g, W, H, A) in GAMES.items() if g == gid)
    raise ValueError(f"the {kind} arena is instantiated for these boards only: {built}; got {w}x{h}")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Arena:
    """A device-resident forest of MCTS trees (+ optional self-play game slots)."""

    def __init__(self, game="connect4", n_trees=2, n_games=0, iterations=100, rng="philox", seed=0,
                 subsequence0=0, strong_play=False, evaluate=False, leaf_format="bf16", leaf_layout="nchw",
                 cpuct=4.0, x_noise=0.25, alpha=1.0, blocks_per_tree=0, device=None, search_threads=1):
        if not torch.cuda.is_available():
            raise _lib.SpmctsError("the HIP arena needs a GPU (torch.cuda.is_available() is False)")
        gid, W, H, A = GAMES[game]
        self.game, self.W, self.H, self.A = game, W, H, A
        self.cells = W * H
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else
                                   torch.device(device).index or 0)
        self.n_trees, self.n_games = n_trees, n_games
        self.leaf_format, self.leaf_layout = leaf_format, leaf_layout
        cfg = _lib.Config()
        cfg.game, cfg.width, cfg.height = gid, W, H
        cfg.n_trees, cfg.n_games, cfg.iterations = n_trees, n_games, iterations
        cfg.blocks_per_tree = blocks_per_tree
        cfg.rng_mode = _lib.RNG_TAPE if rng == "tape" else _lib.RNG_PHILOX
        cfg.strong_play, cfg.evaluate = int(bool(strong_play)), int(bool(evaluate))
        cfg.leaf_format = LEAF_FORMATS[leaf_format]
        cfg.leaf_layout = _lib.NHWC if leaf_layout == "nhwc" else _lib.NCHW
        cfg.compact = 1
        # K simulations in flight per tree with virtual loss (mcts.py:328-331); rows = n_trees * K
        self.search_threads = K = max(1, int(search_threads))
        cfg.search_threads = K
        cfg.cpuct, cfg.x_noise, cfg.alpha = float(cpuct), float(x_noise), float(alpha)
        cfg.seed, cfg.subsequence0 = int(seed) & (2**64 - 1), int(subsequence0)
        self.cfg = cfg
        L = _lib.lib()
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            call("spmcts_arena_create", ctypes.byref(cfg), self.device.index, ctypes.byref(h))
        self.h = h
        geo = [ctypes.c_int32() for _ in range(6)]
        call("spmcts_arena_geometry", h, *[ctypes.byref(g) for g in geo])
        self.blocks_per_tree = geo[3].value
        dev = self.device
        rows = max(n_trees * K, n_games, 1)
        self.max_rows = rows
        if leaf_format == "board":
            self._leaves = torch.zeros((rows, W, H), dtype=torch.int64, device=dev)
        elif leaf_layout == "nhwc":
            self._leaves = torch.zeros((rows, W, H, 3), dtype=_LEAF_DTYPES[leaf_format], device=dev)
        else:
            self._leaves = torch.zeros((rows, 3, W, H), dtype=_LEAF_DTYPES[leaf_format], device=dev)
        self._count = torch.zeros(4, dtype=torch.int32, device=dev)
        self._count_host = torch.zeros(4, dtype=torch.int32).pin_memory()
        self._finish = torch.zeros(2, dtype=torch.int32, device=dev)
        self._i32 = torch.zeros(rows, dtype=torch.int32, device=dev)
        self._i8 = torch.zeros(rows, dtype=torch.int8, device=dev)
        self.n_active = 0
        self.seg1 = n_trees * K  # first leaf row of network 1 (two-network arenas)
        self._L = L

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            _lib.lib().spmcts_arena_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _dev_i32(self, xs):
        return torch.as_tensor(np.asarray(xs, dtype=np.int32)).to(self.device)

    def _dev_i8(self, xs):
        return torch.as_tensor(np.asarray(xs, dtype=np.int8)).to(self.device)

    def leaves(self, n):
        """Leaf rows [:n] as the network's input tensor ([n, 3, W, H]; channels_last if NHWC)."""
        x = self._leaves[:n]
        if self.leaf_format != "board" and self.leaf_layout == "nhwc":
            x = x.permute(0, 3, 1, 2)  # NCHW view with channels_last strides
        return x

    def leaves_from(self, row0, n):
        """Leaf rows [row0, row0 + n) (network-1 rows start at `seg1`)."""
        x = self._leaves[row0:row0 + n]
        if self.leaf_format != "board" and self.leaf_layout == "nhwc":
            x = x.permute(0, 3, 1, 2)
        return x

    def _read_count(self):
        self._count_host.copy_(self._count, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return int(self._count_host[0])

    def segment_counts(self):
        """(network-0 rows, network-1 rows) of the last select / play_action / games_end_ply (sync)."""
        self._count_host.copy_(self._count, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return int(self._count_host[1]), int(self._count_host[2])

    # ------------------------------------------------------------------ configuration
    def set_root_prior(self, probs, net=0):
        p = torch.as_tensor(probs, dtype=torch.float32).to(self.device).contiguous()
        if net == 0:
            self._root_prior = p
            call("spmcts_set_root_prior", self.h, ptr(p), _stream())
        else:
            self._root_prior1 = p
            call("spmcts_set_root_prior_net", self.h, int(net), ptr(p), _stream())

    def set_tree_players(self, nets=None, kinds=None, budgets=None):
        """Per-tree network id (0/1), player kind (_lib.PLAYER_*) and simulations per search.

        Network-1 leaves are written from row `seg1` (= number of network-0 trees) on."""
        T = self.n_trees

        def arr(x, ctype, dtype):
            if x is None:
                return None
            a = np.ascontiguousarray(np.asarray(x, dtype=dtype))
            if a.shape != (T,):
                raise ValueError(f"expected {T} per-tree entries, got {a.shape}")
            return a.ctypes.data_as(ctypes.POINTER(ctype)), a

        n = arr(nets, ctypes.c_uint8, np.uint8)
        k = arr(kinds, ctypes.c_uint8, np.uint8)
        b = arr(budgets, ctypes.c_int32, np.int32)
        torch.cuda.current_stream().synchronize()
        call("spmcts_set_tree_players", self.h, n[0] if n else None, k[0] if k else None, b[0] if b else None)
        seg = ctypes.c_int32()
        call("spmcts_arena_segments", self.h, ctypes.byref(seg))
        self.seg1 = seg.value

    def set_tree_search(self, alpha=None, strong_play=None, search_threads=None):
        """Per-tree search settings (include/spmcts.h spmcts_set_tree_search): each side of an
        evaluation game searches with its own MCTreeSearch kwargs (selfplayworker.py:71-81):
        Dirichlet alpha, strong_play, sims in flight (1 .. this arena's search_threads).  None =
        unchanged."""
        T = self.n_trees

        def arr(x, ctype, dtype):
            if x is None:
                return None
            a = np.ascontiguousarray(np.asarray(x, dtype=dtype))
            if a.shape != (T,):
                raise ValueError(f"expected {T} per-tree entries, got {a.shape}")
            return a.ctypes.data_as(ctypes.POINTER(ctype)), a

        al = arr(alpha, ctypes.c_double, np.float64)
        st = arr(strong_play, ctypes.c_uint8, np.uint8)
        k = arr(search_threads, ctypes.c_int32, np.int32)
        torch.cuda.current_stream().synchronize()
        call("spmcts_set_tree_search", self.h, al[0] if al else None, st[0] if st else None, k[0] if k else None)
        if search_threads is not None:
            self.tree_threads = np.asarray(search_threads, dtype=np.int64)

    def games_set_record(self, record=True):
        call("spmcts_games_set_record", self.h, int(bool(record)))

    def set_leaf_dedup(self, on=True):
        """One leaf row per distinct network input of a simulation step (search_threads > 1;
        include/spmcts.h spmcts_set_leaf_dedup).  Only for evaluators that are a pure function of the
        leaf planes (the ResNet evaluators), not for per-row salted table nets."""
        call("spmcts_set_leaf_dedup", self.h, int(bool(on)))
        self.leaf_dedup = bool(on) and self.search_threads > 1

    symmetry = None

    def set_symmetry(self, mode):
        """Mirror symmetry (include/spmcts.h spmcts_set_symmetry): "mirror" puts every leaf's network input in
        canonical form (symmetry.canonical), so a position and its mirror image share one row, one peer row and
        one cache record, and the search runs symmetry.SymmetricNet of the network.  None: off (the default).
        Before the arena's first search or game start and before set_leaf_peer; SpmctsError (-2) afterwards."""
        call("spmcts_set_symmetry", self.h, symmetry_mode(mode))
        self.symmetry = "mirror" if symmetry_mode(mode) else None

    def leaf_rows(self):
        """The pending leaves gathered into network rows, as the network's input tensor (sync on the count)."""
        self.leaf_rows_async()
        return self.leaves(self._read_count())

    def set_leaf_peer(self, leader):
        """Cross-lane leaf dedup (include/spmcts.h spmcts_set_leaf_peer): in each simulation step a pending leaf
        whose network input `leader` (another lane's arena, stepped first) evaluates in the same step takes the
        leader's row.  The follower's simulation-step expand is then preceded by peer_push.  None unpairs."""
        call("spmcts_set_leaf_peer", self.h, None if leader is None else leader.h)
        self._leader = leader  # the leader outlives the pairing (its destroy unpairs its followers)

    def peer_push(self, probs, values, leader_probs, leader_values, leader_stream):
        """Before expand() of a follower lane's simulation step: the leader's outputs of the step (its
        evaluator's output buffers, valid on `leader_stream`) fill the leader-served rows of probs / values."""
        assert probs.dtype == torch.float32 and probs.is_contiguous() and values.is_contiguous()
        assert leader_probs.dtype == torch.float32 and leader_probs.is_contiguous() and leader_values.is_contiguous()
        call("spmcts_peer_push", self.h, ptr(probs), ptr(values), ptr(leader_probs), ptr(leader_values), _stream(),
             ctypes.c_void_p(leader_stream.cuda_stream))

    def set_eval_cache(self, window, capacity_log2=0):
        """Evaluation cache (include/spmcts.h spmcts_set_eval_cache): a leaf whose network input this arena
        evaluated in the last `window` plies (searches) takes those outputs instead of a row of its own; 0 =
        off.  Needs leaf dedup (idle without it).  Same evaluator contract as leaf dedup (pure,
        batch-independent; the two networks of an evaluation arena keep separate keys); call eval_cache_clear()
        when the weights change."""
        torch.cuda.current_stream().synchronize()
        call("spmcts_set_eval_cache", self.h, int(window), int(capacity_log2))
        self.eval_cache = int(window)

    def set_sim_cap(self, cap):
        """Sims one tree may start per kernel launch (include/spmcts.h spmcts_set_sim_cap): 0 = off, else at
        least 2 * search_threads.  Results do not depend on it."""
        call("spmcts_set_sim_cap", self.h, int(cap))

    def sim_pauses(self):
        """Tree-launches that paused at the sim cap so far (sync)."""
        n = ctypes.c_int64()
        call("spmcts_get_sim_pauses", self.h, ctypes.byref(n))
        return n.value

    def eval_cache_clear(self):
        call("spmcts_eval_cache_clear", self.h)

    def set_tapes(self, tapes):
        """Parity mode: one flat float64 stream per tree (list indexed by tree id)."""
        offs = np.zeros(self.n_trees + 1, dtype=np.int64)
        for t in range(self.n_trees):
            offs[t + 1] = offs[t] + (len(tapes[t]) if t < len(tapes) and tapes[t] is not None else 0)
        flat = np.concatenate([np.asarray(tapes[t], dtype=np.float64) for t in range(min(len(tapes), self.n_trees))
                               if tapes[t] is not None] + [np.zeros(1)])
        self._tape = torch.as_tensor(flat).to(self.device)
        self._tape_offs = torch.as_tensor(offs).to(self.device)
        call("spmcts_set_tape", self.h, ptr(self._tape), ptr(self._tape_offs), _stream())

    # ------------------------------------------------------------------ tree API
    def tree_reset(self, trees, players, priors=None):
        """priors: optional float32 [n, A] per-tree root priors (default: the arena's root prior)."""
        t = self._dev_i32(trees)
        p = self._dev_i8(players)
        pr = None if priors is None else torch.as_tensor(priors, dtype=torch.float32).to(self.device).contiguous()
        call("spmcts_tree_reset", self.h, ptr(t), ptr(p), ptr(pr), len(trees), _stream())

    def search_begin(self, trees):
        t = self._dev_i32(trees)
        self._active = t
        self.n_active = len(trees)
        call("spmcts_search_begin", self.h, ptr(t), len(trees), _stream())

    def select(self, timer=None):
        """One simulation for every active tree; returns the number of leaf rows to evaluate.

        `timer` (optional): object with start()/stop() bracketing the tree-walk kernel alone
        (HIP events on this stream, used by bench.py for the select roofline)."""
        if timer is None:
            call("spmcts_select", self.h, ptr(self._leaves), ptr(self._count), _stream())
        else:
            timer.start()
            call("spmcts_select_tree", self.h, _stream())
            timer.stop()
            call("spmcts_leaf_rows", self.h, ptr(self._leaves), ptr(self._count), _stream())
        return self._read_count()

    def select_async(self, timer=None):
        """select() without reading the row count back (for device-count evaluators)."""
        if timer is None:
            call("spmcts_select", self.h, ptr(self._leaves), ptr(self._count), _stream())
        else:
            timer.start()
            call("spmcts_select_tree", self.h, _stream())
            timer.stop()
            call("spmcts_leaf_rows", self.h, ptr(self._leaves), ptr(self._count), _stream())

    def leaf_rows_async(self):
        """Gather the pending leaves into network rows (k_scan_need + k_encode) without a select."""
        call("spmcts_leaf_rows", self.h, ptr(self._leaves), ptr(self._count), _stream())

    def games_end_ply_async(self):
        call("spmcts_games_end_ply", self.h, ptr(self._leaves), ptr(self._count), _stream())

    @property
    def count_dev(self):
        """Device int32 holding the row count of the last select / play_action / games_end_ply."""
        return self._count

    def segment_count_dev(self, net):
        """Device int32 holding network `net`'s row count (element 1 + net of the count buffer)."""
        return self._count[1 + net:2 + net]

    def expand(self, probs, values):
        probs = probs.float().contiguous()
        values = values.float().reshape(-1).contiguous()
        call("spmcts_expand", self.h, ptr(probs), ptr(values), _stream())

    def expand2(self, probs0, values0, probs1, values1):
        """Two-network expand: network-0 outputs by row, network-1 outputs by row - seg1."""
        t = [x.float().contiguous() if x.dtype != torch.float32 or not x.is_contiguous() else x
             for x in (probs0, values0.reshape(-1), probs1, values1.reshape(-1))]
        call("spmcts_expand2", self.h, *[ptr(x) for x in t], _stream())

    def search_end(self, temp=1.0):
        n = self.n_active
        dev = self.device
        out = dict(
            action=torch.zeros(n, dtype=torch.int32, device=dev),
            state=torch.zeros((n, self.cells), dtype=torch.int8, device=dev),
            tree_probs=torch.zeros((n, self.A), dtype=torch.float32, device=dev),
            q=torch.zeros(n, dtype=torch.float64, device=dev),
            q_f64=torch.zeros(n, dtype=torch.uint8, device=dev),
            recorded=torch.zeros(n, dtype=torch.uint8, device=dev),
        )
        call("spmcts_search_end", self.h, float(temp), ptr(out["action"]), ptr(out["state"]), ptr(out["tree_probs"]),
             ptr(out["q"]), ptr(out["q_f64"]), ptr(out["recorded"]), _stream())
        return out

    def play_action(self, trees, actions):
        t = self._dev_i32(trees)
        a = self._dev_i32(actions)
        call("spmcts_play_action", self.h, ptr(t), ptr(a), len(trees), ptr(self._leaves), ptr(self._count), _stream())
        return self._read_count()

    def leaf_trees(self, n):
        """Tree id of each of the first n leaf rows (device int32 tensor)."""
        out = torch.empty(self.n_trees * self.search_threads, dtype=torch.int32, device=self.device)
        call("spmcts_leaf_trees", self.h, ptr(out), _stream())
        out = out[:n]
        return out // self.search_threads if self.search_threads > 1 else out

    def root_stats(self, tree):
        A, cells = self.A, self.cells
        cn = (ctypes.c_int32 * A)()
        cw = (ctypes.c_double * A)()
        cp = (ctypes.c_float * A)()
        rn, rw, rp = ctypes.c_int32(), ctypes.c_double(), ctypes.c_int32()
        board = (ctypes.c_int8 * cells)()
        torch.cuda.current_stream().synchronize()
        call("spmcts_root_stats", self.h, int(tree), cn, cw, cp, ctypes.byref(rn), ctypes.byref(rw), ctypes.byref(rp),
             board)
        return dict(child_n=list(cn), child_w=list(cw), child_p=list(cp), root_n=rn.value, root_w=rw.value,
                    root_player=rp.value, board=np.array(list(board), dtype=np.int8).reshape(self.W, self.H))

    def root_stats_batch(self, trees):
        """root_stats of the listed trees (a list or a device int32 tensor) as device tensors, queued on the
        current stream without a host synchronisation (include/spmcts.h spmcts_root_stats_batch): child_n int32
        [n, A], child_w float64 [n, A], child_p float32 [n, A], root_n int32 [n], root_w float64 [n], root_player
        int8 [n], board int8 [n, W, H]."""
        t = trees.to(self.device, torch.int32).contiguous() if torch.is_tensor(trees) else self._dev_i32(trees)
        n, A, dev = int(t.numel()), self.A, self.device
        out = dict(child_n=torch.zeros((n, A), dtype=torch.int32, device=dev),
                   child_w=torch.zeros((n, A), dtype=torch.float64, device=dev),
                   child_p=torch.zeros((n, A), dtype=torch.float32, device=dev),
                   root_n=torch.zeros(n, dtype=torch.int32, device=dev),
                   root_w=torch.zeros(n, dtype=torch.float64, device=dev),
                   root_player=torch.zeros(n, dtype=torch.int8, device=dev),
                   board=torch.zeros((n, self.W, self.H), dtype=torch.int8, device=dev))
        call("spmcts_root_stats_batch", self.h, ptr(t), n, ptr(out["child_n"]), ptr(out["child_w"]),
             ptr(out["child_p"]), ptr(out["root_n"]), ptr(out["root_w"]), ptr(out["root_player"]), ptr(out["board"]),
             _stream())
        self._stats_trees = t  # alive until the kernel has run
        return out

    def pv_batch(self, trees, max_len=None, min_visits=1):
        """The principal variation of the listed trees (a list or a device int32 tensor) as device tensors, queued
        on the current stream without a host synchronisation (include/spmcts.h spmcts_tree_pv_batch): from the
        active root the most visited child, the lowest action on ties, while it has at least max(min_visits, 1)
        visits, for at most max_len moves (default: the board's cells).  pv int8 [n, max_len] (-1 past the end),
        pv_n / pv_vl int32, pv_w float64, pv_p float32 [n, max_len] (the chosen children's fields, 0 past the end),
        pv_len int32 [n], pv_end uint8 [n] (0 cut at max_len, 1 no child with enough visits, 2 the game ended),
        end_board int8 [n, W, H] (tree frame)."""
        t = trees.to(self.device, torch.int32).contiguous() if torch.is_tensor(trees) else self._dev_i32(trees)
        n, dev = int(t.numel()), self.device
        L = self.cells if max_len is None else int(max_len)
        out = dict(pv=torch.full((n, L), -1, dtype=torch.int8, device=dev),
                   pv_n=torch.zeros((n, L), dtype=torch.int32, device=dev),
                   pv_vl=torch.zeros((n, L), dtype=torch.int32, device=dev),
                   pv_w=torch.zeros((n, L), dtype=torch.float64, device=dev),
                   pv_p=torch.zeros((n, L), dtype=torch.float32, device=dev),
                   pv_len=torch.zeros(n, dtype=torch.int32, device=dev),
                   pv_end=torch.zeros(n, dtype=torch.uint8, device=dev),
                   end_board=torch.zeros((n, self.W, self.H), dtype=torch.int8, device=dev))
        call("spmcts_tree_pv_batch", self.h, ptr(t), n, L, int(min_visits), ptr(out["pv"]), ptr(out["pv_n"]),
             ptr(out["pv_vl"]), ptr(out["pv_w"]), ptr(out["pv_p"]), ptr(out["pv_len"]), ptr(out["pv_end"]),
             ptr(out["end_board"]), _stream())
        self._pv_trees = t  # alive until the kernel has run
        return out

    EXPORT_FIELDS = (("parent", torch.int32, -1), ("action", torch.int8, -1), ("depth", torch.int16, 0),
                     ("node_n", torch.int32, 0), ("node_vl", torch.int32, 0), ("node_w", torch.float64, 0),
                     ("node_p", torch.float32, 0), ("player", torch.int8, 0), ("flags", torch.uint8, 0))

    EXPORT_BOUND_FIELDS = (("move_lo", torch.int8, -128), ("move_hi", torch.int8, -128))

    def export_subtrees(self, trees, max_nodes, min_visits=1, max_depth=None, out=None, bounds=False):
        """The subtree under the active root of the listed trees in breadth-first order as device tensors, queued
        on the current stream without a host synchronisation (include/spmcts.h spmcts_tree_export_batch).  Row i
        lists tree trees[i]: entry 0 the root, then for each entry in order its children with at least min_visits
        visits (0: every child of every expanded node) at a depth of at most max_depth (None: no limit), in action
        order.  [n, max_nodes] each, padded: parent int32 (-1 for the root and the padding), action int8 (-1
        likewise), depth int16, node_n / node_vl int32, node_w float64, node_p float32, player int8, flags uint8
        (bit 0 expanded, bit 1 valid, bit 2 terminal); count int32 [n], the nodes that qualify: where it exceeds
        max_nodes the first max_nodes are there and the call may be repeated with more room (tree.TreeView's
        `truncated`).  out: a dict of the caller's own contiguous device tensors to write into instead of new ones
        (the same keys and dtypes; rows of max_nodes entries from the start of each, so at least n * max_nodes
        elements; whatever lies past them is not touched).  bounds=True (an arena with stored bounds,
        set_stored_bounds; spmcts_tree_export_bounds_batch): two more columns, move_lo / move_hi int8, each node's
        stored entry -- the score bounds of the move into it, seen from its parent; -128 for the root, an illegal
        move and the padding (tree.TreeView.node_bounds recomputes them on the host)."""
        t = trees.to(self.device, torch.int32).contiguous() if torch.is_tensor(trees) else self._dev_i32(trees)
        n, M, dev = int(t.numel()), int(max_nodes), self.device
        fields = self.EXPORT_FIELDS + (self.EXPORT_BOUND_FIELDS if bounds else ())
        if out is None:
            out = {k: torch.full((n, M), fill, dtype=dt, device=dev) for k, dt, fill in fields}
            out["count"] = torch.zeros(n, dtype=torch.int32, device=dev)
        else:
            for k, dt, _ in fields + (("count", torch.int32, 0),):
                need = n if k == "count" else n * max(M, 0)
                if out[k].dtype != dt or out[k].device != dev or not out[k].is_contiguous() or out[k].numel() < need:
                    raise ValueError(f"export_subtrees: out[{k!r}] must be a contiguous {dt} tensor on {dev} with at "
                                     f"least {need} elements")
        nbytes = ctypes.c_uint64()
        call("spmcts_tree_export_work_bytes", self.h, n, M, ctypes.byref(nbytes))
        work = torch.empty((nbytes.value + 7) // 8, dtype=torch.int64, device=dev)
        depth = -1 if max_depth is None else int(max_depth)
        call("spmcts_tree_export_bounds_batch" if bounds else "spmcts_tree_export_batch", self.h, ptr(t), n, M,
             int(min_visits), depth, *[ptr(out[k]) for k, _, _ in self.EXPORT_FIELDS], ptr(out["count"]),
             *[ptr(out[k]) for k, _, _ in (self.EXPORT_BOUND_FIELDS if bounds else ())], ptr(work), nbytes.value,
             _stream())
        self._export_keep = (t, work)  # alive until the kernel has run
        return out

    BOUNDS_FIELDS = ("lo", "hi", "move_lo", "move_hi", "best", "empty", "nodes")

    def bounds_batch(self, trees):
        """What the listed trees (a list or a device int32 tensor) prove about the exact score s of their root
        positions, as device tensors, queued on the current stream without a host synchronisation (include/spmcts.h
        spmcts_tree_bounds_batch): a minimax over each stored tree in which an unexpanded node may still be worth
        anything.  lo, hi int8 [n]: lo <= s <= hi (lo == hi: the search has solved the position); move_lo, move_hi
        int8 [n, A]: the same per root move, -128 in both for an illegal move; best int8 [n]: the lowest action with
        move_lo == lo; empty int8 [n]: the root's empty cells; nodes int32 [n]: the expanded nodes walked.
        tree.bounds_to_codes turns the values into the solvers' move codes, tree.classify_bounds names the case."""
        t = trees.to(self.device, torch.int32).contiguous() if torch.is_tensor(trees) else self._dev_i32(trees)
        n, dev = int(t.numel()), self.device
        i8 = lambda *shape: torch.full(shape, -128, dtype=torch.int8, device=dev)  # noqa: E731
        out = dict(lo=i8(n), hi=i8(n), move_lo=i8(n, self.A), move_hi=i8(n, self.A), best=i8(n), empty=i8(n),
                   nodes=torch.zeros(n, dtype=torch.int32, device=dev))
        call("spmcts_tree_bounds_batch", self.h, ptr(t), n, *[ptr(out[k]) for k in self.BOUNDS_FIELDS], _stream())
        self._bounds_trees = t  # alive until the kernel has run
        return out

    # ------------------------------------------------------------------ stored score bounds
    stored_bounds = False

    def set_stored_bounds(self):
        """Keep the score bounds in the nodes from now on (include/spmcts.h spmcts_set_solver_search): every child
        block carries its moves' move_lo / move_hi, stamped when the block is created and carried up the expansion's
        path, so that they equal bounds_batch's walk on the tree as it stands.  The search does not read them (its
        results are bit-identical) unless set_solver_rules says so; the proof-play verdict, proof_moves_batch and proof_stop then read the root's
        block and walk nothing, and export_subtrees(bounds=True) lists them.  Before the first search only;
        synchronises; cannot be switched off."""
        self.set_solver_search(False)

    def set_solver_search(self, on=False):
        """include/spmcts.h spmcts_set_solver_search: `on`, True / False for every tree or one flag per tree, says
        whose search uses the stored bounds; the first call starts their maintenance for the whole arena (before
        the first search only).  It is the maintenance switch alone: a flag that is on raises SpmctsError (-2) and
        changes nothing, and set_solver_search(False) is set_stored_bounds().  The rules that read the bounds during
        a search are switched by set_solver_rules.  Synchronises."""
        torch.cuda.current_stream().synchronize()
        if isinstance(on, (bool, int, np.bool_)):
            flags = np.full(self.n_trees, 1 if on else 0, dtype=np.uint8)
        else:
            flags = np.ascontiguousarray(np.asarray(on, dtype=bool).astype(np.uint8))
            if flags.shape != (self.n_trees,):
                raise ValueError(f"expected {self.n_trees} per-tree entries, got {flags.shape}")
        call("spmcts_set_solver_search", self.h, flags.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
        self.stored_bounds = True

    # ------------------------------------------------------------------ solver-aware search
    SOLVER_REFUTE, SOLVER_PROVED = 1, 2
    SOLVER_STATS = ("proved", "refuted_levels")
    _solver_rules = None

    @property
    def solver_rules(self):
        """The trees' rule bits as last set (numpy uint8 [T]; all 0 on an arena that never set any)."""
        if self._solver_rules is None:
            return np.zeros(self.n_trees, dtype=np.uint8)
        return self._solver_rules

    def _per_tree_bool(self, x):
        if isinstance(x, (bool, int, np.bool_)):
            return np.full(self.n_trees, bool(x))
        f = np.asarray(x, dtype=bool)
        if f.shape != (self.n_trees,):
            raise ValueError(f"expected {self.n_trees} per-tree entries, got {f.shape}")
        return f

    def set_solver_rules(self, refute=True, proved=True):
        """The search rules that read the stored bounds (include/spmcts.h spmcts_set_solver_rules; the host form is
        tree.solver_select): refute, a child that cannot reach what a sibling already secures scores like an
        invalid one; proved, a sim whose chosen child is solved ends there with the proved value and buys no row.
        Each a bool for every tree or one flag per tree.  Off by default.  Switches the stored bounds on first if
        they are off (before the first search only).  Synchronises; takes effect at the next launch."""
        bits = (self._per_tree_bool(refute) * self.SOLVER_REFUTE + self._per_tree_bool(proved) * self.SOLVER_PROVED)
        bits = np.ascontiguousarray(bits.astype(np.uint8))
        if not self.stored_bounds:
            self.set_stored_bounds()
        torch.cuda.current_stream().synchronize()
        call("spmcts_set_solver_rules", self.h, bits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
        self._solver_rules = bits

    def solver_stats(self, per_tree=False):
        """Counts of the search rules so far (spmcts_get_solver_stats; sync): proved, the sims that ended at a
        solved child; refuted_levels, the select levels at which the refute rule removed at least one child that
        was otherwise valid.  per_tree=True: a device int64 [T][2] tensor instead, no host sync."""
        if per_tree:
            out = torch.empty((self.n_trees, len(self.SOLVER_STATS)), dtype=torch.int64, device=self.device)
            call("spmcts_solver_stats_trees", self.h, ptr(out), _stream())
            return out
        out = (ctypes.c_int64 * len(self.SOLVER_STATS))()
        call("spmcts_get_solver_stats", self.h, out)
        return dict(zip(self.SOLVER_STATS, (int(x) for x in out)))

    def search_progress(self):
        """Per tree, device int32 [T] each, no host sync (spmcts_search_progress): started, the search_node calls
        the current search has started (0x3fffffff: none in progress, or stopped by proof_stop); resume, the slot
        the tree's cycle goes on at * 2, + 1 while the sim cap has it paused inside a fill."""
        out = dict(started=torch.empty(self.n_trees, dtype=torch.int32, device=self.device),
                   resume=torch.empty(self.n_trees, dtype=torch.int32, device=self.device))
        call("spmcts_search_progress", self.h, ptr(out["started"]), ptr(out["resume"]), _stream())
        return out

    # ------------------------------------------------------------------ proof-guided play
    PROOF_STATS = ("plies", "solved", "secured_win", "restricted", "trees_stopped", "sims_skipped")

    def set_proof_play(self, on=True):
        """Let the move choice use what the tree has proved (include/spmcts.h spmcts_set_proof_play): before a move
        is chosen, the moves outside the tree's keep set (tree.proof_move_set of its score bounds) lose their visit
        weight.  `on`: True / False for every tree, or one flag per tree.  Off by default; synchronises."""
        torch.cuda.current_stream().synchronize()
        if isinstance(on, (bool, int, np.bool_)):
            flags = np.full(self.n_trees, 1 if on else 0, dtype=np.uint8)
        else:
            flags = np.ascontiguousarray(np.asarray(on, dtype=bool).astype(np.uint8))
            if flags.shape != (self.n_trees,):
                raise ValueError(f"expected {self.n_trees} per-tree entries, got {flags.shape}")
        call("spmcts_set_proof_play", self.h, flags.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
        self.proof_play = flags.astype(bool)

    def proof_moves_batch(self, trees):
        """The verdict of the listed trees (a list or a device int32 tensor) as they stand, as device tensors,
        queued on the current stream without a host synchronisation and at any point of a search
        (spmcts_tree_proof_moves_batch): keep int32 [n], bit a set: move a is in the keep set (tree.proof_move_set of
        bounds_batch's values); lo, hi int8 [n], the root's score bounds.  Whatever the trees' proof_play flags."""
        t = trees.to(self.device, torch.int32).contiguous() if torch.is_tensor(trees) else self._dev_i32(trees)
        n, dev = int(t.numel()), self.device
        out = dict(keep=torch.full((n,), -1, dtype=torch.int32, device=dev),
                   lo=torch.full((n,), -128, dtype=torch.int8, device=dev),
                   hi=torch.full((n,), -128, dtype=torch.int8, device=dev))
        call("spmcts_tree_proof_moves_batch", self.h, ptr(t), n, ptr(out["keep"]), ptr(out["lo"]), ptr(out["hi"]),
             _stream())
        self._proof_trees = t  # alive until the kernel has run
        return out

    def proof_last(self):
        """What the last games_end_ply / search_end decided with, per tree, as device tensors (spmcts_proof_last):
        keep int32 [T] (-1, all bits: no restriction -- the feature off for the tree, a hard-coded player, a book
        ply), lo, hi int8 [T] (-128 beside -1).  A tree that chose no move keeps its earlier row."""
        T, dev = self.n_trees, self.device
        out = dict(keep=torch.empty(T, dtype=torch.int32, device=dev), lo=torch.empty(T, dtype=torch.int8, device=dev),
                   hi=torch.empty(T, dtype=torch.int8, device=dev))
        call("spmcts_proof_last", self.h, ptr(out["keep"]), ptr(out["lo"]), ptr(out["hi"]), _stream())
        return out

    def proof_stats(self):
        """Counts of proof-guided play so far (sync; spmcts_get_proof_stats): plies chosen with it on, those with a
        solved root, with a secured win, with fewer kept moves than legal ones (restricted); trees_stopped and
        sims_skipped of proof_stop."""
        out = (ctypes.c_int64 * len(self.PROOF_STATS))()
        call("spmcts_get_proof_stats", self.h, out)
        return dict(zip(self.PROOF_STATS, (int(x) for x in out)))

    def proof_stop(self):
        """Between two simulation steps of a threaded search: every searching tree with proof play on whose root
        is now solved starts no more sims (spmcts_proof_stop).  Queued on the current stream, no host sync."""
        call("spmcts_proof_stop", self.h, _stream())

    def proof_stopped(self):
        """Per tree, device int32 [T]: the searches of the tree that proof_stop has stopped so far (no host sync)."""
        out = torch.empty(self.n_trees, dtype=torch.int32, device=self.device)
        call("spmcts_proof_stopped", self.h, ptr(out), _stream())
        return out

    # ------------------------------------------------------------------ games API
    def games_set_openings(self, openings, id_period=0):
        """The arena's opening book (include/spmcts.h spmcts_games_set_openings): `openings` a list of move
        lists from the empty board; game id i plays opening ((i mod id_period) >> 1) mod len(openings), its book
        plies without a search.  None or [] turns the book off.  Raises SpmctsError for a sequence with an illegal
        or game-ending move ("opening I ply P: ..."), an odd id_period, or while a game is active."""
        from .openings import pack_openings

        moves, lens, max_len = pack_openings(openings or [])
        torch.cuda.current_stream().synchronize()
        call("spmcts_games_set_openings", self.h, moves.ctypes.data_as(ctypes.c_void_p),
             lens.ctypes.data_as(ctypes.c_void_p), len(lens), max_len, int(id_period))
        self.n_openings = len(lens)

    def games_openings(self):
        """Opening index of each slot's game (sync; -1: an idle slot, or no book)."""
        out = np.zeros(max(self.n_games, 1), dtype=np.int32)
        torch.cuda.current_stream().synchronize()
        call("spmcts_games_openings", self.h, out.ctypes.data_as(ctypes.c_void_p))
        return out[:self.n_games]

    def games_start(self, slots, priors=None):
        """priors: optional float32 [n, 2, A] (policy tree, opponent tree) root priors per game."""
        s = self._dev_i32(slots)
        pr = None if priors is None else torch.as_tensor(priors, dtype=torch.float32).to(self.device).contiguous()
        call("spmcts_games_start", self.h, ptr(s), ptr(pr), len(slots), _stream())

    def games_set_limit(self, max_games):
        torch.cuda.current_stream().synchronize()
        call("spmcts_games_set_limit", self.h, int(max_games))

    def games_begin_ply(self):
        self.n_active = self.n_games
        call("spmcts_games_begin_ply", self.h, _stream())

    def games_end_ply(self):
        call("spmcts_games_end_ply", self.h, ptr(self._leaves), ptr(self._count), _stream())
        return self._read_count()

    def games_finish_ply(self, refill=True):
        call("spmcts_games_finish_ply", self.h, int(bool(refill)), ptr(self._finish), _stream())
        f = self._finish.cpu()
        return int(f[0]), int(f[1])

    def finish_export_async(self, refill=True):
        """games_finish_ply + export_moves of the whole export ring without a host synchronisation: the records go
        to persistent buffers of the ring's capacity and the counts to pinned host memory; returns an event for
        finish_export_result.  Several lanes can queue theirs before the host waits on any of them."""
        if getattr(self, "_exp", None) is None:
            cap = max(64, 4 * self.n_games * ((self.cells + 1) // 2 + 1))  # spmcts.hip plan_arena: ex_cap (MAXM)
            dev = self.device
            self._exp = dict(
                state=torch.empty((cap, self.cells), dtype=torch.int8, device=dev),
                tree_probs=torch.empty((cap, self.A), dtype=torch.float32, device=dev),
                q=torch.empty(cap, dtype=torch.float64, device=dev),
                q_f64=torch.empty(cap, dtype=torch.uint8, device=dev),
                z=torch.empty(cap, dtype=torch.float32, device=dev),
                game=torch.empty(cap, dtype=torch.int64, device=dev),
            )
            self._exp_cap = cap
            self._exp_count = torch.zeros(4, dtype=torch.int32, device=dev)
            self._exp_host = torch.zeros(3, dtype=torch.int32).pin_memory()
        e = self._exp
        call("spmcts_games_finish_ply", self.h, int(bool(refill)), ptr(self._finish), _stream())
        call("spmcts_export_moves", self.h, ptr(e["state"]), ptr(e["tree_probs"]), ptr(e["q"]), ptr(e["q_f64"]),
             ptr(e["z"]), ptr(e["game"]), self._exp_cap, ptr(self._exp_count), _stream())
        self._exp_host[0:2].copy_(self._finish, non_blocking=True)
        self._exp_host[2:3].copy_(self._exp_count[0:1], non_blocking=True)
        if getattr(self, "games_log", False):  # the finished-game ring rides along: same buffers every ply, same event
            if getattr(self, "_gexp", None) is None:
                self._gexp = self._game_buffers(2 * self.n_games)  # the ring's capacity (spmcts_games_set_log)
                self._gexp_count = torch.zeros(4, dtype=torch.int32, device=self.device)
                self._gexp_host = torch.zeros(1, dtype=torch.int32).pin_memory()
            self._export_games_into(self._gexp, self._gexp_count)
            self._gexp_host.copy_(self._gexp_count[0:1], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return ev

    def finish_export_result(self, ev):
        """(#games finished, Move records) of finish_export_async once `ev` has completed (waits for it); the
        records are copies (queued on the current stream), so the persistent buffers can be reused next ply.  With
        the game log on, the ply's finished-game records (export_games' dict) are left in `last_games`."""
        ev.synchronize()
        finished, ring, k = (int(x) for x in self._exp_host.tolist())
        if k != ring:
            raise _lib.SpmctsError(f"Move export took {k} of {ring} ring records (buffer capacity {self._exp_cap})")
        moves = {key: v[:k].clone() for key, v in self._exp.items()} if k else None
        if getattr(self, "games_log", False):
            g = int(self._gexp_host[0])
            self.last_games = {key: v[:g].clone() for key, v in self._gexp.items()}
        return finished, moves

    def export_moves(self, max_records):
        dev = self.device
        n = max(1, int(max_records))
        out = dict(
            state=torch.zeros((n, self.cells), dtype=torch.int8, device=dev),
            tree_probs=torch.zeros((n, self.A), dtype=torch.float32, device=dev),
            q=torch.zeros(n, dtype=torch.float64, device=dev),
            q_f64=torch.zeros(n, dtype=torch.uint8, device=dev),
            z=torch.zeros(n, dtype=torch.float32, device=dev),
            game=torch.zeros(n, dtype=torch.int64, device=dev),
        )
        call("spmcts_export_moves", self.h, ptr(out["state"]), ptr(out["tree_probs"]), ptr(out["q"]),
             ptr(out["q_f64"]), ptr(out["z"]), ptr(out["game"]), n, ptr(self._count), _stream())
        k = self._read_count()
        return {key: v[:k] for key, v in out.items()}

    def games_set_log(self, on=True):
        """The game log (include/spmcts.h spmcts_games_set_log): every ply's action is kept per slot and each
        finished game leaves a record in the finished-game ring (export_games).  Raises while a game is active."""
        torch.cuda.current_stream().synchronize()
        call("spmcts_games_set_log", self.h, int(bool(on)))
        self.games_log = bool(on)

    def export_games(self, n=None):
        """The finished-game ring as a dict of device tensors, one per field, and the ring cleared (include/spmcts.h
        spmcts_export_games): id int64 [k], slot int32 [k], result int8 [k] (tree 2g's view), swap uint8 [k], plies
        int32 [k], opening int32 [k] (-1 without a book), moves uint8 [k, W*H] (bytes past plies zero).  At most `n`
        records (None: the ring's capacity, 2 * n_games).  The call empties the whole ring: records past `n` are
        discarded, so an `n` below the capacity is for callers that know fewer are there."""
        out = self._game_buffers(max(1, 2 * self.n_games if n is None else int(n)))
        self._export_games_into(out, self._count)
        k = self._read_count()
        return {key: v[:k] for key, v in out.items()}

    def _game_buffers(self, n):
        dev = self.device
        return dict(
            id=torch.zeros(n, dtype=torch.int64, device=dev),
            slot=torch.zeros(n, dtype=torch.int32, device=dev),
            result=torch.zeros(n, dtype=torch.int8, device=dev),
            swap=torch.zeros(n, dtype=torch.uint8, device=dev),
            plies=torch.zeros(n, dtype=torch.int32, device=dev),
            opening=torch.zeros(n, dtype=torch.int32, device=dev),
            moves=torch.zeros((n, self.cells), dtype=torch.uint8, device=dev),
        )

    def _export_games_into(self, out, count):
        call("spmcts_export_games", self.h, ptr(out["id"]), ptr(out["slot"]), ptr(out["result"]), ptr(out["swap"]),
             ptr(out["plies"]), ptr(out["opening"]), ptr(out["moves"]), int(out["id"].shape[0]), ptr(count), _stream())

    def games_state(self):
        G = self.n_games
        active = (ctypes.c_uint8 * G)()
        ply = (ctypes.c_int32 * G)()
        swap = (ctypes.c_uint8 * G)()
        gid = (ctypes.c_int64 * G)()
        torch.cuda.current_stream().synchronize()
        call("spmcts_games_state", self.h, active, ply, swap, gid)
        return dict(state=np.array(list(active)), ply=np.array(list(ply)), swap=np.array(list(swap)),
                    game_id=np.array(list(gid)))

    def games_results(self):
        """Per-slot outcome (include/spmcts.h spmcts_games_results; sync): result in tree 2g's view, swap, ply,
        state.  A slot keeps them after its game finished until another game starts in it."""
        G = self.n_games
        res = np.zeros(G, dtype=np.int8)
        swap = np.zeros(G, dtype=np.uint8)
        ply = np.zeros(G, dtype=np.int32)
        state = np.zeros(G, dtype=np.uint8)
        torch.cuda.current_stream().synchronize()
        call("spmcts_games_results", self.h, *[x.ctypes.data_as(ctypes.c_void_p) for x in (res, swap, ply, state)])
        return dict(result=res, swap=swap, ply=ply, state=state)

    # ------------------------------------------------------------------ league (N networks in one arena)
    @property
    def row_bytes(self):
        """Bytes of one leaf row."""
        return self._leaves[0].numel() * self._leaves.element_size()

    def set_league(self, tree_net, n_nets=None):
        """Per-tree network of a league arena (include/spmcts.h spmcts_set_league): `tree_net[t]` in
        [0, n_nets), -1 for a tree that sends no leaves (a hard-coded player); None turns the league off.
        Allocates the routed leaf buffer; `league_seg[j]` = network j's first routed row."""
        torch.cuda.current_stream().synchronize()
        if tree_net is None:
            call("spmcts_set_league", self.h, None, 0)
            self.n_nets, self.league_seg = 0, None
            return
        a = np.ascontiguousarray(np.asarray(tree_net, dtype=np.int32))
        if a.shape != (self.n_trees,):
            raise ValueError(f"expected {self.n_trees} per-tree entries, got {a.shape}")
        n = int(a.max()) + 1 if n_nets is None else int(n_nets)
        call("spmcts_set_league", self.h, a.ctypes.data_as(ctypes.c_void_p), n)
        seg = (ctypes.c_int32 * (n + 1))()
        call("spmcts_league_segments", self.h, seg)
        self.n_nets, self.league_seg = n, list(seg)
        if getattr(self, "_routed", None) is None:
            self._routed = torch.zeros_like(self._leaves)
        self._net_count = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        self._probs = torch.zeros((self.max_rows, self.A), dtype=torch.float32, device=self.device)
        self._values = torch.zeros(self.max_rows, dtype=torch.float32, device=self.device)

    def league_route(self, count_dev=None):
        """The rows of the last select / leaf_rows / play_action / games_end_ply, partitioned by network into
        the routed buffer (no host sync).  `count_dev`: the device row count (default: this arena's)."""
        c = self._count if count_dev is None else count_dev
        self._route_count = c  # alive until the unroute
        call("spmcts_league_route", self.h, ptr(self._leaves), ptr(c), self.row_bytes, ptr(self._routed),
             ptr(self._net_count), _stream())

    def routed_from(self, net):
        """Network `net`'s routed segment as the network's input tensor (every row it can hold)."""
        lo, hi = self.league_seg[net], self.league_seg[net + 1]
        x = self._routed[lo:hi]
        if self.leaf_format != "board" and self.leaf_layout == "nhwc":
            x = x.permute(0, 3, 1, 2)
        return x

    def net_count_dev(self, net):
        """Device int32 holding network `net`'s routed row count of the last league_route."""
        return self._net_count[net:net + 1]

    def net_counts(self):
        """Routed row count per network of the last league_route (sync)."""
        return self._net_count.cpu().tolist()

    def league_unroute(self, outputs):
        """`outputs`: per network (probs f32 [rows, A], values f32 [rows]) indexed from the network's routed row
        0.  Returns (probs, values) in arena-row order, ready for expand()."""
        keep = [(p if p.dtype == torch.float32 and p.is_contiguous() else p.float().contiguous(),
                 v.reshape(-1) if v.dtype == torch.float32 and v.is_contiguous() else v.float().reshape(-1).contiguous())
                for p, v in outputs]
        ptrs = tuple((p.data_ptr(), v.data_ptr()) for p, v in keep)
        if getattr(self, "_out_ptrs", None) != ptrs:  # the pointer tables change only when a buffer moves
            self._out_ptrs = ptrs
            self._ptab = torch.tensor([a for a, _ in ptrs], dtype=torch.int64).to(self.device)
            self._vtab = torch.tensor([b for _, b in ptrs], dtype=torch.int64).to(self.device)
        self._out_keep = keep
        call("spmcts_league_unroute", self.h, ptr(self._ptab), ptr(self._vtab), ptr(self._probs), ptr(self._values),
             _stream())
        return self._probs, self._values

    # ------------------------------------------------------------------ diagnostics
    def counters(self):
        c = _lib.Counters()
        torch.cuda.current_stream().synchronize()
        call("spmcts_get_counters", self.h, ctypes.byref(c))
        return c.as_dict()

    def check(self):
        torch.cuda.current_stream().synchronize()
        rc = _lib.lib().spmcts_check(self.h)
        if rc != 0:
            c = self.counters()
            raise _lib.SpmctsError(f"arena device error: {_lib.describe_flags(c['error_flags'])}")


def solver_search_rules(option):
    """The solver_search= option of the players and engines as (refute, proved) for Arena.set_solver_rules: True both
    rules, "refute" / "proved" one of them, False / None neither."""
    if option is None or option is False:
        return False, False
    if option is True:
        return True, True
    if option in ("refute", "proved"):
        return option == "refute", option == "proved"
    raise ValueError(f'solver_search must be True, False, "refute" or "proved", got {option!r}')


def symmetry_mode(option):
    """The symmetry= option of the arena, players and engines as the library's mode: None / False -> 0 (off),
    "mirror" -> SPMCTS_SYM_MIRROR.  An integer passes through (the library refuses an unknown one)."""
    if option is None or option is False:
        return _lib.SYM_NONE
    if option == "mirror":
        return _lib.SYM_MIRROR
    if isinstance(option, (int, np.integer)) and not isinstance(option, bool):
        return int(option)
    raise ValueError(f'symmetry must be None or "mirror", got {option!r}')


def table_net_eval(game, leaves, leaf_format, leaf_layout, salt=0, salts=None):
    """Run the deterministic table network kernel over leaf rows (parity tests / smoke).

    `salts` (int64 tensor [n] on the device, optional) gives every row its own network."""
    gid, W, H, A = GAMES[game]
    n = leaves.shape[0]
    dev = leaves.device
    probs = torch.empty((max(n, 1), A), dtype=torch.float32, device=dev)
    values = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
    if n:
        src = leaves
        if leaf_format != "board" and leaf_layout == "nhwc":
            src = leaves.permute(0, 2, 3, 1)  # back to the NHWC storage order
        call("spmcts_table_net", gid, W, H, ptr(src), LEAF_FORMATS[leaf_format],
             _lib.NHWC if leaf_layout == "nhwc" else _lib.NCHW, n, int(salt) & (2**64 - 1),
             ptr(salts) if salts is not None else None, ptr(probs), ptr(values), _stream())
    return probs[:n], values[:n]
