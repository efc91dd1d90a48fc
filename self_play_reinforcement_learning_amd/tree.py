"""`TreeView`: a host-side view of one exported search tree.

The reference's MCNode is an anytree node, so its users walk `root.children[a].children[b]` and print
`RenderTree(root)`.  Here the node store lives on the device; `Arena.export_subtrees` lists the subtree under a
tree's active root in breadth-first order (include/spmcts.h spmcts_tree_export_batch), and a TreeView wires one
row of those arrays into nodes with `.parent` / `.children`:

    out = arena.export_subtrees([t], max_nodes=256)
    view = TreeView.from_export(out, 0)
    print(view.render(max_depth=2))
    view.principal_variation()              # [(action, n, q), ...]

`TreeView.from_arrays` takes plain numpy arrays (or lists), so the class needs no GPU.  Data only: a view never
reaches back into the arena, and `to_dict()` / `from_dict()` round-trip through JSON.
"""
import numpy as np

FLAG_EXPANDED, FLAG_VALID, FLAG_TERMINAL = 1, 2, 4
FIELDS = ("parent", "action", "depth", "node_n", "node_vl", "node_w", "node_p", "player", "flags")
BOUND_FIELDS = ("move_lo", "move_hi")  # export_subtrees(bounds=True): each node's stored entry
BOUND_ILLEGAL = -128  # move_lo / move_hi of an illegal move, and its code


def bounds_to_codes(values, empty):
    """Score bounds (Arena.bounds_batch's lo, hi, move_lo, move_hi: values of the exact score s) as the solvers'
    move codes at a root of `empty` empty cells: e + 1 - v for v > 0 (a win in that many plies), -(e + 1 + v) for
    v < 0 (a loss at that ply), 0 for 0, -128 kept.  values: an int, a list, a numpy array or a tensor, `empty`
    broadcast over its last axis ([n] against [n, A]); an int gives an int, anything else a numpy int8 array."""
    scalar = isinstance(values, (int, np.integer))
    v = np.asarray(values.cpu() if hasattr(values, "cpu") else values).astype(np.int64)
    e = np.asarray(empty.cpu() if hasattr(empty, "cpu") else empty).astype(np.int64)
    if v.ndim > e.ndim:
        e = e.reshape(e.shape + (1,) * (v.ndim - e.ndim))
    code = np.where(v == BOUND_ILLEGAL, BOUND_ILLEGAL, np.where(v > 0, e + 1 - v, np.where(v < 0, -(e + 1 + v), 0)))
    return int(code) if scalar else code.astype(np.int8)


def classify_bounds(lo, hi):
    """What lo <= s <= hi says about the side to move: "win" (lo > 0), "loss" (hi < 0), "draw" (lo == hi == 0),
    "not_lost" (lo == 0 < hi), "not_won" (lo < 0 == hi), else "open"."""
    lo, hi = int(lo), int(hi)
    if lo > 0:
        return "win"
    if hi < 0:
        return "loss"
    if lo == 0:
        return "draw" if hi == 0 else "not_lost"
    return "not_won" if hi == 0 else "open"


def describe_bounds(lo, hi, empty, best):
    """One line on what a tree has proved: "proved: win in 5 by 3" (a forced win in 5 plies, secured by action 3),
    "proved: loss in 4", "proved: draw by 2", "bounds: at least a draw", "bounds: at most a draw", "bounds: open".
    Where a win or a loss is proved but its length is not (lo < hi), the ply count is the bound's: "in at most"."""
    status = classify_bounds(lo, hi)
    exact = "" if int(lo) == int(hi) else "at most "
    if status == "win":
        return f"proved: win in {exact}{bounds_to_codes(int(lo), int(empty))} by {int(best)}"
    if status == "loss":
        return f"proved: loss in {exact}{-bounds_to_codes(int(hi), int(empty))}"
    if status == "draw":
        return f"proved: draw by {int(best)}"
    return {"not_lost": "bounds: at least a draw", "not_won": "bounds: at most a draw", "open": "bounds: open"}[status]


def proof_move_set(lo, hi, move_lo, move_hi):
    """The keep set of proof-guided play (include/spmcts.h spmcts_set_proof_play; the host twin of
    Arena.proof_moves_batch's keep) from a root's score bounds (Arena.bounds_batch): bit a of the mask is set iff
    move a is legal (move_lo[a] != -128) and move_lo[a] == lo where lo > 0 (a win is secured) or lo == hi (the root
    is solved), move_hi[a] >= lo otherwise (a move proved worse than what another already secures is dropped).
    Never empty for a root with a legal move.  lo, hi: ints or [n]; move_lo, move_hi: [A] or [n, A] (lists, numpy
    arrays or tensors); an int for one root, else a numpy int64 array [n]."""
    arr = lambda x: np.asarray(x.cpu() if hasattr(x, "cpu") else x).astype(np.int64)  # noqa: E731
    lo, hi, mlo, mhi = arr(lo), arr(hi), arr(move_lo), arr(move_hi)
    scalar = lo.ndim == 0
    lo, hi = lo.reshape(-1, 1), hi.reshape(-1, 1)
    mlo, mhi = mlo.reshape(lo.shape[0], -1), mhi.reshape(lo.shape[0], -1)
    keep = (mlo != BOUND_ILLEGAL) & np.where((lo > 0) | (lo == hi), mlo == lo, mhi >= lo)
    mask = (keep.astype(np.int64) << np.arange(keep.shape[1], dtype=np.int64)).sum(axis=1)
    return int(mask[0]) if scalar else mask


def solver_select(move_lo, move_hi, expanded=None):
    """The two rules of solver-aware search (include/spmcts.h spmcts_set_solver_rules; csrc/arena_solver.h
    sb_refuted / sb_proved) on the stored entries of one node's child block, move_lo / move_hi [A] or [n, A] with
    -128 for an illegal move: (refuted, proved, sign), numpy arrays of the input's shape.  refuted[a]: move a is
    legal and move_hi[a] < lo, lo the largest move_lo of the block -- it cannot reach what a sibling already
    secures; the move that secures lo is never refuted.  proved[a]: move a is legal and move_lo[a] == move_hi[a],
    its score is known; `expanded` (bools of the same shape, optional) restricts it to the children that have a
    block, as the search does (a move that ends the game is solved too, but it keeps the terminal path).  sign[a]:
    the sign of that score for the player to move, 0 where not proved."""
    arr = lambda x: np.asarray(x.cpu() if hasattr(x, "cpu") else x).astype(np.int64)  # noqa: E731
    mlo, mhi = arr(move_lo), arr(move_hi)
    legal = mlo != BOUND_ILLEGAL
    lo = np.where(legal, mlo, BOUND_ILLEGAL).max(axis=-1, keepdims=True)
    refuted = legal & (mhi < lo)
    proved = legal & (mlo == mhi)
    if expanded is not None:
        proved &= np.asarray(expanded, dtype=bool)
    return refuted, proved, np.where(proved, np.sign(mlo), 0)


def describe_proof_moves(keep):
    """The kept moves of a mask as text: "keeps 2 3" (proof_move_set's mask; Arena.proof_moves_batch's keep)."""
    return "keeps " + " ".join(str(a) for a in range(32) if (int(keep) >> a) & 1)


def _env_of(game):
    from .arena import GAMES
    from .envs import Connect4Env, TicTacToeEnv

    if game not in GAMES:
        raise ValueError(f"unknown game {game!r}")
    _, W, H, A = GAMES[game]
    return (TicTacToeEnv() if game == "tictactoe" else Connect4Env(W, H)), W, H, A


class TreeNode:
    """One exported node: MCNode's n, w, p, player, virtual loss (`vl`) and q, plus where it sits in the tree.
    move_lo / move_hi: the node's stored score bounds (the move into it, seen from its parent) where the export
    carried them (Arena.export_subtrees(bounds=True)), else None."""

    __slots__ = ("index", "parent", "children", "action", "depth", "n", "vl", "w", "p", "player", "expanded", "valid",
                 "terminal", "move_lo", "move_hi")

    def __init__(self, index, parent, action, depth, n, vl, w, p, player, flags, move_lo=None, move_hi=None):
        self.index, self.parent, self.children = index, parent, ()
        self.move_lo, self.move_hi = move_lo, move_hi
        self.action, self.depth, self.n, self.vl, self.w, self.p, self.player = action, depth, n, vl, w, p, player
        self.expanded = bool(flags & FLAG_EXPANDED)
        self.valid = bool(flags & FLAG_VALID)
        self.terminal = bool(flags & FLAG_TERMINAL)

    @property
    def q(self):
        """MCNode.q (mcts.py:59-62): (w - virtual_loss) / (n + virtual_loss), 0 where the denominator is 0."""
        d = self.n + self.vl
        return (self.w - self.vl) / d if d else 0

    @property
    def moves(self):
        """The actions from the root to this node."""
        out, node = [], self
        while node.parent is not None:
            out.append(node.action)
            node = node.parent
        return out[::-1]

    def __repr__(self):
        return f"TreeNode(moves={self.moves}, n={self.n}, q={self.q:+.3f}, p={self.p:.3f})"


class TreeView:
    """The exported nodes of one tree; `root`, `nodes` (breadth-first, as exported), `count` (the nodes that
    qualified on the device) and `truncated` (count > the entries the export had room for)."""

    def __init__(self, parent, action, depth, node_n, node_vl, node_w, node_p, player, flags, count=None,
                 max_nodes=None, move_lo=None, move_hi=None):
        parent = np.asarray(parent).reshape(-1)
        room = len(parent) if max_nodes is None else int(max_nodes)
        self.count = int(room if count is None else count)
        self.max_nodes = room
        m = min(self.count, room, len(parent))
        cols = [np.asarray(x).reshape(-1) for x in (action, depth, node_n, node_vl, node_w, node_p, player, flags)]
        if (move_lo is None) != (move_hi is None):
            raise ValueError("TreeView: move_lo and move_hi come together")
        self.has_bounds = move_lo is not None
        bcols = [np.asarray(x).reshape(-1) for x in (move_lo, move_hi)] if self.has_bounds else []
        if any(len(c) < m for c in cols + bcols):
            raise ValueError("TreeView: every array needs an entry per node")
        self.nodes = []
        kids = [[] for _ in range(m)]
        for i in range(m):
            pi = int(parent[i])
            if (i == 0) != (pi < 0) or pi >= i:
                raise ValueError(f"TreeView: entry {i} has parent {pi} (the root comes first, parents before children)")
            a, d, n, vl, w, p, pl, fl = (c[i] for c in cols)
            node = TreeNode(i, self.nodes[pi] if i else None, int(a), int(d), int(n), int(vl), float(w), float(p),
                            int(pl), int(fl), *[int(c[i]) for c in bcols])
            self.nodes.append(node)
            if i:
                kids[pi].append(node)
        for node, ks in zip(self.nodes, kids):
            node.children = tuple(sorted(ks, key=lambda c: c.action))
        self.root = self.nodes[0] if self.nodes else None

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_arrays(cls, count=None, max_nodes=None, **arrays):
        """From plain arrays (numpy or lists), one entry per node in export order: parent, action, depth, node_n,
        node_vl, node_w, node_p, player, flags; and, optionally, move_lo and move_hi (the stored bounds)."""
        return cls(*[arrays[k] for k in FIELDS], count=count, max_nodes=max_nodes,
                   **{k: arrays[k] for k in BOUND_FIELDS if k in arrays})

    @classmethod
    def from_export(cls, out, row=0):
        """From row `row` of Arena.export_subtrees' dict (device tensors; one host copy per field)."""
        host = {k: out[k][row].cpu().numpy() for k in FIELDS + BOUND_FIELDS if k in out}
        return cls.from_arrays(count=int(out["count"][row]), max_nodes=int(out["parent"].shape[1]), **host)

    @classmethod
    def from_dict(cls, d):
        nodes = d["nodes"]
        arrays = {k: [nd[k] for nd in nodes] for k in FIELDS + BOUND_FIELDS if k in FIELDS or (nodes and k in nodes[0])}
        return cls.from_arrays(count=d["count"], max_nodes=d["max_nodes"], **arrays)

    # ------------------------------------------------------------------ reading
    @property
    def truncated(self):
        return self.count > self.max_nodes

    def __len__(self):
        return len(self.nodes)

    def principal_variation(self, min_visits=1):
        """[(action, n, q), ...] from the root: the most visited exported child, the lowest action on ties
        (ns.index(max(ns)), mcts.py:290-295), while it has at least max(min_visits, 1) visits."""
        out, node, need = [], self.root, max(int(min_visits), 1)
        while node is not None and node.children:
            best = max(node.children, key=lambda c: (c.n, -c.action))
            if best.n < need:
                break
            out.append((best.action, best.n, best.q))
            node = best
        return out

    def score_bounds(self, game, board, player, per_node=None):
        """The host twin of Arena.bounds_batch (include/spmcts.h spmcts_tree_bounds_batch; no GPU): what this tree
        proves about the exact score s of its root position, lo <= s <= hi.  game: the arena's game name; board
        [W, H]: the root's board of +-1 stones; player: the side to move there.  The view must hold the whole tree:
        exported with min_visits=0 and not truncated (ValueError otherwise).  A legal move (the env's valid_moves)
        that ends the game is worth e, the root's empty cells, for a win and 0 for a full board; a move into an
        expanded node [-hi(child), -lo(child)]; any other [-(e - 1), e - 2]; lo / hi are the maxima over the legal
        moves.  Returns dict(lo, hi, move_lo [A], move_hi [A] (-128: illegal), best (the lowest action with
        move_lo == lo), empty, nodes (the expanded nodes entered)), plain ints and lists.  per_node: a list with an
        entry per node of the view, filled with (move_lo, move_hi) of the move into each node below the root as seen
        from its parent (node_bounds)."""
        env, W, H, A = _env_of(game)
        if self.truncated or self.root is None:
            raise ValueError("score_bounds needs the whole tree: this view is truncated")
        for nd in self.nodes:
            if nd.expanded and [c.action for c in nd.children] != list(range(A)):
                raise ValueError("score_bounds needs every child of every expanded node: export with min_visits=0")
        entered = [0]

        def walk(node, state, mover):
            """(lo, hi, move_lo, move_hi) of `node`, whose board is `state` with `mover` to move."""
            lo, hi, mlo, mhi = walk_node(node, state, mover)
            if per_node is not None and node.expanded:
                for c in node.children:
                    per_node[c.index] = (mlo[c.action], mhi[c.action])
            return lo, hi, mlo, mhi

        def walk_node(node, state, mover):
            e = int((state == 0).sum())
            entered[0] += node.expanded
            env.set_state(state)
            env.episode_over = False
            legal = env.valid_moves()
            mlo, mhi = [BOUND_ILLEGAL] * A, [BOUND_ILLEGAL] * A
            for a in range(A):
                if not legal[a]:
                    continue
                env.set_state(state.copy())
                env.episode_over = False
                s, r, done, _ = env.step(a, player=mover)
                if done:
                    mlo[a] = mhi[a] = e if r else 0
                elif node.expanded and node.children[a].expanded:
                    clo, chi, _, _ = walk(node.children[a], s.copy(), -mover)
                    mlo[a], mhi[a] = -chi, -clo
                else:
                    mlo[a], mhi[a] = -(e - 1), e - 2
            return max(mlo), max(mhi), mlo, mhi

        state = np.array(board, dtype=np.int64).reshape(W, H)
        lo, hi, mlo, mhi = walk(self.root, state, int(player))
        best = mlo.index(lo) if lo != BOUND_ILLEGAL else -1
        return dict(lo=lo, hi=hi, move_lo=mlo, move_hi=mhi, best=best, empty=int((state == 0).sum()), nodes=entered[0])

    def node_bounds(self, game, board, player):
        """score_bounds' recursion returned for every node: a list with one (move_lo, move_hi) per node of the view,
        the bounds of the move into that node seen from its parent, (-128, -128) for the root and for an illegal
        move.  What an arena with stored bounds keeps in the node itself (Arena.set_stored_bounds; the export's
        move_lo / move_hi columns, TreeNode.move_lo / .move_hi), recomputed from the tree's shape alone."""
        out = [(BOUND_ILLEGAL, BOUND_ILLEGAL)] * len(self.nodes)
        self.score_bounds(game, board, player, per_node=out)
        return out

    def render(self, max_depth=None, min_visits=1):
        """One line per node in the style of anytree's RenderTree: action, n, q, p, `#` on a node whose move
        ended the game.  Only nodes of depth <= max_depth with n >= min_visits are shown (the root always)."""
        lines = []

        def line(node):
            head = "root" if node.parent is None else f"a={node.action}"
            mark = " #" if node.terminal else ""
            return f"{head} n={node.n} q={node.q:+.3f} p={node.p:.3f}{mark}"

        def walk(node, prefix):
            shown = [c for c in node.children if c.n >= min_visits and (max_depth is None or c.depth <= max_depth)]
            for k, c in enumerate(shown):
                last = k == len(shown) - 1
                lines.append(prefix + ("└── " if last else "├── ") + line(c))
                walk(c, prefix + ("    " if last else "│   "))

        if self.root is not None:
            lines.append(line(self.root))
            walk(self.root, "")
        return "\n".join(lines)

    def to_dict(self):
        """Data only, JSON-serialisable: {"count", "max_nodes", "truncated", "nodes": [one dict per node, the
        export's fields]}; TreeView.from_dict reads it back."""
        nodes = [dict(parent=-1 if nd.parent is None else nd.parent.index, action=nd.action, depth=nd.depth,
                      node_n=nd.n, node_vl=nd.vl, node_w=nd.w, node_p=nd.p, player=nd.player,
                      flags=(FLAG_EXPANDED if nd.expanded else 0) | (FLAG_VALID if nd.valid else 0) |
                      (FLAG_TERMINAL if nd.terminal else 0)) for nd in self.nodes]
        if self.has_bounds:
            for d, nd in zip(nodes, self.nodes):
                d.update(move_lo=nd.move_lo, move_hi=nd.move_hi)
        return dict(count=self.count, max_nodes=self.max_nodes, truncated=self.truncated, nodes=nodes)
