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


class TreeNode:
    """One exported node: MCNode's n, w, p, player, virtual loss (`vl`) and q, plus where it sits in the tree."""

    __slots__ = ("index", "parent", "children", "action", "depth", "n", "vl", "w", "p", "player", "expanded", "valid",
                 "terminal")

    def __init__(self, index, parent, action, depth, n, vl, w, p, player, flags):
        self.index, self.parent, self.children = index, parent, ()
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
                 max_nodes=None):
        parent = np.asarray(parent).reshape(-1)
        room = len(parent) if max_nodes is None else int(max_nodes)
        self.count = int(room if count is None else count)
        self.max_nodes = room
        m = min(self.count, room, len(parent))
        cols = [np.asarray(x).reshape(-1) for x in (action, depth, node_n, node_vl, node_w, node_p, player, flags)]
        if any(len(c) < m for c in cols):
            raise ValueError("TreeView: every array needs an entry per node")
        self.nodes = []
        kids = [[] for _ in range(m)]
        for i in range(m):
            pi = int(parent[i])
            if (i == 0) != (pi < 0) or pi >= i:
                raise ValueError(f"TreeView: entry {i} has parent {pi} (the root comes first, parents before children)")
            a, d, n, vl, w, p, pl, fl = (c[i] for c in cols)
            node = TreeNode(i, self.nodes[pi] if i else None, int(a), int(d), int(n), int(vl), float(w), float(p),
                            int(pl), int(fl))
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
        node_vl, node_w, node_p, player, flags."""
        return cls(*[arrays[k] for k in FIELDS], count=count, max_nodes=max_nodes)

    @classmethod
    def from_export(cls, out, row=0):
        """From row `row` of Arena.export_subtrees' dict (device tensors; one host copy per field)."""
        host = {k: out[k][row].cpu().numpy() for k in FIELDS}
        return cls.from_arrays(count=int(out["count"][row]), max_nodes=int(out["parent"].shape[1]), **host)

    @classmethod
    def from_dict(cls, d):
        nodes = d["nodes"]
        arrays = {k: [nd[k] for nd in nodes] for k in FIELDS}
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
        return dict(count=self.count, max_nodes=self.max_nodes, truncated=self.truncated, nodes=nodes)
