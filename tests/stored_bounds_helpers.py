"""Drivers and checks for the stored-bounds tests (Arena.set_stored_bounds, csrc/arena_solver.h): arenas whose
trees are taken to given positions or play whole games with the bounds kept in the nodes or not, and the check of
the invariant -- every stored entry of every block reachable from the active root equals what the host recursion
TreeView.node_bounds computes on the device's own full export of the tree as it stands."""
import numpy as np

from self_play_reinforcement_learning_amd import TreeView
from self_play_reinforcement_learning_amd.arena import Arena, table_net_eval
from self_play_reinforcement_learning_amd.tree import proof_move_set

ALL = 0xffffffff


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_invariant(arena, ids, what):
    """The stored columns of the full export of the listed trees equal TreeView.node_bounds() at every node, the
    root's row is (-128, -128), the entries of the root's children are bounds_batch's move_lo / move_hi (the
    independent walk), and proof_moves_batch (read from the root's stored block) is the host twin on bounds_batch's
    outputs.  Returns (the views, bounds_batch's rows on the host)."""
    count = arena.export_subtrees(ids, 1, min_visits=0)["count"]
    ex = arena.export_subtrees(ids, int(count.max()), min_visits=0, bounds=True)
    assert ex["move_lo"].dtype == ex["move_hi"].dtype and ex["move_lo"].shape == ex["parent"].shape
    rs, bb, pm = host(arena.root_stats_batch(ids)), host(arena.bounds_batch(ids)), host(arena.proof_moves_batch(ids))
    views = []
    for i in range(len(ids)):
        view = TreeView.from_export(ex, i)
        assert view.has_bounds and not view.truncated
        want = view.node_bounds(arena.game, rs["board"][i], int(rs["root_player"][i]))
        got = [(nd.move_lo, nd.move_hi) for nd in view.nodes]
        assert got == want, (what, i, [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w][:4])
        assert got[0] == (-128, -128)
        if view.root.expanded:
            kids = view.root.children
            assert [c.move_lo for c in kids] == bb["move_lo"][i].tolist(), (what, i)
            assert [c.move_hi for c in kids] == bb["move_hi"][i].tolist(), (what, i)
        views.append(view)
    keep = np.asarray(pm["keep"]).astype(np.int64) & ALL
    twin = np.asarray(proof_move_set(bb["lo"], bb["hi"], bb["move_lo"], bb["move_hi"]))
    assert keep.tolist() == twin.tolist(), what
    assert pm["lo"].tolist() == bb["lo"].tolist() and pm["hi"].tolist() == bb["hi"].tolist(), what
    return views, bb


def deep_expansions(view):
    """Expanded nodes at depth >= 2: each one's creation changed its own entry (the bounds of a position with
    children differ from the stamp of an unexpanded move), so its walk went on to the entry of its parent."""
    return sum(1 for nd in view.nodes if nd.expanded and nd.depth >= 2)


class Trees:
    """A tree-mode arena of one tree per position (move lists from the empty board), table net `salt`, Philox, the
    bounds stored or not: the trees are taken to their positions by play_action (its expansions included).  search()
    runs the simulations and leaves the arena before search_end."""

    def __init__(self, game, seqs, sims, K, stored, seed=5, salt=3, blocks_per_tree=0, sim_cap=None, strong=False):
        self.game, self.seqs, self.sims, self.salt = game, seqs, sims, salt
        n = len(seqs)
        self.ids = list(range(n))
        self.arena = a = Arena(game, n_trees=n, iterations=sims, rng="philox", seed=seed, leaf_format="f32",
                               leaf_layout="nchw", search_threads=K, blocks_per_tree=blocks_per_tree, strong_play=strong)
        if sim_cap is not None:
            a.set_sim_cap(sim_cap)
        a.tree_reset(self.ids, [1] * n)
        if stored:
            a.set_stored_bounds()
        for i in range(max(len(s) for s in seqs)):
            on = [t for t in self.ids if i < len(seqs[t])]
            self.step(a.play_action(on, [seqs[t][i] for t in on]))

    def step(self, count):
        if count:
            a = self.arena
            p, v = table_net_eval(self.game, a.leaves(count), a.leaf_format, a.leaf_layout, salt=self.salt)
            a.expand(p, v)

    def search(self, between=None):
        a = self.arena
        a.search_begin(self.ids)
        for s in range(-(-self.sims // a.search_threads)):
            self.step(a.select())
            if between is not None:
                between(s)


def play_games(game, G, sims, K, seed, stored, proof=False, book=None, blocks_per_tree=0, sim_cap=None, on_ply=None,
               max_plies=None, salt=2):
    """G self-play games in one arena (table net, Philox, K sims in flight, no refill) to the end or for max_plies
    plies; on_ply(arena, ply) runs after every ply.  Returns (the arena, dict(moves: the merged Move records,
    counters, results, proof: proof_stats))."""
    a = Arena(game, n_trees=2 * G, n_games=G, iterations=sims, rng="philox", seed=seed, leaf_format="f32",
              leaf_layout="nchw", search_threads=K, blocks_per_tree=blocks_per_tree)
    if sim_cap is not None:
        a.set_sim_cap(sim_cap)
    if proof:
        a.set_proof_play(True)
    if book is not None:
        a.games_set_openings(book)
    a.games_set_limit(G)
    a.games_start(list(range(G)))
    if stored:
        a.set_stored_bounds()

    def step(count):
        if count:
            p, v = table_net_eval(game, a.leaves(count), a.leaf_format, a.leaf_layout, salt=salt)
            a.expand(p, v)

    records, ply = [], 0
    while (a.games_state()["state"] == 1).any() and (max_plies is None or ply < max_plies):
        a.games_begin_ply()
        for _ in range(-(-sims // K)):
            step(a.select())
        step(a.games_end_ply())
        _, ring = a.games_finish_ply(refill=False)
        if ring:
            records.append(host(a.export_moves(ring)))
        if on_ply is not None:
            on_ply(a, ply)
        ply += 1
        assert ply <= a.cells
    a.check()
    moves = {k: np.concatenate([r[k] for r in records]) for k in records[0]} if records else {}
    res = {k: np.asarray(v).tolist() for k, v in a.games_results().items()}
    return a, dict(moves=moves, counters=a.counters(), results=res, proof=a.proof_stats())


def same_bytes(m0, m1):
    assert sorted(m0) == sorted(m1)
    for k in m0:
        assert m0[k].tobytes() == m1[k].tobytes(), k
