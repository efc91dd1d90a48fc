// arena_solver.h — score bounds kept in the nodes: the stamp of a new child block and the walk that carries a
// change up the path of the expansion.  Included by spmcts.hip after arena_rows.h and before arena_expand.h: needs
// View, the node accessors (nd_lo / nd_hi), board.h's step and arena_select.h's DPP helpers.
//
// Entry j of every child block carries [mlo, mhi] of the move into child j, seen from the block's own node (the
// parent of the children): exactly what arena_tree.h's bounds_walk computes for that move on the tree as it stands
// (DESIGN.md §4 "Stored bounds").  A node's own lo / hi are not stored: they are the maxima over its block.
//   * a new block is stamped from the board alone (sb_classify): a winning move [e, e], a board-filling move
//     [0, 0], an illegal move and a pad lane SB_NONE, any other move the trivial [-(e - 1), e - 2] -- what
//     bounds_enter gives a move into a child without a block;
//   * bounds change only when a block is created, so the selects never write them; the expansion then replaces the
//     leaf's entry in its parent's block by [-hi, -lo] of the new block and goes on bottom-up along the stashed
//     path while an entry changes (sb_propagate).  The path's first node is the active root, whose own entry
//     nobody reads: the walk ends below it.
// Only the kernels of the stored-bounds set (the SB = true instantiations, launched once spmcts_set_solver_search
// switched maintenance on) call any of this; the SB = false kernels never touch the two arrays.

// (SB_NONE = -128, an illegal move or a pad lane, is declared with the rules' forward declarations in arena_select.h)

// the largest x of the group, in every lane (arena_tree.h's group_max is this function)
template <int P>
__device__ __forceinline__ int sb_group_max(int x) {
  static_assert(P == 8 || P == 16, "tree groups of 8 or 16 lanes");
  x = max(x, dpp_i<DPP_XOR1>(x));
  x = max(x, dpp_i<DPP_XOR2>(x));
  x = max(x, dpp_i<DPP_HALF_MIRROR>(x));
  if constexpr (P == 16) x = max(x, dpp_i<DPP_MIRROR>(x));
  return x;
}

// ---- the search rules (DESIGN.md §4 "Solver-aware search"; k_select and sim_vl behind the tree's rule bits) ----
// A lane's stored entry in one register: lo in bits 0..7, hi in bits 8..15 (TreeRoot keeps the root block's).
__device__ __forceinline__ int sb_pack(int mlo, int mhi) { return (mlo & 0xff) | ((mhi & 0xff) << 8); }
__device__ __forceinline__ int sb_lo(int packed) { return (int)(int8_t)(packed & 0xff); }
__device__ __forceinline__ int sb_hi(int packed) { return (int)(int8_t)((packed >> 8) & 0xff); }

// R1, refute: this lane's move cannot reach lo(X) = the most a sibling already secures.  Every lane of the group
// calls it (a group maximum); an illegal move and a pad lane hold SB_NONE and are "refuted" too, which their
// callers never see (they are invalid already).  The move that secures lo(X) has mhi >= mlo == lo(X): it stays.
template <int P>
__device__ __forceinline__ bool sb_refuted(int mlo, int mhi) {
  return mhi < sb_group_max<P>(mlo);
}

// R2, proved end: the chosen child has a block of its own and its score is known exactly.  (A terminal move has no
// block and keeps its own path; an open move without a block has mlo < mhi; a locked child has no block.)
__device__ __forceinline__ bool sb_proved(int cc, int mlo, int mhi) { return cc >= 0 && mlo == mhi; }

// The value an R2 end backs up, for the node's `player` and the child's exact score s seen from that player: the
// sign of s for the player, shaped for a strong_play tree as terminal_value shapes the winning move itself -- the
// score is the number of empty cells where that move is played, so np.sum(np.abs(state)) + 1 there is CELLS - |s| + 1.
template <class G>
__device__ __forceinline__ double sb_proved_value(bool strong, int s, int player) {
  const int r = (s > 0 ? 1 : (s < 0 ? -1 : 0)) * player;
  if (strong && s != 0) {
    const int num_steps = G::CELLS - (s > 0 ? s : -s) + 1;
    return (1.18 - ((double)(9 * num_steps) / 350.0)) * (double)r;
  }
  return (double)r;
}

// Lane j's move at a node (board b, `player` to move), from the board alone: legal iff step accepts it and places
// a stone (on the free-placement board step passes over an occupied cell in silence).  A legal move that ends the
// game is worth e (a win) or 0 (the board is full); any other legal move the trivial bounds of a position of e - 1
// empty cells seen from this side, which stand unless the child has a block.  The one classification of the stamp
// here and of arena_tree.h's bounds_enter.  Returns the move's kind.
enum { SB_ILLEGAL = 0, SB_ENDS = 1, SB_OPEN = 2 };
template <class G>
__device__ __forceinline__ int sb_classify(Board b, int player, int lane, int &mlo, int &mhi) {
  const uint64_t occ = b.pos | b.neg;
  const int e = G::CELLS - popc(occ);
  mlo = mhi = SB_NONE;
  int kind = SB_ILLEGAL;
  if (lane < G::A) {
    Board nbd = b;
    int rew = 0, done = 0;
    if (step<G>(nbd, lane, player, &rew, &done) == STEP_OK && (nbd.pos | nbd.neg) != occ) {
      if (done) {
        mlo = mhi = rew ? e : 0;
        kind = SB_ENDS;
      } else {
        mlo = -(e - 1);
        mhi = e - 2;
        kind = SB_OPEN;
      }
    }
  }
  return kind;
}

// Stamp block `blk` of the tree at node base nb (every lane of the group its own entry, pad lanes included) for
// the node with board b and `player` to move; lo / hi: the node's own bounds, in every lane.
template <class G>
__device__ __forceinline__ void sb_stamp(const View &v, size_t nb, int blk, Board b, int player, int lane, int &lo,
                                         int &hi) {
  constexpr int P = G::APAD;
  int mlo, mhi;
  sb_classify<G>(b, player, lane, mlo, mhi);
  const size_t ci = nb + (size_t)blk * P + lane;
  nd_lo<P>(v, ci) = (int8_t)mlo;
  nd_hi<P>(v, ci) = (int8_t)mhi;
  lo = sb_group_max<P>(mlo);
  hi = sb_group_max<P>(mhi);
}

// The new block of node `leaf` has bounds [lo, hi]; the leaf's parent is path node plen - 1 and path(k) is the
// node id of path node k (the same value in every lane).  Rewrites the leaf's entry, then, while an entry changed,
// recomputes the parent's bounds from its block and rewrites the parent's entry in the block above, up to the
// entries of the active root's children.  plen == 0 (the new block is the active root's own): nothing to write.
// Every lane of the group takes the same branches.  Returns whether any entry was written; the caller orders these
// stores before later reads of the same words (one wave owns the tree).  on_root(me, nlo, nhi) runs in every lane
// when the walk rewrites an entry of the active root's own child block (`me`: this lane holds that entry): a launch
// that keeps that block in registers (TreeRoot) updates its copy there.
template <class G, class PathF, class RootF>
__device__ __forceinline__ bool sb_propagate(const View &v, size_t nb, int leaf, int plen, int lo, int hi, int lane,
                                             PathF path, RootF on_root) {
  constexpr int P = G::APAD;
  bool wrote = false;
  int node = leaf;
  for (int k = plen - 1; k >= 0; --k) {  // `node`'s parent is path node k
    const int nlo = -hi, nhi = -lo;
    const size_t ci = nb + (size_t)(node & ~(P - 1)) + lane;  // this lane's entry of the block `node` sits in
    int mlo = nd_lo<P>(v, ci), mhi = nd_hi<P>(v, ci);
    const bool me = lane == (node & (P - 1));
    if (!group_or<P>((me && (mlo != nlo || mhi != nhi)) ? 1 : 0)) break;
    if (me) {
      nd_lo<P>(v, ci) = (int8_t)nlo;
      nd_hi<P>(v, ci) = (int8_t)nhi;
      mlo = nlo;
      mhi = nhi;
    }
    wrote = true;
    if (k == 0) {  // the parent is the active root
      on_root(me, nlo, nhi);
      break;
    }
    lo = sb_group_max<P>(mlo);
    hi = sb_group_max<P>(mhi);
    node = path(k);
  }
  return wrote;
}

// The root block of every fresh tree (reset_tree's state: two blocks, the empty board), for the trees that were
// reset before spmcts_set_solver_search switched the stored bounds on (it launches this once; afterwards
// reset_tree<G, true> stamps the block itself).  One group per tree.
template <class G>
__global__ __launch_bounds__(64) void k_sb_stamp_roots(View v) {
  constexpr int P = G::APAD;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int tree = t / P, lane = t % P;
  if (tree >= v.T) return;
  if (v.used[tree] != 2 || v.root[tree] != 0 || (v.rpos[tree] | v.rneg[tree]) != 0) return;
  int lo, hi;
  sb_stamp<G>(v, nbase<G>(v, tree), 1, Board{0, 0}, v.rplayer[tree], lane, lo, hi);
}
