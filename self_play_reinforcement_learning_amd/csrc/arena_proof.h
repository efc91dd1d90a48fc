// arena_proof.h — playing what the search has proved: k_proof_verdict (the moves a tree's own proof keeps, read by
// play_move_choice) and k_proof_stop (a solved tree starts no more sims).  Included by spmcts.hip after
// arena_tree.h: needs its bounds_walk, TbGrid, group_ballot, and View / set_err / in_book.
//
// Both kernels take one APAD-lane group per tree in 64-thread blocks and run k_tree_bounds' walk with the stack in
// LDS; neither touches the node store.  k_proof_verdict writes View::pf_keep / pf_lo / pf_hi of the trees it covers
// (or a caller's arrays) and the ply counts of View::pf_stats; k_proof_stop writes View::tstarted of the trees it
// stops, its two counts and View::pf_nstop.  The select and backup kernels do not read any of it.

// The keep set S of a root with bounds lo <= s <= hi and this lane's move [mlo, mhi] (TB_NONE: illegal), as a mask
// over the group's lanes.  A secured win (lo > 0) or a solved root (lo == hi): the moves proved to reach lo.
// Otherwise: the moves not proved worse than what another move already secures, mhi >= lo.  The move that secures
// lo is in S either way (its mlo == lo, and mhi >= mlo), so S is not empty; an illegal move is never in it.
template <int P>
__device__ __forceinline__ uint32_t proof_keep(int mlo, int mhi, int lo, int hi) {
  const bool legal = mlo != TB_NONE;
  return group_ballot<P>(legal && ((lo > 0 || lo == hi) ? mlo == lo : mhi >= lo));
}

enum { PF_MODE_LIST = 0, PF_MODE_GAMES = 1, PF_MODE_ACTIVE = 2 };

// The verdict of n trees.  PF_MODE_LIST (spmcts_tree_proof_moves_batch): tree trees[i], row i of the caller's
// arrays, whatever the tree's flag says; an id outside [0, T) raises SPMCTS_ERR_STATE and leaves its row
// untouched.  PF_MODE_GAMES (before k_games_end_ply; n = G): the mover tree of active game i; PF_MODE_ACTIVE (before
// k_search_end; n = the active list's length): tree active[i]; both write row `tree` of View::pf_*, count the ply
// in pf_stats, and give a tree whose flag is off, that belongs to no MCTS player or whose game is in its opening
// book PF_ALL and TB_NONE without a walk.  Any output may be null.
// SB: the root's bounds come from its stored block (bounds_root), not from a walk.
template <class G, bool SB = false>
__global__ __launch_bounds__(TB_THREADS) void k_proof_verdict(View v, const int32_t *trees, int n, int mode,
                                                              uint32_t *keep_out, int8_t *lo_out, int8_t *hi_out) {
  constexpr int P = G::APAD;
  __shared__ typename TbGrid<G>::Stack s_stk;
  const int t = blockIdx.x * TB_THREADS + threadIdx.x;
  const int i = t / P, lane = t % P, grp = threadIdx.x / P;
  if (i >= n) return;
  int tree, row = i;
  bool walk = true;
  if (mode == PF_MODE_LIST) {
    tree = trees[i];
    if (tree < 0 || tree >= v.T) {
      if (lane == 0) set_err(v, SPMCTS_ERR_STATE);
      return;
    }
  } else {
    if (mode == PF_MODE_GAMES) {
      if (v.gstate[i] != GS_ACTIVE) return;
      tree = 2 * i + ((v.gply[i] + v.gswap[i]) & 1);
      walk = !in_book(v, i);
    } else {
      tree = v.active[i];
      if (tree < 0 || tree >= v.T) return;
    }
    row = tree;
    walk = walk && v.pf_on[tree] && v.tkind[tree] == SPMCTS_PLAYER_MCTS;
  }
  int rmlo = TB_NONE, rmhi = TB_NONE, lo = TB_NONE, hi = TB_NONE, e0 = 0, nodes = 0;
  uint32_t keep = PF_ALL;
  if (walk) {
    if (!bounds_root<G, SB>(v, tree, lane, grp, s_stk, rmlo, rmhi, lo, hi, e0, nodes)) {
      if (lane == 0) set_err(v, SPMCTS_ERR_STATE);
      return;
    }
    keep = proof_keep<P>(rmlo, rmhi, lo, hi);
    const uint32_t legal = group_ballot<P>(rmlo != TB_NONE);
    if (keep == 0) {  // (a finished root, which nobody chooses a move at: no restriction)
      keep = PF_ALL;
    } else if (mode != PF_MODE_LIST && lane == 0) {
      atomicAdd(v.pf_stats + PF_PLIES, 1ull);
      if (lo == hi) atomicAdd(v.pf_stats + PF_SOLVED, 1ull);
      if (lo > 0) atomicAdd(v.pf_stats + PF_WON, 1ull);
      if (keep != legal) atomicAdd(v.pf_stats + PF_CUT, 1ull);
    }
  }
  if (lane == 0) {
    if (keep_out) keep_out[row] = keep;
    if (lo_out) lo_out[row] = (int8_t)lo;
    if (hi_out) hi_out[row] = (int8_t)hi;
  }
}

// A tree whose root is solved starts no more sims (spmcts_proof_stop; K > 1 arenas).  One group per tree of the
// arena; a tree is looked at if proof play is on for it, it belongs to an MCTS player, it is searching (tstarted
// below its limit) and it is not paused inside a fill (RES_FILL: stopping it there would leave a paused fill on a
// tree that is not searching, SPMCTS_ERR_STATE in the expand; the next call looks at it again).  If its walk gives
// lo == hi, tstarted takes the "no sims left" value: the state of a search whose sims have all been started, so
// the expand replies its pending slots on its !refill path, the select passes it over, and play_move_choice's
// completeness check holds.  draw_noise resets tstarted at the next search; budget[] stays (k_compact sizes by it).
template <class G, bool SB = false>
__global__ __launch_bounds__(TB_THREADS) void k_proof_stop(View v) {
  constexpr int P = G::APAD;
  __shared__ typename TbGrid<G>::Stack s_stk;
  const int t = blockIdx.x * TB_THREADS + threadIdx.x;
  const int tree = t / P, lane = t % P, grp = threadIdx.x / P;
  if (tree >= v.T) return;
  if (!v.pf_on[tree] || v.tkind[tree] != SPMCTS_PLAYER_MCTS) return;
  const int limit = min(v.budget[tree], v.iters), started = v.tstarted[tree];
  if (started >= limit || (v.tres[tree] & RES_FILL)) return;
  int rmlo, rmhi, lo, hi, e0, nodes;
  if (!bounds_root<G, SB>(v, tree, lane, grp, s_stk, rmlo, rmhi, lo, hi, e0, nodes)) {
    if (lane == 0) set_err(v, SPMCTS_ERR_STATE);
    return;
  }
  if (lo != hi || lane != 0) return;
  v.tstarted[tree] = 0x3fffffff;
  v.pf_nstop[tree] += 1;
  atomicAdd(v.pf_stats + PF_STOPPED, 1ull);
  atomicAdd(v.pf_stats + PF_SKIPPED, (unsigned long long)(limit - started));
}
