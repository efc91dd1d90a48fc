// arena_tree.h — reading the search trees below the root: k_tree_pv (principal variations), k_tree_export
// (subtrees in breadth-first order) and k_tree_bounds (what a tree proves: bounds on the exact score).  Included by
// spmcts.hip after arena_games.h: needs View, the node accessors, set_err, nbase and board.h's step.
//
// The kernels only read the arena (the one write is set_err for a tree id outside [0, T), whose outputs are
// left untouched) and take one APAD-lane group per listed tree as k_root_stats_batch does (lane j: child j of the
// node under inspection).  Reductions inside a group are cross-lane only -- arena_select.h's DPP argmax, and
// ballot plus popcount under the group's lane mask -- with no atomics on the outputs, so the layout is a function
// of the tree (LDS holds k_tree_bounds' stack and nothing else); every loop is bounded by an argument, a board
// constant or cap.  A child-block index read from the store is used only inside [0, cap): anything else counts as
// "no block".
// (No __shfl / __shfl_xor here: they are shared inline functions of the HIP headers, and a new caller in this
// translation unit changed the code hipcc generates for k_expand_vl and k_select_vl, which also call them.  With
// the DPP argmax and the ballots the other kernels' assembly is what it was: scripts/product_isa_equal.sh.)
//
// The virtual loss is a stored field of K > 1 arenas only (reset_tree, k_expand_vl); a sequential arena never
// writes the vl words, and MCNode.virtual_loss is 0 outside search_node there: k_tree_pv and k_tree_export report 0.

// pointers of spmcts_tree_pv_batch's outputs ([n][max_len] unless noted; any may be null)
struct TreePvOut {
  int8_t *pv;
  int32_t *n, *vl;
  double *w;
  float *p;
  int32_t *len;       // [n]
  uint8_t *end;       // [n]
  int8_t *end_board;  // [n][CELLS]
};

// pointers of spmcts_tree_export_batch's outputs ([n][max_nodes] unless noted; any may be null)
struct TreeExportOut {
  int32_t *parent;
  int8_t *action;
  int16_t *depth;
  int32_t *n, *vl;
  double *w;
  float *p;
  int8_t *player;
  uint8_t *flags;
  int32_t *count;  // [n]
  // spmcts_tree_export_bounds_batch only (null otherwise): the node's stored entry, the bounds of the move into it
  // seen from its parent (arena_solver.h); -128 in the root's row
  int8_t *move_lo, *move_hi;
};

enum { PV_END_CUT = 0, PV_END_NO_CHILD = 1, PV_END_GAME = 2 };
enum { TREE_EXPANDED = 1, TREE_VALID = 2, TREE_TERMINAL = 4 };

// bit j: the predicate of the group's lane j
template <int P>
__device__ __forceinline__ uint32_t group_ballot(bool pred) {
  const int gbase = (threadIdx.x & 63) & ~(P - 1);
  return (uint32_t)(__ballot(pred) >> gbase) & ((1u << P) - 1u);
}

__device__ __forceinline__ bool tree_block_ok(const View &v, int cb) { return cb >= 0 && cb < v.cap; }

// The principal variation of each listed tree: from the active root, the child with the largest n, the lowest
// action on ties (ns.index(max(ns)), mcts.py:290-295), until that n is below max(min_visits, 1), the node has no
// child block, the move ended the game or max_len moves are out.
template <class G>
__global__ void k_tree_pv(View v, const int32_t *trees, int n, int max_len, int min_visits, TreePvOut o) {
  constexpr int P = G::APAD;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = t / P, lane = t % P;
  if (i >= n) return;
  const int tree = trees[i];
  if (tree < 0 || tree >= v.T) {
    if (lane == 0) set_err(v, SPMCTS_ERR_STATE);
    return;
  }
  const size_t nb = nbase<G>(v, tree);
  const int mv = min_visits > 1 ? min_visits : 1;
  Board b{v.rpos[tree], v.rneg[tree]};
  int player = v.rplayer[tree];
  int cb = nd_c<P>(v, nb + v.root[tree]);
  int len = 0, end = PV_END_CUT;
  while (len < max_len) {
    if (!tree_block_ok(v, cb)) {
      end = PV_END_NO_CHILD;
      break;
    }
    const size_t ci = nb + (size_t)cb * P + lane;
    const int cn = lane < G::A ? nd_n<P>(v, ci) : -1;
    // the largest n, the lowest action on ties: k_select's group argmax (an int32 is exact as a double)
    double best = (double)cn;
    int a = lane;
    group_argmax<P>(best, a);
    if (best < (double)mv) {
      end = PV_END_NO_CHILD;
      break;
    }
    int rew = 0, done = 0;
    if (step<G>(b, a, player, &rew, &done) != STEP_OK) {  // (a visited child is a legal move)
      end = PV_END_NO_CHILD;
      break;
    }
    if (lane == a) {
      const size_t at = (size_t)i * max_len + len;
      if (o.pv) o.pv[at] = (int8_t)a;
      if (o.n) o.n[at] = cn;
      if (o.vl) o.vl[at] = v.K > 1 ? nd_vl<P>(v, ci) : 0;
      if (o.w) o.w[at] = nd_w<P>(v, ci);
      if (o.p) o.p[at] = nd_p<P>(v, ci);
    }
    ++len;
    if (done) {
      end = PV_END_GAME;
      break;
    }
    cb = nd_c<P>(v, nb + (size_t)cb * P + a);  // (one address for the group)
    player = -player;
  }
  if (o.pv)
    for (int k = len + lane; k < max_len; k += P) o.pv[(size_t)i * max_len + k] = -1;
  if (lane == 0) {
    if (o.len) o.len[i] = len;
    if (o.end) o.end[i] = (uint8_t)end;
  }
  if (o.end_board)
    for (int c = lane; c < G::CELLS; c += P)
      o.end_board[(size_t)i * G::CELLS + c] = cell_value<G>(b, c / G::H, c % G::H);
}

// The export's work buffer, 8-byte words: per listed tree and queue slot the queued node's two board masks and
// its (child block, depth) word, then per listed tree the CELLS + 1 words of the counting walk's stack.
template <class G>
__host__ __device__ constexpr size_t tree_export_work_words(size_t n, size_t max_nodes) {
  return 3 * n * max_nodes + n * (size_t)(G::CELLS + 1);
}

// Queue words are written by the lane of the child and read by every lane of the same group, always inside one
// wave: wavefront-scope relaxed accesses between wavefront-scope fences (plain loads and stores in the code).
__device__ __forceinline__ void wave_store(uint64_t *p, uint64_t x) {
  __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ uint64_t wave_load(uint64_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
__device__ __forceinline__ uint64_t tree_pack(int cb, int depth) {
  return (uint64_t)(uint32_t)cb | ((uint64_t)(uint32_t)depth << 32);
}

// The subtree under each listed tree's active root in breadth-first order.  The output arrays are the queue: entry
// 0 is the root; for queue entry e in order, its children with n >= min_visits (every child for min_visits 0),
// at a depth within max_depth (< 0: no limit), are appended in ascending action order at the positions the
// group's ballot prefix gives.  count = the nodes that qualify; beyond max_nodes nothing is written, and the rest
// of the tree is only counted (a depth-first walk over the expanded qualifying nodes, its stack in `work`).
template <class G>
__global__ void k_tree_export(View v, const int32_t *trees, int n, int max_nodes, int min_visits, int max_depth,
                              TreeExportOut o, uint64_t *work) {
  constexpr int P = G::APAD;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = t / P, lane = t % P;
  if (i >= n) return;
  const int tree = trees[i];
  if (tree < 0 || tree >= v.T) {
    if (lane == 0) set_err(v, SPMCTS_ERR_STATE);
    return;
  }
  const int M = max_nodes;
  const size_t nb = nbase<G>(v, tree), bb = (size_t)tree * v.cap, row = (size_t)i * M;
  uint64_t *wpos = work + row, *wneg = work + (size_t)n * M + row, *wcd = work + 2 * (size_t)n * M + row;
  uint64_t *stk = work + 3 * (size_t)n * M + (size_t)i * (G::CELLS + 1);
  const int rplayer = v.rplayer[tree];
  const size_t root = nb + v.root[tree];
  const int rcb = nd_c<P>(v, root);
  const bool vl_on = v.K > 1;
  if (lane == 0) {
    if (o.parent) o.parent[row] = -1;
    if (o.action) o.action[row] = -1;
    if (o.depth) o.depth[row] = 0;
    if (o.n) o.n[row] = nd_n<P>(v, root);
    if (o.vl) o.vl[row] = vl_on ? nd_vl<P>(v, root) : 0;
    if (o.w) o.w[row] = nd_w<P>(v, root);
    if (o.p) o.p[row] = nd_p<P>(v, root);
    if (o.player) o.player[row] = (int8_t)rplayer;
    if (o.flags) o.flags[row] = (uint8_t)((tree_block_ok(v, rcb) ? TREE_EXPANDED : 0) | TREE_VALID);
    if (o.move_lo) o.move_lo[row] = -128;
    if (o.move_hi) o.move_hi[row] = -128;
    wave_store(wpos, v.rpos[tree]);
    wave_store(wneg, v.rneg[tree]);
    wave_store(wcd, tree_pack(rcb, 0));
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  int tail = 1;
  for (int e = 0; e < M && e < tail; ++e) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint64_t cd = wave_load(wcd + e);
    const int cb = (int32_t)(uint32_t)cd, depth = (int)(cd >> 32);
    if (!tree_block_ok(v, cb) || (max_depth >= 0 && depth >= max_depth)) continue;
    const Board b{wave_load(wpos + e), wave_load(wneg + e)};
    const int player = (depth & 1) ? -rplayer : rplayer;
    const uint32_t vm = nd_vm<P>(v, bb + cb);
    const size_t ci = nb + (size_t)cb * P + lane;
    int cn = 0, cc = -1;
    if (lane < G::A) {
      cn = nd_n<P>(v, ci);
      cc = nd_c<P>(v, ci);
    }
    const bool q = lane < G::A && cn >= min_visits;
    const uint32_t mask = group_ballot<P>(q);
    const int idx = tail + __popc(mask & ((1u << lane) - 1u));
    if (q && idx < M) {
      const bool valid = (vm >> lane) & 1u;
      Board nbd = b;
      int rew = 0, done = 0;
      const bool term = valid && step<G>(nbd, lane, player, &rew, &done) == STEP_OK && done;
      const size_t at = row + idx;
      if (o.parent) o.parent[at] = e;
      if (o.action) o.action[at] = (int8_t)lane;
      if (o.depth) o.depth[at] = (int16_t)(depth + 1);
      if (o.n) o.n[at] = cn;
      if (o.vl) o.vl[at] = vl_on ? nd_vl<P>(v, ci) : 0;
      if (o.w) o.w[at] = nd_w<P>(v, ci);
      if (o.p) o.p[at] = nd_p<P>(v, ci);
      if (o.player) o.player[at] = (int8_t)-player;
      if (o.flags)
        o.flags[at] = (uint8_t)((tree_block_ok(v, cc) ? TREE_EXPANDED : 0) | (valid ? TREE_VALID : 0) |
                                (term ? TREE_TERMINAL : 0));
      if (o.move_lo) o.move_lo[at] = nd_lo<P>(v, ci);
      if (o.move_hi) o.move_hi[at] = nd_hi<P>(v, ci);
      wave_store(wpos + idx, nbd.pos);
      wave_store(wneg + idx, nbd.neg);
      wave_store(wcd + idx, tree_pack(cc, depth + 1));
    }
    tail += __popc(mask);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  }
  int count = tail;
  if (tail > M) {
    // The queue is full: count the whole listing.  Every lane of the group keeps the same stack (the same word to
    // the same address, read back by the lane that wrote it): word = block | child mask << 32 | depth << 48.
    count = 1;
    int sp = 0, cur = rcb, d = 0;
    for (int it = 0; it <= v.cap; ++it) {  // one expanded node per round, at most cap of them
      if (tree_block_ok(v, cur) && !(max_depth >= 0 && d >= max_depth)) {
        const size_t ci = nb + (size_t)cur * P + lane;
        int cn = 0, cc = -1;
        if (lane < G::A) {
          cn = nd_n<P>(v, ci);
          cc = nd_c<P>(v, ci);
        }
        const bool q = lane < G::A && cn >= min_visits;
        count += __popc(group_ballot<P>(q));
        const uint32_t dm = group_ballot<P>(q && tree_block_ok(v, cc));
        if (dm && sp <= G::CELLS) stk[sp++] = (uint64_t)(uint32_t)cur | ((uint64_t)dm << 32) | ((uint64_t)d << 48);
      }
      if (sp == 0) break;
      const uint64_t top = stk[sp - 1];
      const int tcb = (int32_t)(uint32_t)top;
      uint32_t tm = (uint32_t)(top >> 32) & 0xffffu;
      const int td = (int)(top >> 48), a = __ffs((int)tm) - 1;
      tm &= tm - 1u;
      if (tm)
        stk[sp - 1] = (uint64_t)(uint32_t)tcb | ((uint64_t)tm << 32) | ((uint64_t)td << 48);
      else
        --sp;
      cur = nd_c<P>(v, nb + (size_t)tcb * P + a);
      d = td + 1;
    }
  }
  if (lane == 0 && o.count) o.count[i] = count;
}

// ---- score bounds ------------------------------------------------------------
// pointers of spmcts_tree_bounds_batch's outputs ([n] unless noted; any may be null)
struct TreeBoundsOut {
  int8_t *lo, *hi;
  int8_t *move_lo, *move_hi;  // [n][A]
  int8_t *best, *empty;
  int32_t *nodes;
};

enum { TB_THREADS = 64, TB_NONE = -128 };

// the largest x of the group, in every lane
template <int P>
__device__ __forceinline__ int group_max(int x) {
  return sb_group_max<P>(x);  // (arena_solver.h: the stamp of a new block takes the same maxima)
}

// A frame's third word: child block | children still to descend into << 32 | (lo + 128) << 48 | (hi + 128) << 56.
__device__ __forceinline__ uint64_t bounds_pack(int cb, uint32_t dm, int lo, int hi) {
  return (uint64_t)(uint32_t)cb | ((uint64_t)(dm & 0xffffu) << 32) | ((uint64_t)((uint32_t)(lo + 128) & 0xffu) << 48) |
         ((uint64_t)((uint32_t)(hi + 128) & 0xffu) << 56);
}

// The node (board b, mover `player`, child block cb, e empty cells) as the walk enters it: lane j classifies move
// j.  A move is legal iff step accepts it and places a stone (on the free-placement board step passes over an
// occupied cell in silence).  A legal move that ends the game is worth e (a win) or 0 (the board is full); one
// into a child with a child block is left to the walk (its bit in dm) while the stack has a level for it; any
// other is worth the trivial bounds of a position of e - 1 empty cells seen from this side.  mlo / mhi: lane j's
// move (TB_NONE: illegal, or left to the walk); lo / hi: their maxima over the group.
template <class G>
__device__ __forceinline__ void bounds_enter(const View &v, size_t nb, Board b, int player, int cb, int lane,
                                             bool room, int &mlo, int &mhi, int &lo, int &hi, uint32_t &dm) {
  constexpr int P = G::APAD;
  static_assert((int)SB_NONE == (int)TB_NONE, "one code for an illegal move");
  bool desc = false;
  if (sb_classify<G>(b, player, lane, mlo, mhi) == SB_OPEN) {  // (arena_solver.h: the stored bounds' stamp)
    const int cc = tree_block_ok(v, cb) ? nd_c<P>(v, nb + (size_t)cb * P + lane) : -1;
    if (tree_block_ok(v, cc) && room) {
      desc = true;
      mlo = mhi = TB_NONE;
    }
  }
  lo = group_max<P>(mlo);
  hi = group_max<P>(mhi);
  dm = group_ballot<P>(desc);
}

// What a tree proves about the exact score s of its root position (solve.h's s: e if a move wins, 0 if
// it fills the board, else -s(child), maximised over the legal moves): lo <= s <= hi, by a minimax over the stored
// tree with every unexpanded node open.  Depth-first and iterative: the node in hand lives in registers (the same
// values in every lane of the group), its ancestors in the block's LDS, one frame of three 8-byte words per level,
// level-major so that the groups of a wave sit in neighbouring banks.  Every lane of a group writes the same words
// to the same addresses and reads back what it wrote itself, so no lane waits for another.  A round leaves the node
// in hand for its parent or descends into its next expanded child: each expanded node is entered once and left
// once, at most 2 * cap rounds in a sound store.  A walk that is not over by then has met a store that is no tree:
// it returns false (the caller raises SPMCTS_ERR_STATE and leaves its row untouched).
// The one walk of k_tree_bounds and of arena_proof.h's kernels.  s_stk: the calling kernel's LDS stack, TB_LEVELS
// frames for each of its GPB = TB_THREADS / APAD groups; grp: the group's index in the block.  rmlo / rmhi: the
// root's move of this lane (TB_NONE: illegal); lo / hi: the root's bounds; e0: its empty cells; nodes: the expanded
// nodes entered.
template <class G>
struct TbGrid {
  static constexpr int GPB = TB_THREADS / G::APAD, LEVELS = G::CELLS + 1;
  typedef uint64_t Stack[LEVELS][3][GPB];
};

template <class G>
__device__ __forceinline__ bool bounds_walk(const View &v, int tree, int lane, int grp,
                                            typename TbGrid<G>::Stack &s_stk, int &rmlo, int &rmhi, int &lo, int &hi,
                                            int &e0, int &nodes) {
  constexpr int P = G::APAD, LEVELS = TbGrid<G>::LEVELS;
  const size_t nb = nbase<G>(v, tree);
  const int rplayer = v.rplayer[tree];
  Board b{v.rpos[tree], v.rneg[tree]};
  e0 = G::CELLS - popc(b.pos | b.neg);
  int cb = nd_c<P>(v, nb + v.root[tree]);
  int sp = 0, root_a = -1;
  nodes = tree_block_ok(v, cb) ? 1 : 0;
  uint32_t dm;
  bounds_enter<G>(v, nb, b, rplayer, cb, lane, true, rmlo, rmhi, lo, hi, dm);
  for (int it = 0; it <= 2 * v.cap; ++it) {
    if (dm == 0) {  // the node in hand is done: its bounds go to its parent, negated
      if (sp == 0) return true;
      const int clo = lo, chi = hi;
      --sp;
      const uint64_t w = s_stk[sp][2][grp];
      b = Board{s_stk[sp][0][grp], s_stk[sp][1][grp]};
      cb = (int32_t)(uint32_t)w;
      dm = (uint32_t)(w >> 32) & 0xffffu;
      lo = max((int)((w >> 48) & 0xffu) - 128, -chi);
      hi = max((int)((w >> 56) & 0xffu) - 128, -clo);
      if (sp == 0 && lane == root_a) {
        rmlo = -chi;
        rmhi = -clo;
      }
    } else {  // descend into the next expanded child
      const int a = __ffs((int)dm) - 1;
      dm &= dm - 1u;
      s_stk[sp][0][grp] = b.pos;
      s_stk[sp][1][grp] = b.neg;
      s_stk[sp][2][grp] = bounds_pack(cb, dm, lo, hi);
      if (sp == 0) root_a = a;
      play<G>(b, a, (sp & 1) ? -rplayer : rplayer);
      cb = nd_c<P>(v, nb + (size_t)cb * P + a);  // (inside [0, cap): bounds_enter set the bit)
      ++sp;
      ++nodes;
      int mlo, mhi;
      bounds_enter<G>(v, nb, b, (sp & 1) ? -rplayer : rplayer, cb, lane, sp + 1 < LEVELS, mlo, mhi, lo, hi, dm);
    }
  }
  return false;
}

// The root's bounds for arena_proof.h's kernels.  SB (the arena keeps stored bounds, arena_solver.h) and the root
// has a child block: one read of that block, whose entries are the walk's rmlo / rmhi by the stored bounds'
// invariant; nodes is 0.  Otherwise the walk (for a root without a block that is its board-only path).
template <class G, bool SB>
__device__ __forceinline__ bool bounds_root(const View &v, int tree, int lane, int grp,
                                            typename TbGrid<G>::Stack &s_stk, int &rmlo, int &rmhi, int &lo, int &hi,
                                            int &e0, int &nodes) {
  constexpr int P = G::APAD;
  if constexpr (SB) {
    static_assert((int)SB_NONE == (int)TB_NONE, "one code for an illegal move");
    const size_t nb = nbase<G>(v, tree);
    const int cb = nd_c<P>(v, nb + v.root[tree]);
    if (tree_block_ok(v, cb)) {
      const size_t ci = nb + (size_t)cb * P + lane;
      rmlo = nd_lo<P>(v, ci);
      rmhi = nd_hi<P>(v, ci);
      lo = group_max<P>(rmlo);
      hi = group_max<P>(rmhi);
      e0 = G::CELLS - popc(v.rpos[tree] | v.rneg[tree]);
      nodes = 0;
      return true;
    }
  }
  return bounds_walk<G>(v, tree, lane, grp, s_stk, rmlo, rmhi, lo, hi, e0, nodes);
}

// spmcts_tree_bounds_batch: the walk above for each listed tree, one APAD-lane group per tree.
template <class G>
__global__ __launch_bounds__(TB_THREADS) void k_tree_bounds(View v, const int32_t *trees, int n, TreeBoundsOut o) {
  constexpr int P = G::APAD;
  __shared__ typename TbGrid<G>::Stack s_stk;
  const int t = blockIdx.x * TB_THREADS + threadIdx.x;
  const int i = t / P, lane = t % P, grp = threadIdx.x / P;
  if (i >= n) return;
  const int tree = trees[i];
  if (tree < 0 || tree >= v.T) {
    if (lane == 0) set_err(v, SPMCTS_ERR_STATE);
    return;
  }
  int rmlo, rmhi, lo, hi, e0, nodes;
  const bool over = bounds_walk<G>(v, tree, lane, grp, s_stk, rmlo, rmhi, lo, hi, e0, nodes);
  if (!over) {
    if (lane == 0) set_err(v, SPMCTS_ERR_STATE);
    return;
  }
  if (lane < G::A) {
    if (o.move_lo) o.move_lo[(size_t)i * G::A + lane] = (int8_t)rmlo;
    if (o.move_hi) o.move_hi[(size_t)i * G::A + lane] = (int8_t)rmhi;
  }
  const uint32_t secure = group_ballot<P>(rmlo != TB_NONE && rmlo == lo);
  if (lane == 0) {
    if (o.lo) o.lo[i] = (int8_t)lo;
    if (o.hi) o.hi[i] = (int8_t)hi;
    if (o.best) o.best[i] = (int8_t)(__ffs((int)secure) - 1);
    if (o.empty) o.empty[i] = (int8_t)e0;
    if (o.nodes) o.nodes[i] = nodes;
  }
}
