// arena_tree.h — reading the search trees below the root: k_tree_pv (principal variations) and k_tree_export
// (subtrees in breadth-first order).  Included by spmcts.hip after arena_games.h: needs View, the node accessors,
// set_err, nbase and board.h's step.
//
// Both kernels only read the arena (the one write is set_err for a tree id outside [0, T), whose outputs are
// left untouched) and take one APAD-lane group per listed tree as k_root_stats_batch does (lane j: child j of the
// node under inspection).  Reductions inside a group are cross-lane only -- arena_select.h's DPP argmax, and
// ballot plus popcount under the group's lane mask -- with no LDS and no atomics on the outputs, so the layout is a
// function of the tree; every loop is bounded by an argument or a board constant.  A child-block index read from
// the store is used only inside [0, cap): anything else counts as "no block".
// (No __shfl / __shfl_xor here: they are shared inline functions of the HIP headers, and a new caller in this
// translation unit changed the code hipcc generates for k_expand_vl and k_select_vl, which also call them.  With
// the DPP argmax and the ballots the other kernels' assembly is what it was: scripts/product_isa_equal.sh.)
//
// The virtual loss is a stored field of K > 1 arenas only (reset_tree, k_expand_vl); a sequential arena never
// writes the vl words, and MCNode.virtual_loss is 0 outside search_node there: both kernels report 0.

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
