// arena_select.h — tree search, first half: resets and noise, k_compact, the DPP reductions, k_select, the threaded sim (sim_vl) and slot fill, the sim cap.
// Included by spmcts.hip after arena_rng.h: needs View, the node accessors and TreeRng.
// ----------------------------------------------------------------------------
// small helpers
// ----------------------------------------------------------------------------
// (arena_solver.h, included later: the stored bounds' classification of a move from the board alone)
template <class G>
__device__ __forceinline__ int sb_classify(Board b, int player, int lane, int &mlo, int &mhi);
// (arena_solver.h: the two search rules that read the stored bounds, shared by k_select and sim_vl)
template <int P>
__device__ __forceinline__ bool sb_refuted(int mlo, int mhi);
__device__ __forceinline__ bool sb_proved(int cc, int mlo, int mhi);
template <class G>
__device__ __forceinline__ double sb_proved_value(bool strong, int s, int player);
__device__ __forceinline__ int sb_pack(int mlo, int mhi);
__device__ __forceinline__ int sb_lo(int packed);
__device__ __forceinline__ int sb_hi(int packed);
enum { SB_NONE = -128 };  // an illegal move or a pad lane: arena_tree.h's TB_NONE (bounds_root asserts they agree)
// rule bits of a tree (View::sv_rules, spmcts_set_solver_rules) and its two statistics (View::sv_stats)
enum { SBR_REFUTE = 1, SBR_PROVED = 2 };
enum { SV_PROVED = 0, SV_REFLEV = 1, SV_NSTAT = 2 };
__device__ __forceinline__ int sb_rules(const View &v, int tree) { return v.sv_rules ? (int)v.sv_rules[tree] : 0; }

// SB (arena_solver.h): the root block is stamped with the empty board's stored bounds.
template <class G, bool SB = false>
__device__ __forceinline__ void reset_tree(const View &v, int tree, int player, const float *prior) {
  constexpr int P = G::APAD;
  const size_t nb = nbase<G>(v, tree);
  const size_t bb = (size_t)tree * v.cap;
  // block 0 = pseudo block holding the root in slot 0; block 1 = root's children
  nd_n<P>(v, nb + 0) = 0;
  nd_w<P>(v, nb + 0) = 0.0;
  nd_p<P>(v, nb + 0) = 0.f;
  nd_c<P>(v, nb + 0) = 1;
  nd_f<P>(v, nb + 0) = 0;
  if (v.K > 1) {
    nd_vl<P>(v, nb + 0) = 0;
    for (int j = 0; j < P; ++j) nd_vl<P>(v, nb + P + j) = 0;
  }
  for (int j = 0; j < P; ++j) {
    nd_n<P>(v, nb + P + j) = 0;
    nd_w<P>(v, nb + P + j) = 0.0;
    nd_p<P>(v, nb + P + j) = j < G::A ? prior[j] : 0.f;
    nd_c<P>(v, nb + P + j) = -1;
    nd_f<P>(v, nb + P + j) = 0;
  }
  if constexpr (SB) {
    for (int j = 0; j < P; ++j) {  // (one thread resets the tree: every entry in turn, pad entries included)
      int mlo, mhi;
      sb_classify<G>(Board{0, 0}, player, j, mlo, mhi);
      nd_lo<P>(v, nb + P + j) = (int8_t)mlo;
      nd_hi<P>(v, nb + P + j) = (int8_t)mhi;
    }
  }
  nd_vm<P>(v, bb + 0) = 1u;
  nd_vm<P>(v, bb + 1) = legal_mask<G>(Board{0, 0});
  v.used[tree] = 2;
  v.root[tree] = 0;
  v.rpos[tree] = 0;
  v.rneg[tree] = 0;
  v.rplayer[tree] = (int8_t)player;
  v.noise_on[tree] = 0;
  v.tstarted[tree] = 0x3fffffff;  // no search in progress
  v.tres[tree] = 0;
  for (int j = 0; j < v.K; ++j) v.need[(size_t)tree * v.K + j] = NEED_EMPTY;
}

// No pending slot, evaluated or not, and no paused fill: the state a search begins in, a move is chosen in
// (with every search_node call started) and _set_node's expansion takes slot 0 in.
__device__ __forceinline__ bool tree_idle(const View &v, int tree) {
  int busy = v.tres[tree] & RES_FILL;
  for (int j = 0; j < v.K; ++j) busy |= v.need[(size_t)tree * v.K + j] != NEED_EMPTY;
  return !busy;
}

// terminal value of _expand_node (mcts.py:305-313) for the tree's own strong_play; r = reward * mover
__device__ __forceinline__ double terminal_value(bool strong, Board parent, int r) {
  if (strong) {
    const int num_steps = popc(parent.pos | parent.neg) + 1;  // np.sum(np.abs(state)) + 1
    return (1.18 - ((double)(9 * num_steps) / 350.0)) * (double)r;
  }
  return (double)r;
}

// Dirichlet root noise (add_noise, mcts.py:49-53): A components, invalid children included.
template <class G>
__device__ void draw_noise(const View &v, int tree) {
  double g[G::A];
  if (v.rng_mode == SPMCTS_RNG_TAPE) {
    TreeRng r;
    rng_load(v, tree, r);
    bool terr = false;
    for (int j = 0; j < G::A; ++j) g[j] = rng_lane(v, r, j, &terr);
    rng_advance(v, r, G::A);
    if (terr) set_err(v, SPMCTS_ERR_TAPE);
    rng_store(v, tree, r);
  } else {
    // rocRAND's own Gamma path on the whole state (Box-Muller cache included); stores keep its
    // invariant result == philox10(counter), so the state is rocRAND-consistent here
    Philox st = v.rng[tree];
    double acc = 0.0;
    for (int j = 0; j < G::A; ++j) {
      g[j] = gamma_draw(&st, v.talpha[tree]);
      acc += g[j];
    }
    const double inv = acc > 0.0 ? 1.0 / acc : 0.0;
    for (int j = 0; j < G::A; ++j) g[j] *= inv;
    v.rng[tree] = st;
  }
  for (int j = 0; j < G::A; ++j) v.noise[(size_t)tree * G::APAD + j] = g[j];
  v.noise_on[tree] = 1;
  v.tstarted[tree] = 0;  // a search begins: `iterations` search_node calls to start
  if (!tree_idle(v, tree)) set_err(v, SPMCTS_ERR_STATE);
  v.tres[tree] = 0;  // its slot cycle starts at slot 0 (empty: nothing to reply, so with its fill)
}

// ----------------------------------------------------------------------------
// kernels: resets / noise
// ----------------------------------------------------------------------------
template <class G, bool SB = false>
__global__ void k_tree_reset(View v, const int32_t *trees, const int8_t *players, const float *priors, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int t = trees[i];
  if (t < 0 || t >= v.T) {
    set_err(v, SPMCTS_ERR_STATE);
    return;
  }
  reset_tree<G, SB>(v, t, players[i], priors ? priors + (size_t)i * G::A : v.root_prior + 16 * v.tnet[t]);
}

template <class G>
__global__ void k_search_begin(View v, const int32_t *trees, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int t = trees[i];
  v.active[i] = t;
  if (t < 0) return;
  draw_noise<G>(v, t);
}

// ----------------------------------------------------------------------------
// kernel: subtree recycling (node-store compaction of one tree before a search)
// ----------------------------------------------------------------------------
// The reference keeps every node of a game alive (backup runs to the original root, mcts.py:94-98;
// its _prune, mcts.py:197-199, is never called), but nothing above the active root is ever read
// again.  When a tree's remaining blocks cannot hold one more search (iterations + K + 2 blocks:
// one per network expansion, the _set_node expansion, slack), the blocks still reachable from the
// active root are slid down to the front of the tree's region, in their old order, and every child
// index is remapped:
//   * block 0 slot 0 becomes the root (its record copied there: n, w, p, children, dtype flag, vl);
//   * the live blocks (BFS from the root's child block, level-synchronous over the workgroup) keep
//     their relative order, so new index <= old index and the move can run in place, chunk by chunk
//     (a chunk is read completely before any of it is written);
//   * the root's child block is the oldest live block (everything below it was allocated after it),
//     so it lands at block 1 and the relation "child block > parent block" is preserved.
// Results are unchanged bit for bit (tests run the parity fixtures with a tiny blocks_per_tree).
// Without an explicit blocks_per_tree the store is sized for the worst case and this never runs.
// SB (arena_solver.h): the blocks' stored bounds move with the rest of the record.
template <class G, bool SB = false>
__global__ __launch_bounds__(256) void k_compact(View v, int n_active) {
  constexpr int P = G::APAD;
  constexpr int NT = 256;
  __shared__ int s_head, s_tail, s_carry, s_scan[NT];
  const int slot = blockIdx.x;
  if (slot >= n_active) return;
  const int tree = v.active[slot];
  if (tree < 0 || !v.gc) return;
  const int need = min(v.budget[tree], v.iters) + v.K + 2;
  const int used = v.used[tree];
  if (v.cap - used >= need) return;
  const int tid = threadIdx.x;
  const size_t nb = nbase<G>(v, tree);
  const size_t bb = (size_t)tree * v.cap;
  int32_t *list = v.gc_list + bb;
  int32_t *map = v.gc_map + bb;
  const int root = v.root[tree];
  const int croot = nd_c<P>(v, nb + root);
  // 1. live blocks: BFS from the root's child block
  if (tid == 0) {
    s_head = 0;
    s_tail = 0;
    if (croot >= 0) {
      list[0] = croot;
      s_tail = 1;
    }
  }
  for (int b = tid; b < used; b += NT) map[b] = -1;
  __syncthreads();
  for (;;) {
    const int head = s_head, tail = s_tail;
    if (head == tail) break;
    __syncthreads();
    for (int k = head * P + tid; k < tail * P; k += NT) {
      const int blk = list[k / P], j = k % P;
      const int c = j < G::A ? nd_c<P>(v, nb + (size_t)blk * P + j) : -1;
      if (c >= 0) list[atomicAdd(&s_tail, 1)] = c;
    }
    __threadfence_block();
    __syncthreads();
    if (tid == 0) s_head = tail;
    __syncthreads();
  }
  const int L = s_tail;
  for (int k = tid; k < L; k += NT) map[list[k]] = 0;
  __threadfence_block();
  __syncthreads();
  // 2. new indices: 1 + rank among the live blocks in old order (block-wide scan in chunks)
  if (tid == 0) s_carry = 1;
  __syncthreads();
  for (int c0 = 0; c0 < used; c0 += NT) {
    const int b = c0 + tid;
    const int live = (b < used && map[b] == 0) ? 1 : 0;
    s_scan[tid] = live;
    __syncthreads();
    for (int off = 1; off < NT; off <<= 1) {
      const int add = tid >= off ? s_scan[tid - off] : 0;
      __syncthreads();
      s_scan[tid] += add;
      __syncthreads();
    }
    if (live) map[b] = s_carry + s_scan[tid] - 1;
    __syncthreads();
    if (tid == NT - 1) s_carry += s_scan[NT - 1];
    __syncthreads();
  }
  __threadfence_block();
  __syncthreads();
  // 3. the root record into block 0 slot 0 (block 0 is never a destination: live blocks map to >= 1)
  if (tid == 0) {
    const int32_t rn = nd_n<P>(v, nb + root);
    const double rw = nd_w<P>(v, nb + root);
    const float rp = nd_p<P>(v, nb + root);
    const uint8_t rf = nd_f<P>(v, nb + root);
    const int32_t rvl = v.K > 1 ? nd_vl<P>(v, nb + root) : 0;
    nd_n<P>(v, nb) = rn;
    nd_w<P>(v, nb) = rw;
    nd_p<P>(v, nb) = rp;
    nd_f<P>(v, nb) = rf;
    nd_c<P>(v, nb) = croot >= 0 ? map[croot] : croot;
    if (v.K > 1) nd_vl<P>(v, nb) = rvl;
    nd_vm<P>(v, bb) = 1u;
    v.root[tree] = 0;
  }
  __threadfence_block();
  __syncthreads();
  // 4. slide the live blocks down, chunk by chunk; child indices remapped
  for (int c0 = 1; c0 < used; c0 += NT / P) {
    const int b = c0 + tid / P, j = tid % P;
    const int dst = b < used ? map[b] : -1;
    int32_t n = 0, c = -1, vl = 0;
    double w = 0.0;
    float pr = 0.f;
    uint8_t f = 0;
    uint32_t vm = 0;
    int8_t blo = 0, bhi = 0;
    if (dst >= 0) {
      const size_t i = nb + (size_t)b * P + j;
      n = nd_n<P>(v, i);
      w = nd_w<P>(v, i);
      pr = nd_p<P>(v, i);
      c = nd_c<P>(v, i);
      f = nd_f<P>(v, i);
      if (v.K > 1) vl = nd_vl<P>(v, i);
      if constexpr (SB) {
        blo = nd_lo<P>(v, i);
        bhi = nd_hi<P>(v, i);
      }
      if (j == 0) vm = nd_vm<P>(v, bb + b);
      if (c >= 0) c = map[c];
    }
    __syncthreads();
    if (dst >= 0) {
      const size_t o = nb + (size_t)dst * P + j;
      nd_n<P>(v, o) = n;
      nd_w<P>(v, o) = w;
      nd_p<P>(v, o) = pr;
      nd_c<P>(v, o) = c;
      nd_f<P>(v, o) = f;
      if (v.K > 1) nd_vl<P>(v, o) = vl;
      if constexpr (SB) {
        nd_lo<P>(v, o) = blo;
        nd_hi<P>(v, o) = bhi;
      }
      if (j == 0) nd_vm<P>(v, bb + dst) = vm;
    }
    __threadfence_block();
    __syncthreads();
  }
  if (tid == 0) {
    v.used[tree] = 1 + L;
    v.cnt[(size_t)tree * C_NCNT + C_GC] += 1;
    if (v.cap - (1 + L) < need) set_err(v, SPMCTS_ERR_POOL);  // the live subtree alone fills the store
  }
}

// ----------------------------------------------------------------------------
// kernel: select (search_node, mcts.py:340-367)
// ----------------------------------------------------------------------------
// P-lane group reductions on DPP lane permutations (a few cycles each) instead of ds_bpermute (an LDS
// round trip each, ~100 cycles on the tree kernels' dependent chain): partners lane ^ 1 and lane ^ 2
// (quad_perm), then lane ^ 7 (row_half_mirror: the other quad of the 8-lane group) and lane ^ 15
// (row_mirror: the other half of a 16-lane group).  After the two quad steps every lane holds its quad's
// result, so the mirror steps combine whole quads / halves: every lane ends with the group's result.
// Only lanes of the same group are read (the permutations stay within 4, 8 or 16 lanes).
enum { DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140 };
template <int CTRL>
__device__ __forceinline__ int dpp_i(int x) {
  return __builtin_amdgcn_mov_dpp(x, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ double dpp_d(double x) {
  const int2 v = __builtin_bit_cast(int2, x);
  return __builtin_bit_cast(double, make_int2(dpp_i<CTRL>(v.x), dpp_i<CTRL>(v.y)));
}

// argmax with the lowest index on ties (associative and commutative, so the butterfly order does not
// change the result)
template <int P, int CTRL>
__device__ __forceinline__ void argmax_step(double &s, int &idx) {
  const double so = dpp_d<CTRL>(s);
  const int io = dpp_i<CTRL>(idx);
  if (so > s || (so == s && io < idx)) {
    s = so;
    idx = io;
  }
}
template <int P>
__device__ __forceinline__ void group_argmax(double &s, int &idx) {
  static_assert(P == 8 || P == 16, "tree groups of 8 or 16 lanes");
  argmax_step<P, DPP_XOR1>(s, idx);
  argmax_step<P, DPP_XOR2>(s, idx);
  argmax_step<P, DPP_HALF_MIRROR>(s, idx);
  if constexpr (P == 16) argmax_step<P, DPP_MIRROR>(s, idx);
}

// group_argmax that also hands every lane the winning lane's child fields (the payload moves with the
// index through the butterfly, so no ds_bpermute from lane `a` afterwards)
template <int CTRL>
__device__ __forceinline__ void argmax_carry_step(double &s, int &idx, int &c0, int &c1, int &c2, double &d0) {
  const double so = dpp_d<CTRL>(s), d0o = dpp_d<CTRL>(d0);
  const int io = dpp_i<CTRL>(idx), c0o = dpp_i<CTRL>(c0), c1o = dpp_i<CTRL>(c1), c2o = dpp_i<CTRL>(c2);
  if (so > s || (so == s && io < idx)) {
    s = so;
    idx = io;
    c0 = c0o;
    c1 = c1o;
    c2 = c2o;
    d0 = d0o;
  }
}
template <int P>
__device__ __forceinline__ void group_argmax_carry(double &s, int &idx, int &c0, int &c1, int &c2, double &d0) {
  static_assert(P == 8 || P == 16, "tree groups of 8 or 16 lanes");
  argmax_carry_step<DPP_XOR1>(s, idx, c0, c1, c2, d0);
  argmax_carry_step<DPP_XOR2>(s, idx, c0, c1, c2, d0);
  argmax_carry_step<DPP_HALF_MIRROR>(s, idx, c0, c1, c2, d0);
  if constexpr (P == 16) argmax_carry_step<DPP_MIRROR>(s, idx, c0, c1, c2, d0);
}

// the same with a fourth int payload (the SB = true selects carry the winner's stored bounds).  A copy on purpose,
// not a variadic payload under both: the SB = false kernels keep calling group_argmax_carry as it stood, so their
// code stays the parent's instruction for instruction; a change to the comparison must be made in both.  (One
// variadic step under both was tried again later, a fold over the payload: every search kernel changed throughout)
template <int CTRL>
__device__ __forceinline__ void argmax_carry4_step(double &s, int &idx, int &c0, int &c1, int &c2, int &c3, double &d0) {
  const double so = dpp_d<CTRL>(s), d0o = dpp_d<CTRL>(d0);
  const int io = dpp_i<CTRL>(idx), c0o = dpp_i<CTRL>(c0), c1o = dpp_i<CTRL>(c1), c2o = dpp_i<CTRL>(c2);
  const int c3o = dpp_i<CTRL>(c3);
  if (so > s || (so == s && io < idx)) {
    s = so;
    idx = io;
    c0 = c0o;
    c1 = c1o;
    c2 = c2o;
    c3 = c3o;
    d0 = d0o;
  }
}
template <int P>
__device__ __forceinline__ void group_argmax_carry4(double &s, int &idx, int &c0, int &c1, int &c2, int &c3, double &d0) {
  static_assert(P == 8 || P == 16, "tree groups of 8 or 16 lanes");
  argmax_carry4_step<DPP_XOR1>(s, idx, c0, c1, c2, c3, d0);
  argmax_carry4_step<DPP_XOR2>(s, idx, c0, c1, c2, c3, d0);
  argmax_carry4_step<DPP_HALF_MIRROR>(s, idx, c0, c1, c2, c3, d0);
  if constexpr (P == 16) argmax_carry4_step<DPP_MIRROR>(s, idx, c0, c1, c2, c3, d0);
}

template <int P>
__device__ __forceinline__ int group_or(int x) {
  static_assert(P == 8 || P == 16, "tree groups of 8 or 16 lanes");
  x |= dpp_i<DPP_XOR1>(x);
  x |= dpp_i<DPP_XOR2>(x);
  x |= dpp_i<DPP_HALF_MIRROR>(x);
  if constexpr (P == 16) x |= dpp_i<DPP_MIRROR>(x);
  return x;
}

// SB (arena_solver.h "Solver-aware search"): the level's stored bounds are loaded with its other child fields, and
// behind the tree's rule bits a refuted child scores like an invalid one (R1) and a sim whose chosen child is
// solved ends there like a terminal one (R2).
template <class G, bool SB = false>
__global__ __launch_bounds__(64) void k_select(View v, int n_active) {
  constexpr int P = G::APAD;
  constexpr int GPB = 64 / P;  // groups (trees) per block
  __shared__ int32_t s_node[GPB][G::MAXD];
  __shared__ int32_t s_n[GPB][G::MAXD];
  __shared__ double s_w[GPB][G::MAXD];

  const int lane = threadIdx.x & (P - 1);
  const int grp = threadIdx.x / P;
  const int slot = blockIdx.x * GPB + grp;
  if (slot >= n_active) return;
  const int tree = v.active[slot];
  if (tree < 0) return;
  if (v.sim >= v.budget[tree]) return;  // this tree's search is complete (per-player iterations)

  const size_t nb = nbase<G>(v, tree);
  const size_t bb = (size_t)tree * v.cap;
  int node = v.root[tree];
  Board b{v.rpos[tree], v.rneg[tree]};
  int player = v.rplayer[tree];
  const bool noise = v.noise_on[tree] != 0;
  const double nz = (noise && lane < G::A) ? v.noise[(size_t)tree * P + lane] : 0.0;
  TreeRng rng;
  rng_load(v, tree, rng);
  bool terr = false;
  int rules = 0, reflev = 0;  // SB: the tree's rule bits, the levels of this sim at which R1 removed a child
  if constexpr (SB) rules = sb_rules(v, tree);

  int node_n = nd_n<P>(v, nb + node);
  double node_w = nd_w<P>(v, nb + node);
  // the node's child block: read for the root; below it, the child entry read with the parent's
  // block already holds it (one dependent global load per level instead of two)
  int cb = nd_c<P>(v, nb + node);
  int depth = 0;
  for (;;) {
    if (lane == 0) {
      s_node[grp][depth] = node;
      s_n[grp][depth] = node_n;
      s_w[grp][depth] = node_w;
    }
    if (cb < 0) {  // an expanded node is required here
      if (lane == 0) set_err(v, SPMCTS_ERR_STATE);
      return;
    }
    const uint32_t vm = nd_vm<P>(v, bb + cb);
    const size_t ci = nb + (size_t)cb * P + lane;
    int cn = 0, cc = -1;
    double cw = 0.0;
    float cp = 0.f;
    if (lane < G::A) {
      cn = nd_n<P>(v, ci);
      cw = nd_w<P>(v, ci);
      cp = nd_p<P>(v, ci);
      cc = nd_c<P>(v, ci);
    }
    int mlo = SB_NONE, mhi = SB_NONE;
    if constexpr (SB) {
      if (rules && lane < G::A) {
        mlo = nd_lo<P>(v, ci);
        mhi = nd_hi<P>(v, ci);
      }
    }
    const int gbase = (threadIdx.x & 63) & ~(P - 1);
    // the jitter does not depend on the child block: drawn here, it overlaps the loads above
    bool terr_j = false;
    const double jit = rng_group<G>(v, rng, lane, gbase, &terr_j);
    bool valid = (lane < G::A) && ((vm >> lane) & 1u);
    if constexpr (SB) {
      if (rules & SBR_REFUTE) {  // R1: the move cannot reach what a sibling already secures
        const bool cut = sb_refuted<P>(mlo, mhi);  // (a group maximum: every lane calls it)
        const bool ref = valid && cut;
        reflev += group_or<P>(ref ? 1 : 0);
        valid = valid && !ref;
      }
    }
    double score = -10000000000.0;  // mcts.py:347
    if (valid) {
      // q (mcts.py:59-62): children carry no virtual loss in sequential mode
      const double q = cn ? cw / (double)cn : 0.0;
      // p_eff (mcts.py:64-69): noise only on the active root's children
      const double pe = (depth == 0 && noise) ? nz * v.x + (double)cp * (1.0 - v.x) : (double)cp;
      // u (mcts.py:71-78): parent.n + parent.virtual_loss, and the parent holds vl = 1 here
      const double u = ((v.cpuct * pe) * sqrt((double)(node_n + 1))) / (double)(1 + cn);
      // select_prob (mcts.py:80-84): -child.player * q + u = parent.player * q + u
      score = (player > 0 ? q : -q) + u;
    }
    if (!group_or<P>(valid ? 1 : 0)) {  // mcts.py:349-354
      if (lane == 0) set_err(v, SPMCTS_ERR_NOCHILD);
      return;
    }
    // argmax(select_probs + 1e-6 * rand(A)) (mcts.py:355): first index on ties
    terr = terr || terr_j;
    double s = -INFINITY;
    if (lane < G::A) s = score + 0.000001 * jit;
    rng_advance(v, rng, G::A);
    int a = lane;
    group_argmax<P>(s, a);
    const int cc_a = __shfl(cc, gbase + a, 64);
    const int cn_a = __shfl(cn, gbase + a, 64);
    const double cw_a = __shfl(cw, gbase + a, 64);
    const int child = cb * P + a;
    bool proved = false;  // R2: the chosen child is solved, the sim ends here with the proved value
    int s_a = 0;
    if constexpr (SB) {
      if (rules & SBR_PROVED) {
        s_a = __shfl(mlo, gbase + a, 64);
        proved = sb_proved(cc_a, s_a, __shfl(mhi, gbase + a, 64));
      }
    }
    if (cc_a < 0 || proved) {
      // leaf reached: _expand_node (mcts.py:301-321)
      Board nb2 = b;
      int rew = 0, done = 0;
      int st = STEP_OK;
      if (!proved)
        st = step<G>(nb2, a, player, &rew, &done);
      else
        done = 1;
      if (lane == 0) {
        if (st != STEP_OK) set_err(v, SPMCTS_ERR_STATE);
        int64_t *cnt = v.cnt + (size_t)tree * C_NCNT;
        cnt[C_SIMS] += 1;
        cnt[C_DEPTH] += depth + 1;
        if constexpr (SB) {
          if (proved) v.sv_stats[(size_t)tree * SV_NSTAT + SV_PROVED] += 1;
          if (reflev) v.sv_stats[(size_t)tree * SV_NSTAT + SV_REFLEV] += reflev;
        }
        if (done) {
          // terminal: value r (or strong_play shaping), no children, backup in place
          const bool strong = v.tstrong[tree] != 0;
          const double val = proved ? sb_proved_value<G>(strong, s_a, player) : terminal_value(strong, b, rew * player);
          for (int k = 0; k <= depth; ++k) {
            const size_t idx = nb + s_node[grp][k];
            nd_n<P>(v, idx) = s_n[grp][k] + 1;
            nd_w<P>(v, idx) = s_w[grp][k] + val;
            if (strong) nd_f<P>(v, idx) = 1;
          }
          nd_n<P>(v, nb + child) = cn_a + 1;
          nd_w<P>(v, nb + child) = cw_a + val;
          if (strong) nd_f<P>(v, nb + child) = 1;
          if (!proved) cnt[C_TERM] += 1;
        } else {
          // pending network evaluation: stash the path for k_expand
          const size_t pb = (size_t)tree * G::MAXD;
          for (int k = 0; k <= depth; ++k) {
            v.pnode[pb + k] = s_node[grp][k];
            v.pn[pb + k] = s_n[grp][k];
            v.pw[pb + k] = s_w[grp][k];
          }
          v.plen[tree] = depth + 1;
          v.leaf[tree] = child;
          v.leaf_n[tree] = cn_a;
          v.leaf_w[tree] = cw_a;
          v.lpos[tree] = nb2.pos;
          v.lneg[tree] = nb2.neg;
          v.lmover[tree] = (int8_t)player;
          v.need[tree] = NEED_ROW;
        }
        if (terr) set_err(v, SPMCTS_ERR_TAPE);
        rng_store(v, tree, rng);
      }
      return;
    }
    // descend
    play<G>(b, a, player);
    node = child;
    node_n = cn_a;
    node_w = cw_a;
    cb = cc_a;
    player = -player;
    ++depth;
    if (depth >= G::MAXD) {
      if (lane == 0) set_err(v, SPMCTS_ERR_STATE);
      return;
    }
  }
}

// ----------------------------------------------------------------------------
// threaded search: K simulations in flight per tree with virtual loss (the reference's
// thread_count search_node calls under an InferenceProxy, mcts.py:154, :328-331, :340-367).
//
// The reference's K threads each run select -> wait for the network -> backup, then take the next
// search_node task, so at any time ~K sims are in flight and a thread's next select sees the other
// K-1 sims still pending (a ROLLING window).  The arena fixes the order of that rolling schedule:
// pending slots j = 0..K-1 of a tree are completed in slot order, and each freed slot is refilled
// right after its backup (FIFO: the oldest pending sim returns first), so every select after the
// first K sees K-1 pending sims, as with the reference's threads.  One network batch still holds
// the K pending leaves of every tree.  Sims that end without a network call (a terminal leaf: backed
// up at once; a leak: every child invalid or locked, mcts.py:349-354, vl left in place) do not
// occupy a slot: the slot takes the next sim at once, as the reference's thread takes its next task.
// oracle/mcts.py (OracleTree.search, threads=K) restates exactly this schedule; the G6 fixture
// (threaded_stats.json) pins its statistics to the reference's own threaded search.
// ----------------------------------------------------------------------------
enum { SIM_DONE = 0, SIM_PENDING = 1, SIM_LEAK = 2, SIM_PAUSED = 3, SIM_ERROR = -1 };

// ----------------------------------------------------------------------------
// sim cap.  A tree's search is one fixed sequence of operations -- reply slot 0, fill slot 0, reply slot 1,
// fill slot 1, ... cyclically over its kt slots (OracleTree.search) -- and the only outside constraint is that
// a slot's reply comes after the network evaluated its leaf.  Which launch runs which operation is free.  A
// fill keeps starting sims until one waits for the network, and terminal leaves and leaks do not wait: a tree
// on a forced win or loss runs dozens of sims in one launch while every other tree's group is done, and the
// launch lasts as long as its slowest tree.  So a tree that has started View::simcap sims in a launch pauses
// before the next one (never inside a sim) and the next launch goes on at exactly that point: the same
// operations in the same order with the same RNG draws, so results are bit-identical for every cap.  At a
// pause the launch's usual end-of-launch stores describe the tree completely (tstarted, the RNG state, the
// paths' virtual losses, used, TreeRoot's write-through); on top of them View::tres holds the slot the cycle
// goes on at, and the slots whose evaluated outputs the launch had not yet replied keep them in the stash
// (NEED_STASH), since their rows are rewritten by the next step.
//
// Invariant (why a search needs no more launches than without a cap): cap >= 2 K.  A launch walks the cycle
// from the resume point until it meets a slot filled in this same launch (not yet evaluated), i.e. it either
// completes a full cycle of kt fills or pauses having started cap >= 2 K >= 2 kt sims.  Every fill starts at
// least one sim while sims are left, so by induction started >= min(limit, kt * (launch + 1)) after each
// launch, as in the uncapped schedule: a paused tree is ahead of that schedule, never behind it, and the
// launch after a pause completes a full cycle again (every slot pending at its start was evaluated before it).
// spmcts_set_sim_cap refuses 0 < cap < 2 K; k_games_end_ply and k_search_end raise SPMCTS_ERR_STATE if a
// tree's search is not complete when its move is chosen.
// ----------------------------------------------------------------------------
constexpr int SIM_CAP_PER_K = 2;  // default cap = SIM_CAP_PER_K * K (spmcts_arena_create)

// The searching tree's root, loaded once per kernel and kept in registers across the K fills /
// backups / refills (it is on every path): node id, its child block (fixed during a search: the
// root is expanded), board, player, and its visit count and virtual loss — and its child block
// (lane j < A: child j's n, w, p, child index, vl; the valid mask), the first level every sim
// scores.  Every store a sim or backup makes to these nodes is made to the registers as well (the
// same arithmetic), so depth 0 reads no memory.
struct TreeRoot {
  bool strong;  // the tree's strong_play (read once: a global load in a sim would wait on its stores)
  int node, cb, player, n, vl;
  double w;  // the root's w (terminal backups write it from here, no read-modify-write)
  Board b;
  int cn, cc, cvl;
  double cw;
  float cp;
  uint32_t vm;
};
// The root of the SB = true kernels: also the tree's rule bits and, while any is set, the stored bounds of the
// root's child block (lane j < A: sb_pack of entry j).  An sb_propagate that rewrites an entry of that block
// updates the copy too (expand_vl_body interleaves replies and fills in one launch).
struct TreeRootSB : TreeRoot {
  int rules, cbnd;
};
template <bool SB>
using TreeRootT = std::conditional_t<SB, TreeRootSB, TreeRoot>;

template <class G, bool SB = false>
__device__ __forceinline__ TreeRootT<SB> load_root(const View &v, int tree) {
  constexpr int P = G::APAD;
  const size_t nb = nbase<G>(v, tree);
  TreeRootT<SB> R;
  R.strong = v.tstrong[tree] != 0;
  R.node = v.root[tree];
  R.b = Board{v.rpos[tree], v.rneg[tree]};
  R.player = v.rplayer[tree];
  R.n = nd_n<P>(v, nb + R.node);
  R.vl = nd_vl<P>(v, nb + R.node);
  R.w = nd_w<P>(v, nb + R.node);
  R.cb = nd_c<P>(v, nb + R.node);
  const int lane = threadIdx.x & (P - 1);
  R.cn = 0;
  R.cc = -1;
  R.cvl = 0;
  R.cw = 0.0;
  R.cp = 0.f;
  R.vm = 0u;
  if constexpr (SB) {
    R.rules = sb_rules(v, tree);
    R.cbnd = sb_pack(SB_NONE, SB_NONE);
  }
  if (R.cb >= 0) {
    R.vm = nd_vm<P>(v, (size_t)tree * v.cap + R.cb);
    if (lane < G::A) {
      const size_t ci = nb + (size_t)R.cb * P + lane;
      R.cn = nd_n<P>(v, ci);
      R.cw = nd_w<P>(v, ci);
      R.cp = nd_p<P>(v, ci);
      R.cc = nd_c<P>(v, ci);
      R.cvl = nd_vl<P>(v, ci);
      if constexpr (SB) {
        if (R.rules) R.cbnd = sb_pack(nd_lo<P>(v, ci), nd_hi<P>(v, ci));
      }
    }
  }
  return R;
}

// The path of the sim in flight, in LDS (one group per tree): node ids and, per level, the node's n, vl
// (this sim's virtual loss included) and w as this sim read them, and where the node's record sits (cs:
// kRootRegs for the root and the root's children, kept in registers; kUncached = global memory only).  One wave
// owns the tree, so
// nothing changes them between the read and this sim's backup: a terminal backup writes n + 1, w + value,
// vl - 1 from here instead of reading the nodes again (one memory round trip less per terminal sim).
struct PathLds {
  int32_t *node, *n, *vl, *cs;
  double *w;
};
enum { kUncached = -1, kRootRegs = -2 };

// The stores a launch has issued to node records that live in global memory only (kUncached: every node but
// the root and its children, which TreeRoot keeps in registers for the launch).  One wave owns a tree for the
// whole launch, so a sim whose stores all went to the root and its children needs no fence before the next
// sim: nothing it wrote is read back from global memory in this launch.  A store to any other node sets
// `dirty`, and the next global read of node records waits on a workgroup fence first -- a fence only after
// issued stores, instead of one per sim.  (Per-launch LDS copies of the child blocks, written through, were
// measured slower and removed: DESIGN.md §4.)
struct StoreFence {
  bool dirty = false;  // stores to kUncached nodes since the last fence (group-uniform)
  __device__ __forceinline__ void fence_if_dirty() {
    if (dirty) {
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      dirty = false;
    }
  }
};

// The tree's counters of one kernel launch (the same value in every lane of the group), added to the
// arena's counters once at the end of the launch instead of a read-modify-write per sim.
struct SimCnt {
  int64_t sims = 0, depth = 0, term = 0, leak = 0, nn = 0, hwm = 0, pause = 0;
  __device__ void flush(int64_t *cnt) const {
    if (pause) cnt[C_PAUSE] += pause;
    cnt[C_SIMS] += sims;
    cnt[C_DEPTH] += depth;
    cnt[C_TERM] += term;
    cnt[C_LEAK] += leak;
    cnt[C_NN] += nn;
    cnt[C_HWM] = max(cnt[C_HWM], hwm);
  }
};

// The counters of the SB = true kernels: also the two statistics of the search rules (View::sv_stats) -- sims ended
// by R2, select levels at which R1 removed a child.  Only a tree with a rule bit set counts any, and its arena has
// the array (spmcts_set_solver_rules).
struct SimCntSB : SimCnt {
  int64_t proved = 0, reflev = 0;
  __device__ void flush_solver(int64_t *st) const {
    if (proved) st[SV_PROVED] += proved;
    if (reflev) st[SV_REFLEV] += reflev;
  }
};
template <bool SB>
using SimCntT = std::conditional_t<SB, SimCntSB, SimCnt>;

// One search_node with virtual loss (mcts.py:340-367) for pending slot j of `tree`, run by the
// tree's P-lane group.  vl += 1 on every node passed (mcts.py:345), children scored with
// q = (w - vl)/(n + vl) and u = c p sqrt(N + vl_parent)/(1 + n + vl) (mcts.py:59-78), pending leaves
// locked (child-block index -2, score -1e10, mcts.py:86-88).  Returns SIM_PENDING with the leaf
// locked and its path stashed in slot j, SIM_DONE for a terminal leaf (backed up, path vl removed),
// SIM_LEAK for a leak, SIM_ERROR on a corrupt tree; R (the root in registers) is updated to match and sf
// records the stores issued.  The return value is uniform across the group.
// SB (arena_solver.h "Solver-aware search"): the level's stored bounds come with its other child fields (the root's
// block from R), and R1 / R2 apply behind the tree's rule bits; an R2 end is the terminal branch with the proved value.
template <class G, bool SB = false>
__device__ int sim_vl(const View &v, int tree, int j, TreeRootT<SB> &R, TreeRng &rng, bool &terr, const PathLds &pl,
                      bool noise, double nz, SimCntT<SB> &sc, StoreFence &sf) {
  constexpr int P = G::APAD;
  const int lane = threadIdx.x & (P - 1);
  const int gbase = (threadIdx.x & 63) & ~(P - 1);
  const size_t nb = nbase<G>(v, tree);
  const size_t bb = (size_t)tree * v.cap;
  const int ps = tree * v.K + j;
  int node = R.node;
  Board b = R.b;
  int player = R.player;
  int node_n = R.n;
  int node_vl = R.vl + 1;  // this sim's virtual loss on the node (mcts.py:345)
  double node_w = R.w;
  int cb = R.cb;
  int ncs = kRootRegs;  // where path node `depth`'s record sits
  R.vl += 1;
  int depth = 0;
  int a0 = 0;  // the root child this sim took (path node 1)
  for (;;) {
    if (lane == 0) {
      pl.node[depth] = node;
      pl.n[depth] = node_n;
      pl.vl[depth] = node_vl;
      pl.w[depth] = node_w;
      pl.cs[depth] = ncs;
    }
    // the global store of the path's virtual loss waits for the sim's end (one store per path node, all
    // at once): gfx950's vmcnt counts stores too, so a store here would hold up the next level's loads.
    // `dirty` is set where those stores are issued (leak, pending, terminal below), not here: nothing of
    // this sim is in flight yet, so the levels of one sim read without a fence.
    if (depth == 1 && lane == a0) R.cvl = node_vl;  // the root child's vl, in registers too
    if (cb < 0) {
      if (lane == 0) set_err(v, SPMCTS_ERR_STATE);
      return SIM_ERROR;
    }
    uint32_t vm;
    int cn = 0, cc = -1, cvl = 0;
    double cw = 0.0;
    float cp = 0.f;
    int lcs = kRootRegs;  // where this level's child block (cb) sits
    int bnd = 0;          // SB with a rule on: sb_pack of this lane's stored entry
    if (depth == 0) {  // the root's child block, from registers
      vm = R.vm;
      cn = R.cn;
      cw = R.cw;
      cp = R.cp;
      cc = R.cc;
      cvl = R.cvl;
      if constexpr (SB) bnd = R.cbnd;
    } else {
      lcs = kUncached;
      sf.fence_if_dirty();
      vm = nd_vm<P>(v, bb + cb);
      const size_t ci = nb + (size_t)cb * P + lane;
      if (lane < G::A) {
        cn = nd_n<P>(v, ci);
        cw = nd_w<P>(v, ci);
        cp = nd_p<P>(v, ci);
        cc = nd_c<P>(v, ci);
        cvl = nd_vl<P>(v, ci);
      }
      if constexpr (SB) {
        bnd = sb_pack(SB_NONE, SB_NONE);
        if (R.rules && lane < G::A) bnd = sb_pack(nd_lo<P>(v, ci), nd_hi<P>(v, ci));
      }
    }
    // the jitter does not depend on the child block: drawn here, it overlaps the loads above
    bool terr_j = false;
    const double jit = rng_group<G>(v, rng, lane, gbase, &terr_j);
    // valid (mcts.py:86-88): valid move and not locked by a pending sim
    bool ref = false;  // R1: the move cannot reach what a sibling already secures
    if constexpr (SB) {
      if (R.rules & SBR_REFUTE) {
        const bool cut = sb_refuted<P>(sb_lo(bnd), sb_hi(bnd));  // (a group maximum: every lane calls it)
        ref = cut && (lane < G::A) && ((vm >> lane) & 1u) && cc != -2;
        sc.reflev += group_or<P>(ref ? 1 : 0);
      }
    }
    const bool valid = (lane < G::A) && ((vm >> lane) & 1u) && cc != -2 && !ref;
    double score = -10000000000.0;
    if (valid) {
      // q (mcts.py:59-62): (w - vl) / (n + vl)
      const int ne = cn + cvl;
      const double q = ne ? (cw - (double)cvl) / (double)ne : 0.0;
      const double pe = (depth == 0 && noise) ? nz * v.x + (double)cp * (1.0 - v.x) : (double)cp;
      // u (mcts.py:71-78): sqrt(parent.n + parent.virtual_loss) / (1 + n + virtual_loss)
      const double u = ((v.cpuct * pe) * sqrt((double)(node_n + node_vl))) / (double)(1 + cn + cvl);
      score = (player > 0 ? q : -q) + u;
    }
    if (!group_or<P>(valid ? 1 : 0)) {  // mcts.py:349-354: return, virtual loss left in place
      int unc = 0;
      for (int k = lane; k <= depth; k += P) {
        nd_vl<P>(v, nb + pl.node[k]) = pl.vl[k];
        unc |= pl.cs[k] == kUncached;
      }
      if (group_or<P>(unc)) sf.dirty = true;
      sc.leak += 1;
      return SIM_LEAK;
    }
    terr = terr || terr_j;  // (a leak consumes no draw, so its tape check does not count)
    double s = -INFINITY;
    if (lane < G::A) s = score + 0.000001 * jit;
    rng_advance(v, rng, G::A);
    int a = lane;
    int cc_a = cc, cn_a = cn, cvl_a = cvl;
    double cw_a = cw;
    bool proved = false;  // R2: the chosen child is solved, the sim ends here with the proved value
    int bnd_a = bnd;
    if constexpr (SB) {
      group_argmax_carry4<P>(s, a, cc_a, cn_a, cvl_a, bnd_a, cw_a);  // ... and its stored entry
      proved = (R.rules & SBR_PROVED) && sb_proved(cc_a, sb_lo(bnd_a), sb_hi(bnd_a));
    } else {
      group_argmax_carry<P>(s, a, cc_a, cn_a, cvl_a, cw_a);  // lane a's child fields in every lane
    }
    const int child = cb * P + a;
    if (cc_a < 0 || proved) {
      // leaf: _expand_node (mcts.py:301-321)
      Board nb2 = b;
      int rew = 0, done = 0;
      int st = STEP_OK;
      if (!proved)
        st = step<G>(nb2, a, player, &rew, &done);
      else
        done = 1;
      if (done) {
        // terminal: backup (mcts.py:94-98) then remove the path's virtual loss (:365); one lane per
        // path node, the values this sim read (pl: written by lane 0 of this wave, LDS stays in order)
        const double val =
            proved ? sb_proved_value<G>(R.strong, sb_lo(bnd_a), player) : terminal_value(R.strong, b, rew * player);
        const bool strong = R.strong;
        int unc = 0;
        for (int k = lane; k <= depth; k += P) {
          const int nk = pl.node[k], ck = pl.cs[k];
          const size_t idx = nb + nk;
          const int32_t n1 = pl.n[k] + 1, vl1 = pl.vl[k] - 1;
          const double w1 = pl.w[k] + val;
          nd_n<P>(v, idx) = n1;
          nd_w<P>(v, idx) = w1;
          if (strong) nd_f<P>(v, idx) = 1;
          nd_vl<P>(v, idx) = vl1;
          unc |= ck == kUncached;
        }
        if (lane == 0) {
          nd_n<P>(v, nb + child) = cn_a + 1;
          nd_w<P>(v, nb + child) = cw_a + val;
          if (strong) nd_f<P>(v, nb + child) = 1;
        }
        if (group_or<P>(unc) || lcs == kUncached) sf.dirty = true;
        R.n += 1;  // the root is path node 0
        R.vl -= 1;
        R.w += val;
        if (depth >= 1 && lane == a0) {  // path node 1, the root child a0
          R.cn += 1;
          R.cw += val;
          R.cvl -= 1;
        }
        if (depth == 0 && lane == a) {  // the terminal leaf is a root child
          R.cn += 1;
          R.cw += val;
        }
        if constexpr (SB) sc.proved += proved ? 1 : 0;
        if (!proved) sc.term += 1;
      } else {
        const size_t pb = (size_t)ps * G::MAXD;
        int unc = 0;
        for (int k = lane; k <= depth; k += P) {
          const int nk = pl.node[k];
          v.pnode[pb + k] = nk;
          nd_vl<P>(v, nb + nk) = pl.vl[k];
          unc |= pl.cs[k] == kUncached;
        }
        if (group_or<P>(unc)) sf.dirty = true;
      }
      sc.sims += 1;
      sc.depth += depth + 1;
      if (lane == 0) {
        if (st != STEP_OK) set_err(v, SPMCTS_ERR_STATE);
        if (!done) {
          // lock the leaf (mcts.py:359); the path was stashed above for the backup
          nd_c<P>(v, nb + child) = -2;
          v.plen[ps] = depth + 1;
          v.leaf[ps] = child;
          v.lpos[ps] = nb2.pos;
          v.lneg[ps] = nb2.neg;
          v.lmover[ps] = (int8_t)player;
          v.need[ps] = NEED_ROW;
        }
      }
      if (!done && lcs == kUncached) sf.dirty = true;
      if (!done && depth == 0 && lane == a) R.cc = -2;
      return done ? SIM_DONE : SIM_PENDING;
    }
    if (depth == 0) a0 = a;
    play<G>(b, a, player);
    node = child;
    node_n = cn_a;
    node_vl = cvl_a + 1;
    node_w = cw_a;
    cb = cc_a;
    ncs = lcs;  // the child's record is in this level's block
    player = -player;
    ++depth;
    if (depth >= G::MAXD) {
      if (lane == 0) set_err(v, SPMCTS_ERR_STATE);
      return SIM_ERROR;
    }
  }
}

// Refill pending slot j: start sims until one waits for the network, the tree's budget of
// search_node calls is spent (`started` counts them, mcts.py:328-331 submits `iterations`), or the launch has
// started View::simcap sims of this tree (`nst` counts them; SIM_PAUSED, before a sim and never in one).  No fence
// between sims: a sim reads the root and its children from the registers, and StoreFence's `dirty` rule fences
// before any global read of node records after a store to one.
template <class G, bool SB = false>
__device__ int fill_slot_vl(const View &v, int tree, int j, int limit, int &started, int &nst, TreeRootT<SB> &R,
                            TreeRng &rng, bool &terr, const PathLds &pl, bool noise, double nz, SimCntT<SB> &sc,
                            StoreFence &sf) {
  while (started < limit) {
    if (v.simcap && nst >= v.simcap) return SIM_PAUSED;
    ++started;
    ++nst;
    const int r = sim_vl<G, SB>(v, tree, j, R, rng, terr, pl, noise, nz, sc, sf);
    if (r == SIM_PENDING || r == SIM_ERROR) return r;
  }
  return SIM_DONE;
}
