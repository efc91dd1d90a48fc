// arena_games.h — the SelfPlayer game state machine (opening book plies included), k_root_stats_batch and the export kernels.
// Included by spmcts.hip after arena_expand.h: needs reset_tree, set_node and the search helpers.
// ----------------------------------------------------------------------------
// games: SelfPlayer.play_episode state machine (selfplayworker.py:164-224)
// ----------------------------------------------------------------------------
template <class G, bool SB = false>
__device__ void start_game(const View &v, int g, int64_t id, const float *priors) {
  const bool swap = (id & 1) != 0;  // swap_sides = not i % 2 == 0 (self_play_parallel.py:237)
  v.gpos[g] = 0;
  v.gneg[g] = 0;
  v.gply[g] = 0;
  v.gswap[g] = swap ? 1 : 0;
  v.gstate[g] = GS_ACTIVE;
  v.gresult[g] = 0;
  v.gid[g] = id;
  v.mv_count[2 * g] = 0;
  v.mv_count[2 * g + 1] = 0;
  // policy.reset(-1 if swap else 1), opposing.reset(1 if swap else -1)  (:175-176)
  reset_tree<G, SB>(v, 2 * g, swap ? -1 : 1, priors ? priors : v.root_prior + 16 * v.tnet[2 * g]);
  reset_tree<G, SB>(v, 2 * g + 1, swap ? 1 : -1, priors ? priors + G::A : v.root_prior + 16 * v.tnet[2 * g + 1]);
  if (v.book_n) {  // ids 2k and 2k + 1 play the same opening, once per colour
    const int64_t i = v.book_period ? id % v.book_period : id;
    const int o = (int)((i >> 1) % v.book_n);
    v.gopen[g] = o;
    v.gbook[g] = v.book_lens[o];
  }
}

template <class G, bool SB = false>
__global__ void k_games_start(View v, const int32_t *slots, const float *priors, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int g = slots[i];
  if (g < 0 || g >= v.G) {
    set_err(v, SPMCTS_ERR_STATE);
    return;
  }
  start_game<G, SB>(v, g, v.gcnt[7] + i, priors ? priors + (size_t)i * 2 * G::A : nullptr);
}

__global__ void k_games_bump_id(View v, int n) { v.gcnt[7] += n; }

template <class G>
__global__ void k_games_begin_ply(View v) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= v.G) return;
  if (v.gstate[g] != GS_ACTIVE) {
    v.active[g] = -1;
    return;
  }
  if (in_book(v, g)) {  // a book ply: nobody searches
    v.active[g] = -1;
    return;
  }
  // policy moves on even plies unless swap_sides (:178-183)
  const int mover = (v.gply[g] + v.gswap[g]) & 1;
  const int tree = 2 * g + mover;
  if (v.tkind[tree] != SPMCTS_PLAYER_MCTS) {  // hard-coded players do not search
    v.active[g] = -1;
    return;
  }
  v.active[g] = tree;
  draw_noise<G>(v, tree);
}

// Hard-coded opponents (games/general/hardcoded_players.py).  `own` = the player's stones,
// `enemy` = the other side's, in the player's own env frame (its stones are +1: play_move passes
// player * -1 to the opposing policy, selfplayworker.py:221-224); `look` = the player sign given to
// reset(player) (selfplayworker.py:175-176), which OneStepLookahead uses as "self.player".
// OneStepLookahead (:18-33): first any move after which step(a, look) ends the game, then any move
// after which step(a, -look) does, else uniform over the legal moves.  Random (:45-49): uniform.
// The uniform draw uses the tree's Philox stream (the reference's `random` module stream is not
// reproduced).  Negamax (no reference form; negamax.h): uniform over the moves with the best code, the
// int(u * n)-th of them in ascending action order, one draw like the uniform fallback's.
template <class G>
__device__ int hardcoded_move(const View &v, int tree, int kind, Board envb, int look) {
  const uint32_t legal = legal_mask<G>(envb);
  if (kind == SPMCTS_PLAYER_LOOKAHEAD) {
    for (int pass = 0; pass < 2; ++pass) {
      const int who = pass == 0 ? look : -look;
      for (int a = 0; a < G::A; ++a) {
        if (!((legal >> a) & 1u)) continue;
        Board b = envb;
        int rew = 0, done = 0;
        step<G>(b, a, who, &rew, &done);
        if (done) return a;
      }
    }
  }
  // the moves the draw chooses among: the legal ones, or for Negamax (negamax.h; k_negamax_games wrote the
  // tree's codes before this kernel) the legal ones whose code is best in the order +1 > +3 > ... > 0 > ... > -2
  uint32_t cand = legal;
  if (kind == SPMCTS_PLAYER_NEGAMAX) {
    const int8_t *code = v.nm_score + (size_t)tree * G::A;
    int best = -1024;
    cand = 0;
    for (int a = 0; a < G::A; ++a) {
      if (!((legal >> a) & 1u)) continue;
      const int rk = nm_rank(code[a]);
      if (rk > best) {
        best = rk;
        cand = 0;
      }
      if (rk == best) cand |= 1u << a;
    }
  }
  const int n = popc((uint64_t)cand);
  if (n == 0) return 0;
  TreeRng r;
  rng_load(v, tree, r);
  bool terr = false;
  const double u = rng_next(v, r, &terr);
  rng_store(v, tree, r);
  if (terr) set_err(v, SPMCTS_ERR_TAPE);
  int k = (int)(u * (double)n);
  if (k >= n) k = n - 1;
  for (int a = 0; a < G::A; ++a)
    if ((cand >> a) & 1u) {
      if (k == 0) return a;
      --k;
    }
  return 0;
}

template <class G>
__global__ void k_games_end_ply(View v) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= v.G) return;
  if (v.gstate[g] != GS_ACTIVE) return;
  const int mover = (v.gply[g] + v.gswap[g]) & 1;
  const int tree = 2 * g + mover;
  const int m = v.mv_count[tree];
  float pr[G::A];
  PlayOut o{0, false, 0.0, 0};
  const int kind = v.tkind[tree];
  const bool book = in_book(v, g);
  if (book) {
    o.action = v.book_moves[(size_t)v.gopen[g] * v.book_len + v.gply[g]];
  } else if (kind == SPMCTS_PLAYER_MCTS) {
    o = play_move_choice<G>(v, tree, 1.0, pr);
  } else {
    const Board envb = mover == 0 ? Board{v.gpos[g], v.gneg[g]} : Board{v.gneg[g], v.gpos[g]};
    o.action = hardcoded_move<G>(v, tree, kind, envb, v.rplayer[tree]);
  }
  if (o.recorded && v.record) {
    if (m < G::MAXM) {
      const size_t rec = (size_t)tree * G::MAXM + m;
      write_state<G>(Board{v.rpos[tree], v.rneg[tree]}, v.mv_state + rec * G::CELLS);
      for (int j = 0; j < G::A; ++j) v.mv_probs[rec * G::A + j] = pr[j];
      v.mv_q[rec] = o.q;
      v.mv_qf64[rec] = o.qf64;
      v.mv_count[tree] = m + 1;
    } else {
      set_err(v, SPMCTS_ERR_STATE);
    }
  }
  // env.step in the policy's frame (play_move :221-224): policy plays +1, opponent -1
  const int p_env = mover == 0 ? 1 : -1;
  Board gb{v.gpos[g], v.gneg[g]};
  int rew = 0, done = 0;
  // a book move is held to the host validation's rule (an occupied TicTacToe cell is a silent no-op of step)
  if (book && (o.action >= G::A || !((legal_mask<G>(gb) >> o.action) & 1u))) set_err(v, SPMCTS_ERR_ACTION);
  const int st = step<G>(gb, o.action, p_env, &rew, &done);
  if (st != STEP_OK) set_err(v, SPMCTS_ERR_ACTION);
  // the game log (spmcts_games_set_log): every ply's action, whoever chose it (a game has at most CELLS plies)
  if (v.glog && v.gply[g] < G::CELLS) v.glog[(size_t)g * G::CELLS + v.gply[g]] = (uint8_t)o.action;
  v.gpos[g] = gb.pos;
  v.gneg[g] = gb.neg;
  v.gply[g] += 1;
  if (done && book) set_err(v, SPMCTS_ERR_STATE);  // host validation keeps a book move from ending the game
  if (done) {
    v.gstate[g] = GS_DONE;
    v.gresult[g] = (int8_t)(rew * p_env);  // r = r * player (:218)
    return;  // both trees are discarded with the game
  }
  if (v.tkind[2 * g] == SPMCTS_PLAYER_MCTS) set_node<G>(v, 2 * g, o.action);
  if (v.tkind[2 * g + 1] == SPMCTS_PLAYER_MCTS) set_node<G>(v, 2 * g + 1, o.action);
}

// finished games: offsets into the export ring + refill ids (single block, slot order)
template <class G>
__global__ __launch_bounds__(1024) void k_games_finish_scan(View v, int refill, int32_t *out) {
  __shared__ int32_t s_rec[1024];
  __shared__ int32_t s_fin[1024];
  const int tid = threadIdx.x;
  const int Gn = v.G;
  const int chunk = (Gn + 1023) / 1024;
  const int lo = min(Gn, tid * chunk), hi = min(Gn, lo + chunk);
  int rec = 0, fin = 0;
  for (int g = lo; g < hi; ++g)
    if (v.gstate[g] == GS_DONE) {
      rec += v.mv_count[2 * g] + v.mv_count[2 * g + 1];
      fin += 1;
    }
  s_rec[tid] = rec;
  s_fin[tid] = fin;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int a1 = tid >= off ? s_rec[tid - off] : 0;
    const int a2 = tid >= off ? s_fin[tid - off] : 0;
    __syncthreads();
    s_rec[tid] += a1;
    s_fin[tid] += a2;
    __syncthreads();
  }
  const int base_rec = v.ex_count[0];
  int r0 = base_rec + s_rec[tid] - rec;
  int f0 = s_fin[tid] - fin;
  // per-game: record offset and finish index (for refill ids) in gscratch[2*g], [2*g+1]
  for (int g = lo; g < hi; ++g)
    if (v.gstate[g] == GS_DONE) {
      v.gscratch[2 * g] = r0;
      v.gscratch[2 * g + 1] = f0;
      r0 += v.mv_count[2 * g] + v.mv_count[2 * g + 1];
      f0 += 1;
    }
  __syncthreads();
  if (tid == 0) {
    const int total_rec = s_rec[1023], total_fin = s_fin[1023];
    int64_t started = v.gcnt[7];
    int64_t limit = v.gcnt[8];
    int64_t can = 0;
    if (refill) {
      if (limit < 0) {
        can = total_fin;
      } else {
        const int64_t room = limit - started;
        can = room < 0 ? 0 : (room < (int64_t)total_fin ? room : (int64_t)total_fin);
      }
    }
    v.gscratch[2 * Gn] = (int32_t)can;     // refills this ply
    v.gscratch[2 * Gn + 1] = (int32_t)(started & 0x7fffffff);
    ((int64_t *)(v.gscratch + 2 * Gn + 2))[0] = started;
    v.gcnt[7] = started + can;
    v.gcnt[0] += total_fin;
    if (base_rec + total_rec > v.ex_cap) atomicOr(v.err, SPMCTS_ERR_EXPORT);
    v.ex_count[0] = min(v.ex_cap, base_rec + total_rec);
    v.gcnt[9] += min(total_rec, v.ex_cap - base_rec);
    if (v.glog) {  // the finished-game ring: game g's record goes to base + its finish index (k_games_finish_apply)
      const int base_log = v.lr_count[0];
      v.gscratch[2 * Gn + 4] = base_log;
      if (base_log + total_fin > v.lr_cap) atomicOr(v.err, SPMCTS_ERR_EXPORT);  // the records past the end are dropped whole
      v.lr_count[0] = min(v.lr_cap, base_log + total_fin);
    }
    if (out) {
      out[0] = total_fin;
      out[1] = v.ex_count[0];
    }
  }
}

template <class G, bool SB = false>
__global__ void k_games_finish_apply(View v) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= v.G) return;
  if (v.gstate[g] != GS_DONE) return;
  const int r = v.gresult[g];
  const int swap = v.gswap[g];
  // results breakdown (self_play_parallel.py:302-327): reward in the policy's view
  atomicAdd((unsigned long long *)&v.gcnt[1 + swap * 3 + (r == 1 ? 0 : (r == 0 ? 1 : 2))], 1ull);
  // push_to_queue: policy's moves with r, then opposing's with -r (selfplayworker.py:186-190)
  int off = v.gscratch[2 * g];
  for (int side = 0; side < 2; ++side) {
    const int tree = 2 * g + side;
    const float z = side == 0 ? (float)r : (float)(-r);
    const int m = v.mv_count[tree];
    for (int k = 0; k < m; ++k, ++off) {
      if (off >= v.ex_cap) continue;
      const size_t src = (size_t)tree * G::MAXM + k;
      for (int c = 0; c < G::CELLS; ++c) v.ex_state[(size_t)off * G::CELLS + c] = v.mv_state[src * G::CELLS + c];
      for (int j = 0; j < G::A; ++j) v.ex_probs[(size_t)off * G::A + j] = v.mv_probs[src * G::A + j];
      v.ex_q[off] = v.mv_q[src];
      v.ex_qf64[off] = v.mv_qf64[src];
      v.ex_z[off] = z;
      v.ex_game[off] = v.gid[g];
    }
  }
  const int fin_idx = v.gscratch[2 * g + 1];
  const int can = v.gscratch[2 * v.G];
  if (v.glog) {  // the game's record, before start_game reuses the slot
    const int at = v.gscratch[2 * v.G + 4] + fin_idx;
    if (at < v.lr_cap) {
      const int plies = min(v.gply[g], (int)G::CELLS);
      v.lr_id[at] = v.gid[g];
      v.lr_slot[at] = g;
      v.lr_result[at] = (int8_t)r;
      v.lr_swap[at] = (uint8_t)swap;
      v.lr_plies[at] = plies;
      v.lr_open[at] = v.book_n ? v.gopen[g] : -1;
      for (int c = 0; c < G::CELLS; ++c)
        v.lr_moves[(size_t)at * G::CELLS + c] = c < plies ? v.glog[(size_t)g * G::CELLS + c] : (uint8_t)0;
    }
  }
  const int64_t started = ((const int64_t *)(v.gscratch + 2 * v.G + 2))[0];
  if (fin_idx < can) {
    start_game<G, SB>(v, g, started + fin_idx, nullptr);
  } else {
    v.gstate[g] = GS_IDLE;
  }
}

// Root statistics of n listed trees, the values of spmcts_root_stats, with no host synchronisation: one
// APAD-lane group per tree (lane j: child j; lane 0: the root's own fields; the board's cells strided).
template <class G>
__global__ void k_root_stats_batch(View v, const int32_t *trees, int n, int32_t *child_n, double *child_w,
                                   float *child_p, int32_t *root_n, double *root_w, int8_t *root_player, int8_t *boards) {
  constexpr int P = G::APAD;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = t / P, j = t % P;
  if (i >= n) return;
  const int tree = trees[i];
  if (tree < 0 || tree >= v.T) {
    if (j == 0) set_err(v, SPMCTS_ERR_STATE);
    return;
  }
  const size_t nb = nbase<G>(v, tree);
  const int root = v.root[tree];
  const int cb = nd_c<P>(v, nb + root);
  if (j < G::A) {
    const size_t c = nb + (size_t)(cb >= 0 ? cb : 0) * P + j, o = (size_t)i * G::A + j;
    if (child_n) child_n[o] = cb >= 0 ? nd_n<P>(v, c) : 0;
    if (child_w) child_w[o] = cb >= 0 ? nd_w<P>(v, c) : 0.0;
    if (child_p) child_p[o] = cb >= 0 ? nd_p<P>(v, c) : 0.f;
  }
  if (j == 0) {
    if (root_n) root_n[i] = nd_n<P>(v, nb + root);
    if (root_w) root_w[i] = nd_w<P>(v, nb + root);
    if (root_player) root_player[i] = v.rplayer[tree];
  }
  if (boards) {
    const Board b{v.rpos[tree], v.rneg[tree]};
    for (int c = j; c < G::CELLS; c += P) boards[(size_t)i * G::CELLS + c] = cell_value<G>(b, c / G::H, c % G::H);
  }
}

__global__ void k_export(View v, int A, int cells, int8_t *st, float *pr, double *q, uint8_t *qf, float *z, int64_t *gid,
                         int max_records, int32_t *count_out) {
  const int n = min(v.ex_count[0], max_records);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 && count_out) count_out[0] = n;
  if (i >= n) return;
  for (int c = 0; c < cells; ++c) st[(size_t)i * cells + c] = v.ex_state[(size_t)i * cells + c];
  for (int j = 0; j < A; ++j) pr[(size_t)i * A + j] = v.ex_probs[(size_t)i * A + j];
  q[i] = v.ex_q[i];
  qf[i] = v.ex_qf64[i];
  z[i] = v.ex_z[i];
  gid[i] = v.ex_game[i];
}

__global__ void k_export_clear(View v) { v.ex_count[0] = 0; }

// the finished-game ring (spmcts_games_set_log) out to the caller's arrays, one per field: the twin of k_export
__global__ void k_export_games(View v, int cells, int64_t *id, int32_t *slot, int8_t *result, uint8_t *swap, int32_t *plies,
                               int32_t *opening, uint8_t *moves, int max_records, int32_t *count_out) {
  const int n = min(v.lr_count[0], max_records);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 && count_out) count_out[0] = n;
  if (i >= n) return;
  id[i] = v.lr_id[i];
  slot[i] = v.lr_slot[i];
  result[i] = v.lr_result[i];
  swap[i] = v.lr_swap[i];
  plies[i] = v.lr_plies[i];
  opening[i] = v.lr_open[i];
  for (int c = 0; c < cells; ++c) moves[(size_t)i * cells + c] = v.lr_moves[(size_t)i * cells + c];
}

__global__ void k_export_games_clear(View v) { v.lr_count[0] = 0; }
