// arena_expand.h — tree search, second half: k_expand, the threaded expand and select (one slot-cycle walk), _play, k_search_end, set_node, k_play_action.
// Included by spmcts.hip after arena_rows.h: needs the select helpers and the cache record layout.
// ----------------------------------------------------------------------------
// kernel: expand + backup of network-evaluated leaves (mcts.py:316-321, :94-98)
// ----------------------------------------------------------------------------
// SB (arena_solver.h): the new block is stamped with its moves' score bounds and the change carried up the path.
// SYM (spmcts_set_symmetry): rows are in canonical orientation (arena_rows.h, leaf_key); a leaf whose input was
// flipped takes prior a from prow[m(a)], so node priors are in the tree's orientation.
template <class G, bool SB = false, bool SYM = false>
__global__ __launch_bounds__(64) void k_expand(View v, const float *probs0, const float *values0,
                                               const float *probs1, const float *values1) {
  constexpr int P = G::APAD;
  const int lane = threadIdx.x & (P - 1);
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) / P;
  if (row >= v.T || !row_live(v, row)) return;
  // network-1 rows read their outputs from the second network's buffers (row - seg1)
  const bool s1 = row >= v.seg1;
  const float *prow = s1 ? probs1 + (size_t)(row - v.seg1) * G::A : probs0 + (size_t)row * G::A;
  const float vrow = s1 ? values1[row - v.seg1] : values0[row];
  const int tree = v.row_tree[row];
  const size_t nb = nbase<G>(v, tree);
  const size_t bb = (size_t)tree * v.cap;
  const int blk = v.used[tree];
  if (blk >= v.cap) {
    if (lane == 0) set_err(v, SPMCTS_ERR_POOL);
    return;
  }
  const int leaf = v.leaf[tree];
  // create_children (mcts.py:103-107): A children in action order, validity = valid_moves
  {
    const size_t ci = nb + (size_t)blk * P + lane;
    nd_n<P>(v, ci) = 0;
    nd_w<P>(v, ci) = 0.0;
    int src = lane;
    if constexpr (SYM) {
      const bool pm = v.lmover[tree] > 0;  // (K = 1: the tree is its pending slot)
      uint64_t own = pm ? v.lpos[tree] : v.lneg[tree], opp = pm ? v.lneg[tree] : v.lpos[tree];
      if (canonical_pair<G>(own, opp) && lane < G::A) src = mirror_action<G>(lane);
    }
    nd_p<P>(v, ci) = lane < G::A ? prow[src] : 0.f;
    nd_c<P>(v, ci) = -1;
    nd_f<P>(v, ci) = 0;
  }
  const int mover = v.lmover[tree];
  // network(s, parent.player) returns value * player (modules.py:109-112)
  const double val = (double)vrow * (double)mover;
  const int plen = v.plen[tree];
  const size_t pb = (size_t)tree * G::MAXD;
  for (int k = lane; k < plen; k += P) {
    const size_t idx = nb + v.pnode[pb + k];
    nd_n<P>(v, idx) = v.pn[pb + k] + 1;
    nd_w<P>(v, idx) = v.pw[pb + k] + val;
  }
  if (lane == 0) {
    nd_vm<P>(v, bb + blk) = legal_mask<G>(Board{v.lpos[tree], v.lneg[tree]});
    nd_c<P>(v, nb + leaf) = blk;
    nd_n<P>(v, nb + leaf) = v.leaf_n[tree] + 1;
    nd_w<P>(v, nb + leaf) = v.leaf_w[tree] + val;
    v.used[tree] = blk + 1;
    v.need[tree] = NEED_EMPTY;
    v.cnt[(size_t)tree * C_NCNT + C_NN] += 1;
    v.cnt[(size_t)tree * C_NCNT + C_HWM] = max(v.cnt[(size_t)tree * C_NCNT + C_HWM], (int64_t)(blk + 1));
  }
  if constexpr (SB) {  // (the one expansion of this tree in the launch: nothing it reads was written here)
    int lo, hi;
    sb_stamp<G>(v, nb, blk, Board{v.lpos[tree], v.lneg[tree]}, -mover, lane, lo, hi);
    sb_propagate<G>(v, nb, leaf, plen, lo, hi, lane, [&](int k) { return v.pnode[pb + k]; }, [](bool, int, int) {});
  }
}

// ----------------------------------------------------------------------------
// kernel: the network replies of the threaded search, slot by slot (mcts.py:360-365): create_children,
// backup (n += 1, w += v on the leaf and its path), unlock, vl -= 1 on the path — and, while the
// search has sims left, refill the slot at once (the rolling schedule above).  Read-modify-write:
// earlier slots of the same tree have changed the shared ancestors.  Pending leaves of trees that
// are not searching (a _set_node expansion, slot 0, path length 0) are completed without a refill.
// The slots are walked cyclically from the tree's resume point (View::tres; arena_select.h "sim cap"): a
// slot's reply takes its outputs from its row (NEED_ROW: evaluated by the network launch before this one) or
// from the stash (NEED_STASH), and a launch that pauses at the cap leaves the outputs of the slots it has not
// replied yet in the stash.
// ----------------------------------------------------------------------------
// (The body is a function of its own, inlined into the kernel: hipcc optimises it before it inlines it, and
// written straight into the kernel the prefetch below lost its merged LDS stores.)
// Workgroup of k_expand_vl: four waves, a P-lane group per tree; the waves share nothing (no barrier, per-group
// LDS).  With every wave live (the packed domain) fewer, larger workgroups wait for fewer CU grants beside
// the other lane's trunk: 256 threads measured +0.6 % on the bench against 64 and +0.4 % against 128, every
// run above every run of either ("Packed launch domain").
constexpr int EXPAND_THREADS = 256;
// k_select_vl, the first step of a search (and every step of a host loop that selects per step), is the same
// walk without rows (ROWS false): no network launch precedes it, so a NEED_ROW slot is not evaluated yet and
// ends the walk; empty slots are filled and NEED_STASH slots replied.  The latter matters to host loops that
// skip the expand of a step without rows: a paused tree's stashed replies then still run, in the select.  One
// wave per workgroup there: workgroups of 2..8 waves were measured slower for the once-per-ply first fill, as
// were LDS copies of the child blocks a tree's sims read (the isolated expand 250 -> 295-300 us: a launch
// starts with no copies, so most blocks are copied once and read once, and the levels of a sim are a chain of
// short dependent LDS / permute / FP64 latencies, not memory round trips): DESIGN.md §4.
constexpr int SELECT_THREADS = 64;

// SYM (spmcts_set_symmetry; only with ROWS): lane j < K works out whether its slot's input was flipped, from the
// record it holds anyway, and the row read below takes prob m(lane) of a flipped slot's canonical row.  The LDS
// copy, the node priors and the stash are then in the tree's orientation, as without the mode.
template <class G, int THREADS, bool ROWS, bool SB = false, bool SYM = false>
__device__ __forceinline__ void expand_vl_body(View v, const float *probs0, const float *values0,
                                               const float *probs1, const float *values1) {
  constexpr int P = G::APAD;
  constexpr int GPB = THREADS / P;
  constexpr int KMAX = P;  // slots whose records one lane each prefetches (spmcts_arena_create: K <= P)
  __shared__ int32_t s_node[GPB][G::MAXD], s_n[GPB][G::MAXD], s_vl[GPB][G::MAXD], s_cs[GPB][G::MAXD];
  __shared__ double s_w[GPB][G::MAXD];
  // the prefetched path nodes (k < P) and network outputs of each slot, per tree group; each LDS word
  // is written and later read by the same wave (LDS operations of a wave stay in order)
  __shared__ int32_t s_pnode[GPB][KMAX][P];
  __shared__ float s_pr[GPB][KMAX][P];
  __shared__ float s_vr[GPB][KMAX];
  const int lane = threadIdx.x & (P - 1);
  const int grp = threadIdx.x / P;
  const int gbase = (threadIdx.x & 63) & ~(P - 1);
  // one lane group per entry of the launch domain (View::dn): every tree, or the searching trees only
  const int entry = (blockIdx.x * blockDim.x + threadIdx.x) / P;
  if (entry >= v.dn) return;
  const int tree = dom_tree(v, entry);
  if (tree < 0) return;
  const PathLds pl{s_node[grp], s_n[grp], s_vl[grp], s_cs[grp], s_w[grp]};
  StoreFence sf;
  const int K = v.K;
  const size_t nb = nbase<G>(v, tree);
  const size_t bb = (size_t)tree * v.cap;
  // prefetch (independent loads, one round trip): lane j < K holds pending slot j's record, every lane
  // the j-th path node of each slot; the tree's counters
  const int psl = tree * K + (lane < K ? lane : 0);
  const int my_need = lane < K ? (int)v.need[psl] : 0;
  const int res = v.tres[tree];
  const int my_srow = v.srow[psl], my_leaf = v.leaf[psl], my_plen = v.plen[psl];
  const int my_mover = v.lmover[psl];
  const uint64_t my_pos = v.lpos[psl], my_neg = v.lneg[psl];
  {
    int pn[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
      pn[j] = (j < K && lane < G::MAXD) ? v.pnode[(size_t)(tree * K + j) * G::MAXD + lane] : 0;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) s_pnode[grp][j][lane] = pn[j];
  }
  // nothing pending and no paused fill: the tree takes no part in this step
  if (ROWS && !group_or<P>(my_need) && !(res & RES_FILL)) return;
  const int limit = min(v.budget[tree], v.iters);
  int started = v.tstarted[tree];
  const bool refill = started < limit;
  if (!ROWS && !refill) return;  // a select: searching trees only
  int used = v.used[tree];
  const bool noise = v.noise_on[tree] != 0;
  const double nz = (noise && lane < G::A) ? v.noise[(size_t)tree * P + lane] : 0.0;
  TreeRng rng;
  TreeRootT<SB> R;
  if (refill) {
    rng_load(v, tree, rng);
    R = load_root<G, SB>(v, tree);
  }
  // the network outputs of the pending slots (second round trip: they depend on the rows)
  {
    float pr[KMAX], vr[KMAX];
    int my_flip = 0, mlane = lane;
    if constexpr (ROWS && SYM) {
      uint64_t own = my_mover > 0 ? my_pos : my_neg, opp = my_mover > 0 ? my_neg : my_pos;
      my_flip = canonical_pair<G>(own, opp) ? 1 : 0;
      if (lane < G::A) mlane = mirror_action<G>(lane);
    }
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      const int nj = __shfl(my_need, gbase + j, 64), row = __shfl(my_srow, gbase + j, 64);
      const int fj = (ROWS && SYM) ? __shfl(my_flip, gbase + j, 64) : 0;
      pr[j] = 0.f;
      vr[j] = 0.f;
      if (ROWS && j < K && nj == NEED_ROW) {
        const bool s1 = row >= v.seg1;
        const float *prow = s1 ? probs1 + (size_t)(row - v.seg1) * G::A : probs0 + (size_t)row * G::A;
        if (lane < G::A) pr[j] = prow[fj ? mlane : lane];
        vr[j] = s1 ? values1[row - v.seg1] : values0[row];
      } else if (j < K && nj == NEED_STASH) {  // evaluated in an earlier step, kept across a pause
        const size_t sj = (size_t)tree * K + j;
        pr[j] = v.stash_p[sj * P + lane];
        vr[j] = v.stash_v[sj];
      }
    }
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      s_pr[grp][j][lane] = pr[j];
      if (lane == 0) s_vr[grp][j] = vr[j];
    }
  }
  bool terr = false;
  SimCntT<SB> sc;
  // the cycle from the resume slot, once round (a slot met again was filled in this launch: its reply is the
  // next launch's); a searching tree cycles over its own kt slots, any other over all K (its one pending slot)
  const int kt = refill ? v.tK[tree] : K;
  int j = res >> 1, nst = 0;
  if ((unsigned)j >= (unsigned)kt) j = 0;  // (a tree whose sims in flight were lowered since its last search)
  if ((res & RES_FILL) && (!refill || __shfl(my_need, gbase + j, 64))) {
    if (lane == 0) set_err(v, SPMCTS_ERR_STATE);  // a paused fill is of an empty slot of a searching tree
    return;
  }
  int paused_at = -1;  // iterations done when the cap paused the tree
  // one copy of the slot body (a rolled loop: the unrolled form was 70 KB of code, more than the
  // instruction cache two CUs share, for a kernel that runs one wave per CU on a latency chain)
#pragma unroll 1
  for (int i = 0; i < kt; ++i, j = j + 1 == kt ? 0 : j + 1) {
    const int ps = tree * K + j;
    const int nj = __shfl(my_need, gbase + j, 64);
    if (!ROWS && nj == NEED_ROW) break;  // not evaluated: the cycle goes on at this reply, in an expand
    if (nj != NEED_EMPTY) {
      const int leaf = __shfl(my_leaf, gbase + j, 64), plen = __shfl(my_plen, gbase + j, 64);
      const int mover = __shfl(my_mover, gbase + j, 64);
      const uint64_t lpos = __shfl(my_pos, gbase + j, 64), lneg = __shfl(my_neg, gbase + j, 64);
      const int blk = used;
      if (blk >= v.cap) {  // sticky SPMCTS_ERR_POOL; the counters of the slots done so far are still flushed
        if (lane == 0) set_err(v, SPMCTS_ERR_POOL);
        break;
      }
      ++used;
      const float pnew = lane < G::A ? s_pr[grp][j][lane] : 0.f;
      const uint32_t vmnew = legal_mask<G>(Board{lpos, lneg});
      {
        const size_t ci = nb + (size_t)blk * P + lane;
        nd_n<P>(v, ci) = 0;
        nd_w<P>(v, ci) = 0.0;
        nd_p<P>(v, ci) = pnew;
        nd_c<P>(v, ci) = -1;
        nd_f<P>(v, ci) = 0;
        nd_vl<P>(v, ci) = 0;
      }
      const double val = (double)s_vr[grp][j] * (double)mover;
      if (!refill) {
        // no sims in this launch (the root not in registers): read-modify-write backup of the
        // path (distinct nodes): one lane per path node, the node ids prefetched; a node's depth fixes its
        // lane, so the slots' updates of a shared ancestor are one lane's program order
        for (int k = lane; k < plen; k += P) {
          const size_t idx = nb + (k < P ? s_pnode[grp][j][k] : v.pnode[(size_t)ps * G::MAXD + k]);
          nd_n<P>(v, idx) += 1;
          nd_w<P>(v, idx) += val;
          nd_vl<P>(v, idx) -= 1;
        }
        if (lane == 0) {
          nd_vm<P>(v, bb + blk) = vmnew;
          nd_c<P>(v, nb + leaf) = blk;
          nd_n<P>(v, nb + leaf) += 1;
          nd_w<P>(v, nb + leaf) += val;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      } else {
        // with sims in this launch: the root and its children from the registers (TreeRoot), deeper path
        // nodes and the leaf read-modify-write in global memory, after a fence if a store is outstanding
        // (StoreFence: the new block's stores above are)
        if (lane == 0) nd_vm<P>(v, bb + blk) = vmnew;
        sf.dirty = true;
        const int a1 = plen > 1 ? s_pnode[grp][j][1] - R.cb * P : 0;  // path node 1: root child a1
        const int r1n = __shfl(R.cn, gbase + a1, 64), r1vl = __shfl(R.cvl, gbase + a1, 64);
        const double r1w = __shfl(R.cw, gbase + a1, 64);
        sf.fence_if_dirty();
        int unc = 0;
        for (int k = lane; k < plen; k += P) {
          const int nk = k < P ? s_pnode[grp][j][k] : v.pnode[(size_t)ps * G::MAXD + k];
          const size_t idx = nb + nk;
          if (k == 0) {  // the root
            nd_n<P>(v, idx) = R.n + 1;
            nd_w<P>(v, idx) = R.w + val;
            nd_vl<P>(v, idx) = R.vl - 1;
          } else if (k == 1) {  // root child a1
            nd_n<P>(v, idx) = r1n + 1;
            nd_w<P>(v, idx) = r1w + val;
            nd_vl<P>(v, idx) = r1vl - 1;
          } else {
            nd_n<P>(v, idx) += 1;
            nd_w<P>(v, idx) += val;
            nd_vl<P>(v, idx) -= 1;
            unc = 1;
          }
        }
        // the leaf: a root child (plen 1, registers: lane la), or a deeper node
        const int la = leaf - R.cb * P;
        if (plen == 1) {
          if (lane == la) {
            nd_c<P>(v, nb + leaf) = blk;
            nd_n<P>(v, nb + leaf) = R.cn + 1;
            nd_w<P>(v, nb + leaf) = R.cw + val;
          }
        } else {
          if (lane == 0) {
            nd_c<P>(v, nb + leaf) = blk;
            nd_n<P>(v, nb + leaf) += 1;
            nd_w<P>(v, nb + leaf) += val;
          }
          unc = 1;
        }
        if (group_or<P>(unc)) sf.dirty = true;
      }
      if constexpr (SB) {
        // stored bounds (arena_solver.h): stamp the new block, carry the change up the slot's path.  The entries
        // the walk reads may have been written by an earlier slot's walk of this launch: StoreFence's rule
        int lo, hi;
        sb_stamp<G>(v, nb, blk, Board{lpos, lneg}, -mover, lane, lo, hi);
        sf.dirty = true;
        if (plen > 0) {
          sf.fence_if_dirty();
          // (a rewritten entry of the root's own block reaches TreeRoot's copy too: the fills below select on it)
          if (sb_propagate<G>(
                  v, nb, leaf, plen, lo, hi, lane,
                  [&](int k) { return k < P ? s_pnode[grp][j][k] : v.pnode[(size_t)ps * G::MAXD + k]; },
                  [&](bool me, int nlo, int nhi) {
                    if (refill && R.rules && me) R.cbnd = sb_pack(nlo, nhi);
                  }))
            sf.dirty = true;
        }
      }
      if (lane == 0) {
        v.used[tree] = blk + 1;
        v.need[ps] = NEED_EMPTY;
      }
      sc.nn += 1;
      sc.hwm = max(sc.hwm, (int64_t)(blk + 1));
      if (refill && plen > 0) {  // the root is the path's first node
        R.n += 1;
        R.vl -= 1;
        R.w += val;
      }
      if (refill && plen > 1) {  // path node 1 is a root child: its copy in registers
        if (lane == s_pnode[grp][j][1] - R.cb * P) {
          R.cn += 1;
          R.cw += val;
          R.cvl -= 1;
        }
      } else if (refill && plen == 1) {  // the leaf itself is a root child
        if (lane == leaf - R.cb * P) {
          R.cc = blk;
          R.cn += 1;
          R.cw += val;
        }
      }
    }
    if (refill) {
      const int r = fill_slot_vl<G, SB>(v, tree, j, limit, started, nst, R, rng, terr, pl, noise, nz, sc, sf);
      if (r == SIM_ERROR) break;  // sticky SPMCTS_ERR_STATE; counters flushed below
      if (r == SIM_PAUSED) {
        paused_at = i;
        break;
      }
    }
  }
  if (paused_at >= 0) {
    // the cycle goes on at slot j's fill; the slots after it whose rows this launch read keep their outputs
    // (lane a < A: prob a, lane 0: the value; their need was NEED_ROW, the stash of a NEED_STASH slot stands)
    sc.pause += 1;
    int q = j;
    for (int i = paused_at + 1; i < kt; ++i) {
      q = q + 1 == kt ? 0 : q + 1;
      if (!ROWS || __shfl(my_need, gbase + q, 64) != NEED_ROW) continue;
      const size_t sq = (size_t)tree * K + q;
      v.stash_p[sq * P + lane] = s_pr[grp][q][lane];
      if (lane == 0) {
        v.stash_v[sq] = s_vr[grp][q];
        v.need[sq] = NEED_STASH;
      }
    }
  }
  if (lane == 0) {
    sc.flush(v.cnt + (size_t)tree * C_NCNT);
    if constexpr (SB) {
      if (sc.proved | sc.reflev) sc.flush_solver(v.sv_stats + (size_t)tree * SV_NSTAT);
    }
  }
  if (refill && lane == 0) {
    v.tstarted[tree] = started;
    // a complete cycle ends where it began (j is back there), at that slot's reply
    v.tres[tree] = j * 2 + (paused_at >= 0 ? RES_FILL : 0);
    if (terr) set_err(v, SPMCTS_ERR_TAPE);
    rng_store(v, tree, rng);
  }
}

template <class G, bool SB = false, bool SYM = false>
__global__ __launch_bounds__(EXPAND_THREADS) void k_expand_vl(View v, const float *probs0, const float *values0,
                                                  const float *probs1, const float *values1) {
  expand_vl_body<G, EXPAND_THREADS, true, SB, SYM>(v, probs0, values0, probs1, values1);
}

// (its domain: the active list, View::dn = its length, dpack = 1: spmcts_select_tree)
template <class G, bool SB = false>
__global__ __launch_bounds__(SELECT_THREADS) void k_select_vl(View v) {
  expand_vl_body<G, SELECT_THREADS, false, SB>(v, nullptr, nullptr, nullptr, nullptr);
}

// ----------------------------------------------------------------------------
// _play (mcts.py:272-299): choose the move from root visit counts
// ----------------------------------------------------------------------------
struct PlayOut {
  int action;
  bool recorded;
  double q;
  uint8_t qf64;
};

// numpy kahan_sum used by RandomState.choice's validation
__device__ __forceinline__ double kahan_sum(const double *p, int n) {
  double s = p[0], c = 0.0;
  for (int i = 1; i < n; ++i) {
    const double y = p[i] - c;
    const double t = s + y;
    c = (t - s) - y;
    s = t;
  }
  return s;
}

template <class G>
__device__ PlayOut play_move_choice(const View &v, int tree, double temp, float *probs_out) {
  constexpr int P = G::APAD;
  const size_t nb = nbase<G>(v, tree);
  const int root = v.root[tree];
  const int cb = nd_c<P>(v, nb + root);
  PlayOut o{0, false, 0.0, 0};
  // the move is chosen from a complete search: every search_node call started, every reply made (the sim cap
  // moves work between launches and must never leave any behind: arena_select.h "sim cap")
  if (v.K > 1 && (!tree_idle(v, tree) || v.tstarted[tree] < min(v.budget[tree], v.iters))) set_err(v, SPMCTS_ERR_STATE);
  int n[G::A];
  for (int j = 0; j < G::A; ++j) n[j] = cb >= 0 ? nd_n<P>(v, nb + (size_t)cb * P + j) : 0;
  double t = temp;
  if (v.evaluate) t = t / 20.0;
  const double inv = 1.0 / t;
  double pp[G::A];
  for (int j = 0; j < G::A; ++j) pp[j] = inv == 1.0 ? (double)n[j] : pow((double)n[j], inv);
  // proof-guided play (arena_proof.h): the moves the tree's own proof keeps, written by k_proof_verdict before
  // this kernel.  A move outside them weighs nothing; if no kept move has a visit (a win is classified from the
  // board alone), the kept moves weigh the same.  PF_ALL, the feature off for the tree: nothing here runs
  const uint32_t keep = v.pf_keep ? v.pf_keep[tree] : PF_ALL;
  if (keep != PF_ALL) {
    double ks = 0.0;
    for (int j = 0; j < G::A; ++j) {
      if (!((keep >> j) & 1u)) pp[j] = 0.0;
      ks = ks + pp[j];
    }
    if (ks == 0.0)
      for (int j = 0; j < G::A; ++j) pp[j] = ((keep >> j) & 1u) ? 1.0 : 0.0;
  }
  double s = 0.0;
  for (int j = 0; j < G::A; ++j) s = s + pp[j];
  double pr[G::A];
  for (int j = 0; j < G::A; ++j) pr[j] = pp[j] / s;
  // np.random.choice(A, p) validation (ValueError -> argmax fallback, mcts.py:290-295)
  bool ok = true;
  for (int j = 0; j < G::A; ++j)
    if (pr[j] < 0.0 || pr[j] != pr[j]) ok = false;
  if (ok && fabs(kahan_sum(pr, G::A) - 1.0) > 1.4901161193847656e-08) ok = false;
  if (ok) {
    TreeRng r;
    rng_load(v, tree, r);
    bool terr = false;
    const double u = rng_next(v, r, &terr);
    rng_store(v, tree, r);
    if (terr) set_err(v, SPMCTS_ERR_TAPE);
    double cdf[G::A];
    double c = 0.0;
    for (int j = 0; j < G::A; ++j) {
      c = c + pr[j];
      cdf[j] = c;
    }
    const double last = cdf[G::A - 1];
    int a = 0;
    for (int j = 0; j < G::A; ++j) {
      cdf[j] = cdf[j] / last;
      if (cdf[j] <= u) a = j + 1;  // searchsorted(u, side='right') on a non-decreasing cdf
    }
    if (a >= G::A) a = G::A - 1;
    o.action = a;
    o.recorded = true;
    for (int j = 0; j < G::A; ++j) probs_out[j] = (float)pr[j];
    const int rn = nd_n<P>(v, nb + root);
    if (v.K > 1) {
      // q (mcts.py:59-62) with the root's virtual loss, nonzero after a leaked sim (:349-354)
      const int rvl = nd_vl<P>(v, nb + root);
      o.q = (rn + rvl) ? (nd_w<P>(v, nb + root) - (double)rvl) / (double)(rn + rvl) : 0.0;
    } else {
      o.q = rn ? nd_w<P>(v, nb + root) / (double)rn : 0.0;
    }
    o.qf64 = nd_f<P>(v, nb + root);
  } else {
    int best = keep == PF_ALL ? 0 : __ffs((int)keep) - 1;  // (over the kept moves; PF_ALL keeps every j)
    for (int j = 1; j < G::A; ++j)
      if (((keep >> j) & 1u) && n[j] > n[best]) best = j;
    o.action = best;
  }
  v.noise_on[tree] = 0;  // remove_noise (mcts.py:55-57)
  v.cnt[(size_t)tree * C_NCNT + C_MOVES] += 1;
  return o;
}

template <class G>
__device__ __forceinline__ void write_state(Board b, int8_t *dst) {
  for (int x = 0; x < G::W; ++x)
    for (int y = 0; y < G::H; ++y) dst[x * G::H + y] = cell_value<G>(b, x, y);
}

template <class G>
__global__ void k_search_end(View v, int n_active, double temp, int32_t *actions, int8_t *states, float *tprobs,
                             double *qs, uint8_t *qf64, uint8_t *recorded) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_active) return;
  const int tree = v.active[i];
  if (tree < 0) return;
  float pr[G::A];
  const PlayOut o = play_move_choice<G>(v, tree, temp, pr);
  actions[i] = o.action;
  recorded[i] = o.recorded ? 1 : 0;
  qs[i] = o.q;
  qf64[i] = o.qf64;
  for (int j = 0; j < G::A; ++j) tprobs[(size_t)i * G::A + j] = o.recorded ? pr[j] : 0.f;
  write_state<G>(Board{v.rpos[tree], v.rneg[tree]}, states + (size_t)i * G::CELLS);
}

// _set_node (mcts.py:201-209) for one tree; returns false on an illegal action.
template <class G>
__device__ bool set_node(const View &v, int tree, int a) {
  constexpr int P = G::APAD;
  const size_t nb = nbase<G>(v, tree);
  const size_t bb = (size_t)tree * v.cap;
  const int root = v.root[tree];
  const int cb = nd_c<P>(v, nb + root);
  if (cb < 0 || a < 0 || a >= G::A || !((nd_vm<P>(v, bb + cb) >> a) & 1u)) {
    set_err(v, SPMCTS_ERR_ACTION);
    return false;
  }
  const int child = cb * P + a;
  const int rp = v.rplayer[tree];
  Board b{v.rpos[tree], v.rneg[tree]};
  int rew = 0, done = 0;
  step<G>(b, a, rp, &rew, &done);
  if (nd_n<P>(v, nb + child) == 0) {
    int64_t *cnt = v.cnt + (size_t)tree * C_NCNT;
    cnt[C_SETNODE] += 1;
    if (done) {
      const double val = terminal_value(v.tstrong[tree] != 0, Board{v.rpos[tree], v.rneg[tree]}, rew * rp);
      nd_n<P>(v, nb + child) = 1;
      nd_w<P>(v, nb + child) = nd_w<P>(v, nb + child) + val;
      if (v.tstrong[tree]) nd_f<P>(v, nb + child) = 1;
    } else {
      const int ps = tree * v.K;  // pending slot 0 of the tree
      if (!tree_idle(v, tree)) set_err(v, SPMCTS_ERR_STATE);  // the slot is taken only from an idle tree
      v.plen[ps] = 0;
      v.leaf[ps] = child;
      v.leaf_n[ps] = 0;
      v.leaf_w[ps] = nd_w<P>(v, nb + child);
      v.lpos[ps] = b.pos;
      v.lneg[ps] = b.neg;
      v.lmover[ps] = (int8_t)rp;
      v.need[ps] = NEED_ROW;
    }
  }
  v.root[tree] = child;
  v.rpos[tree] = b.pos;
  v.rneg[tree] = b.neg;
  v.rplayer[tree] = (int8_t)(-rp);
  return true;
}

template <class G>
__global__ void k_play_action(View v, const int32_t *trees, const int32_t *actions, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int t = trees[i];
  if (t < 0 || t >= v.T) return;
  set_node<G>(v, t, actions[i]);
}
