// arena_view.h — the device view of an arena (View), the node-record accessors, set_err, nbase.
// Included by spmcts.hip, first of the arena headers: needs board.h and spmcts.h.
// ----------------------------------------------------------------------------
// device view of an arena (passed by value to kernels)
// ----------------------------------------------------------------------------
typedef rocrand_state_philox4x32_10 Philox;

struct View {
  int T, cap, G, A;
  int iters;  // MCTreeSearch.iterations (bounds the last step of a K-in-flight search)
  int K, NS;  // simulations in flight per tree (virtual loss; 1 = sequential), pending slots = T * K
  // launch domain of a step's per-slot kernels (by value per launch, launch_rows): the pending slots of dn
  // trees -- every tree (dpack 0: entry i is tree i, dn = T) or the active list (dpack 1: entry i is tree
  // active[i], -1 = none, dn = its length).  Slot ids stay global (tree * K + j): dom_tree / dom_slot below
  int dn, dpack;
  double cpuct, x, alpha;
  int strong, evaluate, rng_mode, leaf_format, leaf_layout;
  // node store: one record of 32 * P bytes per child block (nd_* below)
  char *nodes;
  // trees
  int32_t *root;
  uint64_t *rpos, *rneg;
  int8_t *rplayer;
  int32_t *used;
  int32_t gc;         // 1: blocks_per_tree below the worst case -> compaction before a search (k_compact)
  int32_t *gc_list;   // [T][cap] scratch: live blocks (BFS order)
  int32_t *gc_map;    // [T][cap] scratch: old block -> new block (-1 dead)
  int32_t *tstarted;  // threaded search: search_node calls started in the current search (inactive: >= limit)
  double *noise;
  uint8_t *noise_on;
  int32_t *pnode;   // [T][MAXD] path node ids (root .. parent of leaf)
  int32_t *pn;      // [T][MAXD] their visit counts as read during select
  double *pw;       // [T][MAXD] their w as read during select
  int32_t *plen;
  int32_t *leaf;    // leaf node (local id)
  int32_t *leaf_n;
  double *leaf_w;
  uint64_t *lpos, *lneg;
  int8_t *lmover;
  uint8_t *need;      // per pending slot: NEED_EMPTY, NEED_ROW or NEED_STASH (below)
  // the sim cap (K > 1, arena_select.h "sim cap"): where the tree's slot cycle goes on in the next launch
  // (tres [T]: slot * 2 + RES_FILL), and the network outputs of NEED_STASH slots (stash_p [NS][P] probs,
  // stash_v [NS] value); simcap = sims a tree may start per launch (0 = no cap)
  int32_t *tres;
  float *stash_p, *stash_v;
  int simcap;
  Philox *rng;
  const double *tape;
  const int64_t *tape_end;  // [T] end offset
  int64_t *tape_cur;        // [T]
  int64_t *cnt;             // per-tree counters [T][8]
  int32_t *active;
  int32_t *row_tree;  // row -> pending slot (tree * K + j)
  int32_t *srow;      // pending slot -> row (K > 1)
  int32_t *row_count;
  // the step's row flags in the launch domain's compact order (k_dedup_owner[_peer] -> k_scan_need): entry c =
  // slot * 4 + d for a slot with a row (d as `down` below: 1 a row its network evaluates, 2 / 3 a served row),
  // else 0.  One contiguous word per slot of the domain, so each scan thread's chunk is one round of loads
  int32_t *crow;
  // batch leaf dedup (K > 1, spmcts_set_leaf_dedup): pending leaves with the same network input share
  // one row.  dtab: open-addressing table of (generation << 32 | owner slot), dent: a slot's entry
  uint64_t *dtab;
  int32_t *dent;
  uint8_t *down;  // 1 = the slot owns its key's row, 2 = the leader lane's row serves it (set per step)
  int dedup, dmask;
  uint32_t dgen;
  // cross-lane dedup (round 6, spmcts_set_leaf_peer): a leader arena keeps each owner slot's key in okey
  // (2 x u64 per slot) for the step; a follower's owner slot whose key the leader evaluates this step
  // takes the leader's row (down 2, xpeer = the leader's owner slot), copied in by k_peer_push
  uint64_t *okey;
  int32_t *xpeer;
  int lead;     // 1: this arena has followers (k_dedup_owner writes okey)
  int peer_on;  // 1 in a follower's simulation-step launches (down-2 slots: rows after its own, k_scan_need)
  // evaluation cache (round 6, spmcts_set_eval_cache): network outputs of the arena's own rows kept for `cwin`
  // generations (one per ply / search), keyed like the dedup table; an owner slot whose key is there takes
  // the cached outputs (down 3, xc = the entry) in a row after the network rows, filled by k_cache_io.
  // crec: one 64-byte record per entry (one line per probe): tag u64 ((generation << 32) | state, 0 = never used),
  // own u64, opp u64, then A probs + value as f32
  uint64_t *crec;
  int32_t *xc;
  int cwin, cmask;  // cwin 0 = off (also in launches where the cache is not live)
  uint32_t cgen;
  int cshared;  // 1: a follower lane using its leader's table (the leader inserts the rows it serves)
  float *root_prior;
  uint32_t *err;
  // games
  uint64_t *gpos, *gneg;
  int32_t *gply;
  uint8_t *gswap, *gstate;
  int8_t *gresult;
  int64_t *gid;
  int8_t *mv_state;
  float *mv_probs;
  double *mv_q;
  uint8_t *mv_qf64;
  int32_t *mv_count;
  int8_t *ex_state;
  float *ex_probs;
  double *ex_q;
  uint8_t *ex_qf64;
  float *ex_z;
  int64_t *ex_game;
  int32_t *ex_count;
  int32_t ex_cap;
  int64_t *gcnt;  // games counters: [0] finished [1..6] results [7] next id [8] limit [9] exported
  int32_t *gscratch;
  // per-tree players (two-network arenas, compare_models / evaluation games)
  uint8_t *tnet;     // [T] network whose leaves this tree sends (0 / 1)
  uint8_t *tkind;    // [T] SPMCTS_PLAYER_*: MCTS, or a hard-coded player (hardcoded_players.py)
  int32_t *budget;   // [T] simulations per search of this tree (MCTreeSearch.iterations)
  // per-tree search settings (each side of an evaluation game is built from its own container's
  // kwargs, selfplayworker.py:71-81): Dirichlet alpha, strong_play, sims in flight (<= K)
  double *talpha;
  uint8_t *tstrong;
  int32_t *tK;
  int32_t seg1;      // first leaf row of network 1 (= number of network-0 trees)
  int32_t record;    // games mode: keep Move records (play_episode update=True)
  int32_t sim;       // index of the current simulation within the search (by value per launch)
  // opening book (spmcts_games_set_openings): book_n openings of book_len bytes each (book_n = 0: off, the one
  // scalar the game kernels branch on), game id i plays opening ((i mod book_period) >> 1) mod book_n
  // (book_period 0: no modulus).  A game is in its book while gply < gbook: its ply's action is
  // book_moves[gopen * book_len + gply], nobody searches and no random number is drawn
  int32_t book_n, book_len, book_period;
  uint8_t *book_moves;  // [BOOK_MAX_OPENINGS][cells - 1] capacity, rows of book_len
  int32_t *book_lens;   // [BOOK_MAX_OPENINGS]
  int32_t *gopen;       // [G] the game's opening (-1: none)
  int32_t *gbook;       // [G] that opening's length (0: none)
  // negamax players (SPMCTS_PLAYER_NEGAMAX, negamax.h): the codes of each tree's moves for the ply, int8 [T][A],
  // written by k_negamax_games before k_games_end_ply reads them; null until a tree of the kind is set
  int8_t *nm_score;
  // game log (spmcts_games_set_log; null = off, the one pointer the game kernels test): glog uint8 [G][cells], the
  // action of every ply of the slot's current game (k_games_end_ply), and the finished-game ring of lr_cap records
  // (k_games_finish_scan / _apply -> spmcts_export_games), one array per field; lr_count[0] = records in the ring
  uint8_t *glog;
  int32_t lr_cap;
  int32_t *lr_count;
  int64_t *lr_id;
  int32_t *lr_slot;
  int8_t *lr_result;  // in tree 2g's view (gresult)
  uint8_t *lr_swap;
  int32_t *lr_plies;
  int32_t *lr_open;   // the game's opening, -1 without a book
  uint8_t *lr_moves;  // [lr_cap][cells], bytes past plies zero
  // proof-guided play (spmcts_set_proof_play, arena_proof.h; null until it is switched on, pf_keep the one pointer
  // the move choice tests): pf_on uint8 [T], the trees it is on for; the verdict k_proof_verdict wrote before the
  // tree's last move choice: pf_keep uint32 [T], the moves the choice may take (PF_ALL: no restriction), pf_lo /
  // pf_hi int8 [T], the root's score bounds (TB_NONE beside PF_ALL); pf_stats [PF_NSTAT], the PF_* counts below;
  // pf_nstop int32 [T], the searches of the tree that k_proof_stop has stopped so far
  uint8_t *pf_on;
  uint32_t *pf_keep;
  int8_t *pf_lo, *pf_hi;
  unsigned long long *pf_stats;
  int32_t *pf_nstop;
  // solver-aware search (spmcts_set_solver_rules, arena_solver.h; null until first use): sv_rules uint8 [T], the
  // search rules each tree's selects apply to the stored bounds (SBR_REFUTE | SBR_PROVED; null again while every
  // tree has none); sv_stats int64 [T][SV_NSTAT], sims ended by R2 and select levels at which R1 removed a child
  uint8_t *sv_rules;
  int64_t *sv_stats;
};

enum : uint32_t { PF_ALL = 0xffffffffu };
// View::pf_stats: plies chosen with proof play on, those with a solved root (lo == hi), with a secured win
// (lo > 0), with fewer kept moves than legal ones; trees k_proof_stop stopped, the sims they did not start
enum { PF_PLIES = 0, PF_SOLVED = 1, PF_WON = 2, PF_CUT = 3, PF_STOPPED = 4, PF_SKIPPED = 5, PF_NSTAT = 6 };

enum { BOOK_MAX_OPENINGS = 65536 };

// Node store.  A child block (the A children of one expanded node, P = APAD slots) is ONE contiguous
// record of 32 * P bytes: n i32[P] | vl i32[P] | child-block i32[P] | p f32[P] | w f64[P] | f64 flag
// u8[P] | valid-children mask u32 | pad.  The fields a select level scores (n, vl, child, p: the first
// 16 P bytes; w, the mask: the next) lie in two 128-byte lines for Connect4 (P = 8) instead of one line
// per field array.  Node id i = (tree * cap + block) * P + slot, as before; the flag is "w is a numpy
// float64" (strong_play dtype quirk, mcts.py:287/:308), vl is MCNode.virtual_loss (mcts.py:44).
// Stored score bounds (arena_solver.h; written only once spmcts_set_solver_search switched them on): lo i8[P] |
// hi i8[P] in what was pad, the bounds of the move into child j seen from the block's own node.
template <int P>
struct NodeRec {
  static constexpr int N = 0, VL = 4 * P, C = 8 * P, PR = 12 * P, W = 16 * P, F = 24 * P, VM = 25 * P, BYTES = 32 * P;
  static constexpr int LO = 26 * P, HI = 27 * P;
  static_assert(VM + 4 <= BYTES && W % 8 == 0 && VM % 4 == 0, "record layout");
  static_assert(VM + 4 <= LO && HI + P <= BYTES, "record layout: stored bounds");
};
template <int P>
__host__ __device__ __forceinline__ char *nd_rec(const View &v, size_t i) {
  return v.nodes + (i / P) * (size_t)NodeRec<P>::BYTES;
}
template <int P>
__host__ __device__ __forceinline__ int32_t &nd_n(const View &v, size_t i) {
  return ((int32_t *)(nd_rec<P>(v, i) + NodeRec<P>::N))[i % P];
}
template <int P>
__host__ __device__ __forceinline__ int32_t &nd_vl(const View &v, size_t i) {
  return ((int32_t *)(nd_rec<P>(v, i) + NodeRec<P>::VL))[i % P];
}
template <int P>
__host__ __device__ __forceinline__ int32_t &nd_c(const View &v, size_t i) {
  return ((int32_t *)(nd_rec<P>(v, i) + NodeRec<P>::C))[i % P];
}
template <int P>
__host__ __device__ __forceinline__ float &nd_p(const View &v, size_t i) {
  return ((float *)(nd_rec<P>(v, i) + NodeRec<P>::PR))[i % P];
}
template <int P>
__host__ __device__ __forceinline__ double &nd_w(const View &v, size_t i) {
  return ((double *)(nd_rec<P>(v, i) + NodeRec<P>::W))[i % P];
}
template <int P>
__host__ __device__ __forceinline__ uint8_t &nd_f(const View &v, size_t i) {
  return ((uint8_t *)(nd_rec<P>(v, i) + NodeRec<P>::F))[i % P];
}
template <int P>
__host__ __device__ __forceinline__ int8_t &nd_lo(const View &v, size_t i) {
  return ((int8_t *)(nd_rec<P>(v, i) + NodeRec<P>::LO))[i % P];
}
template <int P>
__host__ __device__ __forceinline__ int8_t &nd_hi(const View &v, size_t i) {
  return ((int8_t *)(nd_rec<P>(v, i) + NodeRec<P>::HI))[i % P];
}
// valid-children mask of block `gb` = tree * cap + block
template <int P>
__host__ __device__ __forceinline__ uint32_t &nd_vm(const View &v, size_t gb) {
  return *(uint32_t *)(v.nodes + gb * (size_t)NodeRec<P>::BYTES + NodeRec<P>::VM);
}

enum { C_SIMS = 0, C_NN = 1, C_TERM = 2, C_DEPTH = 3, C_SETNODE = 4, C_MOVES = 5, C_LEAK = 6, C_GC = 7, C_HWM = 8, C_PAUSE = 9, C_NCNT = 10 };
enum { GS_IDLE = 0, GS_ACTIVE = 1, GS_DONE = 2 };
// View::need of a pending slot.  NEED_ROW: its leaf waits for a network row (the only state the row pipeline
// sees: dedup, scan, alias, encode, cache, peer push).  NEED_STASH: the network has evaluated the leaf, its
// outputs are in View::stash_p / stash_v, and the reply has not run yet (a launch that paused at the sim cap).
enum { NEED_EMPTY = 0, NEED_ROW = 1, NEED_STASH = 2 };
// View::tres bit 0: the resume slot's reply is done and its fill was cut short by the cap (the tree is paused
// with sims left to start, whether or not a slot is pending); clear: the cycle goes on with the slot's reply
enum { RES_FILL = 1 };

__device__ __forceinline__ void set_err(const View &v, uint32_t f) { atomicOr(v.err, f); }

template <class G>
__device__ __forceinline__ size_t nbase(const View &v, int tree) {
  return (size_t)tree * (size_t)v.cap * G::APAD;
}

// The launch domain (View::dn, dpack): the tree of entry i < dn (-1: an empty list entry), and the pending
// slot of compact index c < dn * K (entry c / K, in-flight index c % K; -1 for an empty entry).  Compact
// order is slot order wherever the list ascends (the identity map; k_games_begin_ply's list).
__device__ __forceinline__ int dom_tree(const View &v, int i) { return v.dpack ? v.active[i] : i; }
__device__ __forceinline__ int dom_slot(const View &v, int c) {
  const int i = c / v.K, tree = dom_tree(v, i);
  return tree < 0 ? -1 : tree * v.K + (c - i * v.K);
}

// The game plays a move of its opening this ply (SelfPlayer.play_move, selfplayworker.py:221-224, on a given
// action): no search, no noise, no random number, no Move record.
__device__ __forceinline__ bool in_book(const View &v, int g) { return v.book_n && v.gply[g] < v.gbook[g]; }
