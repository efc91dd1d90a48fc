// spmcts.hip — MI355X (gfx950) batched self-play MCTS arena: kernels + C ABI.
//
// Replaces the per-game Python object tree of games/algos/mcts.py (MCNode /
// MCTreeSearch) and the episode loop of games/algos/selfplayworker.py
// (SelfPlayer) with one device-resident arena:
//
//   node store   one 32*APAD-byte record per "child block" (one per expansion):
//                n, vl, child (local block of the child's own children, -1 =
//                unexpanded), p, w, f64 flag per slot + the valid-children mask
//                (NodeRec).  A node = (block, slot); trees own disjoint block ranges.
//   trees        root node, root board (2 x u64 bitboards), root player, bump
//                allocator, Dirichlet noise, per-sim path scratch, RNG.
//   games        SelfPlayer state machine: board (policy frame), ply, swap_sides,
//                two trees, Move record buffers, export ring.
//
// Every simulation of every active tree runs in lock step:
//   k_select   one APAD-lane group per tree walks root -> leaf, scoring the A
//              children of each node lane-parallel in fp64 (bit-exact with the
//              reference's Python float arithmetic: fp-contract off), argmax via
//              in-group shuffles, jitter from Philox or the parity tape;
//              terminal leaves are backed up in place (no network call).
//   k_scan     orders pending leaves by tree id (deterministic rows).
//   k_encode   writes network input rows (planes or boards) for those leaves.
//   [network on the same stream — PyTorch ResNet or the table net]
//   k_expand   creates the leaf's child block from the priors, backs the value up.
//
// This file is the host side (allocation plan, launches, C ABI); the device code lies in headers,
// included below in this order:
//   arena_view.h    device view (View), NodeRec accessors, set_err, nbase
//   arena_rng.h     Philox / tape RNG
//   arena_select.h  resets and noise, k_compact, DPP reductions, k_select, the threaded sim and slot fill
//   arena_rows.h    leaf dedup, evaluation cache, peer push, k_scan_need, k_encode
//   arena_solver.h  score bounds kept in the nodes: the stamp of a new child block, the walk up the expansion's path
//   arena_expand.h  k_expand, threaded expand and select (one slot-cycle walk), _play, k_search_end, set_node, k_play_action
//   negamax.h       exact depth-limited negamax: the search core (host and device), its batch and arena kernels
//   solve.h         exact solver to the end of the game: alpha-beta with a transposition table, resumable launches
//   arena_games.h   game state machine (opening book plies included), the hard-coded players, k_root_stats_batch, export
//   arena_tree.h    reading the trees below the root: k_tree_pv (principal variations), k_tree_export (subtrees),
//                   k_tree_bounds (what a tree proves: bounds on the exact score)
//   arena_proof.h   playing what a tree has proved: k_proof_verdict (the moves the move choice may take), k_proof_stop
//   records.h       game records (move lists) to the positions before their moves: spmcts_log_positions and its host twin
//   arena_misc.h    k_env_step, k_table_net, k_copy_probe, the init kernels
//   arena_league.h  league routing: a step's rows partitioned by their tree's network, and back
//
// Compile: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see Makefile).
#include <hip/hip_runtime.h>
#include <rocrand/rocrand_normal.h>
#include <rocrand/rocrand_philox4x32_10.h>
#include <rocrand/rocrand_uniform.h>

#include "philox.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "board.h"
#include "spmcts.h"

#pragma clang fp contract(off)

using namespace spm;

// ----------------------------------------------------------------------------
// error reporting
// ----------------------------------------------------------------------------
static thread_local std::string g_last_error;

static int fail(int code, const std::string &msg) {
  g_last_error = msg;
  return code;
}

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess)                                                                      \
      return fail(-(int)_e - 1000, std::string(#expr) + ": " + hipGetErrorString(_e));        \
  } while (0)

#define TRY(call)                          \
  do {                                     \
    if (const int _rc = (call)) return _rc; \
  } while (0)

// device code, in definition order (see the list at the top of this file)
#include "arena_view.h"
#include "arena_rng.h"
#include "arena_select.h"
#include "arena_rows.h"
#include "arena_solver.h"
#include "arena_expand.h"
#include "negamax.h"
#include "solve.h"
#include "arena_games.h"
#include "arena_tree.h"
#include "arena_proof.h"
#include "records.h"
#include "arena_misc.h"
#include "arena_league.h"

// ----------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------
struct spmcts_arena {
  spmcts_config cfg;
  int device;
  int A, W, H, P, cells, maxd, maxm;
  View v;
  std::vector<void *> allocs;
  int n_active;  // active-set size for select / search_end
  // cross-lane dedup (spmcts_set_leaf_peer): a follower's leader, a leader's followers, and the events that
  // order the two streams (leader: ev_ins after its table of a step; follower: ev_rows after its rows,
  // ev_push after the leader's outputs reached its rows)
  spmcts_arena *peer = nullptr;
  std::vector<spmcts_arena *> followers;
  hipEvent_t ev_ins = nullptr, ev_rows = nullptr, ev_push = nullptr, ev_lead = nullptr;
  hipStream_t push_stream = nullptr;  // a follower's stream for k_peer_push (spmcts_peer_push)
  bool peer_step = false;  // the last launch_rows of this follower used the leader's table
  bool push_pending = false;  // the leader's stream has not yet waited for this follower's last push
  // evaluation cache (spmcts_set_eval_cache): its allocations, and whether the last launch_rows consulted it
  // (the next expand then runs k_cache_io)
  std::vector<void *> cache_allocs;
  bool cache_step = false;
  bool cache_shared_step = false;  // that launch used the leader's table (cache_view)
  const uint64_t *cache_tab = nullptr;  // the table that launch looked its keys up in
  // the packed launch domain (launch_rows): the active list is k_games_begin_ply's (ascending, one searching
  // tree per game at most), and the last launch_rows ran over it; that step's spmcts_peer_push and
  // spmcts_expand2 use the same domain
  bool games_list = false;
  bool packed_step = false;
  // league (spmcts_set_league): the trees' networks and the routing buffers (lg.n = 0: off), and whether a
  // route of the current step's rows has run (spmcts_league_unroute needs it)
  League lg = {};
  std::vector<int32_t> lg_seg;
  std::vector<void *> league_allocs;
  bool route_step = false;
  // negamax players (spmcts_set_tree_players): the score rows' allocation (View::nm_score), whether any tree is
  // of the kind, and the deepest horizon among them (sizes the launches of spmcts_games_end_ply)
  void *nm_alloc = nullptr;
  bool nm_on = false;
  int nm_depth = 0;
  // game log (spmcts_games_set_log): the log's and the finished-game ring's allocations, kept while the log is
  // off (View::glog null), and the log's address for turning it on again
  std::vector<void *> log_allocs;
  uint8_t *log_dev = nullptr;
  // proof-guided play (spmcts_set_proof_play): the View::pf_* arrays' allocations (flags, keep, lo, hi, stats, stop
  // counts), kept while the feature is off for every tree (View::pf_keep null)
  std::vector<void *> proof_allocs;
  // stored score bounds (spmcts_set_solver_search, arena_solver.h): the arena launches the SB = true kernels
  // (LAUNCH_SB below), the resets' among them
  bool sb = false;
  // solver-aware search (spmcts_set_solver_rules): the rule bits' and the statistics' allocations (View::sv_*)
  std::vector<void *> solver_allocs;
  // mirror symmetry (spmcts_set_symmetry): the arena launches the SYM = true kernels (LAUNCH_SYM, LAUNCH_SB_SYM
  // below); `begun`: a search or a game has started, after which the mode is fixed
  int sym = 0;
  bool begun = false;
};

static bool league_on(const spmcts_arena *h) { return h->lg.n > 0; }
static const char *const LEAGUE_EXCLUDES =
    "a league arena is single-network and runs without leaf dedup, evaluation cache and leaf peer";

// The launch domain of a step's per-slot kernels (View::dn, dpack): the active list, or every tree.
static void set_domain(const spmcts_arena *h, View &v, bool packed) {
  v.dn = packed ? h->n_active : v.T;
  v.dpack = packed ? 1 : 0;
}

// The evaluation-cache table of a launch: a follower lane (spmcts_set_leaf_peer) whose leader runs a cache of
// the same window, one generation apart at most, uses the leader's table -- one table for the GPU's lanes, so a
// position either lane evaluated serves both -- and inserts only the rows its own network evaluated; otherwise
// the arena's own table.
static bool cache_view(const spmcts_arena *h, View &v) {
  v.cshared = 0;
  const spmcts_arena *p = h->peer;
  if (!v.cwin || !p || p->v.cwin != v.cwin || !p->v.crec) return false;
  const int d = (int)(v.cgen - p->v.cgen);
  if (d < -1 || d > 1) return false;
  v.crec = p->v.crec;
  v.cmask = p->v.cmask;
  v.cshared = 1;
  return true;
}

// The one (game, width, height) switch, and the one list of instantiated boards: f(G{}) for the game type G,
// else -2 with UNSUPPORTED.  Every per-game kernel launch goes through it (LAUNCH below).
static const char *const UNSUPPORTED =
    "unsupported game/board size (instantiated: connect4 7x6, connect4 6x5, connect4 8x7, tictactoe 3x3)";
template <class F>
static int with_game(int game, int width, int height, F &&f) {
  if (game == SPMCTS_CONNECT4 && width == 7 && height == 6) return f(C4{});
  if (game == SPMCTS_CONNECT4 && width == 6 && height == 5) return f(C4_6x5{});
  if (game == SPMCTS_CONNECT4 && width == 8 && height == 7) return f(C4_8x7{});
  if (game == SPMCTS_TICTACTOE && width == 3 && height == 3) return f(TTT{});
  return fail(-2, UNSUPPORTED);
}

static int geometry(const spmcts_config *c, int *A, int *P, int *cells, int *maxd, int *maxm) {
  return with_game(c->game, c->width, c->height, [&](auto g) {
    using G = decltype(g);
    *A = G::A; *P = G::APAD; *cells = G::CELLS; *maxd = G::MAXD; *maxm = G::MAXM;
    return 0;
  });
}

// worst-case node blocks per tree per game: root pseudo block + root children + one
// block per expansion; a tree searches at most ceil(cells/2) times and play_action
// expands at most once per ply.
static int default_cap(const spmcts_config *c, int cells) {
  const long long it = std::max(1, c->iterations);
  const long long cap = 2 + ((cells + 1) / 2) * it + cells + 2;
  return (int)std::min<long long>(cap, 1 << 26);
}

struct Plan {
  size_t off = 0;
  std::vector<std::pair<void **, size_t>> items;
  template <class T>
  void add(T **p, size_t count) {
    items.push_back({(void **)p, sizeof(T) * std::max<size_t>(count, 1)});
  }
  size_t total() const {
    size_t t = 0;
    for (auto &it : items) t += (it.second + 255) & ~size_t(255);
    return t;
  }
};

// device address of a field of node i (host side; off = the field's NodeRec offset in units of P bytes)
static const char *node_field(const spmcts_arena *h, int off, int elt, size_t i) {
  const size_t P = h->P;
  return h->v.nodes + (i / P) * 32 * P + off * P + (i % P) * elt;
}

static void plan_arena(spmcts_arena *h, Plan &pl) {
  View &v = h->v;
  const size_t T = v.T, P = h->P, cap = v.cap, G = v.G;
  pl.add(&v.nodes, T * cap * 32 * P);  // 32 * P bytes per child block (NodeRec)
  pl.add(&v.root, T);
  pl.add(&v.rpos, T);
  pl.add(&v.rneg, T);
  pl.add(&v.rplayer, T);
  pl.add(&v.used, T);
  pl.add(&v.gc_list, v.gc ? T * cap : 1);
  pl.add(&v.gc_map, v.gc ? T * cap : 1);
  pl.add(&v.tstarted, T);
  pl.add(&v.noise, T * P);
  pl.add(&v.noise_on, T);
  const size_t NS = v.NS;  // pending slots
  pl.add(&v.pnode, NS * h->maxd);
  pl.add(&v.pn, NS * h->maxd);
  pl.add(&v.pw, NS * h->maxd);
  pl.add(&v.plen, NS);
  pl.add(&v.leaf, NS);
  pl.add(&v.leaf_n, NS);
  pl.add(&v.leaf_w, NS);
  pl.add(&v.lpos, NS);
  pl.add(&v.lneg, NS);
  pl.add(&v.lmover, NS);
  pl.add(&v.need, NS);
  pl.add(&v.tres, T);
  pl.add(&v.stash_p, v.K > 1 ? NS * P : 1);  // the sim cap's stash: APAD probs and one value per pending slot
  pl.add(&v.stash_v, v.K > 1 ? NS : 1);
  pl.add(&v.rng, T);
  pl.add((int64_t **)&v.tape_end, T);
  pl.add(&v.tape_cur, T);
  pl.add(&v.cnt, T * C_NCNT);
  pl.add(&v.active, std::max(T, G));
  pl.add(&v.row_tree, NS);
  pl.add(&v.srow, NS);
  pl.add(&v.row_count, 4);
  pl.add(&v.crow, NS + SCAN_BATCH);
  {
    size_t tab = 1;
    while (tab < 2 * NS) tab <<= 1;
    v.dmask = (int)(tab - 1);
    pl.add(&v.dtab, v.K > 1 ? tab : 1);
    pl.add(&v.dent, v.K > 1 ? NS : 1);
    pl.add(&v.down, v.K > 1 ? NS : 1);
    pl.add(&v.okey, v.K > 1 ? 2 * NS : 1);
    pl.add(&v.xpeer, v.K > 1 ? NS : 1);
  }
  pl.add(&v.root_prior, 32);  // [net][16]
  pl.add(&v.err, 4);
  pl.add(&v.gpos, G);
  pl.add(&v.gneg, G);
  pl.add(&v.gply, G);
  pl.add(&v.gswap, G);
  pl.add(&v.gstate, G);
  pl.add(&v.gresult, G);
  pl.add(&v.gid, G);
  pl.add(&v.mv_state, 2 * G * h->maxm * h->cells);
  pl.add(&v.mv_probs, 2 * G * h->maxm * h->A);
  pl.add(&v.mv_q, 2 * G * h->maxm);
  pl.add(&v.mv_qf64, 2 * G * h->maxm);
  pl.add(&v.mv_count, 2 * G);
  const size_t X = std::max<size_t>(64, 4 * G * h->maxm);
  v.ex_cap = (int32_t)X;
  pl.add(&v.ex_state, X * h->cells);
  pl.add(&v.ex_probs, X * h->A);
  pl.add(&v.ex_q, X);
  pl.add(&v.ex_qf64, X);
  pl.add(&v.ex_z, X);
  pl.add(&v.ex_game, X);
  pl.add(&v.ex_count, 4);
  pl.add(&v.gcnt, 16);
  pl.add(&v.gscratch, 2 * G + 8);
  pl.add(&v.tnet, T);
  pl.add(&v.tkind, T);
  pl.add(&v.budget, T);
  pl.add(&v.talpha, T);
  pl.add(&v.tstrong, T);
  pl.add(&v.tK, T);
  // the opening book at its limits (spmcts_games_set_openings): BOOK_MAX_OPENINGS sequences shorter than the board
  pl.add(&v.book_moves, G ? (size_t)BOOK_MAX_OPENINGS * (h->cells - 1) : 1);
  pl.add(&v.book_lens, G ? (size_t)BOOK_MAX_OPENINGS : 1);
  pl.add(&v.gopen, G);
  pl.add(&v.gbook, G);
}

static int setup_view(spmcts_arena *h, const spmcts_config *cfg) {
  int A, P, cells, maxd, maxm;
  if (geometry(cfg, &A, &P, &cells, &maxd, &maxm)) return -2;
  h->cfg = *cfg;
  h->A = A;
  h->P = P;
  h->cells = cells;
  h->maxd = maxd;
  h->maxm = maxm;
  h->W = cfg->width;
  h->H = cfg->height;
  View &v = h->v;
  memset(&v, 0, sizeof(v));
  v.T = cfg->n_trees;
  v.G = cfg->n_games;
  v.A = A;
  v.cap = cfg->blocks_per_tree > 0 ? cfg->blocks_per_tree : default_cap(cfg, cells);
  v.gc = v.cap < default_cap(cfg, cells) ? 1 : 0;  // below the worst case: recycle subtrees (k_compact)
  v.cpuct = cfg->cpuct;
  v.x = cfg->x_noise;
  v.alpha = cfg->alpha;
  v.strong = cfg->strong_play;
  v.evaluate = cfg->evaluate;
  v.rng_mode = cfg->rng_mode;
  v.leaf_format = cfg->leaf_format;
  v.leaf_layout = cfg->leaf_layout;
  v.K = std::max(1, cfg->search_threads);
  if (v.K > P) return fail(-3, "search_threads must not exceed the lane group (8 for the connect4 boards, 16 for tictactoe)");
  v.iters = std::max(1, cfg->iterations);
  v.NS = v.T * v.K;
  v.simcap = v.K > 1 ? SIM_CAP_PER_K * v.K : 0;  // on by default (spmcts_set_sim_cap)
  v.dn = v.T;  // full width (set_domain)
  v.dpack = 0;
  v.seg1 = v.NS;
  v.record = 1;
  v.sim = 0;
  if (v.T <= 0) return fail(-3, "n_trees must be > 0");
  if (v.G < 0 || 2 * (long long)v.G > v.T) return fail(-3, "games mode needs n_trees >= 2 * n_games");
  if (v.T > (1 << 24)) return fail(-3, "too many trees");
  if (v.K > 64 || (long long)v.T * v.K > (1 << 24)) return fail(-3, "search_threads too large");
  if (v.cap < 4) return fail(-3, "blocks_per_tree too small");
  if ((long long)v.cap * P >= (1ll << 31)) return fail(-3, "blocks_per_tree too large");
  return 0;
}

// The one launch path: kernel k over n elements (threads) in blocks of B, at least one block, on stream s.
// enqueue() only launches; launch() also returns the launch status.
template <class... P, class... A>
static void enqueue(void (*k)(P...), long long n, int B, hipStream_t s, const A &...a) {
  const int blocks = (int)std::max<long long>(1, (n + B - 1) / B);
  hipLaunchKernelGGL(k, dim3(blocks), dim3(B), 0, s, static_cast<P>(a)...);
}
template <class... P, class... A>
static int launch(void (*k)(P...), long long n, int B, hipStream_t s, const A &...a) {
  enqueue(k, n, B, s, a...);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(-(int)e - 1000, std::string("launch: ") + hipGetErrorString(e));
  return 0;
}
// launch() of a kernel template on the arena's game type: k<G>, G from with_game
#define LAUNCH(h, k, n, B, s, ...) \
  with_game((h)->cfg.game, (h)->W, (h)->H, [&](auto game_) { return launch(k<decltype(game_)>, n, B, s, __VA_ARGS__); })
// the same for a kernel template <class G, bool SB>: the stored-bounds instantiation once the arena keeps them
#define LAUNCH_SB(h, k, n, B, s, ...)                                                                       \
  with_game((h)->cfg.game, (h)->W, (h)->H, [&](auto game_) {                                                \
    return (h)->sb ? launch(k<decltype(game_), true>, n, B, s, __VA_ARGS__)                                 \
                   : launch(k<decltype(game_), false>, n, B, s, __VA_ARGS__);                               \
  })
// the same for the kernels that take a leaf key or read a row (template <class G, bool SYM> and
// <class G, bool SB, bool SYM>): the canonical-form instantiation once the arena's symmetry mode is on
#define LAUNCH_SYM(h, k, n, B, s, ...)                                                                      \
  with_game((h)->cfg.game, (h)->W, (h)->H, [&](auto game_) {                                                \
    return (h)->sym ? launch(k<decltype(game_), true>, n, B, s, __VA_ARGS__)                                \
                    : launch(k<decltype(game_), false>, n, B, s, __VA_ARGS__);                              \
  })
#define LAUNCH_SB_SYM(h, k, n, B, s, ...)                                                                   \
  with_game((h)->cfg.game, (h)->W, (h)->H, [&](auto game_) {                                                \
    using G_ = decltype(game_);                                                                             \
    if ((h)->sym)                                                                                           \
      return (h)->sb ? launch(k<G_, true, true>, n, B, s, __VA_ARGS__) : launch(k<G_, false, true>, n, B, s, __VA_ARGS__); \
    return (h)->sb ? launch(k<G_, true, false>, n, B, s, __VA_ARGS__) : launch(k<G_, false, false>, n, B, s, __VA_ARGS__); \
  })

// ---- negamax launches --------------------------------------------------------
// A launch's worst-case node bound, positions * sum_{k = 1 .. D} A^k, stays below NM_LAUNCH_NODES: a batch (and
// an arena's games) is split into launches of nm_launch_positions positions.  Measured on one MI355X (DESIGN.md
// §4 "Exact depth-limited negamax", profiles/negamax/): 8.9e10 nodes/s at depth 6 (4,096 positions in one
// launch), 2.7e10 nodes/s at depth 8 with launches of 594 positions (4.0e9: 455 waves, under half of the chip's
// 1,024 SIMDs).  At the lower of the two rates a launch of 8.0e9 nodes, the bound's worst case, takes 0.3 s;
// the launches of a depth-8 batch then hold 1,188 positions (910 waves), and the same batch measured 4.8e10
// nodes/s: 0.13 s per launch, 0.17 s for one at the bound.
static const double NM_LAUNCH_NODES = 8.0e9;

static long long nm_launch_positions(int A, int depth) {
  double bound = 0, term = 1;
  for (int k = 1; k <= depth; ++k) {
    term *= A;
    bound += term;
  }
  const double n = NM_LAUNCH_NODES / bound;
  return n < 1 ? 1 : (n > (double)(1 << 24) ? (1 << 24) : (long long)n);
}

// k over positions [0, n) in launches of at most `per` positions: f(first position, count) launches one
template <class G, class F>
static int nm_launches(long long n, int depth, F &&f) {
  const long long per = nm_launch_positions(G::A, depth);
  for (long long p0 = 0; p0 < n; p0 += per) TRY(f(p0, (int)std::min(per, n - p0)));
  return 0;
}

static int negamax_games(spmcts_arena *h, hipStream_t s) {
  return with_game(h->cfg.game, h->W, h->H, [&](auto g) {
    using G = decltype(g);
    return nm_launches<G>(h->v.G, h->nm_depth, [&](long long g0, int n) {
      return launch(k_negamax_games<G>, ((long long)n + NmGrid<G>::PPB - 1) / NmGrid<G>::PPB * NM_THREADS, NM_THREADS, s,
                    h->v, (int)g0, n);
    });
  });
}

// ---- solver launches -----------------------------------------------------------
// A launch of spmcts_solve_batch gives every running item at most SV_LAUNCH_STEPS steps of sv_iter, each at most
// one move (csrc/solve.h); an item that is not through parks and the next launch resumes it.
// Measured on one MI355X (DESIGN.md §4 "Exact solver to the end of the game", profiles/solve/): 4,096 positions of
// 7x6 after 20 random plies, 1.33e9 moves in 1.476 s = 9.0e8 nodes/s over 17 launches of 65,536 steps, 87 ms per
// launch on average (the full first launches of 200,704 lanes and the tail's few lanes are in that mean; they were
// not timed apart): a lane takes about 7.5e5 steps/s.  At that rate a launch of 2^16 steps takes 0.09 s, and stays
// under a second with lanes ten times slower.
static const uint32_t SV_LAUNCH_STEPS = 1u << 16;
static thread_local int g_solve_launches = 0;

static int sv_table_check(const void *table, uint64_t entries) {
  if (!table) return fail(-1, "null argument");
  if (entries < (1ull << SV_MIN_TABLE_BITS) || (entries & (entries - 1)))
    return fail(-3, "solve table: a power-of-two number of entries, at least 2^16");
  return 0;
}

extern "C" {

int spmcts_version(void) { return 1; }

const char *spmcts_last_error(void) { return g_last_error.c_str(); }

int spmcts_arena_bytes(const spmcts_config *cfg, uint64_t *bytes_out) {
  spmcts_arena tmp;
  if (setup_view(&tmp, cfg)) return -2;
  Plan pl;
  plan_arena(&tmp, pl);
  *bytes_out = pl.total();
  return 0;
}

int spmcts_arena_create(const spmcts_config *cfg, int device, spmcts_arena **out) {
  if (!cfg || !out) return fail(-1, "null argument");
  spmcts_arena *h = new spmcts_arena();
  h->device = device;
  h->n_active = 0;
  int rc = setup_view(h, cfg);
  if (rc) {
    delete h;
    return rc;
  }
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) {
    delete h;
    return fail(-1000 - (int)e, std::string("hipSetDevice: ") + hipGetErrorString(e));
  }
  Plan pl;
  plan_arena(h, pl);
  for (auto &it : pl.items) {
    void *p = nullptr;
    e = hipMalloc(&p, it.second);
    if (e != hipSuccess) {
      for (void *q : h->allocs) (void)hipFree(q);
      delete h;
      return fail(-1000 - (int)e, std::string("hipMalloc: ") + hipGetErrorString(e));
    }
    h->allocs.push_back(p);
    *it.first = p;
  }
  if (h->v.K > 1) (void)hipMemset(h->v.dtab, 0, sizeof(uint64_t) * ((size_t)h->v.dmask + 1));  // generation 0
  (void)hipMemset(h->v.used, 0, sizeof(int32_t) * (size_t)h->v.T);  // no blocks before a reset (spmcts_set_solver_search reads it)
  enqueue(k_rng_init, h->v.T, 256, nullptr, h->v, cfg->seed, cfg->subsequence0);  // (a failed launch surfaces at the synchronize below)
  enqueue(k_games_init, h->v.G, 256, nullptr, h->v);
  // default root prior: uniform (replaced by spmcts_set_root_prior)
  std::vector<float> pri(32, 0.f);
  for (int j = 0; j < h->A; ++j) pri[j] = pri[16 + j] = 1.0f / h->A;
  e = hipMemcpy(h->v.root_prior, pri.data(), 32 * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    for (void *q : h->allocs) (void)hipFree(q);
    delete h;
    return fail(-1000 - (int)e, std::string("arena init: ") + hipGetErrorString(e));
  }
  *out = h;
  return 0;
}

int spmcts_arena_destroy(spmcts_arena *h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  (void)spmcts_set_leaf_peer(h, nullptr);
  for (spmcts_arena *f : h->followers) {  // a destroyed leader leaves its followers lane-local
    f->peer = nullptr;
    f->peer_step = false;
  }
  for (hipEvent_t e : {h->ev_ins, h->ev_rows, h->ev_push, h->ev_lead})
    if (e) (void)hipEventDestroy(e);
  if (h->push_stream) (void)hipStreamDestroy(h->push_stream);
  for (void *p : h->allocs) (void)hipFree(p);
  for (void *p : h->cache_allocs) (void)hipFree(p);
  for (void *p : h->league_allocs) (void)hipFree(p);
  if (h->nm_alloc) (void)hipFree(h->nm_alloc);
  for (void *p : h->log_allocs) (void)hipFree(p);
  for (void *p : h->proof_allocs) (void)hipFree(p);
  for (void *p : h->solver_allocs) (void)hipFree(p);
  delete h;
  return 0;
}

int spmcts_set_leaf_peer(spmcts_arena *h, spmcts_arena *leader) {
  if (!h) return fail(-1, "null arena");
  if (h->peer) {
    auto &f = h->peer->followers;
    f.erase(std::remove(f.begin(), f.end(), h), f.end());
    h->peer = nullptr;
  }
  h->peer_step = false;
  h->push_pending = false;
  if (!leader) return 0;
  if (leader == h) return fail(-3, "an arena cannot be its own leader");
  if (league_on(h) || league_on(leader)) return fail(-3, LEAGUE_EXCLUDES);
  if (leader->peer || !h->followers.empty()) return fail(-3, "one level of lanes: a leader cannot follow");
  if (leader->cfg.game != h->cfg.game || leader->device != h->device)
    return fail(-3, "leader and follower must play the same game on the same device");
  if (h->v.K < 2 || leader->v.K != h->v.K) return fail(-3, "cross-lane dedup needs equal search_threads > 1");
  if (h->v.seg1 < h->v.NS || leader->v.seg1 < leader->v.NS) return fail(-3, "cross-lane dedup: single-network arenas");
  if (leader->sym != h->sym) return fail(-3, "leader and follower must run the same symmetry mode (spmcts_set_symmetry)");
  for (hipEvent_t *e : {&leader->ev_ins, &h->ev_rows, &h->ev_push, &h->ev_lead})
    if (!*e) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
  leader->followers.push_back(h);
  h->peer = leader;
  return 0;
}

int spmcts_peer_push(spmcts_arena *h, float *probs_dev, float *values_dev, const float *leader_probs_dev,
                     const float *leader_values_dev, spmcts_stream stream, spmcts_stream leader_stream) {
  if (!h) return fail(-1, "null arena");
  if (!h->peer_step) return 0;
  if (!probs_dev || !values_dev || !leader_probs_dev || !leader_values_dev) return fail(-1, "null argument");
  const hipStream_t s = (hipStream_t)stream, ls = (hipStream_t)leader_stream;
  // on the follower's own push stream, once the leader's outputs of this step (everything the caller has
  // issued on leader_stream: its heads) and our rows are there; the leader's stream goes on at once (its
  // expand does not wait) and waits for the push only before it next rewrites its table, keys or outputs
  // (launch_rows: its next step's rows)
  if (!h->push_stream) HIP_TRY(hipStreamCreateWithFlags(&h->push_stream, hipStreamNonBlocking));
  HIP_TRY(hipEventRecord(h->ev_lead, ls));
  HIP_TRY(hipStreamWaitEvent(h->push_stream, h->ev_lead, 0));
  HIP_TRY(hipStreamWaitEvent(h->push_stream, h->ev_rows, 0));
  View v = h->v;
  set_domain(h, v, h->packed_step);  // the domain whose k_dedup_owner_peer wrote this step's down / xpeer
  const int rc = launch(k_peer_push, (long long)v.dn * v.K, 256, h->push_stream, v, h->peer->v.srow, leader_probs_dev,
                        leader_values_dev, probs_dev, values_dev);
  HIP_TRY(hipEventRecord(h->ev_push, h->push_stream));
  h->push_pending = true;
  HIP_TRY(hipStreamWaitEvent(s, h->ev_push, 0));
  h->peer_step = false;
  return rc;
}

int spmcts_arena_geometry(const spmcts_arena *h, int32_t *A, int32_t *W, int32_t *H, int32_t *bpt, int32_t *nt,
                          int32_t *ng) {
  if (!h) return fail(-1, "null arena");
  if (A) *A = h->A;
  if (W) *W = h->W;
  if (H) *H = h->H;
  if (bpt) *bpt = h->v.cap;
  if (nt) *nt = h->v.T;
  if (ng) *ng = h->v.G;
  return 0;
}

int spmcts_set_root_prior(spmcts_arena *h, const float *probs_dev, spmcts_stream stream) {
  if (!h || !probs_dev) return fail(-1, "null argument");
  HIP_TRY(hipMemcpyAsync(h->v.root_prior, probs_dev, sizeof(float) * h->A, hipMemcpyDeviceToDevice,
                         (hipStream_t)stream));
  return 0;
}

int spmcts_set_tape(spmcts_arena *h, const double *tape_dev, const int64_t *offsets_dev, spmcts_stream stream) {
  if (!h || !offsets_dev) return fail(-1, "null argument");
  if (h->cfg.rng_mode != SPMCTS_RNG_TAPE) return fail(-4, "arena is not in tape RNG mode");
  h->v.tape = tape_dev;
  return launch(k_set_tape, h->v.T, 256, (hipStream_t)stream, h->v, offsets_dev);
}

int spmcts_tree_reset(spmcts_arena *h, const int32_t *trees_dev, const int8_t *root_player_dev,
                      const float *priors_dev, int32_t n, spmcts_stream stream) {
  if (!h) return fail(-1, "null arena");
  if (n <= 0) return 0;
  return LAUNCH_SB(h, k_tree_reset, n, 128, (hipStream_t)stream, h->v, trees_dev, root_player_dev, priors_dev, n);
}

int spmcts_search_begin(spmcts_arena *h, const int32_t *trees_dev, int32_t n, spmcts_stream stream) {
  if (!h) return fail(-1, "null arena");
  if (n > std::max(h->v.T, h->v.G)) return fail(-3, "too many active trees");
  h->n_active = n;
  h->begun = true;
  h->games_list = false;  // a caller's list: any order, so its steps launch at full width (launch_rows)
  h->v.sim = 0;
  if (h->v.cwin) ++h->v.cgen;  // a new evaluation-cache generation per search
  if (n <= 0) return 0;
  TRY(LAUNCH(h, k_search_begin, n, 128, (hipStream_t)stream, h->v, trees_dev, n));
  if (h->v.gc) TRY(LAUNCH_SB(h, k_compact, 256ll * n, 256, (hipStream_t)stream, h->v, n));  // one block per tree
  return 0;
}

// cross-lane dedup is live for this step: a follower whose leader and itself dedup (spmcts_set_leaf_peer)
static bool peer_live(const spmcts_arena *h) { return h->peer && h->v.dedup && h->peer->v.dedup; }

// `sim_step`: a simulation step's rows (spmcts_select / spmcts_leaf_rows), where a follower lane looks its
// owner keys up in its leader's table; the end-of-ply expansions (spmcts_play_action, games_end_ply) stay
// lane-local
//
// Launch domain.  A simulation step of a games-mode ply (the active list is k_games_begin_ply's) runs its
// per-slot kernels -- dedup, scan, alias, encode here, then k_peer_push, k_cache_io and k_expand_vl
// (spmcts_peer_push, spmcts_expand2) -- over the pending slots of the listed trees only: one tree per game
// searches, so half of the T = 2 G trees' slots.  This rests on one invariant: in such a step no tree outside
// the list has a pending slot (need set).  need is set in two places.  fill_slot_vl / k_select set it for the
// tree they run on, and they run on listed trees only (k_select_vl, k_select: entries of `active`; k_expand_vl's
// refill: a tree with started < limit, which draw_noise arms for listed trees alone, and which the domain
// restricts to the list anyway).  set_node (k_games_end_ply, k_play_action) sets it for slot 0 of trees that do
// not search, and the launch_rows that follows it is never a simulation step: it and its expand run at full
// width and clear those slots before the next ply's list is written.  A listed tree's own slots are all
// cleared by the last step's expand: without the sim cap every pending slot of a domain tree is completed in
// each step's expand; with it a paused tree carries pending and stashed slots (NEED_STASH: evaluated, no row --
// every kernel here takes only NEED_ROW slots) from step to step, but never past the search's last step
// (arena_select.h "sim cap": cap >= 2 K; k_games_end_ply raises SPMCTS_ERR_STATE otherwise), so nothing
// carries over when the other tree of the game searches next.  The list ascends (active[g] = 2 g + mover), so
// compact order is slot order and k_scan_need numbers the same rows as at full width.  A caller's list
// (spmcts_search_begin) may be in any order: those searches, and every end-of-ply launch, stay at full width.
// Flags written per step (down, xpeer, xc, dent, srow) are written for the domain's slots only, so an idle
// tree's slots keep those of its last search.  Every reader either tests need first (k_cache_io, k_dedup_alias,
// k_expand_vl), runs on the writer's domain in the same step (k_peer_push: down, xpeer), or reads a leader's
// slot found in the leader's table of this generation, which the leader's k_dedup_insert / k_dedup_owner wrote
// this step (k_dedup_owner_peer: pdown, pkey).  k_scan_need reads no per-slot flag: the owner kernel of its
// launch writes the row flag of every compact index of the domain (crow), empty entries included.  The
// full-width passes rewrite down for every slot.
static int launch_rows(spmcts_arena *h, void *leaves_dev, int32_t *leaf_count_dev, hipStream_t s, bool sim_step) {
  h->peer_step = false;
  h->begun = true;
  h->route_step = false;  // new rows: the last route's map is stale
  h->packed_step = sim_step && h->games_list;
  for (spmcts_arena *f : h->followers)  // a leader rewrites its table, keys and (later) outputs only after the pushes
    if (f->push_pending) {
      HIP_TRY(hipStreamWaitEvent(s, f->ev_push, 0));
      f->push_pending = false;
    }
  View v = h->v;
  set_domain(h, v, h->packed_step);
  const long long slots = (long long)v.dn * v.K;  // the domain's pending slots: one thread each
  v.peer_on = 0;
  // the evaluation cache is live in leaf-dedup launches (spmcts_set_eval_cache)
  h->cache_step = v.cwin > 0 && v.dedup;
  if (!h->cache_step) v.cwin = 0;
  h->cache_shared_step = h->cache_step && cache_view(h, v);
  h->cache_tab = h->cache_step ? v.crec : nullptr;
  if (v.dedup) {
    if (++h->v.dgen == 0) ++h->v.dgen;  // generation 0 = the zeroed table
    v.dgen = h->v.dgen;
    v.lead = h->followers.empty() ? 0 : 1;
    TRY(LAUNCH_SYM(h, k_dedup_insert, slots, 256, s, v));
    if (sim_step && peer_live(h)) {
      // the leader's table and keys of this step are complete (its ev_ins), and stay so until this step's
      // rows are numbered (the leader's stream waits for our ev_rows before it moves on: spmcts_peer_push)
      const spmcts_arena *p = h->peer;
      HIP_TRY(hipStreamWaitEvent(s, p->ev_ins, 0));
      v.peer_on = 1;
      TRY(LAUNCH_SYM(h, k_dedup_owner_peer, slots, 256, s, v, p->v.dtab, p->v.okey, p->v.down, p->v.dmask, p->v.dgen));
    } else {
      TRY(LAUNCH_SYM(h, k_dedup_owner, slots, 256, s, v));
    }
    if (v.lead) HIP_TRY(hipEventRecord(h->ev_ins, s));
  } else {
    TRY(LAUNCH_SYM(h, k_dedup_owner, slots, 256, s, v));  // no dedup: every pending slot's row flag (crow)
  }
  TRY(launch(k_scan_need, SCAN_THREADS, SCAN_THREADS, s, v, leaf_count_dev));  // one block
  if (v.dedup) TRY(launch(k_dedup_alias, slots, 256, s, v));
  if (v.peer_on) {
    HIP_TRY(hipEventRecord(h->ev_rows, s));
    h->peer_step = true;  // spmcts_peer_push brings the leader's outputs before the expand
  }
  if (leaves_dev) TRY(LAUNCH_SYM(h, k_encode, slots * h->cells, 256, s, v, leaves_dev));
  return 0;
}

int spmcts_select_tree(spmcts_arena *h, spmcts_stream stream) {
  if (!h) return fail(-1, "null arena");
  hipStream_t s = (hipStream_t)stream;
  const int n = h->n_active;
  int rc = 0;
  if (n > 0) {  // one P-lane group per tree, 64 / P groups per block
    const long long lanes = (long long)n * h->P;
    View dv = h->v;  // k_select_vl walks the active list as a packed domain
    set_domain(h, dv, true);
    rc = h->v.K > 1 ? LAUNCH_SB(h, k_select_vl, lanes, SELECT_THREADS, s, dv) : LAUNCH_SB(h, k_select, lanes, 64, s, h->v, n);
  }
  h->v.sim += h->v.K;
  return rc;
}

int spmcts_leaf_rows(spmcts_arena *h, void *leaves_dev, int32_t *leaf_count_dev, spmcts_stream stream) {
  if (!h) return fail(-1, "null arena");
  return launch_rows(h, leaves_dev, leaf_count_dev, (hipStream_t)stream, true);
}

int spmcts_select(spmcts_arena *h, void *leaves_dev, int32_t *leaf_count_dev, spmcts_stream stream) {
  const int rc = spmcts_select_tree(h, stream);
  if (rc) return rc;
  return spmcts_leaf_rows(h, leaves_dev, leaf_count_dev, stream);
}

int spmcts_expand2(spmcts_arena *h, const float *probs0_dev, const float *values0_dev, const float *probs1_dev,
                   const float *values1_dev, spmcts_stream stream) {
  if (!h) return fail(-1, "null arena");
  if (h->peer_step) return fail(-4, "a follower lane's simulation step needs spmcts_peer_push before its expand");
  if (h->v.seg1 < h->v.NS && (!probs1_dev || !values1_dev))
    return fail(-1, "two-network arena needs network-1 outputs");
  View dv = h->v;  // the domain of the step's rows (launch_rows)
  set_domain(h, dv, h->packed_step);
  if (h->cache_step) {  // the rows of this step consulted the evaluation cache: fills and inserts first
    View v = dv;
    if (h->cache_shared_step) cache_view(h, v);
    if (v.crec != h->cache_tab) return fail(-4, "the evaluation cache table changed between a step's rows and its expand");
    TRY(LAUNCH_SYM(h, k_cache_io, (long long)v.dn * v.K, 256, (hipStream_t)stream, v, (float *)probs0_dev,
               (float *)values0_dev, (float *)probs1_dev, (float *)values1_dev));
    h->cache_step = false;
  }
  if (h->v.K > 1)  // one P-lane group per tree of the domain
    return LAUNCH_SB_SYM(h, k_expand_vl, (long long)dv.dn * h->P, EXPAND_THREADS, (hipStream_t)stream, dv, probs0_dev,
                     values0_dev, probs1_dev, values1_dev);
  const long long lanes = (long long)h->v.T * h->P;  // one P-lane group per row
  return LAUNCH_SB_SYM(h, k_expand, lanes, 64, (hipStream_t)stream, h->v, probs0_dev, values0_dev, probs1_dev, values1_dev);
}

int spmcts_expand(spmcts_arena *h, const float *probs_dev, const float *values_dev, spmcts_stream stream) {
  if (!h) return fail(-1, "null arena");
  // one buffer indexed by row: network-1 rows (if any) sit at their own row index
  const size_t s1 = (size_t)h->v.seg1;
  const bool dual = h->v.seg1 < h->v.NS;
  return spmcts_expand2(h, probs_dev, values_dev, dual ? probs_dev + s1 * h->A : nullptr,
                        dual ? values_dev + s1 : nullptr, stream);
}

int spmcts_set_tree_players(spmcts_arena *h, const uint8_t *nets, const uint8_t *kinds, const int32_t *budgets) {
  if (!h) return fail(-1, "null arena");
  const int T = h->v.T;
  std::vector<uint8_t> nt(T, 0), kd(T, SPMCTS_PLAYER_MCTS);
  std::vector<int32_t> bd(T, 0x7fffffff);
  int n0 = 0, nm_depth = 0;
  const int nm_cap = with_game(h->cfg.game, h->W, h->H, [](auto g) { return (int)NmCap<decltype(g)>::PLAYER; });
  for (int t = 0; t < T; ++t) {
    if (nets) nt[t] = nets[t] ? 1 : 0;
    if (kinds) {
      if (kinds[t] > SPMCTS_PLAYER_NEGAMAX) return fail(-3, "unknown player kind");
      kd[t] = kinds[t];
    }
    if (budgets) bd[t] = budgets[t] < 0 ? 0x7fffffff : budgets[t];
    if (kd[t] == SPMCTS_PLAYER_NEGAMAX) {  // its budget is its horizon
      if (!budgets || budgets[t] < 1 || budgets[t] > nm_cap)
        return fail(-3, "a negamax player's budget is its depth: 1 .. " + std::to_string(nm_cap));
      nm_depth = std::max(nm_depth, budgets[t]);
    }
    n0 += nt[t] ? 0 : 1;
  }
  if (league_on(h) && n0 < T) return fail(-3, LEAGUE_EXCLUDES);
  HIP_TRY(hipDeviceSynchronize());
  if (nm_depth && !h->nm_alloc) {  // the first tree of the kind: its arena gets the score rows
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMalloc(&h->nm_alloc, (size_t)T * h->A));
    HIP_TRY(hipMemset(h->nm_alloc, 0, (size_t)T * h->A));
    h->v.nm_score = (int8_t *)h->nm_alloc;
  }
  h->nm_on = nm_depth > 0;
  h->nm_depth = nm_depth;
  HIP_TRY(hipMemcpy(h->v.tnet, nt.data(), T, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->v.tkind, kd.data(), T, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->v.budget, bd.data(), 4 * (size_t)T, hipMemcpyHostToDevice));
  h->v.seg1 = n0 * h->v.K;  // network-0 trees never have more than n0 * K pending leaves
  return 0;
}

int spmcts_set_tree_search(spmcts_arena *h, const double *alpha, const uint8_t *strong_play,
                           const int32_t *search_threads) {
  if (!h) return fail(-1, "null arena");
  const int T = h->v.T;
  if (alpha) {
    for (int t = 0; t < T; ++t)
      if (!(alpha[t] > 0.0)) return fail(-3, "alpha must be > 0");
  }
  if (search_threads) {
    for (int t = 0; t < T; ++t)
      if (search_threads[t] < 1 || search_threads[t] > h->v.K)
        return fail(-3, "per-tree search_threads must be in [1, the arena's search_threads]");
  }
  HIP_TRY(hipDeviceSynchronize());
  if (alpha) HIP_TRY(hipMemcpy(h->v.talpha, alpha, sizeof(double) * (size_t)T, hipMemcpyHostToDevice));
  if (strong_play) {
    std::vector<uint8_t> st(T);
    for (int t = 0; t < T; ++t) st[t] = strong_play[t] ? 1 : 0;
    HIP_TRY(hipMemcpy(h->v.tstrong, st.data(), (size_t)T, hipMemcpyHostToDevice));
  }
  if (search_threads) HIP_TRY(hipMemcpy(h->v.tK, search_threads, 4 * (size_t)T, hipMemcpyHostToDevice));
  return 0;
}

int spmcts_arena_segments(const spmcts_arena *h, int32_t *seg1) {
  if (!h) return fail(-1, "null arena");
  if (seg1) *seg1 = h->v.seg1;
  return 0;
}

int spmcts_set_root_prior_net(spmcts_arena *h, int32_t net, const float *probs_dev, spmcts_stream stream) {
  if (!h || !probs_dev) return fail(-1, "null argument");
  if (net < 0 || net > 1) return fail(-3, "network index must be 0 or 1");
  HIP_TRY(hipMemcpyAsync(h->v.root_prior + 16 * net, probs_dev, sizeof(float) * h->A, hipMemcpyDeviceToDevice,
                         (hipStream_t)stream));
  return 0;
}

int spmcts_set_leaf_dedup(spmcts_arena *h, int32_t on) {
  if (!h) return fail(-1, "null arena");
  if (on && league_on(h)) return fail(-3, LEAGUE_EXCLUDES);
  h->v.dedup = (on && h->v.K > 1) ? 1 : 0;  // K = 1 keeps one row per tree (k_expand walks rows)
  return 0;
}

int spmcts_set_sim_cap(spmcts_arena *h, int32_t cap) {
  if (!h) return fail(-1, "null arena");
  // below 2 K a search could need more launches than ceil(iterations / K) + 1 (arena_select.h "sim cap")
  if (cap < 0 || (cap > 0 && cap < 2 * h->v.K)) return fail(-3, "sim cap: 0 (off) or at least 2 * search_threads");
  h->v.simcap = h->v.K > 1 ? cap : 0;
  return 0;
}

int spmcts_search_progress(spmcts_arena *h, int32_t *started_dev, int32_t *resume_dev, spmcts_stream stream) {
  if (!h) return fail(-1, "null arena");
  const size_t T = h->v.T;
  if (started_dev) HIP_TRY(hipMemcpyAsync(started_dev, h->v.tstarted, 4 * T, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (resume_dev) HIP_TRY(hipMemcpyAsync(resume_dev, h->v.tres, 4 * T, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

int spmcts_get_sim_pauses(spmcts_arena *h, int64_t *pauses_out) {
  if (!h || !pauses_out) return fail(-1, "null argument");
  HIP_TRY(hipDeviceSynchronize());
  std::vector<int64_t> c((size_t)h->v.T * C_NCNT);
  HIP_TRY(hipMemcpy(c.data(), h->v.cnt, c.size() * 8, hipMemcpyDeviceToHost));
  int64_t n = 0;
  for (int t = 0; t < h->v.T; ++t) n += c[(size_t)t * C_NCNT + C_PAUSE];
  *pauses_out = n;
  return 0;
}

int spmcts_set_eval_cache(spmcts_arena *h, int32_t window, int32_t capacity_log2) {
  if (!h) return fail(-1, "null arena");
  if (window < 0 || window > (1 << 20)) return fail(-3, "eval cache window out of range");
  if (capacity_log2 != 0 && (capacity_log2 < 10 || capacity_log2 > 28)) return fail(-3, "eval cache capacity_log2: 10..28 (0 = sized from the arena)");
  if (window > 0 && league_on(h)) return fail(-3, LEAGUE_EXCLUDES);
  if (h->cache_step) return fail(-4, "a step that consulted the evaluation cache has not been expanded yet");
  for (const spmcts_arena *f : h->followers)
    if (f->cache_step && f->cache_shared_step)
      return fail(-4, "a follower lane's step that uses this arena's evaluation cache has not been expanded yet");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());  // no launch of this arena reads the old table any more
  for (void *p : h->cache_allocs) (void)hipFree(p);
  h->cache_allocs.clear();
  View &v = h->v;
  v.crec = nullptr;
  v.xc = nullptr;
  v.cwin = 0;
  v.cmask = 0;
  h->cache_step = h->cache_shared_step = false;
  if (window == 0) return 0;
  if (v.K < 2) return fail(-3, "the evaluation cache needs search_threads > 1 (it extends leaf dedup)");
  int L = capacity_log2;
  if (L == 0) {
    // entries held: window + 1 generations (the slack one) of at most one row per searching tree per sim, plus
    // the end-of-ply rows; a leader's table also takes a follower lane's rows (cache_view): twice one lane's, and
    // twice that again so probe chains stay short
    const long long searching = std::max<long long>(v.G > 0 ? v.G : v.T, 1);
    const long long held = (long long)(window + 1) * searching * ((long long)v.iters + 2);
    L = 10;
    while (L < 26 && (1ll << L) < 4 * held) ++L;
  }
  const size_t E = (size_t)1 << L;
  void *p[2] = {};
  const size_t bytes[2] = {E * CACHE_REC * 8, (size_t)v.NS * 4};
  for (int i = 0; i < 2; ++i) {
    const hipError_t e = hipMalloc(&p[i], bytes[i]);
    if (e != hipSuccess) {
      for (int j = 0; j < i; ++j) (void)hipFree(p[j]);
      return fail(-1000 - (int)e, std::string("eval cache hipMalloc: ") + hipGetErrorString(e));
    }
    h->cache_allocs.push_back(p[i]);
  }
  HIP_TRY(hipMemset(p[0], 0, bytes[0]));  // every entry never used
  v.crec = (uint64_t *)p[0];
  v.xc = (int32_t *)p[1];
  v.cmask = (int)(E - 1);
  v.cwin = window;
  v.cgen = (uint32_t)window + 1;  // generation 0 never read as live
  HIP_TRY(hipDeviceSynchronize());
  return 0;
}

int spmcts_eval_cache_clear(spmcts_arena *h) {
  if (!h) return fail(-1, "null arena");
  if (h->v.cwin) h->v.cgen += (uint32_t)h->v.cwin + 1;  // every entry leaves the window
  return 0;
}

int spmcts_games_set_record(spmcts_arena *h, int32_t record) {
  if (!h) return fail(-1, "null arena");
  h->v.record = record ? 1 : 0;
  return 0;
}

int spmcts_games_set_log(spmcts_arena *h, int32_t on) {
  if (!h) return fail(-1, "null arena");
  if (h->v.G <= 0) return fail(-4, "arena has no game slots");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t G = h->v.G, cells = h->cells;
  std::vector<uint8_t> st(G);
  HIP_TRY(hipMemcpy(st.data(), h->v.gstate, G, hipMemcpyDeviceToHost));
  for (uint8_t s : st)
    if (s != GS_IDLE) return fail(-4, "the game log cannot change while a game is active");
  View &v = h->v;
  if (!on) {
    v.glog = nullptr;
    return 0;
  }
  if (h->log_allocs.empty()) {
    // the ring holds the games of two plies (a ply finishes at most n_games): drained once per ply it never fills
    const size_t cap = 2 * G;
    const size_t bytes[9] = {G * cells, 16, 8 * cap, 4 * cap, cap, cap, 4 * cap, 4 * cap, cap * cells};
    void *p[9] = {};
    for (int i = 0; i < 9; ++i) {
      hipError_t e = hipMalloc(&p[i], bytes[i]);
      if (e == hipSuccess) e = hipMemset(p[i], 0, bytes[i]);
      if (e != hipSuccess) {
        for (int j = 0; j <= i; ++j)
          if (p[j]) (void)hipFree(p[j]);
        return fail(-1000 - (int)e, std::string("game log hipMalloc: ") + hipGetErrorString(e));
      }
    }
    h->log_allocs.assign(p, p + 9);
    h->log_dev = (uint8_t *)p[0];
    v.lr_cap = (int32_t)cap;
    v.lr_count = (int32_t *)p[1];
    v.lr_id = (int64_t *)p[2];
    v.lr_slot = (int32_t *)p[3];
    v.lr_result = (int8_t *)p[4];
    v.lr_swap = (uint8_t *)p[5];
    v.lr_plies = (int32_t *)p[6];
    v.lr_open = (int32_t *)p[7];
    v.lr_moves = (uint8_t *)p[8];
    HIP_TRY(hipDeviceSynchronize());
  }
  v.glog = h->log_dev;
  return 0;
}

int spmcts_search_end(spmcts_arena *h, double temp, int32_t *actions_dev, int8_t *states_dev, float *tree_probs_dev,
                      double *q_dev, uint8_t *q_f64_dev, uint8_t *recorded_dev, spmcts_stream stream) {
  if (!h) return fail(-1, "null arena");
  const int n = h->n_active;
  if (n <= 0) return 0;
  if (h->v.pf_keep)  // the active trees' verdicts, read by k_search_end
    TRY(LAUNCH_SB(h, k_proof_verdict, (long long)n * h->P, TB_THREADS, (hipStream_t)stream, h->v, (const int32_t *)nullptr,
               n, (int)PF_MODE_ACTIVE, h->v.pf_keep, h->v.pf_lo, h->v.pf_hi));
  return LAUNCH(h, k_search_end, n, 64, (hipStream_t)stream, h->v, n, temp, actions_dev, states_dev, tree_probs_dev,
                q_dev, q_f64_dev, recorded_dev);
}

int spmcts_play_action(spmcts_arena *h, const int32_t *trees_dev, const int32_t *actions_dev, int32_t n,
                       void *leaves_dev, int32_t *leaf_count_dev, spmcts_stream stream) {
  if (!h) return fail(-1, "null arena");
  hipStream_t s = (hipStream_t)stream;
  if (n > 0) TRY(LAUNCH(h, k_play_action, n, 64, s, h->v, trees_dev, actions_dev, n));
  return launch_rows(h, leaves_dev, leaf_count_dev, s, false);
}

int spmcts_leaf_trees(spmcts_arena *h, int32_t *trees_dev, spmcts_stream stream) {
  if (!h || !trees_dev) return fail(-1, "null argument");
  HIP_TRY(hipMemcpyAsync(trees_dev, h->v.row_tree, sizeof(int32_t) * h->v.NS, hipMemcpyDeviceToDevice,
                         (hipStream_t)stream));
  return 0;
}

int spmcts_root_stats(spmcts_arena *h, int32_t tree, int32_t *child_n, double *child_w, float *child_p,
                      int32_t *root_n, double *root_w, int32_t *root_player, int8_t *board) {
  if (!h) return fail(-1, "null arena");
  if (tree < 0 || tree >= h->v.T) return fail(-3, "tree out of range");
  HIP_TRY(hipDeviceSynchronize());
  const size_t nb = (size_t)tree * h->v.cap * h->P;
  int32_t root = 0, cb = -1;
  int8_t rp = 0;
  uint64_t pos = 0, neg = 0;
  HIP_TRY(hipMemcpy(&root, h->v.root + tree, 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&cb, node_field(h, 8, 4, nb + root), 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&rp, h->v.rplayer + tree, 1, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&pos, h->v.rpos + tree, 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&neg, h->v.rneg + tree, 8, hipMemcpyDeviceToHost));
  if (root_n) HIP_TRY(hipMemcpy(root_n, node_field(h, 0, 4, nb + root), 4, hipMemcpyDeviceToHost));
  if (root_w) HIP_TRY(hipMemcpy(root_w, node_field(h, 16, 8, nb + root), 8, hipMemcpyDeviceToHost));
  if (root_player) *root_player = rp;
  if (cb >= 0) {
    const size_t ci = nb + (size_t)cb * h->P;
    if (child_n) HIP_TRY(hipMemcpy(child_n, node_field(h, 0, 4, ci), 4 * h->A, hipMemcpyDeviceToHost));
    if (child_w) HIP_TRY(hipMemcpy(child_w, node_field(h, 16, 8, ci), 8 * h->A, hipMemcpyDeviceToHost));
    if (child_p) HIP_TRY(hipMemcpy(child_p, node_field(h, 12, 4, ci), 4 * h->A, hipMemcpyDeviceToHost));
  } else {
    for (int j = 0; j < h->A; ++j) {
      if (child_n) child_n[j] = 0;
      if (child_w) child_w[j] = 0.0;
      if (child_p) child_p[j] = 0.f;
    }
  }
  if (board) {
    for (int x = 0; x < h->W; ++x)
      for (int y = 0; y < h->H; ++y) {
        const uint64_t bit = 1ull << (x * (h->H + 1) + y);
        board[x * h->H + y] = (pos & bit) ? 1 : ((neg & bit) ? -1 : 0);
      }
  }
  return 0;
}

int spmcts_games_start(spmcts_arena *h, const int32_t *slots_dev, const float *priors_dev, int32_t n,
                       spmcts_stream stream) {
  if (!h) return fail(-1, "null arena");
  if (h->v.G <= 0) return fail(-4, "arena has no game slots");
  if (n <= 0) return 0;
  h->begun = true;
  hipStream_t s = (hipStream_t)stream;
  TRY(LAUNCH_SB(h, k_games_start, n, 128, s, h->v, slots_dev, priors_dev, n));
  return launch(k_games_bump_id, 1, 1, s, h->v, n);
}

int spmcts_games_set_limit(spmcts_arena *h, int64_t max_games) {
  if (!h) return fail(-1, "null arena");
  HIP_TRY(hipMemcpy(h->v.gcnt + 8, &max_games, 8, hipMemcpyHostToDevice));
  return 0;
}

int spmcts_games_begin_ply(spmcts_arena *h, spmcts_stream stream) {
  if (!h) return fail(-1, "null arena");
  if (h->v.G <= 0) return fail(-4, "arena has no game slots");
  h->n_active = h->v.G;
  h->games_list = true;  // active[g] = the searching tree of game g, or -1: ascending
  h->v.sim = 0;
  if (h->v.cwin) ++h->v.cgen;  // a new evaluation-cache generation per ply
  TRY(LAUNCH(h, k_games_begin_ply, h->v.G, 128, (hipStream_t)stream, h->v));
  if (h->v.gc) TRY(LAUNCH_SB(h, k_compact, 256ll * h->v.G, 256, (hipStream_t)stream, h->v, h->v.G));  // one block per tree
  return 0;
}

int spmcts_games_end_ply(spmcts_arena *h, void *leaves_dev, int32_t *leaf_count_dev, spmcts_stream stream) {
  if (!h) return fail(-1, "null arena");
  hipStream_t s = (hipStream_t)stream;
  if (h->nm_on) TRY(negamax_games(h, s));  // the negamax movers' codes, read by k_games_end_ply
  if (h->v.pf_keep)  // the mover trees' verdicts, read by k_games_end_ply
    TRY(LAUNCH_SB(h, k_proof_verdict, (long long)h->v.G * h->P, TB_THREADS, s, h->v, (const int32_t *)nullptr, h->v.G,
               (int)PF_MODE_GAMES, h->v.pf_keep, h->v.pf_lo, h->v.pf_hi));
  TRY(LAUNCH(h, k_games_end_ply, h->v.G, 64, s, h->v));
  return launch_rows(h, leaves_dev, leaf_count_dev, s, false);
}

int spmcts_games_finish_ply(spmcts_arena *h, int32_t refill, int32_t *out_dev, spmcts_stream stream) {
  if (!h) return fail(-1, "null arena");
  hipStream_t s = (hipStream_t)stream;
  TRY(LAUNCH(h, k_games_finish_scan, 1024, 1024, s, h->v, refill, out_dev));  // one block
  return LAUNCH_SB(h, k_games_finish_apply, h->v.G, 64, s, h->v);
}

int spmcts_export_moves(spmcts_arena *h, int8_t *states_dev, float *tree_probs_dev, double *q_dev, uint8_t *q_f64_dev,
                        float *z_dev, int64_t *game_dev, int32_t max_records, int32_t *count_dev,
                        spmcts_stream stream) {
  if (!h) return fail(-1, "null arena");
  hipStream_t s = (hipStream_t)stream;
  TRY(launch(k_export, max_records, 256, s, h->v, h->A, h->cells, states_dev, tree_probs_dev, q_dev, q_f64_dev, z_dev,
             game_dev, max_records, count_dev));
  return launch(k_export_clear, 1, 1, s, h->v);
}

int spmcts_export_games(spmcts_arena *h, int64_t *id_dev, int32_t *slot_dev, int8_t *result_dev, uint8_t *swap_dev,
                        int32_t *plies_dev, int32_t *opening_dev, uint8_t *moves_dev, int32_t max_records,
                        int32_t *count_dev, spmcts_stream stream) {
  if (!h) return fail(-1, "null arena");
  if (h->log_allocs.empty()) return fail(-4, "the arena has no game log (spmcts_games_set_log)");
  if (max_records < 0) return fail(-3, "max_records must not be negative");
  if (max_records > 0 && (!id_dev || !slot_dev || !result_dev || !swap_dev || !plies_dev || !opening_dev || !moves_dev))
    return fail(-1, "null argument");
  hipStream_t s = (hipStream_t)stream;
  TRY(launch(k_export_games, max_records, 256, s, h->v, h->cells, id_dev, slot_dev, result_dev, swap_dev, plies_dev,
             opening_dev, moves_dev, max_records, count_dev));
  return launch(k_export_games_clear, 1, 1, s, h->v);
}

int spmcts_games_state(spmcts_arena *h, uint8_t *active, int32_t *ply, uint8_t *swap, int64_t *game_id) {
  if (!h) return fail(-1, "null arena");
  HIP_TRY(hipDeviceSynchronize());
  const size_t G = h->v.G;
  if (active) HIP_TRY(hipMemcpy(active, h->v.gstate, G, hipMemcpyDeviceToHost));
  if (ply) HIP_TRY(hipMemcpy(ply, h->v.gply, 4 * G, hipMemcpyDeviceToHost));
  if (swap) HIP_TRY(hipMemcpy(swap, h->v.gswap, G, hipMemcpyDeviceToHost));
  if (game_id) HIP_TRY(hipMemcpy(game_id, h->v.gid, 8 * G, hipMemcpyDeviceToHost));
  return 0;
}

int spmcts_games_results(spmcts_arena *h, int8_t *result, uint8_t *swap, int32_t *ply, uint8_t *state) {
  if (!h) return fail(-1, "null arena");
  HIP_TRY(hipDeviceSynchronize());
  const size_t G = h->v.G;
  if (!G) return 0;
  if (result) HIP_TRY(hipMemcpy(result, h->v.gresult, G, hipMemcpyDeviceToHost));
  if (swap) HIP_TRY(hipMemcpy(swap, h->v.gswap, G, hipMemcpyDeviceToHost));
  if (ply) HIP_TRY(hipMemcpy(ply, h->v.gply, 4 * G, hipMemcpyDeviceToHost));
  if (state) HIP_TRY(hipMemcpy(state, h->v.gstate, G, hipMemcpyDeviceToHost));
  return 0;
}

// ---- opening book ---------------------------------------------------------
int spmcts_openings_validate(int32_t game, int32_t width, int32_t height, const uint8_t *moves, const int32_t *lens,
                             int32_t n_openings, int32_t max_len) {
  if (n_openings < 0 || n_openings > BOOK_MAX_OPENINGS) return fail(-3, "openings: 0 .. 65536 sequences");
  if (n_openings == 0) return 0;
  if (!moves || !lens) return fail(-1, "null argument");
  return with_game(game, width, height, [&](auto g) {
    using G = decltype(g);
    if (max_len < 0 || max_len >= G::CELLS) return fail(-3, "openings: max_len must be below width * height");
    char buf[160];
    for (int i = 0; i < n_openings; ++i) {
      if (lens[i] < 0 || lens[i] > max_len) {
        snprintf(buf, sizeof(buf), "opening %d: length %d outside [0, max_len = %d]", i, lens[i], max_len);
        return fail(-3, buf);
      }
      Board b{0, 0};
      int player = 1;  // legality and the game's end do not depend on who moves first
      for (int p = 0; p < lens[i]; ++p, player = -player) {
        const int a = moves[(size_t)i * max_len + p];
        int r = 0, d = 0;
        if (a >= G::A || !((legal_mask<G>(b) >> a) & 1u) || step<G>(b, a, player, &r, &d) != STEP_OK) {
          snprintf(buf, sizeof(buf), "opening %d ply %d: illegal move %d", i, p, a);
          return fail(-3, buf);
        }
        if (d) {
          snprintf(buf, sizeof(buf), "opening %d ply %d: move %d ends the game", i, p, a);
          return fail(-3, buf);
        }
      }
    }
    return 0;
  });
}

int spmcts_games_set_openings(spmcts_arena *h, const uint8_t *moves, const int32_t *lens, int32_t n_openings,
                              int32_t max_len, int32_t id_period) {
  if (!h) return fail(-1, "null arena");
  if (h->v.G <= 0) return fail(-4, "arena has no game slots");
  if (id_period < 0 || (id_period & 1)) return fail(-3, "openings: id_period must be even (0 = no modulus)");
  TRY(spmcts_openings_validate(h->cfg.game, h->W, h->H, moves, lens, n_openings, max_len));
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t G = h->v.G;
  std::vector<uint8_t> st(G);
  HIP_TRY(hipMemcpy(st.data(), h->v.gstate, G, hipMemcpyDeviceToHost));
  for (uint8_t s : st)
    if (s != GS_IDLE) return fail(-4, "openings cannot change while a game is active");
  View &v = h->v;
  HIP_TRY(hipMemset(v.gopen, 0xff, 4 * G));  // -1: no opening
  HIP_TRY(hipMemset(v.gbook, 0, 4 * G));
  v.book_n = v.book_len = v.book_period = 0;
  if (n_openings == 0) return 0;
  if (max_len > 0) HIP_TRY(hipMemcpy(v.book_moves, moves, (size_t)n_openings * max_len, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(v.book_lens, lens, 4 * (size_t)n_openings, hipMemcpyHostToDevice));
  v.book_n = n_openings;
  v.book_len = max_len;
  v.book_period = id_period;
  return 0;
}

int spmcts_games_openings(spmcts_arena *h, int32_t *opening_of_slot) {
  if (!h || !opening_of_slot) return fail(-1, "null argument");
  const size_t G = h->v.G;
  if (!G) return 0;
  HIP_TRY(hipDeviceSynchronize());
  std::vector<uint8_t> st(G);
  HIP_TRY(hipMemcpy(st.data(), h->v.gstate, G, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(opening_of_slot, h->v.gopen, 4 * G, hipMemcpyDeviceToHost));
  for (size_t g = 0; g < G; ++g)
    if (!h->v.book_n || st[g] == GS_IDLE) opening_of_slot[g] = -1;
  return 0;
}

int spmcts_root_stats_batch(spmcts_arena *h, const int32_t *trees_dev, int32_t n, int32_t *child_n_dev,
                            double *child_w_dev, float *child_p_dev, int32_t *root_n_dev, double *root_w_dev,
                            int8_t *root_player_dev, int8_t *boards_dev, spmcts_stream stream) {
  if (!h) return fail(-1, "null arena");
  if (n <= 0) return 0;
  if (!trees_dev) return fail(-1, "null argument");
  return LAUNCH(h, k_root_stats_batch, (long long)n * h->P, 256, (hipStream_t)stream, h->v, trees_dev, n, child_n_dev,
                child_w_dev, child_p_dev, root_n_dev, root_w_dev, root_player_dev, boards_dev);
}

// ---- reading the trees ------------------------------------------------------
int spmcts_tree_pv_batch(spmcts_arena *h, const int32_t *trees_dev, int32_t n, int32_t max_len, int32_t min_visits,
                         int8_t *pv_dev, int32_t *pv_n_dev, int32_t *pv_vl_dev, double *pv_w_dev, float *pv_p_dev,
                         int32_t *pv_len_dev, uint8_t *pv_end_dev, int8_t *end_board_dev, spmcts_stream stream) {
  if (!h) return fail(-1, "null arena");
  if (n < 0) return fail(-3, "tree_pv: n must not be negative");
  if (max_len < 1 || max_len > h->cells) return fail(-3, "tree_pv: max_len must be in [1, width * height]");
  if (min_visits < 0) return fail(-3, "tree_pv: min_visits must not be negative");
  if (n == 0) return 0;
  if (!trees_dev) return fail(-1, "null argument");
  const TreePvOut o{pv_dev, pv_n_dev, pv_vl_dev, pv_w_dev, pv_p_dev, pv_len_dev, pv_end_dev, end_board_dev};
  return LAUNCH(h, k_tree_pv, (long long)n * h->P, 256, (hipStream_t)stream, h->v, trees_dev, n, max_len, min_visits,
                o);
}

int spmcts_tree_export_work_bytes(spmcts_arena *h, int32_t n, int32_t max_nodes, uint64_t *bytes_out) {
  if (!h || !bytes_out) return fail(-1, "null argument");
  if (n < 0 || max_nodes < 1) return fail(-3, "tree_export: n must not be negative and max_nodes at least 1");
  return with_game(h->cfg.game, h->W, h->H, [&](auto g) {
    *bytes_out = 8 * (uint64_t)tree_export_work_words<decltype(g)>((size_t)n, (size_t)max_nodes);
    return 0;
  });
}

static int tree_export(spmcts_arena *h, const int32_t *trees_dev, int32_t n, int32_t max_nodes, int32_t min_visits,
                       int32_t max_depth, TreeExportOut o, void *work_dev, uint64_t work_bytes, spmcts_stream stream);

int spmcts_tree_export_batch(spmcts_arena *h, const int32_t *trees_dev, int32_t n, int32_t max_nodes,
                             int32_t min_visits, int32_t max_depth, int32_t *parent_dev, int8_t *action_dev,
                             int16_t *depth_dev, int32_t *node_n_dev, int32_t *node_vl_dev, double *node_w_dev,
                             float *node_p_dev, int8_t *player_dev, uint8_t *flags_dev, int32_t *count_dev,
                             void *work_dev, uint64_t work_bytes, spmcts_stream stream) {
  const TreeExportOut o{parent_dev, action_dev, depth_dev, node_n_dev, node_vl_dev, node_w_dev, node_p_dev, player_dev,
                        flags_dev, count_dev, nullptr, nullptr};
  return tree_export(h, trees_dev, n, max_nodes, min_visits, max_depth, o, work_dev, work_bytes, stream);
}

int spmcts_tree_export_bounds_batch(spmcts_arena *h, const int32_t *trees_dev, int32_t n, int32_t max_nodes,
                                    int32_t min_visits, int32_t max_depth, int32_t *parent_dev, int8_t *action_dev,
                                    int16_t *depth_dev, int32_t *node_n_dev, int32_t *node_vl_dev, double *node_w_dev,
                                    float *node_p_dev, int8_t *player_dev, uint8_t *flags_dev, int32_t *count_dev,
                                    int8_t *move_lo_dev, int8_t *move_hi_dev, void *work_dev, uint64_t work_bytes,
                                    spmcts_stream stream) {
  if (!h) return fail(-1, "null arena");
  if (!h->sb) return fail(-4, "the arena keeps no stored bounds (spmcts_set_solver_search)");
  const TreeExportOut o{parent_dev, action_dev, depth_dev, node_n_dev, node_vl_dev, node_w_dev, node_p_dev, player_dev,
                        flags_dev, count_dev, move_lo_dev, move_hi_dev};
  return tree_export(h, trees_dev, n, max_nodes, min_visits, max_depth, o, work_dev, work_bytes, stream);
}

static int tree_export(spmcts_arena *h, const int32_t *trees_dev, int32_t n, int32_t max_nodes, int32_t min_visits,
                       int32_t max_depth, TreeExportOut o, void *work_dev, uint64_t work_bytes, spmcts_stream stream) {
  if (!h) return fail(-1, "null arena");
  if (n < 0) return fail(-3, "tree_export: n must not be negative");
  if (max_nodes < 1) return fail(-3, "tree_export: max_nodes must be at least 1");
  if (min_visits < 0) return fail(-3, "tree_export: min_visits must not be negative");
  if (n == 0) return 0;
  uint64_t need = 0;
  TRY(spmcts_tree_export_work_bytes(h, n, max_nodes, &need));
  if (!trees_dev || !work_dev) return fail(-1, "null argument");
  if (work_bytes < need || ((uintptr_t)work_dev & 7))
    return fail(-3, "tree_export: work buffer too small or not 8-byte aligned (spmcts_tree_export_work_bytes)");
  return LAUNCH(h, k_tree_export, (long long)n * h->P, 256, (hipStream_t)stream, h->v, trees_dev, n, max_nodes,
                min_visits, max_depth, o, (uint64_t *)work_dev);
}

int spmcts_tree_bounds_batch(spmcts_arena *h, const int32_t *trees_dev, int32_t n, int8_t *lo_dev, int8_t *hi_dev,
                             int8_t *move_lo_dev, int8_t *move_hi_dev, int8_t *best_dev, int8_t *empty_dev,
                             int32_t *nodes_dev, spmcts_stream stream) {
  if (!h) return fail(-1, "null arena");
  if (n < 0) return fail(-3, "tree_bounds: n must not be negative");
  if (n == 0) return 0;
  if (!trees_dev) return fail(-1, "null argument");
  const TreeBoundsOut o{lo_dev, hi_dev, move_lo_dev, move_hi_dev, best_dev, empty_dev, nodes_dev};
  return LAUNCH(h, k_tree_bounds, (long long)n * h->P, TB_THREADS, (hipStream_t)stream, h->v, trees_dev, n, o);
}

// ---- proof-guided play -------------------------------------------------------
int spmcts_set_proof_play(spmcts_arena *h, const uint8_t *on) {
  if (!h) return fail(-1, "null arena");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  const size_t T = h->v.T;
  std::vector<uint8_t> f(T, 1);
  bool any = !on;
  if (on)
    for (size_t t = 0; t < T; ++t) any |= (f[t] = on[t] ? 1 : 0) != 0;
  View &v = h->v;
  if (!any && h->proof_allocs.empty()) return 0;  // never on: nothing to switch off
  const size_t bytes[6] = {T, 4 * T, T, T, 8 * PF_NSTAT, 4 * T};
  if (h->proof_allocs.empty()) {
    void *p[6] = {};
    for (int i = 0; i < 6; ++i) {
      hipError_t e = hipMalloc(&p[i], bytes[i]);
      if (e == hipSuccess) e = hipMemset(p[i], 0, bytes[i]);
      if (e != hipSuccess) {
        for (int j = 0; j <= i; ++j)
          if (p[j]) (void)hipFree(p[j]);
        return fail(-1000 - (int)e, std::string("proof play hipMalloc: ") + hipGetErrorString(e));
      }
    }
    h->proof_allocs.assign(p, p + 6);
  }
  void *const *p = h->proof_allocs.data();
  HIP_TRY(hipMemcpy(p[0], f.data(), T, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(p[1], 0xff, bytes[1]));  // PF_ALL: no verdict yet
  HIP_TRY(hipMemset(p[2], 0x80, bytes[2]));  // TB_NONE
  HIP_TRY(hipMemset(p[3], 0x80, bytes[3]));
  HIP_TRY(hipDeviceSynchronize());
  v.pf_on = any ? (uint8_t *)p[0] : nullptr;
  v.pf_keep = any ? (uint32_t *)p[1] : nullptr;
  v.pf_lo = any ? (int8_t *)p[2] : nullptr;
  v.pf_hi = any ? (int8_t *)p[3] : nullptr;
  v.pf_stats = any ? (unsigned long long *)p[4] : nullptr;
  v.pf_nstop = any ? (int32_t *)p[5] : nullptr;
  return 0;
}

int spmcts_tree_proof_moves_batch(spmcts_arena *h, const int32_t *trees_dev, int32_t n, uint32_t *keep_dev,
                                  int8_t *lo_dev, int8_t *hi_dev, spmcts_stream stream) {
  if (!h) return fail(-1, "null arena");
  if (n < 0) return fail(-3, "tree_proof_moves: n must not be negative");
  if (n == 0) return 0;
  if (!trees_dev) return fail(-1, "null argument");
  return LAUNCH_SB(h, k_proof_verdict, (long long)n * h->P, TB_THREADS, (hipStream_t)stream, h->v, trees_dev, n,
                   (int)PF_MODE_LIST, keep_dev, lo_dev, hi_dev);
}

int spmcts_proof_last(spmcts_arena *h, uint32_t *keep_dev, int8_t *lo_dev, int8_t *hi_dev, spmcts_stream stream) {
  if (!h) return fail(-1, "null arena");
  if (!h->v.pf_keep) return fail(-4, "proof play is off (spmcts_set_proof_play)");
  const size_t T = h->v.T;
  hipStream_t s = (hipStream_t)stream;
  if (keep_dev) HIP_TRY(hipMemcpyAsync(keep_dev, h->v.pf_keep, 4 * T, hipMemcpyDeviceToDevice, s));
  if (lo_dev) HIP_TRY(hipMemcpyAsync(lo_dev, h->v.pf_lo, T, hipMemcpyDeviceToDevice, s));
  if (hi_dev) HIP_TRY(hipMemcpyAsync(hi_dev, h->v.pf_hi, T, hipMemcpyDeviceToDevice, s));
  return 0;
}

int spmcts_get_proof_stats(spmcts_arena *h, int64_t *out) {
  if (!h || !out) return fail(-1, "null argument");
  for (int i = 0; i < SPMCTS_PROOF_NSTAT; ++i) out[i] = 0;
  if (h->proof_allocs.empty()) return 0;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  static_assert(SPMCTS_PROOF_NSTAT == PF_NSTAT, "proof stats layout");
  HIP_TRY(hipMemcpy(out, h->proof_allocs[4], 8 * PF_NSTAT, hipMemcpyDeviceToHost));
  return 0;
}

int spmcts_proof_stopped(spmcts_arena *h, int32_t *count_dev, spmcts_stream stream) {
  if (!h || !count_dev) return fail(-1, "null argument");
  const size_t T = h->v.T;
  if (h->proof_allocs.empty()) {
    HIP_TRY(hipMemsetAsync(count_dev, 0, 4 * T, (hipStream_t)stream));
  } else {
    HIP_TRY(hipMemcpyAsync(count_dev, h->proof_allocs[5], 4 * T, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  }
  return 0;
}

int spmcts_proof_stop(spmcts_arena *h, spmcts_stream stream) {
  if (!h) return fail(-1, "null arena");
  if (h->v.K <= 1) return fail(-4, "proof_stop needs search_threads > 1 (a sequential search has no sims left to skip)");
  if (!h->v.pf_keep) return fail(-4, "proof_stop needs proof play (spmcts_set_proof_play)");
  return LAUNCH_SB(h, k_proof_stop, (long long)h->v.T * h->P, TB_THREADS, (hipStream_t)stream, h->v);
}

// ---- mirror symmetry ------------------------------------------------------------
int spmcts_set_symmetry(spmcts_arena *h, int32_t mode) {
  if (!h) return fail(-1, "null arena");
  if (mode != 0 && mode != SPMCTS_SYM_MIRROR) return fail(-3, "symmetry: unknown mode (0 or SPMCTS_SYM_MIRROR)");
  if (mode == h->sym) return 0;
  // rows, peer rows and cache records of one orientation rule only: fixed once a search has run or a lane is paired
  if (h->begun) return fail(-2, "symmetry must be set before the arena's first search or game start");
  if (h->peer || !h->followers.empty()) return fail(-2, "symmetry must be set before the arena is paired with a peer");
  h->sym = mode;
  return 0;
}

int spmcts_get_symmetry(const spmcts_arena *h) { return h ? h->sym : fail(-1, "null arena"); }

int spmcts_canonical_host(int32_t game, int32_t width, int32_t height, const int8_t *board, int32_t player, int8_t *canon,
                          int32_t *flipped) {
  if (!board || !canon || !flipped) return fail(-1, "null argument");
  return with_game(game, width, height, [&](auto g) {
    using G = decltype(g);
    const Board b = from_cells<G>(board);
    uint64_t own = player > 0 ? b.pos : b.neg, opp = player > 0 ? b.neg : b.pos;
    *flipped = canonical_pair<G>(own, opp) ? 1 : 0;
    for (int x = 0; x < G::W; ++x)
      for (int y = 0; y < G::H; ++y) canon[x * G::H + y] = cell_value<G>(Board{own, opp}, x, y);
    return 0;
  });
}

// ---- stored score bounds -----------------------------------------------------
int spmcts_set_solver_search(spmcts_arena *h, const uint8_t *on) {
  if (!h) return fail(-1, "null arena");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  // the use flags stay refused here: the search rules that read the stored bounds are switched per tree by
  // spmcts_set_solver_rules, and this call remains the maintenance switch
  bool any = !on;
  if (on)
    for (int t = 0; t < h->v.T; ++t) any |= on[t] != 0;
  if (any) return fail(-2, "solver search: the search rules are not built in this version (every use flag must be 0)");
  if (h->sb) return 0;
  // every block that exists must carry its bounds: only the root blocks may exist, and those are stamped here
  std::vector<int32_t> used(h->v.T);
  HIP_TRY(hipMemcpy(used.data(), h->v.used, 4 * (size_t)h->v.T, hipMemcpyDeviceToHost));
  for (int32_t u : used)
    if (u > 2) return fail(-4, "solver search must be switched on before the first search (a tree holds more than its root block)");
  h->sb = true;
  // the root blocks of the trees reset so far (from here on reset_tree stamps them itself)
  const int rc = LAUNCH(h, k_sb_stamp_roots, (long long)h->v.T * h->P, 64, (hipStream_t) nullptr, h->v);
  if (rc) {
    h->sb = false;
    return rc;
  }
  HIP_TRY(hipDeviceSynchronize());
  return 0;
}

// ---- solver-aware search -----------------------------------------------------
int spmcts_set_solver_rules(spmcts_arena *h, const uint8_t *rules) {
  if (!h) return fail(-1, "null arena");
  static_assert(SPMCTS_SOLVER_REFUTE == SBR_REFUTE && SPMCTS_SOLVER_PROVED == SBR_PROVED, "rule bits");
  const size_t T = h->v.T;
  bool any = false;
  if (rules)
    for (size_t t = 0; t < T; ++t) {
      if (rules[t] & ~(SPMCTS_SOLVER_REFUTE | SPMCTS_SOLVER_PROVED))
        return fail(-3, "solver rules: a bit outside SPMCTS_SOLVER_REFUTE | SPMCTS_SOLVER_PROVED");
      any |= rules[t] != 0;
    }
  if (!h->sb) return fail(-4, "the arena keeps no stored bounds (spmcts_set_solver_search)");
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  if (!any && h->solver_allocs.empty()) return 0;  // never on: nothing to switch off
  const size_t bytes[2] = {T, 8 * (size_t)SV_NSTAT * T};
  if (h->solver_allocs.empty()) {
    void *p[2] = {};
    for (int i = 0; i < 2; ++i) {
      hipError_t e = hipMalloc(&p[i], bytes[i]);
      if (e == hipSuccess) e = hipMemset(p[i], 0, bytes[i]);
      if (e != hipSuccess) {
        for (int j = 0; j <= i; ++j)
          if (p[j]) (void)hipFree(p[j]);
        return fail(-1000 - (int)e, std::string("solver rules hipMalloc: ") + hipGetErrorString(e));
      }
    }
    h->solver_allocs.assign(p, p + 2);
  }
  if (any) {
    HIP_TRY(hipMemcpy(h->solver_allocs[0], rules, T, hipMemcpyHostToDevice));
  } else {
    HIP_TRY(hipMemset(h->solver_allocs[0], 0, T));
  }
  HIP_TRY(hipDeviceSynchronize());
  h->v.sv_rules = any ? (uint8_t *)h->solver_allocs[0] : nullptr;
  h->v.sv_stats = (int64_t *)h->solver_allocs[1];
  return 0;
}

int spmcts_get_solver_stats(spmcts_arena *h, int64_t *out) {
  if (!h || !out) return fail(-1, "null argument");
  static_assert(SPMCTS_SOLVER_NSTAT == SV_NSTAT, "solver stats layout");
  for (int i = 0; i < SV_NSTAT; ++i) out[i] = 0;
  if (h->solver_allocs.empty()) return 0;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  std::vector<int64_t> st((size_t)SV_NSTAT * h->v.T);
  HIP_TRY(hipMemcpy(st.data(), h->solver_allocs[1], 8 * st.size(), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < st.size(); ++i) out[i % SV_NSTAT] += st[i];
  return 0;
}

int spmcts_solver_stats_trees(spmcts_arena *h, int64_t *out_dev, spmcts_stream stream) {
  if (!h || !out_dev) return fail(-1, "null argument");
  const size_t bytes = 8 * (size_t)SV_NSTAT * h->v.T;
  if (h->solver_allocs.empty()) {
    HIP_TRY(hipMemsetAsync(out_dev, 0, bytes, (hipStream_t)stream));
  } else {
    HIP_TRY(hipMemcpyAsync(out_dev, h->solver_allocs[1], bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  }
  return 0;
}

// ---- league ---------------------------------------------------------------
int spmcts_set_league(spmcts_arena *h, const int32_t *tree_net, int32_t n_nets) {
  if (!h) return fail(-1, "null arena");
  if (!tree_net && n_nets == 0) {  // off
    HIP_TRY(hipDeviceSynchronize());
    h->lg.n = 0;
    h->route_step = false;
    return 0;
  }
  if (!tree_net) return fail(-1, "null argument");
  if (n_nets < 1 || n_nets > LEAGUE_MAX_NETS) return fail(-3, "league: 1 .. 32 networks");
  const View &v = h->v;
  if (v.dedup || v.cwin || h->peer || !h->followers.empty() || v.seg1 < v.NS) return fail(-3, LEAGUE_EXCLUDES);
  const int T = v.T;
  std::vector<int32_t> seg(LEAGUE_MAX_NETS + 1, 0);
  for (int t = 0; t < T; ++t) {
    if (tree_net[t] < -1 || tree_net[t] >= n_nets) return fail(-3, "league: tree_net entries are -1 or in [0, n_nets)");
    if (tree_net[t] >= 0) seg[tree_net[t] + 1] += v.K;  // K rows per tree of the network at most
  }
  for (int j = 0; j < LEAGUE_MAX_NETS; ++j) seg[j + 1] += seg[j];
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipDeviceSynchronize());
  if (h->league_allocs.empty()) {
    const size_t blocks = ((size_t)v.NS + LEAGUE_SPAN - 1) / LEAGUE_SPAN;
    const size_t bytes[5] = {4 * (size_t)T, 4 * (size_t)(LEAGUE_MAX_NETS + 1), 4 * (size_t)v.NS, 4 * (size_t)v.NS,
                             4 * blocks * LEAGUE_MAX_NETS};
    void *p[5] = {};
    for (int i = 0; i < 5; ++i) {
      const hipError_t e = hipMalloc(&p[i], bytes[i]);
      if (e != hipSuccess) {
        for (int j = 0; j < i; ++j) (void)hipFree(p[j]);
        return fail(-1000 - (int)e, std::string("league hipMalloc: ") + hipGetErrorString(e));
      }
    }
    h->league_allocs.assign(p, p + 5);
    h->lg.tree_net = (int32_t *)p[0];
    h->lg.seg = (int32_t *)p[1];
    h->lg.rank = (int32_t *)p[2];
    h->lg.map = (int32_t *)p[3];
    h->lg.hist = (int32_t *)p[4];
  }
  HIP_TRY(hipMemcpy(h->lg.tree_net, tree_net, 4 * (size_t)T, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(h->lg.seg, seg.data(), 4 * seg.size(), hipMemcpyHostToDevice));
  h->lg_seg = seg;
  h->lg.n = n_nets;
  h->route_step = false;
  return 0;
}

int spmcts_league_segments(const spmcts_arena *h, int32_t *seg) {
  if (!h || !seg) return fail(-1, "null argument");
  if (!league_on(h)) return fail(-4, "not a league arena (spmcts_set_league)");
  for (int j = 0; j <= h->lg.n; ++j) seg[j] = h->lg_seg[j];
  return 0;
}

int spmcts_league_route(spmcts_arena *h, const void *leaves_dev, const int32_t *leaf_count_dev, int32_t row_bytes,
                        void *routed_dev, int32_t *net_count_dev, spmcts_stream stream) {
  if (!h || !leaves_dev || !routed_dev || !net_count_dev) return fail(-1, "null argument");
  if (!league_on(h)) return fail(-4, "not a league arena (spmcts_set_league)");
  if (row_bytes < 2 || (row_bytes & 1)) return fail(-3, "league: row_bytes must be a positive even number");
  const uintptr_t a = (uintptr_t)leaves_dev | (uintptr_t)routed_dev | (uintptr_t)row_bytes;
  if (a & 1) return fail(-3, "league: leaf rows must be 2-byte aligned");
  const hipStream_t s = (hipStream_t)stream;
  const View &v = h->v;
  League lg = h->lg;
  lg.count = leaf_count_dev ? leaf_count_dev : v.row_count;
  h->lg.count = lg.count;
  TRY(launch(k_league_hist, v.NS, LEAGUE_SPAN, s, v, lg));
  TRY(launch(k_league_scan, 64, 64, s, v, lg, net_count_dev));
  const int unit = (a & 15) == 0 ? 16 : (a & 7) == 0 ? 8 : (a & 3) == 0 ? 4 : 2;  // the widest aligned unit
  const int upr = row_bytes / unit;
  const long long n = std::min<long long>((long long)v.NS * upr, 256ll * LEAGUE_COPY_BLOCKS);
  if (unit == 16)
    TRY(launch(k_league_copy<uint4>, n, 256, s, v, lg, leaves_dev, routed_dev, upr));
  else if (unit == 8)
    TRY(launch(k_league_copy<uint2>, n, 256, s, v, lg, leaves_dev, routed_dev, upr));
  else if (unit == 4)
    TRY(launch(k_league_copy<uint32_t>, n, 256, s, v, lg, leaves_dev, routed_dev, upr));
  else
    TRY(launch(k_league_copy<uint16_t>, n, 256, s, v, lg, leaves_dev, routed_dev, upr));
  h->route_step = true;
  return 0;
}

int spmcts_league_unroute(spmcts_arena *h, const float *const *probs_by_net_dev, const float *const *values_by_net_dev,
                          float *probs_dev, float *values_dev, spmcts_stream stream) {
  if (!h || !probs_by_net_dev || !values_by_net_dev || !probs_dev || !values_dev) return fail(-1, "null argument");
  if (!league_on(h)) return fail(-4, "not a league arena (spmcts_set_league)");
  if (!h->route_step) return fail(-4, "spmcts_league_unroute needs spmcts_league_route of this step's rows first");
  const View &v = h->v;
  const long long n = std::min<long long>((long long)v.NS * (v.A + 1), 256ll * LEAGUE_COPY_BLOCKS);
  TRY(launch(k_league_unroute, n, 256, (hipStream_t)stream, v, h->lg, probs_by_net_dev, values_by_net_dev, probs_dev,
             values_dev));
  h->route_step = false;
  return 0;
}

int spmcts_get_counters(spmcts_arena *h, spmcts_counters *out) {
  if (!h || !out) return fail(-1, "null argument");
  HIP_TRY(hipDeviceSynchronize());
  memset(out, 0, sizeof(*out));
  std::vector<int64_t> c((size_t)h->v.T * C_NCNT);
  HIP_TRY(hipMemcpy(c.data(), h->v.cnt, c.size() * 8, hipMemcpyDeviceToHost));
  for (int t = 0; t < h->v.T; ++t) {
    const int64_t *ct = c.data() + (size_t)t * C_NCNT;
    out->sims += ct[C_SIMS];
    out->nn_leaves += ct[C_NN];
    out->terminal_leaves += ct[C_TERM];
    out->depth_sum += ct[C_DEPTH];
    out->set_node_expansions += ct[C_SETNODE];
    out->moves += ct[C_MOVES];
    out->leaked_sims += ct[C_LEAK];
    out->compactions += ct[C_GC];
    out->blocks_in_use_max = std::max<int64_t>(out->blocks_in_use_max, ct[C_HWM]);
  }
  std::vector<int32_t> used(h->v.T);
  HIP_TRY(hipMemcpy(used.data(), h->v.used, 4 * used.size(), hipMemcpyDeviceToHost));
  for (int32_t u : used) out->blocks_in_use_max = std::max<int64_t>(out->blocks_in_use_max, u);
  int64_t g[16];
  HIP_TRY(hipMemcpy(g, h->v.gcnt, sizeof(g), hipMemcpyDeviceToHost));
  out->games_finished = g[0];
  for (int k = 0; k < 6; ++k) out->results[k / 3][k % 3] = g[1 + k];
  out->positions_exported = g[9];
  out->nn_rows = g[10];
  out->cache_rows = g[11];
  HIP_TRY(hipMemcpy(&out->error_flags, h->v.err, 4, hipMemcpyDeviceToHost));
  return 0;
}

int spmcts_check(spmcts_arena *h) {
  if (!h) return fail(-1, "null arena");
  HIP_TRY(hipDeviceSynchronize());
  uint32_t e = 0;
  HIP_TRY(hipMemcpy(&e, h->v.err, 4, hipMemcpyDeviceToHost));
  if (e) {
    char buf[128];
    snprintf(buf, sizeof(buf), "device error flags 0x%x", e);
    return fail(-5, buf);
  }
  return 0;
}

int spmcts_env_step(int32_t game, int32_t width, int32_t height, const int8_t *boards_dev, const int32_t *actions_dev,
                    const int8_t *players_dev, const uint8_t *over_dev, int32_t n, int8_t *out_boards_dev,
                    int8_t *reward_dev, uint8_t *done_dev, int8_t *status_dev, uint8_t *valid_dev,
                    spmcts_stream stream) {
  if (n <= 0) return 0;
  return with_game(game, width, height, [&](auto g) {
    return launch(k_env_step<decltype(g)>, n, 256, (hipStream_t)stream, boards_dev, actions_dev, players_dev, over_dev,
                  n, out_boards_dev, reward_dev, done_dev, status_dev, valid_dev);
  });
}

int spmcts_env_step_host(int32_t game, int32_t width, int32_t height, int8_t *board, int32_t action, int32_t player,
                         int32_t *reward, int32_t *done) {
  return with_game(game, width, height, [&](auto g) {
    using G = decltype(g);
    if (action < 0 || action >= G::A) return fail(-3, "action out of range");
    Board b = from_cells<G>(board);
    int r = 0, d = 0;
    const int st = step<G>(b, action, player, &r, &d);
    for (int x = 0; x < G::W; ++x)
      for (int y = 0; y < G::H; ++y) board[x * G::H + y] = cell_value<G>(b, x, y);
    *reward = r;
    *done = d;
    return st;
  });
}

int spmcts_valid_moves_host(int32_t game, int32_t width, int32_t height, const int8_t *board, uint8_t *valid) {
  return with_game(game, width, height, [&](auto g) {
    using G = decltype(g);
    const uint32_t m = legal_mask<G>(from_cells<G>(board));
    for (int a = 0; a < G::A; ++a) valid[a] = (m >> a) & 1u;
    return 0;
  });
}

// ---- game records ----------------------------------------------------------------
static int lp_check(int32_t n, int32_t first_ply, int32_t max_rows, const void *const *ptrs, int np) {
  if (n < 0) return fail(-3, "n must not be negative");
  if (first_ply < 0) return fail(-3, "first_ply must not be negative");
  if (max_rows < 0) return fail(-3, "max_rows must not be negative");
  for (int i = 0; i < np; ++i)
    if (!ptrs[i] && (n > 0 && (i < 4 || max_rows > 0))) return fail(-1, "null argument");
  return 0;
}

int spmcts_log_positions(int32_t game, int32_t width, int32_t height, const uint8_t *moves_dev, const int32_t *plies_dev,
                         int32_t n, int32_t first_ply, int32_t max_rows, int8_t *boards_dev, int8_t *players_dev,
                         int32_t *row_record_dev, int32_t *row_ply_dev, uint8_t *status_dev, int32_t *offsets_dev,
                         spmcts_stream stream) {
  return with_game(game, width, height, [&](auto g) {
    using G = decltype(g);
    const void *ptrs[8] = {moves_dev, plies_dev, status_dev, offsets_dev, boards_dev, players_dev, row_record_dev, row_ply_dev};
    TRY(lp_check(n, first_ply, max_rows, ptrs, 8));
    if (n == 0) return 0;
    const hipStream_t s = (hipStream_t)stream;
    TRY(launch(k_log_status<G>, n, 128, s, moves_dev, plies_dev, n, first_ply, status_dev, offsets_dev));
    TRY(launch(k_log_scan, 1024, 1024, s, offsets_dev, n));  // one block
    return launch(k_log_rows<G>, n, 128, s, moves_dev, plies_dev, n, first_ply, status_dev, offsets_dev, max_rows,
                  boards_dev, players_dev, row_record_dev, row_ply_dev);
  });
}

int spmcts_log_positions_host(int32_t game, int32_t width, int32_t height, const uint8_t *moves, const int32_t *plies,
                              int32_t n, int32_t first_ply, int32_t max_rows, int8_t *boards, int8_t *players,
                              int32_t *row_record, int32_t *row_ply, uint8_t *status, int32_t *offsets) {
  return with_game(game, width, height, [&](auto g) {
    const void *ptrs[8] = {moves, plies, status, offsets, boards, players, row_record, row_ply};
    TRY(lp_check(n, first_ply, max_rows, ptrs, 8));
    if (n == 0) return 0;
    lp_host<decltype(g)>(moves, plies, n, first_ply, max_rows, boards, players, row_record, row_ply, status, offsets);
    return 0;
  });
}

// ---- negamax -------------------------------------------------------------------
int spmcts_negamax_max_depth(int32_t game, int32_t width, int32_t height) {
  return with_game(game, width, height, [](auto g) { return (int)NmCap<decltype(g)>::DEPTH; });
}

int spmcts_negamax_launch_positions(int32_t game, int32_t width, int32_t height, int32_t depth) {
  const int cap = spmcts_negamax_max_depth(game, width, height);
  if (cap < 0) return cap;
  if (depth < 1 || depth > cap) return fail(-3, "negamax depth: 1 .. " + std::to_string(cap));
  return with_game(game, width, height,
                   [&](auto g) { return (int)std::min<long long>(nm_launch_positions(decltype(g)::A, depth), 0x7fffffff); });
}

int spmcts_negamax_host(int32_t game, int32_t width, int32_t height, const int8_t *board, int32_t player, int32_t depth,
                        int8_t *scores, uint64_t *nodes) {
  const int cap = spmcts_negamax_max_depth(game, width, height);
  if (cap < 0) return cap;
  if (!board || !scores) return fail(-1, "null argument");
  if (depth < 1 || depth > cap) return fail(-3, "negamax depth: 1 .. " + std::to_string(cap));
  return with_game(game, width, height, [&](auto g) {
    using G = decltype(g);
    const Board b = from_cells<G>(board);
    nm_solve_host<G>(player > 0 ? b.pos : b.neg, player > 0 ? b.neg : b.pos, depth, scores, nodes);
    return 0;
  });
}

int spmcts_negamax_batch(int32_t game, int32_t width, int32_t height, const int8_t *boards_dev, const int8_t *players_dev,
                         int32_t n, int32_t depth, int8_t *scores_dev, uint64_t *nodes_dev, spmcts_stream stream) {
  const int cap = spmcts_negamax_max_depth(game, width, height);
  if (cap < 0) return cap;
  if (depth < 1 || depth > cap) return fail(-3, "negamax depth: 1 .. " + std::to_string(cap));
  if (n <= 0) return 0;
  if (!boards_dev || !players_dev || !scores_dev) return fail(-1, "null argument");
  return with_game(game, width, height, [&](auto g) {
    using G = decltype(g);
    return nm_launches<G>(n, depth, [&](long long p0, int m) {
      return launch(k_negamax_batch<G>, ((long long)m + NmGrid<G>::PPB - 1) / NmGrid<G>::PPB * NM_THREADS, NM_THREADS,
                    (hipStream_t)stream, boards_dev, players_dev, p0, m, depth, scores_dev, nodes_dev);
    });
  });
}

// ---- exact solver to the end of the game -------------------------------------------
int spmcts_solve_host(int32_t game, int32_t width, int32_t height, const int8_t *board, int32_t player, uint64_t *table,
                      uint64_t table_entries, uint64_t max_nodes, int8_t *scores, uint64_t *nodes) {
  return with_game(game, width, height, [&](auto g) {
    using G = decltype(g);
    if (!board || !scores) return fail(-1, "null argument");
    TRY(sv_table_check(table, table_entries));
    if (max_nodes < 1) return fail(-3, "max_nodes must be at least 1");
    const Board b = from_cells<G>(board);
    if (popc(b.pos | b.neg) == G::CELLS) return fail(-3, "the position is finished: the board is full");
    if (sv_has_line<G>(b.pos) || sv_has_line<G>(b.neg)) return fail(-3, "the position is finished: the board holds a line");
    sv_solve_host<G>(player > 0 ? b.pos : b.neg, player > 0 ? b.neg : b.pos, table, table_entries - 1, max_nodes, scores,
                     nodes);
    return 0;
  });
}

int spmcts_solve_work_bytes(int32_t game, int32_t width, int32_t height, int32_t n, uint64_t *bytes_out) {
  return with_game(game, width, height, [&](auto g) {
    if (!bytes_out) return fail(-1, "null argument");
    if (n < 0) return fail(-3, "n must not be negative");
    *bytes_out = (uint64_t)sv_work_bytes<decltype(g)>(n);
    return 0;
  });
}

int spmcts_solve_launches(void) { return g_solve_launches; }

int spmcts_solve_batch(int32_t game, int32_t width, int32_t height, const int8_t *boards_dev, const int8_t *players_dev,
                       int32_t n, uint64_t *table_dev, uint64_t table_entries, void *work_dev, uint64_t max_nodes,
                       uint32_t launch_nodes, int8_t *scores_dev, uint64_t *nodes_dev, spmcts_stream stream) {
  return with_game(game, width, height, [&](auto g) {
    using G = decltype(g);
    g_solve_launches = 0;
    if (n < 0) return fail(-3, "n must not be negative");
    if (max_nodes < 1) return fail(-3, "max_nodes must be at least 1");
    if (launch_nodes != 0 && launch_nodes < 4) return fail(-3, "launch_nodes: 0 (the default slice) or at least 4");
    if (table_entries < (1ull << SV_MIN_TABLE_BITS) || (table_entries & (table_entries - 1)))
      return fail(-3, "solve table: a power-of-two number of entries, at least 2^16");
    if (n == 0) return 0;
    if (!boards_dev || !players_dev || !scores_dev || !table_dev || !work_dev) return fail(-1, "null argument");
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t slice = launch_nodes ? launch_nodes : SV_LAUNCH_STEPS;
    const SvWork w = sv_work<G>(work_dev, n);
    const uint64_t tmask = table_entries - 1;
    uint32_t head[4] = {0, 0, 0xffffffffu, 0};
    HIP_TRY(hipMemsetAsync(work_dev, 0, 16 + (size_t)n * 8, s));
    HIP_TRY(hipMemcpyAsync(work_dev, head, sizeof(head), hipMemcpyHostToDevice, s));
    TRY(launch(k_solve_init<G>, w.N, SV_THREADS, s, boards_dev, players_dev, w, table_dev, tmask));
    HIP_TRY(hipMemcpyAsync(head, work_dev, sizeof(head), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (head[1])
      return fail(-3, "position " + std::to_string(head[2]) + " is finished (a full board or a line): " +
                          std::to_string(head[1]) + " such in the batch");
    // a launch with an item still running makes at least (slice - 1) / 2 moves for that item's position (a step
    // that makes no move pops a level a move pushed), so the budget ends the loop
    const uint64_t max_launches = max_nodes / ((slice - 1) / 2) + 2;
    for (uint64_t l = 0; l < max_launches; ++l) {
      HIP_TRY(hipMemsetAsync(work_dev, 0, 4, s));
      TRY(launch(k_solve_step<G>, w.N, SV_THREADS, s, w, table_dev, tmask, max_nodes, slice));
      HIP_TRY(hipMemcpyAsync(head, work_dev, 4, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      ++g_solve_launches;
      if (head[0] == 0) break;
    }
    TRY(launch(k_solve_fold<G>, n, SV_THREADS, s, boards_dev, w, n, scores_dev, nodes_dev));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
  });
}

int spmcts_table_net(int32_t game, int32_t width, int32_t height, const void *leaves_dev, int32_t leaf_format,
                     int32_t leaf_layout, int32_t n, uint64_t salt, const uint64_t *salts_dev, float *probs_dev,
                     float *values_dev, spmcts_stream stream) {
  if (n <= 0) return 0;
  return with_game(game, width, height, [&](auto g) {
    return launch(k_table_net<decltype(g)>, n, 128, (hipStream_t)stream, leaves_dev, leaf_format, leaf_layout, n, salt,
                  salts_dev, probs_dev, values_dev);
  });
}

int spmcts_copy_probe(const void *src_dev, void *dst_dev, uint64_t bytes, spmcts_stream stream) {
  return launch(k_copy_probe, 4096 * 256, 256, (hipStream_t)stream, (const float4 *)src_dev, (float4 *)dst_dev,
                bytes / 16);  // 4096 blocks, grid-stride
}

}  // extern "C"
