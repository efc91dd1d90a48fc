/*
 * spmcts.h — C ABI of the MI355X-native batched self-play MCTS arena.
 *
 * The arena replaces the per-process Python object tree of the reference
 * (reubenvanammers/self_play_reinforcement_learning, games/algos/mcts.py) and
 * the per-game episode loop that drives it (games/algos/selfplayworker.py
 * SelfPlayer, fed by games/algos/self_play_parallel.py SelfPlayScheduler).
 * Thousands of trees live in one device-resident struct-of-arrays node store;
 * every entry point below launches HIP kernels for gfx950 on the caller's
 * stream.  The reference is pure Python, so there is no C FFI to bind: the
 * drop-in boundary is the reference's own Python policy API (MCTreeSearch /
 * SelfPlayScheduler / Memory), re-implemented in
 * self_play_reinforcement_learning_amd/ on top of these functions via ctypes.
 * Each function cites the reference interface it replaces.
 *
 * Conventions
 *   - All array arguments named *_dev are DEVICE pointers owned by the caller
 *     (torch tensors); the arena owns only its node store and game state.
 *   - `stream` is a hipStream_t (NULL = legacy default stream).  Calls are
 *     stream-ordered; none synchronises unless stated ("(sync)").
 *   - Return value: 0 on success, < 0 on error; spmcts_last_error() returns a
 *     thread-local message.  Errors raised on the device (node-pool
 *     exhaustion, RNG tape exhaustion, invalid action) are sticky flags read by
 *     spmcts_check() / spmcts_get_counters().
 *   - No exceptions cross the ABI.  One arena per device per process; calls on
 *     one arena must be serialised by the host (single writer).
 *
 * Board frame: +1 = the tree's owner (each MCTreeSearch sees itself as +1,
 * selfplayworker.py:175-176).  Boards are int8/int64 [W][H] = [column][row],
 * row 0 = bottom (connect4env.py:22).
 */
#ifndef SPMCTS_H
#define SPMCTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spmcts_arena spmcts_arena; /* opaque */
typedef void *spmcts_stream;              /* hipStream_t */

enum spmcts_game { SPMCTS_CONNECT4 = 0, SPMCTS_TICTACTOE = 1 };
enum spmcts_rng_mode {
  SPMCTS_RNG_PHILOX = 0, /* rocRAND Philox4x32-10, one subsequence per tree          */
  SPMCTS_RNG_TAPE = 1    /* replay injected per-tree double streams (parity mode)     */
};
enum spmcts_leaf_format {
  SPMCTS_LEAF_F32 = 0,      /* float  planes [B,3,W,H] (empty, own, enemy)  modules.py:115-125 */
  SPMCTS_LEAF_F16 = 1,      /* half   planes                                                   */
  SPMCTS_LEAF_BF16 = 2,     /* bf16   planes                                                   */
  SPMCTS_LEAF_BOARD_I64 = 3 /* int64 boards [B,W,H] = state * mover, for net.forward(s)        */
};
enum spmcts_layout { SPMCTS_NCHW = 0, SPMCTS_NHWC = 1 };
/* What plays a tree's moves in games mode (games/general/hardcoded_players.py) */
enum spmcts_player_kind {
  SPMCTS_PLAYER_MCTS = 0,     /* MCTreeSearch (the default)                                 */
  SPMCTS_PLAYER_RANDOM = 1,   /* Random: uniform over valid moves (hardcoded_players.py:36-56) */
  SPMCTS_PLAYER_LOOKAHEAD = 2,/* OneStepLookahead: win / block / random (:8-33)               */
  SPMCTS_PLAYER_NEGAMAX = 3   /* exact depth-limited negamax (no reference form): uniform over the moves with
                                 the best code of spmcts_negamax_batch at the tree's depth        */
};

/* return code of the tower entry points (spmcts_tower_forward*, spmcts_tower_heads*): an environment switch
 * of the A/B library (SPMCTS_TOWER_C256, SPMCTS_HEADS, SPMCTS_HEADS_C256 -- whatever its value; `make ab`
 * builds libspmcts_ab.so, which reads them) is set while the product library is loaded: refused instead of
 * silently ignored */
#define SPMCTS_ERR_AB_SWITCH (-5)

/* device error flags (sticky) */
#define SPMCTS_ERR_POOL 0x1u      /* a tree ran out of node blocks                 */
#define SPMCTS_ERR_TAPE 0x2u      /* RNG tape exhausted                            */
#define SPMCTS_ERR_NOCHILD 0x4u   /* select reached a node whose children are all invalid */
#define SPMCTS_ERR_ACTION 0x8u    /* play_action on an illegal action              */
#define SPMCTS_ERR_STATE 0x10u    /* inconsistent tree state (also: a move chosen, or a root advanced, while
                                     the tree's search still has sims to start or replies to make) */
#define SPMCTS_ERR_EXPORT 0x20u   /* move export ring overflow                     */

typedef struct spmcts_config {
  int32_t game;            /* enum spmcts_game                                               */
  int32_t width, height;   /* Connect4 7x6, 6x5, 8x7; TicTacToe 3x3 (only these are instantiated) */
  int32_t n_trees;         /* tree slots (games mode needs >= 2*n_games)                     */
  int32_t n_games;         /* game slots for the self-play state machine (0 = tree mode only) */
  int32_t iterations;      /* simulations per move (mcts.py:125, sizes the node pool)        */
  int32_t blocks_per_tree; /* node blocks per tree; 0 = worst case from iterations          */
  int32_t rng_mode;        /* enum spmcts_rng_mode                                            */
  int32_t strong_play;     /* mcts.py:133, :307-311                                           */
  int32_t evaluate;        /* mcts.py:273-274 (temp / 20)                                     */
  int32_t leaf_format;     /* enum spmcts_leaf_format                                         */
  int32_t leaf_layout;     /* enum spmcts_layout (planes only)                                */
  int32_t compact;         /* 1: leaf rows compacted in tree order; 0: one row per active slot */
  int32_t search_threads;  /* K simulations in flight per tree with virtual loss (the reference's
                              thread_count, mcts.py:328-331, :345); 0 or 1 = sequential search.
                              Leaf rows per select = n_trees * K; K > 1 keeps a per-node vl.  */
  double cpuct;            /* MCNode.cpuct = 4 (mcts.py:25)                                   */
  double x_noise;          /* MCNode.x = 0.25 (mcts.py:25)                                    */
  double alpha;            /* Dirichlet alpha (mcts.py:135)                                   */
  uint64_t seed;           /* Philox key                                                      */
  uint64_t subsequence0;   /* Philox subsequence of tree 0 (rank * n_trees for multi-GPU)     */
} spmcts_config;

typedef struct spmcts_counters {
  int64_t sims;                /* simulations completed (search_node calls)                  */
  int64_t nn_leaves;           /* leaves sent to the network (search + play_action)          */
  int64_t terminal_leaves;     /* simulations that ended on a terminal leaf (no NN)          */
  int64_t depth_sum;           /* sum over sims of edges descended (select depth D)          */
  int64_t set_node_expansions; /* play_action expansions (mcts.py:203-208)                   */
  int64_t moves;               /* moves played by searching trees (= Move records)           */
  int64_t games_finished;
  int64_t positions_exported;  /* Move records exported                                      */
  int64_t results[2][3];       /* [swap_sides][win, draw, loss] (self_play_parallel.py:302-327) */
  int64_t blocks_in_use_max;   /* peak node blocks used by any tree (high-water since creation) */
  uint32_t error_flags;
  uint32_t reserved;
  int64_t leaked_sims;         /* threaded mode: sims that found every child invalid or locked and
                                  ended without a backup, their virtual loss left in place
                                  (mcts.py:349-354); sims + leaked_sims = searches x iterations */
  int64_t compactions;         /* subtree recyclings (node-store compactions before a search; only
                                  when blocks_per_tree is below the worst case)                 */
  int64_t nn_rows;             /* network rows emitted (= nn_leaves unless leaf dedup is on)  */
  int64_t cache_rows;          /* leaf rows served from the evaluation cache (spmcts_set_eval_cache) */
} spmcts_counters;

/* ---- library ------------------------------------------------------------ */
int spmcts_version(void);
const char *spmcts_last_error(void);
/* (sync) size of the device allocation an arena with this config needs */
int spmcts_arena_bytes(const spmcts_config *cfg, uint64_t *bytes_out);

/* ---- arena lifetime ------------------------------------------------------ */
/* Replaces MCTreeSearch.__init__ (mcts.py:119-164) for many trees at once. */
int spmcts_arena_create(const spmcts_config *cfg, int device, spmcts_arena **out);
int spmcts_arena_destroy(spmcts_arena *h);
/* geometry: A = actions, W, H, blocks per tree, lanes per tree */
int spmcts_arena_geometry(const spmcts_arena *h, int32_t *A, int32_t *W, int32_t *H, int32_t *blocks_per_tree,
                          int32_t *n_trees, int32_t *n_games);

/* Priors of the empty-board root: `self.network(base_state)` in MCTreeSearch.reset
 * (mcts.py:167-170).  Constant per network weights; used by every tree/game reset. */
int spmcts_set_root_prior(spmcts_arena *h, const float *probs_dev /*[A]*/, spmcts_stream stream);
/* Parity mode: per-tree flat double streams, consumed in the reference's call
 * order (dirichlet(A) per search, rand(A) per select level, one uniform per
 * np.random.choice).  offsets_dev[T+1] (int64) index into tape_dev. */
int spmcts_set_tape(spmcts_arena *h, const double *tape_dev, const int64_t *offsets_dev, spmcts_stream stream);

/* ---- tree-level API (the MCTreeSearch policy protocol) -------------------- */
/* MCTreeSearch.reset(player) (mcts.py:166-174): new root on the empty board.
 * priors_dev: NULL = the arena's root prior, else [n][A] per tree. */
int spmcts_tree_reset(spmcts_arena *h, const int32_t *trees_dev, const int8_t *root_player_dev,
                      const float *priors_dev, int32_t n, spmcts_stream stream);
/* MCTreeSearch.search prologue (mcts.py:323-327): Dirichlet noise on the roots of
 * the listed trees; they become the active set for spmcts_select. */
int spmcts_search_begin(spmcts_arena *h, const int32_t *trees_dev, int32_t n, spmcts_stream stream);
/* One search_node (mcts.py:340-367) for every active tree: PUCT select with
 * jitter, terminal leaves backed up in place, other leaves written to the leaf
 * batch (rows in tree order).  leaf_count_dev int32[3] = {rows, network-0 rows,
 * network-1 rows}: network-0 leaves occupy rows [0, n0), network-1 leaves rows
 * [seg1, seg1 + n1) (see spmcts_set_tree_players; single-network arenas: n1 = 0). */
int spmcts_select(spmcts_arena *h, void *leaves_dev, int32_t *leaf_count_dev, spmcts_stream stream);
/* spmcts_select in two launches (for per-kernel timing): the tree walk alone,
 * then the leaf-row compaction + encode of whatever is pending. */
int spmcts_select_tree(spmcts_arena *h, spmcts_stream stream);
int spmcts_leaf_rows(spmcts_arena *h, void *leaves_dev, int32_t *leaf_count_dev, spmcts_stream stream);
/* _expand_node tail + backup (mcts.py:316-321, :94-98, :361-364) for the rows of
 * the last select / play_action: create children with the network's priors,
 * back the value up the path.  probs_dev [rows][A] f32, values_dev [rows] f32
 * (network outputs from the mover's perspective, modules.py:109-112). */
int spmcts_expand(spmcts_arena *h, const float *probs_dev, const float *values_dev, spmcts_stream stream);
/* Two-network arenas: network-0 outputs indexed by row, network-1 outputs by row - seg1. */
int spmcts_expand2(spmcts_arena *h, const float *probs0_dev, const float *values0_dev, const float *probs1_dev,
                   const float *values1_dev, spmcts_stream stream);
/* (sync) Per-tree players, for evaluation games between two networks or against a
 * hard-coded player (SelfPlayWorker.set_up_policies evaluate=True, selfplayworker.py:68-94;
 * compare_models, self_play_parallel.py:355-379).  Host arrays of n_trees entries, each
 * may be NULL (default): nets = network id 0/1 of the tree's leaves; kinds = enum
 * spmcts_player_kind; budgets = simulations per search (MCTreeSearch.iterations of that
 * player; < 0 = unlimited).  Network-1 leaves are placed from row seg1 = #network-0 trees.
 * For a tree of kind SPMCTS_PLAYER_NEGAMAX budgets[t] is its depth, 1 .. 6; anything else (budgets NULL
 * included) returns -3.  The first call that names such a tree allocates the arena's int8 [n_trees][A] score
 * rows; from then on spmcts_games_end_ply solves the positions of the games whose mover is such a tree before
 * it plays the ply.  An arena without such a tree launches and allocates nothing more than before. */
int spmcts_set_tree_players(spmcts_arena *h, const uint8_t *nets, const uint8_t *kinds, const int32_t *budgets);
/* (sync) Per-tree search settings: each side of an evaluation game searches with its own
 * MCTreeSearch kwargs (selfplayworker.py:71-81 builds the opponent from its own container;
 * mcts.py:119-136): alpha = Dirichlet alpha of the root noise (mcts.py:49-53, > 0),
 * strong_play = terminal-value shaping (mcts.py:305-311), search_threads = sims in flight
 * (thread_count, mcts.py:328-331; 1 .. the arena's search_threads).  Host arrays of n_trees
 * entries; NULL = unchanged (defaults: the arena config's values). */
int spmcts_set_tree_search(spmcts_arena *h, const double *alpha, const uint8_t *strong_play,
                           const int32_t *search_threads);
int spmcts_arena_segments(const spmcts_arena *h, int32_t *seg1);
/* Empty-board root prior of network `net` (0 / 1), used by resets of that network's trees. */
int spmcts_set_root_prior_net(spmcts_arena *h, int32_t net, const float *probs_dev, spmcts_stream stream);
/* Games mode: keep Move records (play_episode update=True, the default) or not (evaluation games). */
int spmcts_games_set_record(spmcts_arena *h, int32_t record);
/* Batch leaf dedup (search_threads > 1 only; no effect with 1): pending leaves whose
 * network input is the same ((own, opp) stones from the mover's view, same network) share one
 * leaf row, so each distinct position of a simulation step is evaluated once and every leaf reads
 * its row's outputs.  The reference evaluates each leaf separately (InferenceWorker,
 * inference_worker.py:89-119); with a deterministic, batch-independent evaluator the outputs each
 * leaf receives are unchanged.  Off by default; leave it off for evaluators that give rows of
 * different trees different networks (per-row salts).  Leaf counts then count rows, not leaves. */
int spmcts_set_leaf_dedup(spmcts_arena *h, int32_t on);
/* Cross-lane leaf dedup (round 6).  Pair `h` (a follower lane) with `leader` (another arena of the same game,
 * device and search_threads > 1, both single-network; NULL unpairs): in each simulation step
 * (spmcts_select / spmcts_leaf_rows, with leaf dedup on in both) a follower's pending leaf whose network input
 * the leader evaluates in the SAME step takes the leader's row instead of one of its own -- the lanes of
 * engine.LanedEngine run in lock step, and the reference evaluates every leaf (inference_worker.py:89-119),
 * so with a deterministic, batch-independent evaluator each leaf's outputs are unchanged.  Contract: per step
 * the leader's rows are built before the follower's (host order), and the follower's expand is
 * preceded by spmcts_peer_push; the end-of-ply expansions (spmcts_play_action / spmcts_games_end_ply) stay lane-local.
 * Leaf counts of the follower count its own rows (the leader-served rows follow them). */
int spmcts_set_leaf_peer(spmcts_arena *h, spmcts_arena *leader);
/* Before a follower's expand of a simulation step: on leader_stream (after the leader's network outputs of
 * the step) the leader's rows are copied into the follower's leader-served rows of probs_dev / values_dev
 * (k_peer_push), and `stream` waits for them (events).  A no-op when the step had no leader-served rows
 * (unpaired, dedup off, an end-of-ply step); a follower's spmcts_expand / spmcts_expand2 after a
 * leader-served step without it fails (-4). */
int spmcts_peer_push(spmcts_arena *h, float *probs_dev, float *values_dev, const float *leader_probs_dev,
                     const float *leader_values_dev, spmcts_stream stream, spmcts_stream leader_stream);
/* Sim cap (search_threads > 1): the simulations one tree may start in one kernel launch.  A tree that reaches
 * it pauses at a simulation boundary and the next launch resumes its slot cycle at exactly that point, so a
 * tree whose sims end on terminal leaves (which wait for no network) no longer holds up the launch for every
 * other tree; the operations, their order and the RNG draws are unchanged, so results are bit-identical for
 * every cap.  0 = off; 0 < cap < 2 * search_threads is refused (-3): from 2 * search_threads on a search
 * takes no more launches than without a cap.  Default: on, 2 * search_threads. */
int spmcts_set_sim_cap(spmcts_arena *h, int32_t cap);
/* (sync) tree-launches that paused at the sim cap since the arena was created */
int spmcts_get_sim_pauses(spmcts_arena *h, int64_t *pauses_out);
/* Evaluation cache (round 6; search_threads > 1 with leaf dedup on): the network
 * outputs of the arena's own leaf rows are kept, keyed like leaf dedup ((own, opp) stones from the mover's
 * view), for `window` generations -- one generation per spmcts_games_begin_ply / spmcts_search_begin, so
 * window 1 = within the ply (search) that evaluated them.  An owner leaf whose key is cached takes a row
 * after the network rows (and a follower's leader-served rows) and, at spmcts_expand / spmcts_expand2, the
 * cached outputs are written into that row of probs / values (k_cache_io), and the rows the network (or the
 * leader) filled go into the cache.  Two-network arenas keep the networks' keys apart (served rows follow each
 * segment's network rows); a follower lane whose leader runs a cache of the same window uses the leader's
 * table.  The reference evaluates every leaf (inference_worker.py:89-119); with
 * a deterministic, batch-independent evaluator every leaf still receives exactly its own outputs.  After the
 * network's weights change call spmcts_eval_cache_clear.  window 0 turns it off; capacity_log2 = log2 of the
 * table's entries (10..28; 0 = four times the rows window + 1 plies can hold, at most 2^26), allocated here
 * (one 64-byte record per entry + 4 bytes per pending slot, outside spmcts_arena_bytes).  (sync) */
int spmcts_set_eval_cache(spmcts_arena *h, int32_t window, int32_t capacity_log2);
/* Every cached output leaves the window (host-side generation step; no device work). */
int spmcts_eval_cache_clear(spmcts_arena *h);
/* MCTreeSearch._play (mcts.py:272-299) for the active trees + remove_noise:
 * visit-count^(1/temp) distribution, np.random.choice semantics, Move record.
 * Outputs per active tree i: actions_dev[i], states_dev[i][W*H] (int8, tree
 * frame), tree_probs_dev[i][A], q_dev[i] (double; exported as a float32 tensor
 * unless q_f64_dev[i]), recorded_dev[i] (0 = numpy ValueError fallback). */
int spmcts_search_end(spmcts_arena *h, double temp, int32_t *actions_dev, int8_t *states_dev, float *tree_probs_dev,
                      double *q_dev, uint8_t *q_f64_dev, uint8_t *recorded_dev, spmcts_stream stream);
/* MCTreeSearch.play_action/_set_node (mcts.py:188-209): advance each listed
 * root; an unvisited child is expanded (rows for the network) and backed up. */
int spmcts_play_action(spmcts_arena *h, const int32_t *trees_dev, const int32_t *actions_dev, int32_t n,
                       void *leaves_dev, int32_t *leaf_count_dev, spmcts_stream stream);
/* Tree id of every leaf row of the last select / play_action / games_end_ply
 * (rows in tree order; trees_dev has room for n_trees entries). */
int spmcts_leaf_trees(spmcts_arena *h, int32_t *trees_dev, spmcts_stream stream);
/* (sync) root statistics of one tree: children n/w/p (A each), root n/w, player, board */
int spmcts_root_stats(spmcts_arena *h, int32_t tree, int32_t *child_n, double *child_w, float *child_p,
                      int32_t *root_n, double *root_w, int32_t *root_player, int8_t *board /*[W*H]*/);
/* spmcts_root_stats of the n listed trees into device arrays, with no host synchronisation: the root's
 * children's visit counts, w and priors (the n, w, p that _play reads, mcts.py:272-277; [n][A] each), the
 * root's own n and w (its q, mcts.py:59-62), the player to move ([n] each) and the root board (int8 [n][W*H],
 * tree frame).  The values are those of spmcts_root_stats, bit for bit; any output may be NULL.  A tree id
 * outside the arena raises SPMCTS_ERR_STATE. */
int spmcts_root_stats_batch(spmcts_arena *h, const int32_t *trees_dev, int32_t n, int32_t *child_n_dev,
                            double *child_w_dev, float *child_p_dev, int32_t *root_n_dev, double *root_w_dev,
                            int8_t *root_player_dev, int8_t *boards_dev, spmcts_stream stream);

/* ---- reading the trees below the root (read-only; csrc/arena_tree.h) ------- */
/* The principal variation of each of the n listed trees, queued on the stream with no host synchronisation: from
 * the active root, the child with the largest n (the lowest action on ties: ns.index(max(ns)), mcts.py:290-295),
 * while that n is at least max(min_visits, 1), the node has a child block, the game goes on and fewer than
 * max_len (1 .. W*H) moves are out.  Per tree i: pv int8 [n][max_len] (-1 past the end); pv_n, pv_vl int32, pv_w
 * double, pv_p float [n][max_len], the chosen children's fields as stored (entries past the end are not written;
 * vl is 0 in an arena with search_threads 1, which keeps no virtual loss); pv_len int32 [n]; pv_end uint8 [n]
 * (0: cut at max_len, 1: the last node has no child with enough visits, 2: the last move ended the game);
 * end_board int8 [n][W*H], the board after the last move (tree frame, cells as spmcts_root_stats_batch).  Any
 * output may be NULL.  A tree id outside the arena raises SPMCTS_ERR_STATE and leaves its row untouched.
 * -1: null handle; -3: n < 0, max_len outside [1, W*H], min_visits < 0; n == 0 launches nothing. */
int spmcts_tree_pv_batch(spmcts_arena *h, const int32_t *trees_dev, int32_t n, int32_t max_len, int32_t min_visits,
                         int8_t *pv_dev, int32_t *pv_n_dev, int32_t *pv_vl_dev, double *pv_w_dev, float *pv_p_dev,
                         int32_t *pv_len_dev, uint8_t *pv_end_dev, int8_t *end_board_dev, spmcts_stream stream);
/* Bytes of the work buffer spmcts_tree_export_batch needs for n trees of max_nodes entries (24 per queue slot: the
 * queued node's two board masks and its child block and depth; plus 8 * (W*H + 1) per tree for the counting walk). */
int spmcts_tree_export_work_bytes(spmcts_arena *h, int32_t n, int32_t max_nodes, uint64_t *bytes_out);
/* The subtree under the active root of each of the n listed trees in breadth-first order, no host synchronisation.
 * Entry 0 is the root; for entry e in order, its children with n >= min_visits (0: every child of every expanded
 * node, invalid ones included) whose depth is within max_depth (< 0: no limit) follow in ascending action order.
 * Per tree, [n][max_nodes] each: parent int32 (index in the row, -1 for the root), action int8 (-1 for the root),
 * depth int16, node_n / node_vl int32, node_w double, node_p float (as stored; vl as in spmcts_tree_pv_batch),
 * player int8 (root player * (-1)^depth: MCNode.player), flags uint8 (bit 0: expanded, bit 1: valid, set for the
 * root, bit 2: the move into the node ended the game).  count int32 [n]: the nodes that qualify; where it exceeds
 * max_nodes exactly the first max_nodes are written and nothing past them is touched (not an error: call again
 * with more room).  Any output may be NULL.  work_dev: device scratch of spmcts_tree_export_work_bytes bytes,
 * 8-byte aligned, no initial contents needed.  A tree id outside the arena raises SPMCTS_ERR_STATE and leaves
 * its row untouched.  -1: null handle / trees / work; -3: n < 0, max_nodes < 1, min_visits < 0, work too small. */
int spmcts_tree_export_batch(spmcts_arena *h, const int32_t *trees_dev, int32_t n, int32_t max_nodes,
                             int32_t min_visits, int32_t max_depth, int32_t *parent_dev, int8_t *action_dev,
                             int16_t *depth_dev, int32_t *node_n_dev, int32_t *node_vl_dev, double *node_w_dev,
                             float *node_p_dev, int8_t *player_dev, uint8_t *flags_dev, int32_t *count_dev,
                             void *work_dev, uint64_t work_bytes, spmcts_stream stream);
/* What each of the n listed trees proves about the exact score s of its root position ("exact solver to the end
 * of the game" below: e, the position's empty cells, if a move wins, 0 if it fills the board, else -s(child),
 * maximised over the legal moves), queued on the stream with no host synchronisation: a minimax over the stored
 * tree (score-bounded MCTS).  A legal move that ends the game is worth e or 0; a move into a node with a child
 * block is worth [-hi(child), -lo(child)]; any other move [-(e - 1), e - 2]; a node's lo / hi are the maxima over
 * its legal moves.  A root without a child block has its moves classified from the board alone.  The root must be
 * unfinished, as for the solvers.  Per tree i: lo, hi int8 [n], lo <= s <= hi (lo == hi: solved); move_lo,
 * move_hi int8 [n][A], the same per root move (-128 in both for an illegal move); best int8 [n], the lowest action
 * with move_lo == lo (it secures lo); empty int8 [n], e of the root; nodes int32 [n], the expanded nodes the walk
 * entered.  Any output may be NULL.  The walk's stack lives in the kernel's LDS: there is no work buffer.  A tree
 * id outside the arena raises SPMCTS_ERR_STATE and leaves its row untouched (so does a store whose blocks do not
 * form a tree).  -1: null handle / trees; -3: n < 0; n == 0 launches nothing. */
int spmcts_tree_bounds_batch(spmcts_arena *h, const int32_t *trees_dev, int32_t n, int8_t *lo_dev, int8_t *hi_dev,
                             int8_t *move_lo_dev, int8_t *move_hi_dev, int8_t *best_dev, int8_t *empty_dev,
                             int32_t *nodes_dev, spmcts_stream stream);

/* ---- proof-guided play ------------------------------------------------------ */
/* Let the move choice use what the tree has proved (off by default).  `on` uint8 [T]: the trees it is on for, or
 * NULL: every tree.  Synchronises; the first call that switches a tree on allocates the arrays below.  Before a
 * move is chosen (spmcts_games_end_ply: each active game's mover tree; spmcts_search_end: the active trees), the
 * walk of spmcts_tree_bounds_batch gives the root's lo, hi and its moves' move_lo, move_hi, and the keep set
 *   S = { legal a : move_lo[a] == lo }   if lo > 0 (a win is secured) or lo == hi (the root is solved),
 *   S = { legal a : move_hi[a] >= lo }   otherwise (moves proved worse than what another secures are dropped).
 * S is never empty and holds no illegal move.  The visit-count weights of the moves outside S are set to 0; if no
 * move of S has a visit, each weighs 1; normalisation, validation, the one random draw and the argmax fallback (over
 * S) are as without the feature, and the Move record takes the masked probabilities.  A tree whose flag is off, a
 * tree of a hard-coded player and a game in its opening book choose as before, bit for bit. */
int spmcts_set_proof_play(spmcts_arena *h, const uint8_t *on);
/* The verdict of the n listed trees as they stand, queued on the stream with no host synchronisation, whatever
 * their flags: keep uint32 [n] (bit a: move a is in S), lo, hi int8 [n].  Read-only, at any point of a search.  Any
 * output may be NULL.  A tree id outside the arena raises SPMCTS_ERR_STATE and leaves its row untouched.
 * -1: null handle / trees; -3: n < 0; n == 0 launches nothing. */
int spmcts_tree_proof_moves_batch(spmcts_arena *h, const int32_t *trees_dev, int32_t n, uint32_t *keep_dev,
                                  int8_t *lo_dev, int8_t *hi_dev, spmcts_stream stream);
/* What the last spmcts_games_end_ply / spmcts_search_end wrote, per tree [T]: keep 0xffffffff (no restriction) and
 * lo = hi = -128 for a tree the feature did not apply to; a tree that chose no move then keeps its earlier row.
 * Any output may be NULL.  -4: proof play is off. */
int spmcts_proof_last(spmcts_arena *h, uint32_t *keep_dev, int8_t *lo_dev, int8_t *hi_dev, spmcts_stream stream);
/* Counts since the arrays were allocated, int64 [SPMCTS_PROOF_NSTAT] (synchronises): [0] plies chosen with the
 * feature on, [1] those with a solved root, [2] with a secured win (lo > 0), [3] with S smaller than the legal
 * set; [4] trees spmcts_proof_stop stopped, [5] the sims they did not start (limit - started at the stop). */
enum { SPMCTS_PROOF_NSTAT = 6 };
int spmcts_get_proof_stats(spmcts_arena *h, int64_t *out);
/* A searching tree whose root is now solved (lo == hi) starts no more sims, queued on the stream with no host
 * synchronisation, between two simulation steps: for every tree with proof play on that is searching (started <
 * min(budget, iterations)) and not paused inside a fill by the sim cap (such a tree is looked at again by the next
 * call), the walk; if lo == hi the tree is left as a search whose sims have all been started: its pending slots are
 * replied by the following expands, it selects no more, and the move choice finds it complete.  Over the arena
 * sims + leaked_sims + stats[5] == searches x iterations.  -4: search_threads <= 1, or proof play is off. */
int spmcts_proof_stop(spmcts_arena *h, spmcts_stream stream);
/* Per tree, int32 [T]: the searches of the tree that spmcts_proof_stop has stopped so far (their sum is stats[4]),
 * queued on the stream with no host synchronisation; all 0 where proof play was never on. */
int spmcts_proof_stopped(spmcts_arena *h, int32_t *count_dev, spmcts_stream stream);

/* ---- stored score bounds ---------------------------------------------------- */
/* The maintenance switch of the stored bounds.  `on` uint8 [T] must be all 0: the call starts the maintenance of the
 * bounds for the whole arena (it cannot be switched off again).  A call with any flag set (NULL included) returns -2
 * and changes nothing: which trees' searches READ the bounds is spmcts_set_solver_rules' business below, and without
 * it no search does.  From the first call on every
 * entry j of every child block carries move_lo / move_hi of the move into child j as int8, seen from the block's
 * own node -- the values the walk of spmcts_tree_bounds_batch computes for that move -- in bytes of the node record
 * that were padding, so no layout, size or offset changes.  A new block is stamped from its board alone (a winning
 * move [e, e], a board-filling move [0, 0], an illegal move -128, any other move [-(e - 1), e - 2]); the expansion
 * that created it then rewrites the leaf's entry in its parent's block as [-hi, -lo] of the new block and goes on
 * bottom-up along the expansion's path while an entry changes, up to the entries of the active root's children.
 * Between any two launches, mid-search included, the stored entries of every block reachable from the active root
 * equal the walk's values on the tree as it stands.  Without search rules the search does not read them: counters,
 * visit counts, Move records and results are bit-identical with and without.  With the bounds stored,
 * spmcts_set_proof_play's verdict before a move choice, spmcts_tree_proof_moves_batch and spmcts_proof_stop read the
 * root's block (one read) and walk nothing; a root without a child block is classified from its board as before.
 * spmcts_tree_bounds_batch keeps walking: it is the independent check.
 * The first call is legal only while no tree holds more than its root block (before the first search): -4
 * otherwise.  It stamps every fresh tree's root block.  Every call synchronises.  -1: null handle; -2: a use flag
 * is set. */
int spmcts_set_solver_search(spmcts_arena *h, const uint8_t *on);
/* Solver-aware search (off by default): the search rules that read the stored bounds, per tree.  `rules` uint8 [T],
 * a mask of the two bits below, or NULL: every rule off.  At a node X with `player` to move, with mlo[j] / mhi[j]
 * the stored entries of X's child block and lo(X) their largest mlo:
 *   SPMCTS_SOLVER_REFUTE  a child j with mhi[j] < lo(X) scores like an invalid or locked child (-1e10): it cannot
 *                         reach what a sibling already secures.  The move that secures lo(X) is never refuted, so
 *                         only locks can leave a select without a child (a leak, as before);
 *   SPMCTS_SOLVER_PROVED  if the chosen child a has a child block and mlo[a] == mhi[a] = s, the sim ends there like
 *                         a terminal one: value sign(s) * player -- for a strong_play tree and s != 0,
 *                         (1.18 - 9 * (cells - |s| + 1) / 350.0) * sign(s) * player, what the winning move itself
 *                         would back up -- n + 1 and w + value on the path and on a, the path's virtual loss removed.
 *                         It counts in sims and depth_sum, not in terminal_leaves, and buys no network row.
 * A tree without bits searches bit-identically to an arena that only stores the bounds.  The stored-bounds
 * invariant holds with the rules on (they write no bound).  Synchronises; takes effect at the next launch.
 * -1: null handle; -3: a bit outside the two; -4: the arena keeps no stored bounds (spmcts_set_solver_search). */
enum { SPMCTS_SOLVER_REFUTE = 1, SPMCTS_SOLVER_PROVED = 2 };
int spmcts_set_solver_rules(spmcts_arena *h, const uint8_t *rules);
/* Counts since the first spmcts_set_solver_rules with a bit set, summed over the trees, int64
 * [SPMCTS_SOLVER_NSTAT] (synchronises): [0] sims ended by SPMCTS_SOLVER_PROVED, [1] select levels at which
 * SPMCTS_SOLVER_REFUTE removed at least one child that was otherwise valid.  All zeros before that call. */
enum { SPMCTS_SOLVER_NSTAT = 2 };
int spmcts_get_solver_stats(spmcts_arena *h, int64_t *out);
/* The same per tree, int64 [T][SPMCTS_SOLVER_NSTAT] to device memory, queued on the stream with no host
 * synchronisation. */
int spmcts_solver_stats_trees(spmcts_arena *h, int64_t *out_dev, spmcts_stream stream);
/* Where each tree's search stands, queued on the stream with no host synchronisation, int32 [T] each, either may be
 * NULL: started, the search_node calls the tree's current search has started (0x3fffffff: no search in progress,
 * or stopped by spmcts_proof_stop); resume, the slot its cycle goes on at * 2 + 1 if the sim cap paused it inside a
 * fill (the state spmcts_proof_stop passes over).  Read-only. */
int spmcts_search_progress(spmcts_arena *h, int32_t *started_dev, int32_t *resume_dev, spmcts_stream stream);
/* spmcts_tree_export_batch (the same arguments, the same kernel) with two more outputs, int8 [n][max_nodes] each and
 * nullable like the others: the stored entry of each exported node, i.e. move_lo / move_hi of the move into it seen
 * from its parent; -128 in both for the root's row and for an illegal move.  -4: the arena keeps no stored bounds
 * (spmcts_set_solver_search). */
int spmcts_tree_export_bounds_batch(spmcts_arena *h, const int32_t *trees_dev, int32_t n, int32_t max_nodes,
                                    int32_t min_visits, int32_t max_depth, int32_t *parent_dev, int8_t *action_dev,
                                    int16_t *depth_dev, int32_t *node_n_dev, int32_t *node_vl_dev, double *node_w_dev,
                                    float *node_p_dev, int8_t *player_dev, uint8_t *flags_dev, int32_t *count_dev,
                                    int8_t *move_lo_dev, int8_t *move_hi_dev, void *work_dev, uint64_t work_bytes,
                                    spmcts_stream stream);

/* ---- mirror symmetry ---------------------------------------------------------- */
/* Every board here is left-right symmetric.  M maps cell (x, y) to (W-1-x, y); the action map m is a -> W-1-a on the
 * gravity boards and a = x*H + y -> (W-1-x)*H + y on tictactoe.  With SPMCTS_SYM_MIRROR a leaf's network input
 * (own, opp) is put in canonical form before it is keyed and encoded: it is replaced by (M own, M opp) iff that pair
 * is smaller, as two unsigned 64-bit masks of the board.h layout, own first (a self-symmetric position is never
 * flipped).  Leaf rows, outputs, peer rows and cache records are canonical; a flipped leaf's expansion reads prior a
 * from prob m(a) of its row, so node priors, the sim cap's stash, Move records and every read-out stay in the tree's
 * orientation.  The search then runs the function f(x) = g(x) where x is not flipped, else m(g(Mx).p), g(Mx).v: a
 * position and its mirror image share one row, and f(Mx) = m(f(x)) bit for bit.  Mode 0 (the default) launches the
 * kernels of an arena without the feature.
 * -2: after the arena's first search or game start, or on an arena paired by spmcts_set_leaf_peer (which refuses
 * lanes of different modes, -3); -3: unknown mode. */
enum { SPMCTS_SYM_NONE = 0, SPMCTS_SYM_MIRROR = 1 };
int spmcts_set_symmetry(spmcts_arena *h, int32_t mode);
int spmcts_get_symmetry(const spmcts_arena *h);
/* The host twin of the rule (no GPU): board int8 [W][H] and the player to move -> canon int8 [W][H] with own = +1,
 * opp = -1 in canonical orientation, *flipped = 1 iff the mirror image was taken. */
int spmcts_canonical_host(int32_t game, int32_t width, int32_t height, const int8_t *board /*[W][H]*/, int32_t player,
                          int8_t *canon /*[W][H], own = +1*/, int32_t *flipped);

/* ---- games-level API (SelfPlayer.play_episode state machine) -------------- */
/* Start games in the listed slots (selfplayworker.py:172-179): both trees reset,
 * swap_sides = game id odd (self_play_parallel.py:237).  Game ids continue from
 * the arena's counter. */
int spmcts_games_start(spmcts_arena *h, const int32_t *slots_dev, const float *priors_dev /* NULL or [n][2][A] */,
                       int32_t n, spmcts_stream stream);
/* Cap on games started by automatic refill (< 0 = unlimited). */
int spmcts_games_set_limit(spmcts_arena *h, int64_t max_games);
/* Each active game's player to move begins its search (noise); active set = movers. */
int spmcts_games_begin_ply(spmcts_arena *h, spmcts_stream stream);
/* Each active game: _play on the mover, Move recorded, env.step, play_action on
 * both trees (selfplayworker.py:209-224); expansions go to the leaf batch. */
int spmcts_games_end_ply(spmcts_arena *h, void *leaves_dev, int32_t *leaf_count_dev, spmcts_stream stream);
/* Finished games: result, push_to_queue of both trees' Moves into the export
 * ring (mcts.py:225-232, selfplayworker.py:185-190), refill (if `refill`).
 * out_dev[0] = games finished this ply, out_dev[1] = records in the ring. */
int spmcts_games_finish_ply(spmcts_arena *h, int32_t refill, int32_t *out_dev /*[2]*/, spmcts_stream stream);
/* Copy the export ring out and clear it: states int8 [n][W*H], tree_probs f32
 * [n][A], q f64 [n], q_f64 u8 [n], z f32 [n] (actual_val), game ids i64 [n]. */
int spmcts_export_moves(spmcts_arena *h, int8_t *states_dev, float *tree_probs_dev, double *q_dev, uint8_t *q_f64_dev,
                        float *z_dev, int64_t *game_dev, int32_t max_records, int32_t *count_dev,
                        spmcts_stream stream);
/* The game log: with `on`, every ply of every game (searched moves, the hard-coded players' moves, opening-book
 * plies) stores its action in the slot's log, uint8 [n_games][W*H], and spmcts_games_finish_ply puts each finished
 * game's record into the finished-game ring before the slot is reused: game id i64, slot i32, result i8 (tree 2g's
 * view, the value spmcts_games_results gives), swap u8, plies i32, opening i32 (-1 without a book), moves u8 [W*H]
 * (bytes past `plies` zero).  A ply's records lie in slot order after those already in the ring (no atomics: the
 * layout is the same on every run).  The ring holds 2 * n_games records, the games two plies can finish: drained
 * once per ply (spmcts_export_games) it never fills.  A record that does not fit is dropped whole, with
 * SPMCTS_ERR_EXPORT raised; nothing is overwritten.  The first `on` allocates the log and the ring (n_games * W*H
 * bytes + 2 * n_games * (22 + W*H) bytes, outside spmcts_arena_bytes, as the evaluation cache's memory is); an
 * arena that never calls this allocates nothing and its kernels see a null log.  The log changes no search, random
 * draw, Move record or result.  Refused (-4) while any game slot is active.  (sync) */
int spmcts_games_set_log(spmcts_arena *h, int32_t on);
/* Copy the finished-game ring out (at most max_records records, the fields of spmcts_games_set_log one array
 * each) and clear it; count_dev[0] = records copied.  The twin of spmcts_export_moves: no host synchronisation.
 * Like it, the call empties the whole ring: with max_records below the ring's count the records past max_records
 * are discarded without a flag, so pass the ring's capacity, 2 * n_games, to lose none. */
int spmcts_export_games(spmcts_arena *h, int64_t *id_dev, int32_t *slot_dev, int8_t *result_dev, uint8_t *swap_dev,
                        int32_t *plies_dev, int32_t *opening_dev, uint8_t *moves_dev, int32_t max_records,
                        int32_t *count_dev, spmcts_stream stream);
/* (sync) per-slot game state: active flag, ply, swap, game id */
int spmcts_games_state(spmcts_arena *h, uint8_t *active, int32_t *ply, uint8_t *swap, int64_t *game_id);

/* (sync) per-slot game outcome, host arrays of n_games entries (each may be NULL): result = the reward in the
 * view of tree 2g (+1 win, 0 draw or unfinished, -1 loss: r * player, selfplayworker.py:218), swap, plies
 * played, state (0 idle, 1 active, 2 done and not yet finished by spmcts_games_finish_ply).  A slot keeps its
 * values after its game is finished until another game starts in it, so an arena that plays one game per slot
 * (no refill) reads every game's outcome here (the per-pairing results of compare_models, elo.py:49-71). */
int spmcts_games_results(spmcts_arena *h, int8_t *result, uint8_t *swap, int32_t *ply, uint8_t *state);

/* ---- opening book: games that start from given move sequences ------------------------------------------------ */
/* An opening is a sequence of actions m[0..L) from the empty board, m[0] played by whoever moves first in the
 * game.  While ply < L the game is in its book: the ply is SelfPlayer.play_move (selfplayworker.py:221-224)
 * applied to m[ply] -- the same env.step and the same play_action / _set_node on both trees (mcts.py:188-209),
 * expansion rows and backup included -- but nobody searches: no root noise, no random number, no tree in the
 * active set, no Move record (the reference records in _play only, mcts.py:272-299).  From ply L on the game
 * runs as without a book.  Game id i plays opening ((i mod id_period) >> 1) mod n_openings (id_period 0: no
 * modulus), so ids 2k and 2k + 1 play one opening with and without swap_sides (self_play_parallel.py:237);
 * refilled games take theirs from their new id.
 *
 * (sync) host arrays: moves uint8 [n_openings][max_len], lens int32 [n_openings].  n_openings <= 65536 (0 turns
 * the book off), max_len < W * H, id_period even.  Every sequence is validated on the host with the board rules
 * of spmcts_env_step_host: an illegal move, or one that ends the game, returns -3 and spmcts_last_error names
 * the opening and the ply ("opening I ply P: ...").  Refused (-4) while any game slot is active.  On the device
 * a book move that is illegal or ends the game raises SPMCTS_ERR_ACTION / SPMCTS_ERR_STATE. */
int spmcts_games_set_openings(spmcts_arena *h, const uint8_t *moves, const int32_t *lens, int32_t n_openings,
                              int32_t max_len, int32_t id_period);
/* The validation of spmcts_games_set_openings alone (host only: no arena, no GPU), same return and message. */
int spmcts_openings_validate(int32_t game, int32_t width, int32_t height, const uint8_t *moves, const int32_t *lens,
                             int32_t n_openings, int32_t max_len);
/* (sync) host int32 [n_games]: the opening each slot's game plays; -1 for an idle slot or without a book. */
int spmcts_games_openings(spmcts_arena *h, int32_t *opening_of_slot);

/* ---- league: N networks in one arena (Elo.compare_models(*names), games/algos/elo.py:73-100) ---------------- */
/* A league arena is a single-network arena (spmcts_set_tree_players nets all 0) whose trees send their leaves
 * to one of n_nets networks: the step's rows are numbered and encoded as always, spmcts_league_route copies
 * each network's rows into that network's segment of a second buffer, each network evaluates its segment, and
 * spmcts_league_unroute brings the outputs back into arena-row order for the unchanged spmcts_expand.  Every
 * leaf is evaluated on its own (InferenceWorker, inference_worker.py:89-119): no dedup, no evaluation cache.
 *
 * (sync) tree_net: host array of n_trees entries in [0, n_nets), or -1 for a tree that sends no leaves (a
 * hard-coded player); 1 <= n_nets <= 32.  Network j's routed segment starts at seg[j] = K * (trees of networks
 * < j) and holds K * (trees of network j) rows (K = search_threads; a tree never has more than K pending rows,
 * and the end-of-ply expansions are at most one per tree).  -3 when leaf dedup, the evaluation cache or a leaf
 * peer is on or the arena is a two-network arena; turning one of those on afterwards fails the same way.
 * tree_net NULL with n_nets 0 turns the league off. */
int spmcts_set_league(spmcts_arena *h, const int32_t *tree_net, int32_t n_nets);
/* seg[0 .. n_nets]: first routed row of each network; seg[n_nets] = the routed buffer's rows in use. */
int spmcts_league_segments(const spmcts_arena *h, int32_t *seg);
/* The rows of the last select / leaf_rows / play_action / games_end_ply (leaves_dev, row_bytes bytes each;
 * leaf_count_dev = that call's count buffer, read on the device; NULL = the arena's own copy): network j's
 * rows to routed rows [seg[j], seg[j] + net_count_dev[j]) in ascending arena-row order.  A stable partition by
 * per-workgroup histograms and a scan (no atomics): the same layout every run.  row_bytes: any even number;
 * both buffers 2-byte aligned at least.  The row -> routed-row map stays in the arena for the unroute.  A row
 * of a tree without a network raises SPMCTS_ERR_STATE.  No host synchronisation. */
int spmcts_league_route(spmcts_arena *h, const void *leaves_dev, const int32_t *leaf_count_dev, int32_t row_bytes,
                        void *routed_dev, int32_t *net_count_dev /*[n_nets]*/, spmcts_stream stream);
/* probs_by_net_dev / values_by_net_dev: device arrays of n_nets device pointers to each network's outputs
 * ([rows][A] f32 / [rows] f32, indexed from that network's routed row 0).  Writes probs_dev [rows][A] and
 * values_dev [rows] in arena-row order.  -4 unless spmcts_league_route ran on this step's rows. */
int spmcts_league_unroute(spmcts_arena *h, const float *const *probs_by_net_dev,
                          const float *const *values_by_net_dev, float *probs_dev, float *values_dev,
                          spmcts_stream stream);

/* ---- diagnostics --------------------------------------------------------- */
int spmcts_get_counters(spmcts_arena *h, spmcts_counters *out); /* (sync) */
int spmcts_check(spmcts_arena *h);                                /* (sync) <0 if a device error flag is set */

/* ---- stand-alone kernels -------------------------------------------------- */
/* Batched env step (Connect4Env.step connect4env.py:29-43 / TicTacToeEnv.step
 * tictactoe_env.py:23-33) on device: boards int8 [n][W][H]. status: 0 ok,
 * 1 ValueError (full column), 2 GameOver (over_dev[i] set). */
int spmcts_env_step(int32_t game, int32_t width, int32_t height, const int8_t *boards_dev, const int32_t *actions_dev,
                    const int8_t *players_dev, const uint8_t *over_dev, int32_t n, int8_t *out_boards_dev,
                    int8_t *reward_dev, uint8_t *done_dev, int8_t *status_dev, uint8_t *valid_dev,
                    spmcts_stream stream);
/* Host-compiled twin of the same bitboard code (single board, host pointers), used
 * by the Python env facade for interactive play (not on the self-play path). */
int spmcts_env_step_host(int32_t game, int32_t width, int32_t height, int8_t *board /*[W][H] in/out*/,
                         int32_t action, int32_t player, int32_t *reward, int32_t *done);
int spmcts_valid_moves_host(int32_t game, int32_t width, int32_t height, const int8_t *board, uint8_t *valid);
/* ---- exact depth-limited negamax (csrc/negamax.h) -------------------------------------------------------------
 * A position is seen from the side to move.  For a depth D >= 1 every action gets one int8 code:
 *   +k (k odd, 1 <= k <= D)   playing it, the mover forces a win within k plies and not sooner (the move is ply 1)
 *   -k (k even, 2 <= k <= D)  every line loses by force; k = the latest ply the loss can be delayed to
 *    0                        not decided within D plies (a full-board draw and the horizon are both 0)
 *   -128                      an illegal move
 * Preference: +1 > +3 > ... > 0 > ... > -4 > -2.  Legal moves, wins and full boards are those of
 * spmcts_env_step_host.  The position is assumed not to be finished: a board that already holds a line is
 * searched as if play went on.  The search is full width; nodes = moves made (it stops at wins, full boards
 * and the horizon). */
/* The deepest D: 9 for TicTacToe (a full solve), 8 for the Connect4 boards; -2 for a board not instantiated. */
int spmcts_negamax_max_depth(int32_t game, int32_t width, int32_t height);
/* Positions per kernel launch at this depth: spmcts_negamax_batch splits a larger batch, so that no launch's
 * worst-case node bound, positions * sum_{k <= D} A^k, exceeds a constant (csrc/spmcts.hip NM_LAUNCH_NODES). */
int spmcts_negamax_launch_positions(int32_t game, int32_t width, int32_t height, int32_t depth);
/* Host twin (the kernel's search core compiled for the host; no GPU): board int8 [W][H] of +-1 stones, player =
 * the side to move; scores int8 [A], nodes (may be NULL).  -3 for a depth outside [1, max_depth]. */
int spmcts_negamax_host(int32_t game, int32_t width, int32_t height, const int8_t *board /*[W][H]*/, int32_t player,
                        int32_t depth, int8_t *scores /*[A]*/, uint64_t *nodes);
/* n positions on the device: boards_dev int8 [n][W][H], players_dev int8 [n] -> scores_dev int8 [n][A],
 * nodes_dev uint64 [n] (may be NULL).  No arena, asynchronous on `stream`; n = 0 is a no-op; -3 (with a
 * spmcts_last_error text) for a depth outside [1, max_depth].  Bit-equal to the host twin. */
int spmcts_negamax_batch(int32_t game, int32_t width, int32_t height, const int8_t *boards_dev,
                         const int8_t *players_dev, int32_t n, int32_t depth, int8_t *scores_dev, uint64_t *nodes_dev,
                         spmcts_stream stream);
/* ---- exact solver to the end of the game (csrc/solve.h) ---------------------------------------------------------
 * An alpha-beta search with a transposition table that runs every line to the end of the game.  A root move's
 * code is what spmcts_negamax_* would give at any depth D >= the number of empty cells:
 *   +k    playing it, the mover forces a win in k plies and not sooner (the move is ply 1)
 *   -k    every line loses by force; k = the latest ply the loss can be delayed to
 *    0    a draw under best play (nothing is undecided)
 *   -128  an illegal move
 *   -127  a legal move whose search gave up at the node budget (never a guess)
 * Equivalently s(pos) = the maximum over the legal moves of e if the move wins, 0 if it fills the board, -s(child)
 * otherwise, e = the empty cells of pos; the code of a move with value s is e + 1 - s, -(e + 1 + s) or 0.
 * The position must be unfinished and hold no line of L for either side: -3 otherwise.
 * The table is the caller's: uint64 entries, zeroed (0 = empty), a power-of-two count >= 2^16, for one board only;
 * it may be kept across calls and shared by a batch (an entry is a truth about a position: a hit proves the
 * position's identity bit for bit, one entry is one 64-bit load or store).  max_nodes >= 1 is a position's budget
 * of moves made (nodes); a position that reaches it stops: the moves it has not finished get -127, what it
 * finished stays exact, nothing unfinished is stored in the table.  A move that wins at once or fills the board
 * needs no search and keeps its code under any budget. */
/* Host twin (the kernels' search core compiled for the host; no GPU): a host table; board int8 [W][H] of +-1
 * stones, player = the side to move; scores int8 [A], nodes (may be NULL): the moves made.  The root's own moves are
 * always made (A at the most); past them a move is made only while the count is below max_nodes. */
int spmcts_solve_host(int32_t game, int32_t width, int32_t height, const int8_t *board /*[W][H]*/, int32_t player,
                      uint64_t *table, uint64_t table_entries, uint64_t max_nodes, int8_t *scores /*[A]*/,
                      uint64_t *nodes);
/* The bytes of spmcts_solve_batch's work buffer for n positions (A * A parked searches each). */
int spmcts_solve_work_bytes(int32_t game, int32_t width, int32_t height, int32_t n, uint64_t *bytes_out);
/* n positions on the device: boards_dev int8 [n][W][H], players_dev int8 [n], table_dev uint64 [table_entries],
 * work_dev (spmcts_solve_work_bytes; contents arbitrary) -> scores_dev int8 [n][A], nodes_dev uint64 [n] (may be
 * NULL).  One lane per (position, first move, second move); a launch gives every running lane at most
 * launch_nodes steps of at most one move each (0: the default, csrc/spmcts.hip SV_LAUNCH_STEPS; else >= 4), a lane
 * that is not through parks its stack in work_dev and the next launch resumes it there.  Synchronous: the count
 * of running lanes is read back after every launch; a position whose lanes have made max_nodes moves is given up
 * at the next launch (so it may overshoot by its lanes' last slices).  n = 0 is a no-op; -3 with a
 * spmcts_last_error text for a bad table size, max_nodes = 0, a launch_nodes of 1 .. 3 or a finished position.
 * The codes of solved positions are bit-equal to the host twin's (both are exact); node counts depend on the
 * table's contents and on the lanes that share it. */
int spmcts_solve_batch(int32_t game, int32_t width, int32_t height, const int8_t *boards_dev,
                       const int8_t *players_dev, int32_t n, uint64_t *table_dev, uint64_t table_entries,
                       void *work_dev, uint64_t max_nodes, uint32_t launch_nodes, int8_t *scores_dev,
                       uint64_t *nodes_dev, spmcts_stream stream);
/* The step launches of this thread's last spmcts_solve_batch. */
int spmcts_solve_launches(void);
/* ---- game records: from move lists to the positions before their moves (csrc/records.h; no arena) ----------- */
/* moves u8 [n][W*H] and plies i32 [n]: n game records (spmcts_export_games' fields, or any move lists from the
 * empty board).  Each record is replayed with the rules of spmcts_env_step_host, the first mover's stones +1 and
 * the mover +1 on even plies, -1 on odd ones.  status u8 [n]: 0 legal; 1 an illegal move (outside the action
 * range, a full column, an occupied TicTacToe cell); 2 a move after the game was over; 3 plies outside
 * [0, W*H].  Every legal record gives one row per ply p in [first_ply, plies), in (record, ply) order: boards i8
 * [N][W][H] the board before move p, players i8 [N] the side to move (the boards / players of
 * spmcts_negamax_batch and spmcts_solve_batch), row_record and row_ply i32 [N].  offsets i32 [n + 1]: each
 * record's first row (the exclusive scan of the legal records' row counts; no atomics, so the layout is the same
 * on every run), offsets[n] = N.  Rows at or past max_rows are not written (sum of max(0, plies - first_ply) is
 * always enough).  Asynchronous on `stream`; n = 0 is a no-op. */
int spmcts_log_positions(int32_t game, int32_t width, int32_t height, const uint8_t *moves_dev, const int32_t *plies_dev,
                         int32_t n, int32_t first_ply, int32_t max_rows, int8_t *boards_dev, int8_t *players_dev,
                         int32_t *row_record_dev, int32_t *row_ply_dev, uint8_t *status_dev, int32_t *offsets_dev,
                         spmcts_stream stream);
/* The host twin (the same core compiled for the host; no GPU): host pointers, every output bit-equal. */
int spmcts_log_positions_host(int32_t game, int32_t width, int32_t height, const uint8_t *moves, const int32_t *plies,
                              int32_t n, int32_t first_ply, int32_t max_rows, int8_t *boards, int8_t *players,
                              int32_t *row_record, int32_t *row_ply, uint8_t *status, int32_t *offsets);
/* Deterministic table network (oracle/table_net.py) over leaf rows, for bit-exact
 * search parity tests: leaves in any spmcts_leaf_format/layout; per-row salts optional. */
int spmcts_table_net(int32_t game, int32_t width, int32_t height, const void *leaves_dev, int32_t leaf_format,
                     int32_t leaf_layout, int32_t n, uint64_t salt, const uint64_t *salts_dev /* [n] or NULL */,
                     float *probs_dev, float *values_dev, spmcts_stream stream);
/* Fused residual-tower trunk for leaf evaluation (games/general/modules.py:43-107
 * with BatchNorm folded): stem conv3x3 + num_blocks BasicBlocks + the policy/value
 * 1x1 head convs, bias + ReLU (+ residual) fused, activations resident in LDS,
 * bf16 (or, with SPMCTS_TOWER_F16, fp16 = the reference's autocast dtype,
 * inference_worker.py:117) MFMA with fp32 accumulation.  planes_dev: bf16 [batch][W][H][3]
 * (NHWC leaf rows, 0/1 planes); weights and features_dev [batch][W*H][channels/2] (policy |
 * value head channels, cell-major) in the flags' element type.  Packed weight/bias layout:
 * csrc/tower_kernels.h (the M16 layout's block convs: csrc/tower_m16.h).  Instantiated for 7x6 and 3x3 boards with channels 128 or 256 (libspmcts_boards.so: the same six entry points for 6x5 and 8x7). */
#define SPMCTS_TOWER_F16 2
int spmcts_tower_forward(int32_t width, int32_t height, int32_t channels, int32_t n_blocks, const void *planes_dev,
                         int32_t batch, const void *weights_dev, const float *bias_dev, void *features_dev,
                         int32_t flags, spmcts_stream stream);
/* The linear heads on the trunk features (modules.py:96-105), fused: policy softmax over
 * `actions` and tanh value.  head_w: bf16 rows [32 (policy, zero-padded)] ++ [8ff] over K = W*H*ff
 * columns in (cell, channel) order, fragment-swizzled: for 32-row tile j and 16-column step s, one
 * contiguous 1 KiB block whose 16-byte lane l holds row 32j + (l % 32), columns 16s + 8(l / 32) .. +8;
 * head_b: f32 bp[32] ++ bv[8ff] ++ wo[8ff] ++ bo.  flags: SPMCTS_TOWER_F16 = features and head_w
 * are fp16 (else bf16). */
int spmcts_tower_heads(int32_t width, int32_t height, int32_t channels, int32_t actions, const void *features_dev,
                       int32_t batch, const void *head_w_dev, const float *head_b_dev, float *probs_dev,
                       float *values_dev, int32_t flags, spmcts_stream stream);
/* Head epilogue after one GEMM Z = features @ Wc^T (Wc rows: value hidden [hidden] then
 * policy [actions]): value = tanh(relu(Z[:hidden] + bv) . wo + bo), probs = softmax(Z[hidden:] + bp).
 * z_dev bf16 [batch][ldz]; head_b: f32 bv[hidden] ++ wo[hidden] ++ bo ++ bp[actions]. */
int spmcts_head_epilogue(int32_t hidden, int32_t actions, const void *z_dev, int32_t ldz, int32_t batch,
                         const float *head_b_dev, float *probs_dev, float *values_dev, spmcts_stream stream);
int spmcts_tower_supported(int32_t width, int32_t height, int32_t channels);
/* The packed weight blob layout the trunk of this shape expects (replaces nothing in the reference: the
 * blob is this library's own format, built by evaluator.HipTowerEvaluator.refresh from the module's
 * state_dict, modules.py:88-107).  SPMCTS_WLAYOUT_32X32: every conv as [Cout/32][taps][Cin/16][64 lanes][8],
 * block and head convs' input channels in the phys_off order.  SPMCTS_WLAYOUT_M16 (the 7x6 C = 128 and
 * C = 256 trunks, tower_m16.h / tower_wide16.h): the stem as 32X32; the block convs as [Cout/16][taps][Cin/32][64 lanes][8] (lane 16q + n:
 * output channel 16 ct + n, input channels 32 k + 8 q ..) and the block and head convs' input channels in
 * the phys16 order.  Returns -2 for an unsupported shape. */
#define SPMCTS_WLAYOUT_32X32 0
#define SPMCTS_WLAYOUT_M16 1
int spmcts_tower_weight_layout(int32_t width, int32_t height, int32_t channels);
/* Device-count variants: the batch size is read from count_dev (e.g. the leaf-row count written by
 * spmcts_select) so no host synchronisation is needed; max_batch bounds the grid.
 * flags: SPMCTS_TOWER_PACK = the launch shares the chip with concurrent launches on other streams
 * (engine.LanedEngine): every board goes in full-size tiles and only the last few boards in one
 * smaller tile, instead of whole chip rounds of full tiles plus one round of smaller tiles;
 * SPMCTS_TOWER_F16 = fp16 weights / activations / features. */
#define SPMCTS_TOWER_PACK 1
int spmcts_tower_forward_dev(int32_t width, int32_t height, int32_t channels, int32_t n_blocks, const void *planes_dev,
                             const int32_t *count_dev, int32_t max_batch, const void *weights_dev,
                             const float *bias_dev, void *features_dev, int32_t flags, spmcts_stream stream);
int spmcts_tower_heads_dev(int32_t width, int32_t height, int32_t channels, int32_t actions, const void *features_dev,
                           const int32_t *count_dev, int32_t max_batch, const void *head_w_dev,
                           const float *head_b_dev, float *probs_dev, float *values_dev, int32_t flags,
                           spmcts_stream stream);
/* The trainer's 3x3 residual-block convolutions (stride 1, padding 1) on the matrix cores, fp16 NCHW tensors
 * as torch autocast hands them to conv2d (replaces MIOpen's conv2d forward / backward-data / backward-weight
 * calls that the UpdateWorker's autocast SGD step makes, updateworker.py:141-149 -> mcts.py:254-270 ->
 * modules.py:13-40); fp32 accumulation, deterministic (no atomics).
 *   _supported: 1 if the (board, channels) shape is handled, in both directions (forward and input grad).
 *   _pack: the fp32 parameter w [cout][cin][3][3], rounded to fp16 -> wf [cout][9][cin] (forward) and
 *          wb [cin][9][cout] (taps flipped: the input-gradient convolution's weights).
 *   _fwd: y [n][cout][W][H] (fp16) = fp16(bias) + conv(x [n][cin][W][H] fp16, wpk = wf of _pack); bias is the
 *         fp32 parameter or NULL.  The input gradient is _fwd(dy, wb) with cin and cout swapped and no bias.
 *   _wgrad: dw [cout][cin][3][3] = fp16(sum over the batch of dy x x-patches) stored as f32, one slice of 8
 *           boards per partial sum (splits must be ceil(n / 8)) into part [splits][cout][9][cin] (f32 scratch),
 *           summed in order; db [cout] (f32 of the fp16 sum, may be NULL) = sum of dy over the batch and cells.
 * Return 0, -1 bad argument, -2 unsupported shape, -3 launch error. */
int spmcts_conv3x3_supported(int32_t width, int32_t height, int32_t cin, int32_t cout);
int spmcts_conv3x3_pack(int32_t cin, int32_t cout, const void *w, void *wf, void *wb, spmcts_stream stream);
int spmcts_conv3x3_fwd(int32_t n, int32_t width, int32_t height, int32_t cin, int32_t cout, const void *x,
                       const void *wpk, const void *bias, void *y, spmcts_stream stream);
int spmcts_conv3x3_wgrad(int32_t n, int32_t width, int32_t height, int32_t cin, int32_t cout, const void *x,
                         const void *dy, float *part, int32_t splits, void *dw, void *db, spmcts_stream stream);
/* Memory-roofline helper: device copy bandwidth probe (bytes each way). */
int spmcts_copy_probe(const void *src_dev, void *dst_dev, uint64_t bytes, spmcts_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* SPMCTS_H */
