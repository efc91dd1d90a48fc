// negamax.h — exact depth-limited negamax over the bitboards of board.h: the search core (host and device),
// the batch kernel and the arena player's kernel.
// Included by spmcts.hip before arena_games.h (hardcoded_move ranks the codes): needs board.h, View and in_book.
// ----------------------------------------------------------------------------
// Semantics.  A position is (own, opp): the mover's stones and the other side's.  Legal moves are legal_mask's,
// a win and a full board are step's (board.h).  For a horizon D >= 1, s(pos, d) is the maximum over the legal
// moves of: d if the move wins, 0 if it fills the board, -s(child, d - 1) otherwise; s(., 0) = 0.  The code of
// a root move with value s at d = D is D + 1 - s for s > 0 (+k: a forced win in k plies, the move itself being
// ply 1, and not sooner), -(D + 1 + s) for s < 0 (-k: a forced loss, delayed to ply k at the latest), else 0
// (not decided within D plies; a full-board draw and the horizon are both 0); an illegal move is -128.
// Preference: +1 > +3 > ... > 0 > ... > -4 > -2, the order of s.
// The position is assumed not to be finished.  A board that already holds a line is searched as if play went on:
// step reports a win for a move whose row, column or diagonal holds a run, whichever stone completed it.
//
// Shape.  The search is full width (no pruning: the node counts are those of the plain recursion, and every
// root move's code is exact by construction).  The work item is (position, first move a, second move b): one
// lane plays a and b and searches the grandchild to depth D - 2, or records that ply 1 or 2 ended the game (or
// the horizon did: D = 1 and D = 2 take the same path with no grandchild search).  A second step folds a
// position's A * A items into its A codes in ascending b, no atomics.  The levels below the grandchild are
// NmLevel<G, L>: L falls at compile time, so the nesting is bounded by construction, each level's state (its two
// masks, the move index, the best value) has its own registers, and there is no stack.  Every loop runs a move
// index that only rises over A moves.  nodes = moves made (step calls), the count of the plain recursion.
// ----------------------------------------------------------------------------
#pragma once

namespace spm {

enum { NM_ILLEGAL = -128 };
// what an item holds instead of a value in [-D, D]
enum { NM_A_ILLEGAL = 127, NM_B_ILLEGAL = 126, NM_A_WINS = 125, NM_A_ZERO = 124 };

// The deepest horizon: TicTacToe 9 (a full solve), the Connect4 boards 8.  A lane's grandchild search is then at
// most sum_{k <= 7} 9!/(9-2-k)! < 2^14 (TicTacToe) or sum_{k <= 6} 8^k < 2^19 (8x7) nodes: its count fits 32 bits.
template <class G>
struct NmCap {
  static constexpr int DEPTH = G::GRAVITY ? 8 : 9;
  static constexpr int PLAYER = 6;  // arena player (spmcts_set_tree_players): a ply's launch stays short
};

template <class G, int L>
struct NmLevel {
  // s(pos, d) for d <= L
  static SPM_HD int run(uint64_t own, uint64_t opp, int d, uint32_t &nodes) {
    if (d <= 0) return 0;
    const uint32_t legal = legal_mask<G>(Board{own, opp});
    int best = NM_ILLEGAL;
    for (int a = 0; a < G::A; ++a) {
      if (!((legal >> a) & 1u)) continue;
      Board b{own, opp};
      int rew = 0, done = 0;
      step<G>(b, a, 1, &rew, &done);
      ++nodes;
      const int v = rew ? d : (done ? 0 : -NmLevel<G, L - 1>::run(b.neg, b.pos, d - 1, nodes));
      best = v > best ? v : best;
    }
    return best == NM_ILLEGAL ? 0 : best;
  }
};
template <class G>
struct NmLevel<G, 0> {
  static SPM_HD int run(uint64_t, uint64_t, int, uint32_t &) { return 0; }
};

// Item (a, b) of a position at horizon D (1 <= D <= NmCap<G>::DEPTH): the value move b gives the side that
// answers a (a term of s(child, D - 1)), or one of the NM_* marks; *nodes = moves made at ply 2 and below.
template <class G>
SPM_HD int8_t nm_item(uint64_t own, uint64_t opp, int a, int b, int D, uint32_t *nodes) {
  *nodes = 0;
  if (!((legal_mask<G>(Board{own, opp}) >> a) & 1u)) return NM_A_ILLEGAL;
  Board p{own, opp};
  int rew = 0, done = 0;
  step<G>(p, a, 1, &rew, &done);
  if (rew) return NM_A_WINS;
  if (done || D == 1) return NM_A_ZERO;
  if (!((legal_mask<G>(p) >> b) & 1u)) return NM_B_ILLEGAL;
  Board q{p.neg, p.pos};  // the answering side's view
  step<G>(q, b, 1, &rew, &done);
  uint32_t n = 1;
  const int v = rew ? D - 1 : (done ? 0 : -NmLevel<G, NmCap<G>::DEPTH - 2>::run(q.neg, q.pos, D - 2, n));
  *nodes = n;
  return (int8_t)v;
}

// The code of move a from its A items (ascending b), and the moves made under it (a itself included).
template <class G>
SPM_HD int8_t nm_fold(const int8_t *vals, const uint32_t *nodes, int D, uint64_t *made) {
  *made = 0;
  if (vals[0] == NM_A_ILLEGAL) return NM_ILLEGAL;
  *made = 1;
  int s = 0;
  if (vals[0] == NM_A_WINS) {
    s = D;
  } else if (vals[0] != NM_A_ZERO) {
    int best = NM_ILLEGAL;
    for (int b = 0; b < G::A; ++b) {
      if (vals[b] == NM_B_ILLEGAL) continue;
      best = vals[b] > best ? vals[b] : best;
      *made += nodes[b];
    }
    s = best == NM_ILLEGAL ? 0 : -best;
  }
  return (int8_t)(s > 0 ? D + 1 - s : (s < 0 ? -(D + 1 + s) : 0));
}

// The host twin: the items and the fold of one position, in the kernel's order.
template <class G>
inline void nm_solve_host(uint64_t own, uint64_t opp, int D, int8_t *scores, uint64_t *nodes) {
  uint64_t total = 0;
  for (int a = 0; a < G::A; ++a) {
    int8_t vals[G::A];
    uint32_t nn[G::A];
    for (int b = 0; b < G::A; ++b) vals[b] = nm_item<G>(own, opp, a, b, D, &nn[b]);
    uint64_t made = 0;
    scores[a] = nm_fold<G>(vals, nn, D, &made);
    total += made;
  }
  if (nodes) *nodes = total;
}

// The order of the codes as one integer: larger is better.
SPM_HD int nm_rank(int code) { return code > 0 ? 256 - code : (code < 0 ? -256 - code : 0); }

}  // namespace spm

// ----------------------------------------------------------------------------
// kernels: NM_THREADS lanes per block hold NmGrid<G>::PPB whole positions of A * A items each
// ----------------------------------------------------------------------------
enum { NM_THREADS = 256 };
template <class G>
struct NmGrid {
  static constexpr int ITEMS = G::A * G::A;
  static constexpr int PPB = NM_THREADS / ITEMS;  // 5 (7x6), 7 (6x5), 4 (8x7), 3 (3x3)
  static_assert(PPB >= 1 && PPB * G::A <= 64, "block geometry");
};

// One block's positions: every lane of the block calls it (two barriers inside).  slot = the lane's position
// within the block, `on` = that position is to be solved, D its horizon; scores = its [A] row, nodes = its
// count (or null).
template <class G>
__device__ __forceinline__ void nm_block(int slot, int item, bool on, uint64_t own, uint64_t opp, int D, int8_t *scores,
                                         uint64_t *nodes) {
  constexpr int A = G::A, ITEMS = NmGrid<G>::ITEMS, PPB = NmGrid<G>::PPB;
  __shared__ int8_t s_val[NM_THREADS];
  __shared__ uint32_t s_nodes[NM_THREADS];
  __shared__ uint64_t s_made[64];
  const int tid = threadIdx.x;
  const bool lane_on = on && slot < PPB;
  if (lane_on) {
    uint32_t n = 0;
    s_val[tid] = nm_item<G>(own, opp, item / A, item % A, D, &n);
    s_nodes[tid] = n;
  }
  __syncthreads();
  if (lane_on && item % A == 0) {  // the lane of (a, b = 0) folds move a
    uint64_t made = 0;
    const int a = item / A;
    scores[a] = nm_fold<G>(s_val + slot * ITEMS + a * A, s_nodes + slot * ITEMS + a * A, D, &made);
    s_made[slot * A + a] = made;
  }
  __syncthreads();
  if (lane_on && item == 0 && nodes) {
    uint64_t total = 0;
    for (int a = 0; a < A; ++a) total += s_made[slot * A + a];
    *nodes = total;
  }
}

// positions [p0, p0 + n) of a batch: boards int8 [.][W][H] of +-1 stones, players = the side to move
template <class G>
__global__ __launch_bounds__(NM_THREADS) void k_negamax_batch(const int8_t *boards, const int8_t *players, long long p0,
                                                              int n, int D, int8_t *scores, uint64_t *nodes) {
  constexpr int ITEMS = NmGrid<G>::ITEMS, PPB = NmGrid<G>::PPB;
  const int slot = threadIdx.x / ITEMS, item = threadIdx.x % ITEMS;
  const long long i = (long long)blockIdx.x * PPB + slot;
  const bool on = slot < PPB && i < n;
  uint64_t own = 0, opp = 0;
  const size_t p = (size_t)(p0 + (on ? i : 0));
  if (on) {
    const Board b = from_cells<G>(boards + p * G::CELLS);
    const bool plus = players[p] > 0;
    own = plus ? b.pos : b.neg;
    opp = plus ? b.neg : b.pos;
  }
  nm_block<G>(slot, item, on, own, opp, D, scores + p * G::A, nodes ? nodes + p : nullptr);
}

// games [g0, g0 + n) of an arena: the active games outside their book whose mover is a negamax tree; the
// tree's horizon is its budget, its codes go to its row of View::nm_score (read by hardcoded_move)
template <class G>
__global__ __launch_bounds__(NM_THREADS) void k_negamax_games(View v, int g0, int n) {
  constexpr int ITEMS = NmGrid<G>::ITEMS, PPB = NmGrid<G>::PPB;
  const int slot = threadIdx.x / ITEMS, item = threadIdx.x % ITEMS;
  const long long i = (long long)blockIdx.x * PPB + slot;
  bool on = slot < PPB && i < n;
  const int g = g0 + (int)(on ? i : 0);
  uint64_t own = 0, opp = 0;
  int D = 1, tree = 0;
  if (on) {
    const int mover = (v.gply[g] + v.gswap[g]) & 1;
    tree = 2 * g + mover;
    on = v.gstate[g] == GS_ACTIVE && !in_book(v, g) && v.tkind[tree] == SPMCTS_PLAYER_NEGAMAX;
    if (on) {
      own = mover == 0 ? v.gpos[g] : v.gneg[g];
      opp = mover == 0 ? v.gneg[g] : v.gpos[g];
      D = min(max(v.budget[tree], 1), NmCap<G>::PLAYER);  // (validated by spmcts_set_tree_players)
    }
  }
  nm_block<G>(slot, item, on, own, opp, D, v.nm_score + (size_t)tree * G::A, nullptr);
}
