// solve.h — exact solver to the end of the game over the bitboards of board.h: an iterative alpha-beta with a
// transposition table (host and device), its resumable batch kernels and the host twin.
// Included by spmcts.hip after negamax.h (it reuses the NM_* item marks): needs board.h.
// ----------------------------------------------------------------------------
// Semantics.  A position is (own, opp): the mover's stones and the other side's, e its number of empty cells.
// s(pos) is the maximum over the legal moves of: e if the move wins, 0 if it fills the board, -s(child)
// otherwise.  s depends on the position alone, so a table entry is a truth about a position, whoever wrote it.
// The code of a root move is negamax.h's at the horizon D = e (what spmcts_negamax_* gives at any D >= e):
// D + 1 - s for s > 0, -(D + 1 + s) for s < 0, else 0 (now a draw under best play, nothing is undecided);
// -128 for an illegal move; SV_UNKNOWN (-127) for a legal move whose search gave up at the node budget.
// The position must be unfinished and hold no line of L for either side: a move then wins iff it completes a
// run through its own cell, which is what sv_win_cells tests without making the move.
//
// Shape.  The work item is negamax.h's (position, first move a, second move b): one lane plays a and b and
// searches the grandchild by alpha-beta with the full window, sv_fold folds a position's A * A items in
// ascending b.  The search is iterative: SvLane holds the node under search (its two masks and its level sp),
// level l's frame is one 32-bit word (next move's place in the static centre-first order, alpha, beta, the
// alpha the node was entered with: 4 + 3 * 7 bits), a child's move is taken back from the parent's frame, so
// the stack is CELLS words per lane and nothing recurses.  sv_iter is one step: it finishes the node (table
// store, pop, the parent's alpha) or makes the node's next move (one node of the count) and either scores the
// child at once (sv_enter: the child's mover wins on the spot, the window closes on the bounds -(e - 1) <= s <=
// max(e - 2, 0) of a node without an immediate win, or the table answers) or pushes it.  Returned values are
// fail-hard: r inside the window is exact, r <= alpha says s <= r, r >= beta says s >= r.
// nodes = moves made (sv_win_cells makes none), at most the full-width search's.
//
// Table.  uint64 entries, a power-of-two count >= 2^16, 0 = empty; one entry is read and written by one 64-bit
// load or store.  h = splitmix64(key) is a bijection of the key (own + occupied + bottom row on the gravity
// boards, a unique code of the position); the index is h's low bits, the entry keeps h's upper 48 bits, so a
// hit proves the position's identity, beside the value (7 bits, + 64) and the bound kind (2 bits) in its low
// 16.  Only a node whose search completed is stored; a racing writer replaces one true bound with another.
// ----------------------------------------------------------------------------
#pragma once

namespace spm {

enum { SV_UNKNOWN = -127 };
enum { SV_RUN = 0, SV_DONE = 1, SV_GAVE_UP = 2 };   // an item's status
enum { SV_LOWER = 1, SV_UPPER = 2, SV_EXACT = 3 };  // an entry's bound kind (0: empty)
enum { SV_MIN_TABLE_BITS = 16 };

template <class G>
constexpr uint64_t sv_bottom_mask() {
  uint64_t m = 0;
  for (int x = 0; x < G::W; ++x) m |= 1ull << (x * G::CB);
  return m;
}

template <class G>
struct Sv {
  static constexpr uint64_t BOTTOM = sv_bottom_mask<G>();
  static constexpr uint64_t BOARD = BOTTOM * ((1ull << G::H) - 1ull);
  static_assert(G::CELLS + 1 < 64, "a value does not fit a frame's 7 bits");
  static_assert(G::A <= 15, "a move index does not fit a frame's 4 bits");
  static_assert(G::GRAVITY || G::W * G::CB <= 32, "the free-placement key packs two 32-bit masks");
};

// the static move order, centre first: A/2, A/2 - 1, A/2 + 1, ...
template <class G>
SPM_HD int sv_order(int i) { return G::A / 2 + (1 - 2 * (i & 1)) * ((i + 1) / 2); }

// the cells a stone can go to next, and the cells of action a: (playable & move_mask) is the stone a places
template <class G>
SPM_HD uint64_t sv_playable(uint64_t occ) {
  return G::GRAVITY ? ((occ + Sv<G>::BOTTOM) & Sv<G>::BOARD) : (~occ & Sv<G>::BOARD);
}
template <class G>
SPM_HD uint64_t sv_move_mask(int a) {
  return G::GRAVITY ? col_mask<G>(a) : (1ull << cell_bit<G>(a / G::H, a % G::H));
}

// the empty cells where a stone of p completes a run of L (the board holds no line yet)
template <class G>
SPM_HD uint64_t sv_win_cells(uint64_t p, uint64_t occ) {
  uint64_t r = 0;
  if (G::L == 4) {  // three of p and the fourth cell, at strides 1 (column), CB (row), CB +- 1 (diagonals)
    r = (p << 1) & (p << 2) & (p << 3);
    const int strides[3] = {G::CB, G::CB - 1, G::CB + 1};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int s = strides[d];
      uint64_t pp = (p << s) & (p << (2 * s));
      r |= pp & (p << (3 * s));
      r |= pp & (p >> s);
      pp = (p >> s) & (p >> (2 * s));
      r |= pp & (p << s);
      r |= pp & (p >> (3 * s));
    }
  } else {
#pragma unroll
    for (int x = 0; x < G::W; ++x)
#pragma unroll
      for (int y = 0; y < G::H; ++y) {
        const uint64_t bit = 1ull << cell_bit<G>(x, y);
        if (!(occ & bit) && win_through<G>(p | bit, x, y)) r |= bit;
      }
  }
  return r & Sv<G>::BOARD & ~occ;
}

// a line of L of p anywhere on the board
template <class G>
SPM_HD bool sv_has_line(uint64_t p) {
  const int strides[4] = {1, G::CB, G::CB - 1, G::CB + 1};
  bool any = false;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    uint64_t r = p;
#pragma unroll
    for (int k = 1; k < G::L; ++k) r &= p >> (k * strides[d]);
    any = any || r != 0;
  }
  return any;
}

// ---- table -------------------------------------------------------------------
template <class G>
SPM_HD uint64_t sv_key(uint64_t own, uint64_t occ) {
  return G::GRAVITY ? own + occ + Sv<G>::BOTTOM : ((own | ((occ & ~own) << 32)) + 1ull);
}
SPM_HD uint64_t sv_load(const uint64_t *t, uint64_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(t + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return __atomic_load_n(t + i, __ATOMIC_RELAXED);
#endif
}
SPM_HD void sv_store(uint64_t *t, uint64_t i, uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  __hip_atomic_store(t + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  __atomic_store_n(t + i, v, __ATOMIC_RELAXED);
#endif
}
SPM_HD void sv_table_put(uint64_t *t, uint64_t tmask, uint64_t key, int val, int kind) {
  const uint64_t h = splitmix64(key);
  sv_store(t, h & tmask, (h & ~0xFFFFull) | (uint64_t)(((val + 64) << 2) | kind));
}

// ---- frames --------------------------------------------------------------------
SPM_HD uint32_t sv_pack(int mi, int alpha, int beta, int alpha0) {
  return (uint32_t)mi | ((uint32_t)(alpha + 64) << 4) | ((uint32_t)(beta + 64) << 11) | ((uint32_t)(alpha0 + 64) << 18);
}
SPM_HD void sv_unpack(uint32_t f, int &mi, int &alpha, int &beta, int &alpha0) {
  mi = (int)(f & 15u);
  alpha = (int)((f >> 4) & 127u) - 64;
  beta = (int)((f >> 11) & 127u) - 64;
  alpha0 = (int)((f >> 18) & 127u) - 64;
}

struct SvLane {
  uint64_t own, opp;  // the node under search, its mover's view
  uint64_t nodes;     // moves made so far
  int32_t sp;         // its level (0 = the item's grandchild)
  int32_t status;     // SV_*
  int32_t val;        // SV_DONE: the item's value or its NM_* mark
};

// A node with e >= 1 empties entered with the window (alpha, beta), alpha < beta.  True: *v answers it (see the
// fail-hard rule at the top).  False: it is to be searched, with the window narrowed by its bounds and the table.
template <class G>
SPM_HD bool sv_enter(uint64_t own, uint64_t opp, int e, const uint64_t *table, uint64_t tmask, int &alpha, int &beta,
                     int *v) {
  const uint64_t occ = own | opp;
  if (sv_win_cells<G>(own, occ) & sv_playable<G>(occ)) {
    *v = e;
    return true;
  }
  // no move wins here: the mover's next stone is two plies on, the other side's one ply on
  const int ub = e >= 2 ? e - 2 : 0, lb = -(e - 1);
  const bool low = alpha >= ub;
  beta = beta > ub ? ub : beta;
  alpha = alpha < lb ? lb : alpha;
  if (alpha >= beta) {
    *v = low ? ub : lb;
    return true;
  }
  const uint64_t h = splitmix64(sv_key<G>(own, occ));
  const uint64_t ent = sv_load(table, h & tmask);
  const int kind = (int)(ent & 3u);
  if (((ent ^ h) >> 16) == 0 && kind != 0) {
    const int val = (int)((ent >> 2) & 127u) - 64;
    *v = val;
    if (kind == SV_EXACT) return true;
    if (kind == SV_LOWER) {
      if (val >= beta) return true;
      alpha = val > alpha ? val : alpha;
    } else {
      if (val <= alpha) return true;
      beta = val < beta ? val : beta;
    }
  }
  return false;
}

// One step of a running lane: at most one move made.  F: get(level) / set(level, frame) over the lane's stack.
template <class G, class F>
SPM_HD void sv_iter(SvLane &s, F &fr, uint64_t *table, uint64_t tmask) {
  const uint64_t occ = s.own | s.opp;
  const int e = G::CELLS - popc(occ);
  int mi, alpha, beta, alpha0;
  sv_unpack(fr.get(s.sp), mi, alpha, beta, alpha0);
  const uint64_t can = sv_playable<G>(occ);
  uint64_t bit = 0;
  if (alpha < beta) {
    for (; mi < G::A && !bit; ++mi) bit = can & sv_move_mask<G>(sv_order<G>(mi));
  }
  if (!bit) {  // the node is finished: its value is alpha
    sv_table_put(table, tmask, sv_key<G>(s.own, occ), alpha,
                 alpha <= alpha0 ? SV_UPPER : (alpha >= beta ? SV_LOWER : SV_EXACT));
    if (s.sp == 0) {
      s.status = SV_DONE;
      s.val = -alpha;  // the item's value is the answering side's (sv_item_init)
      return;
    }
    --s.sp;
    int pmi, palpha, pbeta, palpha0;
    sv_unpack(fr.get(s.sp), pmi, palpha, pbeta, palpha0);
    const int a = sv_order<G>(pmi - 1);  // the move that led here: its stone is the top of its column
    const uint64_t stone = G::GRAVITY ? 1ull << (a * G::CB + popc(occ & col_mask<G>(a)) - 1) : sv_move_mask<G>(a);
    const uint64_t pown = s.opp & ~stone;
    s.opp = s.own;
    s.own = pown;
    palpha = -alpha > palpha ? -alpha : palpha;
    fr.set(s.sp, sv_pack(pmi, palpha, pbeta, palpha0));
    return;
  }
  ++s.nodes;
  const uint64_t cown = s.opp, copp = s.own | bit;
  int ca = -beta, cb = -alpha, cv = 0;
  const bool known = e == 1 || sv_enter<G>(cown, copp, e - 1, table, tmask, ca, cb, &cv);  // e == 1: the board is full
  if (known) alpha = -cv > alpha ? -cv : alpha;
  fr.set(s.sp, sv_pack(mi, alpha, beta, alpha0));
  if (known) return;
  if (s.sp + 1 >= G::CELLS) {  // (cannot happen: a level has at least one empty cell fewer than the one above)
    s.status = SV_GAVE_UP;
    return;
  }
  ++s.sp;
  fr.set(s.sp, sv_pack(0, ca, cb, ca));
  s.own = cown;
  s.opp = copp;
}

// Item (a, b) of an unfinished position without a line: SV_DONE with its value for the side that answers a (or an
// NM_* mark) where no search is needed, else SV_RUN with the grandchild at level 0.  nodes = b's move.  The first
// move is always made; !room (the position's budget is used up): the item gives up before its second.
template <class G, class F>
SPM_HD void sv_item_init(uint64_t own, uint64_t opp, int a, int b, bool room, const uint64_t *table, uint64_t tmask,
                         SvLane &s, F &fr) {
  s.own = s.opp = s.nodes = 0;
  s.sp = 0;
  s.status = SV_DONE;
  const int e = G::CELLS - popc(own | opp);
  Board p{own, opp};
  int rew = 0, done = 0;
  if (!((legal_mask<G>(p) >> a) & 1u)) {
    s.val = NM_A_ILLEGAL;
    return;
  }
  step<G>(p, a, 1, &rew, &done);
  if (rew || done) {
    s.val = rew ? NM_A_WINS : NM_A_ZERO;
    return;
  }
  if (!((legal_mask<G>(p) >> b) & 1u)) {
    s.val = NM_B_ILLEGAL;
    return;
  }
  if (!room) {
    s.status = SV_GAVE_UP;
    s.val = 0;
    return;
  }
  Board q{p.neg, p.pos};  // the answering side's view
  step<G>(q, b, 1, &rew, &done);
  s.nodes = 1;
  if (rew || done) {
    s.val = rew ? e - 1 : 0;
    return;
  }
  int alpha = -(e - 2), beta = e - 1, v = 0;  // the full window of a node with e - 2 empties
  if (sv_enter<G>(q.neg, q.pos, e - 2, table, tmask, alpha, beta, &v)) {
    s.val = -v;
    return;
  }
  s.status = SV_RUN;
  s.own = q.neg;
  s.opp = q.pos;
  fr.set(0, sv_pack(0, alpha, beta, alpha));
}

// The code of move a from its A items (ascending b; st = status | value << 8), and the moves made under it (a
// itself included).  SV_UNKNOWN if an item's search gave up.
template <class G>
SPM_HD int8_t sv_fold(const int32_t *st, const uint64_t *nodes, int e, uint64_t *made) {
  *made = 0;
  const int v0 = st[0] >> 8;
  if (v0 == NM_A_ILLEGAL) return NM_ILLEGAL;
  *made = 1;
  int s = 0;
  if (v0 == NM_A_WINS) {
    s = e;
  } else if (v0 != NM_A_ZERO) {
    int best = NM_ILLEGAL;
    bool unknown = false;
    for (int b = 0; b < G::A; ++b) {
      const int v = st[b] >> 8;
      if (v == NM_B_ILLEGAL) continue;
      *made += nodes[b];
      unknown = unknown || (st[b] & 0xff) != SV_DONE;
      best = v > best ? v : best;
    }
    if (unknown) return SV_UNKNOWN;
    s = best == NM_ILLEGAL ? 0 : -best;
  }
  return (int8_t)(s > 0 ? e + 1 - s : (s < 0 ? -(e + 1 + s) : 0));
}

// The host twin: one position's items in ascending (a, b), each searched to its end or to the position's budget:
// past the root's own moves, a move is made only while the count is below max_nodes.
template <class G>
struct SvHostFrames {
  uint32_t f[G::CELLS];
  uint32_t get(int l) const { return f[l]; }
  void set(int l, uint32_t v) { f[l] = v; }
};

template <class G>
inline void sv_solve_host(uint64_t own, uint64_t opp, uint64_t *table, uint64_t tmask, uint64_t max_nodes,
                          int8_t *scores, uint64_t *nodes) {
  const int e = G::CELLS - popc(own | opp);
  uint64_t total = 0;
  for (int a = 0; a < G::A; ++a) {
    int32_t st[G::A];
    uint64_t nn[G::A];
    if ((legal_mask<G>(Board{own, opp}) >> a) & 1u) ++total;  // a's move: the root's moves are always made
    for (int b = 0; b < G::A; ++b) {
      SvLane s;
      SvHostFrames<G> fr;
      sv_item_init<G>(own, opp, a, b, total < max_nodes, table, tmask, s, fr);
      total += s.nodes;
      while (s.status == SV_RUN && total < max_nodes) {
        const uint64_t n0 = s.nodes;
        sv_iter<G>(s, fr, table, tmask);
        total += s.nodes - n0;
      }
      if (s.status != SV_DONE) {
        s.status = SV_GAVE_UP;
        s.val = 0;
      }
      st[b] = s.status | (s.val * 256);
      nn[b] = s.nodes;
    }
    uint64_t made = 0;
    scores[a] = sv_fold<G>(st, nn, e, &made);
  }
  if (nodes) *nodes = total;
}

}  // namespace spm

// ----------------------------------------------------------------------------
// kernels: one lane per item, SV_THREADS lanes (one wave) per block, item i = position * A * A + a * A + b
// ----------------------------------------------------------------------------
enum { SV_THREADS = 64 };

// The work buffer of n positions (N = n * A * A items): what a lane parks between launches.
struct SvWork {
  uint32_t *unsolved;  // [4] the items still running after a launch (word 0); k_solve_init: the positions that
                       // are finished or hold a line (word 1) and the first of them (word 2)
  uint64_t *used;      // [n] moves made for a position so far
  uint64_t *own, *opp, *nodes;  // [N] SvLane
  int32_t *sp, *st;    // [N] level; status | value << 8
  uint32_t *frames;    // [CELLS][N] level-major: a wave's lanes read one level side by side
  long long N;
};

template <class G>
static size_t sv_work_bytes(long long n) {
  const size_t N = (size_t)n * G::A * G::A;
  return 16 + (size_t)n * 8 + N * (3 * 8 + 2 * 4) + N * G::CELLS * 4;
}
template <class G>
static SvWork sv_work(void *base, long long n) {
  const size_t N = (size_t)n * G::A * G::A;
  char *p = (char *)base;
  SvWork w;
  w.unsolved = (uint32_t *)p;
  w.used = (uint64_t *)(p + 16);
  w.own = w.used + n;
  w.opp = w.own + N;
  w.nodes = w.opp + N;
  w.sp = (int32_t *)(w.nodes + N);
  w.st = w.sp + N;
  w.frames = (uint32_t *)(w.st + N);
  w.N = (long long)N;
  return w;
}

struct SvGlobalFrames {  // an item's stack in the work buffer
  uint32_t *base;
  long long N;
  __device__ uint32_t get(int l) const { return base[(size_t)l * N]; }
  __device__ void set(int l, uint32_t v) { base[(size_t)l * N] = v; }
};
struct SvLdsFrames {  // a lane's stack in its block's LDS, level-major (bank = lane)
  uint32_t *base;
  __device__ uint32_t get(int l) const { return base[l * SV_THREADS]; }
  __device__ void set(int l, uint32_t v) { base[l * SV_THREADS] = v; }
};

// every item of the batch: its marks, or its grandchild parked at level 0; a position's a and b moves counted
template <class G>
__global__ __launch_bounds__(SV_THREADS) void k_solve_init(const int8_t *boards, const int8_t *players, SvWork w,
                                                           const uint64_t *table, uint64_t tmask) {
  constexpr int ITEMS = G::A * G::A;
  const long long i = (long long)blockIdx.x * SV_THREADS + threadIdx.x;
  if (i >= w.N) return;
  const long long p = i / ITEMS;
  const int item = (int)(i % ITEMS);
  const Board b = from_cells<G>(boards + (size_t)p * G::CELLS);
  const bool plus = players[p] > 0;
  SvLane s;
  SvGlobalFrames fr{w.frames + i, w.N};
  if (popc(b.pos | b.neg) == G::CELLS || sv_has_line<G>(b.pos) || sv_has_line<G>(b.neg)) {  // refused by the host
    if (item == 0) {
      atomicAdd(w.unsolved + 1, 1u);
      atomicMin(w.unsolved + 2, (uint32_t)p);
    }
    w.st[i] = SV_DONE | (NM_A_ILLEGAL * 256);
    w.nodes[i] = 0;
    return;
  }
  sv_item_init<G>(plus ? b.pos : b.neg, plus ? b.neg : b.pos, item / G::A, item % G::A, true, table, tmask, s, fr);
  w.own[i] = s.own;
  w.opp[i] = s.opp;
  w.nodes[i] = s.nodes;
  w.sp[i] = 0;
  w.st[i] = s.status | (s.val * 256);
  const unsigned long long made = s.nodes + (item % G::A == 0 && s.val != NM_A_ILLEGAL ? 1u : 0u);
  if (made) atomicAdd((unsigned long long *)&w.used[p], made);
}

// One launch: every running item whose position is within its budget takes up its stack, makes at most `slice`
// steps (each at most one move) and parks again.  The step index is the same for all lanes of the wave, so an
// item's interleaving with its wave does not depend on where the launches cut.
template <class G>
__global__ __launch_bounds__(SV_THREADS) void k_solve_step(SvWork w, uint64_t *table, uint64_t tmask, uint64_t max_nodes,
                                                           uint32_t slice) {
  constexpr int ITEMS = G::A * G::A;
  __shared__ uint32_t s_fr[G::CELLS * SV_THREADS];
  const long long i = (long long)blockIdx.x * SV_THREADS + threadIdx.x;
  if (i >= w.N) return;
  const int32_t st = w.st[i];
  if ((st & 0xff) != SV_RUN) return;
  const long long p = i / ITEMS;
  if (w.used[p] >= max_nodes) {
    w.st[i] = SV_GAVE_UP;
    return;
  }
  SvLane s;
  s.own = w.own[i];
  s.opp = w.opp[i];
  s.nodes = w.nodes[i];
  s.sp = min(max(w.sp[i], 0), G::CELLS - 1);
  s.status = SV_RUN;
  s.val = 0;
  SvLdsFrames fr{s_fr + threadIdx.x};
  for (int l = 0; l <= s.sp; ++l) fr.set(l, w.frames[(size_t)l * w.N + i]);
  const uint64_t n0 = s.nodes;
  for (uint32_t it = 0; it < slice && s.status == SV_RUN; ++it) sv_iter<G>(s, fr, table, tmask);
  if (s.nodes != n0) atomicAdd((unsigned long long *)&w.used[p], (unsigned long long)(s.nodes - n0));
  w.nodes[i] = s.nodes;
  w.st[i] = s.status | (s.val * 256);
  if (s.status != SV_RUN) return;
  w.own[i] = s.own;
  w.opp[i] = s.opp;
  w.sp[i] = s.sp;
  for (int l = 0; l <= s.sp; ++l) w.frames[(size_t)l * w.N + i] = fr.get(l);
  atomicAdd(w.unsolved, 1u);
}

// a position's A codes and its node count from its items
template <class G>
__global__ __launch_bounds__(SV_THREADS) void k_solve_fold(const int8_t *boards, SvWork w, int n, int8_t *scores,
                                                           uint64_t *nodes) {
  constexpr int ITEMS = G::A * G::A;
  const long long p = (long long)blockIdx.x * SV_THREADS + threadIdx.x;
  if (p >= n) return;
  const Board b = from_cells<G>(boards + (size_t)p * G::CELLS);
  const int e = G::CELLS - popc(b.pos | b.neg);
  uint64_t total = 0;
  for (int a = 0; a < G::A; ++a) {
    uint64_t made = 0;
    const size_t i0 = (size_t)p * ITEMS + (size_t)a * G::A;
    scores[(size_t)p * G::A + a] = sv_fold<G>(w.st + i0, w.nodes + i0, e, &made);
    total += made;
  }
  if (nodes) nodes[p] = total;
}
