// records.h — from game records (move lists) to the positions before their moves: spmcts_log_positions and its
// host twin.  Included by spmcts.hip after arena_games.h: needs board.h only (no arena).
//
// A record r is moves uint8 [CELLS] and plies.  It is replayed from the empty board with board.h's step<G>, the
// first mover's stones +1 (the absolute frame), the mover +1 on even plies and -1 on odd ones.  Its status:
// LP_OK; LP_ILLEGAL a move outside the action range, into a full column or onto an occupied cell; LP_OVER a move
// after the game's end; LP_RANGE plies outside [0, CELLS].  A record that is LP_OK gives one row per ply p in
// [first_ply, plies): the board before move p.  Rows lie in (r, p) order: record r's first row is the exclusive
// scan of the records' row counts (no atomics), so the layout is the same on every run and on the host.
enum { LP_OK = 0, LP_ILLEGAL = 1, LP_OVER = 2, LP_RANGE = 3 };

// Replay record `m`; rows (boards == nullptr: none) are written from row `row0` on, those at or past max_rows left
// out.  Returns the status.
template <class G>
SPM_HD int lp_replay(const uint8_t *m, int plies, int first_ply, int row0, int rec, int max_rows, int8_t *boards,
                     int8_t *players, int32_t *row_record, int32_t *row_ply) {
  if (plies < 0 || plies > G::CELLS) return LP_RANGE;
  Board b{0, 0};
  int over = 0;
  for (int p = 0; p < plies; ++p) {
    const int a = m[p], player = (p & 1) ? -1 : 1;
    if (over) return LP_OVER;
    if (a >= G::A || !((legal_mask<G>(b) >> a) & 1u)) return LP_ILLEGAL;
    if (boards && p >= first_ply) {
      const int row = row0 + (p - first_ply);
      if (row < max_rows) {
        for (int x = 0; x < G::W; ++x)
          for (int y = 0; y < G::H; ++y) boards[(size_t)row * G::CELLS + x * G::H + y] = cell_value<G>(b, x, y);
        players[row] = (int8_t)player;
        row_record[row] = rec;
        row_ply[row] = p;
      }
    }
    int rew = 0;
    if (step<G>(b, a, player, &rew, &over) != STEP_OK) return LP_ILLEGAL;
  }
  return LP_OK;
}

SPM_HD int lp_rows(int status, int plies, int first_ply) {
  return status == LP_OK && plies > first_ply ? plies - first_ply : 0;
}

// one thread per record: its status and its row count (into offsets[r], scanned by k_log_scan)
template <class G>
__global__ void k_log_status(const uint8_t *moves, const int32_t *plies, int n, int first_ply, uint8_t *status,
                             int32_t *offsets) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int st = lp_replay<G>(moves + (size_t)r * G::CELLS, plies[r], first_ply, 0, r, 0, nullptr, nullptr, nullptr, nullptr);
  status[r] = (uint8_t)st;
  offsets[r] = lp_rows(st, plies[r], first_ply);
}

// offsets [n + 1]: row counts -> their exclusive scan, offsets[n] = the total (single block, record order)
__global__ __launch_bounds__(1024) void k_log_scan(int32_t *offsets, int n) {
  __shared__ int32_t s_sum[1024];
  const int tid = threadIdx.x;
  const int chunk = (n + 1023) / 1024;
  const int lo = min(n, tid * chunk), hi = min(n, lo + chunk);
  int sum = 0;
  for (int r = lo; r < hi; ++r) sum += offsets[r];
  s_sum[tid] = sum;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int a = tid >= off ? s_sum[tid - off] : 0;
    __syncthreads();
    s_sum[tid] += a;
    __syncthreads();
  }
  int at = s_sum[tid] - sum;
  for (int r = lo; r < hi; ++r) {
    const int c = offsets[r];
    offsets[r] = at;
    at += c;
  }
  if (tid == 1023) offsets[n] = s_sum[1023];
}

// one thread per legal record: its rows, from offsets[r] on
template <class G>
__global__ void k_log_rows(const uint8_t *moves, const int32_t *plies, int n, int first_ply, const uint8_t *status,
                           const int32_t *offsets, int max_rows, int8_t *boards, int8_t *players, int32_t *row_record,
                           int32_t *row_ply) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n || status[r] != LP_OK) return;
  lp_replay<G>(moves + (size_t)r * G::CELLS, plies[r], first_ply, offsets[r], r, max_rows, boards, players, row_record,
               row_ply);
}

// the host twin: the same core, the scan a running sum
template <class G>
static void lp_host(const uint8_t *moves, const int32_t *plies, int n, int first_ply, int max_rows, int8_t *boards,
                    int8_t *players, int32_t *row_record, int32_t *row_ply, uint8_t *status, int32_t *offsets) {
  int at = 0;
  for (int r = 0; r < n; ++r) {
    const uint8_t *m = moves + (size_t)r * G::CELLS;
    const int st = lp_replay<G>(m, plies[r], first_ply, 0, r, 0, nullptr, nullptr, nullptr, nullptr);
    status[r] = (uint8_t)st;
    offsets[r] = at;
    if (st == LP_OK) lp_replay<G>(m, plies[r], first_ply, at, r, max_rows, boards, players, row_record, row_ply);
    at += lp_rows(st, plies[r], first_ply);
  }
  offsets[n] = at;
}
