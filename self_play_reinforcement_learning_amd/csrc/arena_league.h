// arena_league.h — league routing: a step's leaf rows partitioned by their tree's network, and back.
// Included by spmcts.hip after arena_misc.h: needs View and set_err.
// ----------------------------------------------------------------------------
// A league arena (spmcts_set_league) is a single-segment arena whose trees belong to up to LEAGUE_MAX_NETS
// networks.  The row pipeline is unchanged: k_scan_need numbers the step's rows in slot order, k_encode writes
// them.  k_league_* then copy network j's rows, in ascending arena-row order, to routed rows
// [seg[j], seg[j] + net_count[j]) of a second buffer, each network evaluates its segment from its routed row 0,
// and k_league_unroute gathers the outputs back into arena-row order for the unchanged expand.
//
// The partition is a counting sort without atomics, so the layout is the same bits every run:
//   k_league_hist   one row per thread, LEAGUE_SPAN rows per workgroup: the row's network, its rank among the
//                   workgroup's rows of that network (wave ballots + the wave totals), the workgroup's histogram
//   k_league_scan   one thread per network: exclusive scan of the histograms over the workgroups -> each
//                   workgroup's base per network, net_count
//   k_league_copy   routed row = seg[net] + base[workgroup][net] + rank; the row's bytes in the widest units the
//                   rows' alignment allows (2, 4, 8 or 16 bytes); the row -> routed-row map for the unroute
// ----------------------------------------------------------------------------
constexpr int LEAGUE_MAX_NETS = 32;
constexpr int LEAGUE_SPAN = 256;  // rows per workgroup of the partition (one per thread)
constexpr int LEAGUE_WAVES = LEAGUE_SPAN / 64;
constexpr int LEAGUE_COPY_BLOCKS = 4096;  // grid bound of the grid-stride kernels

// device view of the league state (by value to the kernels)
struct League {
  int n;              // networks
  int32_t *tree_net;  // [T] network of each tree, -1 = none (a hard-coded player)
  int32_t *seg;       // [LEAGUE_MAX_NETS + 1] first routed row of each network; seg[n] = the routed rows in all
  int32_t *rank;      // [NS] per arena row: net * LEAGUE_SPAN + rank within its workgroup, -1 = no network
  int32_t *map;       // [NS] arena row -> routed row (-1 = none)
  int32_t *hist;      // [workgroups][LEAGUE_MAX_NETS] histogram, then (k_league_scan) base per network
  const int32_t *count;  // device row count of the step
};

__device__ __forceinline__ int league_rows(const View &v, const League &lg) { return min(max(lg.count[0], 0), v.NS); }

__global__ __launch_bounds__(LEAGUE_SPAN) void k_league_hist(View v, League lg) {
  __shared__ int32_t s_cnt[LEAGUE_WAVES][LEAGUE_MAX_NETS];
  const int rows = league_rows(v, lg);
  if ((int)blockIdx.x * LEAGUE_SPAN >= rows) return;  // the whole workgroup: no barrier is skipped by a part of it
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = blockIdx.x * LEAGUE_SPAN + tid;
  int net = -1;
  if (r < rows) {
    const int slot = v.row_tree[r];
    if (slot >= 0 && slot < v.NS) net = lg.tree_net[slot / v.K];
    if (net < 0 || net >= lg.n) {  // a row of a tree without a network
      set_err(v, SPMCTS_ERR_STATE);
      net = -1;
    }
  }
  int rank = 0;
  for (int j = 0; j < lg.n; ++j) {
    const unsigned long long b = __ballot(net == j);
    if (net == j) rank = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) s_cnt[wave][j] = __popcll(b);
  }
  __syncthreads();
  if (r < rows) {
    for (int w = 0; w < wave; ++w)
      if (net >= 0) rank += s_cnt[w][net];
    lg.rank[r] = net >= 0 ? net * LEAGUE_SPAN + rank : -1;
  }
  if (tid < lg.n) {
    int c = 0;
    for (int w = 0; w < LEAGUE_WAVES; ++w) c += s_cnt[w][tid];
    lg.hist[(size_t)blockIdx.x * LEAGUE_MAX_NETS + tid] = c;
  }
}

__global__ __launch_bounds__(64) void k_league_scan(View v, League lg, int32_t *net_count) {
  const int j = threadIdx.x;
  if (j >= lg.n) return;
  const int nb = (league_rows(v, lg) + LEAGUE_SPAN - 1) / LEAGUE_SPAN;
  int sum = 0;
  for (int b = 0; b < nb; ++b) {
    int32_t *p = lg.hist + (size_t)b * LEAGUE_MAX_NETS + j;
    const int c = *p;
    *p = sum;
    sum += c;
  }
  if (sum > lg.seg[j + 1] - lg.seg[j]) {  // more rows than K per tree of the network: not a state the arena reaches
    set_err(v, SPMCTS_ERR_STATE);
    sum = lg.seg[j + 1] - lg.seg[j];
  }
  net_count[j] = sum;
}

// U: the copy unit (uint16_t, uint32_t, uint2, uint4), upr = units per row
template <class U>
__global__ __launch_bounds__(256) void k_league_copy(View v, League lg, const U *leaves, U *routed, int upr) {
  const long long total = (long long)league_rows(v, lg) * upr;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int r = (int)(i / upr), u = (int)(i - (long long)r * upr);
    const int pk = lg.rank[r];
    int dst = -1;
    if (pk >= 0) {
      const int net = pk / LEAGUE_SPAN;
      dst = lg.seg[net] + lg.hist[(size_t)(r / LEAGUE_SPAN) * LEAGUE_MAX_NETS + net] + pk % LEAGUE_SPAN;
      if (dst >= lg.seg[net + 1]) dst = -1;  // past the segment (k_league_scan raised the error)
    }
    if (u == 0) lg.map[r] = dst;
    if (dst >= 0) routed[(size_t)dst * upr + u] = leaves[(size_t)r * upr + u];
  }
}

// outputs back into arena-row order: probs [rows][A], values [rows]; each network's buffers are indexed from
// its routed row 0
__global__ __launch_bounds__(256) void k_league_unroute(View v, League lg, const float *const *probs_by_net,
                                                        const float *const *values_by_net, float *probs,
                                                        float *values) {
  const int A = v.A;
  const long long total = (long long)league_rows(v, lg) * (A + 1);
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int r = (int)(i / (A + 1)), a = (int)(i - (long long)r * (A + 1));
    const int dst = lg.map[r];
    float x = 0.f;
    if (dst >= 0) {
      const int net = lg.rank[r] / LEAGUE_SPAN;
      const size_t rr = (size_t)(dst - lg.seg[net]);
      x = a < A ? probs_by_net[net][rr * A + a] : values_by_net[net][rr];
    }
    if (a < A)
      probs[(size_t)r * A + a] = x;
    else
      values[r] = x;
  }
}
