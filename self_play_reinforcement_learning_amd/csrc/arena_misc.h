// arena_misc.h — stand-alone kernels (env step, table net, copy probe) and the arena init kernels.
// Included by spmcts.hip after arena_games.h: needs View, Philox and board.h.
// ----------------------------------------------------------------------------
// stand-alone kernels
// ----------------------------------------------------------------------------
template <class G>
__global__ void k_env_step(const int8_t *boards, const int32_t *actions, const int8_t *players, const uint8_t *over,
                           int n, int8_t *out, int8_t *reward, uint8_t *done, int8_t *status, uint8_t *valid) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Board b = from_cells<G>(boards + (size_t)i * G::CELLS);
  int rew = 0, dn = 0, st;
  if (over && over[i]) {
    st = STEP_GAME_OVER;
    dn = 1;
  } else {
    st = step<G>(b, actions[i], players[i], &rew, &dn);
  }
  for (int x = 0; x < G::W; ++x)
    for (int y = 0; y < G::H; ++y) out[(size_t)i * G::CELLS + x * G::H + y] = cell_value<G>(b, x, y);
  reward[i] = (int8_t)rew;
  done[i] = (uint8_t)dn;
  status[i] = (int8_t)st;
  const uint32_t lm = legal_mask<G>(b);
  for (int a = 0; a < G::A; ++a) valid[(size_t)i * G::A + a] = (lm >> a) & 1u;
}

// table network (oracle/table_net.py) from leaf rows
template <class G>
__global__ void k_table_net(const void *leaves, int fmt, int layout, int n, uint64_t salt, const uint64_t *salts,
                            float *probs, float *values) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t h = 0xCBF29CE484222325ull;
  for (int cell = 0; cell < G::CELLS; ++cell) {
    int c = 0;
    if (fmt == SPMCTS_LEAF_BOARD_I64) {
      const int64_t val = ((const int64_t *)leaves)[(size_t)i * G::CELLS + cell];
      c = val == 1 ? 1 : (val == -1 ? 2 : 0);
    } else {
      size_t i1, i2;
      if (layout == SPMCTS_NHWC) {
        i1 = ((size_t)i * G::CELLS + cell) * 3 + 1;
        i2 = i1 + 1;
      } else {
        i1 = (size_t)i * 3 * G::CELLS + G::CELLS + cell;
        i2 = i1 + G::CELLS;
      }
      float own, opp;
      if (fmt == SPMCTS_LEAF_F32) {
        own = ((const float *)leaves)[i1];
        opp = ((const float *)leaves)[i2];
      } else {
        own = ((const uint16_t *)leaves)[i1] ? 1.f : 0.f;
        opp = ((const uint16_t *)leaves)[i2] ? 1.f : 0.f;
      }
      c = own != 0.f ? 1 : (opp != 0.f ? 2 : 0);
    }
    h = (h ^ (uint64_t)(c + 3 * cell + 1)) * 0x100000001B3ull;
  }
  h ^= salts ? salts[i] : salt;
  uint32_t k[G::A];
  uint32_t tot = 0;
  for (int j = 0; j < G::A; ++j) {
    k[j] = 1u + (uint32_t)((splitmix64(h + (uint64_t)j) >> 40) & 0xFFFFull);
    tot += k[j];
  }
  const float ft = (float)tot;
  for (int j = 0; j < G::A; ++j) probs[(size_t)i * G::A + j] = __fdiv_rn((float)k[j], ft);
  const int raw = (int)((splitmix64(h ^ 0x5DEECE66Dull) >> 40) & 0xFFFFull) - 32768;
  values[i] = __fdiv_rn((float)raw, 32768.0f);
}

__global__ void k_copy_probe(const float4 *src, float4 *dst, size_t n4) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n4; i += stride) dst[i] = src[i];
}

__global__ void k_rng_init(View v, uint64_t seed, uint64_t sub0) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= v.T) return;
  Philox s;
  rocrand_init(seed, sub0 + (uint64_t)t, 0ull, &s);
  v.rng[t] = s;
  v.tape_cur[t] = 0;
  ((int64_t *)v.tape_end)[t] = 0;
  // (trees that are never reset are still walked by the full-width launches: every per-tree word they read)
  for (int j = 0; j < v.K; ++j) v.need[(size_t)t * v.K + j] = NEED_EMPTY;
  v.tres[t] = 0;
  v.tstarted[t] = 0x3fffffff;
  v.noise_on[t] = 0;
  v.tnet[t] = 0;
  v.tkind[t] = SPMCTS_PLAYER_MCTS;
  v.budget[t] = 0x7fffffff;
  v.talpha[t] = v.alpha;
  v.tstrong[t] = (uint8_t)(v.strong ? 1 : 0);
  v.tK[t] = v.K;
  for (int k = 0; k < C_NCNT; ++k) v.cnt[(size_t)t * C_NCNT + k] = 0;
}

__global__ void k_games_init(View v) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g == 0) {
    for (int k = 0; k < 16; ++k) v.gcnt[k] = 0;
    v.gcnt[8] = -1;  // unlimited refill
    v.ex_count[0] = 0;
    v.err[0] = 0;
    v.row_count[0] = 0;
    v.row_count[1] = 0;
  }
  if (g >= v.G) return;
  v.gstate[g] = GS_IDLE;
  v.mv_count[2 * g] = 0;
  v.mv_count[2 * g + 1] = 0;
  v.gopen[g] = -1;  // no opening book (spmcts_games_set_openings)
  v.gbook[g] = 0;
}

__global__ void k_set_tape(View v, const int64_t *offsets) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= v.T) return;
  v.tape_cur[t] = offsets[t];
  ((int64_t *)v.tape_end)[t] = offsets[t + 1];
}
