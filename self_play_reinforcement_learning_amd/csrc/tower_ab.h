// tower_ab.h — what only the A/B library has (make ab: libspmcts_ab.so, -DSPMCTS_AB): the two alternates a test
// uses as the reference of a product kernel, behind environment switches read once:
//   SPMCTS_TOWER_C256=3                          the 7x6 C = 256 trunk on 3-board two-buffer tiles (tower_b32.h)
//   SPMCTS_HEADS=lds, SPMCTS_HEADS_C256=lds      the LDS-staged linear heads k_heads (every shape / C = 256 only)
//
// Included by tower.hip under #ifdef SPMCTS_AB, inside namespace tower, in place of the product's three hooks
// (tiles_7x6c256, launch_heads_lds, ab_switch_guard), after TileSet and the product tile sets, which it uses;
// also uses BoardMajor32 (tower_common.h) and HeadsCfg (tower_heads.h).
static bool env_is(const char *name, const char *val) {
  const char *e = getenv(name);
  return e && strcmp(e, val) == 0;
}
static bool c256_board3() {
  static const bool v = env_is("SPMCTS_TOWER_C256", "3");
  return v;
}
template <int FF>
static bool heads_lds() {
  static const bool v = env_is("SPMCTS_HEADS", "lds") || (FF != 32 && env_is("SPMCTS_HEADS_C256", "lds"));
  return v;
}
// the switches are this library's own: nothing to refuse
static int ab_switch_guard() { return 0; }

// SPMCTS_TOWER_C256=3: 7x6, C = 256 on 3-board two-buffer tiles (32x32x16 layout)
template <class E>
using Tiles7x6c256Board3 = TileSet<7, BoardMajor32<256, 128, 7, 6, E>>;
template <class E, class Fn>
static int tiles_7x6c256(Fn &&f) {
  return c256_board3() ? f(Tiles7x6c256Board3<E>{}) : f(Tiles7x6c256<E>{});
}

// The LDS-staged linear heads, BOARDS boards per workgroup (M = 32 MFMA rows of which BOARDS are boards): the
// workgroup's features are staged once into LDS (coalesced; per-board stride padded by 16 B so the 16-B operand
// reads of 16 different boards are bank-conflict free), the weights stream through a 4-deep register ring.
template <int FF, int CELLS, int A>
struct HeadsLds : HeadsCfg<FF, CELLS, A> {
  static constexpr int BOARDS = HeadsCfg<FF, CELLS, A>::FROW * 16 + 16 * 16 <= 96 * 1024 ? 16 : 8;
  static constexpr int FS = HeadsCfg<FF, CELLS, A>::FROW + 16;  // LDS stride per board
};

template <int FF, int CELLS, int A, class E = __bf16>
__global__ __launch_bounds__(256) void k_heads(const uint16_t *feats, int n, const int32_t *count, const bf16x8 *wf,
                                               const float *hb, float *probs, float *values) {
  using H = HeadsLds<FF, CELLS, A>;
  if (count) n = min(*count, n);  // n = the caller's buffer rows
  const int b0 = blockIdx.x * H::BOARDS;
  if (b0 >= n) return;
  __shared__ __attribute__((aligned(16))) char s_feat[H::BOARDS * H::FS];
  __shared__ float s_part[4][32];        // per-wave value partial sums
  __shared__ float s_pol[4][32][33];     // per-wave policy partial logits
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int nb = min(H::BOARDS, n - b0);
  // stage the features of this workgroup's boards (16 B per thread-iteration, coalesced)
  {
    constexpr int CH = H::FROW / 16;
    const uint4 *src = (const uint4 *)(feats + (size_t)b0 * CELLS * 2 * FF);
    for (int i = tid; i < H::BOARDS * CH; i += 256) {
      const int bd = i / CH, c = i % CH;
      const uint4 v = bd < nb ? src[(size_t)bd * CH + c] : make_uint4(0, 0, 0, 0);
      *(uint4 *)(s_feat + bd * H::FS + c * 16) = v;
    }
  }
  const float *bp = hb, *bv = hb + 32, *wo = hb + 32 + H::HID, *bo = hb + 32 + 2 * H::HID;
  const int row = r % H::BOARDS;  // rows >= BOARDS duplicate a board; their results are ignored
  const char *frow = s_feat + row * H::FS;
  f32x16 acc[H::VTW];
  f32x16 pacc = {};
#pragma unroll
  for (int v = 0; v < H::VTW; ++v) acc[v] = f32x16{};
  // weight ring: VTW value fragments (+ 1 policy fragment while s is in this wave's quarter)
  constexpr int D = 4;
  bf16x8 ring[D][H::VTW];
  const bf16x8 *wv = wf + (size_t)(1 + wave * H::VTW) * H::KS * 64 + lane;
  const bf16x8 *wp = wf + lane;
  const int q0 = wave * H::KQ, q1 = min(H::KS, q0 + H::KQ);
  __syncthreads();
#pragma unroll
  for (int d = 0; d < D; ++d)
#pragma unroll
    for (int v = 0; v < H::VTW; ++v) ring[d][v] = wv[((size_t)v * H::KS + d) * 64];
  bf16x8 pnext = wp[(size_t)q0 * 64];
  for (int s0 = 0; s0 < H::KS; s0 += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int s = s0 + d;
      if (s >= H::KS) break;
      const int k0 = 16 * s + 8 * h;
      const int cell = k0 / FF, c = k0 % FF;
      const bf16x8 av = *(const bf16x8 *)(frow + (cell * 2 * FF + FF + c) * 2);
      bf16x8 wcur[H::VTW];
#pragma unroll
      for (int v = 0; v < H::VTW; ++v) {
        wcur[v] = ring[d][v];
        if (s + D < H::KS) ring[d][v] = wv[((size_t)v * H::KS + s + D) * 64];
      }
#pragma unroll
      for (int v = 0; v < H::VTW; ++v) acc[v] = Ty<E>::mfma(av, wcur[v], acc[v]);
      if (s >= q0 && s < q1) {
        const bf16x8 ap = *(const bf16x8 *)(frow + (cell * 2 * FF + c) * 2);
        const bf16x8 pw = pnext;
        if (s + 1 < q1) pnext = wp[(size_t)(s + 1) * 64];
        pacc = Ty<E>::mfma(ap, pw, pacc);
      }
    }
  }
  // value: relu(acc + bv[col]) * wo[col], summed over the hidden units (cols)
  // D layout: lane (r, h): col = r, rows (boards) = (i & 3) + 8 * (i >> 2) + 4 * h
  float part[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) part[i] = 0.f;
#pragma unroll
  for (int v = 0; v < H::VTW; ++v) {
    const int col = (wave * H::VTW + v) * 32 + r;
    const float bb = bv[col], ww = wo[col];
#pragma unroll
    for (int i = 0; i < 16; ++i) part[i] += fmaxf(acc[v][i] + bb, 0.f) * ww;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    float x = part[i];
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) x += __shfl_xor(x, off, 32);
    part[i] = x;
  }
  if (r == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) s_part[wave][(i & 3) + 8 * (i >> 2) + 4 * h] = part[i];
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) s_pol[wave][(i & 3) + 8 * (i >> 2) + 4 * h][r] = pacc[i];
  __syncthreads();
  if (tid < nb) {
    const int bd = b0 + tid;
    values[bd] = tanhf(((s_part[0][tid] + s_part[1][tid]) + (s_part[2][tid] + s_part[3][tid])) + bo[0]);
    float lg[A];
    float m = -INFINITY;
#pragma unroll
    for (int a = 0; a < A; ++a) {
      lg[a] = ((s_pol[0][tid][a] + s_pol[1][tid][a]) + (s_pol[2][tid][a] + s_pol[3][tid][a])) + bp[a];
      m = fmaxf(m, lg[a]);
    }
    float e[A], sum = 0.f;
#pragma unroll
    for (int a = 0; a < A; ++a) {
      e[a] = __expf(lg[a] - m);
      sum += e[a];
    }
    const float inv = 1.f / sum;
#pragma unroll
    for (int a = 0; a < A; ++a) probs[(size_t)bd * A + a] = e[a] * inv;
  }
}

// launches k_heads when the shape's switch asks for the LDS-staged heads; false = the product's k_heads_co runs
template <int FF, int CELLS, int A, class E>
static bool launch_heads_lds(const void *feats, int batch, const int32_t *count, const void *w, const float *b,
                             float *probs, float *values, hipStream_t s) {
  if (!heads_lds<FF>()) return false;
  constexpr int BOARDS = HeadsLds<FF, CELLS, A>::BOARDS;
  hipLaunchKernelGGL((k_heads<FF, CELLS, A, E>), dim3((batch + BOARDS - 1) / BOARDS), dim3(256), 0, s,
                     (const uint16_t *)feats, batch, count, (const bf16x8 *)w, b, probs, values);
  return true;
}
