// tower_common.h — what the three fused-trunk families share (namespace tower): the vector types, Ty (element
// type and its MFMAs), the edge-layout tables, Cfg (one tile plan) and its two named forms, one_opaque, lds_b128, WBuf
// (weight ring loads), Nbr (neighbour rows), XLive (skipped edge tiles), phys_off, acc_init (the stems'
// accumulator start) and head_layer (the 1x1 head convs that end every family's tile).
//
// Included by tower_b32.h, tower_m16.h, tower_wide16.h, tower_heads.h and tower_ab.h.  Uses the tables of
// tower_edge.h and nothing else of the project.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tower_edge.h"

namespace tower {

// edge-tile layout tables (tower_edge.h): row -> (board, x, y) packed (the inverse map,
// EDGE_CELL_ROW_INIT, is used only by the host-side layout tests)
constexpr uint16_t kEdgeRow[256] = EDGE_ROW_INIT;
// [tap][row] source row (zero rows off the board, at bank positions no on-board lane of the
// 16-lane read group uses)
constexpr uint16_t kEdgeNbr[9 * 256] = EDGE_NBR_INIT;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// Element type of the weights, the LDS activations and the head features: bf16, or fp16 = the
// reference's own inference dtype (amp.autocast, inference_worker.py:117).  Operands travel in 16-byte
// containers typed bf16x8 whatever E is (a bit cast at the MFMA is free); both MFMA forms take the
// same cycles on gfx950 (MI355X_MICROARCH.md).  fp32 accumulation either way.  mfma = 32x32x16 (the stems, the
// head convs, tower_b32.h's block convs), mfma16 = 16x16x32 (the block convs of tower_m16.h and tower_wide16.h).
template <class E>
struct Ty;
template <>
struct Ty<__bf16> {
  static constexpr bool BF16 = true;
  static __device__ __forceinline__ f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  // relu of a pair, packed (v_cvt_pk_bf16_f32 + v_pk_max_i16: a negative bf16 is a negative int16)
  static __device__ __forceinline__ uint32_t relu_pk(f32x2 v) {
    const bf16x2 b = __builtin_convertvector(v, bf16x2);
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(i16x2, b), i16x2{0, 0}));
  }
  static __device__ __forceinline__ f32x2 unpk(uint32_t x) {
    return f32x2{__uint_as_float(x << 16), __uint_as_float(x & 0xffff0000u)};
  }
  // v + the pair packed in x.  `one` is unused: the widening is a shift or a mask, one operation already, and this
  // chip has no mixed-precision FMA that reads a bf16 half
  static __device__ __forceinline__ f32x2 add_pk(f32x2 v, uint32_t x, float one) { return v + unpk(x); }
  static __device__ __forceinline__ uint16_t from_bf16(__bf16 x) { return __builtin_bit_cast(uint16_t, x); }
};
template <>
struct Ty<_Float16> {
  static constexpr bool BF16 = false;
  static __device__ __forceinline__ f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0,
                                                  0);
  }
  static __device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0,
                                                  0);
  }
  // round to nearest even (as torch's fp16 casts), then relu as a signed 16-bit max with 0
  static __device__ __forceinline__ uint32_t relu_pk(f32x2 v) {
    const f16x2 b = __builtin_convertvector(v, f16x2);
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(i16x2, b), i16x2{0, 0}));
  }
  static __device__ __forceinline__ f32x2 unpk(uint32_t x) {
    return __builtin_convertvector(__builtin_bit_cast(f16x2, x), f32x2);
  }
  // v + the pair packed in x, one v_fma_mix_f32 per element: it reads the fp16 half in place, and x * 1 + v rounds
  // once, as cvt + add does (the widening is exact).  `one` is 1.0f in a register the compiler cannot see through
  // (one_opaque): with a literal 1 it folds the fma back into cvt + add.
  static __device__ __forceinline__ f32x2 add_pk(f32x2 v, uint32_t x, float one) {
    const f16x2 h = __builtin_bit_cast(f16x2, x);
    float a = __builtin_fmaf((float)h[0], one, v[0]), b = __builtin_fmaf((float)h[1], one, v[1]);
    asm("" : "+v"(a));  // scalar results: packed into one v_pk_fma_f32, the pair would need its two cvts back
    asm("" : "+v"(b));
    return f32x2{a, b};
  }
  static __device__ __forceinline__ uint16_t from_bf16(__bf16 x) {
    return __builtin_bit_cast(uint16_t, (_Float16)(float)x);
  }
};
template <int C_, int ROWS_, int W_, int H_, int CG_ = 2, int WAVES_ = 4, int DEPTH_ = 4, int OCC_ = 1, bool XMAJ_ = false,
          bool EDGE_ = false, class E_ = __bf16, bool ONEBUF_ = false, bool M16_ = false>
struct Cfg : Ty<E_> {
  // M16 (tower_m16.h): the block convs on v_mfma_f32_16x16x32 with the phys16 channel order
  static constexpr bool M16 = M16_;
  using E = E_;  // operand / activation element type (Ty)
  static constexpr int OCC = OCC_;  // resident workgroups per CU the register budget is sized for
  static constexpr int DEPTH = DEPTH_;  // weight-fragment prefetch distance (k-steps)
  static constexpr int C = C_, ROWS = ROWS_, W = W_, H = H_;
  static constexpr int WAVES = WAVES_, THREADS = 64 * WAVES_;
  static constexpr int CG = CG_;            // waves split output channels into CG groups ...
  static constexpr int MG = WAVES_ / CG_;   // ... and cell rows into MG groups
  static constexpr int CELLS = W * H;
  static constexpr int BOARDS = ROWS / CELLS;
  static constexpr int VROWS = BOARDS * CELLS;
  static constexpr int RS = C * 2 + 16;  // bytes per LDS row
  static constexpr int ZROW = ROWS;
  // 16 zero rows: an off-board neighbour reads the zero row in its own bank position (rows r and
  // r + 16 share banks at a 4-dword row shift), so zero reads never conflict with on-board reads
  static constexpr int NZ = 16;
  static constexpr int NT = ROWS / 32 / MG;  // 32-cell tiles per wave
  static constexpr int MT = C / 32 / CG;     // 32-channel tiles per wave
  static constexpr int BUF = (ROWS + NZ) * RS;
  // Row layout of the tile, one of two.  Board-major (default): row = board * CELLS + x * H + y; a neighbour
  // is the affine row offset dx * DX + dy.  Edge tiles (EDGE): rows ordered by tower_edge.h so that whole cell
  // tiles hold only x = 0, y = 0, x = W-1 or y = H-1 cells; 12 of the workgroup's 72 (tile, tap) pairs read
  // zero padding only and are skipped, and neighbours come from a 9 x ROWS table of neighbour rows (zero rows
  // for off-board) that sits in LDS after the buffers.  XMAJ_ (column-major across boards, the family the edge
  // layout grew out of) only ever accompanies EDGE_.
  static_assert(XMAJ_ == EDGE_, "two row layouts: board-major, or edge tiles (XMAJ_ and EDGE_ both set)");
  // The parameter list is the kernels' identity (their mangled names), so the axes that no longer vary stay in
  // it, pinned here; BoardMajor32 and Edge16 below take the ones that do.
  static_assert(WAVES_ == 4, "every trunk workgroup is 4 waves (k_tower_dyn's one block size)");
  static_assert(OCC_ == 1, "every trunk kernel is sized for one workgroup per CU");
  static_assert(!ONEBUF_ || M16_, "the one-buffer trunk is the 16x16x32 form (tower_wide16.h)");
  static_assert(M16_ == EDGE_, "the 16x16x32 trunks run on edge tiles, the 32x32x16 trunk on board-major tiles");
  static constexpr bool EDGE = EDGE_;
  static constexpr int DX = H;
  static constexpr int TAB = EDGE ? 9 * ROWS * 2 : 0;
  // ONEBUF (tower_wide16.h): one activation buffer, convs in place between two barriers
  static constexpr bool ONEBUF = ONEBUF_;
  // ONEBUF also stages each conv's bias (C floats) in LDS
  static constexpr int LDS = (ONEBUF ? 1 : 2) * BUF + TAB + (ONEBUF ? C * 4 : 0);
  static constexpr int HEAD = C / 2;  // policy filter_factor | value filter_factor channels (filter_factor = C/4)
  static constexpr int HCT = HEAD / 32;  // head channel tiles
  static_assert(MT >= 1 && NT >= 1 && MT * NT <= (ONEBUF_ ? 16 : 8), "tile plan: at most 8 (one buffer: 16) accumulator tiles per wave");
  static_assert(CG * MG == WAVES, "wave plan");
  static_assert(BOARDS >= 1, "board larger than a tile");
  static_assert(LDS <= 163840, "LDS budget");
  static_assert(!EDGE_ || (W == 7 && H == 6 && ROWS == 256 && BOARDS == 6 && (MG == 2 || MG == 1)),
                "edge layout: 6 Connect4 boards, two row halves or one");
  // (board, x, y) of a row < VROWS
  __host__ __device__ static constexpr int row_board(int row) { return EDGE ? kEdgeRow[row] >> 6 : row / CELLS; }
  __host__ __device__ static constexpr int row_x(int row) { return EDGE ? (kEdgeRow[row] >> 3) & 7 : (row % CELLS) / H; }
  __host__ __device__ static constexpr int row_y(int row) { return EDGE ? kEdgeRow[row] & 7 : row % H; }
  // does row `row` (< ROWS) hold a cell?  Board-major tiles: rows < VROWS; edge tiles: the
  // rows tower_edge.h does not mark as padding (255), which may sit anywhere in the tile
  __host__ __device__ static constexpr bool row_ok(int row) { return EDGE ? kEdgeRow[row] != 255 : row < VROWS; }
  // does any on-board row of cell tile T have an on-board neighbour for `tap`?
  __host__ __device__ static constexpr bool tile_tap_live(int T, int tap) {
    for (int r = T * 32; r < T * 32 + 32 && r < ROWS; ++r) {
      if (!row_ok(r)) continue;
      const int nx = row_x(r) + tap / 3 - 1, ny = row_y(r) + tap % 3 - 1;
      if (nx >= 0 && nx < W && ny >= 0 && ny < H) return true;
    }
    return false;
  }
  __host__ __device__ static constexpr int row_cell(int row) { return row_x(row) * H + row_y(row); }
};

// The two plans that exist, by the parameters that vary.  Either way a wave owns 64 output channels (CG = C / 64
// channel groups, the rest of the 4 waves split the cell rows).
// Board-major two-buffer tiles on 32x32x16 (tower_b32.h): ROWS rows of whole W x H boards, weight ring 4 deep.
template <int C, int ROWS, int W, int H, class E>
using BoardMajor32 = Cfg<C, ROWS, W, H, C / 64, 4, 4, 1, false, false, E>;
// 6-board Connect4 edge tiles on 16x16x32, weight ring 2 deep: two buffers (tower_m16.h) or one (tower_wide16.h).
template <int C, bool ONEBUF, class E>
using Edge16 = Cfg<C, 256, 7, 6, C / 64, 4, 2, 1, true, true, E, ONEBUF, true>;

// 1.0f as a wave-uniform value the compiler treats as unknown (Ty::add_pk's multiplier)
__device__ __forceinline__ float one_opaque() {
  float one = 1.0f;
  asm("" : "+s"(one));
  return one;
}

__device__ __forceinline__ bf16x8 lds_b128(const char *p) { return *(const bf16x8 *)p; }

// Weight fragments through a buffer resource: the per-lane part of the address is a constant
// 32-bit voffset (lane * 16) and the fragment's byte offset is a wave-uniform soffset, so a ring
// refill is one buffer_load_dwordx4 with no per-load 64-bit address arithmetic.
struct WBuf {
  __amdgpu_buffer_rsrc_t rsrc;
  int voff;
  template <int AUX = 0>
  __device__ __forceinline__ bf16x8 load(uint32_t byte_off) const {
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    const i32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, (int)byte_off, AUX);
    return __builtin_bit_cast(bf16x8, v);
  }
};

// Per-lane neighbour geometry: for each of the wave's cell tiles t, the byte offset of the
// lane's cell row and a 9-bit mask of the taps whose neighbour lies on the board.
template <class K>
struct Nbr {
  int base[K::NT];
  int rowi[K::NT];
  uint32_t mask[K::NT];
  const uint16_t *tab;  // Cfg::EDGE: LDS neighbour-row table [9][ROWS]
  int off0[K::NT];      // tap 0's operand offsets (the same for every layer; set by finish())
  __device__ __forceinline__ void init(int r, int mg) {
#pragma unroll
    for (int t = 0; t < K::NT; ++t) {
      const int row = (mg * K::NT + t) * 32 + r;
      base[t] = row * K::RS;
      rowi[t] = row;
      uint32_t m = 0;
      if (K::row_ok(row)) {
        const int x = K::row_x(row), y = K::row_y(row);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int nx = x + tap / 3 - 1, ny = y + tap % 3 - 1;
          if (nx >= 0 && nx < K::W && ny >= 0 && ny < K::H) m |= 1u << tap;
        }
      }
      mask[t] = m;
    }
  }
  // once the table is in LDS: tap 0's offsets.  Nothing reads off0 any more, but the call stays: without it
  // all 16 trunk kernels compile to other code (292 to 1,629 lines of assembly each)
  __device__ __forceinline__ void finish() {
#pragma unroll
    for (int t = 0; t < K::NT; ++t) off0[t] = off(t, 0);
  }
  // byte offset of the source row of tile t for `tap` (the zero row when off the board); a
  // branch-free select (hipcc otherwise emits an exec-mask branch per tile and tap)
  __device__ __forceinline__ int off(int t, int tap) const {
    if constexpr (K::EDGE) return (int)tab[tap * K::ROWS + rowi[t]] * K::RS;
    const int dr = (tap / 3 - 1) * K::DX + (tap % 3 - 1);
    const int on = base[t] + dr * K::RS;
    const int zero = (K::ZROW + ((rowi[t] + dr) & (K::NZ - 1))) * K::RS;
    const int live = (int)((mask[t] >> tap) & 1u);
    return zero + live * (on - zero);
  }
};

// Per-tap live cell tiles of an edge-tile layer (Cfg::EDGE) for the waves of row group MG_: a tile whose
// taps read zero padding only would multiply zeros; its MFMAs and operand reads are skipped (the skipped
// contributions are exact zeros).  Used by the 16x16x32 trunks (tower_m16.h, tower_wide16.h).
template <class K, int MG_>
struct XLive {
  static constexpr uint32_t popc(uint32_t m) { return m ? (m & 1u) + popc(m >> 1) : 0u; }
  static constexpr uint32_t ALL = (1u << K::NT) - 1;
  // per-tap live tiles (Cfg::EDGE: a tile can be dead for taps of one dy as well)
  static constexpr uint32_t lt(int tap) {
    uint32_t m = 0;
    for (int t = 0; t < K::NT; ++t)
      if (K::tile_tap_live(MG_ * K::NT + t, tap)) m |= 1u << t;
    return m;
  }
  static constexpr uint32_t ZPRE_T = ALL & ~lt(0);
};

// Channel order in LDS of the 32x32x16 trunk (tower_b32.h; the 16x16x32 trunks: tower_m16.h's phys16).  A lane's 16 accumulator values of a 32x32 MFMA tile are the output channels
// ct*32 + 8g + 4h + j (g, j = 0..3, h = lane half); they are stored at the PHYSICAL positions
// ct*32 + 16h + 4g + j, so that each lane's 16 values are one contiguous 32-byte run (two 16-byte
// LDS stores instead of four 8-byte ones; the epilogue's store burst is the layer boundary's cost).
// The next layer's weights are packed with their input channels in the same physical order
// (evaluator._pack_conv(in_perm=True)), so the MFMAs see consistent K chunks.
__device__ __forceinline__ int phys_off(int ct, int h, int g) { return (ct * 32 + 16 * h + 4 * g) * 2; }

// The two-buffer stems' accumulators start from the bias (b32::stem_layer, m16::stem), so their epilogue is only
// ReLU + convert + store.
template <class K>
__device__ __forceinline__ void acc_init(f32x16 (&acc)[K::MT][K::NT], const float *bias, int wave, int lane) {
  const int h = lane >> 5;
#pragma unroll
  for (int m = 0; m < K::MT; ++m)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int ch = ((wave % K::CG) * K::MT + m) * 32 + 8 * g + 4 * h;
      const float4 bv = *(const float4 *)(bias + ch);
#pragma unroll
      for (int t = 0; t < K::NT; ++t) {
        acc[m][t][4 * g + 0] = bv.x;
        acc[m][t][4 * g + 1] = bv.y;
        acc[m][t][4 * g + 2] = bv.z;
        acc[m][t][4 * g + 3] = bv.w;
      }
    }
}

// 1x1 head convs (C -> C/4 policy | C/4 value) + bias + ReLU, to global features
// [board][cell][C/2] (cell-major: the order the NHWC-reordered linear heads expect).
template <class K>
__device__ __forceinline__ void head_layer(const char *src, const bf16x8 *w, const float *bias, uint16_t *out,
                                           int board0, int batch, int wave, int lane) {
  constexpr int KK = K::C / 16;
  constexpr int GROUPS = K::WAVES / K::HCT;  // waves sharing one head channel tile
  constexpr int TILES = K::ROWS / 32;      // all cell tiles of the workgroup
  constexpr int TPW = TILES / GROUPS;      // cell tiles per wave
  static_assert(K::HCT * GROUPS == K::WAVES && TPW * GROUPS == TILES, "head tile plan");
  const int r = lane & 31, h = lane >> 5;
  const int ct = wave % K::HCT;
  const int t0 = (wave / K::HCT) * TPW;
  f32x16 acc[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
  // all KK weight fragments requested up front: one global-load latency instead of one per group
  bf16x8 wf[KK];
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) wf[kk] = w[((size_t)ct * KK + kk) * 64 + lane];
  // the epilogue's bias too (fetched inside the store loop, each fetch waited behind the stores)
  float4 bvs[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) bvs[g] = *(const float4 *)(bias + ct * 32 + 8 * g + 4 * h);
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) {
    const bf16x8 a = wf[kk];
    const int koff = (kk * 16 + 8 * h) * 2;
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int cell = (t0 + t) * 32 + r;
      const bf16x8 b = lds_b128(src + cell * K::RS + koff);
      acc[t] = K::mfma(a, b, acc[t]);
    }
  }
  // each lane's output rows, looked up once per cell tile (the row -> board/cell table is read from
  // global memory: looked up inside the store loop, every lookup waited for its own load)
  size_t obase[TPW];
  bool okr[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int row = (t0 + t) * 32 + r;
    const int rr = K::row_ok(row) ? row : 0;
    const int board = board0 + K::row_board(rr);
    okr[t] = K::row_ok(row) && board < batch;
    obase[t] = ((size_t)board * K::CELLS + K::row_cell(rr)) * K::HEAD;
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int ch = ct * 32 + 8 * g + 4 * h;
    const float4 bv = bvs[g];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      if (!okr[t]) continue;
      *(uint2 *)(out + obase[t] + ch) = make_uint2(K::relu_pk(f32x2{acc[t][4 * g + 0] + bv.x, acc[t][4 * g + 1] + bv.y}),
                                                   K::relu_pk(f32x2{acc[t][4 * g + 2] + bv.z, acc[t][4 * g + 3] + bv.w}));
    }
  }
}

}  // namespace tower
