// tower_wide16.h — the C = 256 one-buffer trunk on v_mfma_f32_16x16x32_{bf16,f16} (round 5).
//
// Included by tower_kernels.h; tower.hip sizes the residual scratch by Scr.  Uses Cfg (ONEBUF, M16), Ty, Nbr,
// XLive, WBuf, lds_b128 and head_layer from tower_common.h, and lane_row, src_row, conv_tap and stem_store
// from tower_m16.h.
//
// Two ping-pong buffers of a 6-board tile at C = 256 would need 2 x 143.6 KB of LDS, so a two-buffer kernel can
// run C = 256 only on 3-board, board-major tiles (tower_b32.h on 128 rows: no edge-tile skipping, each weight
// fragment serves 128 rows).  With ONE activation buffer the 6-board edge layout of the C = 128 trunk
// (tower_edge.h) runs at C = 256:
//   * 4 waves = 4 channel quarters x all 8 cell tiles.  A conv reads the buffer for all its k-steps with the
//     k-loop of tower_m16.h (each 32-row x 32-channel output tile as 2 x 2 tiles of 16 x 16 over K = 32 input
//     channels, operand rows by lane_row, the phys16 channel order; 12 of the 72 (tile, tap) pairs read zero
//     padding only and are skipped), the waves meet at a barrier, then each wave writes its own output
//     channels of all 256 rows in place, and a second barrier publishes them;
//   * per wave: 4 16-channel tiles (64 output channels: one whole phys16 group, so a lane's 16 outputs of
//     a cell are one contiguous 32-byte run) x 8 cell tiles x 2 row fragments = 64 f32x4 accumulators
//     (the full AGPR file);
//   * the residual of a block's second conv (the block input, overwritten by the first conv's outputs) goes
//     through global memory: the stem and every second conv also store their outputs (the next block input,
//     the same bf16 / fp16 bits as in LDS) to a per-workgroup scratch region (Scr, 128 KB), and the next
//     second conv's epilogue reads them back, each lane its own 32-byte runs (the same lane and tile wrote
//     them two layers earlier; coalesced 16-byte accesses);
//   * the 16x16x32 MFMA holds a higher clock than the 32x32x16 one on the same operands: the trunk ran 6.5 %
//     faster at 1.90 vs 1.80 GHz (profiles/r05/c256/shape_probe.txt).
// Every tile of a launch is a 6-board tile (a batch tail takes one partly empty tile): every board goes
// through the same arithmetic, so outputs are batch-independent bit for bit.  The weight blob is the M16
// layout (evaluator._pack_conv_m16; spmcts_tower_weight_layout reports it for this shape).
#pragma once
#include "tower_common.h"
#include "tower_m16.h"

namespace tower {
namespace wide16 {

using m16::lane_row;
using m16::src_row;

// residual scratch per workgroup: [wave][cell tile t][fragment h][64 lanes] x 32 bytes (the lane's run; soff)
template <class K>
struct Scr {
  static constexpr size_t PER_WG = (size_t)K::WAVES * K::NT * 2 * 64 * 32;
};

// Residual-scratch access through a buffer resource over this workgroup's region: the per-lane part of a
// load's address is one 32-bit voffset (lane * 32 + half * 16) and the (wave, cell tile, fragment) part a
// wave-uniform soffset, instead of 16 hoisted 64-bit addresses (the pointer form spilled 110 VGPRs on them).
// Stores take the whole offset in the voffset and soffset = 0: hipcc (ROCm 7.2) inserts no wait state between
// a buffer_store_dwordx4 whose soffset is an SGPR and a following VALU write of its data VGPRs (LLVM's
// store-data hazard check exempts a register soffset), and on gfx950 that form stored wrong data -- every
// C = 256 output differed (profiles/r04/c256_rsrc/probe_summary.txt: rsrc loads + pointer stores bit-equal,
// pointer loads + SGPR-soffset rsrc stores not).  With soffset = 0 the hazard check applies.
template <class K>
struct ScrBuf {
  static constexpr int AUX = 2;  // gfx950 CPol: nt, as the pointer form's nontemporal accesses
  __amdgpu_buffer_rsrc_t rsrc;
  __device__ __forceinline__ explicit ScrBuf(uint4 *base) {
    rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)base, (short)0, (int)Scr<K>::PER_WG, 0x00020000);
  }
  __device__ __forceinline__ uint4 load(int lane, int half, int so) const {
    return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane * 32 + half * 16, so, AUX));
  }
  __device__ __forceinline__ void store(uint4 v, int lane, int half, int so) const {
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, v), rsrc, lane * 32 + half * 16 + so, 0, AUX);
  }
};

// the stem's bias, per 32-channel tile m of the wave and accumulator group g
template <class K>
__device__ __forceinline__ void load_bias(float4 (&bv)[K::MT][4], const float *bias, int wave, int lane) {
#pragma unroll
  for (int m = 0; m < K::MT; ++m)
#pragma unroll
    for (int g = 0; g < 4; ++g) bv[m][g] = *(const float4 *)(bias + (wave * K::MT + m) * 32 + 8 * g + 4 * (lane >> 5));
}

template <class K>
__device__ __forceinline__ int soff(int wave, int t, int h) {
  return ((wave * K::NT + t) * 2 + h) * 64 * 32;
}

// In place: out = relu(acc + bias (+ the block input from scratch)); SAVE also stores the outputs to
// scratch (the next block's residual).  Every wave has finished reading the buffer (barrier before); a
// barrier publishes the outputs.
template <class K, bool RESID, bool SAVE>
__device__ __forceinline__ void epilogue(char *X, const f32x4 (&acc)[4][K::NT][2], const float4 (&bv)[4], uint4 *scr,
                                         int wave, int q, int rb, int lane) {
  const ScrBuf<K> sb(scr);
  const int wu = __builtin_amdgcn_readfirstlane(wave);
  const int ro = (64 * wave + 16 * q) * 2;  // the lane's run: channels 64 wave + 16 q .. + 16 (phys16)
  // residual reads two cell tiles at a time (32 registers in flight beside the 256 accumulator AGPRs)
  constexpr int TB = 2;
#pragma unroll
  for (int t0 = 0; t0 < K::NT; t0 += TB) {
    uint4 res[RESID ? TB : 1][2][2];
    if constexpr (RESID) {
#pragma unroll
      for (int i = 0; i < TB; ++i)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int so = soff<K>(wu, t0 + i, h);
          res[i][h][0] = sb.load(lane, 0, so);
          res[i][h][1] = sb.load(lane, 1, so);
        }
    }
#pragma unroll
    for (int i = 0; i < TB; ++i) {
      const int t = t0 + i;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        char *p = X + (t * 32 + rb + h) * K::RS + ro;
        uint32_t o[8];
#pragma unroll
        for (int mm = 0; mm < 4; ++mm) {
          // physical 4 mm + r within the run: output channel 64 wave + 16 mm + 4 q + r
          float v0 = acc[mm][t][h][0] + bv[mm].x, v1 = acc[mm][t][h][1] + bv[mm].y;
          float v2 = acc[mm][t][h][2] + bv[mm].z, v3 = acc[mm][t][h][3] + bv[mm].w;
          if constexpr (RESID) {
            const f32x2 x0 = K::unpk(((const uint32_t *)&res[i][h][mm >> 1])[2 * (mm & 1)]);
            const f32x2 x1 = K::unpk(((const uint32_t *)&res[i][h][mm >> 1])[2 * (mm & 1) + 1]);
            v0 += x0[0];
            v1 += x0[1];
            v2 += x1[0];
            v3 += x1[1];
          }
          o[2 * mm] = K::relu_pk(f32x2{v0, v1});
          o[2 * mm + 1] = K::relu_pk(f32x2{v2, v3});
        }
        const uint4 lo = make_uint4(o[0], o[1], o[2], o[3]), hi = make_uint4(o[4], o[5], o[6], o[7]);
        *(uint4 *)p = lo;
        *(uint4 *)(p + 16) = hi;
        if constexpr (SAVE) {
          const int so = soff<K>(wu, t, h);
          sb.store(lo, lane, 0, so);
          sb.store(hi, lane, 1, so);
        }
      }
    }
  }
  __syncthreads();
}

// One 3x3 conv over the resident tile, in place: tower_m16.h's k-loop (conv_tap, one channel quarter, all
// cell tiles), then the in-place epilogue.
template <class K, int DEPTH, bool RESID, bool SAVE>
__device__ __forceinline__ void conv(char *X, const Nbr<K> &nb, bf16x8 (&a)[DEPTH][4], const float *bias, int wave,
                                     int lane, const WBuf &wb, uint32_t wl_off, uint32_t wn_off, uint4 *scr,
                                     float *sbias) {
  using Xl = XLive<K, 0>;
  constexpr int KK32 = K::C / 32;
  static_assert(K::C == K::THREADS, "one bias value per thread");
  static_assert(KK32 % DEPTH == 0, "ring slot must be a compile-time function of k");
  const int q = lane >> 4, rb = lane_row(lane & 15), qoff = 16 * q;
  // the epilogue's bias: one value per thread now, staged in LDS after the k-loop (1 register
  // through the k-loop instead of 32; the previous layer's epilogue finished reading the staging area at its
  // closing barrier)
  const float bmine = bias[threadIdx.x];
  f32x4 acc[4][K::NT][2];
#pragma unroll
  for (int t = 0; t < K::NT; ++t)
#pragma unroll
    for (int mm = 0; mm < 4; ++mm)
      if ((Xl::ZPRE_T >> t) & 1u) acc[mm][t][0] = acc[mm][t][1] = f32x4{};
  int off_cur[K::NT][2], off_nxt[K::NT][2];
  bf16x8 bc[K::NT][2], bn[K::NT][2];
#pragma unroll
  for (int t = 0; t < K::NT; ++t)
    if ((Xl::lt(0) >> t) & 1u) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        off_cur[t][h] = src_row(nb, 0, t, h, rb, 0) * K::RS + qoff;
        bc[t][h] = lds_b128(X + off_cur[t][h]);
      }
    }
#define TAPW16(T) \
  m16::conv_tap<K, KK32, DEPTH, 0, T>(X, nb, acc, bc, bn, off_cur, off_nxt, a, qoff, rb, wb, wl_off, wn_off)
  TAPW16(0); TAPW16(1); TAPW16(2); TAPW16(3); TAPW16(4); TAPW16(5); TAPW16(6); TAPW16(7); TAPW16(8);
#undef TAPW16
  sbias[threadIdx.x] = bmine;
  __syncthreads();  // every wave has read the layer input: outputs may overwrite it
  float4 bv[4];
#pragma unroll
  for (int mm = 0; mm < 4; ++mm) bv[mm] = *(const float4 *)(sbias + 16 * (4 * wave + mm) + 4 * q);
  epilogue<K, RESID, SAVE>(X, acc, bv, scr, wave, q, rb, lane);
}

// Stem (3 planes padded to one 16-channel k-step per tap, on 32x32x16 MFMAs, bias in the
// accumulators), stored in the phys16 order in place; then each lane copies its runs (the first block's
// input) to scratch in the layout the epilogue reads.
template <class K>
__device__ __forceinline__ void stem(char *X, const Nbr<K> &nb, const bf16x8 *w, const float *bias, int wave, int lane,
                                     uint4 *scr) {
  const int h = lane >> 5;
  f32x16 acc[K::MT][K::NT];
  float4 bv[K::MT][4];
  load_bias<K>(bv, bias, wave, lane);
#pragma unroll
  for (int m = 0; m < K::MT; ++m)
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int t = 0; t < K::NT; ++t) {
        acc[m][t][4 * g + 0] = bv[m][g].x;
        acc[m][t][4 * g + 1] = bv[m][g].y;
        acc[m][t][4 * g + 2] = bv[m][g].z;
        acc[m][t][4 * g + 3] = bv[m][g].w;
      }
  bf16x8 a[9][K::MT];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int m = 0; m < K::MT; ++m) a[tap][m] = w[((size_t)(wave * K::MT + m) * 9 + tap) * 64 + lane];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
    for (int t = 0; t < K::NT; ++t) {
      const bf16x8 b = lds_b128(X + nb.off(t, tap) + 16 * h);
#pragma unroll
      for (int m = 0; m < K::MT; ++m) acc[m][t] = K::mfma(a[tap][m], b, acc[m][t]);
    }
  }
  __syncthreads();  // every wave has read the stem input
  m16::stem_store<K>(acc, X, wave, lane);
  __syncthreads();
  const ScrBuf<K> sb(scr);
  const int wu = __builtin_amdgcn_readfirstlane(wave);
  const int q = lane >> 4, rb = lane_row(lane & 15), ro = (64 * wave + 16 * q) * 2;
#pragma unroll
  for (int t = 0; t < K::NT; ++t)
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const char *p = X + (t * 32 + rb + hh) * K::RS + ro;
      const int so = soff<K>(wu, t, hh);
      sb.store(*(const uint4 *)p, lane, 0, so);
      sb.store(*(const uint4 *)(p + 16), lane, 1, so);
    }
}

// One workgroup's tile: boards [board0, board0 + BOARDS), all layers; scr = this workgroup's residual
// scratch (Scr<K>::PER_WG bytes).
template <class K>
__device__ __forceinline__ void tile(char *smem, const __bf16 *planes, int batch, int board0, int n_blocks,
                                     const bf16x8 *wpk, const float *bias, uint16_t *out, uint4 *scr) {
  static_assert(K::EDGE && K::ONEBUF && K::M16 && K::MG == 1 && K::CG == 4 && K::WAVES == 4 && K::C == 256,
                "wide16 trunk: C = 256 6-board edge tiles, one buffer, 4 channel quarters x all cell tiles");
  char *X = smem;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  Nbr<K> nb;
  nb.init(lane & 31, 0);
  for (int i = tid; i < K::NZ * K::RS / 4; i += K::THREADS) ((uint32_t *)(X + K::ZROW * K::RS))[i] = 0u;
  uint16_t *tab = (uint16_t *)(smem + K::BUF);
  float *sbias = (float *)(smem + K::BUF + K::TAB);
#pragma unroll
  for (int j = 0; j < (9 * K::ROWS + K::THREADS - 1) / K::THREADS; ++j)
    if (9 * K::ROWS % K::THREADS == 0 || tid + j * K::THREADS < 9 * K::ROWS)
      tab[tid + j * K::THREADS] = kEdgeNbr[tid + j * K::THREADS];
  nb.tab = tab;
  for (int row = tid; row < K::ROWS; row += K::THREADS) {
    const int board = board0 + K::row_board(row);
    uint16_t *dst = (uint16_t *)(X + row * K::RS);
    const bool ok = K::row_ok(row) && board < batch;
    const size_t src = ((size_t)board * K::CELLS + K::row_cell(row)) * 3;
#pragma unroll
    for (int c = 0; c < 16; ++c) dst[c] = (ok && c < 3) ? K::from_bf16(planes[src + c]) : (uint16_t)0;
  }
  __syncthreads();
  nb.finish();
  constexpr int KK32 = K::C / 32;
  constexpr int DEPTH = K::DEPTH;
  constexpr size_t STEM = (size_t)K::C / 32 * 9 * 64;         // stem fragments (32x32x16 layout)
  constexpr size_t LAYER = (size_t)K::C / 16 * 9 * KK32 * 64;  // one block conv's fragments (16x16x32 layout)
  constexpr int LSTEPS = 9 * KK32;
  stem<K>(X, nb, wpk, bias, wave, lane, scr);
  const bf16x8 *wblk = wpk + STEM;
  const float *b = bias + K::C;
  // per-wave weight streams: layer L, 16-channel tile (4 wave + mm) at wblk + L*LAYER + (4 wave + mm)*LSTEPS*64
  bf16x8 ring[DEPTH][4];
  const int n_convs = 2 * n_blocks;
  if (n_convs > 0) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
#pragma unroll
      for (int mm = 0; mm < 4; ++mm) ring[d][mm] = wblk[(size_t)(4 * wave + mm) * LSTEPS * 64 + (size_t)d * 64 + lane];
  }
  WBuf wb;
  wb.rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)wpk, (short)0, 0x7fffffff, 0x00020000);
  wb.voff = lane * 16;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const uint32_t ct0_off = (uint32_t)(STEM + (size_t)(4 * wave_u) * LSTEPS * 64) * 16u;
  // one iteration per residual block: its first conv, then its second (residual + save) -- a straight line,
  // where an odd/even branch per conv made the register allocator merge the two bodies' live ranges at the
  // branch (66 spilled VGPRs, reloaded there)
  for (int L = 0; L < n_convs; L += 2) {
    const uint32_t wl_off = ct0_off + (uint32_t)((size_t)L * LAYER * 16u);
    conv<K, DEPTH, false, false>(X, nb, ring, b, wave, lane, wb, wl_off, wl_off + (uint32_t)(LAYER * 16u), scr, sbias);
    b += K::C;
    const uint32_t wl1 = wl_off + (uint32_t)(LAYER * 16u);
    const uint32_t wn1 = L + 2 == n_convs ? wl1 : wl1 + (uint32_t)(LAYER * 16u);
    conv<K, DEPTH, true, true>(X, nb, ring, b, wave, lane, wb, wl1, wn1, scr, sbias);
    b += K::C;
  }
  head_layer<K>(X, wblk + (size_t)n_convs * LAYER, b, out, board0, batch, wave, lane);
}

}  // namespace wide16
}  // namespace tower
