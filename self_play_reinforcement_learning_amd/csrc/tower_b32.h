// tower_b32.h — the board-major two-buffer trunk on v_mfma_f32_32x32x16_{bf16,f16}, the first of the three
// families.  Today it serves the 3x3 boards (C = 128 with its 256 / 192 / 128-row tail tiles, C = 256 on
// 128 rows) and the A/B library's 3-board 7x6 C = 256 set (tower_ab.h); the 7x6 product shapes run on
// tower_m16.h (C = 128) and tower_wide16.h (C = 256).
//
// Included by tower_kernels.h.  Uses Cfg, Ty, Nbr, WBuf, lds_b128, phys_off, acc_init and head_layer from
// tower_common.h.
//
// One workgroup owns BOARDS whole boards (ROWS = 256, 192 or 128 cell rows, NHWC; row = board * CELLS + x * H + y)
// and keeps their activations resident in LDS for the whole tower: two ping-pong buffers X / Y of (ROWS + 16)
// rows x (C*2 + 16) bytes (the +16 pad makes the 16-byte MFMA operand reads bank-conflict free; rows ROWS.. are
// all zeros and stand for the conv's zero padding).  A 3x3 conv is an implicit GEMM
//     out[c_out][cell] = sum_{tap, c_in} W[c_out][tap][c_in] * act[nbr(cell, tap)][c_in]
// with A = weights (32 output channels x 16 k), streamed from global memory (L2/MALL resident, pre-swizzled so
// every wave reads one contiguous 1 KiB fragment per k-step), B = activations (16 k x 32 cells) read from LDS at
// the affine neighbour offsets of Nbr::off.  Each wave owns 64 output channels for its share of the cells; fp32
// accumulators, bf16 / fp16 activations between layers.  The activations never leave the CU.
#pragma once
#include <type_traits>

#include "tower_common.h"

namespace tower {
namespace b32 {

// Epilogue (the first k-step's MFMAs start from zero; bias and residual are added here): out = relu(acc +
// bias (+ dst)), into dst, with the bias already in registers (bv[m][g] = bias[ch(m, g) .. + 4], loaded at the
// start of the layer so its global-load latency hides under the k-loop instead of stalling the epilogue).
template <class K, bool RESID>
__device__ __forceinline__ void acc_store_bias_relu_pre(const f32x16 (&acc)[K::MT][K::NT], char *dst,
                                                        const float4 (&bv)[K::MT][4], int wave, int lane) {
  const int r = lane & 31, h = lane >> 5;
  // per channel tile m: the residuals (block input) of its NT output runs are read in one batch
  // before any of them is written, so the LDS latency is paid once per batch instead of once per
  // read -> add -> write chain; each run is the lane's 16 channels, contiguous (phys_off)
#pragma unroll
  for (int m = 0; m < K::MT; ++m) {
    const int ct = (wave % K::CG) * K::MT + m;
    uint4 res[RESID ? K::NT : 1][2];
    if constexpr (RESID) {
#pragma unroll
      for (int t = 0; t < K::NT; ++t) {
        const char *p = dst + (((wave / K::CG) * K::NT + t) * 32 + r) * K::RS + phys_off(ct, h, 0);
        res[t][0] = *(const uint4 *)p;
        res[t][1] = *(const uint4 *)(p + 16);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int t = 0; t < K::NT; ++t) {
      char *p = dst + (((wave / K::CG) * K::NT + t) * 32 + r) * K::RS + phys_off(ct, h, 0);
      uint32_t o[8];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        float v0 = acc[m][t][4 * g + 0] + bv[m][g].x, v1 = acc[m][t][4 * g + 1] + bv[m][g].y;
        float v2 = acc[m][t][4 * g + 2] + bv[m][g].z, v3 = acc[m][t][4 * g + 3] + bv[m][g].w;
        if constexpr (RESID) {
          const f32x2 x0 = K::unpk(((const uint32_t *)&res[t][g >> 1])[2 * (g & 1)]);
          const f32x2 x1 = K::unpk(((const uint32_t *)&res[t][g >> 1])[2 * (g & 1) + 1]);
          v0 += x0[0];
          v1 += x0[1];
          v2 += x1[0];
          v3 += x1[1];
        }
        // ReLU on the converted pairs (bf16: v_cvt_pk_bf16_f32 + v_pk_max_i16: identical bits to
        // converting max(v, 0), one instruction per pair instead of one per value)
        o[2 * g] = K::relu_pk(f32x2{v0, v1});
        o[2 * g + 1] = K::relu_pk(f32x2{v2, v3});
      }
      *(uint4 *)p = make_uint4(o[0], o[1], o[2], o[3]);
      *(uint4 *)(p + 16) = make_uint4(o[4], o[5], o[6], o[7]);
    }
  }
}

template <class K>
__device__ __forceinline__ void acc_store_relu(const f32x16 (&acc)[K::MT][K::NT], char *dst, int wave, int lane) {
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int m = 0; m < K::MT; ++m)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
      for (int t = 0; t < K::NT; ++t) {
        const uint2 o = make_uint2(K::relu_pk(f32x2{acc[m][t][4 * g + 0], acc[m][t][4 * g + 1]}),
                                   K::relu_pk(f32x2{acc[m][t][4 * g + 2], acc[m][t][4 * g + 3]}));
        *(uint2 *)(dst + (((wave / K::CG) * K::NT + t) * 32 + r) * K::RS + phys_off((wave % K::CG) * K::MT + m, h, g)) = o;
      }
    }
}

// One 3x3 conv layer over the resident tile: src (LDS) -> dst (LDS); RESID adds dst's old
// contents (the block input).  KK = input channels / 16 (k-steps per tap).
// Software pipeline: the NT B (activation) fragments of step s+1 are read from LDS while the
// MFMAs of step s run; the A (weight) fragment ring runs DEPTH steps ahead and continues into
// the next layer's weights (wn_off), so a layer starts with its first weights already in registers.
template <class K, int KK, int DEPTH, bool RESID>
__device__ __forceinline__ void conv_layer(const char *src, char *dst, const Nbr<K> &nb, bf16x8 (&a)[DEPTH][K::MT],
                                           const float *bias, int wave, int lane, const WBuf &wb, uint32_t wl_off,
                                           uint32_t wn_off) {
  // wl_off / wn_off: byte offset of (this layer / next layer, this wave's first channel tile, step 0);
  // channel tile m adds m * 9 * KK fragments of 1 KiB, step s adds s KiB
  constexpr uint32_t MSTRIDE = 9u * KK * 1024u;
  constexpr int STEPS = 9 * KK;
  static_assert(KK % DEPTH == 0, "ring slot must be a compile-time function of kk");
  const int h = lane >> 5;
  f32x16 acc[K::MT][K::NT];  // the first k-step starts from zero; bias and residual are added in the epilogue
  const int hoff = 16 * h;  // byte offset of this lane's 8 channels inside a 16-channel k-step
  // the epilogue's bias, fetched now, so the global-load latency hides under the k-loop
  float4 bv[K::MT][4];
#pragma unroll
  for (int m = 0; m < K::MT; ++m)
#pragma unroll
    for (int g = 0; g < 4; ++g) bv[m][g] = *(const float4 *)(bias + ((wave % K::CG) * K::MT + m) * 32 + 8 * g + 4 * h);
  int off_cur[K::NT], off_nxt[K::NT];
#pragma unroll
  for (int t = 0; t < K::NT; ++t) off_cur[t] = nb.off(t, 0) + hoff;
  bf16x8 bc[K::NT], bn[K::NT];
#pragma unroll
  for (int t = 0; t < K::NT; ++t) bc[t] = lds_b128(src + off_cur[t]);

  // taps fully unrolled: a straight-line k-loop schedules 4-7 % faster than a rolled tap loop
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    if (tap + 1 < 9) {
#pragma unroll
      for (int t = 0; t < K::NT; ++t) off_nxt[t] = nb.off(t, tap + 1) + hoff;
    }
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      const int s = tap * KK + kk;
      if (kk + 1 < KK) {
#pragma unroll
        for (int t = 0; t < K::NT; ++t) bn[t] = lds_b128(src + off_cur[t] + (kk + 1) * 32);
      } else if (tap + 1 < 9) {
#pragma unroll
        for (int t = 0; t < K::NT; ++t) bn[t] = lds_b128(src + off_nxt[t]);
      }
      const int slot = kk % DEPTH;
      bf16x8 acur[K::MT];
#pragma unroll
      for (int m = 0; m < K::MT; ++m) acur[m] = a[slot][m];
      const int sn = s + DEPTH;
      if (sn < STEPS) {
#pragma unroll
        for (int m = 0; m < K::MT; ++m) a[slot][m] = wb.load(wl_off + m * MSTRIDE + (uint32_t)sn * 1024u);
      } else {
        // The weight ring's loads for the next layer's first DEPTH k-steps are issued unconditionally (the
        // last conv re-reads its own first steps, discarded): a conditional load made hipcc merge the ring
        // registers with copies at every layer's last k-step, behind an s_waitcnt vmcnt(0) that drained
        // the whole weight pipeline once per layer.
#pragma unroll
        for (int m = 0; m < K::MT; ++m) a[slot][m] = wb.load(wn_off + m * MSTRIDE + (uint32_t)(sn - STEPS) * 1024u);
      }
      if (s == 0) {
#pragma unroll
        for (int t = 0; t < K::NT; ++t)
#pragma unroll
          for (int m = 0; m < K::MT; ++m)
            acc[m][t] = K::mfma(acur[m], bc[t], f32x16{});
      } else {
#pragma unroll
        for (int t = 0; t < K::NT; ++t)
#pragma unroll
          for (int m = 0; m < K::MT; ++m)
            acc[m][t] = K::mfma(acur[m], bc[t], acc[m][t]);
      }
      // interleave this step's loads (next B fragments, ring refill) between its MFMAs:
      // one LDS read or global load per MFMA gap instead of a burst between MFMA blocks
#pragma unroll
      for (int i = 0; i < K::NT; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // DS read
      }
#pragma unroll
      for (int i = 0; i < K::MT; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // VMEM read
      }
      __builtin_amdgcn_sched_group_barrier(0x008, K::MT * K::NT - K::NT - K::MT, 0);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < K::NT; ++t) bc[t] = bn[t];
    }
#pragma unroll
    for (int t = 0; t < K::NT; ++t) off_cur[t] = off_nxt[t];
  }
  acc_store_bias_relu_pre<K, RESID>(acc, dst, bv, wave, lane);
}

// Stem: 3 input planes padded to one 16-channel k-step per tap (9 steps, weights loaded in place).
template <class K>
__device__ __forceinline__ void stem_layer(const char *src, char *dst, const Nbr<K> &nb, const bf16x8 *w,
                                           const float *bias, int wave, int lane) {
  const int h = lane >> 5;
  f32x16 acc[K::MT][K::NT];
  acc_init<K>(acc, bias, wave, lane);
  bf16x8 a[9][K::MT];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int m = 0; m < K::MT; ++m) a[tap][m] = w[((size_t)((wave % K::CG) * K::MT + m) * 9 + tap) * 64 + lane];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
    for (int t = 0; t < K::NT; ++t) {
      const bf16x8 b = lds_b128(src + nb.off(t, tap) + 16 * h);
#pragma unroll
      for (int m = 0; m < K::MT; ++m)
        acc[m][t] = K::mfma(a[tap][m], b, acc[m][t]);
    }
  }
  acc_store_relu<K>(acc, dst, wave, lane);
}

// One workgroup's tile: boards [board0, board0 + BOARDS) of the batch (board < batch), all layers.  It takes the
// kernels' own argument list (no scratch is used) because the kernels call it directly (tower_kernels.h): behind
// a dispatching wrapper, one more level of inlining, every kernel of this family compiles to other code (335 to
// 1,413 lines of assembly each: another layout of the stem-input loop, another register allocation).
template <class K>
__device__ __forceinline__ std::enable_if_t<!K::M16> tile(char *smem, const __bf16 *planes, int batch, int board0,
                                                          int n_blocks, const bf16x8 *wpk, const float *bias,
                                                          uint16_t *out, uint4 *) {
  char *X = smem;
  char *Y = smem + K::BUF;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  Nbr<K> nb;
  nb.init(lane & 31, wave / K::CG);

  // zero rows + stem input: Y rows hold 16 channels (3 planes, 13 zeros)
  for (int i = tid; i < K::NZ * K::RS / 4; i += K::THREADS) {
    ((uint32_t *)(X + K::ZROW * K::RS))[i] = 0u;
    ((uint32_t *)(Y + K::ZROW * K::RS))[i] = 0u;
  }
  for (int row = tid; row < K::ROWS; row += K::THREADS) {
    const int board = board0 + K::row_board(row);
    uint16_t *dst = (uint16_t *)(Y + row * K::RS);
    const bool ok = K::row_ok(row) && board < batch;
    const size_t src = ((size_t)board * K::CELLS + K::row_cell(row)) * 3;
#pragma unroll
    for (int c = 0; c < 16; ++c) dst[c] = (ok && c < 3) ? K::from_bf16(planes[src + c]) : (uint16_t)0;
  }
  __syncthreads();
  nb.finish();

  constexpr int KK = K::C / 16;
  constexpr int DEPTH = K::DEPTH;
  constexpr size_t STEM = (size_t)K::C / 32 * 9 * 64;          // stem fragments
  constexpr size_t LAYER = (size_t)K::C / 32 * 9 * KK * 64;     // one block conv's fragments
  constexpr int LSTEPS = 9 * KK;
  stem_layer<K>(Y, X, nb, wpk, bias, wave, lane);
  __syncthreads();
  const bf16x8 *wblk = wpk + STEM;
  const float *b = bias + K::C;
  // per-wave weight streams: layer L, ctile (wave*MT + m) starts at wblk + L*LAYER + ct*LSTEPS*64 + lane
  bf16x8 ring[DEPTH][K::MT];
  const int n_convs = 2 * n_blocks;
  if (n_convs > 0) {
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
#pragma unroll
      for (int m = 0; m < K::MT; ++m)
        ring[d][m] = wblk[(size_t)((wave % K::CG) * K::MT + m) * LSTEPS * 64 + (size_t)d * 64 + lane];
  }
  WBuf wb;
  wb.rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)wpk, (short)0, 0x7fffffff, 0x00020000);
  wb.voff = lane * 16;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const uint32_t ct0_off = (uint32_t)(STEM + (size_t)((wave_u % K::CG) * K::MT) * LSTEPS * 64) * 16u;
  for (int L = 0; L < n_convs; ++L) {
    const uint32_t wl_off = ct0_off + (uint32_t)((size_t)L * LAYER * 16u);
    const uint32_t wn_off = L + 1 == n_convs ? wl_off : wl_off + (uint32_t)(LAYER * 16u);
    if ((L & 1) == 0) {
      conv_layer<K, KK, DEPTH, false>(X, Y, nb, ring, b, wave, lane, wb, wl_off, wn_off);
    } else {
      conv_layer<K, KK, DEPTH, true>(Y, X, nb, ring, b, wave, lane, wb, wl_off, wn_off);
    }
    b += K::C;
    __syncthreads();
  }
  const bf16x8 *w = wblk + (size_t)n_convs * LAYER;
  head_layer<K>(X, w, b, out, board0, batch, wave, lane);
}

}  // namespace b32
}  // namespace tower
