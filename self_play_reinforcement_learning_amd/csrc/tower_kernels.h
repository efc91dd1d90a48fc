// tower_kernels.h — the fused trunk's kernel entry points (namespace tower): one launch evaluates stem conv3x3,
// n_blocks BasicBlocks and the two 1x1 head convs of games/general/modules.py ResidualTower for a batch of
// boards, BatchNorm folded into the conv weights / bias on the host (eval-mode statistics).  tile<K> picks
// the family of a tile plan (Cfg); k_tower takes the batch size from the host, k_tower_dyn from device memory.
//
// Included by tower.hip.  Uses Cfg and bf16x8 from tower_common.h and tile<K> of the three families:
// b32 (tower_b32.h), m16 (tower_m16.h), wide16 (tower_wide16.h, with its per-workgroup scratch Scr).
#pragma once
#include <type_traits>

#include "tower_b32.h"
#include "tower_common.h"
#include "tower_m16.h"
#include "tower_wide16.h"

namespace tower {

// Packed weight blob (bf16x8 units) and bias blob (floats), in layer order (SPMCTS_WLAYOUT_32X32; the block
// convs of the M16 layout: tower_m16.h):
//   stem   [C/32][9][1][64 lanes]      k = 16 input channels (3 planes + 13 zero)
//   block  2 x [C/32][9][C/16][64]      per BasicBlock (conv1, conv2)
//   head   [C/64][1][C/16][64]          policy C/4 | value C/4 output channels
// lane l of fragment (ct, tap, kk) holds W[ct*32 + (l & 31)][tap][kk*16 + 8*(l >> 5) + j], j = 0..7.
// bias: stem C, blocks 2*C each, head C/2.

// One workgroup's tile: boards [board0, board0 + BOARDS) of the batch (board < batch), all layers, by the
// plan's family: three overloads, one of which accepts a given K.  The board-major one is b32::tile itself
// (see there why it is not wrapped); scr = the launch's residual scratch (one-buffer plans; else null).
using b32::tile;
template <class K>
__device__ __forceinline__ std::enable_if_t<K::M16 && !K::ONEBUF> tile(char *smem, const __bf16 *planes, int batch,
                                                                       int board0, int n_blocks, const bf16x8 *wpk,
                                                                       const float *bias, uint16_t *out, uint4 *) {
  m16::tile<K>(smem, planes, batch, board0, n_blocks, wpk, bias, out);
}
template <class K>
__device__ __forceinline__ std::enable_if_t<K::ONEBUF> tile(char *smem, const __bf16 *planes, int batch, int board0,
                                                            int n_blocks, const bf16x8 *wpk, const float *bias,
                                                            uint16_t *out, uint4 *scr) {
  wide16::tile<K>(smem, planes, batch, board0, n_blocks, wpk, bias, out, scr + blockIdx.x * (wide16::Scr<K>::PER_WG / 16));
}

template <class K>
__global__ __launch_bounds__(K::THREADS) __attribute__((amdgpu_waves_per_eu(K::WAVES / 4 * K::OCC, K::WAVES / 4 * K::OCC))) void k_tower(
    const __bf16 *planes, int batch, int n_blocks, const bf16x8 *wpk, const float *bias, uint16_t *out, uint4 *scr) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  tile<K>(smem, planes, batch, blockIdx.x * K::BOARDS, n_blocks, wpk, bias, out, scr);
}

// Tail tile for a remainder of `rem` boards after whole rounds of full tiles: the smallest tile
// (fewest LDS rows, so the shortest workgroup) whose one round of `cus` workgroups covers it.
// 0 = half (KH), 1 = middle (KM), 2 = full (KF).
template <class KF, class KM, class KH>
__host__ __device__ __forceinline__ int tail_kind(int rem, int cus) {
  if (rem <= cus * KH::BOARDS) return 0;
  if (rem <= cus * KM::BOARDS) return 1;
  return 2;
}

// Device-count driven variant: the batch size is read from device memory (the arena's leaf-row
// counter), so the host never waits for it.  Workgroups are assigned in whole
// chip rounds of full-size tiles, then the remainder in one round of the smallest tile that covers
// it (tail_kind); surplus workgroups of the (maximum-size) grid exit at once.
template <class KF, class KM, class KH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_tower_dyn(
    const __bf16 *planes, const int32_t *count, int max_batch, int cus, int n_blocks, const bf16x8 *wpk,
    const float *bias, uint16_t *out, uint4 *scr) {
  static_assert(KF::THREADS == 256 && KM::THREADS == 256 && KH::THREADS == 256, "one block size");
  // residual scratch is sized per workgroup of the full tiles (wide16::Scr<KF>, tower.hip's launch): a one-buffer tail tile
  // must be the full tile itself
  static_assert((!KM::ONEBUF || std::is_same<KM, KF>::value) && (!KH::ONEBUF || std::is_same<KH, KF>::value),
                "one-buffer tail tiles must be the full tiles");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int n = min(*count, max_batch);  // never past the caller's buffers
  const int full_wgs = (n / KF::BOARDS) / cus * cus;
  const int n_full = full_wgs * KF::BOARDS;
  const int rem = n - n_full;
  const int b = blockIdx.x;
  if constexpr (std::is_same<KM, KF>::value && std::is_same<KH, KF>::value) {
    // one tile kind: one inlined copy of the tile body (whole rounds and the tail alike)
    const int board0 = b < full_wgs ? b * KF::BOARDS : n_full + (b - full_wgs) * KF::BOARDS;
    if (board0 < n) tile<KF>(smem, planes, n, board0, n_blocks, wpk, bias, out, scr);
    return;
  }
  if (b < full_wgs) {
    tile<KF>(smem, planes, n, b * KF::BOARDS, n_blocks, wpk, bias, out, scr);
    return;
  }
  const int j = b - full_wgs;
  const int kind = tail_kind<KF, KM, KH>(rem, cus);
  if (kind == 0) {
    if (n_full + j * KH::BOARDS < n) tile<KH>(smem, planes, n, n_full + j * KH::BOARDS, n_blocks, wpk, bias, out, scr);
  } else if (kind == 1) {
    if (n_full + j * KM::BOARDS < n) tile<KM>(smem, planes, n, n_full + j * KM::BOARDS, n_blocks, wpk, bias, out, scr);
  } else {
    if (n_full + j * KF::BOARDS < n) tile<KF>(smem, planes, n, n_full + j * KF::BOARDS, n_blocks, wpk, bias, out, scr);
  }
}

}  // namespace tower
