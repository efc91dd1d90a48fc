// tower_boards.hip — the fused trunk and heads for the Connect4 variant boards 6x5 ("connect4_6_5") and 8x7
// ("connect4_8_7"): host side of the add-on library libspmcts_boards.so.  The product library (tower.hip) holds
// exactly the kernels of the four shipped (C, W, H) sets; the variant boards' kernels live here, in a library of
// their own that is loaded only when such a net is evaluated (_lib.boards_lib).  It exports the six
// spmcts_tower_* entry points of include/spmcts.h with the same signatures and return codes (-2 for a shape it
// does not hold, 7x6 and 3x3 among them).
//
// The device code is the product's: the board-major 32x32x16 family (tower_b32.h) through k_tower / k_tower_dyn
// (tower_kernels.h), and k_heads_co (tower_heads.h).  Every tile holds whole boards and no layer reads across a
// board, so a board's outputs do not depend on the batch it is in (leaf dedup and the evaluation cache rely on it).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spmcts.h"
#include "tower_heads.h"
#include "tower_kernels.h"

namespace tower {

static int num_cus() {
  static int n = 0;
  if (!n) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        n <= 0)
      n = 256;
  }
  return n;
}

// One trunk launch, as tower.hip's (kept apart so that tower.hip's object does not change): the kernel's
// dynamic-LDS limit raised once (-10), the launch (-11).  Two-buffer tiles only: no residual scratch.
template <auto Kern, class K, int LDS, class... Args>
static int launch(int grid, hipStream_t s, Args... args) {
  static_assert(!K::ONEBUF, "the variant boards run on two-buffer tiles");
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute((const void *)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, LDS) != hipSuccess)
      return -10;
    attr_set = true;
  }
  hipLaunchKernelGGL(Kern, dim3(grid), dim3(K::THREADS), LDS, s, args..., (uint4 *)nullptr);
  return hipGetLastError() == hipSuccess ? 0 : -11;
}

// F / M / H = the full / middle / half tiles of the device-count path; the host-count path runs F alone.
template <int A_, class F_, class M_ = F_, class H_ = F_>
struct TileSet {
  static constexpr int A = A_;
  using F = F_;
  using M = M_;
  using H = H_;
};
// C = 128: 256-row tiles (8 boards of 6x5, 4 of 8x7), a batch ending on a 192- or 128-row tile; C = 256: 128-row
// tiles (4 boards of 6x5, 2 of 8x7), the most two buffers of 528-byte rows leave room for in 160 KB of LDS
template <int W, int H, class E>
using TilesC128 = TileSet<W, BoardMajor32<128, 256, W, H, E>, BoardMajor32<128, 192, W, H, E>, BoardMajor32<128, 128, W, H, E>>;
template <int W, int H, class E>
using TilesC256 = TileSet<W, BoardMajor32<256, 128, W, H, E>>;

// The one (dtype, width, height, channels) switch: f(the shape's tile set for the element type), or -2.
template <class E, class Fn>
static int with_tiles_of(int32_t width, int32_t height, int32_t channels, Fn &&f) {
  if (channels != 128 && channels != 256) return -2;
  if (width == 6 && height == 5) return channels == 128 ? f(TilesC128<6, 5, E>{}) : f(TilesC256<6, 5, E>{});
  if (width == 8 && height == 7) return channels == 128 ? f(TilesC128<8, 7, E>{}) : f(TilesC256<8, 7, E>{});
  return -2;
}
template <class Fn>
static int with_tiles(int32_t flags, int32_t width, int32_t height, int32_t channels, Fn &&f) {
  return flags & SPMCTS_TOWER_F16 ? with_tiles_of<_Float16>(width, height, channels, f)
                                  : with_tiles_of<__bf16>(width, height, channels, f);
}

static int heads(int32_t width, int32_t height, int32_t channels, int32_t actions, const void *features_dev,
                 int32_t batch, const int32_t *count_dev, const void *head_w_dev, const float *head_b_dev,
                 float *probs_dev, float *values_dev, int32_t flags, hipStream_t s) {
  if (flags & ~SPMCTS_TOWER_F16) return -3;
  if (batch <= 0) return batch < 0 ? -3 : 0;
  return with_tiles(flags, width, height, channels, [&](auto t) {
    using T = decltype(t);
    using E = typename T::F::E;
    constexpr int FF = T::F::C / 4, CELLS = T::F::CELLS, A = T::A;
    if (actions != A) return -2;
    // as the product: C = 256 (FF = 64) runs its value tiles in two passes of 2
    hipLaunchKernelGGL((k_heads_co<FF, CELLS, A, E, 5, FF == 64 ? 2 : HeadsCfg<FF, CELLS, A>::VTW>), dim3((batch + 31) / 32),
                       dim3(256), 0, s, (const uint16_t *)features_dev, batch, count_dev, (const bf16x8 *)head_w_dev,
                       head_b_dev, probs_dev, values_dev);
    return hipGetLastError() == hipSuccess ? 0 : -11;
  });
}

}  // namespace tower

using namespace tower;

extern "C" int spmcts_tower_forward_dev(int32_t width, int32_t height, int32_t channels, int32_t n_blocks,
                                        const void *planes_dev, const int32_t *count_dev, int32_t max_batch,
                                        const void *weights_dev, const float *bias_dev, void *features_dev,
                                        int32_t flags, spmcts_stream stream) {
  if (n_blocks < 0 || max_batch < 0 || !count_dev || (flags & ~(SPMCTS_TOWER_PACK | SPMCTS_TOWER_F16))) return -3;
  if (max_batch == 0) return 0;
  return with_tiles(flags, width, height, channels, [&](auto t) {
    using T = decltype(t);
    using F = typename T::F;
    using M = typename T::M;
    using H = typename T::H;
    constexpr int LDS = F::LDS > M::LDS ? (F::LDS > H::LDS ? F::LDS : H::LDS) : (M::LDS > H::LDS ? M::LDS : H::LDS);
    const int cus = flags & SPMCTS_TOWER_PACK ? 1 : num_cus();
    const int grid = (max_batch + F::BOARDS - 1) / F::BOARDS + cus;
    return launch<k_tower_dyn<F, M, H>, F, LDS>(grid, (hipStream_t)stream, (const __bf16 *)planes_dev, count_dev, max_batch,
                                                cus, n_blocks, (const bf16x8 *)weights_dev, bias_dev,
                                                (uint16_t *)features_dev);
  });
}

extern "C" int spmcts_tower_forward(int32_t width, int32_t height, int32_t channels, int32_t n_blocks,
                                    const void *planes_dev, int32_t batch, const void *weights_dev,
                                    const float *bias_dev, void *features_dev, int32_t flags, spmcts_stream stream) {
  if (n_blocks < 0 || batch < 0 || (flags & ~SPMCTS_TOWER_F16)) return -3;
  return with_tiles(flags, width, height, channels, [&](auto t) {
    using F = typename decltype(t)::F;
    const int grid = (batch + F::BOARDS - 1) / F::BOARDS;
    if (grid <= 0) return 0;
    return launch<k_tower<F>, F, F::LDS>(grid, (hipStream_t)stream, (const __bf16 *)planes_dev, batch, n_blocks,
                                         (const bf16x8 *)weights_dev, bias_dev, (uint16_t *)features_dev);
  });
}

extern "C" int spmcts_tower_heads(int32_t width, int32_t height, int32_t channels, int32_t actions,
                                  const void *features_dev, int32_t batch, const void *head_w_dev,
                                  const float *head_b_dev, float *probs_dev, float *values_dev, int32_t flags,
                                  spmcts_stream stream) {
  return heads(width, height, channels, actions, features_dev, batch, nullptr, head_w_dev, head_b_dev, probs_dev,
               values_dev, flags, (hipStream_t)stream);
}

extern "C" int spmcts_tower_heads_dev(int32_t width, int32_t height, int32_t channels, int32_t actions,
                                      const void *features_dev, const int32_t *count_dev, int32_t max_batch,
                                      const void *head_w_dev, const float *head_b_dev, float *probs_dev,
                                      float *values_dev, int32_t flags, spmcts_stream stream) {
  return heads(width, height, channels, actions, features_dev, max_batch, count_dev, head_w_dev, head_b_dev, probs_dev,
               values_dev, flags, (hipStream_t)stream);
}

extern "C" int spmcts_tower_supported(int32_t width, int32_t height, int32_t channels) {
  return with_tiles(0, width, height, channels, [](auto) { return 1; }) == 1;
}

extern "C" int spmcts_tower_weight_layout(int32_t width, int32_t height, int32_t channels) {
  return with_tiles(0, width, height, channels, [](auto) { return (int)SPMCTS_WLAYOUT_32X32; });
}
