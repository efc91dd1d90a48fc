// tower.hip — host side of the fused residual-tower inference for the leaf evaluator (gfx950): the residual
// scratch table, the one launch helper, the product tile sets, the (dtype, shape) switch and the
// spmcts_tower_* / spmcts_head_epilogue C ABI (include/spmcts.h).  The device code is in the headers:
//   tower_common.h    Ty, Cfg and its named plans, Nbr, WBuf, XLive, head_layer: what the families share
//   tower_b32.h / tower_m16.h / tower_wide16.h    the three trunk families (3x3 boards / 7x6 C = 128 / 7x6 C = 256)
//   tower_kernels.h   tile<K> (family dispatch), k_tower, k_tower_dyn;  tower_heads.h   k_heads_co, k_head_epilogue
//   tower_ab.h        A/B library only: environment switches, the 3-board C = 256 tile set, k_heads
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "spmcts.h"
#include "tower_heads.h"
#include "tower_kernels.h"

namespace tower {

// Residual scratch of the one-buffer trunk (tower_wide16.h): one region per workgroup of a launch, one
// buffer per stream (launches on different streams run concurrently), grown on demand.
static uint4 *wide_scratch(hipStream_t s, size_t bytes) {
  struct Ent {
    hipStream_t s;
    void *p;
    size_t n;
  };
  static std::vector<Ent> tab;
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  for (auto &e : tab)
    if (e.s == s) {
      if (e.n >= bytes) return (uint4 *)e.p;
      if (hipStreamSynchronize(s) != hipSuccess || hipFree(e.p) != hipSuccess) return nullptr;
      e.p = nullptr;
      e.n = 0;
      if (hipMalloc(&e.p, bytes) != hipSuccess) return nullptr;
      e.n = bytes;
      return (uint4 *)e.p;
    }
  void *p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
  tab.push_back({s, p, bytes});
  return (uint4 *)p;
}

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

// One trunk launch (Kern = k_tower<K> or k_tower_dyn<KF, KM, KH>; args = its parameters but the last, the
// scratch): the residual scratch of `grid` workgroups of K (one-buffer tiles only; -12), the kernel's
// dynamic-LDS limit raised once (-10), the launch (-11).
template <auto Kern, class K, int LDS, class... Args>
static int launch(int grid, hipStream_t s, Args... args) {
  uint4 *scr = nullptr;
  if constexpr (K::ONEBUF) {
    if (!(scr = wide_scratch(s, (size_t)grid * wide16::Scr<K>::PER_WG))) return -12;
  }
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute((const void *)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, LDS) != hipSuccess)
      return -10;
    attr_set = true;
  }
  hipLaunchKernelGGL(Kern, dim3(grid), dim3(K::THREADS), LDS, s, args..., scr);
  return hipGetLastError() == hipSuccess ? 0 : -11;
}

// The product tile sets, each written out once: F / M / H = the full / middle / half tiles of the device-count
// path (k_tower_dyn: whole rounds of F, the tail in the smallest that covers it); the host-count path (k_tower)
// runs F alone.  A = the game's action count on that board (the policy head's width).
template <int A_, class F_, class M_ = F_, class H_ = F_>
struct TileSet {
  static constexpr int A = A_;
  using F = F_;
  using M = M_;
  using H = H_;
};
// 7x6, C = 128: 16x16x32 edge tiles for every board, tails included (tower_m16.h)
template <class E>
using Tiles7x6c128 = TileSet<7, Edge16<128, false, E>>;
// 7x6, C = 256: every tile a 6-board one-buffer 16x16x32 tile (tower_wide16.h; a batch tail takes one partly
// empty tile), so every board goes through the same arithmetic
template <class E>
using Tiles7x6c256 = TileSet<7, Edge16<256, true, E>>;
// 3x3: board-major 32x32x16 tiles (tower_b32.h); C = 128 ends a batch on a 192- or 128-row tile
template <class E>
using Tiles3x3c128 = TileSet<9, BoardMajor32<128, 256, 3, 3, E>, BoardMajor32<128, 192, 3, 3, E>, BoardMajor32<128, 128, 3, 3, E>>;
template <class E>
using Tiles3x3c256 = TileSet<9, BoardMajor32<256, 128, 3, 3, E>>;

#ifdef SPMCTS_AB
#include "tower_ab.h"
#else
// The product library has exactly one kernel per (shape, dtype) and reads no switch; a switch of the
// A/B library set in the environment is refused (SPMCTS_ERR_AB_SWITCH, read once) rather than silently ignored.
static int ab_switch_guard() {
  static const int rc = [] {
    for (const char *n : {"SPMCTS_TOWER_C256", "SPMCTS_HEADS", "SPMCTS_HEADS_C256"})
      if (getenv(n)) return SPMCTS_ERR_AB_SWITCH;
    return 0;
  }();
  return rc;
}
template <class E, class Fn>
static int tiles_7x6c256(Fn &&f) {
  return f(Tiles7x6c256<E>{});
}
template <int FF, int CELLS, int A, class E>
static bool launch_heads_lds(const void *, int, const int32_t *, const void *, const float *, float *, float *, hipStream_t) {
  return false;
}
#endif

// The one (dtype, width, height, channels) switch: f(the shape's tile set for the element type), or -2.
template <class E, class Fn>
static int with_tiles_of(int32_t width, int32_t height, int32_t channels, Fn &&f) {
  if (channels != 128 && channels != 256) return -2;
  if (width == 7 && height == 6) return channels == 128 ? f(Tiles7x6c128<E>{}) : tiles_7x6c256<E>(f);
  if (width == 3 && height == 3) return channels == 128 ? f(Tiles3x3c128<E>{}) : f(Tiles3x3c256<E>{});
  return -2;
}
template <class Fn>
static int with_tiles(int32_t flags, int32_t width, int32_t height, int32_t channels, Fn &&f) {
  return flags & SPMCTS_TOWER_F16 ? with_tiles_of<_Float16>(width, height, channels, f)
                                  : with_tiles_of<__bf16>(width, height, channels, f);
}

}  // namespace tower

using namespace tower;

// the device-count path: the batch size is read on the device; pack (SPMCTS_TOWER_PACK): the launch runs beside
// launches on other streams, so tiles are assigned as if the chip had one CU (all boards in full tiles, the
// last < BOARDS in one smaller tile); the other streams' workgroups fill the CUs a partial round would leave idle
extern "C" int spmcts_tower_forward_dev(int32_t width, int32_t height, int32_t channels, int32_t n_blocks,
                                        const void *planes_dev, const int32_t *count_dev, int32_t max_batch,
                                        const void *weights_dev, const float *bias_dev, void *features_dev,
                                        int32_t flags, spmcts_stream stream) {
  if (n_blocks < 0 || max_batch < 0 || !count_dev || (flags & ~(SPMCTS_TOWER_PACK | SPMCTS_TOWER_F16))) return -3;
  if (const int g = ab_switch_guard()) return g;
  if (max_batch == 0) return 0;
  return with_tiles(flags, width, height, channels, [&](auto t) {
    using T = decltype(t);
    using F = typename T::F;
    using M = typename T::M;
    using H = typename T::H;
    // (scratch is sized for F: the tail kinds M / H are two-buffer tiles, or F itself)
    constexpr int LDS = F::LDS > M::LDS ? (F::LDS > H::LDS ? F::LDS : H::LDS) : (M::LDS > H::LDS ? M::LDS : H::LDS);
    const int cus = flags & SPMCTS_TOWER_PACK ? 1 : num_cus();
    const int grid = (max_batch + F::BOARDS - 1) / F::BOARDS + cus;
    return launch<k_tower_dyn<F, M, H>, F, LDS>(grid, (hipStream_t)stream, (const __bf16 *)planes_dev, count_dev, max_batch,
                                                cus, n_blocks, (const bf16x8 *)weights_dev, bias_dev,
                                                (uint16_t *)features_dev);
  });
}

// the host-count path (a batch size known on the host): full tiles only
extern "C" int spmcts_tower_forward(int32_t width, int32_t height, int32_t channels, int32_t n_blocks,
                                    const void *planes_dev, int32_t batch, const void *weights_dev,
                                    const float *bias_dev, void *features_dev, int32_t flags, spmcts_stream stream) {
  if (n_blocks < 0 || batch < 0 || (flags & ~SPMCTS_TOWER_F16)) return -3;
  if (const int g = ab_switch_guard()) return g;
  return with_tiles(flags, width, height, channels, [&](auto t) {
    using F = typename decltype(t)::F;
    const int grid = (batch + F::BOARDS - 1) / F::BOARDS;
    if (grid <= 0) return 0;
    return launch<k_tower<F>, F, F::LDS>(grid, (hipStream_t)stream, (const __bf16 *)planes_dev, batch, n_blocks,
                                         (const bf16x8 *)weights_dev, bias_dev, (uint16_t *)features_dev);
  });
}

// the linear heads of both entry points (count_dev: the batch size on the device, or null)
static int heads(int32_t width, int32_t height, int32_t channels, int32_t actions, const void *features_dev,
                 int32_t batch, const int32_t *count_dev, const void *head_w_dev, const float *head_b_dev,
                 float *probs_dev, float *values_dev, int32_t flags, hipStream_t s) {
  if (flags & ~SPMCTS_TOWER_F16) return -3;
  if (batch <= 0) return batch < 0 ? -3 : 0;
  if (const int g = ab_switch_guard()) return g;
  // the co-resident k_heads_co (C = 256, FF = 64: two value passes of 2 tiles in 96 registers, beside the
  // C = 256 trunk); the A/B library's SPMCTS_HEADS=lds / SPMCTS_HEADS_C256=lds select the LDS-staged k_heads
  return with_tiles(flags, width, height, channels, [&](auto t) {
    using T = decltype(t);
    using E = typename T::F::E;
    constexpr int FF = T::F::C / 4, CELLS = T::F::CELLS, A = T::A;
    if (actions != A) return -2;
    if (!launch_heads_lds<FF, CELLS, A, E>(features_dev, batch, count_dev, head_w_dev, head_b_dev, probs_dev, values_dev, s))
      hipLaunchKernelGGL((k_heads_co<FF, CELLS, A, E, 5, FF == 64 ? 2 : HeadsCfg<FF, CELLS, A>::VTW>), dim3((batch + 31) / 32),
                         dim3(256), 0, s, (const uint16_t *)features_dev, batch, count_dev, (const bf16x8 *)head_w_dev,
                         head_b_dev, probs_dev, values_dev);
    return hipGetLastError() == hipSuccess ? 0 : -11;
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

extern "C" int spmcts_head_epilogue(int32_t hidden, int32_t actions, const void *z_dev, int32_t ldz, int32_t batch,
                                    const float *head_b_dev, float *probs_dev, float *values_dev,
                                    spmcts_stream stream) {
  if (batch <= 0) return batch < 0 ? -3 : 0;
  void (*kern)(const __bf16 *, int, int, const float *, float *, float *) = nullptr;
  if (hidden == 256 && actions == 7) kern = k_head_epilogue<256, 7>;
  if (hidden == 512 && actions == 7) kern = k_head_epilogue<512, 7>;
  if (hidden == 256 && actions == 9) kern = k_head_epilogue<256, 9>;
  if (hidden == 512 && actions == 9) kern = k_head_epilogue<512, 9>;
  if (!kern) return -2;
  hipLaunchKernelGGL(kern, dim3((batch + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const __bf16 *)z_dev, ldz, batch,
                     head_b_dev, probs_dev, values_dev);
  return hipGetLastError() == hipSuccess ? 0 : -11;
}

extern "C" int spmcts_tower_supported(int32_t width, int32_t height, int32_t channels) {
  return with_tiles(0, width, height, channels, [](auto) { return 1; }) == 1;
}

extern "C" int spmcts_tower_weight_layout(int32_t width, int32_t height, int32_t channels) {
  return with_tiles(0, width, height, channels, [](auto t) {
    return decltype(t)::F::M16 ? SPMCTS_WLAYOUT_M16 : SPMCTS_WLAYOUT_32X32;
  });
}
