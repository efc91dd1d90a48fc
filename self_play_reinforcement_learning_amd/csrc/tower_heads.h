// tower_heads.h — the linear heads after the trunk's 1x1 head convs: HeadsCfg, k_heads_co, k_head_epilogue.
// Included by tower.hip and tower_ab.h (k_heads, the LDS-staged form k_heads_co is checked against).  Uses Ty,
// bf16x8 and f32x16 from tower_common.h.
//
// Linear heads (modules.py:96-105 after the 1x1 convs), fused:
//   policy = softmax(pf @ Wp^T + bp)          pf = features[:, :, :ff]  (cell-major, K = cells*ff)
//   value  = tanh(relu(vf @ Wv^T + bv) @ wo + bo)                     vf = features[:, :, ff:]
// on v_mfma_f32_32x32x16 (M = 32 board rows, N = 32 weight rows).  Weight fragments are
// pre-swizzled on the host (one contiguous KiB per (32-row tile, 16-k step): lane (r, h) holds
// W[tile*32 + r][16 s + 8 h .. + 8]) and streamed through a register ring.  Wave w owns
// value tiles [w*VTW, (w+1)*VTW) over all of K and the policy tile over a quarter of K; partial
// sums are combined in a fixed order (deterministic, batch-independent).
// Weight blob: tile 0 = Wp padded to 32 rows, tiles 1..VT = Wv; float blob: bp[32], bv[8ff], wo[8ff], bo.
#pragma once
#include "tower_common.h"

namespace tower {

template <int FF, int CELLS, int A>
struct HeadsCfg {
  static constexpr int K = CELLS * FF, KS = K / 16, HID = 8 * FF, VT = HID / 32, VTW = VT / 4;
  static constexpr int FROW = CELLS * 2 * FF * 2;  // feature bytes per board
  static constexpr int KQ = (KS + 3) / 4;          // policy k-steps per wave
  static_assert(VT % 4 == 0 && FF % 16 == 0 && FROW % 16 == 0, "head tile plan");
};

// The heads with room beside a trunk workgroup; k_heads is the LDS-staged form it replaced (tower_ab.h: the
// A/B library keeps it as this kernel's reference).  The trunk holds 152.5 KB of a CU's 160 KB LDS and
// 416 of each SIMD's 512 registers per lane, so k_heads (86 KB of staged features) could only run on
// a CU no trunk workgroup occupies: its 512 workgroups waited for the other lane's trunk workgroups
// to retire (0.8-1 ms per call in the bench against 11 us alone), and the lane's expand and next
// trunk launch waited behind it.  This form reads the features straight from global memory (L2:
// the trunk wrote them just before) as the MFMA A operand, fills all 32 MFMA rows with boards (32
// per workgroup, half the weight traffic of 16), keeps only the cross-wave sums in LDS (4.6 KB), and
// is held to 96 registers per lane, so one wave fits on each SIMD beside a trunk wave.  Same math
// in the same order as k_heads (per-wave k order, fixed-order cross-wave sums): bit-identical.
//
// C = 256 (FF = 64: 4 value tiles per wave, which spill at 96 registers in one pass) runs the value
// tiles in two passes of 2 over all of K (the features are read twice, from L2) within the same 96
// registers; the C = 256 trunk wave uses 400 of a SIMD's 512, so one heads wave fits beside it.
// part[] still sums the tiles in order 0..3: bit-identical.
template <int FF, int CELLS, int A, class E = __bf16, int WPE = 5, int VP = HeadsCfg<FF, CELLS, A>::VTW>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE))) void k_heads_co(
    const uint16_t *feats, int n, const int32_t *count, const bf16x8 *wf, const float *hb, float *probs, float *values) {
  using H = HeadsCfg<FF, CELLS, A>;
  static_assert(H::VTW % VP == 0, "value tiles per pass");
  constexpr int BOARDS = 32;
  if (count) n = min(*count, n);  // n = the caller's buffer rows
  const int b0 = blockIdx.x * BOARDS;
  if (b0 >= n) return;
  __shared__ float s_part[4][BOARDS];     // per-wave value partial sums
  constexpr int AP = (A + 7) / 8 * 8;
  __shared__ float s_pol[4][BOARDS][AP];  // per-wave policy partial logits
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int nb = min(BOARDS, n - b0);
  const float *bp = hb, *bv = hb + 32, *wo = hb + 32 + H::HID, *bo = hb + 32 + 2 * H::HID;
  // row r = board b0 + r (rows past the batch repeat its last board; their results are not stored)
  const char *frow = (const char *)feats + (size_t)(b0 + min(r, nb - 1)) * H::FROW;
  // value tiles first, then the policy quarter (each in k_heads' per-wave k order): only one set of
  // accumulators is live at a time, which keeps the wave inside 96 registers without spills
  const bf16x8 *wp = wf + lane;
  const int q0 = wave * H::KQ, q1 = min(H::KS, q0 + H::KQ);
  // the features of step s (value half at FF, policy half at 0), one step ahead
  auto feat = [&](int s, int half) {
    const int k0 = 16 * s + 8 * h;
    return *(const bf16x8 *)(frow + ((k0 / FF) * 2 * FF + half + k0 % FF) * 2);
  };
  float part[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) part[i] = 0.f;
#pragma unroll 1
  for (int v0 = 0; v0 < H::VTW; v0 += VP) {
    f32x16 acc[VP];
#pragma unroll
    for (int v = 0; v < VP; ++v) acc[v] = f32x16{};
    constexpr int D = 2;  // weight ring depth
    bf16x8 ring[D][VP];
    const bf16x8 *wv = wf + (size_t)(1 + wave * H::VTW + v0) * H::KS * 64 + lane;
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
      for (int v = 0; v < VP; ++v) ring[d][v] = wv[((size_t)v * H::KS + d) * 64];
    bf16x8 avn = feat(0, FF);
    for (int s0 = 0; s0 < H::KS; s0 += D) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const int s = s0 + d;
        if (s >= H::KS) break;
        const bf16x8 av = avn;
        if (s + 1 < H::KS) avn = feat(s + 1, FF);
        bf16x8 wcur[VP];
#pragma unroll
        for (int v = 0; v < VP; ++v) {
          wcur[v] = ring[d][v];
          if (s + D < H::KS) ring[d][v] = wv[((size_t)v * H::KS + s + D) * 64];
        }
#pragma unroll
        for (int v = 0; v < VP; ++v) acc[v] = Ty<E>::mfma(av, wcur[v], acc[v]);
      }
    }
    // value: relu(acc + bv[col]) * wo[col], summed over the hidden units (cols); as k_heads
#pragma unroll
    for (int v = 0; v < VP; ++v) {
      const int col = (wave * H::VTW + v0 + v) * 32 + r;
      const float bb = bv[col], ww = wo[col];
#pragma unroll
      for (int i = 0; i < 16; ++i) part[i] += fmaxf(acc[v][i] + bb, 0.f) * ww;
    }
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
  f32x16 pacc = {};
  if (q0 < q1) {
    bf16x8 pn = wp[(size_t)q0 * 64], apn = feat(q0, 0);
    for (int s = q0; s < q1; ++s) {
      const bf16x8 pw = pn, ap = apn;
      if (s + 1 < q1) {
        pn = wp[(size_t)(s + 1) * 64];
        apn = feat(s + 1, 0);
      }
      pacc = Ty<E>::mfma(ap, pw, pacc);
    }
  }
  if (r < A) {
#pragma unroll
    for (int i = 0; i < 16; ++i) s_pol[wave][(i & 3) + 8 * (i >> 2) + 4 * h][r] = pacc[i];
  }
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

// Head epilogue after one GEMM  Z = features[n][cells*2ff] @ Wc^T  (Wc = value rows [8ff]
// then policy rows [A], zero where a row meets the other head's channels):
//   value = tanh(sum_j relu(Z[j] + bv[j]) * wo[j] + bo), probs = softmax(Z[8ff + a] + bp[a]).
// One wave per board; the hidden-unit sum is a fixed-order lane reduction (deterministic).
template <int HID, int A>
__global__ __launch_bounds__(256) void k_head_epilogue(const __bf16 *Z, int ldz, int n, const float *hb,
                                                       float *probs, float *values) {
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (wave >= n) return;
  const __bf16 *z = Z + (size_t)wave * ldz;
  const float *bv = hb, *wo = hb + HID, *bo = hb + 2 * HID, *bp = hb + 2 * HID + 1;
  float acc = 0.f;
#pragma unroll
  for (int j = lane; j < HID; j += 64) acc += fmaxf((float)z[j] + bv[j], 0.f) * wo[j];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  float logit = lane < A ? (float)z[HID + lane] + bp[lane] : -INFINITY;
  float m = logit;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  const float e = lane < A ? __expf(logit - m) : 0.f;
  float sum = e;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
  if (lane < A) probs[(size_t)wave * A + lane] = e / sum;
  if (lane == 0) values[wave] = tanhf(acc + bo[0]);
}

}  // namespace tower
