// tower_wide.h — residual scratch and bias loads of the C = 256 trunk on 6-board edge tiles with ONE
// activation buffer.
//
// Included by tower.hip (namespace tower).  The trunk itself is tower_wide16.h; this file holds what it shares
// with the plan it came from (round 3's 32x32x16 one-buffer trunk, removed after the 16x16x32 form replaced
// it: DESIGN.md §4): the residual scratch's size (Scr), its buffer-resource loads and stores (ScrBuf; the
// offsets are tower_wide16.h's soff) and load_bias.
//
// Two ping-pong buffers of a 6-board tile at C = 256 would need 2 x 143.6 KB of LDS, so the two-buffer
// kernel can run C = 256 only on 3-board, board-major tiles (128 rows): no edge-tile skipping (every tap of
// every tile is issued) and each weight fragment serves 128 rows.  With one buffer the 6-board edge layout
// of the C = 128 kernel (tower_edge.h) runs at C = 256:
//   * a conv reads the buffer for all its k-steps (12 of the 72 (tile, tap) pairs of the edge tiles read
//     zero padding only and are skipped), the waves meet at a barrier, then each wave writes its own output
//     channels of all 256 rows in place, and a second barrier publishes them;
//   * the residual of a block's second conv (the block input, overwritten by the first conv's
//     outputs) goes through global memory: the stem and every second conv also store their outputs
//     (the next block input, the same bf16 / fp16 bits as in LDS) to a per-workgroup scratch region,
//     and the next second conv's epilogue reads them back, each lane its own 32-byte runs (the same
//     lane, tile and channel tile wrote them two layers earlier; coalesced 16-byte accesses).

namespace wide {

// residual scratch per workgroup: [wave][channel tile m][cell tile t][64 lanes] x 32 bytes
template <class K>
struct Scr {
  static constexpr size_t PER_WAVE = (size_t)K::MT * K::NT * 64 * 32;
  static constexpr size_t PER_WG = PER_WAVE * K::WAVES;
};
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Residual-scratch access through a buffer resource over this workgroup's region: the per-lane part of a
// load's address is one 32-bit voffset (lane * 32 + half * 16) and the (wave, channel tile, cell tile) part a
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
template <class K>
__device__ __forceinline__ void load_bias(float4 (&bv)[K::MT][4], const float *bias, int wave, int lane) {
#pragma unroll
  for (int m = 0; m < K::MT; ++m)
#pragma unroll
    for (int g = 0; g < 4; ++g) bv[m][g] = *(const float4 *)(bias + (wave * K::MT + m) * 32 + 8 * g + 4 * (lane >> 5));
}

}  // namespace wide
