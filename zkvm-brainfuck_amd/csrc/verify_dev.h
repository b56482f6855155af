// Device helpers shared by the query-phase kernels of verify.hip and verify_machine.hip: the
// failure key and the lane-mode Merkle steps (one Poseidon2 state per 16-lane DPP row; a row's
// lanes must branch together around every call).
#pragma once
#include "kb.h"
#include "poseidon2.h"

namespace bfz {
namespace vdev {

using namespace kb;

__device__ __forceinline__ EF ld_ef(const uint32_t* p) { return EF{{p[0], p[1], p[2], p[3]}}; }
__device__ __forceinline__ void report(uint32_t* keys, uint32_t proof, uint32_t q, uint32_t stage) {
  atomicMin(&keys[proof], q * 64u + stage);
}

// PaddingFreeSponge (overwrite mode, rate 8) of `w` consecutive words in lane mode; the digest is
// lanes 0..7 of the result.
__device__ __forceinline__ uint32_t sponge_lane(const uint32_t* __restrict__ row, uint32_t w, int lane,
                                                const LaneConsts& kc) {
  uint32_t h = 0;
  for (uint32_t at = 0; at < w; at += 8) {
    const uint32_t m = w - at < 8 ? w - at : 8;
    if ((uint32_t)lane < m) h = row[at + lane];
    h = poseidon2_permute_lane(h, lane, kc);
  }
  return h;
}
// compress(l, r) with l in lanes 0..7 of `l` and r in lanes 0..7 of `r`
__device__ __forceinline__ uint32_t compress_lane(uint32_t l, uint32_t r, int lane, const LaneConsts& kc) {
  const uint32_t rs = dpp<DPP_ROR8>(r);  // lanes 8..15 <- r[0..7]
  return poseidon2_permute_lane(lane < 8 ? l : rs, lane, kc);
}
// One level of a path: the node joins its sibling on the side the index's low bit names.
__device__ __forceinline__ uint32_t path_step_lane(uint32_t node, const uint32_t* __restrict__ sib8,
                                                   bool right, int lane, const LaneConsts& kc) {
  const uint32_t sib = sib8[lane & 7];
  const uint32_t ns = dpp<DPP_ROR8>(node);
  const uint32_t lo = right ? sib : node, hi = right ? ns : sib;
  return poseidon2_permute_lane(lane < 8 ? lo : hi, lane, kc);
}

}  // namespace vdev
}  // namespace bfz
