// The device interpreter of a compiled constraint program (air_program.h) and the row check's
// sink, shared by the kernels of air_program.hip, chip_program.hip and machine_program.hip.
// air_program.hip's header argues the design: a wave-uniform list read through the constant
// address space, the slot file in LDS as slots[slot][threadIdx.x].
#pragma once
#include "air_program.h"

namespace bfz {
namespace {
using ConstWords = const __attribute__((address_space(4))) uint32_t*;

// mainc: the column-major matrix (stride words per column); vt / vn: the byte offsets of the
// thread's local and next position in a column.
template <class Sink>
__device__ __forceinline__ void run_program(ConstWords code, int ncode,
                                            uint32_t (*slots)[256], const uint32_t* mainc,
                                            size_t stride, uint32_t vt, uint32_t vn,
                                            uint32_t first, uint32_t last, uint32_t trans,
                                            Sink& sink) {
  using namespace kb;
  const uint32_t tid = threadIdx.x;
  for (int pc = 0; pc < ncode;) {
    const uint32_t w = code[pc++];
    const uint32_t d = (w >> 8) & 0xff, a = (w >> 16) & 0xff, b = w >> 24;
    switch (w & 0xff) {
      case AIR_CONST: slots[d][tid] = code[pc++]; break;
      case AIR_LOCAL: slots[d][tid] = ld_b(rsrc_of(mainc + (size_t)a * stride), vt, 0); break;
      case AIR_NEXT: slots[d][tid] = ld_b(rsrc_of(mainc + (size_t)a * stride), vn, 0); break;
      case AIR_FIRST: slots[d][tid] = first; break;
      case AIR_LAST: slots[d][tid] = last; break;
      case AIR_TRANS: slots[d][tid] = trans; break;
      case AIR_ADD: slots[d][tid] = madd(slots[a][tid], slots[b][tid]); break;
      case AIR_SUB: slots[d][tid] = msub(slots[a][tid], slots[b][tid]); break;
      case AIR_MUL: slots[d][tid] = mmul(slots[a][tid], slots[b][tid]); break;
      case AIR_NEG: slots[d][tid] = mneg(slots[a][tid]); break;
      default: sink.emit(slots[a][tid]);  // AIR_EMIT
    }
  }
}

// The row check's sink: counts the emissions, keeps the first that is not zero and ignores the
// rest (FirstFailAcc; the loop stays wave-uniform).  An EF emission is not zero when any of its
// components is not.
struct FirstFailSink {
  int n = 0, first = -1;
  __device__ __forceinline__ void emit(uint32_t c) {
    if (c != 0 && first < 0) first = n;
    n++;
  }
  __device__ __forceinline__ void emit_ext(const kb::EF& c) { emit(c.c[0] | c.c[1] | c.c[2] | c.c[3]); }
};

// 1 / d for the block's 256 values d (none zero) with one field inversion: an inclusive prefix
// and an inclusive suffix product inside each wave by shuffles (6 steps each), the four wave
// totals through LDS, one minv of the block's product by thread 0, and
//   1 / d_i = (product before i) (product after i) / (product of all).
// Every thread of the block calls it (two barriers).
__device__ __forceinline__ uint32_t block_inverse(uint32_t d, uint32_t* s_wave, uint32_t* s_tinv) {
  using namespace kb;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t pre = d, suf = d;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t up = __shfl_up(pre, off, 64), dn = __shfl_down(suf, off, 64);
    if (lane >= (uint32_t)off) pre = mmul(pre, up);
    if (lane + off < 64) suf = mmul(suf, dn);
  }
  if (lane == 63) s_wave[wave] = pre;  // the wave's product
  __syncthreads();
  if (threadIdx.x == 0)
    *s_tinv = minv(mmul(mmul(s_wave[0], s_wave[1]), mmul(s_wave[2], s_wave[3])));
  // the product before / after the thread's own value: inside the wave, then the other waves
  uint32_t before = __shfl_up(pre, 1, 64), after = __shfl_down(suf, 1, 64);
  if (lane == 0) before = ONE;
  if (lane == 63) after = ONE;
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) {
    const uint32_t wk = s_wave[k];
    if (k < wave) before = mmul(before, wk);
    if (k > wave) after = mmul(after, wk);
  }
  __syncthreads();
  return mmul(mmul(before, after), *s_tinv);
}
}  // namespace
}  // namespace bfz
