// The device interpreter of a compiled constraint program (air_program.h) and the row check's
// sink, shared by the kernels of air_program.hip and chip_program.hip.  air_program.hip's header
// argues the design: a wave-uniform list read through the constant address space, the slot file
// in LDS as slots[slot][threadIdx.x].
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
}  // namespace
}  // namespace bfz
