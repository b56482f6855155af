// Device walkers of a compiled interaction list (lookup_program.h), shared by the kernels that
// read one: k_perm_rows_prog (lookup_program.hip) and the chip kernels (chip_program.hip).  The
// list and the LogUp challenges are read through the constant address space, so every read is a
// scalar load and every loop bound and branch over the list is wave-uniform; a term is one buffer
// load of its column at the thread's position (lookup_program.hip's header argues both).
#pragma once
#include "lookup_program.h"

namespace bfz {
namespace {
using ConstWords = const __attribute__((address_space(4))) uint32_t*;

struct RowCtx {
  ConstWords list;        // the compiled list
  ConstWords chw;         // PermChallenges as words: alpha at 0, beta^j at 4 + 4 j
  const uint32_t* mainc;  // column-major, n words per column
  const uint32_t* prepc;
  size_t n;
  uint32_t vt;  // the thread's byte offset in a column
};

// The VCOL at list[at] over the thread's row: constant + sum weight x column; at advances.
__device__ __forceinline__ uint32_t vcol(const RowCtx& c, int& at) {
  using namespace kb;
  const uint32_t cst = c.list[at];
  const int nt = (int)c.list[at + 1];
  at += 2;
  uint64_t acc = 0;  // 4 raw products < 4 p^2 < 2^64; folded (< 2^57) there is room for 4 more
  for (int i = 0; i < nt; i++, at += 2) {
    const uint32_t w = c.list[at], sc = c.list[at + 1];
    const uint32_t* col = ((sc >> 16) ? c.prepc : c.mainc) + (size_t)(sc & 0xffff) * c.n;
    acc += (uint64_t)w * ld_b(rsrc_of(col), c.vt, 0);
    if (i == 3) acc = fold32(acc);
  }
  return madd(cst, mreduce(acc));
}

// The interaction at list[at]: its denominator and signed multiplicity (a receive's negated).
__device__ __forceinline__ void interaction(const RowCtx& c, int& at, kb::EF& den, uint32_t& mult) {
  using namespace kb;
  const uint32_t head = c.list[at], kind = c.list[at + 1];
  at += 2;
  const int nv = (int)(head & 0xff);
  const uint32_t mu = vcol(c, at);
  mult = (head >> 8) & 1 ? mu : mneg(mu);
  LazyEF lz;
  lz.init();
  for (int v = 0; v < nv; v++) {
    const uint32_t x = vcol(c, at);
    const int bw = 8 + 4 * v;  // beta^(v+1)
    lz.add(EF{{c.chw[bw], c.chw[bw + 1], c.chw[bw + 2], c.chw[bw + 3]}}, x);
  }
  const EF alpha{{c.chw[0], c.chw[1], c.chw[2], c.chw[3]}};
  den = ef_add(lz.get(), ef_add_base(alpha, kind));
}

constexpr int LKP_T = 256;  // threads per block of the permutation-row kernels

// The batch at list[at]: numerator and denominator of m_0 / d_0 + m_1 / d_1, or of m_0 / d_0.
__device__ __forceinline__ void batch_frac(const RowCtx& c, int& at, bool pair, kb::EF& num,
                                           kb::EF& den) {
  using namespace kb;
  EF d0;
  uint32_t m0;
  interaction(c, at, d0, m0);
  if (pair) {
    EF d1;
    uint32_t m1;
    interaction(c, at, d1, m1);
    num = ef_add(ef_mul_base(d1, m0), ef_mul_base(d0, m1));
    den = ef_mul(d0, d1);
  } else {
    num = ef_base(m0);
    den = d0;
  }
}
}  // namespace
}  // namespace bfz
