// The permutation constraints of a compiled interaction list on the device, shared by the kernels
// that fold them after the AIR's interpreter: k_quotient_chip_prog / k_check_chip_prog
// (chip_program.hip, whose header argues the design) and k_quotient_machine (machine_program.hip).
#pragma once
#include "chip_program.h"

#include "air_program_dev.h"
#include "lookup_program_dev.h"

namespace bfz {
namespace {
static_assert(offsetof(QuotParams, perm_alpha) == 0 && offsetof(QuotParams, beta_pows) == 16 &&
                  offsetof(PermChallenges, alpha) == 0 && offsetof(PermChallenges, beta_pows) == 16,
              "QuotParams begins with PermChallenges' words");
constexpr int QP_CUMSUM_WORD = offsetof(QuotParams, cumsum) / 4;

// EF column `col` of the permutation matrix (4 base columns of `stride` words) at a byte offset.
__device__ __forceinline__ kb::EF ld_ef(const uint32_t* permc, size_t stride, int col,
                                        uint32_t voff) {
  kb::EF v;
#pragma unroll
  for (int e = 0; e < 4; e++) v.c[e] = kb::ld_b(kb::rsrc_of(permc + (size_t)(4 * col + e) * stride), voff, 0);
  return v;
}

// The permutation constraints of c.list at the thread's position (c.vt; vn = the next row's byte
// offset): batches + 3 calls of sink.emit_ext.  cumsum: 4 words, constant address space.
template <class Sink>
__device__ __forceinline__ void perm_constraints(const RowCtx& c, const uint32_t* permc, uint32_t vn,
                                                 ConstWords cumsum, uint32_t first, uint32_t last,
                                                 uint32_t trans, Sink& sink) {
  using namespace kb;
  const int ni = (int)c.list[0], nb = (ni + 1) >> 1;
  EF sum_l = ef_zero(), sum_n = ef_zero();
  int at = LKP_HEAD;
  for (int b = 0; b < nb; b++) {
    EF d0;
    uint32_t m0;
    interaction(c, at, d0, m0);
    const EF pl = ld_ef(permc, c.n, b, c.vt);
    sum_l = ef_add(sum_l, pl);
    sum_n = ef_add(sum_n, ld_ef(permc, c.n, b, vn));
    if (2 * b + 1 < ni) {  // (uniform)
      EF d1;
      uint32_t m1;
      interaction(c, at, d1, m1);
      const EF num = ef_add(ef_mul_base(d1, m0), ef_mul_base(d0, m1));
      sink.emit_ext(ef_sub(ef_mul(ef_mul(d0, d1), pl), num));
    } else {
      sink.emit_ext(ef_sub(ef_mul(d0, pl), ef_base(m0)));
    }
  }
  const EF phi_l = ld_ef(permc, c.n, nb, c.vt), phi_n = ld_ef(permc, c.n, nb, vn);
  const EF cs{{cumsum[0], cumsum[1], cumsum[2], cumsum[3]}};
  sink.emit_ext(ef_mul_base(ef_sub(phi_l, sum_l), first));
  sink.emit_ext(ef_mul_base(ef_sub(ef_sub(phi_n, phi_l), sum_n), trans));
  sink.emit_ext(ef_mul_base(ef_sub(phi_l, cs), last));
}
}  // namespace
}  // namespace bfz
