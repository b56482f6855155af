// AIRs as data: a caller-defined AIR arrives as a constraint program (the BFA1 format of
// include/bfz.h: p3's SymbolicExpression [p3-recalled] written flat) and is proven, row-checked
// and verified by the code that serves the built-in chips -- what the reference gets from
// utils::uni_stark_prove / uni_stark_verify being generic over A: Air
// (crates/core/machine/src/utils/prove.rs:97-159).
//
//   air_compile   validation (every failure names the word offset), the shape (K, degree by
//                 DegOps' rules, log quotient degree by uni_air_shape's loop) and the linear
//                 instruction list the interpreters run: unreachable nodes dropped, a leaf loaded
//                 at its first use, slots allocated by linear scan over last uses, one EMIT per
//                 constraint in emission order.
//   air_run       the interpreter over that list on the host, templated on BaseOps / ExtOps as
//                 air.h is: the base-field row check and the EF evaluation at zeta.
//   air_export    a built-in chip's AIR recorded from Air<RecOps, RecAcc>::eval_air<CHIP>.
// The device interpreter and its two kernels are in air_program.hip.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/bfz.h"
#include "air.h"
#include "gpu.h"

namespace bfz {

// Node ops of BFA1; the compiled list uses the same codes plus AIR_EMIT.
enum : uint32_t {
  AIR_CONST = 0, AIR_LOCAL, AIR_NEXT, AIR_FIRST, AIR_LAST, AIR_TRANS, AIR_ADD, AIR_SUB, AIR_MUL,
  AIR_NEG, AIR_EMIT
};
constexpr uint32_t AIR_MAGIC = 0x31414642;  // "BFA1"

// One instruction word: op | dst << 8 | a << 16 | b << 24.  dst, a, b are slots, except that a is
// the column of LOCAL / NEXT; CONST is followed by its Montgomery word; EMIT reads slot a.
constexpr uint32_t air_ins(uint32_t op, uint32_t dst, uint32_t a, uint32_t b) {
  return op | dst << 8 | a << 16 | b << 24;
}

struct AirProgram {
  int width = 0, num_nodes = 0, num_constraints = 0, degree = 0, log_quotient_degree = 0;
  int live_values = 0;         // slots the list uses, at most BFZ_AIR_MAX_LIVE
  std::vector<uint32_t> code;  // the compiled list
  int instructions = 0;        // of the list (a CONST counts once)
};

// Throws std::runtime_error: a malformed program, a degree above 3 (uni_dims_or_throw's message),
// more than BFZ_AIR_MAX_LIVE live values.  Reads nothing outside [prog, prog + len).
AirProgram air_compile(const uint8_t* prog, size_t len);

// The BFA1 bytes of a built-in chip's AIR; refuses the chips uni_air_shape_or_throw refuses.
std::vector<uint8_t> air_export(int chip);

// The interpreter.  L / N: the local and next row (width values).  sink.emit(value) is called once
// per constraint in emission order; returning false ends the run.
template <class Ops, class Sink>
void air_run(const AirProgram& p, const typename Ops::T* L, const typename Ops::T* N,
             const typename Ops::T& first, const typename Ops::T& last,
             const typename Ops::T& trans, Sink& sink) {
  typename Ops::T s[BFZ_AIR_MAX_LIVE];
  const uint32_t* code = p.code.data();
  const size_t n = p.code.size();
  for (size_t pc = 0; pc < n;) {
    const uint32_t w = code[pc++];
    const uint32_t d = (w >> 8) & 0xff, a = (w >> 16) & 0xff, b = w >> 24;
    switch (w & 0xff) {
      case AIR_CONST: s[d] = Ops::cst(code[pc++]); break;
      case AIR_LOCAL: s[d] = L[a]; break;
      case AIR_NEXT: s[d] = N[a]; break;
      case AIR_FIRST: s[d] = first; break;
      case AIR_LAST: s[d] = last; break;
      case AIR_TRANS: s[d] = trans; break;
      case AIR_ADD: s[d] = Ops::add(s[a], s[b]); break;
      case AIR_SUB: s[d] = Ops::sub(s[a], s[b]); break;
      case AIR_MUL: s[d] = Ops::mul(s[a], s[b]); break;
      case AIR_NEG: s[d] = Ops::neg(s[a]); break;
      default:  // AIR_EMIT (air_compile writes nothing else)
        if (!sink.emit(s[a])) return;
    }
  }
}

// One row of the trace domain (debug.rs:43-97 semantics, as check_row_air): the first failing
// constraint index, or -1.  Words must be canonical (< p).
int air_first_fail(const AirProgram& p, const uint32_t* L, const uint32_t* N, bool is_first,
                   bool is_last);
// All K constraint values over EF rows and selectors (the verifier at zeta, bfz_air_eval).
void air_eval_ef(const AirProgram& p, const EF* L, const EF* N, const EF& first, const EF& last,
                 const EF& trans, EF* out);

// ---- device side (air_program.hip).  code_dev: the compiled list in device memory.
struct QuotParams;
struct QuotOut;
void launch_quotient_prog(int lqd, const uint32_t* code_dev, int ncode, const uint32_t* mainc,
                          int logN, const QuotParams* qp_dev, const uint32_t* twf,
                          const uint32_t* sel_inv, const QuotOut& qo, hipStream_t st);
// The row check of a column-major bit-reversed trace of h rows: res = {min(row * K + index) or ~0,
// failing rows}; per_row_dev (optional) by storage position.
void launch_check_prog(const uint32_t* code_dev, int ncode, const uint32_t* mainc, size_t h, int K,
                       unsigned long long* res_dev, int32_t* per_row_dev, hipStream_t st);

}  // namespace bfz
