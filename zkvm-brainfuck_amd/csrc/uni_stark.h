// Per-chip uni-STARK proofs: bf_core_machine::utils::{uni_stark_prove, uni_stark_verify}
// (crates/core/machine/src/utils/prove.rs:97-159), i.e. p3_uni_stark::{prove, verify}
// [p3-recalled] of ONE chip's AIR over one trace with the machine prover's PCS and challenger.
// Under the uni-STARK builders a chip's send / receive are no-ops (air/builder.rs:232-239,
// 273-275): what is proven is Air::eval_air<CHIP> (air.h) and nothing else.  DESIGN.md §2
// (decisions U1-U6) and §4 (the BFU1 normal form, the kernel).
#pragma once
#include <cstdint>
#include <vector>

#include "air_program.h"
#include "prover.h"
#include "verifier.h"

namespace bfz {

// Decision U1: the transcript starts with observe(F(log degree)) (1, default) or with the trace
// commitment alone (0, p3 before the degree was bound); environment BFZ_UNI_OBSERVE_DEGREE.
bool uni_observe_degree_from_env();

struct UniOptions {
  int num_queries = 84;
  bool observe_openings = true;  // decision D1
  bool observe_degree = true;    // decision U1
};

// uni_air_shape (quotient.h) for a chip that has one; throws the refusal the C ABI reports for a
// bad index and for Program, Memory and Byte.  Any output pointer may be null.
void uni_air_shape_or_throw(int chip, int* num_constraints, int* degree, int* log_quotient_degree);

// What the prover, the row check and the verifier take from an AIR: its shape and name, and which
// code evaluates it -- a built-in chip (chip >= 0: the compiled templates of air.h) or a compiled
// constraint program (prog, chip = -1; the program outlives the call).
struct UniAir {
  int chip = -1;
  const AirProgram* prog = nullptr;
  int num_constraints = 0, degree = 0, log_quotient_degree = 0, width = 0;
  const char* name = "custom";
};
UniAir uni_air_of_chip(int chip);  // throws as uni_air_shape_or_throw
UniAir uni_air_of_program(const AirProgram& p);

// trace: row-major Montgomery height x width on the host.  ch is advanced to the state after
// the whole opening (as open_main's `after`).  Returns the BFU1 bytes.  The API lock is held.
std::vector<uint8_t> uni_prove(int chip, const uint32_t* trace, size_t height, size_t width,
                               Challenger& ch, const UniOptions& opt, StageTimes* times);
// The same for any AIR; a program's proof carries the chip word BFZ_AIR_CHIP.
std::vector<uint8_t> uni_prove(const UniAir& air, const uint32_t* trace, size_t height, size_t width,
                               Challenger& ch, const UniOptions& opt, StageTimes* times);

// The same from device evaluations: evals = n x main_w of the chip, column-major and bit-reversed
// (gpu.h LAYOUT, what generate_traces_device leaves in DeviceTraces::evals), read in place.  Same
// bytes and same ending challenger as uni_prove on the same trace.
std::vector<uint8_t> uni_prove_evals(int chip, const uint32_t* evals, size_t n, Challenger& ch,
                                     const UniOptions& opt, StageTimes* times);

// The input checks every uni-STARK call shares, with uni_prove's messages: the chip
// (uni_air_shape_or_throw), a constraint degree above 3, the width, the height.
void uni_dims_or_throw(int chip, size_t height, size_t width);
void uni_dims_or_throw(const UniAir& air, size_t height, size_t width);
[[noreturn]] void uni_noncanonical_throw(const char* name);  // a trace word >= p
// uni_prove's upload: the row-major host trace (n x width) to the device, refused when a word is
// >= p (syncs st; name is the AIR's, for the message), transposed into the library layout.
DBuf<uint32_t> uni_upload_trace(size_t width, const char* name, const uint32_t* trace, size_t n,
                                hipStream_t st);

// Host verifier (verifier.cpp).  ch is advanced as far as the check got; on acceptance it is the
// prover's final state.
VerifyOutcome uni_verify(int chip, Challenger& ch, const uint8_t* proof, size_t len,
                         const UniOptions& opt);
// The same against a constraint program: the proof's chip word is a label and is not interpreted.
VerifyOutcome uni_verify(const UniAir& air, Challenger& ch, const uint8_t* proof, size_t len,
                         const UniOptions& opt);

// n BFU1 proofs, proof i of chip chips[i] against challenger chs[i] (advanced), with
// verify_batch's contract (verifier.h): run_queries == nullptr is uni_verify proof by proof;
// otherwise the query loops are packed into one QueryBatch and handed to run_queries, and the
// outcomes and ending challengers are the same.
std::vector<VerifyOutcome> uni_verify_batch(const int* chips, Challenger* chs,
                                            const uint8_t* const* proofs, const size_t* lens,
                                            size_t n, const UniOptions& opt, QueryRunner run_queries);

}  // namespace bfz
