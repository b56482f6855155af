// A machine of caller-defined chips as a value, and its prover and verifier: what
// StarkMachine::prove / verify (crates/stark/src/machine.rs:258-284, prover.rs:209-553,
// verifier.rs:27-216) do for the eight compiled chips through ProvingKey, MainData and open_main,
// done for up to 32 chip programs (chip_program.h).
//   machine_create   the chips compiled and named; with preprocessed traces they are committed on
//                    the device as setup commits them (one mixed-height MMCS, shift 1) -- without,
//                    from a given root and heights, the machine only verifies.
//   machine_observe  StarkVerifyingKey::observe_into (prover.rs:595-601).
//   machine_prove    machine_program.hip: MachineProver::commit and ::open with the host
//                    challenger; the two steps that interpret programs are one segmented launch
//                    each over every chip (k_perm_rows_machine, k_quotient_machine).
//   machine_verify   verifier.cpp: verify_shard for the machine.
// A chip's main trace is opened at zeta alone exactly when it has an AIR that reads no next-row
// value (AddSub, Jump and IO among the exported chips; a lookup-only chip is opened at both
// points, as Program, Memory and Byte are).
#pragma once
#include <string>
#include <vector>

#include "chip_program.h"
#include "prover.h"
#include "verifier.h"

namespace bfz {

constexpr int MACHINE_MAX_CHIPS = BFZ_MACHINE_MAX_CHIPS;
// Included chips of one height in a proof: the machine prover's own limit (a commit takes any
// number of matrices at any heights, merkle.hip).
constexpr size_t MACHINE_MAX_SAME_HEIGHT = 8;

struct MachineChip {
  std::string name;  // bytes, unique in the machine
  ChipProgram p;
  bool local_only = false;
  int prep_index = -1;   // its matrix in the preprocessed round, or -1
  size_t prep_height = 0;
  DBuf<uint32_t> code, list;     // the device lists (a proving machine)
  DBuf<uint32_t> prep_evals;     // column-major bit-reversed preprocessed trace
  std::vector<uint32_t> prep_host;  // the same trace as given (row-major): machine_check's host path
};

struct MachineProgram {
  std::vector<MachineChip> chips;
  std::vector<int> prep_chips;  // chip of the k-th preprocessed matrix, sorted (Reverse(height), name)
  bool has_prep = false, can_prove = false;
  Round prep;                   // the committed preprocessed round (a proving machine)
  uint32_t prep_root[8] = {0};
  std::vector<std::string> names() const {
    std::vector<std::string> v;
    for (const MachineChip& c : chips) v.push_back(c.name);
    return v;
  }
};

struct MachineChipIn {
  const uint8_t* name;
  size_t name_len;
  const uint8_t *air, *lookups;
  size_t air_len, lookups_len;
  const uint32_t* prep;  // row-major Montgomery words, or nullptr
  size_t prep_height;    // of a chip with preprocessed columns
};
// with_traces: every chip with prep_width > 0 brings its trace (device work: the API lock is
// held); otherwise root (8 Montgomery words, ignored when no chip has preprocessed columns) and
// the heights describe the commitment and no device is touched.
std::unique_ptr<MachineProgram> machine_create(const MachineChipIn* in, size_t n, bool with_traces,
                                               const uint32_t* root);
void machine_observe(const MachineProgram& m, Challenger& ch);

// chips[i]: index in m.chips of the i-th included chip; traces[i]: row-major Montgomery words,
// heights[i] x main width.  ch is advanced to the end of the opening.  Returns BFZ1 bytes whose
// chip words are indices into m.chips.
std::vector<uint8_t> machine_prove(const MachineProgram& m, const int* chips,
                                   const uint32_t* const* traces, const size_t* heights, size_t n,
                                   Challenger& ch, const ProveOptions& opt);
VerifyOutcome machine_verify(const MachineProgram& m, Challenger& ch, const uint8_t* proof,
                             size_t len, const VerifyOptions& opt);
// verify_batch's contract (verifier.h) for machine proofs: chs[i] is proof i's challenger after
// machine_observe.  run_queries == nullptr is machine_verify proof by proof; otherwise the query
// loops of all proofs go to run_queries as one batch of MQProof descriptors (verify_machine.h),
// with machine_verify's outcomes and ending challengers.
std::vector<VerifyOutcome> machine_verify_batch(const MachineProgram& m, Challenger* chs,
                                                const uint8_t* const* proofs, const size_t* lens,
                                                size_t n, const VerifyOptions& opt,
                                                QueryRunner run_queries);

// machine_prove's refusals of its inputs (null or repeated chips, heights, a chip away from its
// preprocessed height, a missing preprocessed chip; with same_height_limit the prover's
// MACHINE_MAX_SAME_HEIGHT), then the commit order: positions in the caller's arrays sorted by
// (Reverse(height), name).
std::vector<int> machine_trace_order(const MachineProgram& m, const int* chips,
                                     const uint32_t* const* traces, const size_t* heights, size_t n,
                                     bool same_height_limit);

// StarkMachine::debug_constraints (crates/stark/src/machine.rs:288-387) for the machine: alpha
// then beta sampled from ch (advanced), every chip's permutation trace and cumulative sum, every
// constraint of every row of every chip on the trace domain.  No LDE, no commit.  Inputs as
// machine_prove's, refused as it refuses them, except that any number of chips may share a height.
// on_device: k_perm_rows_machine, the running sums and k_check_machine<HAS_AIR> (one launch per
// class of chips, every chip a segment); otherwise a single-threaded loop over the same compiled
// lists that touches no device.  Both give the same words.
struct MachineCheck {
  bool ok = false;               // every row of every chip holds and cumsum is zero
  EF alpha{}, beta{}, cumsum{};  // cumsum: the sum of the chips' cumulative sums (machine.rs:337)
  std::vector<ChipCheck> chips;  // the caller's order; chip = the index in m.chips
  // the constraint profile: chip i's num_constraints entries start at the sum of the earlier K
  std::vector<uint64_t> counts;
  std::vector<int64_t> first_rows;
};
MachineCheck machine_check(const MachineProgram& m, const int* chips, const uint32_t* const* traces,
                           const size_t* heights, size_t n, Challenger& ch, bool on_device);

// Diagnostic (bfz_machine_time): single launches of the segmented kernels (form A) against the
// loop of per-chip launches (form B) on the same device inputs, alternating after one warm-up of
// each; perm_ms / quot_ms: [2][runs] HIP-event milliseconds (A then B).  Throws if the two forms'
// words differ.
void machine_time(const MachineProgram& m, const int* chips, const uint32_t* const* traces,
                  const size_t* heights, size_t n, int runs, float* perm_ms, float* quot_ms);

// The permutation constraints of a compiled interaction list over EF rows (the verifier at zeta),
// in perm_constraints' order: batches + 3 values.  perm_l / perm_n: perm_width() EF columns.
void chip_perm_eval_ef(const LookupProgram& lk, const EF* main_l, const EF* prep_l, const EF* perm_l,
                       const EF* perm_n, const EF& alpha, const EF* beta_pows, const EF& cumsum,
                       const EF& first, const EF& last, const EF& trans, EF* out);

}  // namespace bfz
