// LogUp interactions as data: a caller-defined chip's sends and receives arrive as an
// interaction program (the BFL1 format of include/bfz.h: air.h's Lookup / VCol / VTerm written
// flat) and its permutation trace and cumulative sum are computed by one kernel, whatever the
// chip -- what the reference gets from Chip::new deriving the interactions of any AIR
// (crates/stark/src/chip.rs:65-90) and generate_permutation_trace running over whatever it is
// handed (crates/stark/src/permutation.rs:75-148).
//
//   lookups_compile          validation (every failure names the word offset) and the flat list
//                            the kernel and the host loop read.
//   lookups_export           a built-in chip's program, from LookupsOf<CHIP>.
//   lookups_perm_trace_host  a single-threaded loop over the compiled list (on_device = 0).
// The kernel k_perm_rows_prog<WRITE> and its launchers are in lookup_program.hip.
//
// The compiled list, in 32-bit words (field values as Montgomery words):
//     [0]                    n_interactions
//     [1 .. 1 + LKP_BATCHES)  word offset of batch b's first interaction (0 past the last batch)
//     per interaction        (n_values | send << 8, kind)
//                            mult VCOL, then n_values value VCOLs
//     VCOL                   (constant, n_terms), then n_terms x (weight, source << 16 | column)
// Everything is a pair, so a reader advances by two words at a time; the offset table lets the
// kernel's backward pass reach batch b without walking the batches before it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/bfz.h"
#include "air.h"
#include "gpu.h"
#include "logup.h"

namespace bfz {

constexpr uint32_t LKP_MAGIC = 0x314c4642;  // "BFL1"
constexpr int LKP_MAX_VALUES = BFZ_LOOKUPS_MAX_VALUES;  // PermChallenges::beta_pows[8]
constexpr int LKP_MAX_TERMS = BFZ_LOOKUPS_MAX_TERMS;
constexpr int LKP_BATCHES = (BFZ_LOOKUPS_MAX + 1) / 2;  // logup_batch_size = 2
constexpr int LKP_HEAD = 1 + LKP_BATCHES;                // words before the first interaction

struct LookupProgram {
  int main_w = 0, prep_w = 0, n = 0, sends = 0, receives = 0;
  std::vector<uint32_t> list;  // the compiled list
  int batches() const { return (n + 1) / 2; }
  int perm_width() const { return batches() + 1; }  // permutation.rs:15-21, in EF columns
};

// Throws std::runtime_error naming the word offset.  Reads nothing outside [prog, prog + len).
LookupProgram lookups_compile(const uint8_t* prog, size_t len);

// The BFL1 bytes of a built-in chip's interactions (all eight chips).
std::vector<uint8_t> lookups_export(int chip);

// main / prep: row-major natural-order Montgomery words (< p), h rows.  out (optional): h x
// 4 * perm_width() row-major natural order.  A zero denominator is not detected (its inverse is
// taken as 0), as on the device.
void lookups_perm_trace_host(const LookupProgram& p, const uint32_t* main, const uint32_t* prep,
                             size_t h, const PermChallenges& ch, uint32_t* out, kb::EF* cumsum);

// The host loop's step, for other host loops over a compiled list (chip_program.cpp): the
// interaction at list[at] over one row (m / pr: its main and preprocessed words), its denominator
// and signed multiplicity (a receive's negated); at advances past it.
void host_interaction(const uint32_t* list, size_t& at, const uint32_t* m, const uint32_t* pr,
                      const PermChallenges& ch, kb::EF& den, uint32_t& mult);

// ---- device side (lookup_program.hip).  list_dev: the compiled list in device memory; mainc /
// prepc: column-major bit-reversed traces of n rows; ch: device memory.  perm: 4 * perm_width()
// base columns, or nullptr: the cumulative sum alone (k_perm_rows_prog<0>, nothing of a
// permutation trace is written).  A zero denominator is not detected, as in perm_trace.
void perm_trace_prog(const LookupProgram& p, const uint32_t* list_dev, const uint32_t* mainc,
                     const uint32_t* prepc, size_t n, const PermChallenges* ch, uint32_t* perm,
                     kb::EF* cumsum_dev, hipStream_t st);
// The row kernel alone: the batch columns of perm (or none) and rowsum[t], as perm_rows.
void perm_rows_prog(const LookupProgram& p, const uint32_t* list_dev, const uint32_t* mainc,
                    const uint32_t* prepc, size_t n, const PermChallenges* ch, uint32_t* perm,
                    kb::EF* rowsum, hipStream_t st);
// total = the sum of n EF values (the verifier's sum of cumulative sums, verifier.rs:210-213).
void ef_total(const kb::EF* vals, size_t n, kb::EF* total_dev, hipStream_t st);

}  // namespace bfz
