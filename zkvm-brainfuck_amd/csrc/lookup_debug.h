// Per-key lookup discrepancies: the part of debug_interactions_with_all_chips
// (crates/stark/src/lookup/debug.rs:59-196) the constraint checker's per-kind table
// (debug_check.h) leaves out.  For every lookup tuple "{kind} (v0, v1, ...)" (debug.rs:100) the
// sends minus the receives over all chips, each chip's share (debug.rs:145-152) and the first
// interaction that carries the key.  The multiset does not depend on alpha or beta, so it also
// shows keys that differ while the totals match (debug.rs:188-191).
//
// The interactions are the Lookup tables of air.h evaluated with vcol_eval<BaseOps>; lookup_eval
// below is KB_HD: the host path runs it single-threaded over a std::map, the kernels of
// lookup_debug.hip one row per thread into an open-addressing table in HBM.
//
// A key is 8 words: kind << 8 | nvals, then the values as CANONICAL integers (unused entries 0).
// Records are ordered by (kind, values as integers, lexicographically) -- not the reference's
// BTreeMap<String> order, where "10" sorts before "9".
#pragma once
#include <array>
#include <vector>

#include "air.h"
#include "prover.h"

namespace bfz {

constexpr int LK_MAX_VALUES = 7;
constexpr int LK_KEY_WORDS = 8;

// field_to_int (lookup/debug.rs:46-54) of a canonical word: an integer in (-p/2, p/2].
KB_HD int32_t field_to_int(uint32_t canon) {
  return canon > kb::P / 2 ? (int32_t)canon - (int32_t)kb::P : (int32_t)canon;
}

// Interaction J of CHIP on one row (debug.rs:80-115): false when its kind is not selected or its
// multiplicity is zero (debug.rs:81-83,94); else the key and the signed multiplicity, sends
// positive (debug.rs:110-114), as field_to_int gives it.
template <int CHIP, int J>
KB_HD bool lookup_eval(const uint32_t* L, const uint32_t* PL, unsigned kinds_mask,
                       uint32_t (&key)[LK_KEY_WORDS], int32_t& val) {
  constexpr Lookup lk = LookupsOf<CHIP>::v.l[J];
  if (!((kinds_mask >> lk.kind) & 1u)) return false;
  const uint32_t m = vcol_eval<BaseOps>(lk.mult, PL, L);
  if (m == 0) return false;
  const int32_t x = field_to_int(kb::from_mont(m));
  val = lk.send ? x : -x;
  key[0] = ((uint32_t)lk.kind << 8) | (uint32_t)lk.nvals;
#pragma unroll
  for (int v = 0; v < LK_MAX_VALUES; v++)
    key[1 + v] = v < lk.nvals ? kb::from_mont(vcol_eval<BaseOps>(lk.vals[v], PL, L)) : 0;
  return true;
}

struct LookupDiscrepancy {
  int kind = 0, nvals = 0;
  uint32_t values[LK_MAX_VALUES] = {};  // canonical
  int32_t net = 0;                      // field_to_int(sends - receives), != 0
  int32_t chip_net[NUM_CHIPS] = {};
  uint32_t chip_count[NUM_CHIPS] = {};
  int first_chip = -1, first_interaction = -1;  // the smallest (chip, row, interaction)
  int64_t first_row = -1;
};

struct LookupReport {
  bool balanced = false;
  int32_t total_net = 0;
  uint64_t interactions = 0, distinct_keys = 0, unbalanced_keys = 0;
  uint64_t chip_distinct[NUM_CHIPS] = {};
  uint32_t rounds = 0, tag_collisions = 0;
  uint64_t table_bytes = 0;
  std::vector<LookupDiscrepancy> recs;  // the first min(unbalanced_keys, cap) in key order
};

// bit k of kinds_mask selects LookupKind k; 0 or a bit outside 1..7 throws.
void check_kinds_mask(unsigned kinds_mask);

// Host path: row-major natural-order main traces (Montgomery) with the validation of
// upload_host_traces; the preprocessed traces of Program and Byte are the program's
// (machine.rs:309-312).  Single-threaded, no device.
void debug_interactions_host(const Program& program, const int* chips,
                             const uint32_t* const* traces, const size_t* heights,
                             const size_t* widths, size_t nchips, unsigned kinds_mask, size_t cap,
                             LookupReport& out);

// Device path: column-major bit-reversed traces in HBM (gpu.h LAYOUT), pk.prep_evals for Program
// and Byte.  low_hash_bits (tests): the key hash is cut to its low 12 bits before anything uses
// it, so distinct keys share tags and the multi-round path runs.
void debug_interactions_device(const ProvingKey& pk, const DeviceTraces& dt, unsigned kinds_mask,
                               size_t cap, bool low_hash_bits, LookupReport& out);

}  // namespace bfz
