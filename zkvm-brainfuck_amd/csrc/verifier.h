// Host verifier: Verifier::verify_shard (crates/stark/src/verifier.rs:27-329)
// + TwoAdicFriPcs::verify / fri::verifier [p3-recalled] + BfProver::verify's CPU-degree cap
// (crates/prover/src/verify.rs:10-36), over a decoded ShardProof (proof.h) -- so the same checks
// run on the BFZ1 normal form and on the reference's bincode bytes.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "proof.h"

namespace bfz {

struct VerifyOptions {
  int num_queries = 84;
  bool observe_openings = true;  // PCS transcript variant (decision D1)
};

// Main and permutation (base) columns a chip's constraints read at the next row.
struct NextCols {
  std::vector<int> main, perm;
};
NextCols next_row_columns(int chip);

bool verify_shard(const std::string& program_src, const uint32_t vk_commit[8], const ShardProof& pf,
                  const VerifyOptions& opt, std::string* why);

// BFZ1 bytes (decode_bfz1 + verify_shard)
bool verify_proof(const std::string& program_src, const uint32_t vk_commit[8], const uint8_t* proof,
                  size_t len, const VerifyOptions& opt, std::string* why);

// One proof's verdict: the reason is verify_shard's; query is the query whose check failed first,
// -1 when the rejection is not a query's (decode, shape, transcript, OOD, cumulative sum).
struct VerifyOutcome {
  bool ok = false;
  int query = -1;
  std::string why;
};

// n proofs of one program.  run_queries == nullptr: the host verifier, proof by proof.  Otherwise
// every proof's checks before the query loop run on the host, the query loops of the proofs that
// got that far are packed into one QueryBatch (verify.h) and handed to run_queries, which returns
// one key per packed proof, and the checks after the query loop run on the host for the proofs
// whose queries passed.  Either way a proof's outcome is the host verifier's.
struct QueryBatch;
using QueryRunner = void (*)(const QueryBatch& batch, uint32_t* keys);
std::vector<VerifyOutcome> verify_batch(const std::string& program_src, const uint32_t vk_commit[8],
                                        const uint8_t* const* proofs, const size_t* lens, size_t n,
                                        const VerifyOptions& opt, QueryRunner run_queries);

}  // namespace bfz
