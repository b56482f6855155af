// Device query phase of the verifier (verify.hip): the packed batch the host builds
// (verifier.cpp pack_proof) and the entry point that runs it.
//
// The verifier's query loop (TwoAdicFriPcs::verify + fri::verifier [p3-recalled], the host form is
// verifier.cpp check_query) is, per query, one MerkleTreeMmcs opening per input round (four in a
// machine proof, two in a per-chip uni-STARK proof), the reduced openings of every LDE height, the
// FRI fold chain and one Merkle opening per commit-phase step.  Everything a kernel indexes with -- widths, heights, path lengths, offsets -- is written
// into the descriptors below by the host from the program, the vk and the shapes it has already
// validated; the proof's own bytes are only ever read as field words at those offsets.
//
// One batch is one array of 32-bit words:
//   [0, np)            one key per proof, 0xffffffff on upload; the kernels atomicMin the key
//                      query * 64 + stage of every failed check into it (stage: 0..nrounds-1 the input
//                      rounds, 4 + s commit-phase step s, 63 the final-value comparison), so the
//                      smallest key is the first failure in the host verifier's order
//   [np, np + 64)      two_adic_gen(k) and its inverse, k < 32
//   then np VProof descriptors, then per proof: the query indices, the commit-phase roots, the
//   betas, alpha^0..63 and the query records.  A query record holds, per input round, the opened
//   rows in Merkle order (tallest first, stable) followed by the path, then per commit-phase step
//   the sibling (4 words) and the path.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "kb.h"

namespace bfz {

constexpr uint32_t VQ_NO_FAILURE = 0xffffffffu;
constexpr int VQ_STAGE_STEP0 = 4, VQ_STAGE_FINAL = 63;
// Distinct LDE heights of a proof: one per chip when the preprocessed chips claim their key's log
// degrees, as every honest proof does.  A proof that claims others can reach 10; pack_proof refuses
// it and its queries are checked on the host.
constexpr int VQ_MAX_HEIGHTS = 8;
constexpr int VQ_MAX_MATS = 34;     // 2 preprocessed + 8 main + 8 permutation + 16 quotient chunks
constexpr int VQ_MAX_WIDTH = 64;    // widest opened row (Jump: 45)
constexpr int VQ_RO_SLOTS = 32;     // reduced openings of one query, by log height

struct VMatD {       // one opened matrix
  uint32_t off;      // its row inside the query record
  uint32_t w, np;    // width; points it is opened at (1: zeta, 2: zeta and zeta * g)
  kb::EF c0, c1;     // alpha^k of its first column at the first / second point
};
struct VHeightD {    // one LDE height: matrices [m0, m1) of VProof::mats
  uint32_t lh, m0, m1;
  kb::EF a0, a1;     // sum of alpha^k * opened value over the (matrix, column)s of each point
  kb::EF z0, z1;     // the two points
};
struct VRoundD {     // one input round's Merkle opening
  uint32_t rows_off, path_off;  // inside the query record
  uint32_t lb, ngroups;         // path length; height groups, tallest first
  uint32_t g_lh[VQ_MAX_HEIGHTS], g_w[VQ_MAX_HEIGHTS];  // a group's log height and total width
  uint32_t root[8];
};
struct VProof {
  uint32_t nq;                  // queries sent to the device
  uint32_t log_max, ncommit;
  uint32_t qbase, qstride;      // query records: word offset in the batch and record length
  uint32_t idx_off, croot_off, beta_off, apow_off;  // word offsets in the batch
  uint32_t steps_off;           // commit-phase openings inside the query record
  uint32_t leaf_base;           // words into the leaves workspace: 8 * ncommit per query
  uint32_t ro_base;             // words into the reduced-openings workspace: 4 * VQ_RO_SLOTS per query
  uint32_t nheights, nmats;
  uint32_t nrounds;             // input rounds in use: 4 in a machine proof, 2 in a BFU1 proof
  kb::EF final_poly;
  VRoundD rd[4];
  VHeightD hs[VQ_MAX_HEIGHTS];
  VMatD mats[VQ_MAX_MATS];
};
static_assert(sizeof(VProof) % 4 == 0, "VProof is an array of words");

struct QueryBatch {
  std::vector<uint32_t> words;  // the layout above
  uint32_t nproofs = 0;
  uint32_t max_nq = 0, max_ncommit = 0, max_nrounds = 0;
  size_t leaf_words = 0, ro_words = 0;  // workspace sizes
  size_t desc_off() const { return (size_t)nproofs + 64; }
};

// Runs the query phase of every proof of the batch on the calling thread's lane (one upload, three
// kernels, one download) and writes the proofs' keys to keys[0..nproofs).
void verify_queries_device(const QueryBatch& b, uint32_t* keys, hipStream_t st);

}  // namespace bfz
