// Device query phase for machine proofs of caller-defined chips (verify_machine.hip): the packed
// batch verifier.cpp pack_machine_proof builds, and the entry point that runs it.
//
// The batch is verify.h's array of words -- the keys, the two_adic_gen table, one fixed-size
// descriptor per proof, then each proof's data -- but nothing in a descriptor is an array of a
// compile-time length: a proof's rounds, Merkle height groups, LDE heights and coefficient vectors
// are tables of their own in the data words, as long as the machine makes them (32 chips: up to
// 160 opened matrices, 24 heights, any number of matrices in one height group, rows of any width).
// Per proof, in the data words:
//   the query indices, the commit-phase roots, the betas            as in verify.h
//   nrounds MQRound entries, each followed by its group table        (log height, total width) per
//                                                                    Merkle height group, tallest first
//   nheights MQHeight entries, each with two coefficient vectors     coef0[ncols], coef1[ncols] (EF):
//                                                                    alpha^k of the height's columns
//                                                                    at zeta and at zeta * g
//   the query records                                                as in verify.h
// A height's columns are the columns of its matrices in the verifier's order (round, then matrix).
// In a query record a round's rows stand in Merkle order, which is stable, so the matrices of one
// height in one round are one run of words: a height's columns are at most one segment per round.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "verify.h"

namespace bfz {

constexpr int MQ_MAX_ROUNDS = 4;  // preprocessed, main, permutation, quotient (machine_verify)

struct MQRound {     // one input round's Merkle opening
  uint32_t rows_off, path_off;  // inside the query record
  uint32_t lb, ngroups;         // path length; height groups
  uint32_t grp_off;             // word offset in the batch of the ngroups (lh, w) pairs
  uint32_t root[8];
};
struct MQHeight {    // one LDE height
  uint32_t lh, ncols;
  uint32_t coef_off;            // word offset in the batch: coef0[ncols] then coef1[ncols]
  // column c of the height is record word c + seg_delta[s] (mod 2^32) for the last s with
  // seg_c0[s] <= c; unused entries of seg_c0 hold ncols
  uint32_t seg_c0[MQ_MAX_ROUNDS], seg_delta[MQ_MAX_ROUNDS];
  kb::EF a0, a1;                // sum of alpha^k * opened value over the columns of each point
  kb::EF z0, z1;                // the two points
};
struct MQProof {
  uint32_t nq;                  // queries sent to the device
  uint32_t log_max, ncommit, nrounds, nheights;
  uint32_t qbase, qstride;      // query records: word offset in the batch and record length
  uint32_t idx_off, croot_off, beta_off;  // word offsets in the batch
  uint32_t rd_off, ht_off;      // the MQRound and MQHeight tables (word offsets in the batch)
  uint32_t steps_off;           // commit-phase openings inside the query record
  uint32_t leaf_base;           // words into the leaves workspace: 8 * ncommit per query
  uint32_t ro_base;             // words into the reduced-openings workspace: 4 * VQ_RO_SLOTS per query
  kb::EF final_poly;
};
static_assert(sizeof(MQRound) % 4 == 0 && sizeof(MQHeight) % 4 == 0 && sizeof(MQProof) % 4 == 0,
              "the descriptors are arrays of words");

// Runs the query phase of every proof of a batch of MQProof descriptors on the calling thread's
// lane (one upload, four kernels, one download) and writes the proofs' keys to keys[0..nproofs).
void machine_queries_device(const QueryBatch& b, uint32_t* keys, hipStream_t st);

// Diagnostic (bfz_machine_verify_time): HIP-event milliseconds of `runs` passes over one uploaded
// batch after a warm-up pass; ms[5 * r + k], k = clearing the reduced-openings workspace,
// k_mverify_reduce, k_mverify_fold, k_mverify_paths, k_mverify_inputs.
void machine_queries_time(const QueryBatch& b, int runs, float* ms, hipStream_t st);

}  // namespace bfz
