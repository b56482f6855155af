// TwoAdicFriPcs::open [p3-recalled] on the device (see pcs_open.hip): the one PCS opening of the
// machine prover (prover.hip: open_impl) and of the per-chip uni-STARK prover (uni_stark.hip).
#pragma once
#include <functional>
#include <utility>
#include <vector>

#include "proof.h"
#include "prover.h"

namespace bfz {

constexpr int LOG_BLOWUP = 1;
constexpr int POW_BITS = 16;

// How one proof is split over the ranks of a shard context.  Rank k owns the
// bit-reversed positions [k H/G, (k+1) H/G) of every vector of height H >= G * 1024 (LDEs,
// Merkle layers, reduced openings, FRI layers): the natural rows i = r (mod G), r = bitrev_G(k).
// Shorter vectors are replicated.
struct Plan {
  int G = 1, lg = 0, k = 0, r = 0;
  int r2 = 0, k2 = 0;  // residue class of the quotient's next rows (i + 2) and its owner
  bool on() const { return G > 1; }
  bool sharded(size_t H) const { return G > 1 && H >= (size_t)G * SHARD_MIN_LEAVES; }
  size_t blk(size_t H) const { return H >> lg; }
  size_t row0(size_t H) const { return (size_t)k * blk(H); }
};
Plan make_plan();  // of shard_ctx(); the unsharded plan without one

// Stage times of a timed call: event pairs on the prover stream, resolved by collect().
struct EvTimer {
  bool on = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> evs;
  std::vector<double*> dst;
  hipEvent_t begin(hipStream_t st) {
    hipEvent_t e;
    HIP_CHECK(hipEventCreate(&e));
    HIP_CHECK(hipEventRecord(e, st));
    return e;
  }
  void end(hipEvent_t b, hipStream_t st, double* into) {
    hipEvent_t e;
    HIP_CHECK(hipEventCreate(&e));
    HIP_CHECK(hipEventRecord(e, st));
    evs.push_back({b, e});
    dst.push_back(into);
  }
  void collect() {
    for (size_t i = 0; i < evs.size(); i++) {
      HIP_CHECK(hipEventSynchronize(evs[i].second));
      float ms = 0;
      HIP_CHECK(hipEventElapsedTime(&ms, evs[i].first, evs[i].second));
      *dst[i] += ms;
      HIP_CHECK(hipEventDestroy(evs[i].first));
      HIP_CHECK(hipEventDestroy(evs[i].second));
    }
    evs.clear();
    dst.clear();
  }
};

// One committed round of the opening, in transcript order.
struct PcsRound {
  const Round* round;
  // The rounds of one group are opened together and their values copied to the host as soon as
  // they are done, so the host observes a group while the GPU opens the next (single GPU only;
  // groups are numbered from 0 without gaps, in round order, at most Lane::NGEV of them).
  int group;
  std::vector<uint8_t> two;  // per matrix: opened at zeta and zeta w_n (1) or at zeta alone (0)
};

struct PcsOpenIn {
  std::vector<PcsRound> rounds;
  // zeta in device memory, read by the single-GPU openings.  A sharded plan needs the host value
  // too (zeta); the single-GPU path never reads it, so a caller whose zeta is sampled on the
  // device passes `replay`, run once the openings are queued: the host's transcript catches up
  // there (it must leave ch where the opened values are observed).
  const EF* zeta_d = nullptr;
  EF zeta{};
  std::function<void()> replay;
  Plan plan;                        // uni-STARK: the unsharded plan
  const ShardCtx* shard = nullptr;  // ... and no shard context
  bool observe_openings = true;     // decision D1
  int num_queries = 84;
  EvTimer* ev = nullptr;            // timing sink: the open and fri stages (StageTimes) when ev->on
  StageTimes* tms = nullptr;
};

struct PcsOpenOut {
  struct MatPts {
    int npts;
    size_t off[2];  // offsets into `opened`
  };
  std::vector<EF> opened;
  std::vector<std::vector<MatPts>> mp;  // [round][matrix]
  std::vector<Digest> commit_roots;     // the FRI commit phase
  EF final_poly;
  uint32_t pow_witness;  // canonical
  // Every query in serialized form (canonical words + length words), in the lane's pinned tail
  // box: valid until the next opening on this lane.
  const uint32_t* words = nullptr;
  size_t nwords = 0;
};

// Opened values, reduced openings, the FRI commit phase, the grind and the query openings; ch is
// advanced to the end of the opening.  The caller holds the API lock and synchronizes the stream
// before it returns (the lane's pinned boxes are reused by the next call).
PcsOpenOut pcs_open(const PcsOpenIn& in, Challenger& ch);

}  // namespace bfz
