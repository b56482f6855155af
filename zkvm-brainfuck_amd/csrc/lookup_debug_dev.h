// The aggregation table of lookup_debug.hip and its device helpers, shared by the kernels that
// probe it: k_lookup<CHIP, PHASE> (lookup_debug.hip, the compiled chips) and k_lookup_prog<PHASE>
// with the multiplicity kernels (lookup_debug_prog.hip, chips given as interaction lists).  The
// table layout, the rounds protocol and its argument are in lookup_debug.hip's header.
//
// lk_aggregate is the rounds driver: count, size the table, claim / materialise / account until no
// key is unresolved, scan, collect, shares.  What differs between the two callers is "launch this
// phase for chip k", which it takes as a callable.
#pragma once
#include <functional>

#include "lookup_debug.h"

namespace bfz {
namespace {
constexpr uint32_t LK_MAX_ROUNDS = 1u << 12;
constexpr int LK_MAX_BLOCKS = 2048;
constexpr int LK_CACHE_LOG = 11, LK_CACHE = 1 << LK_CACHE_LOG;  // per-block LDS table (account)
constexpr uint32_t LK_NO_SLOT = 0xFFFFFFFFu;
constexpr uint32_t LK_ERR_FULL = 1, LK_ERR_STATE = 2;

enum { PH_COUNT = 0, PH_CLAIM = 1, PH_MATERIALISE = 2, PH_ACCOUNT = 3, PH_SHARES = 4 };
}  // namespace

struct LkTable {
  unsigned long long* tag;
  unsigned long long* net;  // two's complement of the signed sum
  unsigned long long* rep;
  uint32_t* mask;
  uint32_t* aux;  // rounds: the round the key was written in; shares pass: selected index + 1;
                  // multiplicities: the smallest table row that holds the key
  uint32_t* key;  // LK_KEY_WORDS per slot
  int logsize;
};

struct LkCtl {
  unsigned long long interactions, unresolved, collisions;
  unsigned long long distinct, unbalanced, chip_distinct[NUM_CHIPS], total, cursor;
  uint32_t error, pad;
};

// One pass of the driver over the chips: what a launch of a phase is handed.
struct LkPass {
  int phase;
  uint32_t round;
  unsigned long long hash_mask;
  uint32_t combine;  // BFZ_LOOKUP_COMBINE
  LkTable T;
  LkCtl* ctl;
  unsigned long long* share_net;  // PH_SHARES: nsel x stride
  uint32_t* share_count;
  hipStream_t st;
};

struct LkDriver {
  int nchips;         // launches per pass
  int stride;         // chips per record of the share arrays and of chip_distinct
  bool runtime_stride;  // stride is not NUM_CHIPS: k_lookup_scan_n in the place of k_lookup_scan
  int rep_bits;       // the representative is chip << 32 | row << rep_bits | interaction
  std::function<void(int k, const LkPass&)> launch;  // launch this phase for chip k
  std::function<void(const LkPass&)> after_rounds;   // optional: the table holds every net
};

// What the driver leaves beside the LookupReport (whose fixed per-chip arrays it does not touch):
// chip_distinct[stride], and per record share_net / share_count [stride].
struct LkShares {
  std::vector<uint64_t> chip_distinct;
  std::vector<long long> net;
  std::vector<uint32_t> count;
};

void lk_aggregate(const LkDriver& d, size_t cap, bool low_hash_bits, LookupReport& out, LkShares& sh);
int32_t lk_net_to_int(long long net);  // field_to_int of a signed sum

__device__ __forceinline__ unsigned long long lk_hash(const uint32_t (&key)[LK_KEY_WORDS]) {
  unsigned long long h = 0x9E3779B97F4A7C15ull;
#pragma unroll
  for (int i = 0; i < LK_KEY_WORDS; i++) {
    h = (h ^ key[i]) * 0xFF51AFD7ED558CCDull;
    h ^= h >> 32;
  }
  h ^= h >> 29;
  h *= 0xC4CEB9FE1A85EC53ull;
  h ^= h >> 32;
  return h;
}

__device__ __forceinline__ bool lk_key_equal(const uint32_t* __restrict__ slot_key,
                                             const uint32_t (&key)[LK_KEY_WORDS]) {
  const uint4 a = *reinterpret_cast<const uint4*>(slot_key);
  const uint4 b = *reinterpret_cast<const uint4*>(slot_key + 4);
  return a.x == key[0] && a.y == key[1] && a.z == key[2] && a.w == key[3] && b.x == key[4] &&
         b.y == key[5] && b.z == key[6] && b.w == key[7];
}

__device__ __forceinline__ unsigned long long lk_load(const unsigned long long* p) {
  // device-scope load: another CU's atomic on this word is seen, not an older L1 line
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The slot of round `round` for (key, tag), probing from `home`: the first slot of this tag whose
// key is not written yet or was written in this round (resolved = false), or whose key, written
// in an earlier round, is this key (resolved = true).  CLAIM: an empty slot is claimed.  -1 and
// an error bit if the probe runs round the table, or (not CLAIM) meets an empty slot.
template <bool CLAIM>
__device__ __forceinline__ int lk_walk(const LkTable& T, const uint32_t (&key)[LK_KEY_WORDS],
                                       unsigned long long tag, uint32_t home, uint32_t round,
                                       bool& resolved, uint32_t& err) {
  const uint32_t size = 1u << T.logsize, wrap = size - 1;
  resolved = false;
  for (uint32_t step = 0; step < size; step++) {
    const uint32_t i = (home + step) & wrap;
    unsigned long long t = CLAIM ? lk_load(&T.tag[i]) : T.tag[i];
    if (t == 0) {
      if (!CLAIM) {
        err |= LK_ERR_STATE;
        return -1;
      }
      t = atomicCAS(&T.tag[i], 0ull, tag);
      if (t == 0) t = tag;
    }
    if (t != tag) continue;
    const uint32_t rd = T.aux[i];
    if (rd == 0 || rd == round) return (int)i;
    if (lk_key_equal(T.key + (size_t)i * LK_KEY_WORDS, key)) {
      resolved = true;
      return (int)i;
    }
  }
  err |= LK_ERR_FULL;
  return -1;
}

// After the rounds: the slot that holds `key`, or -1 and an error bit.
__device__ __forceinline__ int lk_find(const LkTable& T, const uint32_t (&key)[LK_KEY_WORDS],
                                       unsigned long long tag, uint32_t home, uint32_t& err) {
  const uint32_t size = 1u << T.logsize, wrap = size - 1;
  for (uint32_t step = 0; step < size; step++) {
    const uint32_t i = (home + step) & wrap;
    const unsigned long long t = T.tag[i];
    if (t == 0) break;
    if (t == tag && lk_key_equal(T.key + (size_t)i * LK_KEY_WORDS, key)) return (int)i;
  }
  err |= LK_ERR_STATE;
  return -1;
}

// The same where a key that nobody sent is normal (a table row of the multiplicity kernels): -1
// and no error.  The probe is bounded by the table size, which always has empty slots.
__device__ __forceinline__ int lk_find_opt(const LkTable& T, const uint32_t (&key)[LK_KEY_WORDS],
                                           unsigned long long tag, uint32_t home) {
  const uint32_t size = 1u << T.logsize, wrap = size - 1;
  for (uint32_t step = 0; step < size; step++) {
    const uint32_t i = (home + step) & wrap;
    const unsigned long long t = T.tag[i];
    if (t == 0) break;
    if (t == tag && lk_key_equal(T.key + (size_t)i * LK_KEY_WORDS, key)) return (int)i;
  }
  return -1;
}

__device__ __forceinline__ unsigned long long lk_wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// One atomicAdd per block (every thread of the block calls it).
__device__ __forceinline__ void lk_block_add(unsigned long long v, unsigned long long* dst,
                                             unsigned long long* sh4) {
  v = lk_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long s = sh4[0] + sh4[1] + sh4[2] + sh4[3];
    if (s) atomicAdd(dst, s);
  }
}

}  // namespace bfz
