// Per-key lookup discrepancies (lookup_debug.h): the BTreeMap<String, ..> of
// crates/stark/src/lookup/debug.rs:59-196 as a multiset aggregation in HBM.
//
// TABLE: open addressing, linear probing, structure of arrays.  Per slot a 64-bit tag (the key's
// hash with bit 63 set; 0 = empty), a signed 64-bit net, a 64-bit representative
// chip << 32 | row << 4 | interaction (atomicMin picks the witness), a chip bitmask, a word
// `aux` (the round the slot's key was written in) and the 8 key words.  A tag is written once
// (atomicCAS from 0) and a slot's key once, so whatever a probe has walked past stays as it was.
//
// ROUNDS: k_lookup<CHIP, PHASE> walks every row of a chip, one row per thread per grid-stride
// step, with the chip's interactions unrolled.  Round r runs three phases over all chips:
//   claim        every interaction not accounted yet probes from its home slot, claims the first
//                empty slot or accepts the first slot of its tag whose key is not written yet,
//                and atomicMins the representative;
//   materialise  the interaction that IS its slot's representative writes the key words and
//                aux = r with plain stores (one writer per slot);
//   account      every such interaction compares the full key: equal, it adds its signed
//                multiplicity and chip bit; different (two keys, one tag), it counts a tag
//                collision and takes the next slot of its tag in round r + 1.
// An interaction is accounted exactly when its probe finds its key in a slot written before
// round r; nothing is stored per interaction.  Every accepted slot settles one key per round, so
// the rounds end; with 64-bit tags that is one round.  No thread waits for another: every probe
// loop is bounded by the table size and raises an error flag, and the host bounds the rounds.
// Only integer atomics: the result does not depend on the execution order.
//
// CONTENTION: a few hundred Byte and Program keys are sent millions of times.  The account phase
// combines them in a per-block LDS table (slot -> partial sum, LDS atomics) flushed with one
// global atomic per block and slot; the claim phase skips the atomicMin when the representative
// it reads is already smaller.
//
// These kernels are not part of a proof and are NOT in a PreloadKernels list.
#include "lookup_debug.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <numeric>
#include <type_traits>

namespace bfz {

using namespace kb;

namespace {
constexpr int LK_MAIN_W[NUM_CHIPS] = {31, 1, 7, 45, 12, 2, 41, 5};
constexpr int LK_PREP_W[NUM_CHIPS] = {0, 6, 0, 0, 0, 2, 0, 0};
constexpr unsigned LK_ALL_KINDS = 0xFEu;
constexpr uint32_t LK_MAX_ROUNDS = 1u << 12;
constexpr int LK_MAX_BLOCKS = 2048;
constexpr int LK_CACHE_LOG = 11, LK_CACHE = 1 << LK_CACHE_LOG;  // per-block LDS table (account)
constexpr uint32_t LK_NO_SLOT = 0xFFFFFFFFu;
constexpr uint32_t LK_ERR_FULL = 1, LK_ERR_STATE = 2;

enum { PH_COUNT = 0, PH_CLAIM = 1, PH_MATERIALISE = 2, PH_ACCOUNT = 3, PH_SHARES = 4 };

struct LkTable {
  unsigned long long* tag;
  unsigned long long* net;  // two's complement of the signed sum
  unsigned long long* rep;
  uint32_t* mask;
  uint32_t* aux;  // rounds: the round the key was written in; shares pass: selected index + 1
  uint32_t* key;  // LK_KEY_WORDS per slot
  int logsize;
};

struct LkCtl {
  unsigned long long interactions, unresolved, collisions;
  unsigned long long distinct, unbalanced, chip_distinct[NUM_CHIPS], total, cursor;
  uint32_t error, pad;
};

using LkKey = std::array<uint32_t, LK_KEY_WORDS>;

void check_tables() {
  for (int c = 0; c < NUM_CHIPS; c++)
    if (LK_MAIN_W[c] != CHIP_INFO[c].main_w || LK_PREP_W[c] != CHIP_INFO[c].prep_w)
      throw std::runtime_error("debug_interactions: width tables out of step with CHIP_INFO");
}

int32_t net_to_int(long long net) {  // field_to_int of a signed sum
  long long r = net % (long long)P;
  if (r < 0) r += P;
  return field_to_int((uint32_t)r);
}
}  // namespace

void check_kinds_mask(unsigned kinds_mask) {
  if (kinds_mask == 0) throw std::runtime_error("debug_interactions: kinds_mask selects no LookupKind");
  if (kinds_mask & ~LK_ALL_KINDS)
    throw std::runtime_error("debug_interactions: kinds_mask has bits outside LookupKind 1..7");
}

// ------------------------------------------------------------------------ host path
namespace {
struct HostEntry {
  long long net = 0;
  long long chip_net[NUM_CHIPS] = {};
  uint32_t chip_count[NUM_CHIPS] = {};
  int first_chip = -1, first_interaction = -1;
  int64_t first_row = -1;
};
using HostMap = std::map<LkKey, HostEntry>;  // array order = (kind, values) order

template <int CHIP, int J, int NL>
void host_row(const uint32_t* L, const uint32_t* PL, unsigned kinds_mask, int64_t row, HostMap& m,
              uint64_t& interactions) {
  if constexpr (J < NL) {
    uint32_t key[LK_KEY_WORDS];
    int32_t val;
    if (lookup_eval<CHIP, J>(L, PL, kinds_mask, key, val)) {
      LkKey k;
      std::memcpy(k.data(), key, sizeof key);
      HostEntry& e = m[k];
      if (e.first_chip < 0) {  // chips ascending, rows ascending, J ascending: the smallest
        e.first_chip = CHIP;
        e.first_row = row;
        e.first_interaction = J;
      }
      e.net += val;
      e.chip_net[CHIP] += val;
      e.chip_count[CHIP] += 1;
      interactions++;
    }
    host_row<CHIP, J + 1, NL>(L, PL, kinds_mask, row, m, interactions);
  }
}

template <int CHIP>
void host_chip(const uint32_t* main, const uint32_t* prep, size_t h, unsigned kinds_mask, HostMap& m,
               uint64_t& interactions) {
  constexpr int MW = LK_MAIN_W[CHIP], PW = LK_PREP_W[CHIP];
  const uint32_t none[1] = {0};
  for (size_t i = 0; i < h; i++)
    host_row<CHIP, 0, LookupsOf<CHIP>::v.n>(main + i * MW, PW ? prep + i * PW : none, kinds_mask,
                                            (int64_t)i, m, interactions);
}

void fill_record(const LkKey& k, LookupDiscrepancy& d) {
  d.kind = (int)(k[0] >> 8);
  d.nvals = (int)(k[0] & 0xFF);
  for (int v = 0; v < LK_MAX_VALUES; v++) d.values[v] = k[1 + v];
}
}  // namespace

void debug_interactions_host(const Program& program, const int* chips,
                             const uint32_t* const* traces, const size_t* heights,
                             const size_t* widths, size_t nchips, unsigned kinds_mask, size_t cap,
                             LookupReport& out) {
  check_kinds_mask(kinds_mask);
  check_tables();
  // the validation of upload_host_traces and debug_constraints_device, with their messages
  int at[NUM_CHIPS];
  std::fill(at, at + NUM_CHIPS, -1);
  for (size_t i = 0; i < nchips; i++) {
    const int c = chips[i];
    if (c < 0 || c >= NUM_CHIPS || at[c] >= 0) throw std::runtime_error("traces: bad or repeated chip id");
    at[c] = (int)i;
    const size_t h = heights[i];
    if ((size_t)CHIP_INFO[c].main_w != widths[i])
      throw std::runtime_error(std::string("traces: width mismatch for ") + CHIP_INFO[c].name);
    if (h < 1 || (h & (h - 1)) || h > ((size_t)1 << 23))
      throw std::runtime_error(std::string("traces: height not a power of two in [1, 2^23] for ") +
                               CHIP_INFO[c].name);
    if (!traces[i]) throw std::runtime_error("null argument");
    for (size_t k = 0; k < h * widths[i]; k++)
      if (traces[i][k] >= P)
        throw std::runtime_error(std::string("traces: non-canonical field word (>= p) in ") +
                                 CHIP_INFO[c].name);
  }
  if (at[0] < 0) throw std::runtime_error("traces: the Cpu chip is required");
  std::vector<uint32_t> prep[NUM_CHIPS];
  for (int c = 0; c < NUM_CHIPS; c++)
    if (at[c] >= 0 && CHIP_INFO[c].prep_w) {
      const size_t h = prep_trace(c, program, prep[c]);
      if (h != heights[at[c]])
        throw std::runtime_error(std::string("debug_constraints: height of ") + CHIP_INFO[c].name +
                                 " differs from its preprocessed trace");
    }

  out = LookupReport();
  HostMap m;
#define BFZ_LK_CASE(C) \
  case C: host_chip<C>(traces[at[C]], prep[C].data(), heights[at[C]], kinds_mask, m, out.interactions); break;
  for (int c = 0; c < NUM_CHIPS; c++) {  // machine order (debug.rs:139-144)
    if (at[c] < 0) continue;
    switch (c) {
      BFZ_LK_CASE(CHIP_CPU)
      BFZ_LK_CASE(CHIP_PROGRAM)
      BFZ_LK_CASE(CHIP_ADDSUB)
      BFZ_LK_CASE(CHIP_JUMP)
      BFZ_LK_CASE(CHIP_MEMORY)
      BFZ_LK_CASE(CHIP_BYTE)
      BFZ_LK_CASE(CHIP_MEMINSTRS)
      BFZ_LK_CASE(CHIP_IO)
    }
  }
#undef BFZ_LK_CASE
  long long total = 0;
  out.distinct_keys = m.size();
  for (const auto& kv : m) {
    const HostEntry& e = kv.second;
    total = (total + e.net) % (long long)P;
    for (int c = 0; c < NUM_CHIPS; c++)
      if (e.chip_count[c]) out.chip_distinct[c]++;
    const int32_t net = net_to_int(e.net);
    if (net == 0) continue;
    if (out.unbalanced_keys++ >= cap) continue;
    LookupDiscrepancy d;
    fill_record(kv.first, d);
    d.net = net;
    for (int c = 0; c < NUM_CHIPS; c++) {
      d.chip_net[c] = net_to_int(e.chip_net[c]);
      d.chip_count[c] = e.chip_count[c];
    }
    d.first_chip = e.first_chip;
    d.first_row = e.first_row;
    d.first_interaction = e.first_interaction;
    out.recs.push_back(d);
  }
  out.total_net = net_to_int(total);
  out.balanced = out.unbalanced_keys == 0;
}

// ------------------------------------------------------------------------ kernels
template <int I, int N, class F>
__device__ __forceinline__ void lk_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    lk_for<I + 1, N>(f);
  }
}

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

template <int CHIP, int PHASE>
__global__ __launch_bounds__(256) void k_lookup(const uint32_t* __restrict__ mainc,
                                                const uint32_t* __restrict__ prepc, uint32_t n,
                                                int logn, unsigned kinds_mask,
                                                unsigned long long hash_mask, uint32_t round,
                                                uint32_t combine, LkTable T,
                                                LkCtl* __restrict__ ctl,
                                                unsigned long long* __restrict__ share_net,
                                                uint32_t* __restrict__ share_count) {
  constexpr int MW = LK_MAIN_W[CHIP];
  constexpr int PWD = LK_PREP_W[CHIP] > 0 ? LK_PREP_W[CHIP] : 1;
  constexpr int NL = LookupsOf<CHIP>::v.n;
  constexpr int CN = PHASE == PH_ACCOUNT ? LK_CACHE : 1;
  __shared__ uint32_t c_slot[CN];
  __shared__ unsigned long long c_sum[CN];
  __shared__ unsigned long long sh4[4];
  if constexpr (PHASE == PH_ACCOUNT) {
    for (int h = threadIdx.x; h < LK_CACHE; h += blockDim.x) {
      c_slot[h] = LK_NO_SLOT;
      c_sum[h] = 0;
    }
    __syncthreads();
  }
  unsigned long long counted = 0, unresolved = 0;
  uint32_t err = 0;
  const uint32_t chip_bit = 1u << CHIP;
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
    uint32_t L[MW], PL[PWD];
#pragma unroll
    for (int c = 0; c < MW; c++) L[c] = mainc[(size_t)c * n + t];
#pragma unroll
    for (int c = 0; c < PWD; c++) PL[c] = LK_PREP_W[CHIP] > 0 ? prepc[(size_t)c * n + t] : 0;
    const uint32_t row = dbitrev(t, logn);  // natural row of storage position t
    lk_for<0, NL>([&](auto JJ) {
      constexpr int J = decltype(JJ)::value;
      uint32_t key[LK_KEY_WORDS];
      int32_t val;
      if (!lookup_eval<CHIP, J>(L, PL, kinds_mask, key, val)) return;
      if constexpr (PHASE == PH_COUNT) {
        counted++;
        return;
      }
      const unsigned long long h = lk_hash(key) & hash_mask;
      const unsigned long long tag = h | (1ull << 63);
      const uint32_t home = (uint32_t)((h * 0x9E3779B97F4A7C15ull) >> (64 - T.logsize));
      const unsigned long long me =
          ((unsigned long long)CHIP << 32) | ((unsigned long long)row << 4) | (unsigned)J;
      const unsigned long long add = (unsigned long long)(long long)val;
      if constexpr (PHASE == PH_SHARES) {
        const int s = lk_find(T, key, tag, home, err);
        if (s < 0) return;
        const uint32_t sel = T.aux[s];
        if (sel) {
          atomicAdd(&share_net[(size_t)(sel - 1) * NUM_CHIPS + CHIP], add);
          atomicAdd(&share_count[(size_t)(sel - 1) * NUM_CHIPS + CHIP], 1u);
        }
        return;
      }
      bool resolved;
      const int s = PHASE == PH_CLAIM ? lk_walk<true>(T, key, tag, home, round, resolved, err)
                                      : lk_walk<false>(T, key, tag, home, round, resolved, err);
      if (s < 0 || resolved) return;
      if constexpr (PHASE == PH_CLAIM) {
        // the representative only falls: a larger-or-equal one read now is never the minimum
        if (lk_load(&T.rep[s]) > me) atomicMin(&T.rep[s], me);
      } else if constexpr (PHASE == PH_MATERIALISE) {
        if (T.rep[s] == me) {  // one writer per slot
          uint32_t* k = T.key + (size_t)s * LK_KEY_WORDS;
          *reinterpret_cast<uint4*>(k) = make_uint4(key[0], key[1], key[2], key[3]);
          *reinterpret_cast<uint4*>(k + 4) = make_uint4(key[4], key[5], key[6], key[7]);
          T.aux[s] = round;
        }
      } else {  // PH_ACCOUNT
        if (T.aux[s] != round) {
          err |= LK_ERR_STATE;
          return;
        }
        if (!lk_key_equal(T.key + (size_t)s * LK_KEY_WORDS, key)) {
          unresolved++;  // another key of this tag took the slot: next round
          return;
        }
        constexpr int kind = LookupsOf<CHIP>::v.l[J].kind;
        if (combine && (kind == K_BYTE || kind == K_PROGRAM)) {
          const uint32_t ch = ((uint32_t)s * 2654435761u) >> (32 - LK_CACHE_LOG);
          const uint32_t old = atomicCAS(&c_slot[ch], LK_NO_SLOT, (uint32_t)s);
          if (old == LK_NO_SLOT || old == (uint32_t)s) {
            atomicAdd(&c_sum[ch], add);
            return;
          }
        }
        atomicAdd(&T.net[s], add);
        if (!(T.mask[s] & chip_bit)) atomicOr(&T.mask[s], chip_bit);
      }
    });
  }
  if constexpr (PHASE == PH_ACCOUNT) {
    __syncthreads();
    for (int h = threadIdx.x; h < LK_CACHE; h += blockDim.x) {
      const uint32_t s = c_slot[h];
      if (s == LK_NO_SLOT) continue;
      if (c_sum[h]) atomicAdd(&T.net[s], c_sum[h]);
      if (!(T.mask[s] & chip_bit)) atomicOr(&T.mask[s], chip_bit);
    }
    lk_block_add(unresolved, &ctl->unresolved, sh4);
    lk_block_add(unresolved, &ctl->collisions, sh4);
  }
  if constexpr (PHASE == PH_COUNT) lk_block_add(counted, &ctl->interactions, sh4);
  if (err) atomicOr(&ctl->error, err);
}

// Over the slots: distinct keys, per-chip distinct keys, the sum of the nets and the number of
// keys whose net is not 0 mod p (one atomic per block and counter).
__global__ __launch_bounds__(256) void k_lookup_scan(LkTable T, LkCtl* __restrict__ ctl) {
  __shared__ unsigned long long sh4[4];
  const size_t size = (size_t)1 << T.logsize;
  unsigned long long distinct = 0, unbalanced = 0, total = 0, per_chip[NUM_CHIPS] = {};
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < size;
       i += (size_t)gridDim.x * blockDim.x) {
    if (T.tag[i] == 0) continue;
    distinct++;
    const uint32_t m = T.mask[i];
#pragma unroll
    for (int c = 0; c < NUM_CHIPS; c++) per_chip[c] += (m >> c) & 1u;
    const long long net = (long long)T.net[i];
    total += (unsigned long long)net;
    if (net % (long long)P != 0) unbalanced++;
  }
  lk_block_add(distinct, &ctl->distinct, sh4);
  lk_block_add(unbalanced, &ctl->unbalanced, sh4);
  lk_block_add(total, &ctl->total, sh4);
#pragma unroll
  for (int c = 0; c < NUM_CHIPS; c++) lk_block_add(per_chip[c], &ctl->chip_distinct[c], sh4);
}

// The unbalanced slots as records of 14 words: slot, pad, net (2), representative (2), key (8).
// A cursor hands out the positions; the host sorts.
constexpr int LK_REC_WORDS = 14;
__global__ __launch_bounds__(256) void k_lookup_collect(LkTable T, LkCtl* __restrict__ ctl,
                                                        uint32_t* __restrict__ recs,
                                                        unsigned long long cap) {
  const size_t size = (size_t)1 << T.logsize;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < size;
       i += (size_t)gridDim.x * blockDim.x) {
    if (T.tag[i] == 0) continue;
    const unsigned long long net = T.net[i];
    if ((long long)net % (long long)P == 0) continue;
    const unsigned long long at = atomicAdd(&ctl->cursor, 1ull);
    if (at >= cap) continue;
    uint32_t* r = recs + at * LK_REC_WORDS;
    const unsigned long long rep = T.rep[i];
    r[0] = (uint32_t)i;
    r[1] = 0;
    r[2] = (uint32_t)net;
    r[3] = (uint32_t)(net >> 32);
    r[4] = (uint32_t)rep;
    r[5] = (uint32_t)(rep >> 32);
#pragma unroll
    for (int k = 0; k < LK_KEY_WORDS; k++) r[6 + k] = T.key[i * LK_KEY_WORDS + k];
  }
}

// aux[slots[k]] = k + 1 for the records the caller keeps (aux was cleared).
__global__ __launch_bounds__(256) void k_lookup_mark(LkTable T, const uint32_t* __restrict__ slots,
                                                     uint32_t nsel) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < nsel) T.aux[slots[k] & ((1u << T.logsize) - 1)] = k + 1;
}

namespace {
template <int CHIP, int PHASE>
void launch_phase(const uint32_t* mainc, const uint32_t* prepc, size_t h, unsigned kinds_mask,
                  unsigned long long hash_mask, uint32_t round, const LkTable& T, LkCtl* ctl,
                  unsigned long long* share_net, uint32_t* share_count, hipStream_t st) {
  // BFZ_LOOKUP_COMBINE=0: every account goes to HBM, no per-block LDS table (A/B of DESIGN.md)
  static const uint32_t combine = [] {
    const char* e = std::getenv("BFZ_LOOKUP_COMBINE");
    return (e && e[0] == '0' && !e[1]) ? 0u : 1u;
  }();
  const int nblocks = (int)std::min<size_t>(ceil_div(h, 256), LK_MAX_BLOCKS);
  hipLaunchKernelGGL((k_lookup<CHIP, PHASE>), dim3(nblocks), dim3(256), 0, st, mainc, prepc,
                     (uint32_t)h, log2i(h), kinds_mask, hash_mask, round, combine, T, ctl, share_net,
                     share_count);
  KCHECK();
}

template <int PHASE>
void launch_chip(int chip, const uint32_t* mainc, const uint32_t* prepc, size_t h,
                 unsigned kinds_mask, unsigned long long hash_mask, uint32_t round, const LkTable& T,
                 LkCtl* ctl, unsigned long long* share_net, uint32_t* share_count, hipStream_t st) {
#define BFZ_LK_CASE(C)                                                                          \
  case C:                                                                                       \
    launch_phase<C, PHASE>(mainc, prepc, h, kinds_mask, hash_mask, round, T, ctl, share_net,    \
                           share_count, st);                                                    \
    break;
  switch (chip) {
    BFZ_LK_CASE(CHIP_CPU)
    BFZ_LK_CASE(CHIP_PROGRAM)
    BFZ_LK_CASE(CHIP_ADDSUB)
    BFZ_LK_CASE(CHIP_JUMP)
    BFZ_LK_CASE(CHIP_MEMORY)
    BFZ_LK_CASE(CHIP_BYTE)
    BFZ_LK_CASE(CHIP_MEMINSTRS)
    BFZ_LK_CASE(CHIP_IO)
  }
#undef BFZ_LK_CASE
}

LkCtl fetch_ctl(const LkCtl* ctl_d, hipStream_t st) {
  LkCtl c;
  HIP_CHECK(hipMemcpyAsync(&c, ctl_d, sizeof c, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  if (c.error & LK_ERR_FULL) throw std::runtime_error("debug_interactions: the aggregation table is full");
  if (c.error) throw std::runtime_error("debug_interactions: inconsistent aggregation table");
  return c;
}
}  // namespace

void debug_interactions_device(const ProvingKey& pk, const DeviceTraces& dt, unsigned kinds_mask,
                               size_t cap, bool low_hash_bits, LookupReport& out) {
  check_kinds_mask(kinds_mask);
  check_tables();
  hipStream_t st = stream();
  const int nc = (int)dt.chips.size();
  if (nc == 0 || nc > NUM_CHIPS) throw std::runtime_error("debug_interactions: no traces");
  std::vector<int> ord(nc);  // machine order (debug.rs:139-144); the result does not depend on it
  std::iota(ord.begin(), ord.end(), 0);
  std::sort(ord.begin(), ord.end(), [&](int a, int b) { return dt.chips[a] < dt.chips[b]; });
  std::vector<const uint32_t*> preps(nc, nullptr);
  for (int k = 0; k < nc; k++) {
    const int c = dt.chips[ord[k]];
    const size_t h = dt.heights[ord[k]];
    if (c < 0 || c >= NUM_CHIPS) throw std::runtime_error("debug_interactions: bad chip index");
    if (h < 1 || (h & (h - 1)) || h > ((size_t)1 << 23))
      throw std::runtime_error("debug_interactions: height not a power of two in [1, 2^23]");
    const int pi = pk.idx_of_chip[c];
    if (pi >= 0) {  // the key's preprocessed trace has the program's height (machine.rs:309-312)
      if (pk.prep.mats[pi].n != h)
        throw std::runtime_error(std::string("debug_constraints: height of ") + CHIP_INFO[c].name +
                                 " differs from its preprocessed trace");
      preps[k] = pk.prep_evals[pi].p;
    }
  }
  const unsigned long long hash_mask = low_hash_bits ? 0xFFFull : ~0ull;
  out = LookupReport();

  DBuf<LkCtl> ctl(1);
  HIP_CHECK(hipMemsetAsync(ctl.p, 0, sizeof(LkCtl), st));
  LkTable T{};
  auto each_chip = [&](auto phase, uint32_t round, unsigned long long* share_net, uint32_t* share_count) {
    for (int k = 0; k < nc; k++)
      launch_chip<decltype(phase)::value>(dt.chips[ord[k]], dt.evals[ord[k]].p, preps[k],
                                          dt.heights[ord[k]], kinds_mask, hash_mask, round, T, ctl.p,
                                          share_net, share_count, st);
  };
  // the non-zero interactions: the report's count and the table's size
  each_chip(std::integral_constant<int, PH_COUNT>{}, 0, nullptr, nullptr);
  out.interactions = fetch_ctl(ctl.p, st).interactions;
  if (out.interactions == 0) {
    out.balanced = true;
    return;
  }
  if (out.interactions > ((uint64_t)1 << 30))
    throw std::runtime_error("debug_interactions: more than 2^30 interactions");
  T.logsize = 10;
  while (((uint64_t)1 << T.logsize) < out.interactions + out.interactions / 4) T.logsize++;
  const size_t size = (size_t)1 << T.logsize;
  const size_t slot_bytes = 8 + 8 + 8 + 4 + 4 + 4 * LK_KEY_WORDS;
  out.table_bytes = size * slot_bytes;
  DBuf<unsigned long long> wide;  // tag | net | rep
  DBuf<uint32_t> narrow;          // mask | aux | key
  try {
    wide.reset(3 * size);
    narrow.reset((2 + LK_KEY_WORDS) * size);
  } catch (const HipError&) {
    (void)hipGetLastError();
    throw std::runtime_error("debug_interactions: not enough device memory for the aggregation table (" +
                             std::to_string(out.table_bytes) + " bytes needed for " +
                             std::to_string(out.interactions) + " interactions)");
  }
  T.tag = wide.p;
  T.net = wide.p + size;
  T.rep = wide.p + 2 * size;
  T.mask = narrow.p;
  T.aux = narrow.p + size;
  T.key = narrow.p + 2 * size;
  HIP_CHECK(hipMemsetAsync(T.tag, 0, 2 * size * 8, st));     // tag, net
  HIP_CHECK(hipMemsetAsync(T.rep, 0xFF, size * 8, st));
  HIP_CHECK(hipMemsetAsync(T.mask, 0, 2 * size * 4, st));    // mask, aux

  for (uint32_t round = 1;; round++) {
    if (round > LK_MAX_ROUNDS)
      throw std::runtime_error("debug_interactions: keys still unresolved after " +
                               std::to_string(LK_MAX_ROUNDS) + " rounds");
    HIP_CHECK(hipMemsetAsync(&ctl.p->unresolved, 0, 8, st));
    each_chip(std::integral_constant<int, PH_CLAIM>{}, round, nullptr, nullptr);
    each_chip(std::integral_constant<int, PH_MATERIALISE>{}, round, nullptr, nullptr);
    each_chip(std::integral_constant<int, PH_ACCOUNT>{}, round, nullptr, nullptr);
    const LkCtl c = fetch_ctl(ctl.p, st);
    out.rounds = round;
    out.tag_collisions = (uint32_t)std::min<unsigned long long>(c.collisions, 0xFFFFFFFFull);
    if (c.unresolved == 0) break;
  }

  const int scan_blocks = (int)std::min<size_t>(ceil_div(size, 256), LK_MAX_BLOCKS);
  hipLaunchKernelGGL(k_lookup_scan, dim3(scan_blocks), dim3(256), 0, st, T, ctl.p);
  KCHECK();
  const LkCtl c = fetch_ctl(ctl.p, st);
  out.distinct_keys = c.distinct;
  out.unbalanced_keys = c.unbalanced;
  for (int k = 0; k < NUM_CHIPS; k++) out.chip_distinct[k] = c.chip_distinct[k];
  out.total_net = net_to_int((long long)c.total);
  out.balanced = c.unbalanced == 0;
  if (c.unbalanced == 0 || cap == 0) return;

  // every unbalanced key comes to the host, which orders them and keeps the first `cap`
  const size_t nrec = (size_t)c.unbalanced;
  DBuf<uint32_t> recs_d(nrec * LK_REC_WORDS);
  hipLaunchKernelGGL(k_lookup_collect, dim3(scan_blocks), dim3(256), 0, st, T, ctl.p, recs_d.p,
                     (unsigned long long)nrec);
  KCHECK();
  std::vector<uint32_t> recs(nrec * LK_REC_WORDS);
  HIP_CHECK(hipMemcpyAsync(recs.data(), recs_d.p, recs.size() * 4, hipMemcpyDeviceToHost, st));
  if (fetch_ctl(ctl.p, st).cursor != nrec)
    throw std::runtime_error("debug_interactions: inconsistent aggregation table");
  std::vector<size_t> idx(nrec);
  std::iota(idx.begin(), idx.end(), 0);
  auto key_less = [&](size_t a, size_t b) {
    return std::lexicographical_compare(&recs[a * LK_REC_WORDS + 6], &recs[a * LK_REC_WORDS + 14],
                                        &recs[b * LK_REC_WORDS + 6], &recs[b * LK_REC_WORDS + 14]);
  };
  const size_t nsel = std::min(nrec, cap);
  std::partial_sort(idx.begin(), idx.begin() + nsel, idx.end(), key_less);
  if (nsel > 0xFFFFFFF0u) throw std::runtime_error("debug_interactions: cap too large");

  // the chips' shares of the kept keys: one more pass over the interactions
  std::vector<uint32_t> slots(nsel);
  for (size_t k = 0; k < nsel; k++) slots[k] = recs[idx[k] * LK_REC_WORDS];
  DBuf<uint32_t> slots_d(nsel), share_count(nsel * NUM_CHIPS);
  DBuf<unsigned long long> share_net(nsel * NUM_CHIPS);
  HIP_CHECK(hipMemcpyAsync(slots_d.p, slots.data(), nsel * 4, hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemsetAsync(T.aux, 0, size * 4, st));
  HIP_CHECK(hipMemsetAsync(share_count.p, 0, nsel * NUM_CHIPS * 4, st));
  HIP_CHECK(hipMemsetAsync(share_net.p, 0, nsel * NUM_CHIPS * 8, st));
  hipLaunchKernelGGL(k_lookup_mark, dim3(ceil_div(nsel, 256)), dim3(256), 0, st, T,
                     (const uint32_t*)slots_d.p, (uint32_t)nsel);
  KCHECK();
  each_chip(std::integral_constant<int, PH_SHARES>{}, 0, share_net.p, share_count.p);
  std::vector<unsigned long long> snet(nsel * NUM_CHIPS);
  std::vector<uint32_t> scount(nsel * NUM_CHIPS);
  HIP_CHECK(hipMemcpyAsync(snet.data(), share_net.p, snet.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(scount.data(), share_count.p, scount.size() * 4, hipMemcpyDeviceToHost, st));
  (void)fetch_ctl(ctl.p, st);

  out.recs.resize(nsel);
  for (size_t k = 0; k < nsel; k++) {
    const uint32_t* r = &recs[idx[k] * LK_REC_WORDS];
    LookupDiscrepancy& d = out.recs[k];
    LkKey key;
    std::memcpy(key.data(), r + 6, 4 * LK_KEY_WORDS);
    fill_record(key, d);
    d.net = net_to_int((long long)((unsigned long long)r[2] | ((unsigned long long)r[3] << 32)));
    const unsigned long long rep = (unsigned long long)r[4] | ((unsigned long long)r[5] << 32);
    d.first_chip = (int)(rep >> 32);
    d.first_row = (int64_t)((rep & 0xFFFFFFFFull) >> 4);
    d.first_interaction = (int)(rep & 15);
    for (int c = 0; c < NUM_CHIPS; c++) {
      d.chip_net[c] = net_to_int((long long)snet[k * NUM_CHIPS + c]);
      d.chip_count[c] = scount[k * NUM_CHIPS + c];
    }
  }
}

}  // namespace bfz
