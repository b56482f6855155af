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
#include "lookup_debug_dev.h"

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

// k_lookup_scan for a run-time chip count (up to the 32 bits of the mask): the per-chip counters
// are a block's LDS words, one LDS atomic per set bit of a slot's mask -- a register array
// indexed by the bit would go to scratch -- and come out in chip_distinct[nchips], not in ctl.
__global__ __launch_bounds__(256) void k_lookup_scan_n(LkTable T, LkCtl* __restrict__ ctl,
                                                       unsigned long long* __restrict__ chip_distinct,
                                                       uint32_t nchips) {
  __shared__ unsigned long long sh4[4];
  __shared__ unsigned long long per_chip[32];
  if (threadIdx.x < 32) per_chip[threadIdx.x] = 0;
  __syncthreads();
  const size_t size = (size_t)1 << T.logsize;
  unsigned long long distinct = 0, unbalanced = 0, total = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < size;
       i += (size_t)gridDim.x * blockDim.x) {
    if (T.tag[i] == 0) continue;
    distinct++;
    for (uint32_t m = T.mask[i]; m; m &= m - 1) atomicAdd(&per_chip[__ffs(m) - 1], 1ull);
    const long long net = (long long)T.net[i];
    total += (unsigned long long)net;
    if (net % (long long)P != 0) unbalanced++;
  }
  lk_block_add(distinct, &ctl->distinct, sh4);
  lk_block_add(unbalanced, &ctl->unbalanced, sh4);
  lk_block_add(total, &ctl->total, sh4);  // (its barriers order the LDS atomics above)
  if (threadIdx.x < nchips && per_chip[threadIdx.x])
    atomicAdd(&chip_distinct[threadIdx.x], per_chip[threadIdx.x]);
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
                  const LkPass& p) {
  const int nblocks = (int)std::min<size_t>(ceil_div(h, 256), LK_MAX_BLOCKS);
  hipLaunchKernelGGL((k_lookup<CHIP, PHASE>), dim3(nblocks), dim3(256), 0, p.st, mainc, prepc,
                     (uint32_t)h, log2i(h), kinds_mask, p.hash_mask, p.round, p.combine, p.T, p.ctl,
                     p.share_net, p.share_count);
  KCHECK();
}

template <int CHIP>
void launch_chip(const uint32_t* mainc, const uint32_t* prepc, size_t h, unsigned kinds_mask,
                 const LkPass& p) {
  switch (p.phase) {
    case PH_COUNT: launch_phase<CHIP, PH_COUNT>(mainc, prepc, h, kinds_mask, p); break;
    case PH_CLAIM: launch_phase<CHIP, PH_CLAIM>(mainc, prepc, h, kinds_mask, p); break;
    case PH_MATERIALISE: launch_phase<CHIP, PH_MATERIALISE>(mainc, prepc, h, kinds_mask, p); break;
    case PH_ACCOUNT: launch_phase<CHIP, PH_ACCOUNT>(mainc, prepc, h, kinds_mask, p); break;
    case PH_SHARES: launch_phase<CHIP, PH_SHARES>(mainc, prepc, h, kinds_mask, p); break;
  }
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

int32_t lk_net_to_int(long long net) { return net_to_int(net); }

// The rounds driver (lookup_debug_dev.h).  out.recs get the key, the net and the witness; the
// chips' shares and distinct-key counts go to sh, d.stride words per record.
void lk_aggregate(const LkDriver& d, size_t cap, bool low_hash_bits, LookupReport& out, LkShares& sh) {
  // BFZ_LOOKUP_COMBINE=0: every account goes to HBM, no per-block LDS table (A/B of DESIGN.md)
  static const uint32_t combine = [] {
    const char* e = std::getenv("BFZ_LOOKUP_COMBINE");
    return (e && e[0] == '0' && !e[1]) ? 0u : 1u;
  }();
  hipStream_t st = stream();
  const size_t stride = (size_t)d.stride;
  out = LookupReport();
  sh = LkShares();
  sh.chip_distinct.assign(stride, 0);

  DBuf<LkCtl> ctl(1);
  HIP_CHECK(hipMemsetAsync(ctl.p, 0, sizeof(LkCtl), st));
  LkPass pass{PH_COUNT, 0, low_hash_bits ? 0xFFFull : ~0ull, combine, LkTable{}, ctl.p, nullptr, nullptr, st};
  auto each_chip = [&](int phase, uint32_t round) {
    pass.phase = phase;
    pass.round = round;
    for (int k = 0; k < d.nchips; k++) d.launch(k, pass);
  };
  // the non-zero interactions: the report's count and the table's size
  each_chip(PH_COUNT, 0);
  out.interactions = fetch_ctl(ctl.p, st).interactions;
  if (out.interactions == 0) {
    out.balanced = true;
    return;
  }
  if (out.interactions > ((uint64_t)1 << 30))
    throw std::runtime_error("debug_interactions: more than 2^30 interactions");
  LkTable& T = pass.T;
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
    each_chip(PH_CLAIM, round);
    each_chip(PH_MATERIALISE, round);
    each_chip(PH_ACCOUNT, round);
    const LkCtl c = fetch_ctl(ctl.p, st);
    out.rounds = round;
    out.tag_collisions = (uint32_t)std::min<unsigned long long>(c.collisions, 0xFFFFFFFFull);
    if (c.unresolved == 0) break;
  }

  const int scan_blocks = (int)std::min<size_t>(ceil_div(size, 256), LK_MAX_BLOCKS);
  DBuf<unsigned long long> distinct_d;
  if (d.runtime_stride) {
    distinct_d.reset(stride);
    HIP_CHECK(hipMemsetAsync(distinct_d.p, 0, stride * 8, st));
    hipLaunchKernelGGL(k_lookup_scan_n, dim3(scan_blocks), dim3(256), 0, st, T, ctl.p, distinct_d.p,
                       (uint32_t)stride);
    KCHECK();
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "chip_distinct words");
    HIP_CHECK(hipMemcpyAsync(sh.chip_distinct.data(), distinct_d.p, stride * 8, hipMemcpyDeviceToHost, st));
  } else {
    hipLaunchKernelGGL(k_lookup_scan, dim3(scan_blocks), dim3(256), 0, st, T, ctl.p);
    KCHECK();
  }
  const LkCtl c = fetch_ctl(ctl.p, st);
  out.distinct_keys = c.distinct;
  out.unbalanced_keys = c.unbalanced;
  if (!d.runtime_stride)
    for (int k = 0; k < NUM_CHIPS; k++) sh.chip_distinct[k] = c.chip_distinct[k];
  out.total_net = net_to_int((long long)c.total);
  out.balanced = c.unbalanced == 0;
  if (d.after_rounds) d.after_rounds(pass);
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
  DBuf<uint32_t> slots_d(nsel), share_count(nsel * stride);
  DBuf<unsigned long long> share_net(nsel * stride);
  HIP_CHECK(hipMemcpyAsync(slots_d.p, slots.data(), nsel * 4, hipMemcpyHostToDevice, st));
  HIP_CHECK(hipMemsetAsync(T.aux, 0, size * 4, st));
  HIP_CHECK(hipMemsetAsync(share_count.p, 0, nsel * stride * 4, st));
  HIP_CHECK(hipMemsetAsync(share_net.p, 0, nsel * stride * 8, st));
  hipLaunchKernelGGL(k_lookup_mark, dim3(ceil_div(nsel, 256)), dim3(256), 0, st, T,
                     (const uint32_t*)slots_d.p, (uint32_t)nsel);
  KCHECK();
  pass.share_net = share_net.p;
  pass.share_count = share_count.p;
  each_chip(PH_SHARES, 0);
  std::vector<unsigned long long> snet(nsel * stride);
  sh.count.resize(nsel * stride);
  HIP_CHECK(hipMemcpyAsync(snet.data(), share_net.p, snet.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(sh.count.data(), share_count.p, sh.count.size() * 4, hipMemcpyDeviceToHost, st));
  (void)fetch_ctl(ctl.p, st);
  sh.net.assign(snet.begin(), snet.end());

  out.recs.resize(nsel);
  for (size_t k = 0; k < nsel; k++) {
    const uint32_t* r = &recs[idx[k] * LK_REC_WORDS];
    LookupDiscrepancy& dr = out.recs[k];
    LkKey key;
    std::memcpy(key.data(), r + 6, 4 * LK_KEY_WORDS);
    fill_record(key, dr);
    dr.net = net_to_int((long long)((unsigned long long)r[2] | ((unsigned long long)r[3] << 32)));
    const unsigned long long rep = (unsigned long long)r[4] | ((unsigned long long)r[5] << 32);
    dr.first_chip = (int)(rep >> 32);
    dr.first_row = (int64_t)((rep & 0xFFFFFFFFull) >> d.rep_bits);
    dr.first_interaction = (int)(rep & ((1u << d.rep_bits) - 1));
  }
}

void debug_interactions_device(const ProvingKey& pk, const DeviceTraces& dt, unsigned kinds_mask,
                               size_t cap, bool low_hash_bits, LookupReport& out) {
  check_kinds_mask(kinds_mask);
  check_tables();
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
  LkDriver d;
  d.nchips = nc;
  d.stride = NUM_CHIPS;
  d.runtime_stride = false;
  d.rep_bits = 4;
  d.launch = [&](int k, const LkPass& p) {
    const uint32_t* mainc = dt.evals[ord[k]].p;
    const size_t h = dt.heights[ord[k]];
#define BFZ_LK_CASE(C) \
  case C: launch_chip<C>(mainc, preps[k], h, kinds_mask, p); break;
    switch (dt.chips[ord[k]]) {
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
  };
  LkShares sh;
  lk_aggregate(d, cap, low_hash_bits, out, sh);
  for (int k = 0; k < NUM_CHIPS; k++) out.chip_distinct[k] = sh.chip_distinct[k];
  for (size_t r = 0; r < out.recs.size(); r++)
    for (int c = 0; c < NUM_CHIPS; c++) {
      out.recs[r].chip_net[c] = net_to_int(sh.net[r * NUM_CHIPS + c]);
      out.recs[r].chip_count[c] = sh.count[r * NUM_CHIPS + c];
    }
}

}  // namespace bfz
