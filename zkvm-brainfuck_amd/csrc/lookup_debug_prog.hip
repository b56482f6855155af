// Per-key lookup discrepancies and multiplicity columns for chips that are data
// (lookup_debug.h): k_lookup_prog<PHASE> does for a compiled interaction list
// (lookup_program.h) what k_lookup<CHIP, PHASE> does for LookupsOf<CHIP>, into the same table
// and under the same rounds protocol (lookup_debug.hip's header; helpers and driver in
// lookup_debug_dev.h): open addressing with 64-bit tags, the representative chosen by atomicMin,
// one key settled per slot per round, integer atomics only, every probe bounded.
//
// Design decisions:
//   Work split.  One row (storage position) per thread with a grid stride, at most LK_MAX_BLOCKS
//     blocks, as k_lookup.  The list is read through the constant address space, so every read
//     is a scalar load and every loop over interactions, values and terms is wave-uniform; the
//     position in the list is one scalar register per wave.
//   The debug list.  The host does not hand the kernel LookupProgram::list but a list made from
//     it: only the interactions of the selected kinds (the kernel has no kind filter), each with
//     a header of two pairs,
//         (n_values | send << 8 | chain index << 16,  canonical kind << 8 | n_values)
//         (word offset of the next interaction,       0)
//     then the multiplicity VCOL and the value VCOLs as compiled.  The second word is the key's
//     first word, ready; the chain index is what the representative carries, so
//     first_interaction is the index in the program whatever was selected; the offset lets a wave
//     leave an interaction without walking its VCOLs.
//   Evaluation order.  The multiplicity first.  A wave all of whose rows have multiplicity 0
//     (padding) jumps to the next interaction; otherwise the values are evaluated by every lane
//     -- the list position must stay uniform -- and a lane with multiplicity 0 takes no part in
//     the probe (debug.rs:94).  The key is 8 registers: the loop over the 7 value slots is
//     unrolled and slot v is filled under the uniform condition v < n_values, so no index into
//     the key survives as a run-time value.
//   The row is not held.  The widths are run-time values and a run-time-indexed register array
//     would go to scratch; a term is one buffer load of its column at the thread's position
//     (vcol of lookup_program_dev.h).  A block's loads of one column are 1 KiB, contiguous, and
//     columns shared by several interactions are served by L1 / L2.
//   Representative.  chip << 32 | row << 5 | chain index: BFZ_LOOKUPS_MAX is 32, rows stay
//     below 2^23, so the low word has 28 bits; the chip is the position in the caller's arrays.
//   Hot keys.  k_lookup combines in LDS only the Byte and Program kinds, which it knows when it
//     is compiled.  Here a kind is a number the caller chose.  The choice is to combine EVERY
//     interaction in the per-block LDS table (slot -> partial sum, 2048 entries, 24 KiB), not a
//     per-interaction flag set by the host: the host sees the programs, not the traces, and
//     cannot know which kind is hot, while an entry of the LDS table that is taken by another
//     slot costs one LDS compare-and-swap before the same global atomic.  DESIGN.md records the
//     measurement against BFZ_LOOKUP_COMBINE=0.  The partial sums are 64-bit signed (two's
//     complement) like the nets: 2^23 rows of multiplicity p/2 are below 2^53.
//   Chip count.  Up to 32 chips, the width of a slot's mask; the share arrays have a run-time
//     stride and the scan is k_lookup_scan_n (lookup_debug.hip).  k_lookup_collect and
//     k_lookup_mark serve as they are.
//   No scratch; occupancy is bounded by the registers of the probe loops, as in k_lookup.
//
// The multiplicity kernels run after the senders' rounds, over the rows of a table chip and one
// of its interactions (normally its receive), whose multiplicity VCOL is not read:
//   k_mult_claim  the row's key, its slot by a probe that does not fail (a table row nobody
//                 sent to is normal), the slot kept per row, and atomicMin of the row into the
//                 slot's aux word, which the rounds no longer need (set to all ones before).  The
//                 representative word keeps the senders' witness, which the report of an unmatched
//                 key needs.
//   k_mult_write  mult[row] = the slot's net mod p as a Montgomery word if the row is the slot's
//                 smallest, else 0: duplicate table keys give the first row everything.
//   k_mult_scan   the slots no table row claimed: their count, and per block the smallest key in
//                 (kind, values) order (a lexicographic minimum over 8 words by wave shuffles);
//                 the host takes the smallest of the blocks'.
//
// These kernels are not part of a proof and are NOT in a PreloadKernels list.
#include <algorithm>
#include <cstring>
#include <map>

#include "lookup_debug_dev.h"
#include "lookup_program_dev.h"
#include "uni_stark.h"

namespace bfz {

using namespace kb;

namespace {
constexpr int LKD_HEAD = 1;         // words before the first interaction: the count
constexpr int LKD_REP_BITS = 5;     // BFZ_LOOKUPS_MAX = 32 chain indices
constexpr int LKD_MREC_WORDS = 14;  // k_mult_scan's block record: found, slot, net, rep, key
static_assert(BFZ_LOOKUPS_MAX <= (1 << LKD_REP_BITS), "the representative's interaction bits");

// The value VCOLs of the interaction whose header was read: key[1 ..] canonical, unused entries 0.
__device__ __forceinline__ void lkd_values(const RowCtx& c, int& at, int nv,
                                           uint32_t (&key)[LK_KEY_WORDS]) {
#pragma unroll
  for (int v = 0; v < LK_MAX_VALUES; v++) key[1 + v] = v < nv ? from_mont(vcol(c, at)) : 0u;
}
}  // namespace

// list: the debug list; mainc / prepc: column-major bit-reversed traces of n rows; chip: the
// position in the caller's arrays; nchips: the stride of the share arrays.
template <int PHASE>
__global__ __launch_bounds__(256) void k_lookup_prog(const uint32_t* __restrict__ list,
                                                     const uint32_t* __restrict__ mainc,
                                                     const uint32_t* __restrict__ prepc, uint32_t n,
                                                     int logn, uint32_t chip, uint32_t nchips,
                                                     unsigned long long hash_mask, uint32_t round,
                                                     uint32_t combine, LkTable T,
                                                     LkCtl* __restrict__ ctl,
                                                     unsigned long long* __restrict__ share_net,
                                                     uint32_t* __restrict__ share_count) {
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
  const uint32_t chip_bit = 1u << chip;
  const int ni = (int)((ConstWords)list)[0];
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
    const RowCtx c{(ConstWords)list, nullptr, mainc, prepc, n, t * 4u};
    const uint32_t row = dbitrev(t, logn);  // natural row of storage position t
    int at = LKD_HEAD;
    for (int i = 0; i < ni; i++) {
      const uint32_t head = c.list[at], key0 = c.list[at + 1];
      const int next = (int)c.list[at + 2];
      at += 4;
      const uint32_t mu = vcol(c, at);
      if constexpr (PHASE == PH_COUNT) {
        counted += mu != 0;
        at = next;
        continue;
      }
      if (__ballot(mu != 0) == 0) {  // wave-uniform: padding rows
        at = next;
        continue;
      }
      uint32_t key[LK_KEY_WORDS];
      key[0] = key0;
      lkd_values(c, at, (int)(head & 0xff), key);
      at = next;
      if (mu == 0) continue;  // debug.rs:94
      const int32_t x = field_to_int(from_mont(mu));
      const unsigned long long add = (unsigned long long)(long long)((head >> 8) & 1 ? x : -x);
      const unsigned long long h = lk_hash(key) & hash_mask;
      const unsigned long long tag = h | (1ull << 63);
      const uint32_t home = (uint32_t)((h * 0x9E3779B97F4A7C15ull) >> (64 - T.logsize));
      const unsigned long long me = ((unsigned long long)chip << 32) |
                                    ((unsigned long long)row << LKD_REP_BITS) | ((head >> 16) & 31u);
      if constexpr (PHASE == PH_SHARES) {
        const int s = lk_find(T, key, tag, home, err);
        if (s < 0) continue;
        const uint32_t sel = T.aux[s];
        if (sel) {
          atomicAdd(&share_net[(size_t)(sel - 1) * nchips + chip], add);
          atomicAdd(&share_count[(size_t)(sel - 1) * nchips + chip], 1u);
        }
        continue;
      }
      bool resolved;
      const int s = PHASE == PH_CLAIM ? lk_walk<true>(T, key, tag, home, round, resolved, err)
                                      : lk_walk<false>(T, key, tag, home, round, resolved, err);
      if (s < 0 || resolved) continue;
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
          continue;
        }
        if (!lk_key_equal(T.key + (size_t)s * LK_KEY_WORDS, key)) {
          unresolved++;  // another key of this tag took the slot: next round
          continue;
        }
        if (combine) {
          const uint32_t ch = ((uint32_t)s * 2654435761u) >> (32 - LK_CACHE_LOG);
          const uint32_t old = atomicCAS(&c_slot[ch], LK_NO_SLOT, (uint32_t)s);
          if (old == LK_NO_SLOT || old == (uint32_t)s) {
            atomicAdd(&c_sum[ch], add);
            continue;
          }
        }
        atomicAdd(&T.net[s], add);
        if (!(T.mask[s] & chip_bit)) atomicOr(&T.mask[s], chip_bit);
      }
    }
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

// list: a debug list of ONE interaction of the table chip.  slot_of[t] = the slot of the key of
// storage position t, or LK_NO_SLOT; aux[slot] = the smallest natural row that holds its key.
__global__ __launch_bounds__(256) void k_mult_claim(const uint32_t* __restrict__ list,
                                                    const uint32_t* __restrict__ mainc,
                                                    const uint32_t* __restrict__ prepc, uint32_t n,
                                                    int logn, unsigned long long hash_mask, LkTable T,
                                                    uint32_t* __restrict__ slot_of) {
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
    const RowCtx c{(ConstWords)list, nullptr, mainc, prepc, n, t * 4u};
    int at = LKD_HEAD;
    const uint32_t head = c.list[at], key0 = c.list[at + 1];
    at += 4;
    at += 2 + 2 * (int)c.list[at + 1];  // the multiplicity VCOL is not read
    uint32_t key[LK_KEY_WORDS];
    key[0] = key0;
    lkd_values(c, at, (int)(head & 0xff), key);
    const unsigned long long h = lk_hash(key) & hash_mask;
    const uint32_t home = (uint32_t)((h * 0x9E3779B97F4A7C15ull) >> (64 - T.logsize));
    const int s = lk_find_opt(T, key, h | (1ull << 63), home);
    slot_of[t] = s < 0 ? LK_NO_SLOT : (uint32_t)s;
    if (s >= 0) atomicMin(&T.aux[s], dbitrev(t, logn));
  }
}

// mult: natural row order, Montgomery words.
__global__ __launch_bounds__(256) void k_mult_write(uint32_t n, int logn, LkTable T,
                                                    const uint32_t* __restrict__ slot_of,
                                                    uint32_t* __restrict__ mult) {
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
    const uint32_t s = slot_of[t], row = dbitrev(t, logn);
    uint32_t v = 0;
    if (s != LK_NO_SLOT && T.aux[s] == row) {
      long long r = (long long)T.net[s] % (long long)P;
      if (r < 0) r += P;
      v = to_mont((uint32_t)r);
    }
    mult[row] = v;
  }
}

// recs: LKD_MREC_WORDS per block: found, slot, net (2), representative (2), key (8) of the block's
// smallest unclaimed key; *unmatched: the number of unclaimed slots.
__global__ __launch_bounds__(256) void k_mult_scan(LkTable T, unsigned long long* __restrict__ unmatched,
                                                   uint32_t* __restrict__ recs) {
  __shared__ unsigned long long sh4[4];
  __shared__ uint32_t best_sh[4][LK_KEY_WORDS + 1];
  const size_t size = (size_t)1 << T.logsize;
  uint32_t best[LK_KEY_WORDS + 1];  // the key, then its slot; all ones = none
#pragma unroll
  for (int k = 0; k <= LK_KEY_WORDS; k++) best[k] = 0xFFFFFFFFu;
  // a < b over the 8 key words (a real key's first word is below 2^32 - 1)
  auto less = [](const uint32_t (&a)[LK_KEY_WORDS + 1], const uint32_t (&b)[LK_KEY_WORDS + 1]) {
    bool lt = false, decided = false;
#pragma unroll
    for (int k = 0; k < LK_KEY_WORDS; k++) {
      lt = decided ? lt : a[k] < b[k];
      decided = decided || a[k] != b[k];
    }
    return lt;
  };
  unsigned long long count = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < size;
       i += (size_t)gridDim.x * blockDim.x) {
    if (T.tag[i] == 0 || T.aux[i] != 0xFFFFFFFFu) continue;
    count++;
    const uint4 a = *reinterpret_cast<const uint4*>(T.key + i * LK_KEY_WORDS);
    const uint4 b = *reinterpret_cast<const uint4*>(T.key + i * LK_KEY_WORDS + 4);
    const uint32_t cand[LK_KEY_WORDS + 1] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, (uint32_t)i};
    if (less(cand, best)) {
#pragma unroll
      for (int k = 0; k <= LK_KEY_WORDS; k++) best[k] = cand[k];
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    uint32_t other[LK_KEY_WORDS + 1];
#pragma unroll
    for (int k = 0; k <= LK_KEY_WORDS; k++) other[k] = __shfl_xor(best[k], off);
    if (less(other, best)) {
#pragma unroll
      for (int k = 0; k <= LK_KEY_WORDS; k++) best[k] = other[k];
    }
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k <= LK_KEY_WORDS; k++) best_sh[threadIdx.x >> 6][k] = best[k];
  }
  lk_block_add(count, unmatched, sh4);  // (its barriers publish best_sh)
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) {
      uint32_t other[LK_KEY_WORDS + 1];
#pragma unroll
      for (int k = 0; k <= LK_KEY_WORDS; k++) other[k] = best_sh[w][k];
      if (less(other, best)) {
#pragma unroll
        for (int k = 0; k <= LK_KEY_WORDS; k++) best[k] = other[k];
      }
    }
    uint32_t* r = recs + (size_t)blockIdx.x * LKD_MREC_WORDS;
    const uint32_t slot = best[LK_KEY_WORDS];
    const bool found = slot != 0xFFFFFFFFu;
    const unsigned long long net = found ? T.net[slot] : 0, rep = found ? T.rep[slot] : 0;
    r[0] = found;
    r[1] = slot;
    r[2] = (uint32_t)net;
    r[3] = (uint32_t)(net >> 32);
    r[4] = (uint32_t)rep;
    r[5] = (uint32_t)(rep >> 32);
#pragma unroll
    for (int k = 0; k < LK_KEY_WORDS; k++) r[6 + k] = best[k];
  }
}

// ------------------------------------------------------------------------ host side
namespace {
using LkKey = std::array<uint32_t, LK_KEY_WORDS>;

// The debug list of p (the file's header): the interactions whose kind is among kinds (n_kinds =
// 0: all), or interaction `only` alone.
std::vector<uint32_t> debug_list(const LookupProgram& p, size_t chip, const uint32_t* kinds,
                                 size_t n_kinds, int only, const char* what) {
  std::vector<uint32_t> out(LKD_HEAD, 0);
  size_t at = LKP_HEAD;
  for (int j = 0; j < p.n; j++) {
    const uint32_t head = p.list[at], kind = from_mont(p.list[at + 1]);
    const uint32_t nv = head & 0xff;
    size_t end = at + 2;
    for (uint32_t v = 0; v <= nv; v++) end += 2 + 2 * (size_t)p.list[end + 1];
    if (kind >= (1u << 24))
      throw std::runtime_error(std::string(what) + ": kind " + std::to_string(kind) + " of chip " +
                               std::to_string(chip) + ", interaction " + std::to_string(j) +
                               " is not below 2^24");
    const bool sel = only >= 0 ? j == only
                               : n_kinds == 0 || std::find(kinds, kinds + n_kinds, kind) != kinds + n_kinds;
    if (sel) {
      const size_t next = out.size() + 4 + (end - (at + 2));
      out.insert(out.end(), {head | (uint32_t)j << 16, kind << 8 | nv, (uint32_t)next, 0u});
      out.insert(out.end(), p.list.begin() + at + 2, p.list.begin() + end);
      out[0]++;
    }
    at = end;
  }
  return out;
}

void check_chip(const LookupProgChip& c, const char* what) {
  if (!c.prog || !c.main) throw std::runtime_error("null argument");
  if (c.prog->prep_w && !c.prep) throw std::runtime_error("lookups: the program has preprocessed columns");
  if (c.height == 0 || (c.height & (c.height - 1)) || c.height > ((size_t)1 << 23))
    throw std::runtime_error("lookups: height not a power of two in [1, 2^23]");
  (void)what;
}

void check_canonical(const LookupProgChip& c) {  // the host path's word check
  for (size_t i = 0; i < c.height * (size_t)c.prog->main_w; i++)
    if (c.main[i] >= P) uni_noncanonical_throw("lookups");
  for (size_t i = 0; i < c.height * (size_t)c.prog->prep_w; i++)
    if (c.prep[i] >= P) uni_noncanonical_throw("lookups");
}

// A chip on the device: its traces (column-major, bit-reversed rows) and its debug list.
struct DevChip {
  DBuf<uint32_t> mainc, prepc, list;
  size_t n = 0;
  bool empty = false;  // no interaction selected: nothing to launch
  DevChip(const LookupProgChip& c, const std::vector<uint32_t>& dl, hipStream_t st) : n(c.height) {
    empty = dl[0] == 0;
    if (empty) {  // the upload still refuses a word >= p, as the host path does
      check_canonical(c);
      return;
    }
    mainc = uni_upload_trace((size_t)c.prog->main_w, "lookups", c.main, n, st);
    if (c.prog->prep_w) prepc = uni_upload_trace((size_t)c.prog->prep_w, "lookups", c.prep, n, st);
    list.reset(dl.size());
    upload_async(list.p, dl.data(), dl.size() * 4, st);
  }
};

int row_blocks(size_t n) { return (int)std::min<size_t>(ceil_div(n, 256), LK_MAX_BLOCKS); }

template <int PHASE>
void launch_prog(const DevChip& c, uint32_t chip, uint32_t nchips, const LkPass& p) {
  hipLaunchKernelGGL(k_lookup_prog<PHASE>, dim3(row_blocks(c.n)), dim3(256), 0, p.st,
                     (const uint32_t*)c.list.p, (const uint32_t*)c.mainc.p, (const uint32_t*)c.prepc.p,
                     (uint32_t)c.n, log2i(c.n), chip, nchips, p.hash_mask, p.round, p.combine, p.T,
                     p.ctl, p.share_net, p.share_count);
  KCHECK();
}

LkDriver prog_driver(const std::vector<DevChip>& dev) {
  LkDriver d;
  d.nchips = (int)dev.size();
  d.stride = (int)dev.size();
  d.runtime_stride = true;
  d.rep_bits = LKD_REP_BITS;
  d.launch = [&dev](int k, const LkPass& p) {
    const DevChip& c = dev[k];
    if (c.empty) return;
    const uint32_t nc = (uint32_t)dev.size();
    switch (p.phase) {
      case PH_COUNT: launch_prog<PH_COUNT>(c, k, nc, p); break;
      case PH_CLAIM: launch_prog<PH_CLAIM>(c, k, nc, p); break;
      case PH_MATERIALISE: launch_prog<PH_MATERIALISE>(c, k, nc, p); break;
      case PH_ACCOUNT: launch_prog<PH_ACCOUNT>(c, k, nc, p); break;
      case PH_SHARES: launch_prog<PH_SHARES>(c, k, nc, p); break;
    }
  };
  return d;
}

// ---- the host path: the same debug lists, single-threaded over an ordered map
struct HostEntry {
  long long net = 0;
  std::vector<long long> chip_net;
  std::vector<uint32_t> chip_count;
  int first_chip = -1, first_interaction = -1;
  int64_t first_row = -1;
  bool claimed = false;  // multiplicities: a table row holds the key
};
using HostMap = std::map<LkKey, HostEntry>;  // array order = (kind, values) order

uint32_t host_vcol(const uint32_t* list, size_t& at, const uint32_t* m, const uint32_t* pr) {
  uint32_t r = list[at];
  const uint32_t nt = list[at + 1];
  at += 2;
  for (uint32_t i = 0; i < nt; i++, at += 2) {
    const uint32_t sc = list[at + 1];
    r = madd(r, mmul(list[at], (sc >> 16 ? pr : m)[sc & 0xffff]));
  }
  return r;
}

// The interaction at dl[at] over one row: its key and, with mu, its multiplicity word (else the
// VCOL is skipped); at advances to the next interaction.
LkKey host_key(const std::vector<uint32_t>& dl, size_t& at, const uint32_t* m, const uint32_t* pr,
               uint32_t* mu, uint32_t& head) {
  head = dl[at];
  LkKey key{};
  key[0] = dl[at + 1];
  const size_t next = dl[at + 2];
  at += 4;
  if (mu) *mu = host_vcol(dl.data(), at, m, pr);
  else at += 2 + 2 * (size_t)dl[at + 1];
  if (!mu || *mu)
    for (uint32_t v = 0; v < (head & 0xff); v++) key[1 + v] = from_mont(host_vcol(dl.data(), at, m, pr));
  at = next;
  return key;
}

uint64_t host_aggregate(const std::vector<LookupProgChip>& chips,
                        const std::vector<std::vector<uint32_t>>& lists, HostMap& m) {
  uint64_t interactions = 0;
  for (size_t k = 0; k < chips.size(); k++) {
    const LookupProgChip& c = chips[k];
    check_canonical(c);
    for (size_t r = 0; r < c.height; r++) {
      const uint32_t* mr = c.main + r * (size_t)c.prog->main_w;
      const uint32_t* pr = c.prep ? c.prep + r * (size_t)c.prog->prep_w : nullptr;
      size_t at = LKD_HEAD;
      for (uint32_t i = 0; i < lists[k][0]; i++) {
        uint32_t mu, head;
        const LkKey key = host_key(lists[k], at, mr, pr, &mu, head);
        if (mu == 0) continue;  // debug.rs:94
        const int32_t x = field_to_int(from_mont(mu));
        const long long val = (head >> 8) & 1 ? x : -(long long)x;
        HostEntry& e = m[key];
        if (e.first_chip < 0) {  // chips, rows and interactions ascending: the smallest
          e.first_chip = (int)k;
          e.first_row = (int64_t)r;
          e.first_interaction = (int)((head >> 16) & 31);
          e.chip_net.assign(chips.size(), 0);
          e.chip_count.assign(chips.size(), 0);
        }
        e.net += val;
        e.chip_net[k] += val;
        e.chip_count[k]++;
        interactions++;
      }
    }
  }
  return interactions;
}

void fill_key(const uint32_t* key, LookupDiscrepancy& d) {
  d.kind = (int)(key[0] >> 8);
  d.nvals = (int)(key[0] & 0xFF);
  for (int v = 0; v < LK_MAX_VALUES; v++) d.values[v] = key[1 + v];
}

std::vector<std::vector<uint32_t>> debug_lists(const std::vector<LookupProgChip>& chips,
                                               const uint32_t* kinds, size_t n_kinds, const char* what) {
  if (chips.empty() || chips.size() > (size_t)LKD_MAX_CHIPS)
    throw std::runtime_error(std::string(what) + ": chip count not in [1, " +
                             std::to_string(LKD_MAX_CHIPS) + "]");
  std::vector<std::vector<uint32_t>> lists;
  for (size_t k = 0; k < chips.size(); k++) {
    check_chip(chips[k], what);
    lists.push_back(debug_list(*chips[k].prog, k, kinds, n_kinds, -1, what));
  }
  return lists;
}
}  // namespace

void lookups_debug(const std::vector<LookupProgChip>& chips, const uint32_t* kinds, size_t n_kinds,
                   bool on_device, size_t cap, bool low_hash_bits, LookupProgReport& out) {
  const size_t nc = chips.size();
  const auto lists = debug_lists(chips, kinds, n_kinds, "lookups_debug");
  out = LookupProgReport();
  out.chip_distinct.assign(nc, 0);
  if (on_device) {
    hipStream_t st = stream();
    std::vector<DevChip> dev;
    dev.reserve(nc);
    for (size_t k = 0; k < nc; k++) dev.emplace_back(chips[k], lists[k], st);
    LkShares sh;
    lk_aggregate(prog_driver(dev), cap, low_hash_bits, out.rep, sh);
    out.chip_distinct = sh.chip_distinct;
    out.chip_count = sh.count;
    for (long long v : sh.net) out.chip_net.push_back(lk_net_to_int(v));
    return;
  }
  HostMap m;
  LookupReport& rep = out.rep;
  rep.interactions = host_aggregate(chips, lists, m);
  rep.distinct_keys = m.size();
  long long total = 0;
  for (const auto& kv : m) {
    const HostEntry& e = kv.second;
    total = (total + e.net) % (long long)P;
    for (size_t c = 0; c < nc; c++) out.chip_distinct[c] += e.chip_count[c] != 0;
    const int32_t net = lk_net_to_int(e.net);
    if (net == 0) continue;
    if (rep.unbalanced_keys++ >= cap) continue;
    LookupDiscrepancy d;
    fill_key(kv.first.data(), d);
    d.net = net;
    d.first_chip = e.first_chip;
    d.first_row = e.first_row;
    d.first_interaction = e.first_interaction;
    rep.recs.push_back(d);
    for (size_t c = 0; c < nc; c++) {
      out.chip_net.push_back(lk_net_to_int(e.chip_net[c]));
      out.chip_count.push_back(e.chip_count[c]);
    }
  }
  rep.total_net = lk_net_to_int(total);
  rep.balanced = rep.unbalanced_keys == 0;
}

void lookups_multiplicities(const LookupProgChip& table, int interaction,
                            const std::vector<LookupProgChip>& senders, bool on_device,
                            bool low_hash_bits, uint32_t* mult_out, LookupMultReport& out) {
  const char* what = "lookups_multiplicities";
  if (!mult_out) throw std::runtime_error("null argument");
  check_chip(table, what);
  if (interaction < 0 || interaction >= table.prog->n)
    throw std::runtime_error(std::string(what) + ": interaction " + std::to_string(interaction) +
                             " is not below the table program's " + std::to_string(table.prog->n));
  const auto lists = debug_lists(senders, nullptr, 0, what);
  const std::vector<uint32_t> tlist = debug_list(*table.prog, 0, nullptr, 0, interaction, what);
  out = LookupMultReport();
  std::fill(mult_out, mult_out + table.height, 0u);
  const size_t n = table.height;

  if (!on_device) {
    check_canonical(table);
    HostMap m;
    out.interactions = host_aggregate(senders, lists, m);
    out.distinct_keys = m.size();
    for (size_t r = 0; r < n; r++) {
      size_t at = LKD_HEAD;
      uint32_t head;
      const LkKey key = host_key(tlist, at, table.main + r * (size_t)table.prog->main_w,
                                 table.prep ? table.prep + r * (size_t)table.prog->prep_w : nullptr,
                                 nullptr, head);
      const auto it = m.find(key);
      if (it == m.end() || it->second.claimed) continue;  // the first row of a key takes its net
      it->second.claimed = true;
      long long v = it->second.net % (long long)P;
      if (v < 0) v += P;
      mult_out[r] = to_mont((uint32_t)v);
    }
    for (const auto& kv : m) {
      if (kv.second.claimed) continue;
      if (out.unmatched++ == 0) {  // map order: the smallest
        fill_key(kv.first.data(), out.first);
        out.first.net = lk_net_to_int(kv.second.net);
        out.first.first_chip = kv.second.first_chip;
        out.first.first_row = kv.second.first_row;
        out.first.first_interaction = kv.second.first_interaction;
      }
    }
    return;
  }

  hipStream_t st = stream();
  std::vector<DevChip> dev;
  dev.reserve(senders.size());
  for (size_t k = 0; k < senders.size(); k++) dev.emplace_back(senders[k], lists[k], st);
  const DevChip tdev(table, tlist, st);
  LkDriver d = prog_driver(dev);
  d.after_rounds = [&](const LkPass& p) {  // the table holds every sender's net
    const size_t size = (size_t)1 << p.T.logsize;
    const int blocks = row_blocks(n), scan_blocks = row_blocks(size);
    DBuf<uint32_t> slot_of(n), mult(n), recs_d((size_t)scan_blocks * LKD_MREC_WORDS);
    DBuf<unsigned long long> unmatched(1);
    HIP_CHECK(hipMemsetAsync(p.T.aux, 0xFF, size * 4, st));
    HIP_CHECK(hipMemsetAsync(unmatched.p, 0, 8, st));
    hipLaunchKernelGGL(k_mult_claim, dim3(blocks), dim3(256), 0, st, (const uint32_t*)tdev.list.p,
                       (const uint32_t*)tdev.mainc.p, (const uint32_t*)tdev.prepc.p, (uint32_t)n,
                       log2i(n), p.hash_mask, p.T, slot_of.p);
    KCHECK();
    hipLaunchKernelGGL(k_mult_write, dim3(blocks), dim3(256), 0, st, (uint32_t)n, log2i(n), p.T,
                       (const uint32_t*)slot_of.p, mult.p);
    KCHECK();
    hipLaunchKernelGGL(k_mult_scan, dim3(scan_blocks), dim3(256), 0, st, p.T, unmatched.p, recs_d.p);
    KCHECK();
    std::vector<uint32_t> recs((size_t)scan_blocks * LKD_MREC_WORDS);
    unsigned long long um = 0;
    HIP_CHECK(hipMemcpyAsync(mult_out, mult.p, n * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(recs.data(), recs_d.p, recs.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(&um, unmatched.p, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    out.unmatched = um;
    const uint32_t* best = nullptr;
    for (int b = 0; b < scan_blocks; b++) {
      const uint32_t* r = &recs[(size_t)b * LKD_MREC_WORDS];
      if (r[0] && (!best || std::lexicographical_compare(r + 6, r + 14, best + 6, best + 14))) best = r;
    }
    if ((um != 0) != (best != nullptr))
      throw std::runtime_error("debug_interactions: inconsistent aggregation table");
    if (best) {
      fill_key(best + 6, out.first);
      out.first.net = lk_net_to_int((long long)((unsigned long long)best[2] | ((unsigned long long)best[3] << 32)));
      const unsigned long long rep = (unsigned long long)best[4] | ((unsigned long long)best[5] << 32);
      out.first.first_chip = (int)(rep >> 32);
      out.first.first_row = (int64_t)((rep & 0xFFFFFFFFull) >> LKD_REP_BITS);
      out.first.first_interaction = (int)(rep & ((1u << LKD_REP_BITS) - 1));
    }
  };
  LookupReport rep;
  LkShares sh;
  lk_aggregate(d, 0, low_hash_bits, rep, sh);
  out.interactions = rep.interactions;
  out.distinct_keys = rep.distinct_keys;
}

}  // namespace bfz
