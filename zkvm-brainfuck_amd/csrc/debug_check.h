// Constraint checker: the reference's `--features debug` mode on the device.
//   debug_constraints                      crates/stark/src/debug.rs:24-105
//   StarkMachine::debug_constraints        crates/stark/src/machine.rs:288-387
//   debug_interactions_with_all_chips      crates/stark/src/lookup/debug.rs:59-196, in part:
//     here (bfz_record_debug_constraints): the balance per LookupKIND and chip under the LogUp
//     challenges, kind_sum / kind_net / kind_count;
//     lookup_debug.h (bfz_record_debug_interactions): the per-KEY result the reference prints,
//     every tuple's sends minus receives and each chip's share (debug.rs:100-115,145-171).
// The AIRs and the LogUp constraints are the templates of air.h, evaluated on the TRACE domain
// with a third accumulator (FirstFailAcc) instead of the quotient's alpha fold: row i is local,
// row (i + 1) mod h is next, is_first = [i == 0], is_last = [i == h - 1], is_transition =
// 1 - is_last (debug.rs:43-94).  The row functions are KB_HD: the host path of bfz_check_chip
// runs the same code single-threaded, the kernels of debug_check.hip one row per thread.
//
// Constraint index: the 0-based position in Chip::eval's emission order (chip.rs:222-228): the
// chip's AIR constraints, one LogUp constraint per batch, then first-row, transition, last-row
// (permutation.rs:157-272) -- the order num_constraints(chip) counts.
#pragma once
#include <vector>

#include "air.h"
#include "logup.h"
#include "prover.h"

namespace bfz {

constexpr int NUM_KINDS = 8;  // LookupKind 1..7 (lookup.rs:17-42); index 0 unused
constexpr int DBG_MAIN_W[NUM_CHIPS] = {31, 1, 7, 45, 12, 2, 41, 5};
constexpr int DBG_PREP_W[NUM_CHIPS] = {0, 6, 0, 0, 0, 2, 0, 0};
constexpr int DBG_PERM_W[NUM_CHIPS] = {9, 2, 4, 2, 3, 2, 2, 2};  // EF columns

// Counts the emissions and remembers the first one that is not zero.  Every value kb::madd /
// msub / mmul / mneg return is reduced to [0, p) (one umin against the -p / +p candidate), and
// the inputs are checked to be canonical words before they get here, so a constraint holds
// exactly when its word is 0.
struct FirstFailAcc {
  int n = 0, first = -1;
  KB_HD void emit(uint32_t c) {
    if (c != 0 && first < 0) first = n;
    n++;
  }
  KB_HD void emit_ext(const EF& c) {
    if (!kb::ef_is_zero(c) && first < 0) first = n;
    n++;
  }
};

// Chip::eval on one row of the trace domain (debug.rs:43-97): the first failing constraint
// index, or -1.  L / N: main local / next; PL / PN: preprocessed; pl / pn: permutation (EF).
// PERM = false stops after the chip's own AIR constraints (indices 0 .. K_air - 1, the K of
// uni_air_shape): what p3_uni_stark's debug-build prove checks (utils/prove.rs:97-112), where
// send / receive are no-ops; the permutation arguments are then not read.
template <int CHIP, bool PERM = true>
KB_HD int check_row(const uint32_t* L, const uint32_t* N, const uint32_t* PL, const uint32_t* PN,
                    const EF* pl, const EF* pn, bool is_first, bool is_last, const EF& alpha,
                    const EF* beta_pows, const EF& cumsum) {
  const uint32_t first = is_first ? kb::ONE : 0, last = is_last ? kb::ONE : 0,
                 trans = is_last ? 0 : kb::ONE;
  FirstFailAcc acc;
  Air<BaseOps, FirstFailAcc> air{L, N, PL, PN, first, last, trans, acc};
  air.template eval_air<CHIP>();
  if constexpr (PERM)
    air.template eval_perm<CHIP>(pl, pn, alpha, beta_pows, cumsum, kb::ef_base(first),
                                 kb::ef_base(last), kb::ef_base(trans));
  return acc.first;
}
// The AIR-only row of a chip without a preprocessed trace (the uni-STARK chips).
template <int CHIP>
KB_HD int check_row_air(const uint32_t* L, const uint32_t* N, bool is_first, bool is_last) {
  const uint32_t none[1] = {0};
  const EF z = kb::ef_zero();
  return check_row<CHIP, false>(L, N, none, none, nullptr, nullptr, is_first, is_last, z, nullptr, z);
}

// One row's interactions for the balance table (lookup/debug.rs:79-116): per LookupKind the sum
// of +-mult / (alpha + kind + sum_v beta^(v+1) val_v) over the chip's lookups whose multiplicity
// is not zero, the sum of the signed multiplicities (a field element) and their number.  The
// denominators of the row are inverted together (one EF inversion per row).
struct KindSums {
  EF sum[NUM_KINDS];
  uint32_t net[NUM_KINDS];
  uint32_t count[NUM_KINDS];
  KB_HD void clear() {
#pragma unroll
    for (int k = 0; k < NUM_KINDS; k++) {
      sum[k] = kb::ef_zero();
      net[k] = 0;
      count[k] = 0;
    }
  }
};

template <int CHIP, int J, int NL>
KB_HD void balance_gather(const Air<BaseOps, FirstFailAcc>& air, const EF& alpha,
                          const EF* beta_pows, EF (&den)[NL], uint32_t (&mult)[NL]) {
  if constexpr (J < NL) {
    EF r, m;
    air.template rlc_mult<CHIP, J>(alpha, beta_pows, r, m);
    mult[J] = m.c[0];  // the signed multiplicity is a base-field value
    // a zero multiplicity contributes nothing; a zero denominator (probability ~ 2^-124 per
    // interaction) has no inverse: both are skipped, with 1 in the batch inversion
    if (mult[J] == 0 || kb::ef_is_zero(r)) {
      mult[J] = 0;
      r = kb::ef_one();
    }
    den[J] = r;
    balance_gather<CHIP, J + 1, NL>(air, alpha, beta_pows, den, mult);
  }
}

template <int CHIP, int J, int NL>
KB_HD void balance_scatter(const EF (&inv)[NL], const uint32_t (&mult)[NL], KindSums& ks) {
  if constexpr (J < NL) {
    constexpr int kind = LookupsOf<CHIP>::v.l[J].kind;
    if (mult[J] != 0) {
      ks.sum[kind] = kb::ef_add(ks.sum[kind], kb::ef_mul_base(inv[J], mult[J]));
      ks.net[kind] = kb::madd(ks.net[kind], mult[J]);
      ks.count[kind] += 1;
    }
    balance_scatter<CHIP, J + 1, NL>(inv, mult, ks);
  }
}

template <int CHIP>
KB_HD void balance_row(const uint32_t* L, const uint32_t* PL, const EF& alpha, const EF* beta_pows,
                       KindSums& ks) {
  constexpr int NL = LookupsOf<CHIP>::v.n;
  FirstFailAcc unused;
  Air<BaseOps, FirstFailAcc> air{L, L, PL, PL, 0, 0, 0, unused};
  EF den[NL], inv[NL];
  uint32_t mult[NL];
  balance_gather<CHIP, 0, NL>(air, alpha, beta_pows, den, mult);
  // Montgomery's trick: inv[j] first holds d_0 .. d_(j-1), then 1 / d_j
  EF run = kb::ef_one();
#pragma unroll
  for (int j = 0; j < NL; j++) {
    inv[j] = run;
    run = kb::ef_mul(run, den[j]);
  }
  run = kb::ef_inv(run);
#pragma unroll
  for (int j = NL - 1; j >= 0; j--) {
    inv[j] = kb::ef_mul(inv[j], run);
    run = kb::ef_mul(run, den[j]);
  }
  balance_scatter<CHIP, 0, NL>(inv, mult, ks);
}

// ------------------------------------------------------------------------ results
struct ChipCheck {
  int chip = -1;
  size_t height = 0;
  int num_constraints = 0;
  int num_batches = 0;        // LogUp batch constraints: indices [K - 3 - batches, K - 3)
  uint64_t failing_rows = 0;
  int64_t first_row = -1;     // smallest failing row, -1 if none
  int first_constraint = -1;  // first failing index at that row, -1 if none
  EF cumsum{};
};

struct DebugReport {
  bool ok = false;
  std::vector<ChipCheck> chips;  // included chips in machine order
  EF alpha{}, beta{}, cumsum{};
  bool balance_valid = false;
  // [kind][chip id]: LogUp sum, signed multiplicity sum (field_to_int, lookup/debug.rs:46-54) and
  // number of non-zero interactions
  EF kind_sum[NUM_KINDS][NUM_CHIPS] = {};
  int32_t kind_net[NUM_KINDS][NUM_CHIPS] = {};
  uint32_t kind_count[NUM_KINDS][NUM_CHIPS] = {};
};

// Host path: row-major natural-order traces (Montgomery); perm = the flattened permutation
// trace (h x 4 perm_width).  per_row (optional, h entries): first failing index or -1.
void check_chip_host(int chip, const uint32_t* main, const uint32_t* prep, const uint32_t* perm,
                     size_t h, const EF& alpha, const EF& beta, const EF& cumsum, ChipCheck& out,
                     int32_t* per_row);

// Device path: column-major bit-reversed traces in HBM (gpu.h LAYOUT), the challenges and the
// chip's cumulative sum in device memory.  res receives {min(row * K + idx) or ~0, failing rows};
// per_row_dev (optional): first failing index or -1 per STORAGE position.
void check_chip_device(int chip, const uint32_t* mainc, const uint32_t* prepc,
                       const uint32_t* permc, size_t h, const PermChallenges* ch_dev,
                       const EF* cumsum_dev, unsigned long long* res_dev, int32_t* per_row_dev,
                       hipStream_t st);
// The AIR-only check of one uni-STARK chip (Cpu, AddSub, Jump, MemoryInstrs, IO; others throw as
// uni_air_shape_or_throw): out.num_constraints = the K of uni_air_shape, num_batches = 0.
// Host: row-major natural-order trace.  Device: a device-resident column-major bit-reversed
// trace (gpu.h LAYOUT); the kernel's two result words and its per-row array are brought back
// (syncs st).  per_row (optional, host, h entries) is in natural row order in both.
void check_air_host(int chip, const uint32_t* main, size_t h, ChipCheck& out, int32_t* per_row);
void check_air_resident(int chip, const uint32_t* mainc, size_t h, ChipCheck& out, int32_t* per_row,
                        hipStream_t st);
// The same for any AIR (uni_stark.h UniAir): a built-in chip as above, or a compiled constraint
// program run by the interpreters of air_program.h (out.chip = -1).
struct UniAir;
void check_air_host(const UniAir& air, const uint32_t* main, size_t h, ChipCheck& out,
                    int32_t* per_row);
void check_air_resident(const UniAir& air, const uint32_t* mainc, size_t h, ChipCheck& out,
                        int32_t* per_row, hipStream_t st);
// chip, height, K and the number of LogUp batches of a result.
void fill_chip_header(int chip, size_t h, ChipCheck& out);
// Fills out.{failing_rows, first_row, first_constraint} from the two downloaded words.
void decode_check_result(const unsigned long long res[2], ChipCheck& out);

// out_dev: NUM_KINDS x 6 words (sum[4], net, count) of one chip, reduced over its rows.
void lookup_balance_device(int chip, const uint32_t* mainc, const uint32_t* prepc, size_t h,
                           const PermChallenges* ch_dev, uint32_t* out_dev, hipStream_t st);

// StarkMachine::debug_constraints (machine.rs:288-387) on device-resident main traces: samples
// alpha then beta from ch (advanced), generates the permutation traces, sums the cumulative
// sums, checks every chip and, when the sum is not zero or force_balance, fills the balance
// table.  No LDE, no commit.
void debug_constraints_device(const ProvingKey& pk, const DeviceTraces& dt, Challenger& ch,
                              bool force_balance, DebugReport& out);

#if defined(__HIPCC__)
// ---- the block reduction of the check kernels (debug_check.hip, air_program.hip)
__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off);
    v = o < v ? o : v;
  }
  return v;
}

// The block's failing rows into res: wave minimum of row * K + index and ballot popcount, block
// minimum over the four waves, then one atomicMin / atomicAdd per block that has a failure.
// Every thread of the block calls it (idx < 0: the row holds, or there is no row).
__device__ __forceinline__ void reduce_failures(int idx, uint32_t i, int K,
                                                unsigned long long* __restrict__ res) {
  const bool fail = idx >= 0;
  const unsigned long long key =
      wave_min(fail ? (unsigned long long)i * (unsigned)K + (unsigned)idx : ~0ull);
  const unsigned long long votes = __ballot(fail);
  __shared__ unsigned long long s_key[4];
  __shared__ uint32_t s_cnt[4];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_key[wave] = key;
    s_cnt[wave] = (uint32_t)__popcll(votes);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long k = s_key[0];
    uint32_t cnt = s_cnt[0];
    for (int w = 1; w < 4; w++) {
      k = s_key[w] < k ? s_key[w] : k;
      cnt += s_cnt[w];
    }
    if (cnt) {
      atomicMin(&res[0], k);
      atomicAdd(&res[1], (unsigned long long)cnt);
    }
  }
}
#endif

}  // namespace bfz
