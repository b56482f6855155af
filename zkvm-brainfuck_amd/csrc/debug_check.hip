// Constraint checker kernels (debug_check.h): Chip::eval on every row of the trace domain
// (crates/stark/src/debug.rs:24-105) and the per-kind lookup balance of
// crates/stark/src/lookup/debug.rs:59-196, driven as StarkMachine::debug_constraints
// (crates/stark/src/machine.rs:288-387).
//
// k_check<CHIP>: one thread per storage position t of the column-major bit-reversed traces
// (natural row i = bitrev(t), next row at bitrev((i + 1) mod h)), loads as k_quotient's (one
// buffer descriptor per column, the row as voffset).  Everything is reduced on the device: the
// number of failing rows (ballot popcounts, one atomic per block) and min(row * K + index) (wave
// and block minimum, one 64-bit atomicMin per block) -- integers, so the result does not depend
// on the execution order.
// k_lookup_balance<CHIP>: per block a slab of per-kind partial sums (LDS reduction), summed by
// k_balance_reduce in a second launch: no modular atomics, deterministic.
//
// These kernels are not part of a proof and are NOT in a PreloadKernels list: bfz_init and the
// first proof of a process do not pay for them.
#include "debug_check.h"

#include <algorithm>
#include <cstring>
#include <numeric>
#include <type_traits>

#include "quotient.h"
#include "uni_stark.h"

namespace bfz {

using namespace kb;

template <int I, int N, class F>
__device__ __forceinline__ void dbg_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    dbg_for<I + 1, N>(f);
  }
}

template <int CHIP>
constexpr bool uses_kind(int kind) {
  for (int j = 0; j < LookupsOf<CHIP>::v.n; j++)
    if (LookupsOf<CHIP>::v.l[j].kind == kind) return true;
  return false;
}

// ------------------------------------------------------------------------ row check
template <int CHIP>
__global__ __launch_bounds__(256) void k_check(const uint32_t* __restrict__ mainc,
                                               const uint32_t* __restrict__ prepc,
                                               const uint32_t* __restrict__ permc, uint32_t n,
                                               int logn, const PermChallenges* __restrict__ chp,
                                               const EF* __restrict__ cumsum, int K,
                                               unsigned long long* __restrict__ res,
                                               int32_t* __restrict__ per_row) {
  const PermChallenges ch = *chp;  // uniform: scalar loads
  const EF cs = *cumsum;
  constexpr int MW = DBG_MAIN_W[CHIP];
  constexpr int PWD = DBG_PREP_W[CHIP] > 0 ? DBG_PREP_W[CHIP] : 1;
  constexpr int PMW = DBG_PERM_W[CHIP];
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  int idx = -1;
  uint32_t i = 0;
  if (t < n) {  // (no early return: every thread takes part in the block reduction)
    i = dbitrev(t, logn);
    const uint32_t tn = dbitrev((i + 1) & (n - 1), logn);  // h = 1: the row is its own next
    const uint32_t vt = t * 4u, vn = tn * 4u;               // t, tn < n <= 2^23
    uint32_t L[MW], Nx[MW], PL[PWD], PN[PWD];
#pragma unroll
    for (int c = 0; c < MW; c++) {
      const __amdgpu_buffer_rsrc_t r = rsrc_of(mainc + (size_t)c * n);
      L[c] = ld_b(r, vt, 0);
      Nx[c] = ld_b(r, vn, 0);
    }
#pragma unroll
    for (int c = 0; c < PWD; c++) {
      PL[c] = DBG_PREP_W[CHIP] > 0 ? prepc[(size_t)c * n + t] : 0;
      PN[c] = DBG_PREP_W[CHIP] > 0 ? prepc[(size_t)c * n + tn] : 0;
    }
    EF pl[PMW], pn[PMW];
#pragma unroll
    for (int e = 0; e < PMW; e++)
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const __amdgpu_buffer_rsrc_t r = rsrc_of(permc + (size_t)(4 * e + k) * n);
        pl[e].c[k] = ld_b(r, vt, 0);
        pn[e].c[k] = ld_b(r, vn, 0);
      }
    idx = check_row<CHIP>(L, Nx, PL, PN, pl, pn, i == 0, i == n - 1, ch.alpha, ch.beta_pows, cs);
    if (per_row) per_row[t] = idx;
  }
  reduce_failures(idx, i, K, res);
}

template <int CHIP>
static void launch_check(const uint32_t* mainc, const uint32_t* prepc, const uint32_t* permc,
                         size_t h, const PermChallenges* ch, const EF* cumsum,
                         unsigned long long* res, int32_t* per_row, hipStream_t st) {
  hipLaunchKernelGGL(k_check<CHIP>, dim3(ceil_div(h, 256)), dim3(256), 0, st, mainc, prepc, permc,
                     (uint32_t)h, log2i(h), ch, cumsum, num_constraints(CHIP), res, per_row);
  KCHECK();
}

static void check_shape(int chip, size_t h) {
  if (chip < 0 || chip >= NUM_CHIPS) throw std::runtime_error("check: bad chip index");
  if (h < 1 || (h & (h - 1)) || h > ((size_t)1 << 23))
    throw std::runtime_error("check: height not a power of two in [1, 2^23]");
  if (DBG_MAIN_W[chip] != CHIP_INFO[chip].main_w || DBG_PREP_W[chip] != CHIP_INFO[chip].prep_w ||
      DBG_PERM_W[chip] != perm_width(chip))
    throw std::runtime_error("check: width tables out of step with CHIP_INFO");
}

void check_chip_device(int chip, const uint32_t* mainc, const uint32_t* prepc,
                       const uint32_t* permc, size_t h, const PermChallenges* ch_dev,
                       const EF* cumsum_dev, unsigned long long* res_dev, int32_t* per_row_dev,
                       hipStream_t st) {
  check_shape(chip, h);
  if (CHIP_INFO[chip].prep_w && !prepc) throw std::runtime_error("check: this chip has a preprocessed trace");
#define BFZ_CHECK_CASE(C) \
  case C: launch_check<C>(mainc, prepc, permc, h, ch_dev, cumsum_dev, res_dev, per_row_dev, st); break;
  switch (chip) {
    BFZ_CHECK_CASE(CHIP_CPU)
    BFZ_CHECK_CASE(CHIP_PROGRAM)
    BFZ_CHECK_CASE(CHIP_ADDSUB)
    BFZ_CHECK_CASE(CHIP_JUMP)
    BFZ_CHECK_CASE(CHIP_MEMORY)
    BFZ_CHECK_CASE(CHIP_BYTE)
    BFZ_CHECK_CASE(CHIP_MEMINSTRS)
    BFZ_CHECK_CASE(CHIP_IO)
  }
#undef BFZ_CHECK_CASE
}

void decode_check_result(const unsigned long long res[2], ChipCheck& out) {
  out.failing_rows = res[1];
  if (res[1] == 0) {
    out.first_row = -1;
    out.first_constraint = -1;
  } else {
    out.first_row = (int64_t)(res[0] / (unsigned)out.num_constraints);
    out.first_constraint = (int)(res[0] % (unsigned)out.num_constraints);
  }
}

// ------------------------------------------------------------------------ AIR-only row check
// k_check_air<CHIP>: k_check without the preprocessed and permutation columns and without the
// challenges -- Air::eval_air<CHIP> alone, what p3_uni_stark::prove checks in a debug build
// (crates/core/machine/src/utils/prove.rs:97-112).  K is the chip's AIR constraint count.
template <int CHIP>
__global__ __launch_bounds__(256) void k_check_air(const uint32_t* __restrict__ mainc, uint32_t n,
                                                   int logn, int K,
                                                   unsigned long long* __restrict__ res,
                                                   int32_t* __restrict__ per_row) {
  constexpr int MW = DBG_MAIN_W[CHIP];
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  int idx = -1;
  uint32_t i = 0;
  if (t < n) {  // (no early return: every thread takes part in the block reduction)
    i = dbitrev(t, logn);
    const uint32_t tn = dbitrev((i + 1) & (n - 1), logn);  // h = 1: the row is its own next
    const uint32_t vt = t * 4u, vn = tn * 4u;               // t, tn < n <= 2^23
    uint32_t L[MW], Nx[MW];
#pragma unroll
    for (int c = 0; c < MW; c++) {
      const __amdgpu_buffer_rsrc_t r = rsrc_of(mainc + (size_t)c * n);
      L[c] = ld_b(r, vt, 0);
      Nx[c] = ld_b(r, vn, 0);
    }
    idx = check_row_air<CHIP>(L, Nx, i == 0, i == n - 1);
    if (per_row) per_row[t] = idx;
  }
  reduce_failures(idx, i, K, res);
}

template <int CHIP>
static void rows_air_host(const uint32_t* main, size_t h, ChipCheck& out, int32_t* per_row) {
  constexpr int MW = DBG_MAIN_W[CHIP];
  out.failing_rows = 0;
  out.first_row = -1;
  out.first_constraint = -1;
  for (size_t i = 0; i < h; i++) {
    const size_t nx = (i + 1) & (h - 1);
    const int idx = check_row_air<CHIP>(main + i * MW, main + nx * MW, i == 0, i == h - 1);
    if (per_row) per_row[i] = idx;
    if (idx >= 0 && out.failing_rows++ == 0) {
      out.first_row = (int64_t)i;
      out.first_constraint = idx;
    }
  }
}

static void fill_air_header(int chip, size_t h, ChipCheck& out) {
  int K = 0;
  uni_air_shape_or_throw(chip, &K, nullptr, nullptr);
  check_shape(chip, h);
  out = ChipCheck();
  out.chip = chip;
  out.height = h;
  out.num_constraints = K;
}

#define BFZ_AIR_CHIPS(X) X(CHIP_CPU) X(CHIP_ADDSUB) X(CHIP_JUMP) X(CHIP_MEMINSTRS) X(CHIP_IO)

// The rows of a constraint program on the host (air_run over BaseOps), as rows_air_host.
static void rows_prog_host(const AirProgram& p, const uint32_t* main, size_t h, ChipCheck& out,
                           int32_t* per_row) {
  const size_t w = (size_t)p.width;
  out.failing_rows = 0;
  out.first_row = -1;
  out.first_constraint = -1;
  for (size_t i = 0; i < h; i++) {
    const size_t nx = (i + 1) & (h - 1);
    const int idx = air_first_fail(p, main + i * w, main + nx * w, i == 0, i == h - 1);
    if (per_row) per_row[i] = idx;
    if (idx >= 0 && out.failing_rows++ == 0) {
      out.first_row = (int64_t)i;
      out.first_constraint = idx;
    }
  }
}

static void fill_air_header(const UniAir& air, size_t h, ChipCheck& out) {
  if (air.prog) {
    if (h < 1 || (h & (h - 1)) || h > ((size_t)1 << 23))
      throw std::runtime_error("check: height not a power of two in [1, 2^23]");
    out = ChipCheck();
    out.height = h;
    out.num_constraints = air.num_constraints;
  } else {
    fill_air_header(air.chip, h, out);
  }
}

void check_air_host(const UniAir& air, const uint32_t* main, size_t h, ChipCheck& out,
                    int32_t* per_row) {
  fill_air_header(air, h, out);
  if (air.prog) return rows_prog_host(*air.prog, main, h, out, per_row);
#define BFZ_AIR_CASE(C) \
  case C: rows_air_host<C>(main, h, out, per_row); break;
  switch (air.chip) { BFZ_AIR_CHIPS(BFZ_AIR_CASE) }
#undef BFZ_AIR_CASE
}

void check_air_host(int chip, const uint32_t* main, size_t h, ChipCheck& out, int32_t* per_row) {
  check_air_host(uni_air_of_chip(chip), main, h, out, per_row);
}

void check_air_resident(const UniAir& air, const uint32_t* mainc, size_t h, ChipCheck& out,
                        int32_t* per_row, hipStream_t st) {
  fill_air_header(air, h, out);
  DBuf<unsigned long long> resd(2);
  DBuf<int32_t> rowd;
  DBuf<uint32_t> code_d;
  if (per_row) rowd.reset(h);
  unsigned long long res[2] = {~0ull, 0};
  HIP_CHECK(hipMemcpyAsync(resd.p, res, sizeof(res), hipMemcpyHostToDevice, st));
  if (air.prog) {  // the instruction list, uploaded once per call
    const std::vector<uint32_t>& code = air.prog->code;
    code_d.reset(code.size());
    HIP_CHECK(hipMemcpyAsync(code_d.p, code.data(), code.size() * 4, hipMemcpyHostToDevice, st));
    launch_check_prog(code_d.p, (int)code.size(), mainc, h, out.num_constraints, resd.p, rowd.p, st);
  } else {
#define BFZ_AIR_CASE(C)                                                                        \
  case C:                                                                                      \
    hipLaunchKernelGGL(k_check_air<C>, dim3(ceil_div(h, 256)), dim3(256), 0, st, mainc,        \
                       (uint32_t)h, log2i(h), out.num_constraints, resd.p, rowd.p);            \
    break;
    switch (air.chip) { BFZ_AIR_CHIPS(BFZ_AIR_CASE) }
#undef BFZ_AIR_CASE
    KCHECK();
  }
  std::vector<int32_t> rows(per_row ? h : 0);
  HIP_CHECK(hipMemcpyAsync(res, resd.p, sizeof(res), hipMemcpyDeviceToHost, st));
  if (per_row) HIP_CHECK(hipMemcpyAsync(rows.data(), rowd.p, h * 4, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  decode_check_result(res, out);
  if (per_row) {
    const int logh = log2i(h);
    for (size_t r = 0; r < h; r++) per_row[r] = rows[bitrev32((uint32_t)r, logh)];  // storage -> natural
  }
}

void check_air_resident(int chip, const uint32_t* mainc, size_t h, ChipCheck& out, int32_t* per_row,
                        hipStream_t st) {
  check_air_resident(uni_air_of_chip(chip), mainc, h, out, per_row, st);
}
#undef BFZ_AIR_CHIPS

// ------------------------------------------------------------------------ host path
template <int CHIP>
static void check_rows_host(const uint32_t* main, const uint32_t* prep, const uint32_t* perm,
                            size_t h, const EF& alpha, const EF* beta_pows, const EF& cumsum,
                            ChipCheck& out, int32_t* per_row) {
  constexpr int MW = DBG_MAIN_W[CHIP], PW = DBG_PREP_W[CHIP], PMW = DBG_PERM_W[CHIP];
  const uint32_t none[1] = {0};
  out.failing_rows = 0;
  out.first_row = -1;
  out.first_constraint = -1;
  std::vector<EF> pl(PMW), pn(PMW);
  for (size_t i = 0; i < h; i++) {
    const size_t nx = (i + 1) & (h - 1);
    std::memcpy(pl.data(), perm + i * 4 * PMW, sizeof(EF) * PMW);
    std::memcpy(pn.data(), perm + nx * 4 * PMW, sizeof(EF) * PMW);
    const int idx = check_row<CHIP>(main + i * MW, main + nx * MW, PW ? prep + i * PW : none,
                                    PW ? prep + nx * PW : none, pl.data(), pn.data(), i == 0,
                                    i == h - 1, alpha, beta_pows, cumsum);
    if (per_row) per_row[i] = idx;
    if (idx >= 0) {
      if (out.failing_rows++ == 0) {
        out.first_row = (int64_t)i;
        out.first_constraint = idx;
      }
    }
  }
}

void fill_chip_header(int chip, size_t h, ChipCheck& out) {
  out.chip = chip;
  out.height = h;
  out.num_constraints = num_constraints(chip);
  out.num_batches = perm_width(chip) - 1;
}

void check_chip_host(int chip, const uint32_t* main, const uint32_t* prep, const uint32_t* perm,
                     size_t h, const EF& alpha, const EF& beta, const EF& cumsum, ChipCheck& out,
                     int32_t* per_row) {
  check_shape(chip, h);
  if (CHIP_INFO[chip].prep_w && !prep) throw std::runtime_error("check: this chip has a preprocessed trace");
  fill_chip_header(chip, h, out);
  out.cumsum = cumsum;
  EF bp[8];
  bp[0] = ef_one();
  for (int j = 1; j < 8; j++) bp[j] = ef_mul(bp[j - 1], beta);
#define BFZ_CHECK_CASE(C) \
  case C: check_rows_host<C>(main, prep, perm, h, alpha, bp, cumsum, out, per_row); break;
  switch (chip) {
    BFZ_CHECK_CASE(CHIP_CPU)
    BFZ_CHECK_CASE(CHIP_PROGRAM)
    BFZ_CHECK_CASE(CHIP_ADDSUB)
    BFZ_CHECK_CASE(CHIP_JUMP)
    BFZ_CHECK_CASE(CHIP_MEMORY)
    BFZ_CHECK_CASE(CHIP_BYTE)
    BFZ_CHECK_CASE(CHIP_MEMINSTRS)
    BFZ_CHECK_CASE(CHIP_IO)
  }
#undef BFZ_CHECK_CASE
}

// ------------------------------------------------------------------------ lookup balance
constexpr int BAL_WORDS = NUM_KINDS * 6;  // per kind: sum[4], net, count
constexpr int BAL_MAX_BLOCKS = 1024;

__device__ __forceinline__ uint32_t wave_sum(uint32_t v, bool modular) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t o = __shfl_xor(v, off);
    v = modular ? madd(v, o) : v + o;
  }
  return v;
}

template <int CHIP>
__global__ __launch_bounds__(256) void k_lookup_balance(const uint32_t* __restrict__ mainc,
                                                        const uint32_t* __restrict__ prepc,
                                                        uint32_t n,
                                                        const PermChallenges* __restrict__ chp,
                                                        uint32_t* __restrict__ slabs) {
  const PermChallenges ch = *chp;
  constexpr int MW = DBG_MAIN_W[CHIP];
  constexpr int PWD = DBG_PREP_W[CHIP] > 0 ? DBG_PREP_W[CHIP] : 1;
  KindSums ks;
  ks.clear();
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
    uint32_t L[MW], PL[PWD];
#pragma unroll
    for (int c = 0; c < MW; c++) L[c] = mainc[(size_t)c * n + t];
#pragma unroll
    for (int c = 0; c < PWD; c++) PL[c] = DBG_PREP_W[CHIP] > 0 ? prepc[(size_t)c * n + t] : 0;
    balance_row<CHIP>(L, PL, ch.alpha, ch.beta_pows, ks);
  }
  __shared__ uint32_t sh[4][BAL_WORDS];
  if (threadIdx.x < 4 * BAL_WORDS) (&sh[0][0])[threadIdx.x] = 0;  // kinds the chip does not use
  __syncthreads();
  const int wave = threadIdx.x >> 6;
  const bool lead = (threadIdx.x & 63) == 0;
  dbg_for<1, NUM_KINDS>([&](auto KK) {
    constexpr int kind = decltype(KK)::value;
    if constexpr (uses_kind<CHIP>(kind)) {
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const uint32_t v = wave_sum(ks.sum[kind].c[e], true);
        if (lead) sh[wave][kind * 6 + e] = v;
      }
      const uint32_t nt = wave_sum(ks.net[kind], true);
      const uint32_t ct = wave_sum(ks.count[kind], false);
      if (lead) {
        sh[wave][kind * 6 + 4] = nt;
        sh[wave][kind * 6 + 5] = ct;
      }
    }
  });
  __syncthreads();
  if (threadIdx.x < BAL_WORDS) {
    const bool modular = threadIdx.x % 6 != 5;
    uint32_t v = sh[0][threadIdx.x];
    for (int w = 1; w < 4; w++) v = modular ? madd(v, sh[w][threadIdx.x]) : v + sh[w][threadIdx.x];
    slabs[(size_t)blockIdx.x * BAL_WORDS + threadIdx.x] = v;
  }
}

// out[w] = sum over the blocks' slabs of word w: one block per word.
__global__ __launch_bounds__(256) void k_balance_reduce(const uint32_t* __restrict__ slabs,
                                                        int nblocks, uint32_t* __restrict__ out) {
  __shared__ uint32_t sh[4];
  const int w = blockIdx.x;  // < BAL_WORDS
  const bool modular = w % 6 != 5;
  uint32_t v = 0;
  for (int b = threadIdx.x; b < nblocks; b += blockDim.x) {
    const uint32_t x = slabs[(size_t)b * BAL_WORDS + w];
    v = modular ? madd(v, x) : v + x;
  }
  v = wave_sum(v, modular);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t r = sh[0];
    for (int k = 1; k < 4; k++) r = modular ? madd(r, sh[k]) : r + sh[k];
    out[w] = r;
  }
}

template <int CHIP>
static void launch_balance(const uint32_t* mainc, const uint32_t* prepc, size_t h,
                           const PermChallenges* ch, uint32_t* slabs, int nblocks, hipStream_t st) {
  hipLaunchKernelGGL(k_lookup_balance<CHIP>, dim3(nblocks), dim3(256), 0, st, mainc, prepc,
                     (uint32_t)h, ch, slabs);
  KCHECK();
}

void lookup_balance_device(int chip, const uint32_t* mainc, const uint32_t* prepc, size_t h,
                           const PermChallenges* ch_dev, uint32_t* out_dev, hipStream_t st) {
  check_shape(chip, h);
  if (CHIP_INFO[chip].prep_w && !prepc) throw std::runtime_error("balance: this chip has a preprocessed trace");
  const int nblocks = (int)std::min<size_t>(ceil_div(h, 256), BAL_MAX_BLOCKS);
  DBuf<uint32_t> slabs((size_t)nblocks * BAL_WORDS);
#define BFZ_BAL_CASE(C) \
  case C: launch_balance<C>(mainc, prepc, h, ch_dev, slabs.p, nblocks, st); break;
  switch (chip) {
    BFZ_BAL_CASE(CHIP_CPU)
    BFZ_BAL_CASE(CHIP_PROGRAM)
    BFZ_BAL_CASE(CHIP_ADDSUB)
    BFZ_BAL_CASE(CHIP_JUMP)
    BFZ_BAL_CASE(CHIP_MEMORY)
    BFZ_BAL_CASE(CHIP_BYTE)
    BFZ_BAL_CASE(CHIP_MEMINSTRS)
    BFZ_BAL_CASE(CHIP_IO)
  }
#undef BFZ_BAL_CASE
  hipLaunchKernelGGL(k_balance_reduce, dim3(BAL_WORDS), dim3(256), 0, st, (const uint32_t*)slabs.p, nblocks,
                     out_dev);
  KCHECK();
}

// ------------------------------------------------------------------------ the machine's check
void debug_constraints_device(const ProvingKey& pk, const DeviceTraces& dt, Challenger& ch,
                              bool force_balance, DebugReport& out) {
  hipStream_t st = stream();
  const int nc = (int)dt.chips.size();
  if (nc == 0 || nc > NUM_CHIPS) throw std::runtime_error("debug_constraints: no traces");
  std::vector<int> ord(nc);  // shard_chips: machine order (machine.rs:306)
  std::iota(ord.begin(), ord.end(), 0);
  std::sort(ord.begin(), ord.end(), [&](int a, int b) { return dt.chips[a] < dt.chips[b]; });
  std::vector<const uint32_t*> preps(nc, nullptr);
  for (int k = 0; k < nc; k++) {
    const int c = dt.chips[ord[k]];
    check_shape(c, dt.heights[ord[k]]);
    const int pi = pk.idx_of_chip[c];
    if (pi >= 0) {  // the key's preprocessed trace has the program's height (machine.rs:309-312)
      if (pk.prep.mats[pi].n != dt.heights[ord[k]])
        throw std::runtime_error(std::string("debug_constraints: height of ") + CHIP_INFO[c].name +
                                 " differs from its preprocessed trace");
      preps[k] = pk.prep_evals[pi].p;
    }
  }

  // the permutation challenges: two sample_ext_element (machine.rs:300-303)
  out = DebugReport();
  out.alpha = ch.sample_ef();
  out.beta = ch.sample_ef();
  PermChallenges pc;
  pc.alpha = out.alpha;
  pc.beta_pows[0] = ef_one();
  for (int j = 1; j < 8; j++) pc.beta_pows[j] = ef_mul(pc.beta_pows[j - 1], out.beta);
  DBuf<PermChallenges> pc_d(1);
  HIP_CHECK(hipMemcpyAsync(pc_d.p, &pc, sizeof(pc), hipMemcpyHostToDevice, st));
  DBuf<EF> cums_d(nc);
  DBuf<unsigned long long> res_d(2 * (size_t)nc);
  std::vector<unsigned long long> res(2 * (size_t)nc);
  for (int k = 0; k < nc; k++) {
    res[2 * k] = ~0ull;
    res[2 * k + 1] = 0;
  }
  HIP_CHECK(hipMemcpyAsync(res_d.p, res.data(), res.size() * 8, hipMemcpyHostToDevice, st));

  // permutation trace, then the row check, chip by chip (machine.rs:319-335,369-384); a chip's
  // permutation trace is released once its check is queued
  for (int k = 0; k < nc; k++) {
    const int c = dt.chips[ord[k]];
    const size_t h = dt.heights[ord[k]];
    DBuf<uint32_t> pe(4 * (size_t)perm_width(c) * h);
    perm_trace(c, dt.evals[ord[k]].p, preps[k], h, pc_d.p, pe.p, cums_d.p + k, st);
    check_chip_device(c, dt.evals[ord[k]].p, preps[k], pe.p, h, pc_d.p, cums_d.p + k,
                      res_d.p + 2 * k, nullptr, st);
  }
  std::vector<EF> cums(nc);
  HIP_CHECK(hipMemcpyAsync(cums.data(), cums_d.p, sizeof(EF) * nc, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipMemcpyAsync(res.data(), res_d.p, res.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));

  out.cumsum = ef_zero();
  out.chips.resize(nc);
  bool rows_ok = true;
  for (int k = 0; k < nc; k++) {
    ChipCheck& cc = out.chips[k];
    fill_chip_header(dt.chips[ord[k]], dt.heights[ord[k]], cc);
    cc.cumsum = cums[k];
    decode_check_result(&res[2 * k], cc);
    rows_ok = rows_ok && cc.failing_rows == 0;
    out.cumsum = ef_add(out.cumsum, cums[k]);
  }
  const bool balanced = ef_is_zero(out.cumsum);  // machine.rs:337-349
  out.ok = rows_ok && balanced;

  if (!balanced || force_balance) {
    DBuf<uint32_t> bal_d((size_t)nc * BAL_WORDS);
    for (int k = 0; k < nc; k++)
      lookup_balance_device(dt.chips[ord[k]], dt.evals[ord[k]].p, preps[k], dt.heights[ord[k]],
                            pc_d.p, bal_d.p + (size_t)k * BAL_WORDS, st);
    std::vector<uint32_t> bal((size_t)nc * BAL_WORDS);
    HIP_CHECK(hipMemcpyAsync(bal.data(), bal_d.p, bal.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    for (int k = 0; k < nc; k++) {
      const int c = dt.chips[ord[k]];
      for (int kind = 1; kind < NUM_KINDS; kind++) {
        const uint32_t* w = &bal[(size_t)k * BAL_WORDS + kind * 6];
        std::memcpy(out.kind_sum[kind][c].c, w, 16);
        const uint32_t v = from_mont(w[4]);  // field_to_int (lookup/debug.rs:46-54)
        out.kind_net[kind][c] = v > P / 2 ? (int32_t)v - (int32_t)P : (int32_t)v;
        out.kind_count[kind][c] = w[5];
      }
    }
    out.balance_valid = true;
  }
}

}  // namespace bfz
