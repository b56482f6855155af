// Chip programs on the device (chip_program.h): Chip::eval (chip.rs:222-228) of a caller-defined
// chip, whose AIR is a constraint program and whose sends and receives are an interaction
// program.  One routine, perm_constraints<Sink>, evaluates eval_permutation_constraints
// (permutation.rs:157-272) of an interaction list at the thread's position, in the order
// Air::eval_perm<CHIP> (air.h) emits it:
//     per batch b     d0 d1 perm_l[b] - (m0 d1 + m1 d0)            (a single: d0 perm_l[b] - m0)
//     first-row       first (phi_l - sum_b perm_l[b])
//     transition      trans (phi_n - phi_l - sum_b perm_n[b])
//     last-row        last  (phi_l - cumsum)
// and two kernels run it after the AIR's interpreter (air_program_dev.h run_program) into one
// sink: k_quotient_chip_prog<HAS_AIR> with the frame of k_quotient<CHIP> (quotient.hip) and
// PowAcc over K alpha powers, k_check_chip_prog<HAS_AIR> with the frame of k_check<CHIP>
// (debug_check.hip) and FirstFailSink.  Field arithmetic is exact and every helper returns
// canonical words, so a quotient word equals the compiled kernel's whatever the evaluation order.
//
// Design decisions:
//   Wave-uniform list.  The list, the LogUp challenges and the cumulative sum are read through
//     the constant address space (lookup_program_dev.h's vcol / interaction walkers, the ones
//     k_perm_rows_prog uses): scalar loads, and the batch loop, the pair / single branch and the
//     sink's fold branch are uniform.  QuotParams begins with PermChallenges' words (alpha, then
//     beta^0..7), so the quotient kernel hands the walkers its parameter block as it is.
//   Cleared denominators: no inversion and no LDS in this part.  A batch costs one EF product
//     d0 d1, one EF product with perm_l[b] and -- the multiplicities being base-field words --
//     two ef_mul_base for the numerator, not EF products.  k_perm_rows_prog's prefix file and
//     its one inversion per row have no counterpart here.
//   No runtime-indexed private arrays.  perm_l[b] / perm_n[b] are buffer loads of base column
//     4 b + e, the column in the descriptor's base and the position in the voffset, exactly as
//     the walkers load a term; the batch index never indexes a register array.  sum_b perm_l[b]
//     and sum_b perm_n[b] are two running EF sums in registers, phi_l / phi_n are loaded after
//     the loop.  private_segment_fixed_size is 0 for the four instantiations.
//   Column count.  A permutation trace has up to 17 EF = 68 base columns (BFZ_LOOKUPS_MAX = 32),
//     more than QuotRows' 64-entry column maps hold: the kernels take the three matrices as
//     plain column-major pointers with one stride (the whole LDE, unsharded) and compute every
//     column base from the batch index.
//   Two phases, one accumulator.  Phase 1 is run_program over the main matrix with the 32 KiB
//     LDS slot file; phase 2 is perm_constraints over main, prep and perm.  The slot file is dead
//     in phase 2 and phase 2's registers are dead in phase 1; only the sink (8 VGPRs of PowAcc)
//     lives across.  HAS_AIR = 0 (a lookup-only chip: Program, Memory, Byte shapes) declares no
//     slot file at all, so such a chip is not held to 4 blocks per CU by LDS it never touches:
//     its occupancy is bounded by registers alone.
//   The next row's main values are not read in phase 2: interactions are over the local row
//     (permutation.rs:180-183,219-231); only perm_n is a next-row load.
#include "chip_program.h"

#include "chip_program_dev.h"  // perm_constraints, shared with machine_program.hip

namespace bfz {

using namespace kb;

// One thread per storage position t of the LDEs on 3 H_2n (N = 2^logN rows each): natural index
// i = bitrev(t), next row i + 2 mod N; selectors, Z_H and the output placement as k_quotient.
template <int HAS_AIR>
__global__ __launch_bounds__(256) void k_quotient_chip_prog(ChipLists cl,
                                                            const uint32_t* __restrict__ mainc,
                                                            const uint32_t* __restrict__ prepc,
                                                            const uint32_t* __restrict__ permc,
                                                            int logN,
                                                            const QuotParams* __restrict__ qpp,
                                                            const uint32_t* __restrict__ twf,
                                                            const uint32_t* __restrict__ sel_inv,
                                                            QuotOut qo) {
  uint32_t(*slots)[256] = nullptr;
  if constexpr (HAS_AIR) {
    __shared__ uint32_t file[BFZ_AIR_MAX_LIVE][256];
    slots = file;
  }
  const QuotParams qp = *qpp;  // device memory; uniform: scalar loads of the fields read below
  const size_t N = (size_t)1 << logN, n = N >> 1;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= N) return;  // (no barrier below)
  const uint32_t i = dbitrev((uint32_t)t, logN);
  const uint32_t inext = (i + 2) & (uint32_t)(N - 1);
  const uint32_t vt = (uint32_t)t * 4u, vn = dbitrev(inext, logN) * 4u;  // t < 2^24

  const uint32_t x = quot_point(i, (uint32_t)n, qp.shift, twf);
  const uint32_t zh = (i & 1) ? qp.zh_odd : qp.zh_even;
  const uint32_t zh_inv = (i & 1) ? qp.zh_odd_inv : qp.zh_even_inv;
  const uint32_t a = msub(x, ONE), b = msub(x, qp.wn_inv);
  const uint32_t zi = mmul(zh, sel_inv[t]);
  const uint32_t is_first = mmul(zi, b), is_last = mmul(zi, a), is_trans = b;

  PowAcc acc{{0, 0, 0, 0}, 0, (ConstWords)qp.alpha_pows, 0};
  if constexpr (HAS_AIR)  // phase 1: the AIR's K_air constraints
    run_program((ConstWords)cl.code, cl.ncode, slots, mainc, N, vt, vn, is_first, is_last, is_trans,
                acc);
  // phase 2: batches + 3 LogUp constraints
  const ConstWords qw = (ConstWords)(const uint32_t*)qpp;
  const RowCtx c{(ConstWords)cl.list, qw, mainc, prepc, N, vt};
  perm_constraints(c, permc, vn, qw + QP_CUMSUM_WORD, is_first, is_last, is_trans, acc);

  const EF q = ef_mul_base(acc.value(), zh_inv);
  const size_t chunk = t >> (logN - 1), pos = t & (n - 1);
#pragma unroll
  for (int e = 0; e < 4; e++) qo.chunk[chunk][e * qo.stride + pos] = q.c[e];
}

// The trace domain: row (i + 1) mod n is next (h = 1: the row is its own next), the selectors are
// 0 / 1 and is_transition = 1 - is_last (debug.rs:43-94).  Every thread reaches reduce_failures.
template <int HAS_AIR>
__global__ __launch_bounds__(256) void k_check_chip_prog(ChipLists cl,
                                                         const uint32_t* __restrict__ mainc,
                                                         const uint32_t* __restrict__ prepc,
                                                         const uint32_t* __restrict__ permc,
                                                         uint32_t n, int logn,
                                                         const PermChallenges* __restrict__ chp,
                                                         const EF* __restrict__ cumsum,
                                                         unsigned long long* __restrict__ res,
                                                         int32_t* __restrict__ per_row) {
  uint32_t(*slots)[256] = nullptr;
  if constexpr (HAS_AIR) {
    __shared__ uint32_t file[BFZ_AIR_MAX_LIVE][256];
    slots = file;
  }
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  int idx = -1;
  uint32_t i = 0;
  if (t < n) {  // (no early return: every thread takes part in the block reduction)
    i = dbitrev(t, logn);
    const uint32_t vt = t * 4u, vn = dbitrev((i + 1) & (n - 1), logn) * 4u;  // t < n <= 2^23
    const uint32_t first = i == 0 ? ONE : 0u, last = i == n - 1 ? ONE : 0u,
                   trans = i == n - 1 ? 0u : ONE;
    FirstFailSink sink;
    if constexpr (HAS_AIR)
      run_program((ConstWords)cl.code, cl.ncode, slots, mainc, n, vt, vn, first, last, trans, sink);
    const RowCtx c{(ConstWords)cl.list, (ConstWords)(const uint32_t*)chp, mainc, prepc, n, vt};
    perm_constraints(c, permc, vn, (ConstWords)(const uint32_t*)cumsum, first, last, trans, sink);
    idx = sink.first;
    if (per_row) per_row[t] = idx;
  }
  reduce_failures(idx, i, cl.num_constraints, res);
}

void launch_quotient_chip_prog(const ChipLists& cl, const uint32_t* mainc, const uint32_t* prepc,
                               const uint32_t* permc, int logN, const QuotParams* qp_dev,
                               const uint32_t* twf, const uint32_t* sel_inv, const QuotOut& qo,
                               hipStream_t st) {
  if (!cl.list || !mainc || !permc || !qp_dev)
    throw std::runtime_error("chip program: null device argument");
  const dim3 grid(ceil_div((size_t)1 << logN, 256)), block(256);
  if (cl.ncode > 0 && cl.code)
    hipLaunchKernelGGL(k_quotient_chip_prog<1>, grid, block, 0, st, cl, mainc, prepc, permc, logN,
                       qp_dev, twf, sel_inv, qo);
  else
    hipLaunchKernelGGL(k_quotient_chip_prog<0>, grid, block, 0, st, cl, mainc, prepc, permc, logN,
                       qp_dev, twf, sel_inv, qo);
  KCHECK();
}

void check_chip_prog_device(const ChipLists& cl, const uint32_t* mainc, const uint32_t* prepc,
                            const uint32_t* permc, size_t h, const PermChallenges* ch_dev,
                            const EF* cumsum_dev, unsigned long long* res_dev, int32_t* per_row_dev,
                            hipStream_t st) {
  if (h < 1 || (h & (h - 1)) || h > ((size_t)1 << 23))
    throw std::runtime_error("chip program: height not a power of two in [1, 2^23]");
  if (!cl.list || !mainc || !permc || !ch_dev || !cumsum_dev || !res_dev)
    throw std::runtime_error("chip program: null device argument");
  const dim3 grid(ceil_div(h, 256)), block(256);
  if (cl.ncode > 0 && cl.code)
    hipLaunchKernelGGL(k_check_chip_prog<1>, grid, block, 0, st, cl, mainc, prepc, permc,
                       (uint32_t)h, log2i(h), ch_dev, cumsum_dev, res_dev, per_row_dev);
  else
    hipLaunchKernelGGL(k_check_chip_prog<0>, grid, block, 0, st, cl, mainc, prepc, permc,
                       (uint32_t)h, log2i(h), ch_dev, cumsum_dev, res_dev, per_row_dev);
  KCHECK();
}

// kernels a quotient or a check of a chip program launches (gpu.h PreloadKernels)
static PreloadKernels preload_chip_program{
    (const void*)&k_quotient_chip_prog<0>, (const void*)&k_quotient_chip_prog<1>,
    (const void*)&k_check_chip_prog<0>, (const void*)&k_check_chip_prog<1>};

}  // namespace bfz
