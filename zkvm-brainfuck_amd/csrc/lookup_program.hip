// Interaction programs on the device (lookup_program.h): k_perm_rows_prog<WRITE> does for an
// interaction list that is data what k_perm_rows<CHIP> (logup.hip) does for LookupsOf<CHIP>:
// one thread per storage position (bit-reversed row) of a column-major trace, batch b = the
// interactions 2b and 2b + 1 of the chain (logup_batch_size = 2, an odd count leaves a single),
//     perm[r][b] = sum_j (+-m_j) / (alpha + kind_j + sum_v beta^(v+1) value_jv),
// and the row's sum for the running-sum column, which perm_running_sum (logup.hip) scans
// exactly as perm_trace does.  Field arithmetic is exact, so the words equal the compiled
// kernel's bit for bit whatever the evaluation order.
//
// Design decisions:
//   Wave-uniform list.  The list is read through the constant address space (as run_program
//     reads a constraint program), so every read is a scalar load and every loop bound and
//     branch below is uniform.  The LogUp challenges are read the same way: beta^(v+1) is
//     indexed by the runtime v, and a scalar load costs no register array.
//   Trace values: one load per term, no staging.  A row's main and prep values cannot sit in a
//     runtime-indexed private array (scratch).  Staging the row in LDS would cost
//     (main + prep width) x 256 x 4 bytes per block (31 KiB for Cpu, up to 128 KiB at the
//     format's widths) to save reloads that L1 / L2 serve: a block's reads of one column are
//     1 KiB, contiguous.  So a term is one buffer load of its column at the thread's position
//     (the column in the descriptor's base, the position the 32-bit voffset), and LDS is kept
//     for the prefix file below.
//   Values and denominators.  A VCOL accumulates weight x value unreduced in 64 bits (folded
//     once after four products) and is reduced once; a denominator accumulates
//     beta^(v+1) x value_v per EF component the same way (LazyEF) and is reduced once.
//   One field inversion per row, whatever the interaction count.
//     WRITE = 1: the forward pass keeps the running prefix products of the batch denominators,
//     P_b = D_0 .. D_b, in an LDS file pre[b][component][threadIdx.x]: lane l touches bank
//     l mod 32 whatever the slot (conflict-free) and only its own column (no barrier), like the
//     interpreter's slot file.  The total P_last is inverted by the EF norm into the base field
//     and one minv (ef_inv), as the compiled kernel does.  The backward pass peels off batch b:
//     value_b = N_b x inv x P_(b-1), inv <- inv x D_b.  Of the two ways the file could fit two
//     blocks per CU, this kernel keeps ONLY the prefix in LDS and recomputes N_b and D_b in the
//     backward pass (the offset table at the head of the list reaches batch b directly): 256
//     threads x 16 batches x (numerator + prefix) would be 128 KiB, one block per CU of 160
//     KiB.  Prefix only is 4 KiB per batch, and the file is sized by the program's batch count
//     (dynamic LDS), not by the maximum: 64 KiB at 16 batches = 2 blocks (8 waves) per CU, 32
//     KiB for Cpu's 8 batches = 5 blocks, one batch = 4 KiB, where the registers bound the
//     occupancy.  The recomputation repeats the term loads (L1 / L2 hits) and the lazy dot
//     products, not the inversion; 128-thread blocks would have kept the loads single at half
//     the waves per block for the same two blocks per CU.
//     WRITE = 0 (the balance check: the row sums alone) needs no file and no second pass: the
//     row's sum is accumulated as one fraction, (N, D) <- (N D_b + N_b D, D D_b), and
//     N / D takes the same single inversion.  No LDS; the registers bound the occupancy.
//   Running sum.  rowsum[t] goes through perm_running_sum: k_phi_sums / ef_inclusive_scan /
//     k_phi_write from 2^11 rows, k_scan_block / k_write_phi below; without a permutation
//     trace only the block sums are scanned and the last one is the cumulative sum.
//   No scratch: every array index that survives unrolling is an LDS or global address.
// The vcol / interaction walkers are in lookup_program_dev.h (chip_program.hip reads lists too).
#include "lookup_program.h"

#include "lookup_program_dev.h"

namespace bfz {

using namespace kb;

// perm: 4 * (batches + 1) base columns of n rows (WRITE = 1; the last EF column is written by
// perm_running_sum); rowsum[t]: the sum of row t's batch values.  Dynamic LDS: batches x 4 x
// LKP_T words with WRITE = 1, none with WRITE = 0.  A zero denominator is not detected: its
// inverse is taken as 0, which zeroes the row's values (as a zero norm does in k_perm_rows).
template <int WRITE>
__global__ __launch_bounds__(LKP_T) void k_perm_rows_prog(const uint32_t* __restrict__ list,
                                                          const uint32_t* __restrict__ mainc,
                                                          const uint32_t* __restrict__ prepc,
                                                          size_t n,
                                                          const PermChallenges* __restrict__ chp,
                                                          uint32_t* __restrict__ perm,
                                                          EF* __restrict__ rowsum) {
  extern __shared__ uint32_t pre[];  // [batch][component][LKP_T]
  const size_t t = (size_t)blockIdx.x * LKP_T + threadIdx.x;
  if (t >= n) return;  // (no barrier below)
  const uint32_t tid = threadIdx.x;
  const RowCtx c{(ConstWords)list, (ConstWords)chp, mainc, prepc, n, (uint32_t)t * 4u};
  const int ni = (int)c.list[0], nb = (ni + 1) >> 1;

  // forward: the prefix products of the batch denominators (WRITE) or the row's one fraction
  EF P, N;
  int at = LKP_HEAD;
  for (int b = 0; b < nb; b++) {
    EF num, den;
    batch_frac(c, at, 2 * b + 1 < ni, num, den);
    if (b == 0) {
      N = num;
      P = den;
    } else {
      if (!WRITE) N = ef_add(ef_mul(N, den), ef_mul(num, P));
      P = ef_mul(P, den);
    }
    if (WRITE) {
#pragma unroll
      for (int e = 0; e < 4; e++) pre[(4 * b + e) * LKP_T + tid] = P.c[e];
    }
  }
  EF inv = ef_inv(P);  // the row's one inversion: the norm into the base field, one minv
  EF sum;
  if (!WRITE) {
    sum = ef_mul(N, inv);
  } else {
    sum = ef_zero();
    for (int b = nb - 1; b >= 0; b--) {  // backward: value_b = N_b inv P_(b-1), inv <- inv D_b
      at = (int)c.list[1 + b];
      EF num, den;
      batch_frac(c, at, 2 * b + 1 < ni, num, den);
      EF v;
      if (b) {
        EF pp;
#pragma unroll
        for (int e = 0; e < 4; e++) pp.c[e] = pre[(4 * (b - 1) + e) * LKP_T + tid];
        v = ef_mul(num, ef_mul(inv, pp));
        inv = ef_mul(inv, den);
      } else {
        v = ef_mul(num, inv);
      }
#pragma unroll
      for (int e = 0; e < 4; e++) st_b(rsrc_of(perm + (size_t)(4 * b + e) * n), c.vt, 0, v.c[e]);
      sum = ef_add(sum, v);
    }
  }
  rowsum[t] = sum;
}

// One wave: total = the sum of n EF values (lane-strided partial sums, then a shuffle tree).
__global__ __launch_bounds__(64) void k_ef_total(const EF* __restrict__ vals, uint32_t n,
                                                 EF* __restrict__ total) {
  EF s = ef_zero();
  for (uint32_t i = threadIdx.x; i < n; i += 64) s = ef_add(s, vals[i]);
  for (int off = 32; off; off >>= 1) {
#pragma unroll
    for (int e = 0; e < 4; e++) s.c[e] = madd(s.c[e], __shfl_down(s.c[e], off, 64));
  }
  if (threadIdx.x == 0) *total = s;
}

void perm_rows_prog(const LookupProgram& p, const uint32_t* list_dev, const uint32_t* mainc,
                    const uint32_t* prepc, size_t n, const PermChallenges* ch, uint32_t* perm,
                    EF* rowsum, hipStream_t st) {
  if (p.prep_w && !prepc) throw std::runtime_error("lookups: the program has preprocessed columns");
  if (n == 0 || (n & (n - 1)) || n > ((size_t)1 << 23))
    throw std::runtime_error("lookups: height not a power of two in [1, 2^23]");
  const dim3 grid(ceil_div(n, LKP_T)), block(LKP_T);
  if (perm) {
    const size_t lds = (size_t)p.batches() * 4 * LKP_T * sizeof(uint32_t);  // at most 64 KiB
    hipLaunchKernelGGL(k_perm_rows_prog<1>, grid, block, lds, st, list_dev, mainc, prepc, n, ch,
                       perm, rowsum);
  } else {
    hipLaunchKernelGGL(k_perm_rows_prog<0>, grid, block, 0, st, list_dev, mainc, prepc, n, ch,
                       perm, rowsum);
  }
  KCHECK();
}

void perm_trace_prog(const LookupProgram& p, const uint32_t* list_dev, const uint32_t* mainc,
                     const uint32_t* prepc, size_t n, const PermChallenges* ch, uint32_t* perm,
                     EF* cumsum_dev, hipStream_t st) {
  DBuf<EF> rows(n);
  perm_rows_prog(p, list_dev, mainc, prepc, n, ch, perm, rows.p, st);
  perm_running_sum(rows.p, n, perm, 4 * p.batches(), cumsum_dev, st);
}

void ef_total(const EF* vals, size_t n, EF* total_dev, hipStream_t st) {
  hipLaunchKernelGGL(k_ef_total, dim3(1), dim3(64), 0, st, vals, (uint32_t)n, total_dev);
  KCHECK();
}

// kernels a permutation trace or a balance check of a program launches (gpu.h PreloadKernels)
static PreloadKernels preload_lookup_program{(const void*)&k_perm_rows_prog<0>,
                                             (const void*)&k_perm_rows_prog<1>,
                                             (const void*)&k_ef_total};

}  // namespace bfz
