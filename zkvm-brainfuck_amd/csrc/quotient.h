// Device quotient evaluation (see quotient.hip).
#pragma once
#include "gpu.h"
#include "machine.h"
#include "logup.h"

namespace bfz {

struct QuotParams {
  kb::EF perm_alpha;
  kb::EF beta_pows[8];
  kb::EF cumsum;
  const kb::EF* alpha_pows;  // device array: alpha^(K-1-k), k = 0..K-1
  uint32_t zh_even, zh_odd, zh_even_inv, zh_odd_inv;  // Z_H at even / odd natural index
  uint32_t wn_inv;  // w_n^-1
  uint32_t shift;   // GENERATOR = 3
};
// The challenge-independent fields for a trace of n rows (quotient domain 3 H_2n); the rest zero.
inline QuotParams quot_params_of_height(size_t n, const kb::EF* alpha_pows) {
  using namespace kb;
  QuotParams qp{};
  qp.alpha_pows = alpha_pows;
  const uint32_t three = to_mont(3);
  const uint32_t sn = mpow(three, n);
  qp.zh_even = msub(sn, ONE);
  qp.zh_odd = msub(mneg(sn), ONE);
  qp.zh_even_inv = minv(qp.zh_even);
  qp.zh_odd_inv = minv(qp.zh_odd);
  qp.wn_inv = minv(two_adic_gen(log2i(n)));
  qp.shift = three;
  return qp;
}

// Number of constraints (AIR + LogUp) emitted by a chip's eval.
int num_constraints(int chip);

// Writes Q at all 2n points into qout: 8 base columns of n rows (chunk k, coefficient e at
// column 4k+e), rows in bit-reversed order of the chunk domain.
// Builds (once per process) the selector-denominator table of the quotient domain 3 H_N, N = 2^logN.
void prepare_quotient_tables(int logN);
void quotient(int chip, const uint32_t* mainc, const uint32_t* prepc, const uint32_t* permc,
              int logN, const QuotParams& qp, uint32_t* qout, hipStream_t st);

// Row-range form (sharded proofs): LDE positions [t0, t0 + count) only.  Every
// pointer is indexed by the GLOBAL position: column c of main/perm at ptr[c * stride + t]
// (a shard buffer passes its base minus its first position), prep at prep[c * N + t] (full).
// main_l/perm_l serve the points' own rows, main_n/perm_n their next rows (i + 2); in the
// unsharded form both are the full LDE (identity column maps); a sharded proof's next-row
// shards hold only the columns the chip reads at the next row.  qout is the full 8 x n chunk buffer; only the
// range's entries are written.
struct QuotRows {
  const uint32_t *main_l, *main_n, *perm_l, *perm_n, *prep;
  size_t stride, t0, count;
  uint8_t nmain[64], nperm[64];  // column c's next row: main_n / perm_n column nmain[c] / nperm[c]
};
// qp_dev: the same parameters in device memory (nullptr: qp is uploaded for the launch).
void quotient_rows(int chip, const QuotRows& in, int logN, const QuotParams& qp, uint32_t* qout,
                   hipStream_t st, const QuotParams* qp_dev = nullptr);
// Output placement: chunk k's coefficient column e at chunk[k] + e * stride (row = position
// within the chunk).  qout above is {qout, qout + 4n}, stride n; the single-GPU prover writes
// each chunk straight into its own half of the chunk's LDE buffer ({lde0, lde1 + n}, stride 2n).
struct QuotOut {
  uint32_t* chunk[2];
  size_t stride;
};
void quotient_into(int chip, const QuotRows& in, int logN, const QuotParams& qp, const QuotOut& out,
                   hipStream_t st, const QuotParams* qp_dev = nullptr);
// The AIR-only quotient of one chip's trace (uni_stark.hip; k_quotient_air): mainc = the trace's
// whole LDE (column-major, 2^logN rows), lqd = the chip's log quotient degree (0: one chunk
// over the LDE's first half, 1: two chunks over all of it).  Of qp only alpha_pows (K powers,
// alpha^(K-1-k)), zh_*, wn_inv and shift are read; qp_dev is the same in device memory.
void quotient_air(int chip, int lqd, const uint32_t* mainc, int logN, const QuotParams& qp,
                  const QuotParams* qp_dev, const QuotOut& out, hipStream_t st);
// The same for a compiled constraint program (air_program.h): code_dev = its instruction list in
// device memory, ncode words.
void quotient_prog(const uint32_t* code_dev, int ncode, int lqd, const uint32_t* mainc, int logN,
                   const QuotParams& qp, const QuotParams* qp_dev, const QuotOut& out,
                   hipStream_t st);
// Constraints Air::eval_air<chip> emits, their maximal degree and log2_ceil(degree - 1)
// (chip.rs:82-87), computed from air.h.  false: the chip has no AIR constraints of its own.
bool uni_air_shape(int chip, int* num_constraints, int* degree, int* log_quotient_degree);

// The quotient challenge on the device after the LogUp commit (see k_challenge_quot): ch is the
// device sponge (updated), root the permutation root, cums the chips' cumulative sums, pc the
// LogUp challenges; qps[k]'s perm_alpha / beta_pows / cumsum and apows[k] (K[k] powers) are
// written.  The host replays the step when it fetches the roots.
constexpr int QUOT_MAX_CHIPS = 8;
struct QuotAlphaTargets {
  kb::EF* apows[QUOT_MAX_CHIPS];
  int K[QUOT_MAX_CHIPS];
  kb::EF* alpha_out;  // optional: the sampled alpha itself (checked against the host replay)
};
void challenge_quot(DevChallenger* ch, const uint32_t* root, const kb::EF* cums, int nc,
                    const PermChallenges* pc, QuotParams* qps, const QuotAlphaTargets& tg,
                    hipStream_t st);

#if defined(__HIPCC__)
// ---- device helpers shared by the quotient kernels (quotient.hip, air_program.hip)
// Lazy fold of the constraints: raw 64-bit products of Montgomery values accumulate with
// v_mad_u64_u32 (a base constraint times its EF alpha power is one multiply-add per
// component instead of a Montgomery product + modular add).  Budget: a raw product is < p^2
// (1 unit), a reduced EF term added at scale 2^32 is < 2 p^2 (2 units); the accumulator is
// folded (hi * (2^32 mod p) + lo < 2^57) before 4 units would be exceeded (4 p^2 + 2^57 <
// 2^64), and reduced once at the end -- the same field element as the eager sum.
struct PowAcc {
  static constexpr uint32_t C32 = (1u << 25) - 2;  // 2^32 mod p
  uint64_t a64[4];
  int units;
  // alpha powers, read through the constant address space: the pointer now comes from device
  // memory (QuotParams), and through a generic pointer the reads became vector flat loads (+19
  // VGPRs, k_quotient<0> 930 -> 1031 us); as constant-space loads they stay scalar.
  const __attribute__((address_space(4))) uint32_t* ap;
  int k;
  __device__ __forceinline__ kb::EF pow_k() {
    kb::EF a;
#pragma unroll
    for (int e = 0; e < 4; e++) a.c[e] = ap[4 * k + e];
    k++;
    return a;
  }
  __device__ __forceinline__ void fold() {
#pragma unroll
    for (int e = 0; e < 4; e++) a64[e] = (uint64_t)(uint32_t)(a64[e] >> 32) * C32 + (uint32_t)a64[e];
    units = 0;
  }
  __device__ __forceinline__ void emit(uint32_t c) {
    if (units + 1 > 4) fold();
    const kb::EF a = pow_k();
#pragma unroll
    for (int e = 0; e < 4; e++) a64[e] += (uint64_t)a.c[e] * c;
    units += 1;
  }
  __device__ __forceinline__ void emit_ext(const kb::EF& c) {
    if (units + 2 > 4) fold();
    const kb::EF r = kb::ef_mul(pow_k(), c);
#pragma unroll
    for (int e = 0; e < 4; e++) a64[e] += (uint64_t)r.c[e] << 32;
    units += 2;
  }
  __device__ __forceinline__ kb::EF value() {
    fold();
    kb::EF r;
#pragma unroll
    for (int e = 0; e < 4; e++) r.c[e] = kb::mred_lt_p(a64[e]);  // folded: < 2^57
    return r;
  }
};

// x_i = 3 w_N^i, the natural point i of the quotient domain 3 H_N (twf[N/2 + j] = w_N^j).
__device__ __forceinline__ uint32_t quot_point(uint32_t i, uint32_t half, uint32_t shift,
                                               const uint32_t* __restrict__ twf) {
  const uint32_t w = i < half ? twf[half + i] : kb::mneg(twf[i]);  // twf[half + (i - half)]
  return kb::mmul(shift, w);
}
#endif

}  // namespace bfz
