// Constraint programs on the device (air_program.h): one interpreter, run_program<Sink>, and the
// two kernels around it -- k_quotient_prog<LQD> with the frame of k_quotient_air<CHIP, LQD>
// (quotient.hip) and k_check_prog with the frame of k_check_air<CHIP> (debug_check.hip) -- and
// k_quotient_prog_coset, the quotient frame on a coset slab of the larger quotient domain an AIR
// of degree 4 to 9 needs (uni_stark.hip quotient_slabs).
//
// The compiled list is wave-uniform: it is read through the constant address space (as PowAcc
// reads the alpha powers), so the reads are scalar loads, and decoded with a switch.  The values
// live in a slot file; a private array indexed by the instruction's fields would be
// runtime-indexed and go to scratch, so the file is in LDS, slots[slot][threadIdx.x]: lane l of
// a wave reads bank l mod 32 whatever the slot (conflict-free), and a thread touches its own
// column only, so no barrier is needed.  A LOCAL / NEXT instruction is one buffer load of its
// column at the thread's position.  Field arithmetic is exact, so a constraint's canonical value
// does not depend on the order the compiled template or this interpreter evaluates it in.
#include "air_program.h"

#include "air_program_dev.h"
#include "debug_check.h"
#include "quotient.h"

namespace bfz {

using namespace kb;

// run_program<Sink> and FirstFailSink are in air_program_dev.h (chip_program.hip runs them too).

template <int LQD>
__global__ __launch_bounds__(256) void k_quotient_prog(const uint32_t* __restrict__ code, int ncode,
                                                       const uint32_t* __restrict__ mainc, int logN,
                                                       const QuotParams* __restrict__ qpp,
                                                       const uint32_t* __restrict__ twf,
                                                       const uint32_t* __restrict__ sel_inv,
                                                       QuotOut qo) {
  __shared__ uint32_t slots[BFZ_AIR_MAX_LIVE][256];
  const QuotParams qp = *qpp;
  const size_t N = (size_t)1 << logN, n = N >> 1;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (n << LQD)) return;  // (no barrier below)
  const uint32_t i = dbitrev((uint32_t)t, logN);
  const uint32_t inext = (i + 2) & (uint32_t)(N - 1);
  const uint32_t vt = (uint32_t)t * 4u, vn = dbitrev(inext, logN) * 4u;

  const uint32_t x = quot_point(i, (uint32_t)n, qp.shift, twf);
  const uint32_t zh = (i & 1) ? qp.zh_odd : qp.zh_even;
  const uint32_t zh_inv = (i & 1) ? qp.zh_odd_inv : qp.zh_even_inv;
  const uint32_t a = msub(x, ONE), b = msub(x, qp.wn_inv);
  const uint32_t zi = mmul(zh, sel_inv[t]);
  const uint32_t is_first = mmul(zi, b), is_last = mmul(zi, a), is_trans = b;

  PowAcc acc{{0, 0, 0, 0}, 0, (ConstWords)qp.alpha_pows, 0};
  run_program((ConstWords)code, ncode, slots, mainc, N, vt, vn, is_first, is_last, is_trans, acc);
  const EF q = ef_mul_base(acc.value(), zh_inv);
  const size_t chunk = LQD ? t >> (logN - 1) : 0, pos = t & (n - 1);
#pragma unroll
  for (int e = 0; e < 4; e++) qo.chunk[chunk][e * qo.stride + pos] = q.c[e];
}

// block_inverse is in air_program_dev.h (machine_program.hip runs it too).

// k_quotient_prog<1> on a coset slab S_r = 3 g^r H_2n, r >= 1, of the quotient domain 3 H_(D n)
// (air_program.h SlabParams): one thread per slab point, the slot file and the scalar list as
// above, the trace's next row at i + 2.  What differs from the frame on 3 H_2n: the point is
// sp.shift w_2n^i, Z_H takes the slab's two values, and the selector denominators
// (x - 1)(x - w_n^-1), which quotient_sel_inv tabulates for 3 H_N alone, are inverted here, one
// inversion per block (block_inverse; a slab is disjoint from H_n, so none is zero).  A thread past
// the slab (n = 1 .. 64: a partial block) brings the denominator 1 and stops after the barriers.
// LDS: 32 KiB of slots + 20 bytes, the occupancy of k_quotient_prog.
__global__ __launch_bounds__(256) void k_quotient_prog_coset(const uint32_t* __restrict__ code,
                                                             int ncode,
                                                             const uint32_t* __restrict__ slab,
                                                             int logN,
                                                             const SlabParams* __restrict__ spp,
                                                             const uint32_t* __restrict__ twf,
                                                             QuotOut qo) {
  __shared__ uint32_t slots[BFZ_AIR_MAX_LIVE][256];
  __shared__ uint32_t s_wave[4], s_tinv;
  const SlabParams sp = *spp;
  const size_t N = (size_t)1 << logN, n = N >> 1;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool has_point = t < N;
  const uint32_t i = dbitrev(has_point ? (uint32_t)t : 0u, logN);  // in bounds whatever t
  const uint32_t x = quot_point(i, (uint32_t)n, sp.shift, twf);
  const uint32_t a = msub(x, ONE), b = msub(x, sp.wn_inv);
  const uint32_t inv_ab = block_inverse(has_point ? mmul(a, b) : ONE, s_wave, &s_tinv);
  if (!has_point) return;  // (no barrier below)

  const uint32_t inext = (i + 2) & (uint32_t)(N - 1);
  const uint32_t vt = (uint32_t)t * 4u, vn = dbitrev(inext, logN) * 4u;
  const uint32_t zh = (i & 1) ? sp.zh_odd : sp.zh_even;
  const uint32_t zh_inv = (i & 1) ? sp.zh_odd_inv : sp.zh_even_inv;
  const uint32_t zi = mmul(zh, inv_ab);
  const uint32_t is_first = mmul(zi, b), is_last = mmul(zi, a), is_trans = b;

  PowAcc acc{{0, 0, 0, 0}, 0, (ConstWords)sp.alpha_pows, 0};
  run_program((ConstWords)code, ncode, slots, slab, N, vt, vn, is_first, is_last, is_trans, acc);
  const EF q = ef_mul_base(acc.value(), zh_inv);
  // even i (t < n): chunk r, odd i: chunk r + D/2; position bitrev(i >> 1) = t mod n
  const size_t half = t >> (logN - 1), pos = t & (n - 1);
#pragma unroll
  for (int e = 0; e < 4; e++) qo.chunk[half][e * qo.stride + pos] = q.c[e];
}

__global__ __launch_bounds__(256) void k_check_prog(const uint32_t* __restrict__ code, int ncode,
                                                    const uint32_t* __restrict__ mainc, uint32_t n,
                                                    int logn, int K,
                                                    unsigned long long* __restrict__ res,
                                                    int32_t* __restrict__ per_row) {
  __shared__ uint32_t slots[BFZ_AIR_MAX_LIVE][256];
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  int idx = -1;
  uint32_t i = 0;
  if (t < n) {  // (no early return: every thread takes part in the block reduction)
    i = dbitrev(t, logn);
    const uint32_t tn = dbitrev((i + 1) & (n - 1), logn);  // h = 1: the row is its own next
    FirstFailSink sink;
    run_program((ConstWords)code, ncode, slots, mainc, n, t * 4u, tn * 4u, i == 0 ? ONE : 0u,
                i == n - 1 ? ONE : 0u, i == n - 1 ? 0u : ONE, sink);
    idx = sink.first;
    if (per_row) per_row[t] = idx;
  }
  reduce_failures(idx, i, K, res);
}

// k_profile_prog: k_check_prog's frame with the profile's sink (debug_check.h).  The block's
// count[K] / first[K] tables follow the slot file in LDS: 32 KiB + 4 KiB + reduce_failures' 48
// bytes = 36912 static, 4 blocks (16 waves) per CU of 160 KiB -- what k_check_prog's 32816 bytes
// give it, so the tables cost no occupancy.  sink.n advances with the wave-uniform list, so the
// table index is a scalar.  A thread past the last row interprets row 0 and is ignored: every
// lane reaches every EMIT, and the slot file is per thread as before.
__global__ __launch_bounds__(256) void k_profile_prog(const uint32_t* __restrict__ code, int ncode,
                                                      const uint32_t* __restrict__ mainc,
                                                      uint32_t n, int logn, int K,
                                                      unsigned long long* __restrict__ res) {
  __shared__ uint32_t slots[BFZ_AIR_MAX_LIVE][256];
  __shared__ uint32_t s_cnt[BFZ_AIR_MAX_CONSTRAINTS], s_fst[BFZ_AIR_MAX_CONSTRAINTS];
  profile_clear(s_cnt, s_fst, K);
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const bool has_row = t < n;
  const uint32_t ts = has_row ? t : 0;  // in bounds whatever t
  const uint32_t i = dbitrev(ts, logn);
  const uint32_t tn = dbitrev((i + 1) & (n - 1), logn);  // h = 1: the row is its own next
  ProfileSink sink{s_cnt, s_fst, has_row ? i : PROFILE_NO_ROW};
  run_program((ConstWords)code, ncode, slots, mainc, n, ts * 4u, tn * 4u, i == 0 ? ONE : 0u,
              i == n - 1 ? ONE : 0u, i == n - 1 ? 0u : ONE, sink);
  profile_flush(s_cnt, s_fst, K, res + 2);
  reduce_failures(sink.first, i, K, res);
}

void launch_quotient_prog(int lqd, const uint32_t* code_dev, int ncode, const uint32_t* mainc,
                          int logN, const QuotParams* qp_dev, const uint32_t* twf,
                          const uint32_t* sel_inv, const QuotOut& qo, hipStream_t st) {
  const size_t count = ((size_t)1 << (logN - 1)) << lqd;
  if (lqd == 0)
    hipLaunchKernelGGL(k_quotient_prog<0>, dim3(ceil_div(count, 256)), dim3(256), 0, st, code_dev,
                       ncode, mainc, logN, qp_dev, twf, sel_inv, qo);
  else
    hipLaunchKernelGGL(k_quotient_prog<1>, dim3(ceil_div(count, 256)), dim3(256), 0, st, code_dev,
                       ncode, mainc, logN, qp_dev, twf, sel_inv, qo);
  KCHECK();
}

void launch_quotient_prog_coset(const uint32_t* code_dev, int ncode, const uint32_t* slab, int logN,
                                const SlabParams* sp_dev, const uint32_t* twf, const QuotOut& qo,
                                hipStream_t st) {
  if (logN < 1 || logN > 24) throw std::runtime_error("quotient_prog: bad LDE height");
  const size_t count = (size_t)1 << logN;
  hipLaunchKernelGGL(k_quotient_prog_coset, dim3(ceil_div(count, 256)), dim3(256), 0, st, code_dev,
                     ncode, slab, logN, sp_dev, twf, qo);
  KCHECK();
}

void launch_check_prog(const uint32_t* code_dev, int ncode, const uint32_t* mainc, size_t h, int K,
                       unsigned long long* res_dev, int32_t* per_row_dev, hipStream_t st) {
  hipLaunchKernelGGL(k_check_prog, dim3(ceil_div(h, 256)), dim3(256), 0, st, code_dev, ncode, mainc,
                     (uint32_t)h, log2i(h), K, res_dev, per_row_dev);
  KCHECK();
}

void launch_profile_prog(const uint32_t* code_dev, int ncode, const uint32_t* mainc, size_t h, int K,
                         unsigned long long* res_dev, hipStream_t st) {
  if (K < 1 || K > BFZ_AIR_MAX_CONSTRAINTS)
    throw std::runtime_error("check: the program's constraint count is outside the profile's table");
  hipLaunchKernelGGL(k_profile_prog, dim3(ceil_div(h, 256)), dim3(256), 0, st, code_dev, ncode,
                     mainc, (uint32_t)h, log2i(h), K, res_dev);
  KCHECK();
}

// kernels a proof or a check of a program launches (gpu.h PreloadKernels)
static PreloadKernels preload_air_program{(const void*)&k_quotient_prog<0>,
                                          (const void*)&k_quotient_prog<1>,
                                          (const void*)&k_quotient_prog_coset,
                                          (const void*)&k_check_prog,
                                          (const void*)&k_profile_prog};

}  // namespace bfz
