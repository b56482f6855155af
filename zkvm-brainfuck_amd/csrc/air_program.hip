// Constraint programs on the device (air_program.h): one interpreter, run_program<Sink>, and the
// two kernels around it -- k_quotient_prog<LQD> with the frame of k_quotient_air<CHIP, LQD>
// (quotient.hip) and k_check_prog with the frame of k_check_air<CHIP> (debug_check.hip).
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

#include "debug_check.h"
#include "quotient.h"

namespace bfz {

using namespace kb;

namespace {
using ConstWords = const __attribute__((address_space(4))) uint32_t*;

// mainc: the column-major matrix (stride words per column); vt / vn: the byte offsets of the
// thread's local and next position in a column.
template <class Sink>
__device__ __forceinline__ void run_program(ConstWords code, int ncode,
                                            uint32_t (*slots)[256], const uint32_t* mainc,
                                            size_t stride, uint32_t vt, uint32_t vn,
                                            uint32_t first, uint32_t last, uint32_t trans,
                                            Sink& sink) {
  const uint32_t tid = threadIdx.x;
  for (int pc = 0; pc < ncode;) {
    const uint32_t w = code[pc++];
    const uint32_t d = (w >> 8) & 0xff, a = (w >> 16) & 0xff, b = w >> 24;
    switch (w & 0xff) {
      case AIR_CONST: slots[d][tid] = code[pc++]; break;
      case AIR_LOCAL: slots[d][tid] = ld_b(rsrc_of(mainc + (size_t)a * stride), vt, 0); break;
      case AIR_NEXT: slots[d][tid] = ld_b(rsrc_of(mainc + (size_t)a * stride), vn, 0); break;
      case AIR_FIRST: slots[d][tid] = first; break;
      case AIR_LAST: slots[d][tid] = last; break;
      case AIR_TRANS: slots[d][tid] = trans; break;
      case AIR_ADD: slots[d][tid] = madd(slots[a][tid], slots[b][tid]); break;
      case AIR_SUB: slots[d][tid] = msub(slots[a][tid], slots[b][tid]); break;
      case AIR_MUL: slots[d][tid] = mmul(slots[a][tid], slots[b][tid]); break;
      case AIR_NEG: slots[d][tid] = mneg(slots[a][tid]); break;
      default: sink.emit(slots[a][tid]);  // AIR_EMIT
    }
  }
}

// The row check's sink: counts the emissions, keeps the first that is not zero and ignores the
// rest (FirstFailAcc; the loop stays wave-uniform).
struct FirstFailSink {
  int n = 0, first = -1;
  __device__ __forceinline__ void emit(uint32_t c) {
    if (c != 0 && first < 0) first = n;
    n++;
  }
};
}  // namespace

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

void launch_check_prog(const uint32_t* code_dev, int ncode, const uint32_t* mainc, size_t h, int K,
                       unsigned long long* res_dev, int32_t* per_row_dev, hipStream_t st) {
  hipLaunchKernelGGL(k_check_prog, dim3(ceil_div(h, 256)), dim3(256), 0, st, code_dev, ncode, mainc,
                     (uint32_t)h, log2i(h), K, res_dev, per_row_dev);
  KCHECK();
}

// kernels a proof or a check of a program launches (gpu.h PreloadKernels)
static PreloadKernels preload_air_program{(const void*)&k_quotient_prog<0>,
                                          (const void*)&k_quotient_prog<1>,
                                          (const void*)&k_check_prog};

}  // namespace bfz
