// Quotient evaluation on the device: quotient_values (crates/stark/src/quotient.rs:18-165)
// with the ProverConstraintFolder fold (folder.rs:68-89) and Chip::eval (chip.rs:222-228).
//
// Point i of the quotient domain 3*H_2n (natural index) sits at storage position
// t = bitrev(i) of every LDE; its "next" row is i+2 (quotient.rs:41-42, next_step = 2).
// Selectors [p3-recalled selectors_on_coset]: Z_H(x) = x^n - 1 (= 3^n (-1)^i - 1),
// is_first = Z_H/(x-1), is_last = Z_H/(x - w_n^-1), is_transition = x - w_n^-1.
// The Horner fold acc = acc*alpha + c_k is computed as sum_k alpha^(K-1-k) c_k (identical
// value): base-valued AIR constraints cost 4 base multiplies each instead of an EF multiply.
// Output: Q(x_i) for storage position t lands in quotient chunk (t >> log n) at row
// (t mod n) -- the bit-reversed evaluation order of chunk i mod 2 on its domain
// 3 w_2n^k H_n (split_evals / split_domains), ready for the chunk LDE.
#include "quotient.h"

#include <mutex>

#include <array>
#include <map>

#include "air.h"
#include "air_program.h"

namespace bfz {

using namespace kb;

constexpr int QMAIN_W[NUM_CHIPS] = {31, 1, 7, 45, 12, 2, 41, 5};
constexpr int QPREP_W[NUM_CHIPS] = {0, 6, 0, 0, 0, 2, 0, 0};
constexpr int QPERM_W[NUM_CHIPS] = {9, 2, 4, 2, 3, 2, 2, 2};

// 1 / ((x - 1)(x - w_n^-1)) at every point of 3 H_N, stored by LDE position t (point
// bitrev(t)): the selector denominators depend on the domain alone, so one table per log N
// serves every chip of that height in every proof (built once, cached).
__global__ __launch_bounds__(256) void k_sel_inv(int logN, uint32_t shift, uint32_t wn_inv,
                                                 const uint32_t* __restrict__ twf,
                                                 uint32_t* __restrict__ out) {
  const size_t N = (size_t)1 << logN;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= N) return;
  const uint32_t x = quot_point(dbitrev((uint32_t)t, logN), (uint32_t)(N >> 1), shift, twf);
  out[t] = minv(mmul(msub(x, ONE), msub(x, wn_inv)));
}

// Register budget sized for 3 blocks per CU (4 spilled and was slower,
// profiles/r02/ab_quotient_occupancy.txt).
template <int CHIP>
__global__ __launch_bounds__(256, 3) void k_quotient(QuotRows in, int logN,
                                                  const QuotParams* __restrict__ qpp,
                                                  const uint32_t* __restrict__ twf,
                                                  const uint32_t* __restrict__ sel_inv,
                                                  QuotOut qo) {
  const QuotParams qp = *qpp;  // device memory (the challenges are sampled on the device)
  constexpr int MW = QMAIN_W[CHIP];
  constexpr int PWD = QPREP_W[CHIP] > 0 ? QPREP_W[CHIP] : 1;
  constexpr int PMW = QPERM_W[CHIP];
  const size_t N = (size_t)1 << logN, n = N >> 1;
  const size_t t = in.t0 + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= in.t0 + in.count) return;
  const uint32_t i = dbitrev((uint32_t)t, logN);
  const uint32_t inext = (i + 2) & (uint32_t)(N - 1);
  const size_t tn = dbitrev(inext, logN);

  // buffer loads: one descriptor per column (its base is wave-uniform: scalar arithmetic), the
  // row is the voffset -- no 64-bit address per column in VGPRs, and no 2 GiB limit on a whole
  // column set (a 2^24-row LDE of 36 columns spans 2.4 GB)
  uint32_t L[MW], Nx[MW], PL[PWD], PN[PWD];
  const uint32_t vt = (uint32_t)(t - in.t0) * 4u, vn = (uint32_t)tn * 4u;
#pragma unroll
  for (int c = 0; c < MW; c++) {
    L[c] = ld_b(rsrc_of(in.main_l + (size_t)c * in.stride + in.t0), vt, 0);
    Nx[c] = ld_b(rsrc_of(in.main_n + (size_t)in.nmain[c] * in.stride), vn, 0);
  }
#pragma unroll
  for (int c = 0; c < PWD; c++) {
    PL[c] = QPREP_W[CHIP] > 0 ? in.prep[(size_t)c * N + t] : 0;
    PN[c] = QPREP_W[CHIP] > 0 ? in.prep[(size_t)c * N + tn] : 0;
  }
  EF pl[PMW], pn[PMW];
#pragma unroll
  for (int e = 0; e < PMW; e++)
#pragma unroll
    for (int k = 0; k < 4; k++) {
      pl[e].c[k] = ld_b(rsrc_of(in.perm_l + (size_t)(4 * e + k) * in.stride + in.t0), vt, 0);
      pn[e].c[k] = ld_b(rsrc_of(in.perm_n + (size_t)in.nperm[4 * e + k] * in.stride), vn, 0);
    }

  const uint32_t x = quot_point(i, (uint32_t)n, qp.shift, twf);
  const uint32_t zh = (i & 1) ? qp.zh_odd : qp.zh_even;
  const uint32_t zh_inv = (i & 1) ? qp.zh_odd_inv : qp.zh_even_inv;
  const uint32_t a = msub(x, ONE), b = msub(x, qp.wn_inv);
  const uint32_t inv_ab = sel_inv[t];  // 1 / (a b)
  const uint32_t zi = mmul(zh, inv_ab);
  const uint32_t is_first = mmul(zi, b), is_last = mmul(zi, a), is_trans = b;

  PowAcc acc{{0, 0, 0, 0}, 0,
             (const __attribute__((address_space(4))) uint32_t*)qp.alpha_pows, 0};
  Air<BaseOps, PowAcc> air{L, Nx, PL, PN, is_first, is_last, is_trans, acc};
  air.template eval_air<CHIP>();
  air.template eval_perm<CHIP>(pl, pn, qp.perm_alpha, qp.beta_pows, qp.cumsum, ef_base(is_first),
                               ef_base(is_last), ef_base(is_trans));
  const EF q = ef_mul_base(acc.value(), zh_inv);
  const size_t chunk = t >> (logN - 1), pos = t & (n - 1);
#pragma unroll
  for (int e = 0; e < 4; e++) qo.chunk[chunk][e * qo.stride + pos] = q.c[e];
}

template <int CHIP>
static void launch_q(const QuotRows& in, int logN, const QuotParams* qp_dev, const uint32_t* sel,
                     const QuotOut& qo, hipStream_t st) {
  hipLaunchKernelGGL(k_quotient<CHIP>, dim3(ceil_div(in.count, 256)), dim3(256), 0, st, in, logN,
                     qp_dev, (const uint32_t*)twiddles().fwd(), sel, qo);
  KCHECK();
}

// The selector-denominator table of 3 H_N (k_sel_inv), built on first use per log N.  It is
// written on the prover stream, so every later reader on that stream sees it complete.
static const uint32_t* sel_inv_table(int logN, const QuotParams& qp, hipStream_t st) {
  static std::mutex mu;  // shared by the proof lanes
  std::lock_guard<std::mutex> lk(mu);
  static auto* cache = new std::map<int, DBuf<uint32_t>>();
  auto it = cache->find(logN);
  if (it != cache->end()) return it->second.p;
  const size_t N = (size_t)1 << logN;
  ResidentScope rs;  // cached for the process, not part of the lane's working set
  DBuf<uint32_t> d(N);
  hipLaunchKernelGGL(k_sel_inv, dim3(ceil_div(N, 256)), dim3(256), 0, st, logN, qp.shift,
                     qp.wn_inv, (const uint32_t*)twiddles().fwd(), d.p);
  KCHECK();
  HIP_CHECK(hipStreamSynchronize(st));  // complete before another lane's stream reads it
  const uint32_t* p = d.p;
  cache->emplace(logN, std::move(d));
  return p;
}

void prepare_quotient_tables(int logN) {
  twiddles().ensure(logN);
  QuotParams qp{};  // the fields k_sel_inv reads (prover.hip quotient stage)
  qp.shift = to_mont(3);
  qp.wn_inv = minv(two_adic_gen(logN - 1));
  (void)sel_inv_table(logN, qp, stream());
}

void quotient(int chip, const uint32_t* mainc, const uint32_t* prepc, const uint32_t* permc,
              int logN, const QuotParams& qp, uint32_t* qout, hipStream_t st) {
  const size_t N = (size_t)1 << logN;
  QuotRows in{mainc, mainc, permc, permc, prepc, N, 0, N, {}, {}};
  for (int c = 0; c < 64; c++) in.nmain[c] = in.nperm[c] = (uint8_t)c;
  quotient_rows(chip, in, logN, qp, qout, st);
}

void quotient_rows(int chip, const QuotRows& in, int logN, const QuotParams& qp, uint32_t* qout,
                   hipStream_t st, const QuotParams* qp_dev) {
  const size_t n = (size_t)1 << (logN - 1);
  quotient_into(chip, in, logN, qp, QuotOut{{qout, qout + 4 * n}, n}, st, qp_dev);
}

void quotient_into(int chip, const QuotRows& in, int logN, const QuotParams& qp, const QuotOut& qout,
                   hipStream_t st, const QuotParams* qp_dev) {
  twiddles().ensure(logN);
  const uint32_t* sel = sel_inv_table(logN, qp, st);
  DBuf<QuotParams> up;
  if (!qp_dev) {  // the host's parameters, uploaded (stream-ordered: freed after the launch is fine)
    up.reset(1);
    upload_async(up.p, &qp, sizeof(qp), st);
    qp_dev = up.p;
  }
  switch (chip) {
    case CHIP_CPU: launch_q<CHIP_CPU>(in, logN, qp_dev, sel, qout, st); break;
    case CHIP_PROGRAM: launch_q<CHIP_PROGRAM>(in, logN, qp_dev, sel, qout, st); break;
    case CHIP_ADDSUB: launch_q<CHIP_ADDSUB>(in, logN, qp_dev, sel, qout, st); break;
    case CHIP_JUMP: launch_q<CHIP_JUMP>(in, logN, qp_dev, sel, qout, st); break;
    case CHIP_MEMORY: launch_q<CHIP_MEMORY>(in, logN, qp_dev, sel, qout, st); break;
    case CHIP_BYTE: launch_q<CHIP_BYTE>(in, logN, qp_dev, sel, qout, st); break;
    case CHIP_MEMINSTRS: launch_q<CHIP_MEMINSTRS>(in, logN, qp_dev, sel, qout, st); break;
    case CHIP_IO: launch_q<CHIP_IO>(in, logN, qp_dev, sel, qout, st); break;
    default: throw std::runtime_error("quotient: bad chip");
  }
}

// The AIR-only quotient of ONE chip's trace: p3_uni_stark's quotient_values [p3-recalled] under
// the reference's uni-STARK builders, where send / receive are no-ops (air/builder.rs:232-239,
// 273-275) -- Air::eval_air<CHIP> alone, no preprocessed and no permutation columns.  The
// quotient domain is 3 H_(n 2^LQD): with LQD = 1 every row of the 2n-row LDE (as k_quotient),
// with LQD = 0 the even natural indices, which are the LDE's first n storage rows (bitrev of an
// even index has its top bit clear); there i is always even, so Z_H is the constant 3^n - 1
// (zh_even) and sel_inv is read at the same position t.  The next row is quotient index
// j + 2^LQD, i.e. LDE natural index i + 2 in both shapes.  Output as k_quotient: chunk
// (t >> log n) at row t mod n, the bit-reversed order of chunk j's domain 3 w_2n^j H_n.
template <int CHIP, int LQD>
__global__ __launch_bounds__(256, 3) void k_quotient_air(const uint32_t* __restrict__ mainc,
                                                         int logN,
                                                         const QuotParams* __restrict__ qpp,
                                                         const uint32_t* __restrict__ twf,
                                                         const uint32_t* __restrict__ sel_inv,
                                                         QuotOut qo) {
  const QuotParams qp = *qpp;
  constexpr int MW = QMAIN_W[CHIP];
  const size_t N = (size_t)1 << logN, n = N >> 1;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (n << LQD)) return;
  const uint32_t i = dbitrev((uint32_t)t, logN);
  const uint32_t inext = (i + 2) & (uint32_t)(N - 1);
  const uint32_t vt = (uint32_t)t * 4u, vn = dbitrev(inext, logN) * 4u;

  uint32_t L[MW], Nx[MW];  // the same per-column buffer loads as k_quotient
#pragma unroll
  for (int c = 0; c < MW; c++) {
    const __amdgpu_buffer_rsrc_t r = rsrc_of(mainc + (size_t)c * N);
    L[c] = ld_b(r, vt, 0);
    Nx[c] = ld_b(r, vn, 0);
  }
  const uint32_t none[1] = {0};  // no preprocessed trace (p3_uni_stark takes none)

  const uint32_t x = quot_point(i, (uint32_t)n, qp.shift, twf);
  const uint32_t zh = (i & 1) ? qp.zh_odd : qp.zh_even;
  const uint32_t zh_inv = (i & 1) ? qp.zh_odd_inv : qp.zh_even_inv;
  const uint32_t a = msub(x, ONE), b = msub(x, qp.wn_inv);
  const uint32_t zi = mmul(zh, sel_inv[t]);
  const uint32_t is_first = mmul(zi, b), is_last = mmul(zi, a), is_trans = b;

  PowAcc acc{{0, 0, 0, 0}, 0,
             (const __attribute__((address_space(4))) uint32_t*)qp.alpha_pows, 0};
  Air<BaseOps, PowAcc> air{L, Nx, none, none, is_first, is_last, is_trans, acc};
  air.template eval_air<CHIP>();
  const EF q = ef_mul_base(acc.value(), zh_inv);
  const size_t chunk = LQD ? t >> (logN - 1) : 0, pos = t & (n - 1);
#pragma unroll
  for (int e = 0; e < 4; e++) qo.chunk[chunk][e * qo.stride + pos] = q.c[e];
}

template <int CHIP>
static void launch_qa(int lqd, const uint32_t* mainc, int logN, const QuotParams* qp_dev,
                      const uint32_t* sel, const QuotOut& qo, hipStream_t st) {
  const size_t count = ((size_t)1 << (logN - 1)) << lqd;
  const uint32_t* twf = (const uint32_t*)twiddles().fwd();
  if (lqd == 0)
    hipLaunchKernelGGL((k_quotient_air<CHIP, 0>), dim3(ceil_div(count, 256)), dim3(256), 0, st,
                       mainc, logN, qp_dev, twf, sel, qo);
  else
    hipLaunchKernelGGL((k_quotient_air<CHIP, 1>), dim3(ceil_div(count, 256)), dim3(256), 0, st,
                       mainc, logN, qp_dev, twf, sel, qo);
  KCHECK();
}

void quotient_air(int chip, int lqd, const uint32_t* mainc, int logN, const QuotParams& qp,
                  const QuotParams* qp_dev, const QuotOut& qout, hipStream_t st) {
  if (lqd < 0 || lqd > 1) throw std::runtime_error("quotient_air: log quotient degree not 0 or 1");
  if (logN < 1 || logN > 24) throw std::runtime_error("quotient_air: bad LDE height");
  twiddles().ensure(logN);
  const uint32_t* sel = sel_inv_table(logN, qp, st);
  switch (chip) {
    case CHIP_CPU: launch_qa<CHIP_CPU>(lqd, mainc, logN, qp_dev, sel, qout, st); break;
    case CHIP_ADDSUB: launch_qa<CHIP_ADDSUB>(lqd, mainc, logN, qp_dev, sel, qout, st); break;
    case CHIP_JUMP: launch_qa<CHIP_JUMP>(lqd, mainc, logN, qp_dev, sel, qout, st); break;
    case CHIP_MEMINSTRS: launch_qa<CHIP_MEMINSTRS>(lqd, mainc, logN, qp_dev, sel, qout, st); break;
    case CHIP_IO: launch_qa<CHIP_IO>(lqd, mainc, logN, qp_dev, sel, qout, st); break;
    default: throw std::runtime_error("quotient_air: the chip has no AIR constraints");
  }
}

// quotient_air for an AIR that arrives as a constraint program (air_program.h): the same
// tables, k_quotient_prog<lqd> instead of the chip's compiled template.
void quotient_prog(const uint32_t* code_dev, int ncode, int lqd, const uint32_t* mainc, int logN,
                   const QuotParams& qp, const QuotParams* qp_dev, const QuotOut& qout,
                   hipStream_t st) {
  if (lqd < 0 || lqd > 1) throw std::runtime_error("quotient_prog: log quotient degree not 0 or 1");
  if (logN < 1 || logN > 24) throw std::runtime_error("quotient_prog: bad LDE height");
  twiddles().ensure(logN);
  const uint32_t* sel = sel_inv_table(logN, qp, st);
  launch_quotient_prog(lqd, code_dev, ncode, mainc, logN, qp_dev, (const uint32_t*)twiddles().fwd(),
                       sel, qout, st);
}

// The quotient challenge on the device (challenger.h): the sponge observes the permutation
// root and every chip's cumulative sum, samples alpha (prover.rs:336-342); each chip's alpha
// powers alpha^(K-1-j) and the challenge fields of its QuotParams are written.
// Every 16-lane row runs the sponge (the same values); the powers are then spread over the whole
// block, one (chip, j) pair per thread (64 threads looping over the chips took 28 us).
constexpr int QCH_THREADS = 1024;
__global__ __launch_bounds__(QCH_THREADS) void k_challenge_quot(DevChallenger* __restrict__ c,
                                                                const uint32_t* __restrict__ root,
                                                                const EF* __restrict__ cums, int nc,
                                                                const PermChallenges* __restrict__ pc,
                                                                QuotParams* __restrict__ qps,
                                                                QuotAlphaTargets tg) {
  __shared__ EF s_alpha;
  if (threadIdx.x < 64) {  // one wave: the sponge
    LaneSponge sp;
    sp.load(c);
    for (int i = 0; i < 8; i++) sp.observe(root[i]);
    for (int k = 0; k < nc; k++)
      for (int e = 0; e < 4; e++) sp.observe(cums[k].c[e]);
    const EF alpha = sp.sample_ef();
    sp.store(c);
    if (threadIdx.x == 0) {
      s_alpha = alpha;
      if (tg.alpha_out) *tg.alpha_out = alpha;
    }
  }
  __syncthreads();
  const EF a = s_alpha;
  int total = 0;
  for (int k = 0; k < nc; k++) total += tg.K[k];
  for (int t = threadIdx.x; t < total; t += blockDim.x) {
    int k = 0, j = t;
    while (j >= tg.K[k]) j -= tg.K[k++];
    tg.apows[k][j] = ef_pow(a, (uint64_t)(tg.K[k] - 1 - j));
  }
  if (threadIdx.x < nc) {
    QuotParams& q = qps[threadIdx.x];
    q.perm_alpha = pc->alpha;
    for (int j = 0; j < 8; j++) q.beta_pows[j] = pc->beta_pows[j];
    q.cumsum = cums[threadIdx.x];
  }
}

void challenge_quot(DevChallenger* ch, const uint32_t* root, const EF* cums, int nc,
                    const PermChallenges* pc, QuotParams* qps, const QuotAlphaTargets& tg,
                    hipStream_t st) {
  if (nc > QUOT_MAX_CHIPS) throw std::runtime_error("challenge_quot: too many chips");
  hipLaunchKernelGGL(k_challenge_quot, dim3(1), dim3(QCH_THREADS), 0, st, ch, root, cums, nc, pc, qps, tg);
  KCHECK();
}

}  // namespace bfz

namespace bfz {

template <int CHIP>
static int count_chip() {
  EF z[64];
  for (auto& e : z) e = kb::ef_zero();
  CountAcc acc;
  Air<ExtOps, CountAcc> air{z, z, z, z, z[0], z[0], z[0], acc};
  air.template eval_air<CHIP>();
  EF bp[8];
  for (auto& e : bp) e = kb::ef_zero();
  air.template eval_perm<CHIP>(z, z, z[0], bp, z[0], z[0], z[0], z[0]);
  return acc.n;
}

// The count is a property of the AIR: evaluated symbolically once per chip and cached (the
// prover needs it for every chip of every proof).
static int num_constraints_eval(int chip) {
  switch (chip) {
    case CHIP_CPU: return count_chip<CHIP_CPU>();
    case CHIP_PROGRAM: return count_chip<CHIP_PROGRAM>();
    case CHIP_ADDSUB: return count_chip<CHIP_ADDSUB>();
    case CHIP_JUMP: return count_chip<CHIP_JUMP>();
    case CHIP_MEMORY: return count_chip<CHIP_MEMORY>();
    case CHIP_BYTE: return count_chip<CHIP_BYTE>();
    case CHIP_MEMINSTRS: return count_chip<CHIP_MEMINSTRS>();
    case CHIP_IO: return count_chip<CHIP_IO>();
  }
  return 0;
}

int num_constraints(int chip) {
  static const auto counts = [] {
    std::array<int, NUM_CHIPS> c{};
    for (int i = 0; i < NUM_CHIPS; i++) c[i] = num_constraints_eval(i);
    return c;
  }();
  if (chip < 0 || chip >= NUM_CHIPS) return 0;
  return counts[chip];
}

// Degree of each AIR constraint, by running eval_air over degrees instead of values: the rules
// of SymbolicExpression::degree_multiple [p3-recalled] -- a trace variable 1, a constant 0,
// is_first_row / is_last_row 1, is_transition 0, add / sub the maximum, mul the sum, neg the
// identity.
struct DegOps {
  using T = int;
  static KB_HD T add(T a, T b) { return a > b ? a : b; }
  static KB_HD T sub(T a, T b) { return a > b ? a : b; }
  static KB_HD T mul(T a, T b) { return a + b; }
  static KB_HD T neg(T a) { return a; }
  static KB_HD T cst(uint32_t) { return 0; }
};
struct DegAcc {
  int max = 0;
  void emit(int d) {
    if (d > max) max = d;
  }
};

// K from CountAcc over eval_air alone (count_chip above adds the LogUp constraints), the degree
// from a second evaluation over degrees.
template <int CHIP>
static void air_shape(int* K, int* degree) {
  EF z[64];
  for (auto& e : z) e = kb::ef_zero();
  CountAcc count;
  Air<ExtOps, CountAcc> counted{z, z, z, z, z[0], z[0], z[0], count};
  counted.template eval_air<CHIP>();
  *K = count.n;
  int one[64];
  for (int& v : one) v = 1;
  DegAcc acc;
  Air<DegOps, DegAcc> air{one, one, one, one, 1, 1, 0, acc};
  air.template eval_air<CHIP>();
  *degree = acc.max;
}

bool uni_air_shape(int chip, int* K, int* degree, int* lqd) {
  int k = 0, d = 0;
  switch (chip) {
    case CHIP_CPU: air_shape<CHIP_CPU>(&k, &d); break;
    case CHIP_ADDSUB: air_shape<CHIP_ADDSUB>(&k, &d); break;
    case CHIP_JUMP: air_shape<CHIP_JUMP>(&k, &d); break;
    case CHIP_MEMINSTRS: air_shape<CHIP_MEMINSTRS>(&k, &d); break;
    case CHIP_IO: air_shape<CHIP_IO>(&k, &d); break;
    default: return false;  // Program, Memory, Byte: no AIR constraints of their own
  }
  int l = 0;  // log2_ceil(d - 1), at least 0 (chip.rs:82-87)
  while ((1 << l) < d - 1) l++;
  if (K) *K = k;
  if (degree) *degree = d;
  if (lqd) *lqd = l;
  return true;
}

static PreloadKernels preload_quotient_air{
    (const void*)&k_quotient_air<0, 0>, (const void*)&k_quotient_air<0, 1>,
    (const void*)&k_quotient_air<2, 0>, (const void*)&k_quotient_air<2, 1>,
    (const void*)&k_quotient_air<3, 0>, (const void*)&k_quotient_air<3, 1>,
    (const void*)&k_quotient_air<6, 0>, (const void*)&k_quotient_air<6, 1>,
    (const void*)&k_quotient_air<7, 0>, (const void*)&k_quotient_air<7, 1>};

// kernels a proof launches (gpu.h PreloadKernels)
static PreloadKernels preload_quotient{
    (const void*)&k_quotient<0>,
    (const void*)&k_quotient<1>,
    (const void*)&k_quotient<2>,
    (const void*)&k_quotient<3>,
    (const void*)&k_quotient<4>,
    (const void*)&k_quotient<5>,
    (const void*)&k_quotient<6>,
    (const void*)&k_quotient<7>,
    (const void*)&k_sel_inv,
    (const void*)&k_challenge_quot};

}  // namespace bfz
