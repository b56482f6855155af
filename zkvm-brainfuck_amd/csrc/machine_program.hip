// The prover of a machine of caller-defined chips (machine_program.h): MachineProver::commit and
// ::open (crates/stark/src/prover.rs:209-236, 242-553) in open_main's stage order, with the host
// challenger, over chips that are data.  Every stage but two is the code the built-in prover
// runs (commit_lde, Round::commit, perm_running_sum, coset_lde_ex, pcs_open).  The two steps that
// interpret programs -- a chip's permutation rows and its quotient -- are launched once per chip
// by k_perm_rows_prog / k_quotient_chip_prog; a machine has up to 32 chips, most of them far
// smaller than the device (a 16-row chip is one partial block), so here each step is ONE launch
// whose grid covers every chip: k_perm_rows_machine and k_quotient_machine<HAS_AIR>.
//
// Design decisions:
//   Segment table.  A launch reads one MachTable in device memory: the block offsets of its
//     segments (at most 33 words) and one MachSeg per chip -- the code and list pointers, the
//     column bases of the chip's main, preprocessed and permutation matrices, logN, the output
//     bases, the sel_inv table of the chip's height and the chip's own QuotParams block (its K
//     alpha powers, Z_H values and w_n^-1 differ per chip).  twf is one table for every height
//     (twf[n + i]) and stays a kernel argument.
//   Chip lookup in scalar registers.  A block walks the offsets with blockIdx.x.  The table is
//     read through the constant address space, blockIdx.x is an SGPR, so the walk is a scalar
//     loop of at most 32 s_load + s_cmp steps and every descriptor field -- pointers included --
//     lands in SGPRs, exactly like the list walkers of lookup_program_dev.h.  The alternative, a
//     per-block chip index array (one word per block, 2^15 words for a 2^22-row chip), would trade
//     the walk for a load of the same latency and 128 KiB of table; the walk is free next to a
//     block's thousands of field multiplications.
//   The interpreter frame is the per-chip kernels' frame, unchanged: one thread per storage
//     position, next row i + 2 (quotient domain), PowAcc over the chip's own K powers,
//     run_program and perm_constraints as they are.  The position within the chip is
//     (blockIdx.x - offset) * 256 + threadIdx.x; a block never spans two chips, so list reads,
//     loop bounds and branches stay wave-uniform.
//   Block order.  Segments are laid out in commit order, tallest chip first: the dispatcher
//     hands out blocks in index order, so the long chip's blocks start first and the small chips'
//     few blocks fill the CUs that its tail leaves idle.  A height-1 chip is a partial block of two
//     positions (quotient) or one (permutation rows).
//   Two quotient launches.  HAS_AIR = 1 declares the 32 KiB slot file; the lookup-only chips go
//     into a second launch of HAS_AIR = 0, which declares none and is bounded by registers alone
//     (chip_program.hip's argument, kept).
//   LDS of the permutation kernel.  The prefix file is dynamic LDS, 4 KiB per batch per block, and
//     one launch has one size: the largest batch count in it.  With 256-thread blocks a CU holds at
//     most 8 blocks by waves (4 waves each, 8 per SIMD), so any file of up to 20 KiB (160 KiB / 8),
//     5 batches, costs no occupancy, whatever the chip.  A machine whose chips all have at most 5
//     batches, or all more, is one launch.  Otherwise the launch is split into two classes -- chips
//     of at most 5 batches (file sized by their maximum) and the rest (sized by theirs) -- so a tall
//     one-batch chip (MemoryInstrs, Jump: 8 blocks per CU) is never held to the 5 blocks per CU
//     that Cpu's 8-batch file allows.  Two classes at most: within the large class the tallest chip
//     of the exported set is Cpu itself, and a third class would split launches that are already
//     LDS-bound by their own chips.
//   The constraint check (machine_check, k_check_machine<HAS_AIR>) is the third segmented launch:
//     k_check_chip_prog's frame on the trace domain with ProfileSink through both phases, over the
//     evaluations and the permutation rows where k_perm_rows_machine left them.  LDS: the 32 KiB
//     slot file (HAS_AIR = 1) + reduce_failures' 48 bytes static, then 8 kmax bytes of dynamic
//     count / first tables (kmax <= 531: 4248 bytes) -- 37064 bytes at most, 4 blocks (16 waves)
//     per CU of 160 KiB, as k_check_chip_prog<1>; HAS_AIR = 0 declares the tables alone and is
//     bounded by its 68 VGPRs (7 waves per SIMD).
//   Running sums stay per chip (perm_running_sum): a scan's length is its chip's height.
//   No scratch: the descriptor is read field by field from the constant address space, never
//     copied into a private struct; private_segment_fixed_size is 0.
#include "machine_program.h"

#include <algorithm>
#include <cstring>

#include "chip_program_dev.h"
#include "ntt.h"
#include "pcs_open.h"
#include "uni_stark.h"

namespace bfz {

using namespace kb;

namespace {
struct MachSeg {
  const uint32_t *code, *list;           // device lists; code is unread by HAS_AIR = 0
  const uint32_t *mainc, *prepc, *permc;  // column bases (stride: the segment's row count)
  const uint32_t* sel_inv;                // quotient: the table of 3 H_N
  uint32_t* out[2];                       // quotient: QuotOut::chunk; permutation: out[0] = perm
  EF* rowsum;                             // permutation: the row sums
  unsigned long long* res;                // check: {min key, failing rows, count[K], first[K]}
  size_t out_stride;                      // QuotOut::stride
  uint32_t ncode, log_rows;               // log_rows: logN (quotient), log n (permutation, check)
  uint32_t num_constraints, pad;          // check: K
  QuotParams qp;                          // begins with the LogUp challenges' words
};
struct MachTable {
  uint32_t nseg, pad;
  uint32_t off[MACHINE_MAX_CHIPS + 1];  // first block of each segment, then the grid size
  MachSeg seg[MACHINE_MAX_CHIPS];
};
using ConstTable = const __attribute__((address_space(4))) MachTable*;

// The segment of this block: a scalar walk (blockIdx.x and the table are uniform).
__device__ __forceinline__ uint32_t find_segment(ConstTable T) {
  const uint32_t nseg = T->nseg;
  uint32_t s = 0;
  while (s + 1 < nseg && blockIdx.x >= T->off[s + 1]) s++;
  return s;
}
}  // namespace

// k_quotient_chip_prog<HAS_AIR> for every segment of tab: one thread per storage position t of
// the segment's LDEs on 3 H_2n (N = 2^logN rows), natural index i = bitrev(t), next row i + 2.
template <int HAS_AIR>
__global__ __launch_bounds__(256) void k_quotient_machine(const MachTable* __restrict__ tab,
                                                          const uint32_t* __restrict__ twf) {
  uint32_t(*slots)[256] = nullptr;
  if constexpr (HAS_AIR) {
    __shared__ uint32_t file[BFZ_AIR_MAX_LIVE][256];
    slots = file;
  }
  const ConstTable T = (ConstTable)tab;
  const uint32_t s = find_segment(T);
  const int logN = (int)T->seg[s].log_rows;
  const uint32_t* mainc = T->seg[s].mainc;
  const uint32_t* prepc = T->seg[s].prepc;
  const uint32_t* permc = T->seg[s].permc;
  const uint32_t* sel_inv = T->seg[s].sel_inv;
  const QuotParams* qpp = &tab->seg[s].qp;
  const QuotParams qp = *qpp;  // device memory; uniform: scalar loads of the fields read below
  const size_t N = (size_t)1 << logN, n = N >> 1;
  const size_t t = (size_t)(blockIdx.x - T->off[s]) * blockDim.x + threadIdx.x;
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
    run_program((ConstWords)T->seg[s].code, (int)T->seg[s].ncode, slots, mainc, N, vt, vn, is_first,
                is_last, is_trans, acc);
  // phase 2: batches + 3 LogUp constraints
  const ConstWords qw = (ConstWords)(const uint32_t*)qpp;
  const RowCtx c{(ConstWords)T->seg[s].list, qw, mainc, prepc, N, vt};
  perm_constraints(c, permc, vn, qw + QP_CUMSUM_WORD, is_first, is_last, is_trans, acc);

  const EF q = ef_mul_base(acc.value(), zh_inv);
  const size_t chunk = t >> (logN - 1), pos = t & (n - 1);
  uint32_t* dst = T->seg[s].out[chunk];
  const size_t stride = T->seg[s].out_stride;
#pragma unroll
  for (int e = 0; e < 4; e++) dst[e * stride + pos] = q.c[e];
}

// k_quotient_machine on a coset slab S_r = 3 g^r H_2n, r >= 1, of the quotient domain 3 H_(D n) a
// chip of AIR degree 4 to 9 needs (D = 2^lqd = 4 or 8 chunks, g = w_(D n); air_program.h
// SlabParams has the geometry).  One launch covers every chip of the machine that has a slab r:
// a segment's mainc / prepc / permc are the chip's LDEs ON THE SLAB (Prover::slab_ldes), and its
// QuotParams block is the slab's -- shift = 3 g^r, the slab's two Z_H values and their inverses --
// beside the chip's alpha powers, LogUp challenges and cumulative sum, so the kernel reads the
// descriptor exactly as k_quotient_machine does.  What differs from it:
//   - no selector table exists for a slab: the block's 256 denominators (x - 1)(x - w_n^-1) are
//     inverted with one field inversion (block_inverse; a slab is disjoint from H_n, none is
//     zero).  That needs barriers, so a thread past its segment brings the denominator 1, takes
//     part in both barriers and leaves after them; a block never spans two segments, so the
//     segment walk and everything read from the descriptor stay uniform across the barriers.
//   - the slab's even natural points are chunk r and its odd ones chunk r + D/2: out[0] / out[1]
//     are the two halves of the chip's 2 x 4 x n value buffer (stride n), which the host extends
//     to the two chunks' LDEs.
// LDS: the 32 KiB slot file (HAS_AIR = 1) + block_inverse's 20 bytes; HAS_AIR = 0 declares the 20
// bytes alone.  (Only a chip with an AIR can have degree above 3, so today every slab segment is
// in the HAS_AIR = 1 launch; the other class is kept so that the two quotient launches pair up.)
template <int HAS_AIR>
__global__ __launch_bounds__(256) void k_quotient_machine_coset(const MachTable* __restrict__ tab,
                                                                const uint32_t* __restrict__ twf) {
  uint32_t(*slots)[256] = nullptr;
  if constexpr (HAS_AIR) {
    __shared__ uint32_t file[BFZ_AIR_MAX_LIVE][256];
    slots = file;
  }
  __shared__ uint32_t s_wave[4], s_tinv;
  const ConstTable T = (ConstTable)tab;
  const uint32_t s = find_segment(T);
  const int logN = (int)T->seg[s].log_rows;
  const uint32_t* mainc = T->seg[s].mainc;
  const uint32_t* prepc = T->seg[s].prepc;
  const uint32_t* permc = T->seg[s].permc;
  const QuotParams* qpp = &tab->seg[s].qp;
  const QuotParams qp = *qpp;  // device memory; uniform: scalar loads of the fields read below
  const size_t N = (size_t)1 << logN, n = N >> 1;
  const size_t t = (size_t)(blockIdx.x - T->off[s]) * blockDim.x + threadIdx.x;
  const bool has_point = t < N;
  const uint32_t i = dbitrev(has_point ? (uint32_t)t : 0u, logN);  // in bounds whatever t
  const uint32_t x = quot_point(i, (uint32_t)n, qp.shift, twf);
  const uint32_t a = msub(x, ONE), b = msub(x, qp.wn_inv);
  const uint32_t inv_ab = block_inverse(has_point ? mmul(a, b) : ONE, s_wave, &s_tinv);
  if (!has_point) return;  // (no barrier below)

  const uint32_t inext = (i + 2) & (uint32_t)(N - 1);
  const uint32_t vt = (uint32_t)t * 4u, vn = dbitrev(inext, logN) * 4u;  // t < 2^23
  const uint32_t zh = (i & 1) ? qp.zh_odd : qp.zh_even;
  const uint32_t zh_inv = (i & 1) ? qp.zh_odd_inv : qp.zh_even_inv;
  const uint32_t zi = mmul(zh, inv_ab);
  const uint32_t is_first = mmul(zi, b), is_last = mmul(zi, a), is_trans = b;

  PowAcc acc{{0, 0, 0, 0}, 0, (ConstWords)qp.alpha_pows, 0};
  if constexpr (HAS_AIR)  // phase 1: the AIR's K_air constraints
    run_program((ConstWords)T->seg[s].code, (int)T->seg[s].ncode, slots, mainc, N, vt, vn, is_first,
                is_last, is_trans, acc);
  // phase 2: batches + 3 LogUp constraints
  const ConstWords qw = (ConstWords)(const uint32_t*)qpp;
  const RowCtx c{(ConstWords)T->seg[s].list, qw, mainc, prepc, N, vt};
  perm_constraints(c, permc, vn, qw + QP_CUMSUM_WORD, is_first, is_last, is_trans, acc);

  const EF q = ef_mul_base(acc.value(), zh_inv);
  const size_t half = t >> (logN - 1), pos = t & (n - 1);
  uint32_t* dst = T->seg[s].out[half];
  const size_t stride = T->seg[s].out_stride;
#pragma unroll
  for (int e = 0; e < 4; e++) dst[e * stride + pos] = q.c[e];
}

// k_perm_rows_prog<1> for every segment of tab: one thread per storage position of a trace of
// n = 2^log_rows rows; the batch columns of the segment's perm and rowsum[t].  Dynamic LDS: the
// launch's largest batch count x 4 x LKP_T words (a thread's slots depend on its own batch index
// alone, so a chip with fewer batches uses a prefix of the file).
template <int WRITE>
__global__ __launch_bounds__(LKP_T) void k_perm_rows_machine(const MachTable* __restrict__ tab) {
  static_assert(WRITE == 1, "the balance-only form has no machine counterpart");
  extern __shared__ uint32_t pre[];  // [batch][component][LKP_T]
  const ConstTable T = (ConstTable)tab;
  const uint32_t s = find_segment(T);
  const size_t n = (size_t)1 << T->seg[s].log_rows;
  const size_t t = (size_t)(blockIdx.x - T->off[s]) * LKP_T + threadIdx.x;
  if (t >= n) return;  // (no barrier below)
  const uint32_t tid = threadIdx.x;
  uint32_t* perm = T->seg[s].out[0];
  const RowCtx c{(ConstWords)T->seg[s].list, (ConstWords)(const uint32_t*)&tab->seg[s].qp,
                 T->seg[s].mainc, T->seg[s].prepc, n, (uint32_t)t * 4u};
  const int ni = (int)c.list[0], nb = (ni + 1) >> 1;

  EF P;  // forward: the prefix products of the batch denominators
  int at = LKP_HEAD;
  for (int b = 0; b < nb; b++) {
    EF num, den;
    batch_frac(c, at, 2 * b + 1 < ni, num, den);
    P = b ? ef_mul(P, den) : den;
#pragma unroll
    for (int e = 0; e < 4; e++) pre[(4 * b + e) * LKP_T + tid] = P.c[e];
  }
  EF inv = ef_inv(P);  // the row's one inversion
  EF sum = ef_zero();
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
  T->seg[s].rowsum[t] = sum;
}

// k_check_chip_prog<HAS_AIR> for every segment of tab, with the constraint profile: one thread per
// storage position t of a trace of n = 2^log_rows rows (evaluations, stride n), natural row i =
// bitrev(t), next row (i + 1) mod n (n = 1: the row itself), selectors 0 / 1 words, is_transition =
// 1 - is_last (debug.rs:43-94).  ProfileSink runs through run_program and perm_constraints, so one
// pass gives the segment's summary (reduce_failures) and its count[K] / first[K] tables.
// Dynamic LDS: kmax counts then kmax first rows, after the static slot file (HAS_AIR = 1) and
// reduce_failures' 48 bytes.  kmax = the largest K of the launch; a segment uses a prefix.
// A lane past its segment's last row evaluates row 0 of its OWN segment with row = PROFILE_NO_ROW:
// every lane reaches every ballot, butterfly and barrier, no lane fails for a row that is not
// there, and every load stays inside the segment's matrices (position 0 exists at any height).
template <int HAS_AIR>
__global__ __launch_bounds__(256) void k_check_machine(const MachTable* __restrict__ tab, int kmax) {
  extern __shared__ uint32_t prof[];  // [2][kmax]
  uint32_t(*slots)[256] = nullptr;
  if constexpr (HAS_AIR) {
    __shared__ uint32_t file[BFZ_AIR_MAX_LIVE][256];
    slots = file;
  }
  uint32_t *s_cnt = prof, *s_fst = prof + kmax;
  const ConstTable T = (ConstTable)tab;
  const uint32_t s = find_segment(T);
  const int K = (int)T->seg[s].num_constraints;  // <= kmax
  profile_clear(s_cnt, s_fst, K);
  const int logn = (int)T->seg[s].log_rows;
  const uint32_t n = 1u << logn;
  const uint32_t* mainc = T->seg[s].mainc;
  const uint32_t t = (blockIdx.x - T->off[s]) * 256u + threadIdx.x;
  const bool has_row = t < n;
  const uint32_t ts = has_row ? t : 0u;  // in bounds of this segment whatever t
  const uint32_t i = dbitrev(ts, logn);
  const uint32_t vt = ts * 4u, vn = dbitrev((i + 1) & (n - 1), logn) * 4u;  // ts < n <= 2^23
  const uint32_t first = i == 0 ? ONE : 0u, last = i == n - 1 ? ONE : 0u,
                 trans = i == n - 1 ? 0u : ONE;
  ProfileSink sink{s_cnt, s_fst, has_row ? i : PROFILE_NO_ROW};
  if constexpr (HAS_AIR)  // phase 1: the AIR's K_air constraints
    run_program((ConstWords)T->seg[s].code, (int)T->seg[s].ncode, slots, mainc, n, vt, vn, first,
                last, trans, sink);
  // phase 2: batches + 3 LogUp constraints; the challenges and the cumulative sum head qp
  const ConstWords qw = (ConstWords)(const uint32_t*)&tab->seg[s].qp;
  const RowCtx c{(ConstWords)T->seg[s].list, qw, mainc, T->seg[s].prepc, n, vt};
  perm_constraints(c, T->seg[s].permc, vn, qw + QP_CUMSUM_WORD, first, last, trans, sink);
  unsigned long long* res = T->seg[s].res;
  profile_flush(s_cnt, s_fst, K, res + 2);
  reduce_failures(sink.first, i, K, res);
}

namespace {
constexpr int PERM_FREE_BATCHES = 5;  // 20 KiB: 8 blocks per CU, the wave limit (file header)

// Appends a segment of `rows` positions; the table's last offset is the grid size.
void push_segment(MachTable& T, const MachSeg& sg, size_t rows) {
  T.seg[T.nseg] = sg;
  T.off[T.nseg + 1] = T.off[T.nseg] + ceil_div(rows, 256);
  T.nseg++;
}

struct DevTable {
  DBuf<MachTable> d;
  uint32_t grid = 0;
  int max_batches = 0;
  void upload(const MachTable& T, hipStream_t st) {
    grid = T.off[T.nseg];
    if (!T.nseg) return;
    d.reset(1);
    upload_async(d.p, &T, sizeof(MachTable), st);
  }
};

// A table of one segment: a chip's coset slab alone (bfz_chip_quotient, and machine_time's
// per-chip form, which builds its tables before the timed window as the segmented form does).
void one_slab_table(DevTable& dt, const ChipLists& cl, const uint32_t* mainc, const uint32_t* prepc,
                    const uint32_t* permc, int logN, const QuotParams& slab_qp, const QuotOut& out,
                    hipStream_t st) {
  MachTable T;
  std::memset(&T, 0, sizeof T);
  MachSeg sg{};
  sg.code = cl.code;
  sg.ncode = (uint32_t)cl.ncode;
  sg.list = cl.list;
  sg.mainc = mainc;
  sg.prepc = prepc;
  sg.permc = permc;
  sg.out[0] = out.chunk[0];
  sg.out[1] = out.chunk[1];
  sg.out_stride = out.stride;
  sg.log_rows = (uint32_t)logN;
  sg.qp = slab_qp;
  push_segment(T, sg, (size_t)1 << logN);
  dt.upload(T, st);
}
// Only a chip with an AIR exceeds degree 3, so every slab table there is today is has_air; the
// HAS_AIR = 0 branch mirrors k_quotient_machine's pair and cannot be reached.
void launch_slab_table(const DevTable& dt, bool has_air, hipStream_t st) {
  const uint32_t* twf = (const uint32_t*)twiddles().fwd();
  if (has_air)
    hipLaunchKernelGGL(k_quotient_machine_coset<1>, dim3(dt.grid), dim3(256), 0, st, dt.d.p, twf);
  else
    hipLaunchKernelGGL(k_quotient_machine_coset<0>, dim3(dt.grid), dim3(256), 0, st, dt.d.p, twf);
  KCHECK();
}

// One proof's device state, stage by stage (machine_prove runs them once; machine_time runs the
// two interpreted steps in both forms on the same inputs).
struct Prover {
  const MachineProgram& m;
  hipStream_t st;
  int nc = 0;
  std::vector<int> chip;     // m.chips index of the k-th committed matrix
  std::vector<int> order;    // its position in the caller's arrays
  std::vector<size_t> hn;    // its height
  std::vector<DBuf<uint32_t>> evals, pe;
  std::vector<DBuf<EF>> rows;
  DBuf<EF> cums_d, apows_d;
  std::vector<EF> cums;
  Round mainr, permr, quotr;
  PermChallenges pch;
  DevTable perm_tab[2], quot_tab[2];  // permutation: the LDS classes; quotient: AIR, lookup-only
  DevTable check_tab[2];              // the constraint check: AIR, lookup-only
  int check_kmax[2] = {0, 0};         // the largest K of either check launch (its LDS tables)
  std::vector<size_t> res_at;         // chip k's block in check_res: 2 + 2 K words
  DBuf<unsigned long long> check_res;
  std::vector<unsigned long long> check_host;
  std::vector<const QuotParams*> qp_dev;  // chip k's block inside its quotient table
  std::vector<const uint32_t*> sel;
  std::vector<QuotParams> qph;            // the same block on the host (slab 0's domain fields)
  std::vector<int> qat;                   // chip k's first matrix in the quotient round (D_k each)
  // A chip of D = 4 or 8 chunks: its LDEs on one coset slab -- main, preprocessed, permutation in
  // one buffer of 2n x (w_main + w_prep + 4 perm_width) that every slab reuses -- and the slab's
  // 2 x 4 x n chunk values; slab_tab[r - 1]: the segment tables of slab r (AIR, lookup-only).
  std::vector<DBuf<uint32_t>> slab, vals;
  DevTable slab_tab[3][2];
  std::vector<DevTable> chip_slab_tab;    // machine_time: chip k's slab r alone, at 3 k + r - 1
  int max_half = 1;                       // the largest D / 2: slabs 1 .. max_half - 1 exist

  Prover(const MachineProgram& m_, hipStream_t s) : m(m_), st(s) {}
  const MachineChip& mc(int k) const { return m.chips[chip[k]]; }
  const uint32_t* prep_evals(int k) const { return mc(k).p.lk.prep_w ? mc(k).prep_evals.p : nullptr; }
  const uint32_t* prep_lde(int k) const {
    return mc(k).prep_index >= 0 ? m.prep.mats[mc(k).prep_index].lde.buf.p : nullptr;
  }
  ChipLists lists(int k) const {
    const ChipProgram& p = mc(k).p;
    return ChipLists{p.has_air ? mc(k).code.p : nullptr, p.has_air ? (int)p.air.code.size() : 0,
                     mc(k).list.p, p.air_constraints(), p.num_constraints()};
  }

  // Checks, upload and transpose (uni_upload_trace), the commit order, the main commit.
  // lde = false (the constraint check) stops after the transposed evaluations.
  void commit_main(const int* chips, const uint32_t* const* traces, const size_t* heights, size_t n,
                   bool tree = true, bool lde = true) {
    if (!m.can_prove) throw std::runtime_error("machine: a verifier-only machine cannot prove");
    order = machine_trace_order(m, chips, traces, heights, n, /*same_height_limit=*/tree);
    nc = (int)n;
    chip.resize(nc);
    hn.resize(nc);
    evals.resize(nc);
    size_t tallest = 0;
    for (int k = 0; k < nc; k++) {
      chip[k] = chips[order[k]];
      hn[k] = heights[order[k]];
      tallest = std::max(tallest, hn[k]);
    }
    for (int k = 0; k < nc; k++) {  // before any device work
      try {
        chip_cap_or_throw(mc(k).p);
      } catch (const std::exception& e) {
        throw std::runtime_error("machine: chip " + mc(k).name + ": " + e.what());
      }
      if (lde && hn[k] > chip_max_height(mc(k).p))  // the quotient domain 3 H_(D n) must exist
        throw std::runtime_error("machine: height " + std::to_string(hn[k]) + " of chip " + mc(k).name +
                                 " is above 2^" + std::to_string(24 - mc(k).p.log_quotient_degree()) +
                                 " at log quotient degree " +
                                 std::to_string(mc(k).p.log_quotient_degree()));
    }
    twiddles().ensure(log2i(tallest) + 1);
    for (int k = 0; k < nc; k++)
      evals[k] = uni_upload_trace((size_t)mc(k).p.lk.main_w, mc(k).name.c_str(),
                                  traces[order[k]], hn[k], st);
    if (!lde) return;
    mainr.mats.resize(nc);
    for (int k = 0; k < nc; k++) commit_lde(mainr.mats[k], evals[k].p, hn[k], mc(k).p.lk.main_w, ONE, st);
    if (tree) mainr.commit(st, /*fetch_root=*/true);
  }

  // The permutation buffers and the segment tables of the (at most two) LDS classes.
  void perm_setup(const EF& alpha, const EF& beta) {
    pch.alpha = alpha;
    pch.beta_pows[0] = ef_one();
    for (int j = 1; j < 8; j++) pch.beta_pows[j] = ef_mul(pch.beta_pows[j - 1], beta);
    pe.resize(nc);
    rows.resize(nc);
    cums_d.reset(nc);
    bool small = false, large = false;  // is there a chip on either side of the free file size
    for (int k = 0; k < nc; k++) (mc(k).p.lk.batches() <= PERM_FREE_BATCHES ? small : large) = true;
    const bool split = small && large;
    MachTable T[2];
    std::memset(T, 0, sizeof T);
    for (int k = 0; k < nc; k++) {  // commit order: tallest first
      const int nb = mc(k).p.lk.batches();
      pe[k].reset(4 * (size_t)(nb + 1) * hn[k]);
      rows[k].reset(hn[k]);
      MachSeg sg{};
      sg.list = mc(k).list.p;
      sg.mainc = evals[k].p;
      sg.prepc = prep_evals(k);
      sg.out[0] = pe[k].p;
      sg.rowsum = rows[k].p;
      sg.log_rows = (uint32_t)log2i(hn[k]);
      sg.qp.perm_alpha = pch.alpha;
      for (int j = 0; j < 8; j++) sg.qp.beta_pows[j] = pch.beta_pows[j];
      const int cls = split && nb > PERM_FREE_BATCHES ? 1 : 0;
      push_segment(T[cls], sg, hn[k]);
      perm_tab[cls].max_batches = std::max(perm_tab[cls].max_batches, nb);
    }
    for (int cls = 0; cls < 2; cls++) perm_tab[cls].upload(T[cls], st);
  }
  void perm_rows_segmented() {
    for (const DevTable& t : perm_tab) {
      if (!t.grid) continue;
      const size_t lds = (size_t)t.max_batches * 4 * LKP_T * sizeof(uint32_t);  // at most 64 KiB
      hipLaunchKernelGGL(k_perm_rows_machine<1>, dim3(t.grid), dim3(LKP_T), lds, st, t.d.p);
      KCHECK();
    }
  }
  // The running sums (per chip), the LDEs and the commit; the cumulative sums come to the host.
  void perm_commit(bool tree = true) {
    permr.mats.resize(nc);
    for (int k = 0; k < nc; k++) {
      const int nb = mc(k).p.lk.batches();
      perm_running_sum(rows[k].p, hn[k], pe[k].p, 4 * nb, cums_d.p + k, st);
      commit_lde(permr.mats[k], pe[k].p, hn[k], 4 * (nb + 1), ONE, st);
    }
    if (tree) permr.commit(st, /*fetch_root=*/true);
    cums.resize(nc);
    HIP_CHECK(hipMemcpyAsync(cums.data(), cums_d.p, nc * sizeof(EF), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  }

  // The constraint check's form of perm_commit: the running sums alone, no LDE.
  void perm_sums() {
    for (int k = 0; k < nc; k++)
      perm_running_sum(rows[k].p, hn[k], pe[k].p, 4 * mc(k).p.lk.batches(), cums_d.p + k, st);
    cums.resize(nc);
    HIP_CHECK(hipMemcpyAsync(cums.data(), cums_d.p, nc * sizeof(EF), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  }

  // The check's two segment tables (chips with an AIR, lookup-only chips) over the evaluations
  // and the permutation rows where k_perm_rows_machine left them, and the result buffer: chip k's
  // block is {~0, 0, count[K] = 0, first[K] = ~0} at 2 k + 2 (the sum of the earlier K).
  void check_setup() {
    res_at.resize(nc);
    size_t words = 0;
    for (int k = 0; k < nc; k++) {
      res_at[k] = words;
      words += 2 + 2 * (size_t)mc(k).p.num_constraints();
    }
    check_host.assign(words, 0);
    check_res.reset(words);
    MachTable T[2];
    std::memset(T, 0, sizeof T);
    for (int k = 0; k < nc; k++) {  // commit order: tallest first
      const int K = mc(k).p.num_constraints();
      unsigned long long* r = check_host.data() + res_at[k];
      r[0] = ~0ull;
      std::fill(r + 2 + K, r + 2 + 2 * K, ~0ull);
      MachSeg sg{};
      const ChipLists cl = lists(k);
      sg.code = cl.code;
      sg.ncode = (uint32_t)cl.ncode;
      sg.list = cl.list;
      sg.mainc = evals[k].p;
      sg.prepc = prep_evals(k);
      sg.permc = pe[k].p;
      sg.res = check_res.p + res_at[k];
      sg.log_rows = (uint32_t)log2i(hn[k]);
      sg.num_constraints = (uint32_t)K;
      sg.qp.perm_alpha = pch.alpha;
      for (int j = 0; j < 8; j++) sg.qp.beta_pows[j] = pch.beta_pows[j];
      sg.qp.cumsum = cums[k];
      const int tb = cl.ncode > 0 ? 0 : 1;
      push_segment(T[tb], sg, hn[k]);
      check_kmax[tb] = std::max(check_kmax[tb], K);
    }
    upload_async(check_res.p, check_host.data(), words * sizeof(unsigned long long), st);
    for (int tb = 0; tb < 2; tb++) check_tab[tb].upload(T[tb], st);
  }
  void check_segmented() {
    if (check_tab[0].grid) {
      hipLaunchKernelGGL(k_check_machine<1>, dim3(check_tab[0].grid), dim3(256),
                         2 * (size_t)check_kmax[0] * sizeof(uint32_t), st, check_tab[0].d.p,
                         check_kmax[0]);
      KCHECK();
    }
    if (check_tab[1].grid) {
      hipLaunchKernelGGL(k_check_machine<0>, dim3(check_tab[1].grid), dim3(256),
                         2 * (size_t)check_kmax[1] * sizeof(uint32_t), st, check_tab[1].d.p,
                         check_kmax[1]);
      KCHECK();
    }
  }
  void check_download() {
    HIP_CHECK(hipMemcpyAsync(check_host.data(), check_res.p,
                             check_host.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                             st));
    HIP_CHECK(hipStreamSynchronize(st));
  }

  // The chunk matrices (D_k per chip; chunks 0 and D_k / 2 get their own half from the kernel, as
  // the built-in prover places it), every chip's QuotParams block, the two segment tables of
  // slab 0 and those of the further slabs.
  void quot_setup(const EF& alpha) {
    qat.resize(nc);
    qph.resize(nc);
    size_t ktot = 0, nmat = 0;
    for (int k = 0; k < nc; k++) {
      ktot += (size_t)mc(k).p.num_constraints();
      qat[k] = (int)nmat;
      nmat += (size_t)mc(k).p.chunks();
      max_half = std::max(max_half, mc(k).p.chunks() / 2);
    }
    quotr.mats.resize(nmat);
    slab.resize(nc);
    vals.resize(nc);
    MachTable ST[3][2];
    std::memset(ST, 0, sizeof ST);
    std::vector<EF> ap(ktot);
    apows_d.reset(ktot);
    MachTable T[2];
    std::memset(T, 0, sizeof T);
    std::vector<std::pair<int, int>> where(nc);  // (table, segment) of chip k
    sel.resize(nc);
    const uint32_t three = to_mont(3);
    size_t k0 = 0;
    for (int k = 0; k < nc; k++) {
      const size_t n = hn[k];
      const int logn = log2i(n), K = mc(k).p.num_constraints();
      const int lqd = mc(k).p.log_quotient_degree(), D = 1 << lqd, half = D / 2;
      const uint32_t g = two_adic_gen(logn + lqd);
      for (int cc = 0; cc < D; cc++) {
        CMat& qm = quotr.mats[qat[k] + cc];
        qm.n = n;
        qm.log_n = logn;
        qm.shift = mmul(three, mpow(g, (uint64_t)cc));  // split_domains: shift * g^cc
        qm.lde.height = 2 * n;
        qm.lde.width = 4;
        qm.lde.buf.reset(8 * n);
        qm.sharded = false;
        qm.blk = 2 * n;
        qm.row0 = 0;
        for (int j = 0; j < 64; j++) qm.nmap[j] = (uint8_t)j;
      }
      EF pwr = ef_one();  // alpha^(K-1-j): the Horner fold as a sum (quotient.hip)
      for (int j = K - 1; j >= 0; j--) {
        ap[k0 + j] = pwr;
        pwr = ef_mul(pwr, alpha);
      }
      sel[k] = quotient_sel_inv(logn + 1, st);
      MachSeg sg{};
      const ChipLists cl = lists(k);
      sg.code = cl.code;
      sg.ncode = (uint32_t)cl.ncode;
      sg.list = cl.list;
      sg.mainc = mainr.mats[k].lde.buf.p;
      sg.prepc = prep_lde(k);
      sg.permc = permr.mats[k].lde.buf.p;
      sg.sel_inv = sel[k];
      sg.out[0] = quotr.mats[qat[k]].lde.buf.p;
      sg.out[1] = quotr.mats[qat[k] + half].lde.buf.p + n;
      sg.out_stride = 2 * n;
      sg.log_rows = (uint32_t)(logn + 1);
      sg.qp = quot_params_of_height(n, apows_d.p + k0);
      sg.qp.perm_alpha = pch.alpha;
      for (int j = 0; j < 8; j++) sg.qp.beta_pows[j] = pch.beta_pows[j];
      sg.qp.cumsum = cums[k];
      qph[k] = sg.qp;
      const int tb = cl.ncode > 0 ? 0 : 1;
      where[k] = {tb, (int)T[tb].nseg};
      push_segment(T[tb], sg, 2 * n);
      if (half > 1) {  // slabs 1 .. half - 1: the same segment over the slab's LDEs and values
        const int mw = mc(k).p.lk.main_w, pw = mc(k).p.lk.prep_w;
        slab[k].reset(2 * n * (size_t)(mw + pw + 4 * mc(k).p.perm_width()));
        vals[k].reset(8 * n);
        sg.mainc = slab[k].p;
        sg.prepc = pw ? slab[k].p + 2 * n * (size_t)mw : nullptr;
        sg.permc = slab[k].p + 2 * n * (size_t)(mw + pw);
        sg.sel_inv = nullptr;
        sg.out[0] = vals[k].p;
        sg.out[1] = vals[k].p + 4 * n;
        sg.out_stride = n;
        for (int r = 1; r < half; r++) {
          slab_quot_params(sg.qp, n, lqd, r);
          push_segment(ST[r - 1][tb], sg, 2 * n);
        }
      }
      k0 += (size_t)K;
    }
    upload_async(apows_d.p, ap.data(), ktot * sizeof(EF), st);
    for (int tb = 0; tb < 2; tb++) quot_tab[tb].upload(T[tb], st);
    for (int r = 1; r < max_half; r++)
      for (int tb = 0; tb < 2; tb++) slab_tab[r - 1][tb].upload(ST[r - 1][tb], st);
    qp_dev.resize(nc);
    for (int k = 0; k < nc; k++) qp_dev[k] = &quot_tab[where[k].first].d.p->seg[where[k].second].qp;
  }
  // Slab 0 of every chip (the committed LDEs, the cached selector tables), then slab by slab the
  // chips that have one: their LDEs, one launch per class, their two chunks' LDEs.  A machine of
  // D = 2 chips launches slab 0 alone.
  void quotient_segmented() {
    const uint32_t* twf = (const uint32_t*)twiddles().fwd();
    if (quot_tab[0].grid) {
      hipLaunchKernelGGL(k_quotient_machine<1>, dim3(quot_tab[0].grid), dim3(256), 0, st,
                         quot_tab[0].d.p, twf);
      KCHECK();
    }
    if (quot_tab[1].grid) {
      hipLaunchKernelGGL(k_quotient_machine<0>, dim3(quot_tab[1].grid), dim3(256), 0, st,
                         quot_tab[1].d.p, twf);
      KCHECK();
    }
    for (int r = 1; r < max_half; r++) {
      slab_ldes(r);
      for (int tb = 0; tb < 2; tb++)  // (tb = 1, lookup-only: empty today, launch_slab_table)
        if (slab_tab[r - 1][tb].grid) launch_slab_table(slab_tab[r - 1][tb], tb == 0, st);
      slab_chunks(r);
    }
  }
  // Every chip with a slab r: its three traces extended onto S_r = 3 g^r H_2n from the evaluations.
  // The buffer is the one slab r - 1 used; the stream orders the reuse.
  void slab_ldes(int r) {
    for (int k = 0; k < nc; k++) {
      if (mc(k).p.chunks() / 2 <= r) continue;
      const size_t n = hn[k];
      const int mw = mc(k).p.lk.main_w, pw = mc(k).p.lk.prep_w;
      const uint32_t g = two_adic_gen(log2i(n) + mc(k).p.log_quotient_degree());
      const uint32_t shift = mmul(to_mont(3), mpow(g, (uint64_t)r));
      coset_lde(evals[k].p, n, mw, shift, slab[k].p, st);
      if (pw) coset_lde(prep_evals(k), n, pw, shift, slab[k].p + 2 * n * (size_t)mw, st);
      coset_lde(pe[k].p, n, 4 * mc(k).p.perm_width(), shift, slab[k].p + 2 * n * (size_t)(mw + pw), st);
    }
  }
  // The slab's values are chunks r and r + D/2 on their own domains 3 g^j H_n: each chunk's full
  // LDE on 3 H_2n (shift 3 / (3 g^j)), as quotient_slabs extends them.
  void slab_chunks(int r) {
    for (int k = 0; k < nc; k++) {
      const int half = mc(k).p.chunks() / 2;
      if (half <= r) continue;
      const size_t n = hn[k];
      const uint32_t g_inv = minv(two_adic_gen(log2i(n) + mc(k).p.log_quotient_degree()));
      coset_lde(vals[k].p, n, 4, mpow(g_inv, (uint64_t)r), quotr.mats[qat[k] + r].lde.buf.p, st);
      coset_lde(vals[k].p + 4 * n, n, 4, mpow(g_inv, (uint64_t)(r + half)),
                quotr.mats[qat[k] + r + half].lde.buf.p, st);
    }
  }
  // machine_time's form B: chip k's slab r alone, through a one-segment table.  The tables are
  // built and uploaded once, ahead of the timed runs (chip_slab_setup), as quot_setup uploads the
  // segmented form's: slab_chip is a launch and nothing else.
  void chip_slab_setup() {
    chip_slab_tab.clear();
    chip_slab_tab.resize(3 * (size_t)nc);
    for (int k = 0; k < nc; k++) {
      const size_t n = hn[k];
      const int mw = mc(k).p.lk.main_w, pw = mc(k).p.lk.prep_w;
      for (int r = 1; r < mc(k).p.chunks() / 2; r++) {
        QuotParams qp = qph[k];
        slab_quot_params(qp, n, mc(k).p.log_quotient_degree(), r);
        one_slab_table(chip_slab_tab[3 * k + r - 1], lists(k), slab[k].p,
                       pw ? slab[k].p + 2 * n * (size_t)mw : nullptr,
                       slab[k].p + 2 * n * (size_t)(mw + pw), log2i(n) + 1, qp,
                       QuotOut{{vals[k].p, vals[k].p + 4 * n}, n}, st);
      }
    }
  }
  void slab_chip(int k, int r) { launch_slab_table(chip_slab_tab[3 * k + r - 1], lists(k).ncode > 0, st); }
  QuotOut quot_out(int k) {
    const int half = mc(k).p.chunks() / 2;
    return QuotOut{{quotr.mats[qat[k]].lde.buf.p, quotr.mats[qat[k] + half].lde.buf.p + hn[k]}, 2 * hn[k]};
  }
  void quot_commit() {
    for (int k = 0; k < nc; k++)
      for (int cc = 0; cc < 2; cc++) {  // the other half of the LDEs of chunks 0 and D/2 (slab 0)
        CMat& qm = quotr.mats[qat[k] + cc * (mc(k).p.chunks() / 2)];
        const uint32_t lde_shift = mmul(to_mont(3), minv(qm.shift));  // GENERATOR / shift
        coset_lde_ex(qm.lde.buf.p + (size_t)cc * hn[k], 2 * hn[k], hn[k], 4, lde_shift, qm.lde.buf.p,
                     1 - cc, st);
      }
    quotr.commit(st, /*fetch_root=*/true);
  }
};

struct Bytes {  // the BFZ1 writer (canonical words)
  std::vector<uint8_t> b;
  void put(const void* p, size_t k) {
    const uint8_t* q = static_cast<const uint8_t*>(p);
    b.insert(b.end(), q, q + k);
  }
  void u32(uint32_t v) { put(&v, 4); }
  void ef(const EF& e) {
    for (int i = 0; i < 4; i++) u32(from_mont(e.c[i]));
  }
  void digest(const uint32_t* d) {
    for (int i = 0; i < 8; i++) u32(from_mont(d[i]));
  }
};

struct CallEnd {  // the pinned upload arena is rewound when the call is done
  hipStream_t st;
  ~CallEnd() {
    (void)hipStreamSynchronize(st);
    staging_reset();
  }
};
}  // namespace

// The preprocessed side of a proving machine: the device lists, then every preprocessed trace
// uploaded, transposed and committed as setup commits Program and Byte (shift 1).
void machine_commit_prep(MachineProgram& m, const MachineChipIn* in) {
  if (api_lock_depth() == 0) throw std::logic_error("machine_create called outside the bfz API lock");
  ResidentScope rs;  // the machine lives beside the tables, outside every lane's working set
  hipStream_t st = stream();
  CallEnd end{st};
  twiddles().ensure(TWIDDLE_LOG_MAX);
  for (MachineChip& c : m.chips) {
    c.list.reset(c.p.lk.list.size());
    upload_async(c.list.p, c.p.lk.list.data(), c.p.lk.list.size() * 4, st);
    if (c.p.has_air) {
      c.code.reset(c.p.air.code.size());
      upload_async(c.code.p, c.p.air.code.data(), c.p.air.code.size() * 4, st);
    }
  }
  m.prep.mats.resize(m.prep_chips.size());
  for (size_t k = 0; k < m.prep_chips.size(); k++) {
    const int i = m.prep_chips[k];
    MachineChip& c = m.chips[i];
    c.prep_evals = uni_upload_trace((size_t)c.p.lk.prep_w, c.name.c_str(), in[i].prep, c.prep_height, st);
    commit_lde(m.prep.mats[k], c.prep_evals.p, c.prep_height, c.p.lk.prep_w, ONE, st);
  }
  if (m.has_prep) {
    m.prep.commit(st, /*fetch_root=*/true);
    std::memcpy(m.prep_root, m.prep.tree.root, 32);
  }
  HIP_CHECK(hipStreamSynchronize(st));
}

std::vector<uint8_t> machine_prove(const MachineProgram& m, const int* chips,
                                   const uint32_t* const* traces, const size_t* heights, size_t n,
                                   Challenger& ch_io, const ProveOptions& opt) {
  if (api_lock_depth() == 0) throw std::logic_error("machine_prove called outside the bfz API lock");
  if (!m.can_prove) throw std::runtime_error("machine: a verifier-only machine cannot prove");
  if (opt.num_queries < 1 || opt.num_queries > 4096) throw std::runtime_error("machine: bad query count");
  hipStream_t st = stream();
  CallEnd end{st};
  Prover P(m, st);
  Challenger ch = ch_io;
  P.commit_main(chips, traces, heights, n);            // stages 1-3
  const int nc = P.nc;
  ch.observe_digest(P.mainr.tree.root);                // 4 (prover.rs:265-272)
  const EF pa = ch.sample_ef(), pb = ch.sample_ef();
  P.perm_setup(pa, pb);                                // 5 (prover.rs:281-333)
  P.perm_rows_segmented();
  P.perm_commit();
  ch.observe_digest(P.permr.tree.root);                // 6 (prover.rs:336-342)
  for (int k = 0; k < nc; k++) ch.observe_ef(P.cums[k]);
  const EF alpha = ch.sample_ef();
  P.quot_setup(alpha);                                 // 7 (prover.rs:344-412)
  P.quotient_segmented();
  P.quot_commit();
  ch.observe_digest(P.quotr.tree.root);                // 8 (prover.rs:413-416)
  const EF zeta = ch.sample_ef();

  // ---- 9: PCS open (prover.rs:417-470) over {preprocessed (when present), main, permutation,
  // quotient}; a local-only chip's main (and preprocessed) matrix is opened at zeta alone
  DBuf<EF> zeta_d(1);
  upload_async(zeta_d.p, &zeta, sizeof(EF), st);
  PcsOpenIn oin;
  const int r0 = m.has_prep ? 1 : 0;
  if (m.has_prep) {
    PcsRound pr{&m.prep, 0, {}};
    for (int pc : m.prep_chips) pr.two.push_back(m.chips[pc].local_only ? 0 : 1);
    oin.rounds.push_back(std::move(pr));
  }
  {
    PcsRound mr{&P.mainr, 0, {}};
    for (int k = 0; k < nc; k++) mr.two.push_back(P.mc(k).local_only ? 0 : 1);
    oin.rounds.push_back(std::move(mr));
    oin.rounds.push_back(PcsRound{&P.permr, 1, std::vector<uint8_t>((size_t)nc, 1)});
    oin.rounds.push_back(PcsRound{&P.quotr, 2, std::vector<uint8_t>(P.quotr.mats.size(), 0)});
  }
  oin.zeta_d = zeta_d.p;  // (the unsharded plan reads zeta from the device alone)
  oin.observe_openings = opt.observe_openings;
  oin.num_queries = opt.num_queries;
  EvTimer ev;
  StageTimes tms;
  oin.ev = &ev;
  oin.tms = &tms;
  const PcsOpenOut po = pcs_open(oin, ch);
  const std::vector<EF>& opened = po.opened;
  const std::vector<std::vector<PcsOpenOut::MatPts>>& mp = po.mp;

  // ---- 10: the proof (BFZ1; a chip word is the chip's index in the machine's list)
  Bytes w;
  w.b.reserve(4 * po.nwords + ((size_t)64 << 10));
  w.u32(0x315a4642u);
  w.u32((uint32_t)nc);
  for (int k = 0; k < nc; k++) {
    const std::string& nm = P.mc(k).name;
    w.u32((uint32_t)P.chip[k]);
    w.u32((uint32_t)nm.size());
    w.put(nm.data(), nm.size());
  }
  w.digest(P.mainr.tree.root);
  w.digest(P.permr.tree.root);
  w.digest(P.quotr.tree.root);
  auto vals = [&](const PcsOpenOut::MatPts& pts, int pt, int width) {  // zeros where not opened
    w.u32((uint32_t)width);
    for (int c = 0; c < width; c++) w.ef(pt < pts.npts ? opened[pts.off[pt] + c] : ef_zero());
  };
  for (int k = 0; k < nc; k++) {
    w.u32((uint32_t)P.mainr.mats[k].log_n);
    const int pi = P.mc(k).prep_index;
    if (pi >= 0) {
      vals(mp[0][pi], 0, P.mc(k).p.lk.prep_w);
      vals(mp[0][pi], 1, P.mc(k).p.lk.prep_w);
    } else {
      w.u32(0);
      w.u32(0);
    }
    vals(mp[r0][k], 0, P.mc(k).p.lk.main_w);
    vals(mp[r0][k], 1, P.mc(k).p.lk.main_w);
    vals(mp[r0 + 1][k], 0, 4 * P.mc(k).p.perm_width());
    vals(mp[r0 + 1][k], 1, 4 * P.mc(k).p.perm_width());
    const int D = P.mc(k).p.chunks();  // 2 unless the chip's AIR has degree above 3
    w.u32((uint32_t)D);
    for (int j = 0; j < D; j++) vals(mp[r0 + 2][P.qat[k] + j], 0, 4);
    w.ef(P.cums[k]);
  }
  w.u32((uint32_t)po.commit_roots.size());
  for (const Digest& d : po.commit_roots) w.digest(d.data());
  w.u32((uint32_t)opt.num_queries);
  w.put(po.words, 4 * po.nwords);  // every query in serialized form
  w.ef(po.final_poly);
  w.u32(po.pow_witness);
  ch_io = ch;
  return std::move(w.b);
}

// machine_check's device path (machine_program.cpp refuses a verifier-only machine first): the
// traces uploaded and transposed once, the permutation rows and running sums, the segmented
// check.  Only the cumulative sums and the result words come back.
MachineCheck machine_check_device(const MachineProgram& m, const int* chips,
                                  const uint32_t* const* traces, const size_t* heights, size_t n,
                                  Challenger& ch) {
  if (api_lock_depth() == 0) throw std::logic_error("machine_check called outside the bfz API lock");
  hipStream_t st = stream();
  CallEnd end{st};
  Prover P(m, st);
  P.commit_main(chips, traces, heights, n, /*tree=*/false, /*lde=*/false);
  const int nc = P.nc;
  MachineCheck out;
  out.alpha = ch.sample_ef();  // machine.rs:300-303
  out.beta = ch.sample_ef();
  P.perm_setup(out.alpha, out.beta);
  P.perm_rows_segmented();
  P.perm_sums();
  P.check_setup();
  P.check_segmented();
  P.check_download();

  std::vector<size_t> k0(n + 1, 0);  // the profile's prefix sums, in the caller's order
  for (size_t i = 0; i < n; i++) k0[i + 1] = k0[i] + (size_t)m.chips[chips[i]].p.num_constraints();
  out.chips.resize(n);
  out.counts.resize(k0[n]);
  out.first_rows.resize(k0[n]);
  out.cumsum = ef_zero();
  out.ok = true;
  for (int k = 0; k < nc; k++) {
    const size_t i = (size_t)P.order[k];
    const int K = P.mc(k).p.num_constraints();
    const unsigned long long* r = P.check_host.data() + P.res_at[k];
    ChipCheck& cc = out.chips[i];
    cc.chip = P.chip[k];
    cc.height = P.hn[k];
    cc.num_constraints = K;
    cc.num_batches = P.mc(k).p.lk.batches();
    cc.cumsum = P.cums[k];
    decode_check_result(r, cc);
    for (int j = 0; j < K; j++) {
      out.counts[k0[i] + j] = r[2 + j];
      out.first_rows[k0[i] + j] = r[2 + K + j] == ~0ull ? -1 : (int64_t)r[2 + K + j];
    }
    out.cumsum = ef_add(out.cumsum, P.cums[k]);
    out.ok = out.ok && cc.failing_rows == 0;
  }
  out.ok = out.ok && ef_is_zero(out.cumsum);
  return out;
}

void machine_time(const MachineProgram& m, const int* chips, const uint32_t* const* traces,
                  const size_t* heights, size_t n, int runs, float* perm_ms, float* quot_ms) {
  if (api_lock_depth() == 0) throw std::logic_error("machine_time called outside the bfz API lock");
  if (runs < 1 || !perm_ms || !quot_ms) throw std::runtime_error("machine_time: bad arguments");
  hipStream_t st = stream();
  CallEnd end{st};
  Prover P(m, st);
  // The LDEs without the Merkle trees, which neither form reads: the challenges come from the
  // transcript head alone (a proof takes at most MACHINE_MAX_SAME_HEIGHT chips of one height, the
  // launches measured here any number).
  Challenger ch;
  machine_observe(m, ch);
  P.commit_main(chips, traces, heights, n, /*tree=*/false);
  const int nc = P.nc;
  const EF pa = ch.sample_ef(), pb = ch.sample_ef();
  P.perm_setup(pa, pb);
  DBuf<PermChallenges> chd(1);
  upload_async(chd.p, &P.pch, sizeof(PermChallenges), st);
  struct Events {  // destroyed on every way out, the "differ" errors below included
    hipEvent_t e[2] = {nullptr, nullptr};
    ~Events() {
      for (hipEvent_t x : e)
        if (x) (void)hipEventDestroy(x);
    }
  } evs;
  HIP_CHECK(hipEventCreate(&evs.e[0]));
  HIP_CHECK(hipEventCreate(&evs.e[1]));
  const hipEvent_t e0 = evs.e[0], e1 = evs.e[1];
  auto timed = [&](auto&& body) {
    HIP_CHECK(hipEventRecord(e0, st));
    body();
    HIP_CHECK(hipEventRecord(e1, st));
    HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    return ms;
  };
  // Both forms write the same buffers: the warm-up round keeps form B's words, clears the
  // buffers and compares what form A then writes.
  auto clear = [&](const std::vector<const uint32_t*>& dst, const std::vector<size_t>& words) {
    for (size_t i = 0; i < dst.size(); i++)
      HIP_CHECK(hipMemsetAsync(const_cast<uint32_t*>(dst[i]), 0, words[i] * 4, st));
  };
  auto snapshot = [&](const std::vector<const uint32_t*>& src, const std::vector<size_t>& words) {
    std::vector<std::vector<uint32_t>> out(src.size());
    for (size_t i = 0; i < src.size(); i++) {
      out[i].resize(words[i]);
      HIP_CHECK(hipMemcpyAsync(out[i].data(), src[i], words[i] * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipStreamSynchronize(st));
    return out;
  };
  auto perm_loop = [&] {
    for (int k = 0; k < nc; k++)
      perm_rows_prog(P.mc(k).p.lk, P.mc(k).list.p, P.evals[k].p, P.prep_evals(k), P.hn[k], chd.p,
                     P.pe[k].p, P.rows[k].p, st);
  };
  std::vector<const uint32_t*> psrc;
  std::vector<size_t> pwords;
  for (int k = 0; k < nc; k++) {  // the batch columns and the row sums
    psrc.push_back(P.pe[k].p);
    pwords.push_back(4 * (size_t)P.mc(k).p.lk.batches() * P.hn[k]);
    psrc.push_back((const uint32_t*)P.rows[k].p);
    pwords.push_back(4 * P.hn[k]);
  }
  for (int r = -1; r < runs; r++) {  // r = -1: the warm-up launches
    const float b = timed(perm_loop);
    const auto wb = r < 0 ? snapshot(psrc, pwords) : std::vector<std::vector<uint32_t>>();
    if (r < 0) clear(psrc, pwords);
    const float a = timed([&] { P.perm_rows_segmented(); });
    if (r < 0 && snapshot(psrc, pwords) != wb)
      throw std::runtime_error("machine_time: the segmented permutation rows differ from the per-chip launches'");
    if (r >= 0) {
      perm_ms[r] = a;
      perm_ms[runs + r] = b;
    }
  }
  P.perm_commit(/*tree=*/false);
  for (int k = 0; k < nc; k++) ch.observe_ef(P.cums[k]);
  P.quot_setup(ch.sample_ef());
  P.chip_slab_setup();
  const uint32_t* twf = (const uint32_t*)twiddles().fwd();
  auto quot_loop = [&] {
    for (int k = 0; k < nc; k++)
      launch_quotient_chip_prog(P.lists(k), P.mainr.mats[k].lde.buf.p, P.prep_lde(k),
                                P.permr.mats[k].lde.buf.p, log2i(P.hn[k]) + 1, P.qp_dev[k], twf,
                                P.sel[k], P.quot_out(k), st);
    for (int r = 1; r < P.max_half; r++) {  // the further slabs of the chips of degree above 3
      P.slab_ldes(r);
      for (int k = 0; k < nc; k++)
        if (P.mc(k).p.chunks() / 2 > r) P.slab_chip(k, r);
      P.slab_chunks(r);
    }
  };
  std::vector<const uint32_t*> qsrc;
  std::vector<size_t> qwords;
  for (int k = 0; k < nc; k++)
    for (int j = 0; j < P.mc(k).p.chunks(); j++) {
      qsrc.push_back(P.quotr.mats[P.qat[k] + j].lde.buf.p);
      qwords.push_back(8 * P.hn[k]);
    }
  clear(qsrc, qwords);  // (the halves the kernels do not write hold whatever the pool left there)
  for (int r = -1; r < runs; r++) {
    const float b = timed(quot_loop);
    const auto wb = r < 0 ? snapshot(qsrc, qwords) : std::vector<std::vector<uint32_t>>();
    if (r < 0) clear(qsrc, qwords);
    const float a = timed([&] { P.quotient_segmented(); });
    if (r < 0 && snapshot(qsrc, qwords) != wb)
      throw std::runtime_error("machine_time: the segmented quotient differs from the per-chip launches'");
    if (r >= 0) {
      quot_ms[r] = a;
      quot_ms[runs + r] = b;
    }
  }
}

// One chip's slab through the segmented kernel (chip_program.h; bfz_chip_quotient): a table of
// one segment, built and uploaded by the call.
void quotient_chip_slab(const ChipLists& cl, const uint32_t* mainc, const uint32_t* prepc,
                        const uint32_t* permc, int logN, const QuotParams& slab_qp,
                        const QuotOut& out, hipStream_t st) {
  if (!cl.list || !mainc || !permc) throw std::runtime_error("chip program: null device argument");
  if (logN < 1 || logN > 23) throw std::runtime_error("quotient_chip_slab: bad LDE height");
  twiddles().ensure(logN);
  DevTable dt;  // (freed stream-ordered after the launch)
  one_slab_table(dt, cl, mainc, prepc, permc, logN, slab_qp, out, st);
  launch_slab_table(dt, cl.ncode > 0 && cl.code, st);
}

// kernels a machine proof launches beside the built-in prover's (gpu.h PreloadKernels)
static PreloadKernels preload_machine_program{(const void*)&k_quotient_machine<0>,
                                              (const void*)&k_quotient_machine<1>,
                                              (const void*)&k_quotient_machine_coset<0>,
                                              (const void*)&k_quotient_machine_coset<1>,
                                              (const void*)&k_perm_rows_machine<1>,
                                              (const void*)&k_check_machine<0>,
                                              (const void*)&k_check_machine<1>};

}  // namespace bfz
