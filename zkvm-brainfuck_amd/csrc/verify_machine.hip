// Query phase of the machine verifier on the device (see verify_machine.h for the packed batch).
//
// Four kernels, all indexed by proof = blockIdx.y:
//   k_mverify_reduce  one block per (proof, LDE height): the reduced opening of every query at that
//                     height.  It is two dot products over the height's columns whose EF
//                     coefficients (alpha^k at the two points) are the same for every query, so the
//                     block stages them in LDS once and its waves take the queries in turn; then
//                     one thread per query finishes with the two inversions
//   k_mverify_fold    one thread per query: the fold chain over the reduced openings; writes each
//                     commit-phase step's leaf and compares the final value
//   k_mverify_paths   one 16-lane row per (query, step): the leaf's hash up its path
//   k_mverify_inputs  one 16-lane row per (query, input round): MerkleTreeMmcs::verify_batch over a
//                     group table of any length
// The work of the reduced openings grows with the columns a machine opens (32 chips of wide rows:
// several thousand per height), which one thread per query -- verify.hip's k_verify_fold -- would
// walk as one dependent chain; here it is spread over the lanes of a wave and the heights over
// blocks.  The lane-mode kernels are verify.hip's with tables read through offsets: every loop
// bound is a descriptor word that is the same for the whole 16-lane row.
#include "verify_machine.h"

#include "gpu.h"
#include "verify_dev.h"

namespace bfz {

using namespace kb;
using namespace vdev;

namespace {

// k_mverify_reduce's LDS: a tile of MQ_TILE columns' coefficients at both points (2 x 16 KiB) and
// the running sums of MQ_QPASS queries (4 KiB): 36 KiB a block, four blocks (16 waves) a CU of the
// 160 KiB.  A height of a proof rarely has more than one tile: it takes eight chips of the widest
// shape -- 64 main, 68 permutation, 8 quotient words, 1120 columns -- at one height.
constexpr uint32_t MQ_TILE = 1024, MQ_QPASS = 128, MQ_WAVES = 4;

__device__ __forceinline__ const MQProof* proof_desc(const uint32_t* B, uint32_t np, uint32_t proof) {
  return reinterpret_cast<const MQProof*>(B + np + 64) + proof;
}

__global__ __launch_bounds__(64 * MQ_WAVES) void k_mverify_reduce(const uint32_t* __restrict__ B,
                                                                  uint32_t np,
                                                                  uint32_t* __restrict__ rows_ro) {
  __shared__ __attribute__((aligned(16))) uint32_t s_c0[4 * MQ_TILE];
  __shared__ __attribute__((aligned(16))) uint32_t s_c1[4 * MQ_TILE];
  __shared__ uint32_t s_part[MQ_QPASS][8];
  // everything read from the descriptors is the same for the whole block: scalar loads
  const uint32_t proof = blockIdx.y;
  const MQProof* __restrict__ D = proof_desc(B, np, proof);
  if (blockIdx.x >= D->nheights) return;
  const MQHeight* __restrict__ H = reinterpret_cast<const MQHeight*>(B + D->ht_off) + blockIdx.x;
  const uint32_t nq = D->nq, ncols = H->ncols, lh = H->lh, log_max = D->log_max;
  const uint32_t c1 = H->seg_c0[1], c2 = H->seg_c0[2], c3 = H->seg_c0[3];
  const uint32_t d0 = H->seg_delta[0], d1 = H->seg_delta[1], d2 = H->seg_delta[2], d3 = H->seg_delta[3];
  if (ncols == 0) return;  // (no machine makes one: the slot stays zero, which is the empty sum)
  const uint32_t* __restrict__ coef0 = B + H->coef_off;
  const uint32_t* __restrict__ coef1 = coef0 + 4 * (size_t)ncols;
  const uint32_t* __restrict__ recs = B + D->qbase;
  const uint32_t qstride = D->qstride;
  const uint32_t gen_lh = B[np + lh];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t three = to_mont_c(3);

  for (uint32_t q0 = 0; q0 < nq; q0 += MQ_QPASS) {
    const uint32_t q1 = nq - q0 < MQ_QPASS ? nq : q0 + MQ_QPASS;
    for (uint32_t t0 = 0; t0 < ncols; t0 += MQ_TILE) {
      const uint32_t tn = ncols - t0 < MQ_TILE ? ncols - t0 : MQ_TILE;
      __syncthreads();  // the tile before this one has been read
      for (uint32_t i = threadIdx.x; i < 4 * tn; i += 64 * MQ_WAVES) {
        s_c0[i] = coef0[4 * (size_t)t0 + i];
        s_c1[i] = coef1[4 * (size_t)t0 + i];
      }
      __syncthreads();
      for (uint32_t q = q0 + wave; q < q1; q += MQ_WAVES) {
        const uint32_t* __restrict__ rec = recs + (size_t)q * qstride;
        LazyEF s0, s1;
        s0.init();
        s1.init();
        for (uint32_t c = lane; c < tn; c += 64) {  // consecutive lanes: consecutive record words
          const uint32_t col = t0 + c;
          const uint32_t v = rec[col + (col >= c1 ? (col >= c2 ? (col >= c3 ? d3 : d2) : d1) : d0)];
          const kb_u32x4 k0 = *reinterpret_cast<const kb_u32x4*>(&s_c0[4 * c]);
          const kb_u32x4 k1 = *reinterpret_cast<const kb_u32x4*>(&s_c1[4 * c]);
          s0.add(EF{{k0.x, k0.y, k0.z, k0.w}}, v);
          s1.add(EF{{k1.x, k1.y, k1.z, k1.w}}, v);
        }
        EF e0 = s0.get(), e1 = s1.get();
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
          for (int e = 0; e < 4; e++) {
            e0.c[e] = madd(e0.c[e], __shfl_xor(e0.c[e], off, 64));
            e1.c[e] = madd(e1.c[e], __shfl_xor(e1.c[e], off, 64));
          }
        }
        if (lane == 0) {  // this wave alone owns query q's running sums
          uint32_t* __restrict__ part = s_part[q - q0];
          if (t0) {
            e0 = ef_add(e0, ld_ef(part));
            e1 = ef_add(e1, ld_ef(part + 4));
          }
#pragma unroll
          for (int e = 0; e < 4; e++) {
            part[e] = e0.c[e];
            part[4 + e] = e1.c[e];
          }
        }
      }
    }
    // The pass's sums are complete.  The two inversions of a query are a long dependent chain:
    // finished by the wave that summed it, a wave's queries would wait on one another in lane 0;
    // here one thread finishes one query (MQ_QPASS <= the block's threads).
    __syncthreads();
    const uint32_t q = q0 + threadIdx.x;
    if (q < q1) {
      const uint32_t* __restrict__ part = s_part[threadIdx.x];
      const uint32_t index = B[D->idx_off + q];
      const uint32_t x = mmul(three, mpow(gen_lh, dbitrev(index >> (log_max - lh), (int)lh)));
      EF r = ef_mul(ef_sub(ld_ef(part), H->a0), ef_inv(ef_sub(ef_base(x), H->z0)));
      // (a height opened at one point only has coef1 = 0 and a1 = 0)
      r = ef_add(r, ef_mul(ef_sub(ld_ef(part + 4), H->a1), ef_inv(ef_sub(ef_base(x), H->z1))));
      uint32_t* __restrict__ ro = rows_ro + D->ro_base + ((size_t)q * VQ_RO_SLOTS + lh) * 4;
#pragma unroll
      for (int e = 0; e < 4; e++) ro[e] = r.c[e];
    }
  }
}
static_assert(MQ_QPASS <= 64 * MQ_WAVES, "one thread finishes one query of a pass");

// verify_query: fold with the sibling and beta_s, add the next height's reduced opening (a slot no
// height wrote is zero).
__global__ __launch_bounds__(64) void k_mverify_fold(uint32_t* __restrict__ B, uint32_t np,
                                                     uint32_t* __restrict__ leaves,
                                                     const uint32_t* __restrict__ rows_ro) {
  const uint32_t proof = blockIdx.y;
  const MQProof* __restrict__ D = proof_desc(B, np, proof);
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= D->nq) return;
  const uint32_t* __restrict__ gen = B + np;
  const uint32_t* __restrict__ gen_inv = B + np + 32;
  const uint32_t* __restrict__ ro = rows_ro + D->ro_base + (size_t)q * (VQ_RO_SLOTS * 4);
  const uint32_t log_max = D->log_max, nc = D->ncommit;
  const uint32_t neg_half = mneg(to_mont_c((P + 1) / 2));
  EF folded = ef_zero();
  uint32_t idx = B[D->idx_off + q];
  const uint32_t* __restrict__ step = B + D->qbase + (size_t)q * D->qstride + D->steps_off;
  uint32_t* __restrict__ leaf = leaves + D->leaf_base + (size_t)q * nc * 8;
  for (uint32_t s = 0; s < nc; s++) {
    const uint32_t lfh = log_max - 1 - s;
    folded = ef_add(folded, ld_ef(ro + 4 * (lfh + 1)));
    const EF sib = ld_ef(step);
    step += 4 + 8 * lfh;
    const bool odd = idx & 1;
    const EF ev0 = odd ? sib : folded, ev1 = odd ? folded : sib;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      leaf[8 * s + k] = ev0.c[k];
      leaf[8 * s + 4 + k] = ev1.c[k];
    }
    idx >>= 1;
    const uint32_t rev = dbitrev(idx, (int)lfh);
    const uint32_t x0 = mpow(gen[lfh + 1], rev);
    // 1 / (x1 - x0) with x1 = -x0: -1/2 * x0^-1
    const uint32_t inv = mmul(neg_half, mpow(gen_inv[lfh + 1], rev));
    const EF t = ef_mul(ef_sub(ld_ef(B + D->beta_off + 4 * s), ef_base(x0)), ef_sub(ev1, ev0));
    folded = ef_add(ev0, ef_mul_base(t, inv));
  }
  // a 1-row trace's height-2 input joins after the last fold (D11)
  folded = ef_add(folded, ld_ef(ro + 4 * (log_max - nc)));
  if (!ef_eq(folded, D->final_poly)) report(B, proof, q, VQ_STAGE_FINAL);
}

// k_verify_fri_paths over an MQProof (that kernel strides verify.h's VProof array).
__global__ __launch_bounds__(256) void k_mverify_paths(uint32_t* __restrict__ B, uint32_t np,
                                                       const uint32_t* __restrict__ leaves) {
  const uint32_t proof = blockIdx.y;
  const MQProof* __restrict__ D = proof_desc(B, np, proof);
  const uint32_t job = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const int lane = threadIdx.x & 15;
  const uint32_t nc = D->ncommit;
  if (nc == 0 || job >= D->nq * nc) return;
  const uint32_t q = job / nc, s = job - q * nc;
  const LaneConsts kc = lane_consts(lane);
  const uint32_t lfh = D->log_max - 1 - s;
  // step s of the record: after the s earlier steps' siblings and paths, past this one's sibling
  const uint32_t soff = D->steps_off + 4 * s + 8 * (s * (D->log_max - 1) - s * (s - 1) / 2) + 4;
  const uint32_t* __restrict__ path = B + D->qbase + (size_t)q * D->qstride + soff;
  const uint32_t* __restrict__ leaf = leaves + D->leaf_base + ((size_t)q * nc + s) * 8;
  uint32_t idx = (B[D->idx_off + q] >> s) >> 1;
  uint32_t node = poseidon2_permute_lane(lane < 8 ? leaf[lane] : 0u, lane, kc);
  for (uint32_t L = 0; L < lfh; L++) {
    node = path_step_lane(node, path + 8 * L, idx & 1, lane, kc);
    idx >>= 1;
  }
  if (lane < 8 && node != B[D->croot_off + 8 * s + lane]) report(B, proof, q, VQ_STAGE_STEP0 + s);
}

__global__ __launch_bounds__(256) void k_mverify_inputs(uint32_t* __restrict__ B, uint32_t np) {
  const uint32_t proof = blockIdx.y;
  const MQProof* __restrict__ D = proof_desc(B, np, proof);
  const uint32_t job = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const int lane = threadIdx.x & 15;
  const uint32_t nr = D->nrounds;  // 0 in an empty slot
  if (job >= D->nq * nr) return;
  const uint32_t q = job / nr, rr = job - q * nr;
  const LaneConsts kc = lane_consts(lane);
  const MQRound* __restrict__ R = reinterpret_cast<const MQRound*>(B + D->rd_off) + rr;
  const uint32_t* __restrict__ grp = B + R->grp_off;  // (log height, total width), tallest first
  const uint32_t* __restrict__ rec = B + D->qbase + (size_t)q * D->qstride;
  const uint32_t* __restrict__ rows = rec + R->rows_off;
  const uint32_t* __restrict__ path = rec + R->path_off;
  const uint32_t lb = R->lb, ng = R->ngroups;
  uint32_t idx = B[D->idx_off + q] >> (D->log_max - lb);
  uint32_t at = grp[1], g = 1, cur = lb;
  uint32_t node = sponge_lane(rows, at, lane, kc);
  for (uint32_t L = 0; L < lb; L++) {
    node = path_step_lane(node, path + 8 * L, idx & 1, lane, kc);
    idx >>= 1;
    cur--;
    if (g < ng && grp[2 * g] == cur) {  // shorter matrices join here: compress(node, their hash)
      const uint32_t w = grp[2 * g + 1];
      const uint32_t hh = sponge_lane(rows + at, w, lane, kc);
      node = compress_lane(node, hh, lane, kc);
      at += w;
      g++;
    }
  }
  if (g != ng || (lane < 8 && node != R->root[lane])) report(B, proof, q, rr);
}

}  // namespace

namespace {
// The launches of one pass over an uploaded batch.  ev: nullptr, or six events recorded around the
// clearing of the reduced-openings workspace and the four kernels, in launch order.
void launch_queries(const QueryBatch& b, uint32_t* d, uint32_t* leaves, uint32_t* ro, size_t ro_words,
                    hipStream_t st, hipEvent_t* ev) {
  const uint32_t np = b.nproofs;
  auto mark = [&](int k) {
    if (ev) HIP_CHECK(hipEventRecord(ev[k], st));
  };
  mark(0);
  // a height the proof does not have leaves its slot zero
  HIP_CHECK(hipMemsetAsync(ro, 0, ro_words * 4, st));
  mark(1);
  if (b.max_nheights) {
    hipLaunchKernelGGL(k_mverify_reduce, dim3(b.max_nheights, np), dim3(64 * MQ_WAVES), 0, st, d, np, ro);
    KCHECK();
  }
  mark(2);
  hipLaunchKernelGGL(k_mverify_fold, dim3(ceil_div(b.max_nq, 64), np), dim3(64), 0, st, d, np, leaves, ro);
  KCHECK();
  mark(3);
  if (b.max_ncommit) {
    hipLaunchKernelGGL(k_mverify_paths, dim3(ceil_div((size_t)b.max_nq * b.max_ncommit * 16, 256), np),
                       dim3(256), 0, st, d, np, leaves);
    KCHECK();
  }
  mark(4);
  hipLaunchKernelGGL(k_mverify_inputs, dim3(ceil_div((size_t)b.max_nq * b.max_nrounds * 16, 256), np),
                     dim3(256), 0, st, d, np);
  KCHECK();
  mark(5);
}
}  // namespace

void machine_queries_device(const QueryBatch& b, uint32_t* keys, hipStream_t st) {
  if (b.nproofs == 0 || b.max_nq == 0) return;
  if (b.nproofs > 65535) throw std::runtime_error("verify: too many proofs in one device pass");
  DBuf<uint32_t> d(b.words.size()), leaves(std::max<size_t>(b.leaf_words, 1)),
      ro(std::max<size_t>(b.ro_words, 1));
  upload_bulk(d.p, b.words.data(), b.words.size() * 4, st);
  launch_queries(b, d.p, leaves.p, ro.p, ro.n, st, nullptr);
  HIP_CHECK(hipMemcpyAsync(keys, d.p, (size_t)b.nproofs * 4, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
}

void machine_queries_time(const QueryBatch& b, int runs, float* ms, hipStream_t st) {
  if (b.nproofs == 0 || b.max_nq == 0 || b.nproofs > 65535)
    throw std::runtime_error("machine_verify_time: nothing to time");
  DBuf<uint32_t> d(b.words.size()), leaves(std::max<size_t>(b.leaf_words, 1)),
      ro(std::max<size_t>(b.ro_words, 1));
  upload_bulk(d.p, b.words.data(), b.words.size() * 4, st);
  hipEvent_t ev[6];
  for (hipEvent_t& e : ev) HIP_CHECK(hipEventCreate(&e));
  // a pass only lowers keys and rewrites the workspaces with the same words: it can be repeated
  for (int r = -1; r < runs; r++) {  // one warm-up pass
    launch_queries(b, d.p, leaves.p, ro.p, ro.n, st, ev);
    HIP_CHECK(hipStreamSynchronize(st));
    if (r < 0) continue;
    for (int k = 0; k < 5; k++) HIP_CHECK(hipEventElapsedTime(&ms[5 * r + k], ev[k], ev[k + 1]));
  }
  for (hipEvent_t& e : ev) HIP_CHECK(hipEventDestroy(e));
}

}  // namespace bfz
