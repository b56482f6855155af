// Query phase of the verifier on the device (see verify.h for the packed batch).
//
// Three kernels, all indexed by (proof = blockIdx.y, job = position along x):
//   k_verify_fold       one thread per query: the reduced openings of every LDE height, then the
//                       fold chain; writes each commit-phase step's leaf and compares the final value
//   k_verify_fri_paths  one 16-lane group per (query, step): the leaf's hash up its path
//   k_verify_inputs     one 16-lane group per (query, input round): MerkleTreeMmcs::verify_batch
// The Merkle chains are about a hundred dependent permutations deep and there are only a few
// thousand of them, so they run in lane mode (poseidon2_permute_lane: one state per 16-lane DPP
// row).  A group's lanes always branch together: every loop bound below is a descriptor word that
// is the same for the whole group, so whole rows are active around every DPP step (as
// k_compress_top requires).
#include "verify.h"

#include "gpu.h"
#include "poseidon2.h"

namespace bfz {

using namespace kb;

namespace {

__device__ __forceinline__ EF ld_ef(const uint32_t* p) { return EF{{p[0], p[1], p[2], p[3]}}; }
__device__ __forceinline__ void report(uint32_t* keys, uint32_t proof, uint32_t q, uint32_t stage) {
  atomicMin(&keys[proof], q * 64u + stage);
}

// PaddingFreeSponge (overwrite mode, rate 8) of `w` consecutive words in lane mode; the digest is
// lanes 0..7 of the result.
__device__ __forceinline__ uint32_t sponge_lane(const uint32_t* __restrict__ row, uint32_t w, int lane,
                                                const LaneConsts& kc) {
  uint32_t h = 0;
  for (uint32_t at = 0; at < w; at += 8) {
    const uint32_t m = w - at < 8 ? w - at : 8;
    if ((uint32_t)lane < m) h = row[at + lane];
    h = poseidon2_permute_lane(h, lane, kc);
  }
  return h;
}
// compress(l, r) with l in lanes 0..7 of `l` and r in lanes 0..7 of `r`
__device__ __forceinline__ uint32_t compress_lane(uint32_t l, uint32_t r, int lane, const LaneConsts& kc) {
  const uint32_t rs = dpp<DPP_ROR8>(r);  // lanes 8..15 <- r[0..7]
  return poseidon2_permute_lane(lane < 8 ? l : rs, lane, kc);
}
// One level of a path: the node joins its sibling on the side the index's low bit names.
__device__ __forceinline__ uint32_t path_step_lane(uint32_t node, const uint32_t* __restrict__ sib8,
                                                   bool right, int lane, const LaneConsts& kc) {
  const uint32_t sib = sib8[lane & 7];
  const uint32_t ns = dpp<DPP_ROR8>(node);
  const uint32_t lo = right ? sib : node, hi = right ? ns : sib;
  return poseidon2_permute_lane(lane < 8 ? lo : hi, lane, kc);
}

__global__ __launch_bounds__(256) void k_verify_inputs(uint32_t* __restrict__ B, uint32_t np) {
  const uint32_t proof = blockIdx.y;
  const VProof* __restrict__ D = reinterpret_cast<const VProof*>(B + np + 64) + proof;
  const uint32_t job = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const int lane = threadIdx.x & 15;
  const uint32_t nr = D->nrounds;  // 4 (machine proof) or 2 (BFU1); 0 in an empty slot
  if (job >= D->nq * nr) return;
  const uint32_t q = job / nr, rr = job - q * nr;
  const LaneConsts kc = lane_consts(lane);
  const VRoundD* __restrict__ R = &D->rd[rr];
  const uint32_t* __restrict__ rec = B + D->qbase + (size_t)q * D->qstride;
  const uint32_t* __restrict__ rows = rec + R->rows_off;
  const uint32_t* __restrict__ path = rec + R->path_off;
  const uint32_t lb = R->lb, ng = R->ngroups;
  uint32_t idx = B[D->idx_off + q] >> (D->log_max - lb);
  uint32_t node = sponge_lane(rows, R->g_w[0], lane, kc);
  uint32_t at = R->g_w[0], g = 1, cur = lb;
  for (uint32_t L = 0; L < lb; L++) {
    node = path_step_lane(node, path + 8 * L, idx & 1, lane, kc);
    idx >>= 1;
    cur--;
    if (g < ng && R->g_lh[g] == cur) {  // shorter matrices join here: compress(node, their hash)
      const uint32_t w = R->g_w[g];
      const uint32_t hh = sponge_lane(rows + at, w, lane, kc);
      node = compress_lane(node, hh, lane, kc);
      at += w;
      g++;
    }
  }
  if (g != ng || (lane < 8 && node != R->root[lane])) report(B, proof, q, rr);
}

__global__ __launch_bounds__(256) void k_verify_fri_paths(uint32_t* __restrict__ B, uint32_t np,
                                                          const uint32_t* __restrict__ leaves) {
  const uint32_t proof = blockIdx.y;
  const VProof* __restrict__ D = reinterpret_cast<const VProof*>(B + np + 64) + proof;
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

// One thread per query.  ro[lh] = sum over the (matrix, point, column)s of LDE height 2^lh of
// alpha^k (row[c] - v[c]) / (x - z) = sum over the two points of
// (sum_m alpha^k0(m) S_m - A) / (x - z), S_m = sum_c alpha^c row_m[c]; A (the opened values' part)
// and alpha^k0 come from the host.  The openings are kept in global memory by log height (a
// private array indexed by a run-time height would live in scratch).
__global__ __launch_bounds__(64) void k_verify_fold(uint32_t* __restrict__ B, uint32_t np,
                                                    uint32_t* __restrict__ leaves,
                                                    uint32_t* __restrict__ rows_ro) {
  const uint32_t proof = blockIdx.y;
  const VProof* __restrict__ D = reinterpret_cast<const VProof*>(B + np + 64) + proof;
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= D->nq) return;
  const uint32_t* __restrict__ gen = B + np;
  const uint32_t* __restrict__ gen_inv = B + np + 32;
  const uint32_t* __restrict__ rec = B + D->qbase + (size_t)q * D->qstride;
  const uint32_t* __restrict__ apow = B + D->apow_off;
  uint32_t* __restrict__ ro = rows_ro + D->ro_base + (size_t)q * (VQ_RO_SLOTS * 4);
  const uint32_t index = B[D->idx_off + q];
  const uint32_t log_max = D->log_max, nc = D->ncommit;
  for (int i = 0; i < VQ_RO_SLOTS * 4; i++) ro[i] = 0;
  const uint32_t three = to_mont_c(3);
  for (uint32_t j = 0; j < D->nheights; j++) {
    const VHeightD* __restrict__ H = &D->hs[j];
    EF acc0 = ef_zero(), acc1 = ef_zero();
    for (uint32_t m = H->m0; m < H->m1; m++) {
      const VMatD* __restrict__ M = &D->mats[m];
      const uint32_t* __restrict__ row = rec + M->off;
      LazyEF s;
      s.init();
      for (uint32_t c = 0; c < M->w; c++) s.add(ld_ef(apow + 4 * c), row[c]);
      const EF S = s.get();
      acc0 = ef_add(acc0, ef_mul(M->c0, S));
      if (M->np == 2) acc1 = ef_add(acc1, ef_mul(M->c1, S));
    }
    const uint32_t lh = H->lh;
    const uint32_t x = mmul(three, mpow(gen[lh], dbitrev(index >> (log_max - lh), (int)lh)));
    EF r = ef_mul(ef_sub(acc0, H->a0), ef_inv(ef_sub(ef_base(x), H->z0)));
    // (a height opened at one point only has acc1 = a1 = 0)
    r = ef_add(r, ef_mul(ef_sub(acc1, H->a1), ef_inv(ef_sub(ef_base(x), H->z1))));
    ro[4 * lh + 0] = r.c[0];
    ro[4 * lh + 1] = r.c[1];
    ro[4 * lh + 2] = r.c[2];
    ro[4 * lh + 3] = r.c[3];
  }
  // verify_query: fold with the sibling and beta_s, add the next height's reduced opening
  const uint32_t neg_half = mneg(to_mont_c((P + 1) / 2));
  EF folded = ef_zero();
  uint32_t idx = index;
  const uint32_t* __restrict__ step = rec + D->steps_off;
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

}  // namespace

void verify_queries_device(const QueryBatch& b, uint32_t* keys, hipStream_t st) {
  if (b.nproofs == 0 || b.max_nq == 0) return;
  if (b.nproofs > 65535) throw std::runtime_error("verify: too many proofs in one device pass");
  DBuf<uint32_t> d(b.words.size()), leaves(std::max<size_t>(b.leaf_words, 1)),
      ro(std::max<size_t>(b.ro_words, 1));
  upload_bulk(d.p, b.words.data(), b.words.size() * 4, st);
  const uint32_t np = b.nproofs;
  hipLaunchKernelGGL(k_verify_fold, dim3(ceil_div(b.max_nq, 64), np), dim3(64), 0, st, d.p, np,
                     leaves.p, ro.p);
  KCHECK();
  if (b.max_ncommit) {
    hipLaunchKernelGGL(k_verify_fri_paths, dim3(ceil_div((size_t)b.max_nq * b.max_ncommit * 16, 256), np),
                       dim3(256), 0, st, d.p, np, leaves.p);
    KCHECK();
  }
  hipLaunchKernelGGL(k_verify_inputs, dim3(ceil_div((size_t)b.max_nq * b.max_nrounds * 16, 256), np),
                     dim3(256), 0, st, d.p, np);
  KCHECK();
  HIP_CHECK(hipMemcpyAsync(keys, d.p, (size_t)np * 4, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace bfz
