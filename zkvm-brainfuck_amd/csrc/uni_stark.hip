// Per-chip uni-STARK prover (see uni_stark.h): p3_uni_stark::prove [p3-recalled] as
// utils::uni_stark_prove calls it (crates/core/machine/src/utils/prove.rs:97-127), on the
// default lane, from the machine prover's building blocks:
//   trace commit        commit_lde + Round::commit            (Pcs::commit, one matrix on H_n)
//   transcript head     observe F(log n), the trace commitment, no public values
//                       (utils/prove.rs:111), alpha = sample_ext_element          (U1, U2)
//   quotient            k_quotient_air on 3 H_(n 2^lqd), chunks committed as one round  (U3, U4)
//   PCS open            [trace: (zeta, zeta w_n)], [chunk j: (zeta)] with open_batch,
//                       reduce_prep / reduce_range, the FRI commit phase, the grind and the query
//                       openings exactly as open_impl's single-GPU path (D1-D11)        (U5)
//   proof               the BFU1 normal form                             (U6)
// Every matrix here has the same LDE height 2n, so there is one reduced opening and it is the
// first FRI layer.
#include "uni_stark.h"

#include <cstdlib>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>

#include "fri.h"
#include "ntt.h"
#include "quotient.h"

namespace bfz {

using namespace kb;

bool uni_observe_degree_from_env() {
  const char* s = std::getenv("BFZ_UNI_OBSERVE_DEGREE");
  if (!s) return true;
  if (!std::strcmp(s, "1")) return true;
  if (!std::strcmp(s, "0")) return false;
  throw std::runtime_error(std::string("BFZ_UNI_OBSERVE_DEGREE must be 0 or 1, not '") + s + "'");
}

void uni_air_shape_or_throw(int chip, int* K, int* degree, int* lqd) {
  if (chip < 0 || chip >= NUM_CHIPS) throw std::runtime_error("uni_stark: bad chip index");
  if (!uni_air_shape(chip, K, degree, lqd))
    throw std::runtime_error(std::string("uni_stark: chip ") + CHIP_INFO[chip].name +
                             " has no AIR constraints of its own or needs a preprocessed trace, "
                             "which p3_uni_stark does not take");
}

namespace {
constexpr int LOG_BLOWUP = 1, POW_BITS = 16;

struct StageClock {  // stage times of a timed call: events on the prover stream
  bool on;
  hipStream_t st;
  std::vector<std::pair<hipEvent_t, double*>> marks;
  hipEvent_t first = nullptr;
  StageClock(bool on_, hipStream_t s) : on(on_), st(s) {
    if (!on) return;
    HIP_CHECK(hipEventCreate(&first));
    HIP_CHECK(hipEventRecord(first, st));
  }
  void stage(double* into) {  // the time since the previous mark goes to *into
    if (!on) return;
    hipEvent_t e;
    HIP_CHECK(hipEventCreate(&e));
    HIP_CHECK(hipEventRecord(e, st));
    marks.push_back({e, into});
  }
  void collect(double* total) {
    if (!on) return;
    hipEvent_t prev = first;
    for (auto& m : marks) {
      HIP_CHECK(hipEventSynchronize(m.first));
      float ms = 0;
      HIP_CHECK(hipEventElapsedTime(&ms, prev, m.first));
      *m.second += ms;
      *total += ms;
      prev = m.first;
    }
  }
  ~StageClock() {
    if (first) (void)hipEventDestroy(first);
    for (auto& m : marks) (void)hipEventDestroy(m.first);
  }
};

struct Rewind {  // the pinned upload arena is rewound when the call is done (as ProofScope)
  hipStream_t st;
  ~Rewind() {
    (void)hipStreamSynchronize(st);
    staging_reset();
  }
};

std::vector<uint8_t> prove_core(const UniAir& air, const uint32_t* evals, size_t n,
                                Challenger& ch_io, const UniOptions& opt, StageTimes* tms,
                                StageClock& clock);
}  // namespace

UniAir uni_air_of_chip(int chip) {
  UniAir a;
  uni_air_shape_or_throw(chip, &a.num_constraints, &a.degree, &a.log_quotient_degree);
  a.chip = chip;
  a.width = CHIP_INFO[chip].main_w;
  a.name = CHIP_INFO[chip].name;
  return a;
}

UniAir uni_air_of_program(const AirProgram& p) {
  UniAir a;
  a.prog = &p;
  a.num_constraints = p.num_constraints;
  a.degree = p.degree;
  a.log_quotient_degree = p.log_quotient_degree;
  a.width = p.width;
  return a;
}

void uni_dims_or_throw(const UniAir& air, size_t height, size_t width) {
  if (air.log_quotient_degree > 1)
    throw std::runtime_error("uni_stark: constraint degree above 3 is not supported");
  if ((size_t)air.width != width)
    throw std::runtime_error(std::string("uni_stark: width mismatch for ") + air.name);
  if (height < 1 || (height & (height - 1)) || height > ((size_t)1 << 23))
    throw std::runtime_error(std::string("uni_stark: height not a power of two in [1, 2^23] for ") +
                             air.name);
}

void uni_dims_or_throw(int chip, size_t height, size_t width) {
  uni_dims_or_throw(uni_air_of_chip(chip), height, width);
}

void uni_noncanonical_throw(const char* name) {
  throw std::runtime_error(std::string("uni_stark: non-canonical field word (>= p) in ") + name);
}

DBuf<uint32_t> uni_upload_trace(size_t w, const char* name, const uint32_t* trace, size_t n,
                                hipStream_t st) {
  DBuf<uint32_t> evals(n * w), rm(n * w);
  upload_bulk(rm.p, trace, n * w * 4, st);
  // KoalaBear words are Montgomery residues < p; a larger word breaks mmul's b < p bound
  if (count_noncanonical(rm.p, n * w, st)) uni_noncanonical_throw(name);
  transpose_bitrev(rm.p, n, w, evals.p, st);
  return evals;
}

// The host-trace front: checks, upload, transpose (all inside the main_commit stage time).
std::vector<uint8_t> uni_prove(int chip, const uint32_t* trace, size_t height, size_t width,
                               Challenger& ch, const UniOptions& opt, StageTimes* times) {
  if (api_lock_depth() == 0) throw std::logic_error("uni_prove called outside the bfz API lock");
  if (!trace) throw std::runtime_error("uni_stark: null trace");
  return uni_prove(uni_air_of_chip(chip), trace, height, width, ch, opt, times);
}

std::vector<uint8_t> uni_prove(const UniAir& air, const uint32_t* trace, size_t height, size_t width,
                               Challenger& ch, const UniOptions& opt, StageTimes* times) {
  if (api_lock_depth() == 0) throw std::logic_error("uni_prove called outside the bfz API lock");
  if (!trace) throw std::runtime_error("uni_stark: null trace");
  uni_dims_or_throw(air, height, width);
  if (opt.num_queries < 1 || opt.num_queries > 4096) throw std::runtime_error("uni_stark: bad query count");
  hipStream_t st = stream();
  Rewind rewind{st};
  StageTimes local;
  StageClock clock(times != nullptr, st);
  const DBuf<uint32_t> evals = uni_upload_trace(width, air.name, trace, height, st);
  return prove_core(air, evals.p, height, ch, opt, times ? times : &local, clock);
}

// The device front: the evaluations are where they are, nothing is uploaded, transposed or copied.
std::vector<uint8_t> uni_prove_evals(int chip, const uint32_t* evals, size_t n, Challenger& ch,
                                     const UniOptions& opt, StageTimes* times) {
  if (api_lock_depth() == 0) throw std::logic_error("uni_prove called outside the bfz API lock");
  if (!evals) throw std::runtime_error("uni_stark: null trace");
  const UniAir air = uni_air_of_chip(chip);
  uni_dims_or_throw(air, n, (size_t)air.width);
  if (opt.num_queries < 1 || opt.num_queries > 4096) throw std::runtime_error("uni_stark: bad query count");
  hipStream_t st = stream();
  Rewind rewind{st};
  StageTimes local;
  StageClock clock(times != nullptr, st);
  return prove_core(air, evals, n, ch, opt, times ? times : &local, clock);
}

namespace {
// The prover from device evaluations (evals, n) in the library layout (column-major,
// bit-reversed): everything after the fronts.  The inputs have been checked.
std::vector<uint8_t> prove_core(const UniAir& air, const uint32_t* evals, size_t n,
                                Challenger& ch_io, const UniOptions& opt, StageTimes* tms,
                                StageClock& clock) {
  const int K = air.num_constraints, lqd = air.log_quotient_degree, w = air.width;
  const int logn = log2i(n), Lmax = logn + LOG_BLOWUP;
  const size_t N = 2 * n;
  const int nchunks = 1 << lqd;
  hipStream_t st = stream();
  Challenger ch = ch_io;

  // ---- trace commit (Pcs::commit of one matrix on H_n)
  Round tracer;
  tracer.mats.resize(1);
  commit_lde(tracer.mats[0], evals, n, w, ONE, st);
  tracer.commit(st, /*fetch_root=*/true);
  clock.stage(&tms->main_commit);

  // ---- transcript head (p3_uni_stark::prove): U1, U2
  if (opt.observe_degree) ch.observe(to_mont((uint32_t)logn));
  ch.observe_digest(tracer.tree.root);
  const EF alpha = ch.sample_ef();

  // ---- quotient values on 3 H_(n 2^lqd), chunk j written into its half of chunk j's LDE
  const uint32_t three = to_mont(3);
  std::vector<EF> apows((size_t)K);  // alpha^(K-1-k): the Horner fold as a sum (quotient.hip)
  {
    EF p = ef_one();
    for (int k = K - 1; k >= 0; k--) {
      apows[k] = p;
      p = ef_mul(p, alpha);
    }
  }
  DBuf<EF> apows_d((size_t)K);
  upload_async(apows_d.p, apows.data(), (size_t)K * sizeof(EF), st);
  QuotParams qp{};
  qp.alpha_pows = apows_d.p;
  {
    const uint32_t sn = mpow(three, n);
    qp.zh_even = msub(sn, ONE);
    qp.zh_odd = msub(mneg(sn), ONE);
    qp.zh_even_inv = minv(qp.zh_even);
    qp.zh_odd_inv = minv(qp.zh_odd);
    qp.wn_inv = minv(two_adic_gen(logn));
    qp.shift = three;
  }
  DBuf<QuotParams> qp_d(1);
  upload_async(qp_d.p, &qp, sizeof(qp), st);
  Round quotr;
  quotr.mats.resize(nchunks);
  const uint32_t wq = two_adic_gen(logn + lqd);  // split_domains: chunk j on 3 wq^j H_n
  for (int j = 0; j < nchunks; j++) {
    CMat& qm = quotr.mats[j];
    qm.n = n;
    qm.log_n = logn;
    qm.shift = mmul(three, j ? wq : ONE);
    qm.lde.height = N;
    qm.lde.width = 4;
    qm.lde.buf.reset(4 * N);
    qm.sharded = false;
    qm.blk = N;
    qm.row0 = 0;
    for (int c = 0; c < 64; c++) qm.nmap[c] = (uint8_t)c;
  }
  {
    QuotOut qo{};
    qo.chunk[0] = quotr.mats[0].lde.buf.p;
    qo.chunk[1] = nchunks > 1 ? quotr.mats[1].lde.buf.p + n : nullptr;
    qo.stride = N;
    if (air.prog) {  // the instruction list, uploaded once per call on the proof's stream
      const std::vector<uint32_t>& code = air.prog->code;
      DBuf<uint32_t> code_d(code.size());  // (stream-ordered: freed after the launch is fine)
      upload_async(code_d.p, code.data(), code.size() * 4, st);
      quotient_prog(code_d.p, (int)code.size(), lqd, tracer.mats[0].lde.buf.p, Lmax, qp, qp_d.p, qo, st);
    } else {
      quotient_air(air.chip, lqd, tracer.mats[0].lde.buf.p, Lmax, qp, qp_d.p, qo, st);
    }
  }
  for (int j = 0; j < nchunks; j++) {  // the other half of each chunk's LDE on 3 H_2n
    CMat& qm = quotr.mats[j];
    const uint32_t lde_shift = mmul(three, minv(qm.shift));  // GENERATOR / shift
    coset_lde_ex(qm.lde.buf.p + (size_t)j * n, N, n, 4, lde_shift, qm.lde.buf.p, 1 - j, st);
  }
  quotr.commit(st, /*fetch_root=*/true);
  clock.stage(&tms->quotient);
  ch.observe_digest(quotr.tree.root);
  const EF zeta = ch.sample_ef();

  // ---- PCS open: opened values at zeta (and zeta w_n for the trace)
  const Round* rounds[2] = {&tracer, &quotr};
  struct MatPts {
    int npts;
    size_t off[2];
  };
  std::vector<MatPts> mp[2];
  size_t nvals = 0;
  for (int r = 0; r < 2; r++)
    for (const CMat& m : rounds[r]->mats) {
      MatPts p{};
      p.npts = r == 0 ? 2 : 1;
      for (int j = 0; j < p.npts; j++) {
        p.off[j] = nvals;
        nvals += m.lde.width;
      }
      mp[r].push_back(p);
    }
  DBuf<EF> zeta_d(1);
  upload_async(zeta_d.p, &zeta, sizeof(EF), st);
  DBuf<EF> invd_zeta((size_t)1 << Lmax), w_zeta((size_t)1 << (Lmax - 1));
  inv_denoms_dev(zeta_d.p, Lmax, invd_zeta.p, st, w_zeta.p);
  DBuf<EF> opened_d(nvals);
  std::vector<OpenDesc> open1, open2;
  for (int r = 0; r < 2; r++)
    for (size_t i = 0; i < rounds[r]->mats.size(); i++) {
      const CMat& m = rounds[r]->mats[i];
      const bool two = mp[r][i].npts == 2;
      const uint32_t three_n = mpow(three, m.n);
      const uint32_t n_f = to_mont((uint32_t)(m.n % P));
      OpenDesc o{};
      o.mat = m.lde.buf.p;
      o.height = m.lde.height;
      o.w = m.lde.width;
      o.logH = Lmax;
      o.invd_a = invd_zeta.p;
      o.invd_b = two ? nullptr : o.invd_a;  // nullptr: derived from the zeta table
      o.wtab = w_zeta.p;
      o.zeta = zeta_d.p;  // the scales are computed by the final launch from the device's zeta
      o.zlog = m.log_n;
      o.z3n = three_n;
      o.zc = minv(mmul(three_n, n_f));
      o.zb = ONE;
      o.out_a = opened_d.p + mp[r][i].off[0];
      o.out_b = two ? opened_d.p + mp[r][i].off[1] : o.out_a;
      (two ? open2 : open1).push_back(o);
    }
  open_batch(open2, 2, st);
  open_batch(open1, 1, st);
  std::vector<EF> opened(nvals);
  HIP_CHECK(hipMemcpyAsync(opened.data(), opened_d.p, nvals * sizeof(EF), hipMemcpyDeviceToHost, st));

  // reduced-opening descriptors of the one LDE height (open_impl's order: round, matrix, point a's
  // columns then point b's)
  std::vector<RedCol> red_cols;
  std::vector<RedMat> red_mats;
  std::vector<RedColPrep> col_prep;
  std::vector<RedMatPrep> mat_prep;
  {
    uint32_t e = 0;
    for (int r = 0; r < 2; r++)
      for (size_t i = 0; i < rounds[r]->mats.size(); i++) {
        const CMat& m = rounds[r]->mats[i];
        const int mw = m.lde.width;
        const bool two = mp[r][i].npts == 2;
        RedMat rm{};
        rm.first = (int)red_cols.size();
        rm.count = mw;
        rm.has_b = two ? 1 : 0;
        for (int c = 0; c < mw; c++) {
          RedCol rc{};
          rc.col = m.rows() + (size_t)c * m.stride();
          red_cols.push_back(rc);
          col_prep.push_back({e + (uint32_t)c, (uint32_t)(mp[r][i].off[0] + c),
                              two ? (uint32_t)(mp[r][i].off[1] + c) : 0xffffffffu, (uint32_t)mw});
        }
        // the second point's denominators come from the zeta table times w_n^-1 (reduce_range)
        mat_prep.push_back({(uint32_t)mw, two ? minv(two_adic_gen(m.log_n)) : ONE});
        red_mats.push_back(rm);
        e += (uint32_t)(mp[r][i].npts * mw);
      }
  }
  RedJobPrep jp{};
  jp.col0 = 0;
  jp.ncols = (uint32_t)red_cols.size();
  jp.mat0 = 0;
  jp.nmats = (uint32_t)red_mats.size();
  jp.yb_fold = minv(two_adic_gen(logn));
  DBuf<RedCol> red_cols_d(red_cols.size());
  DBuf<RedMat> red_mats_d(red_mats.size());
  DBuf<RedColPrep> col_prep_d(col_prep.size());
  DBuf<RedMatPrep> mat_prep_d(mat_prep.size());
  DBuf<RedJobPrep> job_prep_d(1);
  upload_async(red_cols_d.p, red_cols.data(), red_cols.size() * sizeof(RedCol), st);
  upload_async(red_mats_d.p, red_mats.data(), red_mats.size() * sizeof(RedMat), st);
  upload_async(col_prep_d.p, col_prep.data(), col_prep.size() * sizeof(RedColPrep), st);
  upload_async(mat_prep_d.p, mat_prep.data(), mat_prep.size() * sizeof(RedMatPrep), st);
  upload_async(job_prep_d.p, &jp, sizeof(jp), st);

  spin_sync(st);  // the opened values are on the host
  if (opt.observe_openings)  // decision D1
    for (const EF& v : opened) ch.observe_ef(v);
  const EF fri_alpha = ch.sample_ef();

  DBuf<EF> alpha_yab(3);  // alpha, then {ya, yb}
  upload_async(alpha_yab.p, &fri_alpha, sizeof(EF), st);
  reduce_prep(red_cols_d.p, col_prep_d.p, red_mats_d.p, mat_prep_d.p, job_prep_d.p, 1, opened_d.p,
              alpha_yab.p, alpha_yab.p + 1, st);
  struct FriLayer {
    DBuf<EF> v;
  };
  std::vector<FriLayer> layers;
  {
    DBuf<EF> r(N);
    reduce_range(red_cols_d.p, red_mats_d.p, (int)red_mats.size(), N, 0, N, invd_zeta.p, nullptr,
                 alpha_yab.p + 1, true, r.p, st, (int)red_cols.size());
    layers.push_back({std::move(r)});
  }
  clock.stage(&tms->open);

  // ---- FRI commit phase (fri::prover::commit_phase), transcript steps on the device
  std::vector<MerkleTree> trees;
  if (ch.nin != 0) throw std::runtime_error("FRI: unexpected pending challenger input");
  DBuf<uint32_t> dstate(16);
  upload_async(dstate.p, ch.st, 64, st);
  const int nrounds = Lmax - LOG_BLOWUP;
  DBuf<EF> betas(std::max(nrounds, 1));
  DBuf<uint32_t> tail_trees;
  DBuf<EF> tail_layers;
  struct PendingFold {
    const EF* in = nullptr;
    const EF* beta = nullptr;
    size_t n = 0;
  } pend;
  size_t len = N;
  for (int rd = 0; len > ((size_t)1 << LOG_BLOWUP); rd++) {
    const size_t h = len / 2;
    FriLayer& cur = layers.back();
    if (h <= (size_t)FRI_TAIL_MAXH) {  // every remaining round in one launch
      if (pend.in) {
        fri_fold_range(pend.in, cur.v.p, pend.n, 0, pend.n, pend.beta, nullptr, st);
        pend = PendingFold{};
      }
      FriTailRounds a;
      a.logh0 = log2i(h);
      a.nr = log2i(len) - LOG_BLOWUP;
      a.in = cur.v.p;
      a.state = dstate.p;
      a.beta = betas.p + rd;
      size_t nw = 0, nv = 0;
      for (int r = 0; r < a.nr; r++) {
        nw += 8 * ((h >> r) * 2 - 1);
        nv += h >> r;
      }
      tail_trees.reset(nw);
      tail_layers.reset(nv);
      nw = nv = 0;
      for (int r = 0; r < a.nr; r++) {
        const size_t hr = h >> r;
        const EF* rows = r ? tail_layers.p + nv - 2 * hr : cur.v.p;
        trees.emplace_back();
        MerkleTree& t = trees.back();
        t.mats = {MatRef{(const uint32_t*)rows, hr, 8}};
        t.layers.resize(log2i(hr) + 1);
        a.tree[r] = tail_trees.p + nw;
        for (size_t L = 0; L < t.layers.size(); L++) {
          t.layers[L] = DBuf<uint32_t>::borrow(tail_trees.p + nw, 8 * (hr >> L));
          nw += 8 * (hr >> L);
        }
        a.layer[r] = tail_layers.p + nv;
        a.add[r] = nullptr;
        layers.push_back({DBuf<EF>::borrow(tail_layers.p + nv, hr)});
        nv += hr;
      }
      fri_tail_rounds(a, st);
      len = h >> (a.nr - 1);
      break;
    }
    trees.emplace_back();
    MerkleTree& t = trees.back();
    std::function<void(size_t, size_t, uint32_t*)> fused;
    if (pend.in) {  // this round's layer is the pending fold's output: fold + hash in one pass
      const PendingFold pf = pend;
      EF* out = cur.v.p;
      fused = [pf, out, h, st](size_t, size_t, uint32_t* dig) {
        fri_fold_leaves(pf.in, out, h, pf.beta, nullptr, dig, st);
      };
      pend = PendingFold{};
    }
    merkle_from_rows8(t, (const uint32_t*)cur.v.p, h, st, /*fetch_root=*/false,
                      RootChallenge{dstate.p, betas.p + rd}, /*allow_shard=*/false, fused);
    DBuf<EF> next(h);
    if (h / 2 >= FRI_FUSE_MIN) pend = PendingFold{cur.v.p, betas.p + rd, h};
    else fri_fold_range(cur.v.p, next.p, h, 0, h, betas.p + rd, nullptr, st);
    layers.push_back({std::move(next)});
    len = h;
  }
  if (pend.in) fri_fold_range(pend.in, layers.back().v.p, pend.n, 0, pend.n, pend.beta, nullptr, st);
  const int nt = (int)trees.size();
  if (nt > MAX_FRI_ROUNDS) throw std::runtime_error("FRI: too many rounds");
  const int nq = opt.num_queries;

  // ---- query openings in serialized form (BFZ1's query encoding, two input rounds)
  std::vector<GatherSeg> segs;
  auto lit = [&](uint32_t v) { segs.push_back({nullptr, 0, 0, v, 0, 1, -1, 0}); };
  lit(2);
  for (int r = 0; r < 2; r++) {
    const Round& R = *rounds[r];
    const int lrm = (int)R.tree.layers.size() - 1;
    lit((uint32_t)R.mats.size());
    for (const CMat& m : R.mats) {
      lit((uint32_t)m.lde.width);
      segs.push_back({m.rows(), (uint64_t)m.stride(), 0, 0, 1, (uint32_t)m.lde.width, -1, 0});
    }
    lit((uint32_t)lrm);
    for (int L = 0; L < lrm; L++)  // sibling digest at layer L
      segs.push_back({R.tree.layers[L].p, 1, (uint32_t)(Lmax - lrm + L), 1, 8, 8, -1, 0});
  }
  lit((uint32_t)nt);
  for (int i = 0; i < nt; i++) {
    segs.push_back({(const uint32_t*)layers[i].v.p, 1, (uint32_t)i, 1, 4, 4, -1, 0});  // sibling EF
    const int lm = (int)trees[i].layers.size() - 1;
    lit((uint32_t)lm);
    for (int L = 0; L < lm; L++)
      segs.push_back({trees[i].layers[L].p, 1, (uint32_t)(i + 1 + L), 1, 8, 8, -1, 0});
  }
  const size_t nwords = query_words(segs) * (size_t)nq;

  // tail = [roots (8 MAX_FRI_ROUNDS) | FRI state (16) | final layer (8) | challenger | witness,
  //         ok | qidx (nq) | query words], as open_impl
  constexpr size_t T_CH = 8 * MAX_FRI_ROUNDS + 16 + 8;
  constexpr size_t T_RES = T_CH + sizeof(DevChallenger) / 4;
  constexpr size_t T_Q = T_RES + 2;
  const size_t T_W = T_Q + (size_t)nq, tail_n = T_W + nwords;
  DBuf<uint32_t> tailbuf(tail_n);
  DevChallenger* dch = reinterpret_cast<DevChallenger*>(tailbuf.p + T_CH);
  if (!nt) {  // no commit-phase round (a 1-row trace): the host challenger as it stands
    DevChallenger hc;
    std::memcpy(hc.st, ch.st, 64);
    std::memcpy(hc.in, ch.in, 32);
    std::memcpy(hc.out, ch.out, 32);
    hc.nin = ch.nin;
    hc.nout = ch.nout;
    upload_async(dch, &hc, sizeof(hc), st);
  }
  FriTail tail{};
  for (int i = 0; i < nt; i++) tail.root[i] = trees[i].layers.back().p;
  tail.nroots = nt;
  tail.state = dstate.p;
  tail.fin = layers.back().v.p;
  pack_fri_tail(tail, tailbuf.p, st);
  fri_transcript_tail(dch, nt ? dstate.p : nullptr, layers.back().v.p, POW_BITS, nq, Lmax,
                      tailbuf.p + T_Q, tailbuf.p + T_RES, st);
  gather_queries(segs, tailbuf.p + T_Q, nq, tailbuf.p + T_W, nullptr, st);
  Lane& tl = lane();  // pinned: the tail of the proof (the lane's, as open_impl)
  if (tail_n > tl.tcap) {  // no copy into it is pending: every proof waits for its tail
    if (tl.tbox) HIP_CHECK(hipHostFree(tl.tbox));
    tl.tbox = nullptr;
    tl.tcap = 0;
    const size_t cap = std::max(tail_n + tail_n / 4, (size_t)1 << 18);
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&tl.tbox), cap * 4, hipHostMallocDefault));
    tl.tcap = cap;
  }
  uint32_t* tbox = tl.tbox;
  HIP_CHECK(hipMemcpyAsync(tbox, tailbuf.p, tail_n * 4, hipMemcpyDeviceToHost, st));
  spin_sync(st);
  std::vector<Digest> croots(nt);
  for (int i = 0; i < nt; i++) std::memcpy(croots[i].data(), &tbox[8 * i], 32);
  EF fin[2];
  std::memcpy(fin, &tbox[8 * MAX_FRI_ROUNDS + 16], sizeof(fin));
  // An invalid trace still proves: each chunk is interpolated from the quotient's values, so
  // every committed matrix is a low-degree polynomial whatever the trace holds, the final layer
  // is constant, and only the verifier's out-of-domain identity fails.
  if (!ef_eq(fin[0], fin[1])) throw std::runtime_error("FRI: final polynomial is not constant");
  const uint32_t witness = tbox[T_RES];
  if (tbox[T_RES + 1] != 1) throw std::runtime_error("grind: bad witness");
  {  // the host replays the device's FRI transcript and must arrive at the device's challenger
    for (int i = 0; i < nt; i++) {
      ch.observe_digest(croots[i].data());
      (void)ch.sample_ef();
    }
    ch.observe_ef(fin[0]);
    if (!ch.check_witness(POW_BITS, witness))
      throw std::runtime_error("device transcript diverged from the host challenger: PoW witness");
    for (int q = 0; q < nq; q++)
      if (ch.sample_bits(Lmax) != tbox[T_Q + q])
        throw std::runtime_error("device transcript diverged from the host challenger: query index");
    DevChallenger dc;
    std::memcpy(&dc, &tbox[T_CH], sizeof(dc));
    if (std::memcmp(ch.st, dc.st, 64) != 0 || ch.nin != (int)dc.nin || ch.nout != (int)dc.nout ||
        std::memcmp(ch.in, dc.in, 4 * (size_t)ch.nin) != 0 ||
        std::memcmp(ch.out, dc.out, 4 * (size_t)ch.nout) != 0)
      throw std::runtime_error("device transcript diverged from the host challenger: final state");
  }
  clock.stage(&tms->fri);
  clock.collect(&tms->total);

  // ---- serialize (BFU1 normal form, proof.cpp)
  UniProof u;
  u.chip = air.prog ? BFZ_AIR_CHIP : (uint32_t)air.chip;
  u.log_degree = (uint32_t)logn;
  std::memcpy(u.pcs.main_root.data(), tracer.tree.root, 32);
  std::memcpy(u.pcs.quot_root.data(), quotr.tree.root, 32);
  u.trace_local.assign(opened.begin() + mp[0][0].off[0], opened.begin() + mp[0][0].off[0] + w);
  u.trace_next.assign(opened.begin() + mp[0][0].off[1], opened.begin() + mp[0][0].off[1] + w);
  for (int j = 0; j < nchunks; j++)
    u.chunks.emplace_back(opened.begin() + mp[1][j].off[0], opened.begin() + mp[1][j].off[0] + 4);
  u.pcs.commit_roots = croots;
  u.pcs.final_poly = fin[0];
  u.pcs.pow_witness = to_mont(witness);
  std::vector<uint8_t> out = encode_bfu1(u, (uint32_t)nq, tbox + T_W, nwords);
  ch_io = ch;
  return out;
}
}  // namespace

}  // namespace bfz
