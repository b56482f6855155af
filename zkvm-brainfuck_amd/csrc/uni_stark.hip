// Per-chip uni-STARK prover (see uni_stark.h): p3_uni_stark::prove [p3-recalled] as
// utils::uni_stark_prove calls it (crates/core/machine/src/utils/prove.rs:97-127), on the
// default lane, from the machine prover's building blocks:
//   trace commit        commit_lde + Round::commit            (Pcs::commit, one matrix on H_n)
//   transcript head     observe F(log n), the trace commitment, no public values
//                       (utils/prove.rs:111), alpha = sample_ext_element          (U1, U2)
//   quotient            k_quotient_air on 3 H_(n 2^lqd), chunks committed as one round  (U3, U4)
//   PCS open            [trace: (zeta, zeta w_n)], [chunk j: (zeta)]: pcs_open (pcs_open.hip), the
//                       machine prover's opening, on the unsharded plan with the two rounds in
//                       one opening group (D1-D11)                                      (U5)
//   proof               the BFU1 normal form                             (U6)
// Every matrix here has the same LDE height 2n, so there is one reduced opening and it is the
// first FRI layer.
#include "uni_stark.h"

#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

#include "ntt.h"
#include "pcs_open.h"
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
// One prove call: the stage events of a timed call (the kernel probes are left alone, which is
// why this is not prover.hip's ProofScope) and, when the call is done, the rewind of the pinned
// upload arena.
struct CallScope {
  hipStream_t st;
  EvTimer ev;
  StageTimes local;
  StageTimes* tms;
  hipEvent_t e_total = nullptr, e_commit = nullptr;  // both begin before the trace is uploaded
  CallScope(StageTimes* times, hipStream_t s) : st(s), tms(times ? times : &local) {
    ev.on = times != nullptr;
    if (!ev.on) return;
    e_total = ev.begin(st);
    e_commit = ev.begin(st);
  }
  ~CallScope() {
    (void)hipStreamSynchronize(st);
    staging_reset();
  }
};

std::vector<uint8_t> prove_core(const UniAir& air, const uint32_t* evals, size_t n,
                                Challenger& ch_io, const UniOptions& opt, CallScope& sc);
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
  CallScope sc(times, st);
  const DBuf<uint32_t> evals = uni_upload_trace(width, air.name, trace, height, st);
  return prove_core(air, evals.p, height, ch, opt, sc);
}

// The device front: the evaluations are where they are, nothing is uploaded, transposed or copied.
std::vector<uint8_t> uni_prove_evals(int chip, const uint32_t* evals, size_t n, Challenger& ch,
                                     const UniOptions& opt, StageTimes* times) {
  if (api_lock_depth() == 0) throw std::logic_error("uni_prove called outside the bfz API lock");
  if (!evals) throw std::runtime_error("uni_stark: null trace");
  const UniAir air = uni_air_of_chip(chip);
  uni_dims_or_throw(air, n, (size_t)air.width);
  if (opt.num_queries < 1 || opt.num_queries > 4096) throw std::runtime_error("uni_stark: bad query count");
  CallScope sc(times, stream());
  return prove_core(air, evals, n, ch, opt, sc);
}

namespace {
// The prover from device evaluations (evals, n) in the library layout (column-major,
// bit-reversed): everything after the fronts.  The inputs have been checked.
std::vector<uint8_t> prove_core(const UniAir& air, const uint32_t* evals, size_t n,
                                Challenger& ch_io, const UniOptions& opt, CallScope& sc) {
  const int K = air.num_constraints, lqd = air.log_quotient_degree, w = air.width;
  const int logn = log2i(n), Lmax = logn + LOG_BLOWUP;
  const size_t N = 2 * n;
  const int nchunks = 1 << lqd;
  hipStream_t st = sc.st;
  EvTimer& ev = sc.ev;
  StageTimes* tms = sc.tms;
  Challenger ch = ch_io;

  // ---- trace commit (Pcs::commit of one matrix on H_n)
  Round tracer;
  tracer.mats.resize(1);
  commit_lde(tracer.mats[0], evals, n, w, ONE, st);
  tracer.commit(st, /*fetch_root=*/true);
  if (ev.on) ev.end(sc.e_commit, st, &tms->main_commit);
  hipEvent_t e_quot = ev.on ? ev.begin(st) : nullptr;

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
  const QuotParams qp = quot_params_of_height(n, apows_d.p);
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
  if (ev.on) ev.end(e_quot, st, &tms->quotient);
  ch.observe_digest(quotr.tree.root);
  const EF zeta = ch.sample_ef();

  // ---- PCS open (pcs_open.hip): the trace at (zeta, zeta w_n), each chunk at zeta, one group
  DBuf<EF> zeta_d(1);
  upload_async(zeta_d.p, &zeta, sizeof(EF), st);
  PcsOpenIn oin;
  oin.rounds = {{&tracer, 0, {1}}, {&quotr, 0, std::vector<uint8_t>((size_t)nchunks, 0)}};
  oin.zeta_d = zeta_d.p;  // (the unsharded plan reads zeta from the device alone)
  oin.observe_openings = opt.observe_openings;
  oin.num_queries = opt.num_queries;
  oin.ev = &ev;
  oin.tms = tms;
  const PcsOpenOut po = pcs_open(oin, ch);
  if (ev.on) {
    ev.end(sc.e_total, st, &tms->total);
    ev.collect();
  }
  const std::vector<EF>& opened = po.opened;
  const std::vector<std::vector<PcsOpenOut::MatPts>>& mp = po.mp;

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
  u.pcs.commit_roots = po.commit_roots;
  u.pcs.final_poly = po.final_poly;
  u.pcs.pow_witness = to_mont(po.pow_witness);
  std::vector<uint8_t> out = encode_bfu1(u, (uint32_t)opt.num_queries, po.words, po.nwords);
  ch_io = ch;
  return out;
}
}  // namespace

}  // namespace bfz
