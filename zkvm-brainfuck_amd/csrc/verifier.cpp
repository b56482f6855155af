// Host verifier (see verifier.h).  Checks, in the reference's order:
//   BfProver::verify           (crates/prover/src/verify.rs:10-36): Cpu present, log deg <= 22
//   Verifier::verify_shard     (crates/stark/src/verifier.rs:27-216): byte-multiplicity bound,
//                              transcript replay, PCS/FRI verification, per-chip OOD check
//                              folded(zeta) * 1/Z_H(zeta) == recomputed quotient(zeta),
//                              sum of cumulative sums == 0.
#include "verifier.h"
#include "host_p2.h"

#include <algorithm>
#include <array>
#include <cstring>
#include <map>
#include <stdexcept>
#include <vector>

#include "air.h"
#include "machine.h"
#include "poseidon2.h"
#include "prover.h"
#include "quotient.h"
#include "uni_stark.h"
#include "verify.h"

namespace bfz {

using namespace kb;

namespace {

constexpr int LOG_BLOWUP = 1, POW_BITS = 16, MAX_CPU_LOG_DEGREE = 22;

struct HornerAcc {
  EF acc = ef_zero();
  EF alpha;
  void emit(const EF& c) { acc = ef_add(ef_mul(acc, alpha), c); }
  void emit_ext(const EF& c) { emit(c); }
};

template <int CHIP>
EF fold_chip(const std::vector<EF>& pl, const std::vector<EF>& pn, const std::vector<EF>& ml,
             const std::vector<EF>& mn, const std::vector<EF>& perml, const std::vector<EF>& permn,
             const EF& pa, const EF* pb_pows, const EF& cumsum, const EF& first, const EF& last,
             const EF& trans, const EF& alpha) {
  HornerAcc acc;
  acc.alpha = alpha;
  static const EF zero1[1] = {ef_zero()};
  const EF* PL = pl.empty() ? zero1 : pl.data();
  const EF* PN = pn.empty() ? zero1 : pn.data();
  Air<ExtOps, HornerAcc> air{ml.data(), mn.data(), PL, PN, first, last, trans, acc};
  air.template eval_air<CHIP>();
  air.template eval_perm<CHIP>(perml.data(), permn.data(), pa, pb_pows, cumsum, first, last, trans);
  return acc.acc;
}

EF fold_any(int chip, const std::vector<EF>& pl, const std::vector<EF>& pn, const std::vector<EF>& ml,
            const std::vector<EF>& mn, const std::vector<EF>& perml, const std::vector<EF>& permn,
            const EF& pa, const EF* pb, const EF& cs, const EF& f, const EF& l, const EF& t,
            const EF& al) {
  switch (chip) {
    case CHIP_CPU: return fold_chip<CHIP_CPU>(pl, pn, ml, mn, perml, permn, pa, pb, cs, f, l, t, al);
    case CHIP_PROGRAM: return fold_chip<CHIP_PROGRAM>(pl, pn, ml, mn, perml, permn, pa, pb, cs, f, l, t, al);
    case CHIP_ADDSUB: return fold_chip<CHIP_ADDSUB>(pl, pn, ml, mn, perml, permn, pa, pb, cs, f, l, t, al);
    case CHIP_JUMP: return fold_chip<CHIP_JUMP>(pl, pn, ml, mn, perml, permn, pa, pb, cs, f, l, t, al);
    case CHIP_MEMORY: return fold_chip<CHIP_MEMORY>(pl, pn, ml, mn, perml, permn, pa, pb, cs, f, l, t, al);
    case CHIP_BYTE: return fold_chip<CHIP_BYTE>(pl, pn, ml, mn, perml, permn, pa, pb, cs, f, l, t, al);
    case CHIP_MEMINSTRS: return fold_chip<CHIP_MEMINSTRS>(pl, pn, ml, mn, perml, permn, pa, pb, cs, f, l, t, al);
    case CHIP_IO: return fold_chip<CHIP_IO>(pl, pn, ml, mn, perml, permn, pa, pb, cs, f, l, t, al);
  }
  throw std::runtime_error("bad chip");
}

void sponge(uint32_t st[16], const std::vector<const uint32_t*>& rows, const std::vector<int>& ws) {
  int pos = 0;
  for (size_t m = 0; m < rows.size(); m++)
    for (int c = 0; c < ws[m]; c++) {
      st[pos++] = rows[m][c];
      if (pos == 8) {
        host_permute(st);
        pos = 0;
      }
    }
  if (pos) host_permute(st);
}

void compress(const uint32_t* l, const uint32_t* r, uint32_t* out) {
  uint32_t s[16];
  std::memcpy(s, l, 32);
  std::memcpy(s + 8, r, 32);
  host_permute(s);
  std::memcpy(out, s, 32);
}

// MerkleTreeMmcs::verify_batch [p3-recalled]; heights are powers of two.
bool verify_batch(const uint32_t root[8], const std::vector<size_t>& heights,
                  const std::vector<int>& widths, size_t index,
                  const std::vector<std::vector<uint32_t>>& rows,
                  const std::vector<uint32_t>& path) {
  std::vector<int> ord(heights.size());
  for (size_t i = 0; i < ord.size(); i++) ord[i] = (int)i;
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return heights[a] > heights[b]; });
  size_t cur = heights[ord[0]];
  size_t k = 0;
  auto take = [&](std::vector<const uint32_t*>& rp, std::vector<int>& wp) {
    while (k < ord.size() && heights[ord[k]] == cur) {
      rp.push_back(rows[ord[k]].data());
      wp.push_back(widths[ord[k]]);
      k++;
    }
  };
  std::vector<const uint32_t*> rp;
  std::vector<int> wp;
  take(rp, wp);
  uint32_t h[16] = {0};
  sponge(h, rp, wp);
  uint32_t node[8];
  std::memcpy(node, h, 32);
  for (size_t L = 0; L < path.size() / 8; L++) {
    const uint32_t* sib = &path[8 * L];
    if (index & 1) compress(sib, node, node);
    else compress(node, sib, node);
    index >>= 1;
    cur >>= 1;
    if (k < ord.size() && heights[ord[k]] == cur) {
      rp.clear();
      wp.clear();
      take(rp, wp);
      uint32_t hh[16] = {0};
      sponge(hh, rp, wp);
      compress(node, hh, node);
    }
  }
  return k == ord.size() && std::memcmp(node, root, 32) == 0;
}

EF monomial(int e) {
  EF m = ef_zero();
  m.c[e] = ONE;
  return m;
}

EF zp_at(int log_n, uint32_t shift, const EF& x) {  // (x / s)^(2^log_n) - 1
  EF u = ef_mul_base(x, minv(shift));
  for (int i = 0; i < log_n; i++) u = ef_mul(u, u);
  return ef_sub(u, ef_one());
}

// number of byte lookups each chip SENDS (Chip::num_sent_byte_lookups)
int sent_byte_lookups(int chip) { return chip == CHIP_CPU ? 7 : chip == CHIP_ADDSUB ? 3 : 0; }

// verify_shard in three stages that share this state: before_queries (everything up to the query
// loop: shapes, transcript replay, PoW, the query indices), check_query (one turn of the query
// loop) and after_queries (the OOD and cumulative-sum checks).  Each throws the reason of the first
// check that fails.  The state refers into the proof, which must outlive it.
struct ChipOpen {
  int log_n;
  const std::vector<EF> &pl, &pn, &ml, &mn, &perml, &permn;
  const std::vector<EF>* q;
  EF cumsum;
};
struct VMat { int log_n; uint32_t shift; int w; int np; EF pt[2]; const std::vector<EF>* v[2]; };
struct ShardState {
  const ShardProof* pf = nullptr;
  std::vector<ChipOpen> co;
  EF pa, pb, alpha, zeta, fri_alpha, final_poly;
  std::vector<VMat> rounds[4];
  int nrounds = 4;  // input rounds in use: 4 in a machine proof, 2 in a per-chip uni-STARK proof
  const uint32_t* roots[4] = {};
  std::vector<EF> betas;
  uint32_t ncommit = 0, nq = 0;
  int log_max = 0;
  std::vector<size_t> index;  // the sampled index of every query
};

// The transcript of TwoAdicFriPcs::verify [p3-recalled] once S.rounds holds the opened values:
// the opened values (D1), the batching challenge, the commit-phase roots and their betas, the
// final value, the PoW check, the query indices.
void pcs_transcript(ShardState& S, Challenger& ch, bool observe_openings, int num_queries) {
  const ShardProof& pf = *S.pf;
  const std::vector<VMat>* rounds = S.rounds;
  if (observe_openings)  // decision D1: opened values enter the transcript
    for (int rr = 0; rr < S.nrounds; rr++)
      for (const VMat& m : rounds[rr])
        for (int p = 0; p < m.np; p++)
          for (int c = 0; c < m.w; c++) ch.observe_ef((*m.v[p])[c]);
  S.fri_alpha = ch.sample_ef();
  const uint32_t ncommit = S.ncommit = (uint32_t)pf.commit_roots.size();
  if (ncommit > 30) throw std::runtime_error("too many FRI rounds");
  const int log_max = S.log_max = (int)ncommit + LOG_BLOWUP;
  {  // the commit phase folds the tallest LDE down to 2^LOG_BLOWUP: every height must fit
    int lh_max = 0;
    for (int rr = 0; rr < S.nrounds; rr++)
      for (const VMat& m : rounds[rr]) lh_max = std::max(lh_max, m.log_n + LOG_BLOWUP);
    if (lh_max != log_max) throw std::runtime_error("FRI round count does not match the tallest matrix");
  }
  S.betas.resize(ncommit);
  for (uint32_t i = 0; i < ncommit; i++) {
    ch.observe_digest(pf.commit_roots[i].data());
    S.betas[i] = ch.sample_ef();
  }
  const uint32_t nq = S.nq = (uint32_t)pf.queries.size();
  if ((int)nq != num_queries) throw std::runtime_error("wrong number of queries");
  S.final_poly = pf.final_poly;
  ch.observe_ef(S.final_poly);
  if (!ch.check_witness(POW_BITS, from_mont(pf.pow_witness))) throw std::runtime_error("bad PoW witness");
  // nothing but the indices is drawn from the transcript from here on, and no check of the
  // query loop touches it: sampling them all first changes no outcome
  S.index.resize(nq);
  for (uint32_t q = 0; q < nq; q++) S.index[q] = ch.sample_bits(log_max);
}

void before_queries(const std::string& src, const uint32_t vk_commit[8], const ShardProof& pf,
                    const VerifyOptions& opt, ShardState& S) {
  S.pf = &pf;
  std::vector<ChipOpen>& co = S.co;
  std::vector<VMat>* rounds = S.rounds;
  {
    Program prog = Program::parse(src);
    // vk.chip_information: prep matrices sorted by (Reverse(height), name)
    size_t prog_h = std::max<size_t>(16, [&] {
      size_t p = 1;
      while (p < prog.instructions.size()) p <<= 1;
      return p;
    }());
    struct PrepInfo { int chip; int log_n; int w; };
    std::vector<PrepInfo> prep = {{CHIP_PROGRAM, log2i(prog_h), 6}, {CHIP_BYTE, 16, 2}};
    if (prep[1].log_n > prep[0].log_n ||
        (prep[1].log_n == prep[0].log_n && std::strcmp("Byte", "Program") < 0))
      std::swap(prep[0], prep[1]);

    const uint32_t nc = (uint32_t)pf.chips.size();
    if (nc == 0 || nc > NUM_CHIPS || pf.opened.size() != nc) throw std::runtime_error("bad chip count");
    const std::vector<int>& chip = pf.chips;
    {
      std::vector<bool> seen(NUM_CHIPS, false);
      for (int c : chip) {
        if (c < 0 || c >= NUM_CHIPS || seen[c]) throw std::runtime_error("bad chip id");
        seen[c] = true;
      }
    }
    const uint32_t* main_root = pf.main_root.data();
    const uint32_t* perm_root = pf.perm_root.data();
    const uint32_t* quot_root = pf.quot_root.data();
    co.reserve(nc);
    for (uint32_t i = 0; i < nc; i++) {
      const ChipOpened& o = pf.opened[i];
      // unsigned: a huge word must not become a negative shift count below
      // log degree 0 is a 1-row trace (the Cpu chip of a one-cycle program: cpu/trace.rs:33
      // pads to next_power_of_two with no minimum)
      if (o.log_degree > 23) throw std::runtime_error("log degree out of range");
      co.push_back(ChipOpen{(int)o.log_degree, o.prep_local, o.prep_next, o.main_local, o.main_next,
                            o.perm_local, o.perm_next, o.quotient, o.cumsum});
      const ChipOpen& c = co.back();
      const int ch = chip[i];
      const size_t pw = CHIP_INFO[ch].prep_w;
      if (c.ml.size() != (size_t)CHIP_INFO[ch].main_w || c.mn.size() != c.ml.size() ||
          c.perml.size() != 4 * (size_t)perm_width(ch) || c.permn.size() != c.perml.size() ||
          c.pl.size() != pw || c.pn.size() != pw || c.q[0].size() != 4 || c.q[1].size() != 4)
        throw std::runtime_error("opened-value shape mismatch");
      // A local-only chip's next values are not opened by the PCS (verifier.rs:109-135), so
      // the reference verifier would accept any words there; its prover writes zeros
      // (prover.rs:484-487, 499-502).  Requiring the zeros keeps accepted proofs
      // non-malleable (tests/test_abi.py fuzz) and rejects nothing an honest prover emits.
      if (CHIP_INFO[ch].local_only) {
        for (const std::vector<EF>* v : {&c.pn, &c.mn})
          for (const EF& e : *v)
            if (e.c[0] | e.c[1] | e.c[2] | e.c[3])
              throw std::runtime_error("local-only chip with non-zero next values");
      }
    }
    // BfProver::verify: Cpu chip present, log degree bound
    int cpu_i = -1;
    for (uint32_t i = 0; i < nc; i++) if (chip[i] == CHIP_CPU) cpu_i = (int)i;
    if (cpu_i < 0) throw std::runtime_error("missing Cpu chip");
    if (co[cpu_i].log_n > MAX_CPU_LOG_DEGREE) throw std::runtime_error("Cpu log degree too large");
    // byte multiplicities must not overflow (verifier.rs:47-62)
    {
      unsigned __int128 tot = 0;
      for (uint32_t i = 0; i < nc; i++) tot += (unsigned __int128)sent_byte_lookups(chip[i]) << co[i].log_n;
      if (tot > P) throw std::runtime_error("byte multiplicities overflow");
    }
    // ---- transcript (verifier.rs:76-101)
    Challenger ch;
    ch.observe_digest(vk_commit);
    for (int i = 0; i < 7; i++) ch.observe(0);
    ch.observe_digest(main_root);
    S.pa = ch.sample_ef();
    S.pb = ch.sample_ef();
    ch.observe_digest(perm_root);
    for (uint32_t i = 0; i < nc; i++) {
      ch.observe_ef(co[i].cumsum);
      // chips with no interactions must have a zero sum (all chips here have interactions)
    }
    S.alpha = ch.sample_ef();
    ch.observe_digest(quot_root);
    const EF zeta = S.zeta = ch.sample_ef();

    // ---- rounds for PCS verify
    for (const PrepInfo& pi : prep) {
      int idx = -1;
      for (uint32_t j = 0; j < nc; j++) if (chip[j] == pi.chip) idx = (int)j;
      if (idx < 0) throw std::runtime_error("preprocessed chip missing from proof");
      VMat m{pi.log_n, ONE, pi.w, CHIP_INFO[pi.chip].local_only ? 1 : 2, {zeta, ef_mul_base(zeta, two_adic_gen(pi.log_n))},
             {&co[idx].pl, &co[idx].pn}};
      rounds[0].push_back(m);
    }
    for (uint32_t i = 0; i < nc; i++) {
      const ChipOpen& c = co[i];
      const EF znext = ef_mul_base(zeta, two_adic_gen(c.log_n));
      rounds[1].push_back(VMat{c.log_n, ONE, (int)c.ml.size(), CHIP_INFO[chip[i]].local_only ? 1 : 2,
                               {zeta, znext}, {&c.ml, &c.mn}});
      rounds[2].push_back(VMat{c.log_n, ONE, (int)c.perml.size(), 2, {zeta, znext}, {&c.perml, &c.permn}});
      const uint32_t w2n = two_adic_gen(c.log_n + 1);
      for (int k = 0; k < 2; k++)
        rounds[3].push_back(VMat{c.log_n, mmul(to_mont(3), k ? w2n : ONE), 4, 1, {zeta, zeta},
                                 {&c.q[k], &c.q[k]}});
    }
    S.roots[0] = vk_commit;
    S.roots[1] = main_root;
    S.roots[2] = perm_root;
    S.roots[3] = quot_root;
    pcs_transcript(S, ch, opt.observe_openings, opt.num_queries);
  }
}

// One turn of the query loop: the four input openings with their reduced openings, then
// verify_query (the fold chain with one commit-phase opening per step).
void check_query(const ShardState& S, uint32_t q) {
  const ShardProof& pf = *S.pf;
  const std::vector<VMat>* rounds = S.rounds;
  const uint32_t* const* roots = S.roots;
  const EF fri_alpha = S.fri_alpha, final_poly = S.final_poly;
  const std::vector<EF>& betas = S.betas;
  const uint32_t ncommit = S.ncommit;
  const int log_max = S.log_max;
  {
    {
      const QueryProof& qp = pf.queries[q];
      const size_t index = S.index[q];
      if (qp.inputs.size() != (size_t)S.nrounds) throw std::runtime_error("bad round count");
      std::map<int, std::pair<EF, EF>> ro;  // log height -> (alpha_pow, ro)
      for (int rr = 0; rr < S.nrounds; rr++) {
        const BatchOpening& bo = qp.inputs[rr];
        const size_t nm = bo.rows.size();
        if (nm != rounds[rr].size()) throw std::runtime_error("bad matrix count");
        const std::vector<std::vector<uint32_t>>& rows = bo.rows;
        std::vector<size_t> heights(nm);
        std::vector<int> widths(nm);
        int lbmax = 0;
        for (size_t i = 0; i < nm; i++) {
          const size_t w = rows[i].size();
          if ((int)w != rounds[rr][i].w) throw std::runtime_error("bad row width");
          heights[i] = (size_t)1 << (rounds[rr][i].log_n + LOG_BLOWUP);
          widths[i] = (int)w;
          lbmax = std::max(lbmax, rounds[rr][i].log_n + LOG_BLOWUP);
        }
        if ((int)bo.path.size() != lbmax) throw std::runtime_error("bad path length");
        std::vector<uint32_t> path(8 * bo.path.size());
        for (size_t L = 0; L < bo.path.size(); L++) std::memcpy(&path[8 * L], bo.path[L].data(), 32);
        const size_t ridx = index >> (log_max - lbmax);
        if (!verify_batch(roots[rr], heights, widths, ridx, rows, path))
          throw std::runtime_error("input Merkle opening rejected");
        for (uint32_t i = 0; i < nm; i++) {
          const VMat& m = rounds[rr][i];
          const int lh = m.log_n + LOG_BLOWUP;
          const uint32_t rev = bitrev32((uint32_t)(index >> (log_max - lh)), lh);
          const uint32_t x = mmul(to_mont(3), mpow(two_adic_gen(lh), rev));
          auto it = ro.find(lh);
          if (it == ro.end()) it = ro.emplace(lh, std::make_pair(ef_one(), ef_zero())).first;
          for (int p = 0; p < m.np; p++) {
            const EF inv = ef_inv(ef_sub(ef_base(x), m.pt[p]));
            for (int c = 0; c < m.w; c++) {
              const EF quo = ef_mul(ef_sub(ef_base(rows[i][c]), (*m.v[p])[c]), inv);
              it->second.second = ef_add(it->second.second, ef_mul(it->second.first, quo));
              it->second.first = ef_mul(it->second.first, fri_alpha);
            }
          }
        }
      }
      // verify_query
      if (qp.steps.size() != ncommit) throw std::runtime_error("bad step count");
      EF folded = ef_zero();
      size_t idx = index;
      for (uint32_t s = 0; s < ncommit; s++) {
        const int lfh = log_max - 1 - (int)s;
        auto it = ro.find(lfh + 1);
        if (it != ro.end()) {
          folded = ef_add(folded, it->second.second);
          ro.erase(it);
        }
        const CommitPhaseStep& stp = qp.steps[s];
        const EF sib = stp.sibling;
        if ((int)stp.path.size() != lfh) throw std::runtime_error("bad FRI path length");
        std::vector<uint32_t> path(8 * stp.path.size());
        for (size_t L = 0; L < stp.path.size(); L++) std::memcpy(&path[8 * L], stp.path[L].data(), 32);
        EF ev[2];
        ev[idx & 1] = folded;
        ev[(idx & 1) ^ 1] = sib;
        std::vector<std::vector<uint32_t>> row(1, std::vector<uint32_t>(8));
        std::memcpy(row[0].data(), ev[0].c, 16);
        std::memcpy(row[0].data() + 4, ev[1].c, 16);
        if (!verify_batch(pf.commit_roots[s].data(), {(size_t)1 << lfh}, {8}, idx >> 1, row, path))
          throw std::runtime_error("FRI commit-phase opening rejected");
        idx >>= 1;
        const uint32_t x0 = mpow(two_adic_gen(lfh + 1), bitrev32((uint32_t)idx, lfh));
        const uint32_t x1 = mneg(x0);
        const EF t = ef_mul(ef_sub(betas[s], ef_base(x0)), ef_sub(ev[1], ev[0]));
        folded = ef_add(ev[0], ef_mul_base(t, minv(msub(x1, x0))));
      }
      {  // a 1-row trace's height-2 input joins after the last fold, as in the commit phase (D11)
        auto it = ro.find(log_max - (int)ncommit);
        if (it != ro.end()) {
          folded = ef_add(folded, it->second.second);
          ro.erase(it);
        }
      }
      if (!ro.empty()) throw std::runtime_error("unconsumed reduced openings");
      if (!ef_eq(folded, final_poly)) throw std::runtime_error("FRI final value mismatch");
    }
  }
}

void after_queries(const ShardState& S) {
  const ShardProof& pf = *S.pf;
  const std::vector<int>& chip = pf.chips;
  const std::vector<ChipOpen>& co = S.co;
  const uint32_t nc = (uint32_t)chip.size();
  const EF pa = S.pa, pb = S.pb, alpha = S.alpha, zeta = S.zeta;
  {
    // ---- OOD constraint checks (verifier.rs:194-213)
    EF total = ef_zero();
    for (uint32_t i = 0; i < nc; i++) {
      const ChipOpen& c = co[i];
      const int n_log = c.log_n;
      const uint32_t w2n = two_adic_gen(n_log + 1);
      const uint32_t sh[2] = {to_mont(3), mmul(to_mont(3), w2n)};
      EF zps[2];
      for (int a = 0; a < 2; a++) {
        const int o = 1 - a;
        zps[a] = ef_mul(zp_at(n_log, sh[o], zeta), ef_inv(zp_at(n_log, sh[o], ef_base(sh[a]))));
      }
      EF quot = ef_zero();
      for (int a = 0; a < 2; a++)
        for (int e = 0; e < 4; e++) quot = ef_add(quot, ef_mul(ef_mul(zps[a], monomial(e)), c.q[a][e]));
      const uint32_t gn_inv = minv(two_adic_gen(n_log));
      EF zh = zeta;
      for (int k = 0; k < n_log; k++) zh = ef_mul(zh, zh);
      zh = ef_sub(zh, ef_one());
      const EF first = ef_mul(zh, ef_inv(ef_sub(zeta, ef_one())));
      const EF last = ef_mul(zh, ef_inv(ef_sub(zeta, ef_base(gn_inv))));
      const EF trans = ef_sub(zeta, ef_base(gn_inv));
      const int pw = perm_width(chip[i]);
      std::vector<EF> perml(pw), permn(pw);
      for (int e = 0; e < pw; e++) {
        perml[e] = ef_zero();
        permn[e] = ef_zero();
        for (int k = 0; k < 4; k++) {
          perml[e] = ef_add(perml[e], ef_mul(monomial(k), c.perml[4 * e + k]));
          permn[e] = ef_add(permn[e], ef_mul(monomial(k), c.permn[4 * e + k]));
        }
      }
      EF pb_pows[8];
      pb_pows[0] = ef_one();
      for (int j = 1; j < 8; j++) pb_pows[j] = ef_mul(pb_pows[j - 1], pb);
      const EF folded = fold_any(chip[i], c.pl, c.pn, c.ml, c.mn, perml, permn, pa, pb_pows, c.cumsum,
                                 first, last, trans, alpha);
      if (!ef_eq(ef_mul(folded, ef_inv(zh)), quot))
        throw std::runtime_error(std::string("OOD evaluation mismatch on chip ") + CHIP_INFO[chip[i]].name);
      total = ef_add(total, c.cumsum);
    }
    if (!ef_is_zero(total)) throw std::runtime_error("cumulative sums do not sum to zero");
  }
}

// The three stages in order, as the reference runs them; *query follows the query loop.
VerifyOutcome run_host(const std::string& src, const uint32_t vk_commit[8], const ShardProof& pf,
                       const VerifyOptions& opt) {
  VerifyOutcome o;
  try {
    ShardState S;
    before_queries(src, vk_commit, pf, opt, S);
    for (uint32_t q = 0; q < S.nq; q++) {
      o.query = (int)q;
      check_query(S, q);
    }
    o.query = -1;
    after_queries(S);
    o.ok = true;
  } catch (const std::exception& e) {
    o.why = e.what();
  }
  return o;
}

// ------------------------------------------------------------------ packing for the device
// The per-query shape checks of check_query, in its order; false at the first that would throw.
bool query_shape_ok(const ShardState& S, const QueryProof& qp) {
  if (qp.inputs.size() != (size_t)S.nrounds) return false;
  for (int rr = 0; rr < S.nrounds; rr++) {
    const BatchOpening& bo = qp.inputs[rr];
    if (bo.rows.size() != S.rounds[rr].size()) return false;
    int lbmax = 0;
    for (size_t i = 0; i < bo.rows.size(); i++) {
      if ((int)bo.rows[i].size() != S.rounds[rr][i].w) return false;
      lbmax = std::max(lbmax, S.rounds[rr][i].log_n + LOG_BLOWUP);
    }
    if ((int)bo.path.size() != lbmax) return false;
  }
  if (qp.steps.size() != S.ncommit) return false;
  for (uint32_t s = 0; s < S.ncommit; s++)
    if ((int)qp.steps[s].path.size() != S.log_max - 1 - (int)s) return false;
  return true;
}

void put_ef(std::vector<uint32_t>& w, const EF& e) { w.insert(w.end(), e.c, e.c + 4); }

// Appends one proof to the batch: its descriptor (slot `slot`) and its data.  Queries
// [0, first_bad) have the shapes the descriptor states and are packed; *first_bad == nq if all do.
// Every offset and length the kernels use is computed here from S (the program, the vk and the
// chips' validated log degrees), never taken from a query's own vectors.
void pack_proof(const ShardState& S, QueryBatch& B, uint32_t slot, uint32_t* first_bad) {
  const ShardProof& pf = *S.pf;
  uint32_t nq = 0;
  while (nq < S.nq && query_shape_ok(S, pf.queries[nq])) nq++;
  *first_bad = nq;
  VProof D;
  std::memset(&D, 0, sizeof D);
  D.nq = nq;
  D.log_max = (uint32_t)S.log_max;
  D.ncommit = S.ncommit;
  D.nrounds = (uint32_t)S.nrounds;
  D.final_poly = S.final_poly;
  if (S.nrounds < 1 || S.nrounds > 4) throw std::runtime_error("verify_batch: bad round count");
  if (S.log_max < 1 || S.log_max > 24) throw std::runtime_error("verify_batch: log height out of range");
  std::vector<uint32_t>& W = B.words;

  // the record of one query: per round the rows in Merkle order and the path, then the steps
  uint32_t rec = 0;
  std::vector<int> ord[4];                  // Merkle order of each round's matrices
  std::vector<uint32_t> mat_off[4];         // record offset of matrix i's row
  for (int rr = 0; rr < S.nrounds; rr++) {
    const std::vector<VMat>& ms = S.rounds[rr];
    ord[rr].resize(ms.size());
    for (size_t i = 0; i < ms.size(); i++) ord[rr][i] = (int)i;
    std::stable_sort(ord[rr].begin(), ord[rr].end(),
                     [&](int a, int b) { return ms[a].log_n > ms[b].log_n; });
    VRoundD& R = D.rd[rr];
    R.rows_off = rec;
    mat_off[rr].resize(ms.size());
    for (int i : ord[rr]) {
      const VMat& m = ms[i];
      if (m.w < 1 || m.w > VQ_MAX_WIDTH) throw std::runtime_error("verify_batch: row width out of range");
      const uint32_t lh = (uint32_t)(m.log_n + LOG_BLOWUP);
      if (R.ngroups == 0 || R.g_lh[R.ngroups - 1] != lh) {
        if (R.ngroups == VQ_MAX_HEIGHTS) throw std::runtime_error("verify_batch: too many heights");
        R.g_lh[R.ngroups] = lh;
        R.g_w[R.ngroups] = 0;
        R.ngroups++;
      }
      R.g_w[R.ngroups - 1] += (uint32_t)m.w;
      mat_off[rr][i] = rec;
      rec += (uint32_t)m.w;
    }
    R.lb = R.g_lh[0];
    R.path_off = rec;
    rec += 8 * R.lb;
    std::memcpy(R.root, S.roots[rr], 32);
  }
  D.steps_off = rec;
  for (uint32_t s = 0; s < S.ncommit; s++) rec += 4 + 8 * (uint32_t)(S.log_max - 1 - (int)s);
  D.qstride = rec;

  // reduced openings: per LDE height, the matrices in the verifier's order (round, then matrix),
  // alpha^k running over (matrix, point, column) across the rounds
  std::vector<int> heights;
  for (int rr = 0; rr < S.nrounds; rr++)
    for (const VMat& m : S.rounds[rr]) {
      const int lh = m.log_n + LOG_BLOWUP;
      if (std::find(heights.begin(), heights.end(), lh) == heights.end()) heights.push_back(lh);
    }
  if (heights.size() > (size_t)VQ_MAX_HEIGHTS) throw std::runtime_error("verify_batch: too many heights");
  D.nheights = (uint32_t)heights.size();
  for (size_t j = 0; j < heights.size(); j++) {
    VHeightD& H = D.hs[j];
    H.lh = (uint32_t)heights[j];
    H.m0 = D.nmats;
    H.a0 = H.a1 = ef_zero();
    H.z0 = S.zeta;
    H.z1 = ef_mul_base(S.zeta, two_adic_gen(heights[j] - LOG_BLOWUP));
    EF apow = ef_one();
    for (int rr = 0; rr < S.nrounds; rr++)
      for (size_t i = 0; i < S.rounds[rr].size(); i++) {
        const VMat& m = S.rounds[rr][i];
        if (m.log_n + LOG_BLOWUP != heights[j]) continue;
        if (D.nmats == (uint32_t)VQ_MAX_MATS) throw std::runtime_error("verify_batch: too many matrices");
        VMatD& M = D.mats[D.nmats++];
        M.off = mat_off[rr][i];
        M.w = (uint32_t)m.w;
        M.np = (uint32_t)m.np;
        M.c0 = M.c1 = ef_zero();
        for (int p = 0; p < m.np; p++) {
          // every point of this height is zeta or zeta * g (the quotient chunks: zeta only)
          const bool second = p == 1;
          if (!ef_eq(m.pt[p], second ? H.z1 : H.z0)) throw std::runtime_error("verify_batch: unexpected opening point");
          (second ? M.c1 : M.c0) = apow;
          EF& a = second ? H.a1 : H.a0;
          for (int c = 0; c < m.w; c++) {
            a = ef_add(a, ef_mul(apow, (*m.v[p])[c]));
            apow = ef_mul(apow, S.fri_alpha);
          }
        }
      }
    H.m1 = D.nmats;
  }

  // data
  D.idx_off = (uint32_t)W.size();
  for (uint32_t q = 0; q < nq; q++) W.push_back((uint32_t)S.index[q]);
  D.croot_off = (uint32_t)W.size();
  for (uint32_t s = 0; s < S.ncommit; s++) W.insert(W.end(), pf.commit_roots[s].begin(), pf.commit_roots[s].end());
  D.beta_off = (uint32_t)W.size();
  for (uint32_t s = 0; s < S.ncommit; s++) put_ef(W, S.betas[s]);
  D.apow_off = (uint32_t)W.size();
  {
    EF a = ef_one();
    for (int c = 0; c < VQ_MAX_WIDTH; c++, a = ef_mul(a, S.fri_alpha)) put_ef(W, a);
  }
  D.qbase = (uint32_t)W.size();
  for (uint32_t q = 0; q < nq; q++) {
    const QueryProof& qp = pf.queries[q];
    for (int rr = 0; rr < S.nrounds; rr++) {
      const BatchOpening& bo = qp.inputs[rr];
      for (int i : ord[rr]) W.insert(W.end(), bo.rows[i].begin(), bo.rows[i].end());
      for (const Digest& d : bo.path) W.insert(W.end(), d.begin(), d.end());
    }
    for (const CommitPhaseStep& st : qp.steps) {
      put_ef(W, st.sibling);
      for (const Digest& d : st.path) W.insert(W.end(), d.begin(), d.end());
    }
    if (W.size() != (size_t)D.qbase + (size_t)(q + 1) * D.qstride)
      throw std::runtime_error("verify_batch: query record length mismatch");
  }
  if (W.size() >= ((size_t)1 << 31)) throw std::runtime_error("verify_batch: batch too large");
  D.leaf_base = (uint32_t)B.leaf_words;
  B.leaf_words += (size_t)nq * S.ncommit * 8;
  D.ro_base = (uint32_t)B.ro_words;
  B.ro_words += (size_t)nq * VQ_RO_SLOTS * 4;
  B.max_nq = std::max(B.max_nq, nq);
  B.max_ncommit = std::max(B.max_ncommit, S.ncommit);
  B.max_nrounds = std::max(B.max_nrounds, (uint32_t)S.nrounds);
  std::memcpy(&W[B.desc_off() + (size_t)slot * (sizeof(VProof) / 4)], &D, sizeof D);
}

const char* reason_of_stage(uint32_t stage) {
  if (stage < (uint32_t)VQ_STAGE_STEP0) return "input Merkle opening rejected";
  if (stage < (uint32_t)VQ_STAGE_FINAL) return "FRI commit-phase opening rejected";
  return "FRI final value mismatch";
}

}  // namespace

bool verify_proof(const std::string& src, const uint32_t vk_commit[8], const uint8_t* proof,
                  size_t len, const VerifyOptions& opt, std::string* why) {
  ShardProof pf;
  try {
    pf = decode_bfz1(proof, len);
  } catch (const std::exception& e) {
    if (why) *why = e.what();
    return false;
  }
  return verify_shard(src, vk_commit, pf, opt, why);
}

bool verify_shard(const std::string& src, const uint32_t vk_commit[8], const ShardProof& pf,
                  const VerifyOptions& opt, std::string* why) {
  const VerifyOutcome o = run_host(src, vk_commit, pf, opt);
  if (!o.ok && why) *why = o.why;
  return o.ok;
}

namespace {
// The device path of a batch, for any proof kind whose query loop is check_query over a
// ShardState: Slot holds one decoded proof and its state `S`; stage(i, slot) decodes proof i and
// runs everything before the query loop (throwing the reason of the first failed check),
// after(i, slot) runs what follows the loop.  The query loops of the proofs that got through
// stage are packed into one QueryBatch per chunk and handed to run_queries.
template <class Slot, class Stage, class After>
std::vector<VerifyOutcome> batch_on_device(const size_t* lens, size_t n, QueryRunner run_queries,
                                           Stage stage, After after) {
  std::vector<VerifyOutcome> out(n);
  // the device pass takes the proofs in chunks that bound the packed batch (2^31 words at most)
  constexpr size_t CHUNK_PROOFS = 1024, CHUNK_BYTES = (size_t)512 << 20;
  for (size_t i0 = 0; i0 < n;) {
    size_t i1 = i0, bytes = 0;
    while (i1 < n && i1 - i0 < CHUNK_PROOFS && (i1 == i0 || bytes + lens[i1] <= CHUNK_BYTES)) bytes += lens[i1++];
    const size_t k = i1 - i0;
    // stage one on the host; the survivors are packed
    std::vector<Slot> slots(k);
    std::vector<size_t> packed;
    for (size_t j = 0; j < k; j++) {
      try {
        stage(i0 + j, slots[j]);
        packed.push_back(j);
      } catch (const std::exception& e) {
        out[i0 + j].why = e.what();
      }
    }
    QueryBatch B;
    B.nproofs = (uint32_t)packed.size();
    B.words.assign(B.desc_off() + packed.size() * (sizeof(VProof) / 4), 0);
    for (uint32_t s = 0; s < B.nproofs; s++) B.words[s] = VQ_NO_FAILURE;
    for (int b = 0; b < 32; b++) {
      const uint32_t g = b <= 24 ? two_adic_gen(b) : ONE;
      B.words[B.nproofs + b] = g;
      B.words[B.nproofs + 32 + b] = minv(g);
    }
    std::vector<uint32_t> first_bad(packed.size());
    for (uint32_t s = 0; s < B.nproofs; s++) {
      // A proof the packing refuses (before_queries lets through shapes no honest prover makes,
      // such as a preprocessed chip whose claimed log degree is not its key's: more heights than
      // the descriptor holds) is that proof's matter, not the call's: its slot stays empty and
      // all its queries run on the host below, so it gets the host's reason.
      const uint32_t max_nq = B.max_nq, max_ncommit = B.max_ncommit, max_nrounds = B.max_nrounds;
      const size_t words = B.words.size(), leaf_words = B.leaf_words, ro_words = B.ro_words;
      try {
        pack_proof(slots[packed[s]].S, B, s, &first_bad[s]);
      } catch (const std::exception&) {
        B.words.resize(words);
        B.max_nq = max_nq;
        B.max_ncommit = max_ncommit;
        B.max_nrounds = max_nrounds;
        B.leaf_words = leaf_words;
        B.ro_words = ro_words;
        std::fill_n(&B.words[B.desc_off() + (size_t)s * (sizeof(VProof) / 4)], sizeof(VProof) / 4, 0u);
        first_bad[s] = 0;
      }
    }
    std::vector<uint32_t> keys(packed.size(), VQ_NO_FAILURE);
    if (B.max_nq) run_queries(B, keys.data());
    for (uint32_t s = 0; s < B.nproofs; s++) {
      const size_t j = packed[s];
      VerifyOutcome& o = out[i0 + j];
      const ShardState& S = slots[j].S;
      if (keys[s] != VQ_NO_FAILURE) {  // the first failure among the packed queries
        if ((keys[s] >> 6) >= first_bad[s]) throw std::runtime_error("verify_batch: device key out of range");
        o.query = (int)(keys[s] >> 6);
        o.why = reason_of_stage(keys[s] & 63);
        continue;
      }
      try {
        // a query of another shape than the descriptor's, and whatever follows it, stays on the host
        for (uint32_t q = first_bad[s]; q < S.nq; q++) {
          o.query = (int)q;
          check_query(S, q);
        }
        o.query = -1;
        after(i0 + j, slots[j]);
        o.ok = true;
      } catch (const std::exception& e) {
        o.why = e.what();
      }
    }
    i0 = i1;
  }
  return out;
}

}  // namespace

std::vector<VerifyOutcome> verify_batch(const std::string& src, const uint32_t vk_commit[8],
                                        const uint8_t* const* proofs, const size_t* lens, size_t n,
                                        const VerifyOptions& opt, QueryRunner run_queries) {
  if (!run_queries) {  // one proof decoded at a time, as bfz_verify
    std::vector<VerifyOutcome> out(n);
    for (size_t i = 0; i < n; i++) {
      try {
        const ShardProof pf = decode_bfz1(proofs[i], lens[i]);
        out[i] = run_host(src, vk_commit, pf, opt);
      } catch (const std::exception& e) {
        out[i].why = e.what();
      }
    }
    return out;
  }
  struct Slot {
    ShardProof pf;
    ShardState S;
  };
  return batch_on_device<Slot>(
      lens, n, run_queries,
      [&](size_t i, Slot& s) {
        s.pf = decode_bfz1(proofs[i], lens[i]);
        before_queries(src, vk_commit, s.pf, opt, s.S);
      },
      [](size_t, const Slot& s) { after_queries(s.S); });
}

// ------------------------------------------------------------------ per-chip uni-STARK proofs
namespace {
template <int CHIP>
EF fold_air(const std::vector<EF>& ml, const std::vector<EF>& mn, const EF& first, const EF& last,
            const EF& trans, const EF& alpha) {
  HornerAcc acc;
  acc.alpha = alpha;
  static const EF zero1[1] = {ef_zero()};  // no preprocessed trace
  Air<ExtOps, HornerAcc> air{ml.data(), mn.data(), zero1, zero1, first, last, trans, acc};
  air.template eval_air<CHIP>();
  return acc.acc;
}
EF fold_air_any(int chip, const std::vector<EF>& ml, const std::vector<EF>& mn, const EF& f,
                const EF& l, const EF& t, const EF& al) {
  switch (chip) {
    case CHIP_CPU: return fold_air<CHIP_CPU>(ml, mn, f, l, t, al);
    case CHIP_ADDSUB: return fold_air<CHIP_ADDSUB>(ml, mn, f, l, t, al);
    case CHIP_JUMP: return fold_air<CHIP_JUMP>(ml, mn, f, l, t, al);
    case CHIP_MEMINSTRS: return fold_air<CHIP_MEMINSTRS>(ml, mn, f, l, t, al);
    case CHIP_IO: return fold_air<CHIP_IO>(ml, mn, f, l, t, al);
  }
  throw std::runtime_error("bad chip");
}
// The same fold for a constraint program: its K values at zeta by Horner (acc = acc * alpha + c).
EF fold_program(const AirProgram& p, const std::vector<EF>& ml, const std::vector<EF>& mn,
                const EF& first, const EF& last, const EF& trans, const EF& alpha) {
  std::vector<EF> c((size_t)p.num_constraints);
  air_eval_ef(p, ml.data(), mn.data(), first, last, trans, c.data());
  EF acc = ef_zero();
  for (const EF& v : c) acc = ef_add(ef_mul(acc, alpha), v);
  return acc;
}
UniAir verifier_air_of_chip(int chip) {  // a refusal here is the proof's verdict, not an error
  int K = 0, degree = 0, lqd = 0;
  if (!uni_air_shape(chip, &K, &degree, &lqd) || lqd > 1)
    throw std::runtime_error("chip has no uni-STARK AIR");
  return uni_air_of_chip(chip);
}
}  // namespace

// p3_uni_stark::verify [p3-recalled] as utils::uni_stark_verify calls it (utils/prove.rs:129-159),
// in verify_shard's three stages: uni_before_queries (decode, shapes from the chip table, never
// from the proof, the transcript head, pcs_transcript), check_query over S with two input rounds,
// uni_after_queries (the quotient recomposed at zeta from its chunks, the selectors at zeta, the
// AIR folded with alpha).  S refers into u: a UniState stays where it was filled.
namespace {
struct UniState {
  UniProof u;
  ShardState S;
  UniAir air;
  int log_n = 0, nchunks = 0;
  EF alpha;
  std::vector<uint32_t> sh;  // chunk j's domain shift
};

void uni_before_queries(const UniAir& air, Challenger& ch, const uint8_t* proof, size_t len,
                        const UniOptions& opt, UniState& U) {
  const int lqd = air.log_quotient_degree;
  if (lqd > 1) throw std::runtime_error("chip has no uni-STARK AIR");
  U.u = decode_bfu1(proof, len);
  const UniProof& u = U.u;
  // a program's proof: the chip word is a label outside the transcript and is not interpreted
  if (!air.prog && u.chip != (uint32_t)air.chip) throw std::runtime_error("proof is for another chip");
  // unsigned: a huge word must not become a negative shift count below
  if (u.log_degree > 23) throw std::runtime_error("log degree out of range");
  const int log_n = U.log_n = (int)u.log_degree, nchunks = U.nchunks = 1 << lqd;
  U.air = air;
  const size_t w = (size_t)air.width;
  if (u.trace_local.size() != w || u.trace_next.size() != w || u.chunks.size() != (size_t)nchunks)
    throw std::runtime_error("opened-value shape mismatch");
  for (const std::vector<EF>& c : u.chunks)
    if (c.size() != 4) throw std::runtime_error("opened-value shape mismatch");

  // ---- transcript head (U1, U2)
  if (opt.observe_degree) ch.observe(to_mont((uint32_t)log_n));
  ch.observe_digest(u.pcs.main_root.data());
  U.alpha = ch.sample_ef();
  ch.observe_digest(u.pcs.quot_root.data());
  const EF zeta = ch.sample_ef();

  // ---- PCS verify: [trace: (zeta, zeta w_n)], [chunk j: (zeta)] on 3 w_(n 2^lqd)^j H_n
  ShardState& S = U.S;
  S.pf = &u.pcs;
  S.nrounds = 2;
  S.zeta = zeta;
  S.roots[0] = u.pcs.main_root.data();
  S.roots[1] = u.pcs.quot_root.data();
  S.rounds[0].push_back(VMat{log_n, ONE, (int)w, 2, {zeta, ef_mul_base(zeta, two_adic_gen(log_n))},
                             {&u.trace_local, &u.trace_next}});
  const uint32_t wq = two_adic_gen(log_n + lqd);
  U.sh.resize(nchunks);
  for (int j = 0; j < nchunks; j++) {
    U.sh[j] = mmul(to_mont(3), mpow(wq, (uint64_t)j));
    S.rounds[1].push_back(VMat{log_n, U.sh[j], 4, 1, {zeta, zeta}, {&u.chunks[j], &u.chunks[j]}});
  }
  pcs_transcript(S, ch, opt.observe_openings, opt.num_queries);
}

// The quotient at zeta from its chunks, the selectors, the folded constraints.
void uni_after_queries(const UniState& U) {
  const UniProof& u = U.u;
  const int log_n = U.log_n, nchunks = U.nchunks;
  const std::vector<uint32_t>& sh = U.sh;
  const EF zeta = U.S.zeta;
  EF quot = ef_zero();
  for (int a = 0; a < nchunks; a++) {
    EF zps = ef_one();
    for (int b = 0; b < nchunks; b++)
      if (b != a)
        zps = ef_mul(zps, ef_mul(zp_at(log_n, sh[b], zeta), ef_inv(zp_at(log_n, sh[b], ef_base(sh[a])))));
    for (int e = 0; e < 4; e++) quot = ef_add(quot, ef_mul(ef_mul(zps, monomial(e)), u.chunks[a][e]));
  }
  const uint32_t gn_inv = minv(two_adic_gen(log_n));
  EF zh = zeta;
  for (int k = 0; k < log_n; k++) zh = ef_mul(zh, zh);
  zh = ef_sub(zh, ef_one());
  const EF first = ef_mul(zh, ef_inv(ef_sub(zeta, ef_one())));
  const EF last = ef_mul(zh, ef_inv(ef_sub(zeta, ef_base(gn_inv))));
  const EF trans = ef_sub(zeta, ef_base(gn_inv));
  const EF folded =
      U.air.prog ? fold_program(*U.air.prog, u.trace_local, u.trace_next, first, last, trans, U.alpha)
                 : fold_air_any(U.air.chip, u.trace_local, u.trace_next, first, last, trans, U.alpha);
  if (!ef_eq(ef_mul(folded, ef_inv(zh)), quot))
    throw std::runtime_error(std::string("OOD evaluation mismatch on chip ") + U.air.name);
}
}  // namespace

namespace {
// air_of: the AIR, made inside the try (a chip without one is a verdict)
template <class AirOf>
VerifyOutcome uni_verify_with(AirOf&& air_of, Challenger& ch, const uint8_t* proof, size_t len,
                              const UniOptions& opt) {
  VerifyOutcome o;
  try {
    UniState U;
    uni_before_queries(air_of(), ch, proof, len, opt, U);
    for (uint32_t q = 0; q < U.S.nq; q++) {
      o.query = (int)q;
      check_query(U.S, q);
    }
    o.query = -1;
    uni_after_queries(U);
    o.ok = true;
  } catch (const std::exception& e) {
    o.why = e.what();
  }
  return o;
}
}  // namespace

VerifyOutcome uni_verify(int chip, Challenger& ch, const uint8_t* proof, size_t len,
                         const UniOptions& opt) {
  return uni_verify_with([&] { return verifier_air_of_chip(chip); }, ch, proof, len, opt);
}

VerifyOutcome uni_verify(const UniAir& air, Challenger& ch, const uint8_t* proof, size_t len,
                         const UniOptions& opt) {
  return uni_verify_with([&] { return air; }, ch, proof, len, opt);
}

std::vector<VerifyOutcome> uni_verify_batch(const int* chips, Challenger* chs,
                                            const uint8_t* const* proofs, const size_t* lens,
                                            size_t n, const UniOptions& opt, QueryRunner run_queries) {
  if (!run_queries) {
    std::vector<VerifyOutcome> out(n);
    for (size_t i = 0; i < n; i++) out[i] = uni_verify(chips[i], chs[i], proofs[i], lens[i], opt);
    return out;
  }
  return batch_on_device<UniState>(
      lens, n, run_queries,
      [&](size_t i, UniState& U) {
        uni_before_queries(verifier_air_of_chip(chips[i]), chs[i], proofs[i], lens[i], opt, U);
      },
      [](size_t, const UniState& U) { uni_after_queries(U); });
}

// Columns a chip's constraints read at the next row (quotient.rs:41-42), found by perturbing
// one next-row value at a time in a random evaluation of fold_any (a column the constraints do
// not read cannot change the folded value; one that they read changes it except with
// probability ~1/p).  The sharded prover computes next-row shards only for these columns.
NextCols next_row_columns(int chip) {
  const ChipInfo& ci = CHIP_INFO[chip];
  uint64_t seed = 0x9E3779B97F4A7C15ull * (uint64_t)(chip + 1);
  auto rnd = [&] {
    seed = seed * 6364136223846793005ull + 1442695040888963407ull;
    return to_mont((uint32_t)((seed >> 33) % P));
  };
  auto rnd_ef = [&] { return EF{{rnd(), rnd(), rnd(), rnd()}}; };
  auto vec = [&](size_t n) {
    std::vector<EF> v(n);
    for (EF& e : v) e = rnd_ef();
    return v;
  };
  const size_t pw = (size_t)perm_width(chip);  // fold_any takes the perm values as EF columns
  std::vector<EF> pl = vec(ci.prep_w), pn = vec(ci.prep_w), ml = vec(ci.main_w), mn = vec(ci.main_w),
                  perml = vec(pw), permn = vec(pw);
  EF pb[8];
  for (EF& e : pb) e = rnd_ef();
  const EF pa = rnd_ef(), cs = rnd_ef(), f = rnd_ef(), l = rnd_ef(), t = rnd_ef(), al = rnd_ef();
  auto fold = [&] { return fold_any(chip, pl, pn, ml, mn, perml, permn, pa, pb, cs, f, l, t, al); };
  const EF base = fold();
  NextCols nc;
  for (int pass = 0; pass < 2; pass++) {
    std::vector<EF>& v = pass ? permn : mn;
    for (size_t c = 0; c < v.size(); c++) {
      const EF keep = v[c];
      v[c] = ef_add(v[c], ef_one());
      if (!ef_eq(fold(), base)) {
        if (pass)
          for (int k = 0; k < 4; k++) nc.perm.push_back(4 * (int)c + k);  // flatten_to_base
        else
          nc.main.push_back((int)c);
      }
      v[c] = keep;
    }
  }
  return nc;
}

}  // namespace bfz
