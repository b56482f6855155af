// TwoAdicFriPcs::open [p3-recalled] (prover.rs:417-470 for the machine proof, p3_uni_stark::prove
// for a chip's): opened values at zeta and zeta w_n, the reduced openings per LDE height, the FRI
// commit phase, the transcript tail on the device (final constant, grind, query indices), the
// query gather, one device-to-host copy of the tail and the host's replay of the device
// transcript.  The callers commit their rounds, bring the transcript to zeta and serialize what
// comes back (BFZ1: prover.hip, BFU1: uni_stark.hip).
#include "pcs_open.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>

#include "fri.h"

namespace bfz {

using namespace kb;

Plan make_plan() {
  Plan p;
  const ShardCtx* c = shard_ctx();
  if (!c || c->world <= 1) return p;
  p.G = c->world;
  p.lg = log2i((size_t)p.G);
  p.k = c->rank;
  p.r = (int)bitrev32((uint32_t)p.k, p.lg);
  p.r2 = (p.r + 2) % p.G;
  p.k2 = (int)bitrev32((uint32_t)p.r2, p.lg);
  return p;
}

// The end of the FRI commit phase packed for one device-to-host copy (the head of the tail
// buffer): [root 0 .. root MAX-1 (8 words each) | state (16) | final layer (2 EF)].  nroots may
// be 0 (state then unused, but still read: 16 valid words).
constexpr int MAX_FRI_ROUNDS = 32;
struct FriTail {
  const uint32_t* root[MAX_FRI_ROUNDS];
  int nroots;
  const uint32_t* state;
  const EF* fin;
};
__global__ void k_pack_fri_tail(FriTail t, uint32_t* __restrict__ packed) {
  const int i = threadIdx.x;
  if (i < 8 * t.nroots) packed[i] = t.root[i >> 3][i & 7];
  if (i < 16) packed[8 * MAX_FRI_ROUNDS + i] = t.state[i];
  if (i < 8) packed[8 * MAX_FRI_ROUNDS + 16 + i] = t.fin[i >> 2].c[i & 3];
}

PcsOpenOut pcs_open(const PcsOpenIn& in, Challenger& ch) {
  hipStream_t st = stream();
  EvTimer untimed;
  EvTimer& ev = in.ev ? *in.ev : untimed;
  StageTimes* tms = in.tms;
  const Plan& plan = in.plan;
  const ShardCtx* shard = in.shard;
  const int nr = (int)in.rounds.size();
  std::vector<const Round*> rounds(nr);
  for (int r = 0; r < nr; r++) rounds[r] = in.rounds[r].round;
  // Single GPU: the openings read zeta from the device, so they are queued with no host round
  // trip behind whatever produced it; the host's value is needed by a sharded plan only.
  const bool dev_zeta = !plan.on();
  const EF* const zeta_d = in.zeta_d;
  const EF zeta = in.zeta;
  PcsOpenOut out;

  // ---- PCS open: opened values (prover.rs:417-470)
  hipEvent_t e3 = ev.on ? ev.begin(st) : nullptr;
  Span span("open multi batches");  // prover.rs:460 (opened values, reduced openings, FRI, queries)
  struct MatPts {
    EF pts[2];  // (sharded plans)
  };
  std::vector<std::vector<MatPts>> mpt(nr);
  std::vector<std::vector<PcsOpenOut::MatPts>>& mp = out.mp;
  mp.resize(nr);
  int Lmax = 0;
  size_t nvals = 0;
  for (int r = 0; r < nr; r++) {
    for (size_t i = 0; i < rounds[r]->mats.size(); i++) {
      const CMat& m = rounds[r]->mats[i];
      PcsOpenOut::MatPts p{};
      p.npts = in.rounds[r].two[i] ? 2 : 1;
      for (int j = 0; j < p.npts; j++) {
        p.off[j] = nvals;
        nvals += m.lde.width;
      }
      mp[r].push_back(p);
      mpt[r].push_back({{zeta, ef_mul_base(zeta, two_adic_gen(m.log_n))}});
      Lmax = std::max(Lmax, m.log_n + LOG_BLOWUP);
    }
  }
  // Inverse denominators 1 / (x_t - point), indexed by global LDE position.  Unsharded: one
  // table over the tallest height for zeta (smaller heights read its prefix) and one per height
  // for the second point.  Sharded: per height, the rank's range where the height is sharded
  // and the whole height where it is replicated.
  // A replicated matrix at a sharded height (the preprocessed ones) is opened over its whole
  // low coset: that height also gets full tables (fa, fb).
  struct Invd {
    DBuf<EF> a, b, fa, fb;
    size_t t0 = 0;
    const EF* pa() const { return a.p - t0; }
    const EF* pb() const { return b.p ? b.p - t0 : nullptr; }
    const EF* full_a() const { return fa.p ? fa.p : a.p; }  // a is full where fa is absent
    const EF* full_b() const { return fa.p ? fb.p : b.p; }
  };
  std::map<int, bool> two_at;  // LDE log heights present -> some matrix opened at two points
  std::map<int, bool> rep_at;  // ... -> a replicated matrix is opened at that height
  for (int r = 0; r < nr; r++)
    for (size_t i = 0; i < rounds[r]->mats.size(); i++) {
      const int lh = rounds[r]->mats[i].log_n + LOG_BLOWUP;
      two_at[lh] |= mp[r][i].npts == 2;
      rep_at[lh] |= !rounds[r]->mats[i].sharded;
    }
  host_mark("inv_denoms launch");
  DBuf<EF> invd_zeta, w_zeta;
  static const bool wtab_on = [] {  // BFZ_OPEN_WTAB=0: weights computed in the openings (A/B)
    const char* e = std::getenv("BFZ_OPEN_WTAB");
    return !(e && *e == '0');
  }();
  if (!plan.on()) {
    invd_zeta.reset((size_t)1 << Lmax);
    if (wtab_on) w_zeta.reset((size_t)1 << (Lmax - 1));
    inv_denoms_dev(zeta_d, Lmax, invd_zeta.p, st, w_zeta.p);
  }
  // a sharded proof's many small opening launches (one per matrix, table and height) go out as
  // one batch each (BFZ_OPEN_SHARD_BATCH=0: one launch per matrix / table / range, A/B)
  static const bool sbatch = [] {
    const char* e = std::getenv("BFZ_OPEN_SHARD_BATCH");
    return !(e && *e == '0');
  }();
  std::vector<InvJob> ijobs;
  auto inv_range = [&](const EF& z, int lh, size_t t0, size_t cnt, EF* o) {
    if (sbatch) ijobs.push_back({z, lh, t0, cnt, o});
    else inv_denoms_range(z, lh, t0, cnt, o, st);
  };
  std::map<int, Invd> invd;
  for (const auto& [lh, two] : two_at) {
    const size_t H = (size_t)1 << lh;
    const bool sh = plan.sharded(H);
    const size_t t0 = sh ? plan.row0(H) : 0, cnt = sh ? plan.blk(H) : H;
    Invd& d = invd[lh];
    d.t0 = t0;
    if (plan.on()) {
      d.a.reset(cnt);
      inv_range(zeta, lh, t0, cnt, d.a.p);
    } else {
      d.a = DBuf<EF>::borrow(invd_zeta.p, H);
    }
    const EF znext = ef_mul_base(zeta, two_adic_gen(lh - LOG_BLOWUP));
    if (two && plan.on()) {  // single GPU: read from the zeta table (prev2_pos, fri.hip)
      d.b.reset(cnt);
      inv_range(znext, lh, t0, cnt, d.b.p);
    }
    if (sh && rep_at[lh]) {  // the low coset only: positions [0, H / 2)
      d.fa.reset(H / 2);
      inv_range(zeta, lh, 0, H / 2, d.fa.p);
      if (two) {
        d.fb.reset(H / 2);
        inv_range(znext, lh, 0, H / 2, d.fb.p);
      }
    }
  }
  inv_denoms_ranges(ijobs, st);
  // Opened values.  Replicated matrices: barycentric over the low coset of the LDE.  Sharded
  // matrices: the rank's 1/G slice of sum_j c_j (z / s)^j (s = the trace domain's shift) from
  // the kept coefficients; the slices are summed across ranks below.
  DBuf<EF> opened_d(nvals);
  std::map<std::array<uint32_t, 5>, DBuf<EF>> ptabs;  // (point, log n) -> powers on the range
  std::vector<PowJob> pjobs;
  auto ptable = [&](const EF& z, int log_n, size_t j0, size_t len) {
    const std::array<uint32_t, 5> key{z.c[0], z.c[1], z.c[2], z.c[3], (uint32_t)log_n};
    auto it = ptabs.find(key);
    if (it != ptabs.end()) return (const EF*)it->second.p;
    DBuf<EF> t(len);
    if (sbatch) pjobs.push_back({z, j0, len, t.p});
    else pow_table(z, j0, len, t.p, st);
    const EF* p = t.p;
    ptabs.emplace(key, std::move(t));
    return p;
  };
  // Unsharded: the openings run in the caller's transcript-ordered groups (the machine proof:
  // preprocessed + main rounds, the permutation round, the quotient round), each copied to the
  // host as soon as it is done, so the host observes a group (~250 host permutations in all)
  // while the GPU computes the next one instead of after all of them.
  const bool grouped = !plan.on();
  auto group_of = [&](int r) { return grouped ? in.rounds[r].group : 0; };
  constexpr int NGROUP = Lane::NGEV;
  int ngroup = 1;
  for (int r = 0; r < nr; r++) ngroup = std::max(ngroup, group_of(r) + 1);
  if (ngroup > NGROUP) throw std::logic_error("pcs_open: more opening groups than lane events");
  std::vector<OpenDesc> open1g[NGROUP], open2g[NGROUP];
  size_t gend[NGROUP] = {};  // end of each group's range in the opened-value buffer
  for (int r = 0; r < nr; r++)
    for (size_t i = 0; i < rounds[r]->mats.size(); i++) {
      const CMat& m = rounds[r]->mats[i];
      const int lh = m.log_n + LOG_BLOWUP;
      const bool two = mp[r][i].npts == 2;
      EF* out_a = opened_d.p + mp[r][i].off[0];
      EF* out_b = two ? opened_d.p + mp[r][i].off[1] : nullptr;
      if (m.sharded) {
        const size_t len = m.n >> plan.lg, j0 = (size_t)plan.k * len;
        const uint32_t sinv = minv(m.shift);
        const EF* tab[2] = {nullptr, nullptr};
        for (int j = 0; j < mp[r][i].npts; j++)
          tab[j] = ptable(ef_mul_base(mpt[r][i].pts[j], sinv), m.log_n, j0, len);
        const EF ninv = ef_base(minv(to_mont((uint32_t)(m.n % P))));
        if (!sbatch) {
          open_coefficients(m.coef.p + j0, m.n, m.lde.width, len, tab[0], ninv, out_a, tab[1],
                            ninv, out_b, st);
          continue;
        }
        OpenDesc o{};  // the coefficient form in the batched launch (fri.h)
        o.tab = 1;
        o.mat = m.coef.p + j0;
        o.height = m.n;  // column stride
        o.rows = len;
        o.w = m.lde.width;
        o.logH = lh;
        o.invd_a = tab[0];
        o.invd_b = two ? tab[1] : tab[0];
        o.scale_a = o.scale_b = ninv;
        o.out_a = out_a;
        o.out_b = two ? out_b : out_a;
        (two ? open2g : open1g)[group_of(r)].push_back(o);
        continue;
      }
      const uint32_t three_n = mpow(to_mont(3), m.n);
      const uint32_t n_f = to_mont((uint32_t)(m.n % P));
      const Invd& d = invd.at(lh);
      OpenDesc o{};
      o.mat = m.lde.buf.p;
      o.height = m.lde.height;
      o.w = m.lde.width;
      o.logH = lh;
      o.invd_a = d.full_a();
      o.invd_b = two ? d.full_b() : o.invd_a;  // nullptr: derived from the zeta table
      // scale = (z^n - 3^n) / (3^n n), the same for both points ((zeta w_n)^n = zeta^n); with
      // derived second-point denominators it also carries w_n^-1 (see k_reduce)
      o.wtab = w_zeta.p;  // unsharded: the weight table (nullptr: weights computed per row)
      const uint32_t zb = two && !o.invd_b && !o.wtab ? minv(two_adic_gen(m.log_n)) : ONE;
      if (dev_zeta) {  // computed by k_open_final_batch from the device's zeta
        o.zeta = zeta_d;
        o.zlog = m.log_n;
        o.z3n = three_n;
        o.zc = minv(mmul(three_n, n_f));
        o.zb = zb;
      } else {
        const EF zn = ef_pow(zeta, m.n);
        o.scale_a = ef_mul_base(ef_sub(zn, ef_base(three_n)), minv(mmul(three_n, n_f)));
        o.scale_b = ef_mul_base(o.scale_a, zb);
      }
      o.out_a = out_a;
      o.out_b = two ? out_b : out_a;
      (two ? open2g : open1g)[group_of(r)].push_back(o);
    }
  pow_tables(pjobs, st);  // before the opening batches that read them (same stream)
  for (int r = 0; r < nr; r++)
    if (!mp[r].empty()) {
      const PcsOpenOut::MatPts& last = mp[r].back();
      gend[group_of(r)] = std::max(gend[group_of(r)], last.off[last.npts - 1] +
                                                          rounds[r]->mats.back().lde.width);
    }
  std::vector<EF>& opened = out.opened;
  opened.resize(nvals);
  // gev / gbox (and tbox below) belong to this proof's lane and are reallocated on the
  // assumption that no copy into them is pending: safe only because every caller holds the API
  // lock (one proof per lane at a time) and every proof synchronizes before it returns.  A
  // caller outside the lock is a bug.
  if (api_lock_depth() == 0) throw std::logic_error("pcs_open called outside the bfz API lock");
  Lane& ln = lane();
  hipEvent_t* gev = ln.gev;
  if (grouped) {
    if (!gev[0])
      for (int g = 0; g < NGROUP; g++) HIP_CHECK(hipEventCreateWithFlags(&gev[g], hipEventDisableTiming));
    if (nvals > ln.gcap) {  // no copy into it is pending: every proof waits for its groups
      if (ln.gbox) HIP_CHECK(hipHostFree(ln.gbox));
      ln.gbox = nullptr;
      ln.gcap = 0;
      const size_t cap = std::max(nvals, (size_t)1024);
      HIP_CHECK(hipHostMalloc(&ln.gbox, cap * sizeof(EF), hipHostMallocDefault));
      ln.gcap = cap;
    }
  }
  EF* gbox = static_cast<EF*>(ln.gbox);
  for (int g = 0; g < (grouped ? ngroup : 1); g++) {
    open_batch(open2g[g], 2, st);  // barycentric openings: two partial + two final launches
    open_batch(open1g[g], 1, st);
    if (!grouped) break;
    const size_t b0 = g ? gend[g - 1] : 0, b1 = std::max(gend[g], b0);
    if (b1 > b0)
      HIP_CHECK(hipMemcpyAsync(gbox + b0, opened_d.p + b0, (b1 - b0) * sizeof(EF),
                               hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipEventRecord(gev[g], st));
  }
  // ---- reduced-opening descriptors (TwoAdicFriPcs::open, prover.rs:460-470), built while the
  // openings run: per LDE height, every column of every matrix opened there in round order; the
  // alpha-dependent parts (column coefficients alpha^k, the matrices' alpha^w, the job's ya / yb)
  // are filled by reduce_prep on the device once alpha is known, so the host's work after the
  // last opened value is observing it and sampling alpha.
  struct RedJob {
    int lh;
    size_t col0, mat0, ncols;
    int nmats;
    bool has_b;
  };
  std::vector<RedCol> red_cols;
  std::vector<RedMat> red_mats;
  std::vector<RedJob> red_jobs;
  std::vector<RedColPrep> col_prep;
  std::vector<RedMatPrep> mat_prep;
  std::vector<RedJobPrep> job_prep;
  for (int lh = Lmax; lh >= 1; lh--) {
    const size_t col0 = red_cols.size(), mat0 = red_mats.size();
    uint32_t e = 0;  // the reduction order: point a's columns, then point b's, matrix by matrix
    bool has_b = false;
    for (int r = 0; r < nr; r++)
      for (size_t i = 0; i < rounds[r]->mats.size(); i++) {
        const CMat& m = rounds[r]->mats[i];
        if (m.log_n + LOG_BLOWUP != lh) continue;
        const int w = m.lde.width;
        const bool two = mp[r][i].npts == 2;
        RedMat rm{};
        rm.first = (int)(red_cols.size() - col0);
        rm.count = w;
        rm.has_b = two ? 1 : 0;
        for (int c = 0; c < w; c++) {
          RedCol rc{};
          rc.col = m.rows() + (size_t)c * m.stride();
          red_cols.push_back(rc);
          col_prep.push_back({e + (uint32_t)c, (uint32_t)(mp[r][i].off[0] + c),
                              two ? (uint32_t)(mp[r][i].off[1] + c) : 0xffffffffu, (uint32_t)w});
        }
        // the second point's coefficients are the first point's times alpha^w; single GPU: its
        // denominators come from the zeta table times w_n^-1 (reduce_range), folded into kb / yb
        mat_prep.push_back({(uint32_t)w, two && !plan.on() ? minv(two_adic_gen(m.log_n)) : ONE});
        red_mats.push_back(rm);
        e += (uint32_t)(mp[r][i].npts * w);
        has_b |= two;
      }
    if (red_cols.size() == col0) continue;
    const size_t ncols = red_cols.size() - col0, nm = red_mats.size() - mat0;
    red_jobs.push_back({lh, col0, mat0, ncols, (int)nm, has_b});
    RedJobPrep jp{};
    jp.col0 = (uint32_t)col0;
    jp.ncols = (uint32_t)ncols;
    jp.mat0 = (uint32_t)mat0;
    jp.nmats = (uint32_t)nm;
    jp.yb_fold = has_b && !plan.on() ? minv(two_adic_gen(lh - LOG_BLOWUP)) : ONE;
    job_prep.push_back(jp);
  }
  DBuf<RedCol> red_cols_d(std::max<size_t>(red_cols.size(), 1));
  DBuf<RedMat> red_mats_d(std::max<size_t>(red_mats.size(), 1));
  DBuf<RedColPrep> col_prep_d(std::max<size_t>(col_prep.size(), 1));
  DBuf<RedMatPrep> mat_prep_d(std::max<size_t>(mat_prep.size(), 1));
  DBuf<RedJobPrep> job_prep_d(std::max<size_t>(job_prep.size(), 1));
  upload_async(red_cols_d.p, red_cols.data(), red_cols.size() * sizeof(RedCol), st);
  upload_async(red_mats_d.p, red_mats.data(), red_mats.size() * sizeof(RedMat), st);
  upload_async(col_prep_d.p, col_prep.data(), col_prep.size() * sizeof(RedColPrep), st);
  upload_async(mat_prep_d.p, mat_prep.data(), mat_prep.size() * sizeof(RedMatPrep), st);
  upload_async(job_prep_d.p, job_prep.data(), job_prep.size() * sizeof(RedJobPrep), st);
  host_mark("reduce descriptors");

  if (in.replay) in.replay();  // the openings are queued: now the host's transcript catches up
  if (plan.on()) {  // one all-gather; sharded matrices' slices summed, replicated ones kept
    DBuf<EF> all(nvals * plan.G);
    coll_sync(st);
    host_mark("sharded openings done");
    shard->allgather(opened_d.p, nvals * sizeof(EF), all.p);
    std::vector<EF> h(nvals * plan.G);
    HIP_CHECK(hipMemcpyAsync(h.data(), all.p, h.size() * sizeof(EF), hipMemcpyDeviceToHost, st));
    coll_sync(st);
    host_mark("sharded openings on host");
    for (int r = 0; r < nr; r++)
      for (size_t i = 0; i < rounds[r]->mats.size(); i++) {
        const CMat& m = rounds[r]->mats[i];
        for (int j = 0; j < mp[r][i].npts; j++)
          for (int c = 0; c < m.lde.width; c++) {
            const size_t o = mp[r][i].off[j] + c;
            EF v = h[(size_t)plan.k * nvals + o];
            if (m.sharded) {
              v = ef_zero();
              for (int g = 0; g < plan.G; g++) v = ef_add(v, h[(size_t)g * nvals + o]);
            }
            opened[o] = v;
          }
      }
  }
  // the opened values reduce_prep reads: the openings' own buffer (single GPU) or, sharded, the
  // rank-summed values assembled above
  DBuf<EF> opened_sum_d;
  const EF* opened_dev = opened_d.p;
  if (plan.on()) {
    opened_sum_d.reset(std::max<size_t>(nvals, 1));
    upload_async(opened_sum_d.p, opened.data(), nvals * sizeof(EF), st);
    opened_dev = opened_sum_d.p;
  }
  auto wait_group = [&](int g) {  // the group's values in `opened`
    for (;;) {
      const hipError_t e = hipEventQuery(gev[g]);
      if (e == hipSuccess) break;
      if (e != hipErrorNotReady) HIP_CHECK(e);
    }
    const size_t b0 = g ? gend[g - 1] : 0, b1 = std::max(gend[g], b0);
    std::copy(gbox + b0, gbox + b1, opened.begin() + b0);
  };
  if (grouped) {
    int have = -1;  // groups copied into `opened` so far
    for (int r = 0; r < nr; r++) {
      while (have < group_of(r)) wait_group(++have);
      if (in.observe_openings)  // decision D1: opened values enter the transcript
        for (size_t i = 0; i < rounds[r]->mats.size(); i++)
          for (int j = 0; j < mp[r][i].npts; j++)
            for (int c = 0; c < rounds[r]->mats[i].lde.width; c++)
              ch.observe_ef(opened[mp[r][i].off[j] + c]);
    }
    while (have < ngroup - 1) wait_group(++have);
    host_mark("opened observed");
  } else if (in.observe_openings) {
    host_mark("opened summed");
    for (int r = 0; r < nr; r++)
      for (size_t i = 0; i < rounds[r]->mats.size(); i++)
        for (int j = 0; j < mp[r][i].npts; j++)
          for (int c = 0; c < rounds[r]->mats[i].lde.width; c++)
            ch.observe_ef(opened[mp[r][i].off[j] + c]);
  }
  const EF fri_alpha = ch.sample_ef();
  host_mark("fri alpha");

  // ---- reduced openings: the alpha-dependent coefficients of the descriptors built above, then
  // one k_reduce launch per LDE height
  DBuf<EF> alpha_yab(1 + 2 * std::max<size_t>(red_jobs.size(), 1));  // alpha, then {ya, yb} per job
  upload_async(alpha_yab.p, &fri_alpha, sizeof(EF), st);
  reduce_prep(red_cols_d.p, col_prep_d.p, red_mats_d.p, mat_prep_d.p, job_prep_d.p,
              (int)red_jobs.size(), opened_dev, alpha_yab.p, alpha_yab.p + 1, st);
  std::map<int, DBuf<EF>> ro;
  for (size_t ji = 0; ji < red_jobs.size(); ji++) {
    const RedJob& j = red_jobs[ji];
    const size_t H = (size_t)1 << j.lh;
    const bool sh = plan.sharded(H);
    const size_t t0 = sh ? plan.row0(H) : 0, cnt = sh ? plan.blk(H) : H;
    DBuf<EF> r(cnt);
    const Invd& d = invd.at(j.lh);
    reduce_range(red_cols_d.p + j.col0, red_mats_d.p + j.mat0, j.nmats, H, t0, cnt, d.pa(),
                 j.has_b ? d.pb() : nullptr, alpha_yab.p + 1 + 2 * ji, j.has_b, r.p - t0, st,
                 (int)j.ncols);
    ro.emplace(j.lh, std::move(r));
  }
  if (ev.on) ev.end(e3, st, &tms->open);

  // ---- FRI commit phase (fri::prover::commit_phase)
  hipEvent_t e4 = ev.on ? ev.begin(st) : nullptr;
  // A layer of a sharded proof stays row-sharded (values [e0, e0 + len / G)) while its fold
  // output has >= G * 1024 values; the first shorter one is all-gathered and the rest is
  // computed by every rank.
  struct FriLayer {
    DBuf<EF> v;
    size_t e0 = 0;
    bool local = false;
  };
  std::vector<FriLayer> layers;
  std::vector<MerkleTree> trees;
  {
    const size_t H = (size_t)1 << Lmax;
    layers.push_back({std::move(ro.at(Lmax)), plan.sharded(H) ? plan.row0(H) : 0, plan.sharded(H)});
  }
  ro.erase(Lmax);
  // The transcript steps of the rounds run on the device (fri_challenge): the input buffer is
  // empty here (fri_alpha was just sampled), so each round is observe(root) -> one duplex ->
  // beta = 4 pops, and no host round trip is needed until the final polynomial.
  if (ch.nin != 0) throw std::runtime_error("FRI: unexpected pending challenger input");
  DBuf<uint32_t> dstate(16);
  upload_async(dstate.p, ch.st, 64, st);
  const int nrounds = Lmax - LOG_BLOWUP;
  DBuf<EF> betas(std::max(nrounds, 1));
  size_t len = (size_t)1 << Lmax;
  // Every sharded round costs one subtree-root all-gather: rounds stay sharded only while
  // h >= FRI_SHARD_MIN and the shorter tail (a few hundred thousand permutations) runs on every
  // rank after one all-gather of the layer.
  // (BFZ_FRI_SHARD_MIN overrides it: the tests shard small proofs' rounds too)
  static const size_t FRI_SHARD_MIN = [] {
    const char* e = std::getenv("BFZ_FRI_SHARD_MIN");
    return e ? (size_t)std::strtoull(e, nullptr, 10) : (size_t)1 << 18;
  }();
  auto fri_sharded = [&](size_t h) { return plan.sharded(h) && h >= FRI_SHARD_MIN; };
  auto gather = [&](DBuf<EF>& v, size_t len) {  // a row-sharded vector of len values, in place
    DBuf<EF> all(len);
    coll_sync(st);
    shard->allgather(v.p, plan.blk(len) * sizeof(EF), all.p);
    v = std::move(all);
  };
  DBuf<uint32_t> tail_trees;  // the tail rounds' trees and layers (views below borrow them)
  DBuf<EF> tail_layers;
  // A replicated round's fold is left pending and runs fused with the next round's leaf hashes
  // (fri_fold_leaves): layers.back() is then allocated but not yet written.
  struct PendingFold {
    const EF* in = nullptr;
    const EF* beta = nullptr;
    const EF* add = nullptr;
    size_t n = 0;  // fold outputs
  } pend;
  auto flush_fold = [&]() {
    if (!pend.in) return;
    fri_fold_range(pend.in, layers.back().v.p, pend.n, 0, pend.n, pend.beta, pend.add, st);
    pend = PendingFold{};
  };
  for (int rd = 0; len > ((size_t)1 << LOG_BLOWUP); rd++) {
    const size_t h = len / 2;
    FriLayer& cur = layers.back();
    if (!cur.local && h <= (size_t)FRI_TAIL_MAXH) {  // every remaining round in one launch
      flush_fold();
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
        const int lgh = log2i(hr);
        a.add[r] = ro.count(lgh) ? ro.at(lgh).p : nullptr;
        layers.push_back({DBuf<EF>::borrow(tail_layers.p + nv, hr), 0, false});
        nv += hr;
      }
      fri_tail_rounds(a, st);
      len = h >> (a.nr - 1);
      break;
    }
    if (cur.local && !fri_sharded(h)) {
      gather(cur.v, len);
      cur.e0 = 0;
      cur.local = false;
    }
    const bool loc = cur.local;
    const size_t i0 = loc ? plan.row0(h) : 0, cnt = loc ? plan.blk(h) : h;
    trees.emplace_back();
    MerkleTree& t = trees.back();
    std::function<void(size_t, size_t, uint32_t*)> fused;
    if (pend.in) {  // this round's layer is the pending fold's output: fold + hash in one pass
      const PendingFold pf = pend;
      EF* fold_out = cur.v.p;
      fused = [pf, fold_out, h, &st](size_t, size_t, uint32_t* dig) {
        fri_fold_leaves(pf.in, fold_out, h, pf.beta, pf.add, dig, st);
      };
      pend = PendingFold{};
    }
    merkle_from_rows8(t, (const uint32_t*)(cur.v.p - 2 * i0), h, st, /*fetch_root=*/false,
                      RootChallenge{dstate.p, betas.p + rd}, /*allow_shard=*/loc, fused);
    DBuf<EF> next(cnt);
    const int lgh = log2i(h);
    if (!loc && ro.count(lgh) && plan.sharded(h)) gather(ro.at(lgh), h);  // replicated tail
    const EF* add = ro.count(lgh) ? ro.at(lgh).p : nullptr;  // same range as next
    if (!loc && h / 2 >= FRI_FUSE_MIN) pend = PendingFold{cur.v.p, betas.p + rd, add, h};
    else fri_fold_range(cur.v.p, next.p, h, i0, cnt, betas.p + rd, add, st);
    layers.push_back({std::move(next), i0, loc});
    len = h;
  }
  flush_fold();
  const int nt = (int)trees.size();
  if (nt > MAX_FRI_ROUNDS) throw std::runtime_error("FRI: too many rounds");
  const int nq = in.num_queries;

  // ---- query openings: every opened word in proof order
  // Opening segments in serialization order (same for every query; see GatherSeg).
  auto owner_shift = [](const MerkleTree& t, int L) {  // layer L of a sharded tree
    const int nl = (int)t.layers.size() - 1;
    return L < t.sharded_below ? nl - L - t.shard_log : -1;
  };
  std::vector<GatherSeg> segs;
  // The segments follow the serialized query layout, its length words included as literal
  // segments (base == nullptr: count words of value xr), so the gathered words are the query
  // section of the proof as is.
  auto lit = [&](uint32_t v) { segs.push_back({nullptr, 0, 0, v, 0, 1, -1, 0}); };
  lit((uint32_t)nr);
  for (int r = 0; r < nr; r++) {
    const Round& R = *rounds[r];
    const int lrm = (int)R.tree.layers.size() - 1;
    lit((uint32_t)R.mats.size());
    for (const CMat& m : R.mats) {  // row (index >> (Lmax - lh)) of every column
      const int lh = log2i(m.lde.height);
      lit((uint32_t)m.lde.width);
      segs.push_back({m.rows(), (uint64_t)m.stride(), (uint32_t)(Lmax - lh), 0, 1,
                      (uint32_t)m.lde.width, m.sharded ? lh - plan.lg : -1, 0});
    }
    lit((uint32_t)lrm);
    for (int L = 0; L < lrm; L++)  // sibling digest at layer L
      segs.push_back({R.tree.layers[L].p, 1, (uint32_t)(Lmax - lrm + L), 1, 8, 8,
                      owner_shift(R.tree, L), 0});
  }
  lit((uint32_t)nt);
  for (int i = 0; i < nt; i++) {
    const FriLayer& fl = layers[i];  // sibling EF
    segs.push_back({(const uint32_t*)(fl.v.p - fl.e0), 1, (uint32_t)i, 1, 4, 4,
                    fl.local ? Lmax - i - plan.lg : -1, 0});
    const int lm = (int)trees[i].layers.size() - 1;
    lit((uint32_t)lm);
    for (int L = 0; L < lm; L++)
      segs.push_back({trees[i].layers[L].p, 1, (uint32_t)(i + 1 + L), 1, 8, 8,
                      owner_shift(trees[i], L), 0});
  }
  const size_t nwords = query_words(segs) * (size_t)nq;

  // ---- the transcript tail on the device: observe the final constant, grind, sample the
  // query indices (fri_transcript_tail), then the gather; one device-to-host copy returns the
  // commit-phase roots, the final layer, the challenger, the witness and the query words.
  // tail = [roots (8 MAX_FRI_ROUNDS) | FRI state (16) | final layer (8) | challenger | witness,
  //         ok | qidx (nq) | query words]
  constexpr size_t T_CH = 8 * MAX_FRI_ROUNDS + 16 + 8;
  constexpr size_t T_RES = T_CH + sizeof(DevChallenger) / 4;
  constexpr size_t T_Q = T_RES + 2;
  static_assert(sizeof(DevChallenger) % 4 == 0, "DevChallenger: whole words");
  const size_t T_W = T_Q + (size_t)nq, tail_n = T_W + nwords;
  DBuf<uint32_t> tailbuf(tail_n);
  DevChallenger* dch = reinterpret_cast<DevChallenger*>(tailbuf.p + T_CH);
  if (!nt) {  // no commit-phase round (a 1-row trace): the host challenger as it stands
    const DevChallenger hc = dev_challenger(ch);
    upload_async(dch, &hc, sizeof(hc), st);
  }
  FriTail tail{};
  for (int i = 0; i < nt; i++) tail.root[i] = trees[i].layers.back().p;
  tail.nroots = nt;
  tail.state = dstate.p;
  tail.fin = layers.back().v.p;
  hipLaunchKernelGGL(k_pack_fri_tail, dim3(1), dim3(256), 0, st, tail, tailbuf.p);
  KCHECK();
  host_mark("grind");
  fri_transcript_tail(dch, nt ? dstate.p : nullptr, layers.back().v.p, POW_BITS, nq, Lmax,
                      tailbuf.p + T_Q, tailbuf.p + T_RES, st);
  gather_queries(segs, tailbuf.p + T_Q, nq, tailbuf.p + T_W, shard, st);
  if (tail_n > ln.tcap) {  // pinned: the tail of the proof (per lane).  No copy into it is
                           // pending: every proof waits for its tail
    if (ln.tbox) HIP_CHECK(hipHostFree(ln.tbox));
    ln.tbox = nullptr;
    ln.tcap = 0;
    const size_t cap = std::max(tail_n + tail_n / 4, (size_t)1 << 18);
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&ln.tbox), cap * 4, hipHostMallocDefault));
    ln.tcap = cap;
  }
  uint32_t* tbox = ln.tbox;
  HIP_CHECK(hipMemcpyAsync(tbox, tailbuf.p, tail_n * 4, hipMemcpyDeviceToHost, st));
  spin_sync(st);
  host_mark("queries gathered");
  out.commit_roots.resize(nt);
  for (int i = 0; i < nt; i++) std::memcpy(out.commit_roots[i].data(), &tbox[8 * i], 32);
  EF fin[2];
  std::memcpy(fin, &tbox[8 * MAX_FRI_ROUNDS + 16], sizeof(fin));
  // (A uni-STARK proof of an invalid trace still gets here with a constant: each chunk is
  // interpolated from the quotient's values, so every committed matrix is a low-degree polynomial
  // whatever the trace holds, and only the verifier's out-of-domain identity fails.)
  if (!ef_eq(fin[0], fin[1]) && !(shard && shard->solo))
    throw std::runtime_error("FRI: final polynomial is not constant (trace violates the AIR)");
  const uint32_t witness = tbox[T_RES];
  if (tbox[T_RES + 1] != 1) throw std::runtime_error("grind: bad witness");
  {  // The host replays the device's FRI transcript (fri::prover: observe each commit-phase
     // root, sample its beta; observe the final constant; the witness check; the query indices)
     // and must arrive at the device's challenger and the device's query indices.
    for (int i = 0; i < nt; i++) {
      ch.observe_digest(out.commit_roots[i].data());
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
  out.final_poly = fin[0];
  out.pow_witness = witness;
  out.words = tbox + T_W;
  out.nwords = nwords;
  if (ev.on) ev.end(e4, st, &tms->fri);
  return out;
}

// kernels a proof launches (gpu.h PreloadKernels)
static PreloadKernels preload_pcs_open{(const void*)&k_pack_fri_tail};

}  // namespace bfz
