// Chip programs on the host (chip_program.h): the pairing of the two programs and the
// single-threaded row check.
#include "chip_program.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <stdexcept>
#include <string>

namespace bfz {

using namespace kb;

namespace {
std::atomic<int> g_chip_max_degree{AIR_DEFAULT_MAX_DEGREE};
}

int chip_max_degree() { return g_chip_max_degree.load(std::memory_order_relaxed); }

void set_chip_max_degree(int degree) {
  if (degree != 0 && (degree < AIR_DEFAULT_MAX_DEGREE || degree > AIR_TOP_MAX_DEGREE))
    throw std::runtime_error("chip max degree must be in [3, 9] (0 = the default, 3)");
  g_chip_max_degree.store(degree ? degree : AIR_DEFAULT_MAX_DEGREE, std::memory_order_relaxed);
}

namespace {
[[noreturn]] void chip_degree_throw(int degree, int cap) {
  throw std::runtime_error("chip program: AIR degree " + std::to_string(degree) + " is above " +
                           std::to_string(cap) + " (log quotient degree " +
                           std::to_string(ChipProgram::chip_lqd_of_degree(cap)) + ")");
}
}  // namespace

void chip_cap_or_throw(const ChipProgram& p) {
  const int cap = chip_max_degree();
  if (p.has_air && p.air.degree > cap) chip_degree_throw(p.air.degree, cap);
}

void slab_quot_params(QuotParams& qp, size_t n, int lqd, int r) {
  const SlabParams sp = slab_params(n, lqd, r, qp.alpha_pows);
  qp.shift = sp.shift;
  qp.zh_even = sp.zh_even;
  qp.zh_odd = sp.zh_odd;
  qp.zh_even_inv = sp.zh_even_inv;
  qp.zh_odd_inv = sp.zh_odd_inv;
  qp.wn_inv = sp.wn_inv;
}

ChipProgram chip_compile(const uint8_t* air, size_t air_len, const uint8_t* lookups,
                         size_t lookups_len) {
  const char* no_lookups =
      "chip program: no interactions -- a chip without lookups is an AIR alone (bfz_air_*)";
  if (!lookups || lookups_len == 0) throw std::runtime_error(no_lookups);
  if (lookups_len >= 16) {  // a well-formed header that declares none: the same message
    uint32_t magic, n;
    std::memcpy(&magic, lookups, 4);
    std::memcpy(&n, lookups + 12, 4);
    if (magic == LKP_MAGIC && n == 0) throw std::runtime_error(no_lookups);
  }
  ChipProgram p;
  p.lk = lookups_compile(lookups, lookups_len);
  p.has_air = air != nullptr && air_len != 0;
  if (p.has_air) {
    // At the default cap the AIR path's own cap refuses first, in its own words, as it always
    // has.  A raised chip cap stands alone: air_compile refuses above it before it compiles
    // anything, and that refusal is reworded into the chip's.
    const int cap = chip_max_degree();
    if (cap == AIR_DEFAULT_MAX_DEGREE) {
      p.air = air_compile(air, air_len);
    } else {
      try {
        p.air = air_compile(air, air_len, cap);
      } catch (const AirDegreeError& e) {
        chip_degree_throw(e.degree, cap);
      }
    }
    chip_cap_or_throw(p);
    if (p.air.width != p.lk.main_w)
      throw std::runtime_error("chip program: the AIR's width " + std::to_string(p.air.width) +
                               " is not the interactions' main width " +
                               std::to_string(p.lk.main_w));
  }
  return p;
}

namespace {
struct HostFail {  // FirstFailAcc continued after the AIR's constraints
  int n, first = -1;
  void emit_ext(const EF& c) {
    if (!ef_is_zero(c) && first < 0) first = n;
    n++;
  }
};
EF ef_at(const uint32_t* w) {
  EF e;
  std::memcpy(e.c, w, 16);
  return e;
}

// The permutation constraints of one row into acc (batches + 3 emit_ext calls), in
// perm_constraints' order.  m / pr: the row's main and preprocessed words; pl / pn: the local and
// next permutation rows (4 * perm_width words each).
template <class Acc>
void host_perm_constraints(const ChipProgram& p, const uint32_t* m, const uint32_t* pr,
                           const uint32_t* pl, const uint32_t* pn, const PermChallenges& ch,
                           const EF& cumsum, bool is_first, bool is_last, Acc& acc) {
  const uint32_t* list = p.lk.list.data();
  const int nb = p.lk.batches(), ni = p.lk.n;
  EF sum_l = ef_zero(), sum_n = ef_zero();
  size_t at = LKP_HEAD;
  for (int b = 0; b < nb; b++) {
    EF d0, d1;
    uint32_t m0, m1;
    host_interaction(list, at, m, pr, ch, d0, m0);
    const EF v = ef_at(pl + 4 * b);
    if (2 * b + 1 < ni) {
      host_interaction(list, at, m, pr, ch, d1, m1);
      acc.emit_ext(ef_sub(ef_mul(ef_mul(d0, d1), v),
                          ef_add(ef_mul_base(d1, m0), ef_mul_base(d0, m1))));
    } else {
      acc.emit_ext(ef_sub(ef_mul(d0, v), ef_base(m0)));
    }
    sum_l = ef_add(sum_l, v);
    sum_n = ef_add(sum_n, ef_at(pn + 4 * b));
  }
  const EF phi_l = ef_at(pl + 4 * nb), phi_n = ef_at(pn + 4 * nb);
  acc.emit_ext(is_first ? ef_sub(phi_l, sum_l) : ef_zero());
  acc.emit_ext(is_last ? ef_zero() : ef_sub(ef_sub(phi_n, phi_l), sum_n));
  acc.emit_ext(is_last ? ef_sub(phi_l, cumsum) : ef_zero());
}

void chip_dims_or_throw(const ChipProgram& p, const uint32_t* prep, size_t h) {
  if (h < 1 || (h & (h - 1)) || h > ((size_t)1 << 23))
    throw std::runtime_error("chip program: height not a power of two in [1, 2^23]");
  if (p.lk.prep_w && !prep) throw std::runtime_error("chip program: the chip has preprocessed columns");
}
}  // namespace

void chip_check_host(const ChipProgram& p, const uint32_t* main, const uint32_t* prep,
                     const uint32_t* perm, size_t h, const PermChallenges& ch, const EF& cumsum,
                     ChipCheck& out, int32_t* per_row) {
  chip_dims_or_throw(p, prep, h);
  const int mw = p.lk.main_w, pw = p.lk.prep_w;
  const size_t w = 4 * (size_t)p.perm_width();
  out = ChipCheck{};
  out.height = h;
  out.num_constraints = p.num_constraints();
  out.num_batches = p.lk.batches();
  out.cumsum = cumsum;
  for (size_t i = 0; i < h; i++) {
    const size_t nx = (i + 1) & (h - 1);
    const bool is_first = i == 0, is_last = i == h - 1;
    const uint32_t* m = main + i * (size_t)mw;
    int idx = p.has_air ? air_first_fail(p.air, m, main + nx * (size_t)mw, is_first, is_last) : -1;
    if (idx < 0) {
      HostFail acc{p.air_constraints()};
      host_perm_constraints(p, m, pw ? prep + i * (size_t)pw : nullptr, perm + i * w, perm + nx * w,
                            ch, cumsum, is_first, is_last, acc);
      idx = acc.first;
    }
    if (per_row) per_row[i] = idx;
    if (idx >= 0 && out.failing_rows++ == 0) {
      out.first_row = (int64_t)i;
      out.first_constraint = idx;
    }
  }
}

void chip_profile_host(const ChipProgram& p, const uint32_t* main, const uint32_t* prep,
                       const uint32_t* perm, size_t h, const PermChallenges& ch, const EF& cumsum,
                       ChipCheck& out, uint64_t* counts, int64_t* first_rows) {
  chip_dims_or_throw(p, prep, h);
  const int mw = p.lk.main_w, pw = p.lk.prep_w, K = p.num_constraints();
  const size_t w = 4 * (size_t)p.perm_width();
  out = ChipCheck{};
  out.height = h;
  out.num_constraints = K;
  out.num_batches = p.lk.batches();
  out.cumsum = cumsum;
  std::fill(counts, counts + K, (uint64_t)0);
  std::fill(first_rows, first_rows + K, (int64_t)-1);
  for (size_t i = 0; i < h; i++) {
    const size_t nx = (i + 1) & (h - 1);
    const bool is_first = i == 0, is_last = i == h - 1;
    const uint32_t* m = main + i * (size_t)mw;
    ProfileAcc acc{counts, first_rows, (int64_t)i};  // every constraint of the row, failed or not
    if (p.has_air)
      air_run<BaseOps>(p.air, m, main + nx * (size_t)mw, is_first ? ONE : 0u, is_last ? ONE : 0u,
                       is_last ? 0u : ONE, acc);
    host_perm_constraints(p, m, pw ? prep + i * (size_t)pw : nullptr, perm + i * w, perm + nx * w, ch,
                          cumsum, is_first, is_last, acc);
    if (acc.first >= 0 && out.failing_rows++ == 0) {
      out.first_row = (int64_t)i;
      out.first_constraint = acc.first;
    }
  }
}

}  // namespace bfz
