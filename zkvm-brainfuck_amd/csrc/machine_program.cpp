// Machines of caller-defined chips on the host (machine_program.h): the value, its transcript
// head and the permutation constraints at zeta.
#include "machine_program.h"

#include <algorithm>
#include <cstring>
#include <set>
#include <stdexcept>

namespace bfz {

using namespace kb;

void machine_commit_prep(MachineProgram& m, const MachineChipIn* in);  // machine_program.hip

std::unique_ptr<MachineProgram> machine_create(const MachineChipIn* in, size_t n, bool with_traces,
                                               const uint32_t* root) {
  if (!in || n == 0) throw std::runtime_error("machine: no chips");
  if (n > (size_t)MACHINE_MAX_CHIPS)
    throw std::runtime_error("machine: " + std::to_string(n) + " chips, at most " +
                             std::to_string(MACHINE_MAX_CHIPS));
  auto m = std::make_unique<MachineProgram>();
  std::set<std::string> seen;
  m->chips.resize(n);
  for (size_t i = 0; i < n; i++) {
    MachineChip& c = m->chips[i];
    if (!in[i].name || in[i].name_len == 0) throw std::runtime_error("machine: a chip without a name");
    c.name.assign((const char*)in[i].name, in[i].name_len);
    if (!seen.insert(c.name).second) throw std::runtime_error("machine: duplicate chip name " + c.name);
    try {
      c.p = chip_compile(in[i].air, in[i].air_len, in[i].lookups, in[i].lookups_len);
    } catch (const std::exception& e) {
      throw std::runtime_error("machine: chip " + c.name + ": " + e.what());
    }
    c.local_only = c.p.has_air;
    if (c.p.has_air)
      for (size_t pc = 0; pc < c.p.air.code.size(); pc++) {
        const uint32_t op = c.p.air.code[pc] & 0xff;
        if (op == AIR_NEXT) c.local_only = false;
        if (op == AIR_CONST) pc++;  // its Montgomery word follows
      }
    if (c.p.lk.prep_w) {
      const size_t h = in[i].prep_height;
      if (h < 1 || (h & (h - 1)) || h > ((size_t)1 << 23))
        throw std::runtime_error("machine: preprocessed height not a power of two in [1, 2^23] for " +
                                 c.name);
      if (with_traces && !in[i].prep)
        throw std::runtime_error("machine: chip " + c.name + " has preprocessed columns and no trace");
      c.prep_height = h;
      m->prep_chips.push_back((int)i);
    }
  }
  // vk.chip_information: the preprocessed matrices sorted by (Reverse(height), name)
  std::sort(m->prep_chips.begin(), m->prep_chips.end(), [&](int a, int b) {
    const MachineChip &x = m->chips[a], &y = m->chips[b];
    return x.prep_height != y.prep_height ? x.prep_height > y.prep_height : x.name < y.name;
  });
  for (size_t k = 0; k < m->prep_chips.size(); k++) m->chips[m->prep_chips[k]].prep_index = (int)k;
  m->has_prep = !m->prep_chips.empty();
  if (with_traces) {
    machine_commit_prep(*m, in);
    m->can_prove = true;
  } else if (m->has_prep) {
    if (!root) throw std::runtime_error("machine: preprocessed columns need a root or traces");
    for (int i = 0; i < 8; i++)
      if (root[i] >= P) throw std::runtime_error("machine: non-canonical root word");
    std::memcpy(m->prep_root, root, 32);
  }
  return m;
}

void machine_observe(const MachineProgram& m, Challenger& ch) {
  ch.observe_digest(m.prep_root);  // eight zero words without preprocessed columns
  for (int i = 0; i < 7; i++) ch.observe(0);
}

namespace {
// One VCOL at list[at] over EF rows; at advances past it.
EF ef_vcol(const uint32_t* list, size_t& at, const EF* m, const EF* pr) {
  EF r = ef_base(list[at]);
  const uint32_t nt = list[at + 1];
  at += 2;
  for (uint32_t i = 0; i < nt; i++, at += 2) {
    const uint32_t sc = list[at + 1];
    r = ef_add(r, ef_mul_base((sc >> 16 ? pr : m)[sc & 0xffff], list[at]));
  }
  return r;
}
// The interaction at list[at]: its denominator and signed multiplicity at zeta.
void ef_interaction(const uint32_t* list, size_t& at, const EF* m, const EF* pr, const EF& alpha,
                    const EF* beta_pows, EF& den, EF& mult) {
  const uint32_t head = list[at], nv = head & 0xff;
  den = ef_add_base(alpha, list[at + 1]);
  at += 2;
  const EF mu = ef_vcol(list, at, m, pr);
  mult = (head >> 8) & 1 ? mu : ef_sub(ef_zero(), mu);
  for (uint32_t v = 0; v < nv; v++)
    den = ef_add(den, ef_mul(beta_pows[v + 1], ef_vcol(list, at, m, pr)));
}
}  // namespace

void chip_perm_eval_ef(const LookupProgram& lk, const EF* main_l, const EF* prep_l, const EF* perm_l,
                       const EF* perm_n, const EF& alpha, const EF* beta_pows, const EF& cumsum,
                       const EF& first, const EF& last, const EF& trans, EF* out) {
  const uint32_t* list = lk.list.data();
  const int ni = lk.n, nb = lk.batches();
  EF sum_l = ef_zero(), sum_n = ef_zero();
  size_t at = LKP_HEAD;
  for (int b = 0; b < nb; b++) {
    EF d0, m0;
    ef_interaction(list, at, main_l, prep_l, alpha, beta_pows, d0, m0);
    if (2 * b + 1 < ni) {
      EF d1, m1;
      ef_interaction(list, at, main_l, prep_l, alpha, beta_pows, d1, m1);
      out[b] = ef_sub(ef_mul(ef_mul(d0, d1), perm_l[b]), ef_add(ef_mul(d1, m0), ef_mul(d0, m1)));
    } else {
      out[b] = ef_sub(ef_mul(d0, perm_l[b]), m0);
    }
    sum_l = ef_add(sum_l, perm_l[b]);
    sum_n = ef_add(sum_n, perm_n[b]);
  }
  out[nb] = ef_mul(ef_sub(perm_l[nb], sum_l), first);
  out[nb + 1] = ef_mul(ef_sub(ef_sub(perm_n[nb], perm_l[nb]), sum_n), trans);
  out[nb + 2] = ef_mul(ef_sub(perm_l[nb], cumsum), last);
}

}  // namespace bfz
