// Machines of caller-defined chips on the host (machine_program.h): the value, its transcript
// head and the permutation constraints at zeta.
#include "machine_program.h"

#include <algorithm>
#include <cstring>
#include <set>
#include <stdexcept>

#include "uni_stark.h"

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
    for (int i : m->prep_chips) {
      const MachineChip& c = m->chips[i];
      m->chips[i].prep_host.assign(in[i].prep, in[i].prep + c.prep_height * (size_t)c.p.lk.prep_w);
    }
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

std::vector<int> machine_trace_order(const MachineProgram& m, const int* chips,
                                     const uint32_t* const* traces, const size_t* heights, size_t n,
                                     bool same_height_limit) {
  if (!chips || !traces || !heights || n == 0) throw std::runtime_error("machine: no traces");
  if (n > m.chips.size()) throw std::runtime_error("machine: more traces than chips");
  std::vector<bool> seen(m.chips.size(), false);
  for (size_t i = 0; i < n; i++) {
    const int c = chips[i];
    if (c < 0 || (size_t)c >= m.chips.size() || seen[c])
      throw std::runtime_error("machine: bad or repeated chip index");
    seen[c] = true;
    const MachineChip& ch = m.chips[c];
    const size_t h = heights[i];
    if (!traces[i]) throw std::runtime_error("machine: null trace for " + ch.name);
    if (h < 1 || (h & (h - 1)) || h > ((size_t)1 << 23))
      throw std::runtime_error("machine: height not a power of two in [1, 2^23] for " + ch.name);
    if (ch.p.lk.prep_w && h != ch.prep_height)
      throw std::runtime_error("machine: chip " + ch.name + " is not at its preprocessed height");
  }
  for (int pc : m.prep_chips)
    if (!seen[pc])
      throw std::runtime_error("machine: chip " + m.chips[pc].name +
                               " has preprocessed columns and must be included");
  if (same_height_limit)  // the machine prover's own limit (the commit has none, merkle.hip)
    for (size_t i = 0; i < n; i++) {
      size_t same = 0;
      for (size_t j = 0; j < n; j++) same += heights[j] == heights[i];
      if (same > MACHINE_MAX_SAME_HEIGHT)
        throw std::runtime_error("machine: " + std::to_string(same) + " chips of height " +
                                 std::to_string(heights[i]) + ", a proof takes at most " +
                                 std::to_string(MACHINE_MAX_SAME_HEIGHT) + " of one height");
    }
  std::vector<int> order(n);
  for (size_t i = 0; i < n; i++) order[i] = (int)i;
  std::sort(order.begin(), order.end(), [&](int a, int b) {  // (Reverse(height), name)
    if (heights[a] != heights[b]) return heights[a] > heights[b];
    return m.chips[chips[a]].name < m.chips[chips[b]].name;
  });
  return order;
}

MachineCheck machine_check_device(const MachineProgram& m, const int* chips,
                                  const uint32_t* const* traces, const size_t* heights, size_t n,
                                  Challenger& ch);  // machine_program.hip

MachineCheck machine_check(const MachineProgram& m, const int* chips, const uint32_t* const* traces,
                           const size_t* heights, size_t n, Challenger& ch, bool on_device) {
  if (!m.can_prove)
    throw std::runtime_error("machine: a verifier-only machine holds no preprocessed traces and "
                             "cannot check constraints");
  if (on_device) return machine_check_device(m, chips, traces, heights, n, ch);
  const std::vector<int> order = machine_trace_order(m, chips, traces, heights, n, false);
  for (int i : order) {  // the device path's refusal, in its (commit) order
    const MachineChip& c = m.chips[chips[i]];
    for (size_t j = 0; j < heights[i] * (size_t)c.p.lk.main_w; j++)
      if (traces[i][j] >= P) uni_noncanonical_throw(c.name.c_str());
  }
  MachineCheck out;
  out.alpha = ch.sample_ef();  // machine.rs:300-303
  out.beta = ch.sample_ef();
  PermChallenges pch;
  pch.alpha = out.alpha;
  pch.beta_pows[0] = ef_one();
  for (int j = 1; j < 8; j++) pch.beta_pows[j] = ef_mul(pch.beta_pows[j - 1], out.beta);
  size_t ktot = 0;
  for (size_t i = 0; i < n; i++) ktot += (size_t)m.chips[chips[i]].p.num_constraints();
  out.chips.resize(n);
  out.counts.resize(ktot);
  out.first_rows.resize(ktot);
  out.cumsum = ef_zero();
  out.ok = true;
  std::vector<uint32_t> perm;
  size_t k0 = 0;
  for (size_t i = 0; i < n; i++) {
    const MachineChip& c = m.chips[chips[i]];
    const uint32_t* prep = c.p.lk.prep_w ? c.prep_host.data() : nullptr;
    perm.resize(heights[i] * 4 * (size_t)c.p.perm_width());
    EF cs;
    lookups_perm_trace_host(c.p.lk, traces[i], prep, heights[i], pch, perm.data(), &cs);
    chip_profile_host(c.p, traces[i], prep, perm.data(), heights[i], pch, cs, out.chips[i],
                      out.counts.data() + k0, out.first_rows.data() + k0);
    out.chips[i].chip = chips[i];
    out.cumsum = ef_add(out.cumsum, cs);
    out.ok = out.ok && out.chips[i].failing_rows == 0;
    k0 += (size_t)c.p.num_constraints();
  }
  out.ok = out.ok && ef_is_zero(out.cumsum);
  return out;
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
