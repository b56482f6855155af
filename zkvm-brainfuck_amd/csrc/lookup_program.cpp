// Interaction programs on the host (lookup_program.h): validation and the compile step, the
// exporter of the built-in chips' interactions and the single-threaded permutation trace.
#include "lookup_program.h"

#include <cstring>
#include <stdexcept>
#include <string>

#include "machine.h"

namespace bfz {

using namespace kb;

namespace {
[[noreturn]] void bad(const std::string& what, size_t word) {
  throw std::runtime_error("lookup program: " + what + " (word " + std::to_string(word) + ")");
}

struct Reader {  // the program's words, every read checked against its length
  const uint8_t* p;
  size_t words, at = 0;
  uint32_t next() {
    if (at >= words) bad("ends inside an interaction", words);
    uint32_t v;
    std::memcpy(&v, p + 4 * at++, 4);  // the bytes need not be aligned
    return v;
  }
};

void compile_vcol(Reader& r, const LookupProgram& p, std::vector<uint32_t>& list) {
  const uint32_t c = r.next();
  if (c >= P) bad("constant not below p", r.at - 1);
  const uint32_t nt = r.next();
  if (nt > LKP_MAX_TERMS) bad("more than " + std::to_string(LKP_MAX_TERMS) + " terms", r.at - 1);
  list.insert(list.end(), {c, nt});
  for (uint32_t i = 0; i < nt; i++) {
    const uint32_t src = r.next();
    if (src > S_PREP) bad("source is neither 0 (main) nor 1 (prep)", r.at - 1);
    const uint32_t col = r.next();
    if (col >= (uint32_t)(src == S_PREP ? p.prep_w : p.main_w))
      bad("column not below the width", r.at - 1);
    const uint32_t w = r.next();
    if (w >= P) bad("weight not below p", r.at - 1);
    list.insert(list.end(), {w, src << 16 | col});
  }
}
}  // namespace

LookupProgram lookups_compile(const uint8_t* prog, size_t len) {
  if (!prog || len < 16) bad("shorter than its header", 0);
  if (len % 4) bad("length is not a multiple of 4 bytes", len / 4);
  Reader r{prog, len / 4};
  if (r.next() != LKP_MAGIC) bad("bad magic, expected \"BFL1\"", 0);
  LookupProgram p;
  const uint32_t mw = r.next(), pw = r.next(), n = r.next();
  if (mw < 1 || mw > BFZ_AIR_MAX_WIDTH)
    bad("main width not in [1, " + std::to_string(BFZ_AIR_MAX_WIDTH) + "]", 1);
  if (pw > BFZ_AIR_MAX_WIDTH) bad("prep width above " + std::to_string(BFZ_AIR_MAX_WIDTH), 2);
  if (n < 1) bad("no interactions", 3);
  if (n > BFZ_LOOKUPS_MAX) bad("more than " + std::to_string(BFZ_LOOKUPS_MAX) + " interactions", 3);
  p.main_w = (int)mw;
  p.prep_w = (int)pw;
  p.n = (int)n;
  p.list.assign(LKP_HEAD, 0);
  p.list[0] = n;
  for (uint32_t j = 0; j < n; j++) {
    if (j % 2 == 0) p.list[1 + j / 2] = (uint32_t)p.list.size();
    const uint32_t kind = r.next();
    if (kind >= P) bad("kind not below p", r.at - 1);
    const uint32_t send = r.next();
    if (send > 1) bad("direction is neither 1 (send) nor 0 (receive)", r.at - 1);
    if (send && p.receives) bad("a send after a receive: the chain is sends, then receives", r.at - 1);
    (send ? p.sends : p.receives)++;
    const uint32_t nv = r.next();
    if (nv > LKP_MAX_VALUES) bad("more than " + std::to_string(LKP_MAX_VALUES) + " values", r.at - 1);
    p.list.insert(p.list.end(), {nv | send << 8, to_mont(kind)});
    for (uint32_t v = 0; v <= nv; v++) compile_vcol(r, p, p.list);  // mult, then the values
  }
  if (r.at != r.words) bad("trailing words after the last interaction", r.at);
  return p;
}

// ------------------------------------------------------------------------ exporter
std::vector<uint8_t> lookups_export(int chip) {
  static const ChipLookups* const all[NUM_CHIPS] = {
      &CPU_LOOKUPS,    &PROGRAM_LOOKUPS, &ADDSUB_LOOKUPS,    &JUMP_LOOKUPS,
      &MEMORY_LOOKUPS, &BYTE_LOOKUPS,    &MEMINSTRS_LOOKUPS, &IO_LOOKUPS};
  if (chip < 0 || chip >= NUM_CHIPS) throw std::runtime_error("bad chip index");
  const ChipLookups& cl = *all[chip];
  std::vector<uint32_t> w = {LKP_MAGIC, (uint32_t)CHIP_INFO[chip].main_w,
                             (uint32_t)CHIP_INFO[chip].prep_w, (uint32_t)cl.n};
  auto vcol = [&](const VCol& v) {
    w.insert(w.end(), {to_mont(v.c), (uint32_t)v.n});
    for (int i = 0; i < v.n; i++)
      w.insert(w.end(), {(uint32_t)v.t[i].src, (uint32_t)v.t[i].col, to_mont(v.t[i].w)});
  };
  for (int j = 0; j < cl.n; j++) {
    const Lookup& lk = cl.l[j];
    w.insert(w.end(), {(uint32_t)lk.kind, lk.send ? 1u : 0u, (uint32_t)lk.nvals});
    vcol(lk.mult);
    for (int v = 0; v < lk.nvals; v++) vcol(lk.vals[v]);
  }
  std::vector<uint8_t> out(4 * w.size());
  std::memcpy(out.data(), w.data(), out.size());
  return out;
}

// ------------------------------------------------------------------------ host trace
namespace {
// One VCOL at list[at] over a row; at advances past it.
uint32_t host_vcol(const uint32_t* list, size_t& at, const uint32_t* m, const uint32_t* pr) {
  uint32_t r = list[at];
  const uint32_t nt = list[at + 1];
  at += 2;
  for (uint32_t i = 0; i < nt; i++, at += 2) {
    const uint32_t sc = list[at + 1];
    r = madd(r, mmul(list[at], (sc >> 16 ? pr : m)[sc & 0xffff]));
  }
  return r;
}
}  // namespace
// The interaction at list[at]: its denominator and signed multiplicity.
void host_interaction(const uint32_t* list, size_t& at, const uint32_t* m, const uint32_t* pr,
                      const PermChallenges& ch, EF& den, uint32_t& mult) {
  const uint32_t head = list[at], nv = head & 0xff;
  den = ef_add_base(ch.alpha, list[at + 1]);
  at += 2;
  const uint32_t mu = host_vcol(list, at, m, pr);
  mult = (head >> 8) & 1 ? mu : mneg(mu);
  for (uint32_t v = 0; v < nv; v++)
    den = ef_add(den, ef_mul_base(ch.beta_pows[v + 1], host_vcol(list, at, m, pr)));
}

void lookups_perm_trace_host(const LookupProgram& p, const uint32_t* main, const uint32_t* prep,
                             size_t h, const PermChallenges& ch, uint32_t* out, EF* cumsum) {
  const uint32_t* list = p.list.data();
  const int nb = p.batches();
  const size_t w = 4 * (size_t)p.perm_width();
  EF phi = ef_zero();
  for (size_t r = 0; r < h; r++) {
    const uint32_t* m = main + r * (size_t)p.main_w;
    const uint32_t* pr = prep ? prep + r * (size_t)p.prep_w : nullptr;
    size_t at = LKP_HEAD;
    for (int b = 0; b < nb; b++) {
      EF d0, v;
      uint32_t m0;
      host_interaction(list, at, m, pr, ch, d0, m0);
      v = ef_mul_base(ef_inv(d0), m0);
      if (2 * b + 1 < p.n) {
        EF d1;
        uint32_t m1;
        host_interaction(list, at, m, pr, ch, d1, m1);
        v = ef_add(v, ef_mul_base(ef_inv(d1), m1));
      }
      if (out) std::memcpy(out + r * w + 4 * (size_t)b, v.c, 16);
      phi = ef_add(phi, v);
    }
    if (out) std::memcpy(out + r * w + 4 * (size_t)nb, phi.c, 16);
  }
  *cumsum = phi;
}

}  // namespace bfz
