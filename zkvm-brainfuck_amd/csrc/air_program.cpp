// Constraint programs on the host (air_program.h): validation, shape, the compile step, the two
// host evaluators and the exporter of the built-in chips' AIRs.
#include "air_program.h"

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>

#include "machine.h"
#include "uni_stark.h"

namespace bfz {

namespace {
[[noreturn]] void bad(const std::string& what, size_t word) {
  throw std::runtime_error("air program: " + what + " (word " + std::to_string(word) + ")");
}
uint32_t word_at(const uint8_t* p, size_t i) {  // the bytes need not be aligned
  uint32_t v;
  std::memcpy(&v, p + 4 * i, 4);
  return v;
}
bool is_arith(uint32_t op) { return op >= AIR_ADD && op <= AIR_NEG; }
constexpr int DEG_CAP = 1 << 20;  // a product chain must not overflow the degree

struct Node {
  uint32_t op, a, b;
};
}  // namespace

AirProgram air_compile(const uint8_t* prog, size_t len) {
  if (!prog || len < 16) bad("shorter than its header", 0);
  if (word_at(prog, 0) != AIR_MAGIC) bad("bad magic, expected \"BFA1\"", 0);
  const uint32_t width = word_at(prog, 1), nn = word_at(prog, 2), K = word_at(prog, 3);
  if (width < 1 || width > BFZ_AIR_MAX_WIDTH) bad("width not in [1, " + std::to_string(BFZ_AIR_MAX_WIDTH) + "]", 1);
  if (nn < 1 || nn > BFZ_AIR_MAX_NODES) bad("node count not in [1, " + std::to_string(BFZ_AIR_MAX_NODES) + "]", 2);
  if (K < 1) bad("no constraints", 3);
  if (K > BFZ_AIR_MAX_CONSTRAINTS) bad("more than " + std::to_string(BFZ_AIR_MAX_CONSTRAINTS) + " constraints", 3);
  const size_t words = 4 + 3 * (size_t)nn + K;
  if (len != 4 * words)
    bad("length is " + std::to_string(len) + " bytes, the header says " + std::to_string(4 * words),
        len < 4 * words ? len / 4 : words);

  // ---- nodes: op codes, operands, degrees (DegOps' rules, quotient.hip)
  std::vector<Node> nodes(nn);
  std::vector<int> deg(nn);
  for (uint32_t i = 0; i < nn; i++) {
    const size_t at = 4 + 3 * (size_t)i;
    Node& nd = nodes[i];
    nd = Node{word_at(prog, at), word_at(prog, at + 1), word_at(prog, at + 2)};
    switch (nd.op) {
      case AIR_CONST:
        if (nd.a >= kb::P) bad("constant not below p", at + 1);
        if (nd.b) bad("unused operand not 0", at + 2);
        deg[i] = 0;
        break;
      case AIR_LOCAL:
      case AIR_NEXT:
        if (nd.a >= width) bad("column not below the width", at + 1);
        if (nd.b) bad("unused operand not 0", at + 2);
        deg[i] = 1;
        break;
      case AIR_FIRST:
      case AIR_LAST:
      case AIR_TRANS:
        if (nd.a) bad("unused operand not 0", at + 1);
        if (nd.b) bad("unused operand not 0", at + 2);
        deg[i] = nd.op == AIR_TRANS ? 0 : 1;
        break;
      case AIR_ADD:
      case AIR_SUB:
      case AIR_MUL:
        if (nd.a >= i) bad("operand is not an earlier node", at + 1);
        if (nd.b >= i) bad("operand is not an earlier node", at + 2);
        deg[i] = nd.op == AIR_MUL ? std::min(deg[nd.a] + deg[nd.b], DEG_CAP) : std::max(deg[nd.a], deg[nd.b]);
        break;
      case AIR_NEG:
        if (nd.a >= i) bad("operand is not an earlier node", at + 1);
        if (nd.b) bad("unused operand not 0", at + 2);
        deg[i] = deg[nd.a];
        break;
      default: bad("unknown op " + std::to_string(nd.op), at);
    }
  }
  std::vector<uint32_t> cons(K);
  int degree = 0;
  for (uint32_t k = 0; k < K; k++) {
    cons[k] = word_at(prog, 4 + 3 * (size_t)nn + k);
    if (cons[k] >= nn) bad("constraint is not a node", 4 + 3 * (size_t)nn + k);
    degree = std::max(degree, deg[cons[k]]);
  }
  int lqd = 0;  // log2_ceil(degree - 1), at least 0 (uni_air_shape)
  while ((1 << lqd) < degree - 1) lqd++;
  if (lqd > 1) throw std::runtime_error("uni_stark: constraint degree above 3 is not supported");

  // ---- compile.  uses[i]: reads of node i by reachable nodes and by constraints still ahead.
  std::vector<uint32_t> uses(nn, 0);
  std::vector<char> reach(nn, 0);
  for (uint32_t k = 0; k < K; k++) {
    reach[cons[k]] = 1;
    uses[cons[k]]++;
  }
  for (uint32_t i = nn; i-- > 0;) {
    if (!reach[i] || !is_arith(nodes[i].op)) continue;
    reach[nodes[i].a] = 1;
    uses[nodes[i].a]++;
    if (nodes[i].op != AIR_NEG) {
      reach[nodes[i].b] = 1;
      uses[nodes[i].b]++;
    }
  }

  AirProgram out;
  out.width = (int)width;
  out.num_nodes = (int)nn;
  out.num_constraints = (int)K;
  out.degree = degree;
  out.log_quotient_degree = lqd;
  std::vector<int> slot_of(nn, -1);
  std::vector<char> busy;  // grows past BFZ_AIR_MAX_LIVE so that a refusal can name the need
  auto take = [&]() {
    size_t s = 0;
    while (s < busy.size() && busy[s]) s++;
    if (s == busy.size()) busy.push_back(0);
    busy[s] = 1;
    return (int)s;
  };
  auto ins = [&](uint32_t op, int d, uint32_t a, uint32_t b) {
    out.code.push_back(air_ins(op, (uint32_t)d & 0xff, a & 0xff, b & 0xff));
    out.instructions++;
  };
  auto need = [&](uint32_t i) {  // a leaf is loaded at its first use; an earlier node has a slot
    if (slot_of[i] >= 0) return;
    const int s = slot_of[i] = take();
    ins(nodes[i].op, s, nodes[i].op == AIR_CONST ? 0 : nodes[i].a, 0);
    if (nodes[i].op == AIR_CONST) out.code.push_back(nodes[i].a);
  };
  auto done = [&](uint32_t i) {  // one read of node i is over
    if (--uses[i] == 0) {
      busy[slot_of[i]] = 0;
      slot_of[i] = -1;
    }
  };
  uint32_t k = 0;
  auto emit_ready = [&](uint32_t upto) {  // constraints whose node is a leaf or computed
    while (k < K && (!is_arith(nodes[cons[k]].op) || cons[k] < upto)) {
      need(cons[k]);
      ins(AIR_EMIT, 0, (uint32_t)slot_of[cons[k]], 0);
      done(cons[k]);
      k++;
    }
  };
  emit_ready(0);
  for (uint32_t i = 0; i < nn; i++) {
    if (!reach[i] || !is_arith(nodes[i].op)) continue;
    const Node& nd = nodes[i];
    const bool two = nd.op != AIR_NEG;
    need(nd.a);
    if (two) need(nd.b);
    const int sa = slot_of[nd.a], sb = two ? slot_of[nd.b] : 0;
    done(nd.a);
    if (two) done(nd.b);
    slot_of[i] = take();  // may be an operand's slot: the interpreters read before they write
    ins(nd.op, slot_of[i], (uint32_t)sa, (uint32_t)sb);
    emit_ready(i + 1);
  }
  out.live_values = (int)busy.size();
  if (out.live_values > BFZ_AIR_MAX_LIVE)
    throw std::runtime_error("air program: needs " + std::to_string(out.live_values) +
                             " simultaneously live values, the limit is " +
                             std::to_string(BFZ_AIR_MAX_LIVE));
  return out;
}

// ------------------------------------------------------------------------ host evaluators
namespace {
struct FirstFailSink {
  int n = 0, first = -1;
  bool emit(uint32_t c) {
    if (c != 0) {
      first = n;
      return false;
    }
    n++;
    return true;
  }
};
struct AllSink {
  EF* out;
  int n = 0;
  bool emit(const EF& c) {
    out[n++] = c;
    return true;
  }
};
}  // namespace

int air_first_fail(const AirProgram& p, const uint32_t* L, const uint32_t* N, bool is_first,
                   bool is_last) {
  FirstFailSink sink;
  air_run<BaseOps>(p, L, N, is_first ? kb::ONE : 0u, is_last ? kb::ONE : 0u, is_last ? 0u : kb::ONE,
                   sink);
  return sink.first;
}

void air_eval_ef(const AirProgram& p, const EF* L, const EF* N, const EF& first, const EF& last,
                 const EF& trans, EF* out) {
  AllSink sink{out};
  air_run<ExtOps>(p, L, N, first, last, trans, sink);
}

// ------------------------------------------------------------------------ exporter
namespace {
struct Recorder {
  std::vector<uint32_t> words, cons;  // (op, a, b) triples; constraint nodes
  uint32_t push(uint32_t op, uint32_t a, uint32_t b) {
    words.insert(words.end(), {op, a, b});
    return (uint32_t)(words.size() / 3 - 1);
  }
};
thread_local Recorder* g_rec = nullptr;

// Air<Ops, Acc> over node indices: every operation appends a node (as DegOps runs it over degrees).
struct RecOps {
  using T = uint32_t;
  static T add(T a, T b) { return g_rec->push(AIR_ADD, a, b); }
  static T sub(T a, T b) { return g_rec->push(AIR_SUB, a, b); }
  static T mul(T a, T b) { return g_rec->push(AIR_MUL, a, b); }
  static T neg(T a) { return g_rec->push(AIR_NEG, a, 0); }
  static T cst(uint32_t mont) { return g_rec->push(AIR_CONST, mont, 0); }
};
struct RecAcc {
  void emit(uint32_t node) { g_rec->cons.push_back(node); }
};

template <int CHIP>
void record_chip(Recorder& r, int w) {
  std::vector<uint32_t> L(w), N(w);
  for (int c = 0; c < w; c++) L[c] = r.push(AIR_LOCAL, (uint32_t)c, 0);
  for (int c = 0; c < w; c++) N[c] = r.push(AIR_NEXT, (uint32_t)c, 0);
  const uint32_t first = r.push(AIR_FIRST, 0, 0), last = r.push(AIR_LAST, 0, 0),
                 trans = r.push(AIR_TRANS, 0, 0);
  RecAcc acc;
  g_rec = &r;
  Air<RecOps, RecAcc> air{L.data(), N.data(), L.data(), N.data(), first, last, trans, acc};
  air.template eval_air<CHIP>();
  g_rec = nullptr;
}
}  // namespace

std::vector<uint8_t> air_export(int chip) {
  uni_air_shape_or_throw(chip, nullptr, nullptr, nullptr);
  const int w = CHIP_INFO[chip].main_w;
  Recorder r;
  switch (chip) {
    case CHIP_CPU: record_chip<CHIP_CPU>(r, w); break;
    case CHIP_ADDSUB: record_chip<CHIP_ADDSUB>(r, w); break;
    case CHIP_JUMP: record_chip<CHIP_JUMP>(r, w); break;
    case CHIP_MEMINSTRS: record_chip<CHIP_MEMINSTRS>(r, w); break;
    case CHIP_IO: record_chip<CHIP_IO>(r, w); break;
  }
  std::vector<uint32_t> words = {AIR_MAGIC, (uint32_t)w, (uint32_t)(r.words.size() / 3),
                                 (uint32_t)r.cons.size()};
  words.insert(words.end(), r.words.begin(), r.words.end());
  words.insert(words.end(), r.cons.begin(), r.cons.end());
  std::vector<uint8_t> out(4 * words.size());
  std::memcpy(out.data(), words.data(), out.size());
  return out;
}

}  // namespace bfz
