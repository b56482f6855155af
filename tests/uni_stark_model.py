"""A small pure-Python model of the per-chip uni-STARK protocol (bfz_uni_prove / bfz_uni_verify):
TEST INFRASTRUCTURE ONLY, the independent yardstick of tests/test_uni_stark*.py.

It shares no code with the library.  KoalaBear and EF = F[x]/(x^4 - 3) arithmetic, the duplex
challenger and the Lagrange evaluation are written out here over canonical integers; the only
outside piece is the oracle's Poseidon2 permutation (oracle_lib.poseidon2).  The AIRs of AddSub
and IO are written from the reference's `eval`:

    AddSub  crates/core/machine/src/alu/mod.rs:159-193 + operations/add.rs:42-75   (8 constraints)
    IO      crates/core/machine/src/io/mod.rs:127-141                              (3 constraints)

(send / receive / range_check_u8 are no-ops under the uni-STARK builders, air/builder.rs:232-239,
273-275.)  What it checks of a BFU1 proof is described at check_transcript, check_openings and
check_quotient.
"""
from __future__ import annotations

import struct

import oracle_lib as O

P = 0x7F000001
R_INV = pow(2, -32, P)
MAGIC = 0x31554642  # "BFU1"
POW_BITS = 16


def from_mont_array(a):
    """Montgomery words (numpy uint32) -> canonical Python ints, same shape as nested lists."""
    import numpy as np
    return ((a.astype(np.uint64) * np.uint64(R_INV)) % np.uint64(P)).astype(np.uint64).tolist()


def two_adic_gen(bits: int) -> int:
    """p - 1 = 2^24 * 127 and 3 generates F*: the generator of the subgroup of order 2^bits."""
    return pow(pow(3, 127, P), 1 << (24 - bits), P)


# ---------------------------------------------------------------------------- EF = F[x]/(x^4 - 3)
class EF:
    __slots__ = ("c",)

    def __init__(self, c):
        self.c = tuple(int(v) % P for v in c)

    @staticmethod
    def base(v: int) -> "EF":
        return EF((v, 0, 0, 0))

    def __add__(self, o):
        o = _ef(o)
        return EF(tuple(a + b for a, b in zip(self.c, o.c)))

    def __sub__(self, o):
        o = _ef(o)
        return EF(tuple(a - b for a, b in zip(self.c, o.c)))

    def __neg__(self):
        return EF(tuple(-a for a in self.c))

    def __mul__(self, o):
        o = _ef(o)
        a, b = self.c, o.c
        r = [0] * 7
        for i in range(4):
            for j in range(4):
                r[i + j] += a[i] * b[j]
        return EF((r[0] + 3 * r[4], r[1] + 3 * r[5], r[2] + 3 * r[6], r[3]))

    __radd__ = __add__
    __rmul__ = __mul__

    def __rsub__(self, o):
        return _ef(o) - self

    def __eq__(self, o):
        return self.c == _ef(o).c

    def __hash__(self):
        return hash(self.c)

    def __repr__(self):
        return f"EF{self.c}"

    def __pow__(self, e: int):
        r, b = EF.base(1), self
        while e:
            if e & 1:
                r = r * b
            b = b * b
            e >>= 1
        return r

    def inv(self) -> "EF":
        # a = A + B x with A = a0 + a2 u, B = a1 + a3 u over F[u]/(u^2 - 3), u = x^2:
        # 1/a = (A - B x) / (A^2 - u B^2), and 1/(d0 + d1 u) = (d0 - d1 u) / (d0^2 - 3 d1^2)
        a0, a1, a2, a3 = self.c
        A2 = ((a0 * a0 + 3 * a2 * a2) % P, (2 * a0 * a2) % P)          # A^2
        B2 = ((a1 * a1 + 3 * a3 * a3) % P, (2 * a1 * a3) % P)          # B^2
        d0 = (A2[0] - 3 * B2[1]) % P                                   # A^2 - u B^2
        d1 = (A2[1] - B2[0]) % P
        n = pow((d0 * d0 - 3 * d1 * d1) % P, P - 2, P)
        e0, e1 = d0 * n % P, (-d1) * n % P                             # 1 / (d0 + d1 u)
        # (A - B x) (e0 + e1 u), coefficients of 1, x, x^2 = u, x^3 = u x
        return EF((a0 * e0 + 3 * a2 * e1, -(a1 * e0 + 3 * a3 * e1), a0 * e1 + a2 * e0,
                   -(a1 * e1 + a3 * e0)))


def _ef(v) -> EF:
    return v if isinstance(v, EF) else EF.base(v)


ZERO, ONE = EF.base(0), EF.base(1)


def monomial(e: int) -> EF:
    c = [0, 0, 0, 0]
    c[e] = 1
    return EF(c)


# ---------------------------------------------------------------------------- challenger
class Challenger:
    """p3 DuplexChallenger<KoalaBear, Poseidon2<16>, 16, 8> over canonical words: observe pushes
    to the input buffer and clears the outputs, duplexing at 8 pending; sample duplexes when
    inputs are pending or no output is left and pops from the END of the outputs."""

    def __init__(self):
        self.state = [0] * 16
        self.inp = []
        self.out = []

    def _duplex(self):
        for i, v in enumerate(self.inp):
            self.state[i] = v
        self.inp = []
        self.state = [int(v) for v in O.poseidon2([self.state]).reshape(-1)]
        self.out = list(self.state[:8])

    def observe(self, v: int):
        self.out = []
        self.inp.append(int(v) % P)
        if len(self.inp) == 8:
            self._duplex()

    def observe_all(self, vs):
        for v in vs:
            self.observe(v)

    def observe_ef(self, e: EF):
        self.observe_all(e.c)

    def sample(self) -> int:
        if self.inp or not self.out:
            self._duplex()
        return self.out.pop()

    def sample_ef(self) -> EF:
        return EF([self.sample() for _ in range(4)])

    def sample_bits(self, bits: int) -> int:
        return self.sample() & ((1 << bits) - 1)

    def words(self):
        """(sponge_state, input_buffer, output_buffer) as canonical words."""
        return list(self.state), list(self.inp), list(self.out)


def challenger_words(ch) -> tuple:
    """A bfz Challenger struct (Montgomery words) in the form of Challenger.words()."""
    fm = lambda v: (int(v) * R_INV) % P
    return ([fm(v) for v in ch.sponge_state], [fm(ch.input_buffer[i]) for i in range(ch.n_input)],
            [fm(ch.output_buffer[i]) for i in range(ch.n_output)])


# ---------------------------------------------------------------------------- BFU1
class Reader:
    def __init__(self, b: bytes):
        self.b, self.off = b, 0

    def u32(self) -> int:
        (v,) = struct.unpack_from("<I", self.b, self.off)
        self.off += 4
        return v

    def words(self, n: int):
        v = struct.unpack_from(f"<{n}I", self.b, self.off)
        self.off += 4 * n
        return list(v)

    def ef(self) -> EF:
        return EF(self.words(4))

    def efs(self):
        return [self.ef() for _ in range(self.u32())]


def parse(proof: bytes) -> dict:
    """The BFU1 normal form, canonical words."""
    r = Reader(proof)
    assert r.u32() == MAGIC
    p = {"chip": r.u32(), "log_degree": r.u32(), "trace_commit": r.words(8),
         "quotient_commit": r.words(8)}
    p["trace_local"] = r.efs()
    p["trace_next"] = r.efs()
    p["chunks"] = [r.efs() for _ in range(r.u32())]
    p["commit_roots"] = [r.words(8) for _ in range(r.u32())]
    queries = []
    for _ in range(r.u32()):
        inputs = []
        for _ in range(r.u32()):
            rows = [r.words(r.u32()) for _ in range(r.u32())]
            path = [r.words(8) for _ in range(r.u32())]
            inputs.append((rows, path))
        steps = []
        for _ in range(r.u32()):
            sib = r.ef()
            steps.append((sib, [r.words(8) for _ in range(r.u32())]))
        queries.append((inputs, steps))
    p["queries"] = queries
    p["final_poly"] = r.ef()
    p["pow_witness"] = r.u32()
    assert r.off == len(proof)
    return p


# ---------------------------------------------------------------------------- AIRs
def _bool(x):
    return x * (x - 1)


def addsub_constraints(local, nxt=None, first=None, last=None, trans=None):
    """AddSubCols: pc 0, add_operation.value 1, .carry 2, operand_1 3, operand_2 4, is_add 5,
    is_sub 6.  alu/mod.rs:164-176 then AddOperation::eval, operations/add.rs:49-67."""
    value, carry, a, b, is_add, is_sub = local[1], local[2], local[3], local[4], local[5], local[6]
    is_real = is_add + is_sub
    out = [_bool(is_add), _bool(is_sub), _bool(is_real)]
    overflow = a + b - value
    out.append(is_real * (overflow * (overflow - 256)))
    out.append(is_real * (carry * (overflow - 256)))
    out.append(is_real * ((carry - 1) * overflow))
    out.append(is_real * _bool(carry))
    out.append(is_real * _bool(is_real))
    return out


def io_constraints(local, nxt=None, first=None, last=None, trans=None):
    """IoCols: pc 0, mp 1, mv 2, is_input 3, is_output 4.  io/mod.rs:131-135."""
    is_input, is_output = local[3], local[4]
    return [_bool(is_input), _bool(is_output), _bool(is_input + is_output)]


AIRS = {2: addsub_constraints, 7: io_constraints}
# the maximal degree of each model AIR, by hand from the expressions above: AddSub's
# is_real * (overflow * (overflow - 256)) is cubic, IO's booleans are quadratic
LOG_QUOTIENT_DEGREE = {2: 1, 7: 0}


def failing_rows(chip: int, trace) -> list:
    """Rows of a canonical trace (list of rows) on which some model constraint is non-zero."""
    air = AIRS[chip]
    n = len(trace)
    bad = []
    for i, row in enumerate(trace):
        loc = [EF.base(v) for v in row]
        nx = [EF.base(v) for v in trace[(i + 1) % n]]
        if any(c != ZERO for c in air(loc, nx, int(i == 0), int(i == n - 1), int(i != n - 1))):
            bad.append(i)
    return bad


# ---------------------------------------------------------------------------- the checks
def replay(p: dict, observe_openings: bool = True, ch: Challenger | None = None) -> dict:
    """The whole transcript from the proof's own commitments and opened values (check (a)): the
    head observe F(log n), the trace commitment, alpha, the quotient commitment, zeta; then the PCS
    transcript: the opened values round by round (trace at zeta, trace at zeta w, each chunk), the
    batching challenge, every commit-phase root and its beta, the final value, the PoW witness,
    the query indices."""
    ch = ch or Challenger()
    k = p["log_degree"]
    ch.observe(k)
    ch.observe_all(p["trace_commit"])
    alpha = ch.sample_ef()
    ch.observe_all(p["quotient_commit"])
    zeta = ch.sample_ef()
    if observe_openings:
        for v in p["trace_local"] + p["trace_next"]:
            ch.observe_ef(v)
        for c in p["chunks"]:
            for v in c:
                ch.observe_ef(v)
    fri_alpha = ch.sample_ef()
    betas = []
    for root in p["commit_roots"]:
        ch.observe_all(root)
        betas.append(ch.sample_ef())
    ch.observe_ef(p["final_poly"])
    ch.observe(p["pow_witness"])
    pow_ok = ch.sample_bits(POW_BITS) == 0
    log_max = len(p["commit_roots"]) + 1
    indices = [ch.sample_bits(log_max) for _ in p["queries"]]
    return {"alpha": alpha, "zeta": zeta, "fri_alpha": fri_alpha, "betas": betas, "pow_ok": pow_ok,
            "indices": indices, "log_max": log_max, "state": ch.words()}


def check_transcript(p: dict, final_state=None, observe_openings: bool = True) -> dict:
    """(a): alpha and zeta are not in the proof, so the replay is pinned at both ends: the proof's
    PoW witness must satisfy the model's sponge after everything before it (a wrong alpha, zeta
    or opening order passes with probability 2^-16), the FRI round count must be log n, and --
    when the code's ending challenger is given (challenger_words) -- the model must end in it."""
    t = replay(p, observe_openings)
    assert t["pow_ok"], "the proof's PoW witness does not satisfy the model's transcript"
    assert t["log_max"] == p["log_degree"] + 1
    if final_state is not None:
        assert [list(s) for s in t["state"]] == [list(s) for s in final_state], \
            "the model's transcript ends in another challenger state"
    return t


def lagrange_eval(column, z: EF) -> EF:
    """The interpolant of column (values on H_n in natural order, v_i at w_n^i) at z, by the
    Lagrange formula  p(z) = sum_i v_i * prod_(j != i) (z - w^j) / (w^i - w^j)."""
    n = len(column)
    w = two_adic_gen(n.bit_length() - 1)
    xs = [pow(w, i, P) for i in range(n)]
    diffs = [z - x for x in xs]
    acc = ZERO
    for i in range(n):
        if column[i] == 0:
            continue
        num, den = ONE, 1
        for j in range(n):
            if j != i:
                num = num * diffs[j]
                den = den * (xs[i] - xs[j]) % P
        acc = acc + num * (column[i] * pow(den, P - 2, P) % P)
    return acc


def check_openings(p: dict, trace, zeta: EF):
    """(c): trace_local / trace_next are the columns' interpolants at zeta and zeta * w_n.
    trace = canonical rows; meant for n <= 64."""
    n = len(trace)
    assert n == 1 << p["log_degree"]
    width = len(trace[0])
    assert len(p["trace_local"]) == width and len(p["trace_next"]) == width
    znext = zeta * two_adic_gen(p["log_degree"])
    for c in range(width):
        col = [row[c] for row in trace]
        assert lagrange_eval(col, zeta) == p["trace_local"][c], f"column {c} at zeta"
        assert lagrange_eval(col, znext) == p["trace_next"][c], f"column {c} at zeta * w"


def quotient_at_zeta(p: dict, zeta: EF) -> EF:
    """The quotient recomposed from its chunk openings: chunk j lives on 3 g^j H_n (g the
    generator of order n * chunks), its 4 base columns are the coefficients of 1, x, x^2, x^3, and
    quotient(zeta) = sum_j zps_j * chunk_j(zeta), zps_j = prod_(k != j) Z_k(zeta) / Z_k(3 g^j)."""
    chunks = p["chunks"]
    m = len(chunks)
    lqd = m.bit_length() - 1
    n_log = p["log_degree"]
    g = two_adic_gen(n_log + lqd)
    shifts = [3 * pow(g, j, P) % P for j in range(m)]

    def z_at(k, x: EF) -> EF:  # the vanishing polynomial of 3 g^k H_n
        return (x * pow(shifts[k], P - 2, P)) ** (1 << n_log) - 1

    q = ZERO
    for j in range(m):
        zps = ONE
        for k in range(m):
            if k != j:
                zps = zps * z_at(k, zeta) * z_at(k, EF.base(shifts[j])).inv()
        q = q + zps * sum((monomial(e) * chunks[j][e] for e in range(4)), ZERO)
    return q


def folded_at_zeta(p: dict, alpha: EF, zeta: EF) -> EF:
    """The model AIR over the opened rows with the selectors at zeta, folded by Horner in emission
    order (acc = acc * alpha + c), times 1 / Z_H(zeta)."""
    n_log = p["log_degree"]
    w_inv = pow(two_adic_gen(n_log), P - 2, P)
    zh = zeta ** (1 << n_log) - 1
    first = zh * (zeta - 1).inv()
    last = zh * (zeta - w_inv).inv()
    trans = zeta - w_inv
    acc = ZERO
    for c in AIRS[p["chip"]](p["trace_local"], p["trace_next"], first, last, trans):
        acc = acc * alpha + c
    return acc * zh.inv()


def check_quotient(p: dict, alpha: EF, zeta: EF):
    """(d), AddSub and IO: folded constraints at zeta / Z_H(zeta) == the recomposed quotient."""
    assert len(p["chunks"]) == 1 << LOG_QUOTIENT_DEGREE[p["chip"]]
    assert all(len(c) == 4 for c in p["chunks"])
    assert folded_at_zeta(p, alpha, zeta) == quotient_at_zeta(p, zeta), \
        "folded constraints / Z_H(zeta) differ from the recomposed quotient"
