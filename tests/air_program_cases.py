"""Shared inputs of tests/test_air_program.py (host paths) and tests/test_air_program_gpu.py (device
paths): two AIRs that are not chips, built with sdk.AirBuilder and mirrored as plain Python
functions in the signature of uni_stark_model.AIRS, their traces, and the built-in chips' cases the
device tests compare the constraint programs against.

Traces here are Montgomery words (the product's ABI) unless a name says canonical."""
import ctypes
from functools import lru_cache

import numpy as np

import oracle_lib as O
import uni_stark_model as M
from bfz import _lib, guests, sdk

P = O.P
CPU, ADDSUB, JUMP, MEMINSTRS, IO = 0, 2, 3, 6, 7
WIDTHS = {CPU: 31, ADDSUB: 7, JUMP: 45, MEMINSTRS: 41, IO: 5}
QUERIES = 6

# (id, chip, program, stdin, height): the cases of tests/test_uni_stark_gpu.py that the parity
# tests use, restated (both quotient shapes, is_first, is_transition, next-row columns, 3 to 44
# constraints)
CHIP_CASES = [
    ("cpu-1", CPU, "+", [], 1),
    ("cpu-4", CPU, "+++.", [], 4),
    ("cpu-512", CPU, guests.HELLO, [], 512),
    ("addsub-16", ADDSUB, "+", [], 16),
    ("addsub-256", ADDSUB, guests.HELLO, [], 256),
    ("jump-32", JUMP, guests.HELLO, [], 32),
    ("jump-8192", JUMP, guests.FIBO, [17], 8192),
    ("meminstrs-16", MEMINSTRS, ">", [], 16),
    ("meminstrs-64", MEMINSTRS, guests.HELLO, [], 64),
    ("io-16", IO, ".", [], 16),
    ("io-32", IO, "." * 17, [], 32),
]
# Why these heights (the LDE is twice the height; the kernels run on LDE points and on trace rows):
# 1: the row is its own next row, no FRI round, a grid smaller than a wave; 2 and 4: the next-row
# index wraps; 16 and 256: one partially filled or one full block; 256 (LDE 512) and above: several
# blocks -- the reduction across blocks and the chunk split at t >> (logN - 1).
FIB_HEIGHTS = [1, 2, 4, 256, 1024]
MULGATE_HEIGHTS = [1, 4, 16, 512]


def mont(a):
    return ((np.asarray(a, dtype=np.uint64) << np.uint64(32)) % np.uint64(P)).astype(np.uint32)


@lru_cache(maxsize=None)
def export(chip):
    return sdk.air_export(chip)


# ---------------------------------------------------------------------------- fib
def fib_canonical(height):
    """Rows (a, b): (0, 1), then (b, a + b) mod p."""
    rows = [(0, 1)]
    for _ in range(height - 1):
        a, b = rows[-1]
        rows.append((b, (a + b) % P))
    return rows


def fib_program(last_b):
    """width 2 (a, b), K = 5, degree 2, one quotient chunk; last_b = the trace's last b."""
    ab = sdk.AirBuilder(2)
    a, b = ab.local(0), ab.local(1)
    ab.assert_zero(ab.is_first_row * a)
    ab.assert_zero(ab.is_first_row * (b - 1))
    ab.assert_zero(ab.is_transition * (ab.next(0) - b))
    ab.assert_zero(ab.is_transition * (ab.next(1) - (a + b)))
    ab.assert_zero(ab.is_last_row * (b - ab.const(last_b)))
    return ab.build()


def fib_mirror(last_b):
    def constraints(local, nxt, first, last, trans):
        a, b = local[0], local[1]
        return [first * a, first * (b - 1), trans * (nxt[0] - b), trans * (nxt[1] - (a + b)),
                last * (b - last_b)]
    return constraints


@lru_cache(maxsize=None)
def fib_case(height):
    """(program, mirror, Montgomery trace (read-only), canonical rows)"""
    rows = fib_canonical(height)
    t = mont(rows)
    t.setflags(write=False)
    return fib_program(rows[-1][1]), fib_mirror(rows[-1][1]), t, rows


# ---------------------------------------------------------------------------- mulgate
def mulgate_canonical(height, seed=7):
    """Rows (a, b, c, s): the first m = height - height // 4 rows are real (s = 1, c = a b, the
    next real row's a is this row's c, b from a seeded generator), the rest all zero."""
    rng = np.random.default_rng([height, seed])
    m = height - height // 4
    rows, a = [], int(rng.integers(1, P))
    for _ in range(m):
        b = int(rng.integers(1, P))
        rows.append((a, b, a * b % P, 1))
        a = rows[-1][2]
    rows += [(0, 0, 0, 0)] * (height - m)
    return rows


def mulgate_program(broken=None):
    """width 4 (a, b, c, s), K = 3, degree 3, two quotient chunks.  broken: a b replaced by
    "square" a a (another AIR of the same shape) or by "sum" a + b (of degree 2, so of another
    quotient shape), for the verifier's rejections."""
    ab = sdk.AirBuilder(4)
    a, b, c, s = (ab.local(i) for i in range(4))
    ab.assert_zero(s * (s - 1))
    gate = {None: lambda: a * b, "square": lambda: a * a, "sum": lambda: a + b}[broken]()
    ab.assert_zero(s * (c + -gate))  # uses NEG
    ab.assert_zero(ab.is_transition * ab.next(3) * (ab.next(0) - c))
    return ab.build()


def mulgate_mirror(local, nxt, first, last, trans):
    a, b, c, s = local[0], local[1], local[2], local[3]
    return [s * (s - 1), s * (c + -(a * b)), trans * nxt[3] * (nxt[0] - c)]


@lru_cache(maxsize=None)
def mulgate_case(height):
    rows = mulgate_canonical(height)
    t = mont(rows)
    t.setflags(write=False)
    return mulgate_program(), mulgate_mirror, t, rows


def custom_case(kind, height):
    return fib_case(height) if kind == "fib" else mulgate_case(height)


# ---------------------------------------------------------------------------- the mirrors as checks
def mirror_rows(mirror, rows):
    """int32[height]: each row's first failing constraint under the mirror, or -1 (row i local,
    row (i + 1) mod height next, 0/1 selectors, is_transition = 1 - is_last)."""
    n = len(rows)
    out = np.full(n, -1, dtype=np.int32)
    for i, row in enumerate(rows):
        vals = mirror(list(row), list(rows[(i + 1) % n]), int(i == 0), int(i == n - 1), int(i != n - 1))
        for k, v in enumerate(vals):
            if v % P:
                out[i] = k
                break
    return out


def summary(res):
    return (res.chip, res.height, res.num_constraints, res.failing_rows, res.first_row,
            res.first_constraint)


def summary_from_rows(rows, k, chip=-1):
    """What the summary of a check must be, given its per-row array."""
    bad = np.nonzero(rows >= 0)[0]
    if not len(bad):
        return (chip, len(rows), k, 0, -1, -1)
    return (chip, len(rows), k, len(bad), int(bad[0]), int(rows[bad[0]]))


def flip(trace, row, col, delta=1):
    """A copy of the Montgomery trace with cell (row, col) set to its canonical value + delta."""
    bad = np.array(trace, dtype=np.uint32)
    bad[row, col] = O.to_mont((O.from_mont(int(bad[row, col])) + delta) % P)
    return bad


def canonical(trace):
    return M.from_mont_array(np.asarray(trace))


# ---------------------------------------------------------------------------- raw calls
def air_verify_one(prog, proof):
    """bfz_air_verify: ((ok, query, why), the ending challenger's bytes)."""
    ch = sdk.Challenger()
    pbuf, pn = _lib.u8buf(prog)
    buf, n = _lib.u8buf(proof)
    out = _lib.VerifyOutcomeC()
    _lib.check(_lib.lib().bfz_air_verify(pbuf, pn, ctypes.byref(ch), buf, n, ctypes.byref(out)))
    return (bool(out.ok), out.query, out.why.decode()), bytes(ch)


def air_info_status(prog):
    """(status, message) of a raw bfz_air_info call."""
    buf, n = _lib.u8buf(prog)
    out = _lib.AirShapeC()
    L = _lib.lib()
    rc = L.bfz_air_info(buf, n, ctypes.byref(out))
    return rc, L.bfz_last_error().decode() if rc else ""


def air_prove_status(prog, m, h=None, w=None):
    """(status, message) of a raw bfz_air_prove call."""
    m = np.ascontiguousarray(m, dtype=np.uint32)
    ch = sdk.Challenger()
    ptr, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t()
    pbuf, pn = _lib.u8buf(prog)
    L = _lib.lib()
    rc = L.bfz_air_prove(pbuf, pn, m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                         m.shape[0] if h is None else h, m.shape[1] if w is None else w,
                         ctypes.byref(ch), ctypes.byref(ptr), ctypes.byref(n), None)
    if rc == 0:
        L.bfz_free(ptr)
    return rc, L.bfz_last_error().decode() if rc else ""
