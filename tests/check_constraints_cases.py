"""Shared inputs of tests/test_check_constraints.py (host path) and
tests/test_check_constraints_gpu.py (kernels): the per-constraint failure profile
(bfz_uni_check_constraints, bfz_air_check_constraints, bfz_record_uni_check_constraints).

The reference is reference(): the BFA1 node list evaluated in integers mod p over all rows at once
(uint64 arrays; p < 2^31, so a product fits), with the debug.rs row semantics.  The built-in chips
go through it as their exported programs.  Traces are Montgomery words."""
import ctypes
from functools import lru_cache

import numpy as np

import air_program_cases as A
import uni_device_cases as U
from bfz import _lib, guests, sdk

P = A.P
R_INV = pow(2, -32, P)
# 1: the row is its own next; 2: the wrap; 64: exactly one wave; 256: one block; 512: two blocks
# (the flush's device atomics); 1024
HEIGHTS = [1, 2, 64, 256, 512, 1024]
PROGRAMS = ["fib", "mulgate", "addsub", "jump", "one", "wide512"]
CASES = [(p, h) for p in PROGRAMS for h in HEIGHTS]
CHIP_OF = {"addsub": A.ADDSUB, "jump": A.JUMP}
# name: (the column the changes go to; a second column whose change breaks other constraints -- a
# one-column AIR has none; the constraints that fail on EVERY row once the first column is off by
# 2 everywhere: those that read it without a selector)
COLUMNS = {"fib": (0, 1, []), "mulgate": (3, 2, [0]), "addsub": (5, 6, [0]), "jump": (43, 44, [0]),
           "one": (0, None, [0]), "wide512": (0, None, list(range(512)))}


@lru_cache(maxsize=None)
def program_and_trace(name, height):
    """(BFA1 bytes, a valid Montgomery trace of `height` rows, read-only)"""
    if name in ("fib", "mulgate"):
        prog, _, t, _ = A.custom_case(name, height)
        return prog, t
    if name in CHIP_OF:  # every constraint of AddSub and Jump is row-local: real rows, repeated
        src = U.trace_of(CHIP_OF[name], guests.HELLO)
        prog, t = A.export(CHIP_OF[name]), np.resize(src, (height, src.shape[1]))
    else:
        ab = sdk.AirBuilder(1)
        x = ab.local(0)
        if name == "one":
            ab.assert_zero(x * (x - 1))
        for k in range(512 if name == "wide512" else 0):  # all fail wherever the column is not 0
            ab.assert_zero(x * (k + 1))
        prog, t = ab.build(), np.zeros((height, 1), dtype=np.uint32)
    t.setflags(write=False)
    return prog, t


def bump(trace, rows, col):
    """A copy with the canonical value + 2 in the cells (rows, col): a 0/1 cell stops being one."""
    bad = np.array(trace, dtype=np.uint32)
    bad[rows, col] = (bad[rows, col].astype(np.uint64) + np.uint64((2 << 32) % P)) % np.uint64(P)
    return bad


def traces(name, height):
    """[(label, trace)]: the valid trace; one cell changed in a middle row, in the last row (the
    wrap-around, is_last / is_transition) and in row 0; the column wrong on every row; two cells of
    the middle row that break different constraints."""
    _, t = program_and_trace(name, height)
    c0, c1, _ = COLUMNS[name]
    mid = height // 2
    out = [("valid", t), ("middle", bump(t, mid, c0)), ("last", bump(t, height - 1, c0)),
           ("row0", bump(t, 0, c0)), ("column", bump(t, slice(None), c0))]
    return out + ([("two", bump(bump(t, mid, c0), mid, c1))] if c1 is not None else [])


def reference(prog, trace):
    """(counts[K], first_rows[K]) of a BFA1 program over a Montgomery trace, as lists."""
    w = np.frombuffer(prog, dtype="<u4")
    nn, k = int(w[2]), int(w[3])
    nodes, cons = w[4:4 + 3 * nn].reshape(nn, 3).tolist(), w[4 + 3 * nn:4 + 3 * nn + k].tolist()
    p = np.uint64(P)
    t = np.asarray(trace, dtype=np.uint64) * np.uint64(R_INV) % p  # canonical
    h = len(t)
    rows, nxt, v = np.arange(h), np.roll(t, -1, axis=0), []
    for op, a, b in nodes:
        v.append([lambda: np.full(h, a * R_INV % P, dtype=np.uint64), lambda: t[:, a],
                  lambda: nxt[:, a], lambda: (rows == 0).astype(np.uint64),
                  lambda: (rows == h - 1).astype(np.uint64), lambda: (rows != h - 1).astype(np.uint64),
                  lambda: (v[a] + v[b]) % p, lambda: (v[a] + p - v[b]) % p,
                  lambda: v[a] * v[b] % p, lambda: (p - v[a]) % p][op]())
    bad = [np.nonzero(v[c])[0] for c in cons]
    return [len(x) for x in bad], [int(x[0]) if len(x) else -1 for x in bad]


def check_case(name, height, on_device):
    """Every trace of the case through bfz_air_check_constraints (a chip's also through
    bfz_uni_check_constraints) against the reference and the first-fail call's summary.  Returns
    [(label, summary, counts, first_rows)] for a comparison between the paths."""
    prog, _ = program_and_trace(name, height)
    got = []
    for label, t in traces(name, height):
        res, counts, first = sdk.air_check_constraints(prog, t, on_device=on_device)
        counts, first = counts.tolist(), first.tolist()
        assert (counts, first) == reference(prog, t), label
        assert A.summary(res) == A.summary(sdk.air_check(prog, t, on_device=on_device)), label
        if name in CHIP_OF:  # the compiled chip against its exported program
            chip = CHIP_OF[name]
            cres, ccounts, cfirst = sdk.uni_stark_check_constraints(chip, t, on_device=on_device)
            assert (ccounts.tolist(), cfirst.tolist()) == (counts, first), label
            assert A.summary(cres) == A.summary(sdk.uni_stark_check(chip, t, on_device=on_device)), label
        if any(counts):  # the summary follows from the tables
            assert res.first_row == min(f for f in first if f >= 0), label
            assert res.first_constraint == first.index(res.first_row), label
        # what each trace is there for
        if label == "valid":
            assert not any(counts) and set(first) == {-1} and res.ok
        elif label == "column":
            assert all(counts[k] == height and first[k] == 0 for k in COLUMNS[name][2])
        else:  # "two": a second constraint, which the first-fail call cannot show
            assert sum(c > 0 for c in counts) >= (2 if label == "two" else 1), label
        got.append((label, A.summary(res), counts, first))
    return got


def refusals(on_device):
    """[(label, (status, message) of the profile call, the same of the first-fail call)]: a wrong
    width, a height that is no power of two, a word >= p, a malformed program; a chip's width and
    height."""
    L = _lib.lib()
    u32p = ctypes.POINTER(ctypes.c_uint32)
    res, counts, first = _lib.UniCheckC(), (ctypes.c_uint64 * 512)(), (ctypes.c_int64 * 512)()
    prog, t = program_and_trace("mulgate", 64)
    big = np.array(t)
    big[3, 1] = P
    out = []
    for label, pr, m, h, w in [("width", prog, t, 64, 3), ("height", prog, t, 48, 4),
                               ("word", prog, big, 64, 4), ("program", prog[:-2], t, 64, 4)]:
        buf, n = _lib.u8buf(pr)
        args = (buf, n, m.ctypes.data_as(u32p), h, w, on_device, ctypes.byref(res))
        new = (L.bfz_air_check_constraints(*args, counts, first), L.bfz_last_error().decode())
        out.append((label, new, (L.bfz_air_check(*args, None), L.bfz_last_error().decode())))
    jt = U.trace_of(A.JUMP, guests.HELLO)
    for label, h, w in [("chip-width", 32, 44), ("chip-height", 24, 45)]:
        rc = L.bfz_uni_check_constraints(A.JUMP, jt.ctypes.data_as(u32p), h, w, on_device,
                                         ctypes.byref(res), counts, first)
        out.append((label, (rc, L.bfz_last_error().decode()),
                    U.uni_check_status(A.JUMP, jt, on_device, h, w)))
    return out
