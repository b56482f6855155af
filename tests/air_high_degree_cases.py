"""Shared inputs of tests/test_air_high_degree.py (host) and tests/test_air_high_degree_gpu.py
(device): two AIRs of degree 4 and 9 built with sdk.AirBuilder, each with a plain Python mirror
in the signature of uni_stark_model.AIRS, and their valid trace.

chain<k>, width 2 (x, y):  y - x^k;  is_transition (next.x - y - 1);  is_first_row (x - 2);
is_last_row (next.x - 2) -- the last row's next row is row 0, so the trace x_0 = 2, y_i = x_i^k,
x_(i+1) = y_i + 1 is valid at every height, 1 included."""
from functools import lru_cache

import air_program_cases as A
from bfz import sdk

P = A.P
POWER = {"chain4": 4, "chain9": 9}
LQD = {"chain4": 2, "chain9": 3}


def power(x, k):
    r = x
    for _ in range(k - 1):
        r = r * x
    return r


@lru_cache(maxsize=None)
def program(kind):
    k = POWER[kind]
    ab = sdk.AirBuilder(2)
    x, y = ab.local(0), ab.local(1)
    ab.assert_zero(y - power(x, k))
    ab.assert_zero(ab.is_transition * (ab.next(0) - y - 1))
    ab.assert_zero(ab.is_first_row * (x - 2))
    ab.assert_zero(ab.is_last_row * (ab.next(0) - 2))
    return ab.build()


def mirror(kind):
    k = POWER[kind]

    def constraints(local, nxt, first, last, trans):
        x, y = local[0], local[1]
        return [y - power(x, k), trans * (nxt[0] - y - 1), first * (x - 2), last * (nxt[0] - 2)]
    return constraints


@lru_cache(maxsize=None)
def case(kind, height):
    """(program, mirror, Montgomery trace (read-only), canonical rows)"""
    rows, x = [], 2
    for _ in range(height):
        rows.append((x, pow(x, POWER[kind], P)))
        x = (rows[-1][1] + 1) % P
    t = A.mont(rows)
    t.setflags(write=False)
    return program(kind), mirror(kind), t, rows
