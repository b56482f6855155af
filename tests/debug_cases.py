"""Shared inputs of tests/test_debug_constraints.py (host path) and
tests/test_debug_constraints_gpu.py (device path): oracle traces and permutation traces under
seeded challenges, and the single-cell corruption cases with what the checker must report.

Everything here is in canonical form (the oracle's); check() converts to Montgomery words at the
product's ABI."""
from functools import lru_cache

import numpy as np

import oracle_lib as O
from bfz import guests, sdk

P = O.P
PROGRAMS = [("hello", guests.HELLO, ()), ("loop", guests.LOOP, ()), ("fibo17", guests.FIBO, (17,)),
            ("plus", "+", ())]
# lookups per chip (csrc/air.h *_LOOKUPS): a chip has ceil(n / 2) LogUp batch constraints
N_LOOKUPS = (16, 1, 5, 1, 4, 2, 1, 1)


def mont(a):
    return ((np.asarray(a, dtype=np.uint64) << np.uint64(32)) % np.uint64(P)).astype(np.uint32)


def challenges(seed):
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(1, P, 4)], [int(x) for x in rng.integers(1, P, 4)]


@lru_cache(maxsize=None)
def _trace(prog, stdin, chip, prep):
    t = O.trace(prog, list(stdin), chip, prep)
    if t is not None:
        t.setflags(write=False)  # shared between tests: corrupt a copy
    return t


def traces(prog, stdin, chip):
    """(main, prep or None) of an included chip, else None."""
    m = _trace(prog, tuple(stdin), chip, False)
    if m is None:
        return None
    return m, (_trace(prog, tuple(stdin), chip, True) if chip in (1, 5) else None)


def included(prog, stdin):
    return [c for c in range(8) if traces(prog, stdin, c) is not None]


def perm(chip, main, prep, alpha, beta):
    p, cs = O.perm_trace(chip, main, prep, alpha, beta)
    return p.copy(), cs


def check(chip, main, prep, perm_t, alpha, beta, cs, on_device=False):
    return sdk.check_chip(chip, mont(main), None if prep is None else mont(prep), mont(perm_t),
                          [O.to_mont(x) for x in alpha], [O.to_mont(x) for x in beta],
                          [O.to_mont(x) for x in cs], on_device=on_device, per_row=True)


def k_air(res):
    return res.num_constraints - res.num_batches - 3


def real_rows(chip, main):
    """Rows of a FIBO [17] trace that hold an event (AddSub: is_add + is_sub, Cpu: is_real)."""
    if chip == 2:
        return np.nonzero((main[:, 5] + main[:, 6]) == 1)[0]
    assert chip == 0
    return np.nonzero(main[:, 30] == 1)[0]


def corruption_cases():
    """[(name, chip, main, prep, perm, alpha, beta, cumsum, expect)] on FIBO [17]'s AddSub and Cpu
    traces.  expect(res) asserts what the issue pins for the case."""
    prog, stdin = guests.FIBO, (17,)
    alpha, beta = challenges(11)
    out = []

    # AddSub is_add = 2 at a real row, permutation trace regenerated: row r alone, index 0
    m, _ = traces(prog, stdin, 2)
    r = int(real_rows(2, m)[3])
    bad = m.copy()
    bad[r, 5] = 2
    p, cs = perm(2, bad, None, alpha, beta)

    def exp_is_add(res, r=r):
        rows = np.nonzero(res.first_fail_per_row >= 0)[0]
        assert list(rows) == [r], rows
        assert res.failing_rows == 1 and res.first_row == r and res.first_constraint == 0
        assert res.first_fail_per_row[r] == 0
    out.append(("addsub_is_add", 2, bad, None, p, alpha, beta, cs, exp_is_add))

    # Cpu is_real (column 30) = 2 at a real row 0 < r < h - 1, permutation trace regenerated
    m, _ = traces(prog, stdin, 0)
    h = m.shape[0]
    assert h > 256
    r = int([x for x in real_rows(0, m) if 0 < x < h - 1][7])
    bad = m.copy()
    bad[r, 30] = 2
    p, cs = perm(0, bad, None, alpha, beta)

    def exp_is_real(res, r=r):
        rows = set(np.nonzero(res.first_fail_per_row >= 0)[0].tolist())
        assert rows and rows <= {r - 1, r}, rows
        assert res.failing_rows == len(rows) and res.first_row == min(rows)
    out.append(("cpu_is_real", 0, bad, None, p, alpha, beta, cs, exp_is_real))

    # valid main, one cell of the permutation trace perturbed
    for chip in (2, 0):
        m, _ = traces(prog, stdin, chip)
        h = m.shape[0]
        p0, cs = perm(chip, m, None, alpha, beta)
        nb = (N_LOOKUPS[chip] + 1) // 2
        phi = 4 * nb  # first base column of the running sum

        def poke(row, col):
            q = p0.copy()
            q[row, col] = (int(q[row, col]) + 1) % P
            return q

        def exp_rows(want):  # {row: first index as an offset from K (negative) or from K_air}
            def f(res, want=want):
                K, ka = res.num_constraints, k_air(res)
                got = {int(i): int(res.first_fail_per_row[i])
                       for i in np.nonzero(res.first_fail_per_row >= 0)[0]}
                exp = {row: (K + v if v < 0 else ka + v) for row, v in want.items()}
                assert got == exp, (got, exp)
                assert res.failing_rows == len(exp)
                assert res.first_row == min(exp) and res.first_constraint == exp[min(exp)]
            return f

        r = h // 2 + 3
        out.append((f"chip{chip}_phi_mid", chip, m, None, poke(r, phi + 1), alpha, beta, cs,
                    exp_rows({r - 1: -2, r: -2})))
        out.append((f"chip{chip}_phi_last", chip, m, None, poke(h - 1, phi), alpha, beta, cs,
                    exp_rows({h - 2: -2, h - 1: -1})))
        out.append((f"chip{chip}_phi_first", chip, m, None, poke(0, phi + 2), alpha, beta, cs,
                    exp_rows({0: -3})))
        b = nb - 1
        out.append((f"chip{chip}_batch", chip, m, None, poke(r, 4 * b + 3), alpha, beta, cs,
                    exp_rows({r - 1: -2, r: b})))
    return out
