"""Shared by tests/test_machine_check.py and tests/test_machine_check_gpu.py: the flipped cells and a
plain recount of a chip's constraints in Python integers (debug.rs:43-94 frame)."""
import numpy as np

import air_program_cases as A
import chip_cases as C
import lookups_cases as L
import machine_cases as M

P = C.P
HEIGHTS = (1, 4, 512)
# (chip, row, column, times + 1): s = 2 in the last row of m512 (a padding row: one flip would give
# a valid row); c + 1 in row 0 of m4 and in m1's only row; one multiplicity of the table
FLIPS = [("m512", 511, 3, 2), ("m4", 0, 2, 1), ("m1", 0, 2, 1), ("table", 3, 0, 1)]
FLIP_IDS = ["m512-last", "m4-row0", "m1-only", "table-mult"]


def flipped(traces, name, row, col, times):
    bad = dict(traces)
    for _ in range(times):
        bad[name] = C.flip(bad[name], row, col)
    return bad


def programs(name):
    """(air, mirror, lookups) of a chip of machine_cases.custom_machine."""
    if name == "table":
        return None, None, M.table_lookups()
    return A.mulgate_program(), A.mulgate_mirror, M.sender_program()


def recount(mirror, prog, main, prep, perm, alpha, beta, cumsum):
    """bool[n][K]: constraint k is not zero on row i.  Montgomery arrays and words in."""
    main, perm = (C.unmont(np.asarray(x)).astype(object).tolist() for x in (main, perm))
    prep = C.unmont(np.asarray(prep)).astype(object).tolist() if prep is not None else None
    alpha, beta, cumsum = ([int(v) for v in C.unmont(np.array(x, dtype=np.uint32))]
                           for x in (alpha, beta, cumsum))
    chain, n = C._parse(prog), len(main)
    nb = (len(chain) + 1) // 2
    bp = [[1, 0, 0, 0]]
    for _ in range(7):
        bp.append(L.ef_mul(bp[-1], beta))
    out = []
    for i in range(n):
        nx, first, last = (i + 1) % n, int(i == 0), int(i == n - 1)
        m, pr = main[i], prep[i] if prep is not None else None
        cons = [[v % P, 0, 0, 0] for v in mirror(m, main[nx], first, last, 1 - last)] if mirror else []

        def ev(vc):
            return (vc[0] + sum(wt * (pr if s else m)[c] for s, c, wt in vc[1])) % P

        dm = []
        for kind, send, mult, vals in chain:
            den = L.ef_add(alpha, [kind, 0, 0, 0])
            for v, vc in enumerate(vals):
                den = L.ef_add(den, C.ef_scale(bp[v + 1], ev(vc)))
            dm.append((den, ev(mult) if send else -ev(mult) % P))
        pl = [perm[i][4 * b:4 * b + 4] for b in range(nb + 1)]
        pn = [perm[nx][4 * b:4 * b + 4] for b in range(nb + 1)]
        sum_l, sum_n = [0] * 4, [0] * 4
        for b in range(nb):
            d0, m0 = dm[2 * b]
            if 2 * b + 1 < len(chain):
                d1, m1 = dm[2 * b + 1]
                cons.append(C.ef_sub(L.ef_mul(L.ef_mul(d0, d1), pl[b]),
                                     L.ef_add(C.ef_scale(d1, m0), C.ef_scale(d0, m1))))
            else:
                cons.append(C.ef_sub(L.ef_mul(d0, pl[b]), [m0, 0, 0, 0]))
            sum_l, sum_n = L.ef_add(sum_l, pl[b]), L.ef_add(sum_n, pn[b])
        cons.append(C.ef_scale(C.ef_sub(pl[nb], sum_l), first))
        cons.append(C.ef_scale(C.ef_sub(C.ef_sub(pn[nb], pl[nb]), sum_n), 1 - last))
        cons.append(C.ef_scale(C.ef_sub(pl[nb], cumsum), last))
        out.append([any(v % P for v in c) for c in cons])
    return np.array(out, dtype=bool)


def same_report(a, b):
    """Two MachineCheckReports agree field for field."""
    assert (a.ok, a.alpha, a.beta, a.cumulative_sum, a.names) == (
        b.ok, b.alpha, b.beta, b.cumulative_sum, b.names)
    assert a.chips == b.chips
    for x, y in zip(a.counts + a.first_rows, b.counts + b.first_rows):
        assert np.array_equal(x, y)
