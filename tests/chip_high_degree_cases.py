"""Shared by tests/test_chip_high_degree.py and tests/test_chip_high_degree_gpu.py: the chips
pow4 and pow9 (AIR degree 4 and 9: 4 and 8 quotient chunks), machines of them beside a mulgate
sender and the lookup table, and a chip's quotient on 3 H_(D n) in Python integers."""
import functools
import struct

import numpy as np

import air_program_cases as A
import chip_cases as C
import lookups_cases as L
import machine_cases as M
from bfz import sdk

P = C.P


@functools.lru_cache(maxsize=None)
def pow_chip(k):
    """(air, lookups, mirror): main (x, y, s), y = x^k on every row, s boolean, (x, y) sent under s."""
    ab = sdk.AirBuilder(3)
    x, y, s = (ab.local(i) for i in range(3))
    xk = x
    for _ in range(k - 1):
        xk = xk * x
    ab.assert_zero(y - xk)
    ab.assert_zero(s * (s - 1))
    b = sdk.LookupBuilder(3)
    b.send(3, [b.main(0), b.main(1)], b.main(2))
    return ab.build(), b.program(), lambda l, n, f, la, t: [l[1] - l[0] ** k, l[2] * (l[2] - 1)]


def pow_rows(k, n):
    """n valid rows, canonical; the first min(n, 3) are sent."""
    rng = np.random.default_rng([k, n])
    return [(x, pow(x, k, P), int(i < 3)) for i, x in enumerate(int(v) for v in rng.integers(2, P, n))]


def pow_trace(k, n):
    return C.mont(np.array(pow_rows(k, n), dtype=np.uint64))


@functools.lru_cache(maxsize=None)
def machine(heights):
    """heights: ((name, height), ...) over pow4 / pow9 / mulgate.  (Machine, traces) with the table
    chip that receives every sent key, its multiplicities from sdk.lookups_multiplicities (as
    machine_cases.custom_machine); the chip cap must admit the chips."""
    progs, senders = {}, {}
    for name, n in heights:
        if name == "mulgate":
            progs[name] = (A.mulgate_program(), M.sender_program())
            senders[name] = C.mont(np.array(M.sender_rows(n), dtype=np.uint64))
        else:
            progs[name] = pow_chip(int(name[3:]))[:2]
            senders[name] = pow_trace(int(name[3:]), n)
    sent = {"mulgate": lambda r: (r[0], r[1], r[3])}
    keys = sorted({(int(r[0]), int(r[1])) for name, t in senders.items()
                   for r in map(sent.get(name, lambda r: r), C.unmont(t)) if r[2]})
    keys += [(k, 0) for k in range(2, 34)][:32 - len(keys)]
    tlk = M.table_lookups()
    prep = C.mont(np.array([[a] for a, _ in keys], dtype=np.uint64))
    main = C.mont(np.array([[0, b] for _, b in keys], dtype=np.uint64))
    mult = sdk.lookups_multiplicities(tlk, main, prep, 0, [progs[n][1] for n in senders],
                                      list(senders.values()), [None] * len(senders))
    assert mult.unmatched == 0
    main[:, 0] = mult.mult
    m = sdk.Machine([(n, *progs[n], None) for n in senders] + [("table", None, tlk, prep)])
    return m, dict(senders, table=main)


def chunk_counts(proof):
    """The quotient chunk count of every chip of a BFZ1 machine proof, in proof order."""
    at, counts = 8, []
    nc = struct.unpack_from("<I", proof, 4)[0]
    for _ in range(nc):
        at += 8 + struct.unpack_from("<I", proof, at + 4)[0]
    at += 96
    for _ in range(nc):
        at += 4
        for _ in range(6):
            at += 4 + 16 * struct.unpack_from("<I", proof, at)[0]
        counts.append(struct.unpack_from("<I", proof, at)[0])
        at += 4 + 68 * counts[-1] + 16  # each chunk: its width word and 4 EF; then the cumulative sum
    return counts


def ref_quotient(mirror, lookups_prog, main, perm, alpha, beta, cumsum, quot_alpha, D):
    """chip_cases.ref_quotient on 3 H_(D n) for a chip without preprocessed columns: Q(3 w_(Dn)^i),
    i < D n, as 4-lists; every input canonical."""
    n = len(main)
    (kind, send, mult, vals), = C._parse(lookups_prog)  # one interaction: one single batch
    cols = [[C.interpolate([row[c] for row in m], n) for c in range(len(m[0]))] for m in (main, perm)]
    wq, wn = C.two_adic_gen((D * n).bit_length() - 1), C.two_adic_gen(n.bit_length() - 1)
    wn_inv = pow(wn, P - 2, P)
    bp = [[1, 0, 0, 0], beta, L.ef_mul(beta, beta)]
    out = []
    for i in range(D * n):
        x = 3 * pow(wq, i, P) % P
        zh = (pow(x, n, P) - 1) % P
        assert zh, "Z_H vanishes on the quotient domain"
        first = zh * pow((x - 1) % P, P - 2, P) % P
        last = zh * pow((x - wn_inv) % P, P - 2, P) % P
        trans = (x - wn_inv) % P
        m, pm = ([C.evaluate(c, x) for c in cs] for cs in cols)
        mn, pmn = ([C.evaluate(c, x * wn % P) for c in cs] for cs in cols)
        cons = [[v % P, 0, 0, 0] for v in mirror(m, mn, first, last, trans)]

        def ev(vc):
            return (vc[0] + sum(wt * m[c] for _, c, wt in vc[1])) % P

        den = L.ef_add(alpha, [kind, 0, 0, 0])
        for v, vc in enumerate(vals):
            den = L.ef_add(den, C.ef_scale(bp[v + 1], ev(vc)))
        m0 = ev(mult) if send else -ev(mult) % P
        cons.append(C.ef_sub(L.ef_mul(den, pm[0:4]), [m0, 0, 0, 0]))
        cons.append(C.ef_scale(C.ef_sub(pm[4:8], pm[0:4]), first))
        cons.append(C.ef_scale(C.ef_sub(C.ef_sub(pmn[4:8], pm[4:8]), pmn[0:4]), trans))
        cons.append(C.ef_scale(C.ef_sub(pm[4:8], cumsum), last))
        acc = [0] * 4
        for c in cons:  # the folder's Horner step, acc = acc alpha + c
            acc = L.ef_add(L.ef_mul(acc, quot_alpha), c)
        out.append(C.ef_scale(acc, pow(zh, P - 2, P)))
    return out
