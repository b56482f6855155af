"""Shared by tests/test_chip_program.py (host paths) and tests/test_chip_program_gpu.py (device
paths): the built-in chips as pairs of exported programs, seeded traces, two custom chips, and a
plain Python-integer reference of a chip's machine quotient (quotient_values, quotient.rs:18-165,
under Chip::eval): canonical integers mod p, EF = Fp[x] / (x^4 - 3) as 4-lists."""
import functools
import struct

import numpy as np

import air_program_cases as A
import lookups_cases as L
import oracle_lib as O
from bfz import guests, sdk

P = L.P
mont, unmont = L.mont, L.unmont
HEIGHTS = [1, 4, 512]  # next = own row; a partial block; two blocks (LDE: 2, 8, 1024 points)
LOOKUP_ONLY = (1, 4, 5)  # Program, Memory, Byte: no AIR of their own


@functools.lru_cache(maxsize=None)
def exported(chip):
    """(air or None, lookups, ChipInfo) of a built-in chip."""
    air = None if chip in LOOKUP_ONLY else sdk.air_export(chip)
    lk = sdk.lookups_export(chip)
    return air, lk, sdk.chip_info(air, lk)


def challenges(seed):
    """alpha, beta, quot_alpha as Montgomery words."""
    rng = np.random.default_rng(seed)
    return [mont(rng.integers(1, P, 4)).tolist() for _ in range(3)]


@functools.lru_cache(maxsize=None)
def random_traces(chip, height):
    """(main, prep or None): seeded Montgomery words, read-only."""
    info = exported(chip)[2]
    rng = np.random.default_rng([chip, height])
    out = []
    for w in (info.main_width, info.prep_width):
        t = mont(rng.integers(0, P, size=(height, w))) if w else None
        if t is not None:
            t.setflags(write=False)
        out.append(t)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def hello_traces(chip):
    """The hello guest's (main, prep or None) of a chip as Montgomery words, or seeded random
    traces of 16 rows where hello leaves the chip out."""
    m = O.trace(guests.HELLO, [], chip, False)
    if m is None:
        return random_traces(chip, 16)
    pr = O.trace(guests.HELLO, [], chip, True) if exported(chip)[2].prep_width else None
    return mont(m), None if pr is None else mont(pr)


def flip(trace, row, col):
    """A copy with one cell's canonical value + 1."""
    bad = np.array(trace, dtype=np.uint32)
    bad[row, col] = mont((int(unmont(bad[row, col])) + 1) % P)
    return bad


def same_check(a, b):
    """Two ChipCheckResults agree in everything but the chip index (-1 for a pair of programs)."""
    assert (a.height, a.num_constraints, a.num_batches, a.failing_rows, a.first_row,
            a.first_constraint, a.cumulative_sum) == (
        b.height, b.num_constraints, b.num_batches, b.failing_rows, b.first_row,
        b.first_constraint, b.cumulative_sum)
    assert np.array_equal(a.first_fail_per_row, b.first_fail_per_row)


# ---------------------------------------------------------------------------- two custom chips
def mulgate_lookups():
    """Over mulgate's (a, b, c, s): one send and two receives -- an odd count, so the last batch
    is a single."""
    b = sdk.LookupBuilder(4)
    a_, b_, c_, s_ = (b.main(i) for i in range(4))
    b.send(3, [a_, b_], s_)
    b.receive(3, [c_], s_)
    b.receive(5, [a_ + 2 * b_, 7], s_ * 3)
    return b.program()


def prep_lookups():
    """A lookup-only chip: main (mult, v), one preprocessed column, a 0-value interaction."""
    b = sdk.LookupBuilder(2, 1)
    b.send(4, [], b.main(0))
    b.receive(2, [b.prep(0), b.main(1) + 5], b.main(0))
    return b.program()


@functools.lru_cache(maxsize=None)
def custom_case(kind, n):
    """(air, mirror, lookups, main, prep): a valid mulgate trace, or seeded words for "prep"."""
    if kind == "mulgate":
        air, mirror, t, _ = A.mulgate_case(n)
        return air, mirror, mulgate_lookups(), t, None
    rng = np.random.default_rng([n, 99])
    main, prep = mont(rng.integers(0, P, size=(n, 2))), mont(rng.integers(0, P, size=(n, 1)))
    return None, None, prep_lookups(), main, prep


# ---------------------------------------------------------------------------- the reference
def two_adic_gen(bits):
    return pow(pow(3, 127, P), 1 << (24 - bits), P)


def _parse(prog):
    """[(kind, send, mult, values)], a VCOL as (constant, [(source, column, weight)])."""
    w = struct.unpack(f"<{len(prog) // 4}I", prog)
    at, chain = 4, []

    def vcol():
        nonlocal at
        c, nt = w[at] * L.R_INV % P, w[at + 1]
        terms = [(w[at + 2 + 3 * i], w[at + 3 + 3 * i], w[at + 4 + 3 * i] * L.R_INV % P) for i in range(nt)]
        at += 2 + 3 * nt
        return c, terms

    for _ in range(w[3]):
        kind, send, nv = w[at:at + 3]
        at += 3
        chain.append((kind, send, vcol(), [vcol() for _ in range(nv)]))
    return chain


def interpolate(col, n):
    """Coefficients of the polynomial of degree < n with f(w_n^k) = col[k], naively."""
    winv, ninv = pow(two_adic_gen(n.bit_length() - 1), P - 2, P), pow(n, P - 2, P)
    return [sum(int(col[k]) * pow(winv, j * k, P) for k in range(n)) * ninv % P for j in range(n)]


def evaluate(coef, x):
    return sum(c * pow(x, j, P) for j, c in enumerate(coef)) % P


def ef_sub(a, b):
    return [(x - y) % P for x, y in zip(a, b)]


def ef_scale(a, k):
    return [x * k % P for x in a]


def ref_quotient(air_mirror, lookups_prog, main, prep, perm, alpha, beta, cumsum, quot_alpha):
    """Q(3 w_2n^i), i < 2n, as 4-lists.  Everything canonical: main / prep / perm are integer
    matrices (perm flattened to base columns), the challenges and cumsum 4-lists.  Asserts that
    Z_H does not vanish on the quotient domain."""
    n = len(main)
    chain = _parse(lookups_prog)
    ni, nb = len(chain), (len(chain) + 1) // 2
    cols = [[interpolate([row[c] for row in m], n) for c in range(len(m[0]))] if m is not None else []
            for m in (main, prep, perm)]
    w2n, wn = two_adic_gen(n.bit_length()), two_adic_gen(n.bit_length() - 1)
    wn_inv = pow(wn, P - 2, P)
    bp = [[1, 0, 0, 0]]
    for _ in range(7):
        bp.append(L.ef_mul(bp[-1], beta))
    out = []
    for i in range(2 * n):
        x = 3 * pow(w2n, i, P) % P
        zh = (pow(x, n, P) - 1) % P
        assert zh, "Z_H vanishes on the quotient domain"
        first = zh * pow((x - 1) % P, P - 2, P) % P
        last = zh * pow((x - wn_inv) % P, P - 2, P) % P
        trans = (x - wn_inv) % P
        m, pr, pm = ([evaluate(c, x) for c in cs] for cs in cols)
        mn, pmn = ([evaluate(c, x * wn % P) for c in cs] for cs in (cols[0], cols[2]))
        cons = [[v % P, 0, 0, 0] for v in air_mirror(m, mn, first, last, trans)] if air_mirror else []

        def ev(vc):
            return (vc[0] + sum(wt * (pr if s else m)[c] for s, c, wt in vc[1])) % P

        dm = []
        for kind, send, mult, vals in chain:
            den = L.ef_add(alpha, [kind, 0, 0, 0])
            for v, vc in enumerate(vals):
                den = L.ef_add(den, ef_scale(bp[v + 1], ev(vc)))
            dm.append((den, ev(mult) if send else -ev(mult) % P))
        pl = [pm[4 * b:4 * b + 4] for b in range(nb + 1)]
        pn = [pmn[4 * b:4 * b + 4] for b in range(nb + 1)]
        sum_l, sum_n = [0] * 4, [0] * 4
        for b in range(nb):
            d0, m0 = dm[2 * b]
            if 2 * b + 1 < ni:
                d1, m1 = dm[2 * b + 1]
                cons.append(ef_sub(L.ef_mul(L.ef_mul(d0, d1), pl[b]),
                                   L.ef_add(ef_scale(d1, m0), ef_scale(d0, m1))))
            else:
                cons.append(ef_sub(L.ef_mul(d0, pl[b]), [m0, 0, 0, 0]))
            sum_l, sum_n = L.ef_add(sum_l, pl[b]), L.ef_add(sum_n, pn[b])
        cons.append(ef_scale(ef_sub(pl[nb], sum_l), first))
        cons.append(ef_scale(ef_sub(ef_sub(pn[nb], pl[nb]), sum_n), trans))
        cons.append(ef_scale(ef_sub(pl[nb], cumsum), last))
        acc = [0] * 4
        for c in cons:  # the folder's Horner step, acc = acc alpha + c
            acc = L.ef_add(L.ef_mul(acc, quot_alpha), c)
        out.append(ef_scale(acc, pow(zh, P - 2, P)))
    return out


def top_coefficients(q, n, count=2):
    """The `count` highest coefficients (each a 4-list) of the interpolant of degree < 2n of
    q[i] = Q(3 w_2n^i)."""
    winv, s_inv = pow(two_adic_gen(n.bit_length()), P - 2, P), pow(3, P - 2, P)
    ninv = pow(2 * n, P - 2, P)
    return [[sum(int(q[k][e]) * pow(winv, j * k, P) for k in range(2 * n)) * ninv * pow(s_inv, j, P) % P
             for e in range(4)] for j in range(2 * n - count, 2 * n)]
