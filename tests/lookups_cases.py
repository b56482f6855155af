"""Shared by tests/test_lookups.py and tests/test_lookups_gpu.py: seeded interaction programs and a
plain Python-integer reference of generate_permutation_trace (permutation.rs:75-148) over
Fp and Fp[x] / (x^4 - 3), canonical integers throughout."""
import functools
import struct

import numpy as np

from bfz import sdk

P = 0x7F000001
R_INV = pow(1 << 32, P - 2, P)


def mont(a):
    return ((np.asarray(a, dtype=np.uint64) << np.uint64(32)) % np.uint64(P)).astype(np.uint32)


def unmont(a):
    return (np.asarray(a, dtype=np.uint64) * np.uint64(R_INV) % np.uint64(P)).astype(np.uint32)


def ef_add(a, b):
    return [(x + y) % P for x, y in zip(a, b)]


def ef_mul(a, b):
    c = [0] * 8
    for i in range(4):
        for j in range(4):
            c[i + j] += a[i] * b[j]
    return [(c[k] + 3 * c[k + 4]) % P for k in range(4)]


def ef_inv(a):
    """a = A + x B over Fp[y] / (y^2 - 3), y = x^2: 1 / a = (A - x B) / (A^2 - y B^2)."""
    a0, a1, a2, a3 = a
    c0 = (a0 * a0 + 3 * a2 * a2 - 6 * a1 * a3) % P  # A^2 - y B^2 = c0 + c1 y
    c1 = (2 * a0 * a2 - a1 * a1 - 3 * a3 * a3) % P
    n = pow((c0 * c0 - 3 * c1 * c1) % P, P - 2, P)
    return ef_mul([a0, -a1 % P, a2, -a3 % P], [c0 * n % P, 0, -c1 * n % P, 0])


def ref_perm_trace(prog, main, prep, alpha, beta):
    """(rows, cumsum): rows[r] = the flattened permutation row.  Reads the BFL1 words itself.
    Asserts that no denominator is zero (the library does not detect one)."""
    w = struct.unpack(f"<{len(prog) // 4}I", prog)
    n, at = w[3], 4
    chain = []

    def vcol():
        nonlocal at
        c, nt = w[at] * R_INV % P, w[at + 1]
        terms = [(w[at + 2 + 3 * i], w[at + 3 + 3 * i], w[at + 4 + 3 * i] * R_INV % P) for i in range(nt)]
        at += 2 + 3 * nt
        return c, terms

    for _ in range(n):
        kind, send, nv = w[at:at + 3]
        at += 3
        chain.append((kind, send, vcol(), [vcol() for _ in range(nv)]))
    bp = [[1, 0, 0, 0]]
    for _ in range(7):
        bp.append(ef_mul(bp[-1], beta))
    rows, phi = [], [0] * 4
    for r in range(len(main)):
        m, pr = [int(x) for x in main[r]], [int(x) for x in prep[r]] if prep is not None else None

        def ev(vc):
            return (vc[0] + sum(wt * (pr if s else m)[c] for s, c, wt in vc[1])) % P

        fr = []
        for kind, send, mult, vals in chain:
            den = ef_add(alpha, [kind, 0, 0, 0])
            for v, vc in enumerate(vals):
                den = ef_add(den, [x * ev(vc) % P for x in bp[v + 1]])
            assert any(den), "the seed hit a zero denominator"
            mu = ev(mult) if send else -ev(mult) % P
            fr.append([x * mu % P for x in ef_inv(den)])
        row = [ef_add(fr[j], fr[j + 1]) if j + 1 < n else fr[j] for j in range(0, n, 2)]
        for v in row:
            phi = ef_add(phi, v)
        rows.append([x for v in row + [phi] for x in v])
    return np.array(rows, dtype=np.uint32), phi


# (interactions, sends among them, values per interaction (cycled), terms per value (cycled), height)
CASES = {
    "single-const-h1": (1, 1, (0,), (0,), 1),          # alpha + kind alone; the row is its own scan
    "pair-h2": (2, 1, (7,), (8,), 2),
    "trailing-single-h256": (3, 2, (7, 0), (8, 0, 1), 256),  # one block
    "lds-file-full-h256": (32, 20, (7, 0, 3), (8, 1), 256),
    "receive-only-h256": (2, 0, (0, 7), (8,), 256),
    "scan-tiles-h8192": (3, 1, (7, 0), (0, 8), 1 << 13),     # 32 blocks, 4 scan tiles
}
MAIN_W, PREP_W = 9, 5


@functools.lru_cache(maxsize=None)
def case(name):
    """(program, main, prep, alpha, beta, expected rows, expected cumsum), canonical integers; the
    traces are drawn from a fixed seed, with multiplicity 0 in every third row."""
    n, sends, nvals, nterms, h = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 1)
    b = sdk.LookupBuilder(MAIN_W, PREP_W)
    cols = [b.main(c) for c in range(MAIN_W)] + [b.prep(c) for c in range(PREP_W)]
    k = 0
    for j in range(n):
        values = []
        for _ in range(nvals[j % len(nvals)]):
            nt = nterms[k % len(nterms)]
            k += 1
            pick = rng.choice(len(cols), size=nt, replace=False)  # both sources among 8 of 14
            values.append(sum((int(rng.integers(1, P)) * cols[c] for c in pick), int(rng.integers(0, P))))
        mult = 3 if n == 1 else b.main(0) * (j + 1)
        (b.send if j < sends else b.receive)(int(rng.integers(1, 8)), values, mult)
    main = rng.integers(0, P, size=(h, MAIN_W), dtype=np.uint32)
    main[::3, 0] = 0
    prep = rng.integers(0, P, size=(h, PREP_W), dtype=np.uint32)
    alpha, beta = ([int(x) for x in rng.integers(0, P, 4)] for _ in range(2))
    prog = b.program()
    return (prog, main, prep, alpha, beta) + ref_perm_trace(prog, main, prep, alpha, beta)


def run_case(name, on_device):
    """The library's (rows, cumsum) of a case, canonical."""
    prog, main, prep, alpha, beta, _, _ = case(name)
    perm, cs = sdk.lookups_perm_trace(prog, mont(main), mont(prep), mont(alpha), mont(beta), on_device)
    return unmont(perm), unmont(cs).tolist()
