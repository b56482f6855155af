"""A plain numpy model of the NTT / coset LDE over KoalaBear and the edge columns of the NTT
tests (test_ntt_reference.py pins the model to the oracle; test_ntt_paths_gpu.py uses it for the
coefficients the sharded LDE stores, which the oracle does not expose).

Canonical values in uint64 arrays: a product of two values below p is below 2^62.
"""
import numpy as np

P = 0x7F000001
TWO_ADICITY = 24
SENTINEL = 0xFFFFFFFF  # what the test hooks leave in a word no kernel wrote (no field word)
_P = np.uint64(P)


def two_adic_gen(bits: int) -> int:
    """w_(2^bits): the generator 3^((p-1)/2^24) of the 2^24-th roots, squared down."""
    return pow(pow(3, (P - 1) >> TWO_ADICITY, P), 1 << (TWO_ADICITY - bits), P)


def mont(a):
    return ((np.asarray(a, dtype=np.uint64) << np.uint64(32)) % _P).astype(np.uint32)


def unmont(a):
    inv = np.uint64(pow(2, -32, P))
    return ((np.asarray(a, dtype=np.uint64) * inv) % _P).astype(np.uint32)


def powers(base: int, count: int):
    """[base^0, .., base^(count-1)] by doubling."""
    out = np.ones(count, dtype=np.uint64)
    k, bk = 1, base % P
    while k < count:
        m = min(k, count - k)
        out[k:k + m] = (out[:m] * np.uint64(bk)) % _P
        bk = bk * bk % P
        k *= 2
    return out


def bitrev_perm(logn: int):
    idx = np.zeros(1 << logn, dtype=np.int64)
    for b in range(logn):
        idx |= ((np.arange(1 << logn, dtype=np.int64) >> b) & 1) << (logn - 1 - b)
    return idx


def dif(x, root: int):
    """Radix-2 decimation in frequency of the columns of x (n x w, natural rows) with the n-th
    root `root`: row bitrev(k) of the result is sum_i x_i root^(i k)."""
    a = np.array(x, dtype=np.uint64, copy=True)
    n, w = a.shape
    if n == 1:
        return a
    tw = powers(root, n // 2)
    h = n // 2
    while h >= 1:
        v = a.reshape(n // (2 * h), 2, h, w)
        t = tw[:: n // (2 * h)][:h].reshape(1, h, 1)
        lo, hi = v[:, 0], v[:, 1]
        s = lo + hi
        d = ((lo + _P - hi) * t) % _P
        v[:, 0] = s - _P * (s >= _P)
        v[:, 1] = d
        h //= 2
    return a


def n_coefficients(evals):
    """n * (coefficients of the interpolant of the columns over H_n), natural order: the inverse
    DFT without its 1/n, the contract of the device's lde_coefficients."""
    x = np.asarray(evals, dtype=np.uint64)
    n = x.shape[0]
    logn = n.bit_length() - 1
    winv = pow(two_adic_gen(logn), P - 2, P)
    return dif(x, winv)[bitrev_perm(logn)].astype(np.uint32)


def first_pass(evals, b1: int):
    """The inverse DFT's first pass, natural-order evaluations in: its DIT stages [0, b1) over the
    bit-reversed rows, i.e. an unscaled size-2^b1 inverse DFT of every run of 2^b1 consecutive
    bit-reversed rows (natural order out).  The sharded LDE's fused path keeps this intermediate in
    the coefficient buffer and overwrites only the rank's range with coefficients."""
    x = np.asarray(evals, dtype=np.uint64)
    n, w = x.shape
    logn = n.bit_length() - 1
    T = 1 << b1
    rev = bitrev_perm(b1)
    t = x[bitrev_perm(logn)].reshape(n // T, T, w).transpose(1, 0, 2).reshape(T, -1)
    out = dif(t[rev], pow(two_adic_gen(b1), P - 2, P))[rev]
    return out.reshape(T, n // T, w).transpose(1, 0, 2).reshape(n, w).astype(np.uint32)


def coset_lde_from_coefficients(ncoef, shift: int):
    """Evaluations of the interpolant on shift * H_2n, bit-reversed rows, from n * coefficients."""
    c = np.asarray(ncoef, dtype=np.uint64)
    n, w = c.shape
    logn = n.bit_length() - 1
    scale = (powers(shift, n) * np.uint64(pow(n, P - 2, P))) % _P
    pad = np.zeros((2 * n, w), dtype=np.uint64)
    pad[:n] = (c * scale.reshape(n, 1)) % _P
    return dif(pad, two_adic_gen(logn + 1)).astype(np.uint32)


EDGE_NAMES = ("zero", "one", "p-1", "(p-1)/2", "(p+1)/2", "alt(p-1,0)", "alt(a,p-a)", "imp@0",
              "imp@1", "imp@n/2", "imp@n-1", "w_n^i", "(-1)^i", "random")


def edge_columns(logn: int, seed: int):
    """The 14 edge columns as device (Montgomery) words, n x 14, natural row order: constants,
    alternating extremes, impulses of p-1, the geometric columns w_n^i and (-1)^i (Montgomery words
    of those values: their inverse DFT is one impulse) and one random column."""
    n = 1 << logn
    a = 0x12345678 % P
    i = np.arange(n)
    cols = [np.full(n, v, dtype=np.uint64) for v in (0, 1, P - 1, (P - 1) // 2, (P + 1) // 2)]
    cols.append(np.where(i % 2 == 0, P - 1, 0).astype(np.uint64))
    cols.append(np.where(i % 2 == 0, a, P - a).astype(np.uint64))
    for row in (0, 1, n // 2, n - 1):
        c = np.zeros(n, dtype=np.uint64)
        c[row % n] = P - 1
        cols.append(c)
    cols.append(mont(powers(two_adic_gen(logn), n)).astype(np.uint64))
    cols.append(mont(np.where(i % 2 == 0, 1, P - 1)).astype(np.uint64))
    cols.append(np.random.default_rng(seed).integers(0, P, size=n, dtype=np.uint64))
    assert len(cols) == len(EDGE_NAMES)
    return np.stack(cols, axis=1).astype(np.uint32)
