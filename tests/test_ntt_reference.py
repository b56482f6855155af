"""The numpy NTT model of ntt_cases.py against the oracle: the coset LDE computed from the
model's n * coefficients is the oracle's coset_lde, so the coefficient reference of
test_ntt_paths_gpu.py does not depend on the code under test."""
import numpy as np
import pytest

import ntt_cases as N
import oracle_lib as O

P = N.P


def test_model_constants_match_oracle():
    assert N.P == O.P
    for bits in range(0, 25):
        assert N.two_adic_gen(bits) == O.two_adic_gen(bits)


def test_direct_evaluation_16_rows():
    """The model against the definition: n * c_k = sum_i x_i w^(-i k), and the LDE row
    bitrev(i) = sum_k c_k (s w_2n^i)^k."""
    rng = np.random.default_rng(16)
    n, s = 16, 3
    x = rng.integers(0, P, size=(n, 2), dtype=np.uint64).astype(np.uint32)
    nc = N.n_coefficients(x)
    winv = pow(N.two_adic_gen(4), P - 2, P)
    for col in range(2):
        for k in range(n):
            assert int(nc[k, col]) == sum(int(x[i, col]) * pow(winv, i * k, P) for i in range(n)) % P
    lde = N.coset_lde_from_coefficients(nc, s)
    ninv, w2n, rev = pow(n, P - 2, P), N.two_adic_gen(5), N.bitrev_perm(5)
    for col in range(2):
        for i in range(2 * n):
            pt = s * pow(w2n, i, P) % P
            want = sum(int(nc[k, col]) * ninv % P * pow(pt, k, P) for k in range(n)) % P
            assert int(lde[rev[i], col]) == want


@pytest.mark.parametrize("logn", range(0, 13))
def test_model_lde_matches_oracle(logn):
    n = 1 << logn
    rng = np.random.default_rng(900 + logn)
    words = N.edge_columns(logn, seed=logn)
    m = N.unmont(words)
    nc = N.n_coefficients(m)
    w2n_inv = pow(N.two_adic_gen(logn + 1), P - 2, P)
    for shift in (1, 3, w2n_inv, int(rng.integers(2, P))):
        assert np.array_equal(N.coset_lde_from_coefficients(nc, shift), O.coset_lde(m, shift)), shift


def test_first_pass_model():
    """One tile is the whole inverse DFT; with tiles of 2^b1 rows, finishing the DIT (stages b1 and
    up, written out here) gives the same coefficients."""
    logn, b1 = 7, 4
    n = 1 << logn
    m = N.unmont(N.edge_columns(logn, seed=3))
    nc = N.n_coefficients(m)
    assert np.array_equal(N.first_pass(m, logn), nc)
    a = N.first_pass(m, b1).astype(np.uint64)
    for t in range(b1, logn):
        h = 1 << t
        tw = N.powers(pow(N.two_adic_gen(t + 1), P - 2, P), h).reshape(1, h, 1)
        v = a.reshape(n // (2 * h), 2, h, -1)
        u, vw = v[:, 0].copy(), (v[:, 1] * tw) % np.uint64(P)
        v[:, 0] = (u + vw) % np.uint64(P)
        v[:, 1] = (u + np.uint64(P) - vw) % np.uint64(P)
    assert np.array_equal(a.astype(np.uint32), nc)


def test_edge_columns_are_what_they_name():
    logn = 5
    n = 1 << logn
    words = N.edge_columns(logn, seed=1)
    assert words.shape == (n, 14) and words.dtype == np.uint32 and int(words.max()) < P
    nc = N.n_coefficients(N.unmont(words))
    names = list(N.EDGE_NAMES)
    # the geometric columns' inverse DFTs are single impulses of n (at k = 1 and k = n/2)
    for name, k in (("w_n^i", 1), ("(-1)^i", n // 2)):
        col = nc[:, names.index(name)]
        assert int(col[k]) == n and np.count_nonzero(col) == 1
    assert words[:, names.index("p-1")].tolist() == [P - 1] * n
    assert words[n // 2, names.index("imp@n/2")] == P - 1
