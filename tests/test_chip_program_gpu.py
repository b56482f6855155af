"""Caller-defined chips as pairs of programs, device paths: k_check_chip_prog against the host
path, k_quotient_chip_prog against the compiled k_quotient<CHIP> word for word and against the
plain Python reference of chip_cases."""
import numpy as np
import pytest

import chip_cases as C
from bfz import sdk

pytestmark = pytest.mark.gpu
CHIP_HEIGHTS = [(c, h) for c in range(8) for h in C.HEIGHTS]


@pytest.mark.parametrize("chip,height", CHIP_HEIGHTS)
def test_device_check_matches_host(chip, height):
    air, lk, info = C.exported(chip)
    main, prep = C.random_traces(chip, height)
    alpha, beta, _ = C.challenges(chip + 1)
    perm, cs = sdk.lookups_perm_trace(lk, main, prep, alpha, beta)
    r, phi = height // 2, 4 * (info.perm_width - 1)
    for m, pm in ((main, perm), (C.flip(main, r, 0), perm), (main, C.flip(perm, r, phi))):
        dev = sdk.chip_check(air, lk, m, prep, pm, alpha, beta, cs, on_device=True, per_row=True)
        host = sdk.chip_check(air, lk, m, prep, pm, alpha, beta, cs, on_device=False, per_row=True)
        assert dev.chip == host.chip == -1
        C.same_check(dev, host)


@pytest.mark.parametrize("chip,height", CHIP_HEIGHTS)
def test_quotient_matches_compiled_kernel(chip, height):
    """Seeded random traces: the values are no polynomial's, and every constraint is not zero."""
    air, lk, info = C.exported(chip)
    main, prep = C.random_traces(chip, height)
    alpha, beta, qa = C.challenges(chip + 1)
    rng = np.random.default_rng([chip, height, 5])
    perm = C.mont(rng.integers(0, C.P, size=(height, 4 * info.perm_width)))
    cs = C.mont(rng.integers(0, C.P, 4)).tolist()
    for pm, c in ((None, None), (perm, cs)):  # the device's permutation trace; the caller's
        q, cs_p = sdk.chip_quotient(air, lk, main, prep, alpha, beta, qa, perm=pm, cumsum=c)
        want, cs_c = sdk.chip_quotient(None, None, main, prep, alpha, beta, qa, perm=pm, cumsum=c,
                                       chip=chip)
        assert cs_p == cs_c
        assert np.array_equal(q, want)


def canonical_case(kind, n, seed):
    """A custom chip's inputs as the library takes them and as canonical integers."""
    air, mirror, lk, main, prep = C.custom_case(kind, n)
    ch = C.challenges(seed)
    perm, cs = sdk.lookups_perm_trace(lk, main, prep, ch[0], ch[1])
    can = lambda a: None if a is None else C.unmont(a).tolist()  # noqa: E731
    return air, mirror, lk, main, prep, perm, cs, ch, can


@pytest.mark.parametrize("n", [2, 4, 16])
@pytest.mark.parametrize("kind", ["mulgate", "prep"])
def test_quotient_matches_reference(kind, n):
    air, mirror, lk, main, prep, perm, cs, ch, can = canonical_case(kind, n, 40 + n)
    # the reference itself: no zero denominator on the trace rows, Z_H != 0 on 3 H_2n (asserted
    # inside ref_perm_trace and ref_quotient), and its permutation trace is the library's
    rows, ref_cs = C.L.ref_perm_trace(lk, can(main), can(prep), can(ch[0]), can(ch[1]))
    assert np.array_equal(rows, C.unmont(perm)) and ref_cs == can(cs)
    want = C.ref_quotient(mirror, lk, can(main), can(prep), can(perm), can(ch[0]), can(ch[1]),
                          can(cs), can(ch[2]))
    q, _ = sdk.chip_quotient(air, lk, main, prep, ch[0], ch[1], ch[2], perm=perm, cumsum=cs)
    assert C.unmont(q).tolist() == want
    q, cs_dev = sdk.chip_quotient(air, lk, main, prep, ch[0], ch[1], ch[2])
    assert C.unmont(q).tolist() == want and cs_dev == cs


@pytest.mark.parametrize("n", [4, 16])
def test_check_and_quotient_agree(n):
    """A valid trace passes the row check and its quotient is a polynomial; one flipped cell
    fails both.  Degrees: the columns have degree <= n - 1, every constraint degree <= 3 and the
    selector-times-difference constraints 2 (n - 1), so C has degree <= 3 n - 3 and Q = C / Z_H
    degree <= 2 n - 3: the two top coefficients of the interpolant of degree < 2 n over 3 H_2n
    are zero exactly then (a C that Z_H does not divide leaves them arbitrary)."""
    air, _, lk, main, prep, perm, cs, ch, _ = canonical_case("mulgate", n, 60 + n)
    zero = [[0] * 4] * 2
    res = sdk.chip_check(air, lk, main, prep, perm, ch[0], ch[1], cs, per_row=True)
    assert res.failing_rows == 0
    q, _ = sdk.chip_quotient(air, lk, main, prep, ch[0], ch[1], ch[2], perm=perm, cumsum=cs)
    assert C.top_coefficients(C.unmont(q), n) == zero
    bad = C.flip(main, 1, 2)  # c of a real row: the gate, and the batch that receives c
    res = sdk.chip_check(air, lk, bad, prep, perm, ch[0], ch[1], cs, per_row=True)
    assert (res.failing_rows, res.first_row, res.first_constraint) == (1, 1, 1)
    q, _ = sdk.chip_quotient(air, lk, bad, prep, ch[0], ch[1], ch[2], perm=perm, cumsum=cs)
    assert C.top_coefficients(C.unmont(q), n) != zero
