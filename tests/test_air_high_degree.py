"""AIR programs of constraint degree 4 to 9 without a device: the opt-in cap
(bfz_set_air_max_degree), the shapes bfz_air_info reports under it, what stays refused, and the
host row check against the Python mirrors of tests/air_high_degree_cases.py."""
import numpy as np
import pytest

import air_high_degree_cases as H
import air_program_cases as A
from bfz import sdk

REFUSAL = "uni_stark: constraint degree above 3 is not supported"


@pytest.fixture(autouse=True)
def default_cap():
    yield
    sdk.set_air_max_degree(0)


def monomial(degree):
    """One constraint of that degree over one column: x^d, or is_first_row x^4 for 5."""
    ab = sdk.AirBuilder(1)
    x = ab.local(0)
    ab.assert_zero(ab.is_first_row * H.power(x, 4) if degree == 5 else H.power(x, degree))
    return ab.build()


@pytest.mark.parametrize("kind", ["chain4", "chain9"])
def test_the_default_cap_refuses_with_todays_message(kind):
    assert A.air_info_status(H.program(kind)) == (-1, REFUSAL)
    sdk.set_air_max_degree(9)
    sdk.set_air_max_degree(0)  # back to the default
    assert A.air_info_status(H.program(kind)) == (-1, REFUSAL)


@pytest.mark.parametrize("degree,lqd", [(4, 2), (5, 2), (6, 3), (9, 3)])
def test_a_raised_cap_reports_the_shape(degree, lqd):
    sdk.set_air_max_degree(9)
    info = sdk.air_info(monomial(degree))
    assert (info.degree, info.log_quotient_degree) == (degree, lqd)
    sdk.set_air_max_degree(degree)  # the cap is a degree: exactly enough, then one too few
    assert sdk.air_info(monomial(degree)).degree == degree
    if degree > 4:
        sdk.set_air_max_degree(degree - 1)
        assert A.air_info_status(monomial(degree)) == \
            (-1, f"uni_stark: constraint degree above {degree - 1} is not supported")


def test_what_stays_refused():
    import chip_cases as C
    sdk.set_air_max_degree(9)
    assert A.air_info_status(monomial(10)) == \
        (-1, "uni_stark: constraint degree above 9 is not supported")
    for bad in (2, 10, -1):
        with pytest.raises(sdk.BfzError, match="max degree"):
            sdk.set_air_max_degree(bad)
    assert sdk.air_info(H.program("chain9")).log_quotient_degree == 3  # a refused value changed nothing
    # chip programs keep their own limit (mulgate's lookups are over 4 columns: widen chain4)
    ab = sdk.AirBuilder(4)
    ab.assert_zero(ab.local(1) - H.power(ab.local(0), 4))
    with pytest.raises(sdk.BfzError, match=r"chip program: AIR degree 4 is above 3"):
        sdk.chip_info(ab.build(), C.mulgate_lookups())


@pytest.mark.parametrize("kind,height", [("chain4", 1), ("chain4", 64), ("chain9", 2), ("chain9", 64)])
def test_host_row_check_agrees_with_the_mirror(kind, height):
    sdk.set_air_max_degree(9)
    prog, mirror, trace, rows = H.case(kind, height)
    assert sdk.air_info(prog).log_quotient_degree == H.LQD[kind]
    assert not (A.mirror_rows(mirror, rows) >= 0).any()
    assert A.summary(sdk.air_check(prog, trace, on_device=False)) == (-1, height, 4, 0, -1, -1)
    r = height // 2
    bad = A.flip(trace, r, 1)
    want = A.mirror_rows(mirror, A.canonical(bad))
    assert want[r] == 0  # y - x^k, the first constraint, on the changed row
    got = sdk.air_check(prog, bad, on_device=False, per_row=True)
    assert np.array_equal(got.first_fail_per_row, want)
    assert A.summary(got) == A.summary_from_rows(want, 4)
    # per constraint: the changed y also breaks the step to the next row, unless the row is the last
    summary, counts, first_rows = sdk.air_check_constraints(prog, bad, on_device=False)
    assert A.summary(summary) == A.summary(got)
    assert list(counts) == [1, int(r != height - 1), 0, 0] and first_rows[0] == r
