"""The chip degree cap (set_chip_max_degree) and the shape of chips of AIR degree 4 to 9, on the host."""
import pytest

import chip_high_degree_cases as H
import machine_cases as M
from bfz import _lib, sdk


@pytest.fixture(autouse=True)
def default_caps():
    yield
    sdk.set_chip_max_degree(0)
    sdk.set_air_max_degree(0)


@pytest.mark.parametrize("air_cap,why", [
    (0, "uni_stark: constraint degree above 3 is not supported"),
    (9, r"chip program: AIR degree 4 is above 3 \(log quotient degree 1\)")])
def test_default_cap_refuses_as_before(air_cap, why):
    sdk.set_air_max_degree(air_cap)
    with pytest.raises(_lib.BfzError, match=why):
        sdk.chip_info(*H.pow_chip(4)[:2])


@pytest.mark.parametrize("k,lqd", [(4, 2), (9, 3)])
def test_raised_cap(k, lqd):
    air, lk, _ = H.pow_chip(k)
    sdk.set_chip_max_degree(9)
    info = sdk.chip_info(air, lk)
    assert (info.degree, info.log_quotient_degree) == (k, lqd)
    assert (info.air_constraints, info.num_constraints) == (2, 6)
    sdk.set_chip_max_degree(k)  # the cap itself is accepted, whatever the AIR cap
    assert sdk.chip_info(air, lk).degree == k
    sdk.set_chip_max_degree(k - 1)
    sdk.set_air_max_degree(9)  # (at the default chip cap, 3, the AIR path's own cap would speak first)
    cap_lqd = 1 if k == 4 else 3
    with pytest.raises(_lib.BfzError, match=rf"chip program: AIR degree {k} is above {k - 1} "
                                            rf"\(log quotient degree {cap_lqd}\)"):
        sdk.chip_info(air, lk)


def test_lookup_only_chip_and_bad_caps():
    sdk.set_chip_max_degree(9)
    info = sdk.chip_info(None, M.table_lookups())
    assert (info.degree, info.log_quotient_degree) == (3, 1)
    for bad in (-1, 1, 2, 10):
        with pytest.raises(_lib.BfzError, match="chip max degree"):
            sdk.set_chip_max_degree(bad)
    assert sdk.chip_info(*H.pow_chip(9)[:2]).degree == 9  # a refused value changes nothing
