"""Caller-defined chips as pairs of programs, host paths: bfz_chip_info and bfz_chip_check_rows
(on_device = 0) against the built-in chips' compiled row check."""
import numpy as np
import pytest

import chip_cases as C
from bfz import _lib, sdk


@pytest.mark.parametrize("chip", range(8))
def test_host_check_matches_builtin(chip):
    air, lk, info = C.exported(chip)
    main, prep = C.hello_traces(chip)
    alpha, beta, _ = C.challenges(chip + 1)
    perm, cs = sdk.lookups_perm_trace(lk, main, prep, alpha, beta, on_device=False)
    assert info.perm_width == sdk.lookups_info(lk).perm_width
    h, phi = main.shape[0], 4 * (info.perm_width - 1)
    cases = {"clean": (main, perm), "main": (C.flip(main, h // 2, 0), perm),
             "phi": (main, C.flip(perm, h // 2, phi))}
    got = {}
    for name, (m, pm) in cases.items():
        got[name] = sdk.chip_check(air, lk, m, prep, pm, alpha, beta, cs, on_device=False, per_row=True)
        want = sdk.check_chip(chip, m, prep, pm, alpha, beta, cs, on_device=False, per_row=True)
        assert got[name].chip == -1 and info.num_constraints == want.num_constraints
        C.same_check(got[name], want)
    if got["clean"].failing_rows == 0:  # a hello trace: the running sum's cell is seen
        assert got["phi"].failing_rows > 0
        assert got["phi"].first_constraint >= info.num_constraints - 3


def test_chip_info_refusals():
    mul_air = C.A.mulgate_program()
    with pytest.raises(_lib.BfzError, match="width"):
        sdk.chip_info(mul_air, C.prep_lookups())
    with pytest.raises(_lib.BfzError, match="bfz_air_"):
        sdk.chip_info(mul_air, sdk.LookupBuilder(4).program())
    ab = sdk.AirBuilder(4)
    ab.assert_zero(ab.local(0) * ab.local(1) * ab.local(2) * ab.local(3))
    with pytest.raises(_lib.BfzError, match="degree"):
        sdk.chip_info(ab.build(), C.mulgate_lookups())
    info = sdk.chip_info(mul_air, C.mulgate_lookups())
    assert (info.air_constraints, info.num_constraints, info.perm_width, info.log_quotient_degree) == (3, 8, 3, 1)
    assert sdk.chip_info(None, C.prep_lookups()).num_constraints == 4
