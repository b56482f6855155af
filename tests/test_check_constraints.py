"""The per-constraint failure profile without a device (on_device = 0): counts and first rows
against the plain evaluation of the program, the summary against the first-fail calls, the
compiled chips against their exported programs, and the refusals."""
import pytest

import check_constraints_cases as C


@pytest.mark.parametrize("name,height", C.CASES, ids=[f"{p}-{h}" for p, h in C.CASES])
def test_host_profile_equals_the_reference(name, height):
    C.check_case(name, height, on_device=False)


def test_host_refusals_are_the_first_fail_calls():
    for label, new, old in C.refusals(0):
        assert new[0] < 0 and new == old, label
