"""The per-constraint failure profile on the device (k_profile_prog, k_profile_air<CHIP>): counts
and first rows against the plain evaluation of the program and against the host path, the summary
against the first-fail kernels, a record's trace profiled in place, and the refusals.

Heights and programs (check_constraints_cases): a trace smaller than a wave, one wave, one block,
two blocks; 1 to 512 constraints; every lane failing every constraint."""
import pytest

import check_constraints_cases as C
import uni_device_cases as U
from bfz import _lib, guests, sdk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.init(0)


@pytest.mark.parametrize("name,height", C.CASES, ids=[f"{p}-{h}" for p, h in C.CASES])
def test_device_profile_equals_the_reference_and_the_host(name, height):
    assert C.check_case(name, height, on_device=True) == C.check_case(name, height, on_device=False)


@pytest.mark.parametrize("chip,prog,height", [(U.JUMP, guests.HELLO, 32), (U.CPU, guests.HELLO, 512)])
def test_record_profile_equals_the_host_trace_profile(chip, prog, height):
    trace = U.trace_of(chip, prog)
    assert trace.shape[0] == height
    client = sdk.ProverClient()
    pk, _ = client.setup(prog)
    res, counts, first = client.uni_stark_check_constraints_record(pk, [], chip)
    want, wcounts, wfirst = sdk.uni_stark_check_constraints(chip, trace, on_device=True)
    assert U.summary(res) == U.summary(want)
    assert (counts.tolist(), first.tolist()) == (wcounts.tolist(), wfirst.tolist())


def test_record_without_the_chip():
    client = sdk.ProverClient()
    pk, _ = client.setup("+")
    assert client.uni_stark_check_constraints_record(pk, [], U.IO) is None


def test_device_refusals_are_the_first_fail_calls():
    for label, new, old in C.refusals(1):
        assert new[0] < 0 and new == old, label
