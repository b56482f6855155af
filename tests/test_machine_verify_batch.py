"""CPU tests of bfz_machine_verify_batch: the host path (on_device = 0) against Machine.verify on
the oracle's hello proof, the host side of the device path under the stand-in for its kernels, and
the argument checks."""
import os
import subprocess
import sys

import pytest

import bincode_ref as BR
import machine_cases as M
import oracle_lib as O
from bfz import _lib, guests


@pytest.fixture(scope="module")
def machine():
    return M.builtin_machine(guests.HELLO, verifier_only=True)


@pytest.fixture(scope="module")
def proofs():
    hello = O.prove(guests.HELLO, [])
    model = BR.parse_bfz1(hello)
    word = model["opened"][0]["main_local"][0]
    word[0] = (word[0] + 1) % O.P
    return [hello, BR.encode_bfz1(model), hello[: len(hello) // 3]]


def _single(machine, proofs):
    want = []
    for pf in proofs:
        ch = machine.observe()
        o = machine.verify(pf, ch)
        want.append(((o.ok, o.query, o.why), bytes(ch)))
    return want


@pytest.mark.parametrize("standin", [False, True], ids=["host", "device-path-host-side"])
def test_batch_equals_verify_proof_by_proof(machine, proofs, standin):
    """standin: on_device = 1 with a stand-in that reports no failure in the kernels' place, so the
    stages and the packing of the device path run here; none of the three proofs fails in a query."""
    want = _single(machine, proofs)
    assert [w[0][0] for w in want] == [True, False, False]
    assert want[1][0][2].startswith("OOD evaluation mismatch on chip")
    chs = [machine.observe() for _ in proofs]
    try:
        _lib.check(_lib.lib().bfz_set_fault_injection(2 if standin else 0))
        out = machine.verify_batch(proofs, chs, on_device=standin)
    finally:
        _lib.check(_lib.lib().bfz_set_fault_injection(0))
    assert [((o.ok, o.query, o.why), bytes(c)) for o, c in zip(out, chs)] == want
    assert machine.verify_batch([], on_device=False) == []


def test_device_path_without_a_device_is_an_error():
    """A fresh process that never binds a device (another test of this session may have)."""
    code = ("import machine_cases as M, oracle_lib as O\n"
            "from bfz import _lib, guests\n"
            "m = M.builtin_machine(guests.HELLO, verifier_only=True)\n"
            "try:\n"
            "    m.verify_batch([O.prove(guests.HELLO, [])], on_device=True)\n"
            "except _lib.BfzError as e:\n"
            "    print('refused:', e)\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, PYTHONPATH=":".join(sys.path)))
    assert r.returncode == 0, r.stderr
    assert "refused:" in r.stdout and "no device bound" in r.stdout
