"""The uni-STARK additions without a device: the AIR-only row check's host path (bfz_uni_check with
on_device = 0) against the model of tests/uni_stark_model.py and against the merged checker
(bfz_check_chip) on real and corrupted traces, and bfz_uni_verify_batch on the fixture proofs of
tests/golden/uni_stark.json, on the host path and on the host side of the device path (fault-
injection bit 1: a stand-in for the kernels)."""
import ctypes
import json
import os
import struct

import numpy as np
import pytest

import debug_cases as D
import oracle_lib as O
import uni_device_cases as C
import uni_stark_model as M
from bfz import _lib, guests, sdk
from uni_device_cases import ADDSUB, CPU, IO, JUMP, MEMINSTRS

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = json.load(open(os.path.join(HERE, "golden", "uni_stark.json")))


@pytest.fixture(autouse=True)
def defaults():
    try:
        yield
    finally:
        _lib.lib().bfz_set_fault_injection(0)
        sdk.set_num_queries(0)


def check(chip, trace):
    return sdk.uni_stark_check(chip, trace, on_device=False, per_row=True)


# ---------------------------------------------------------------------------- row check
def test_real_traces_pass():
    seen = set()
    for name, prog, stdin in D.PROGRAMS:
        for chip in sdk.UNI_STARK_CHIPS:
            t = C.trace_of(chip, prog, stdin)
            if t is None:
                continue
            res = check(chip, t)
            assert C.summary(res) == (chip, t.shape[0], sdk.uni_stark_info(chip).num_constraints,
                                      0, -1, -1), (name, chip)
            assert (res.first_fail_per_row == -1).all()
            assert res.ok and str(res) == f"{sdk.CHIPS[chip]}: {t.shape[0]} row(s) ok"
            seen.add(chip)
    assert seen == set(sdk.UNI_STARK_CHIPS)


def failing(res):
    return [int(i) for i in np.nonzero(res.first_fail_per_row >= 0)[0]]


@pytest.mark.parametrize("chip", [ADDSUB, IO])
def test_row_check_against_the_model(chip):
    prog, stdin, h = C.SMALL[chip]
    t = C.trace_of(chip, prog, stdin)
    assert t.shape[0] == h
    assert failing(check(chip, t)) == M.failing_rows(chip, M.from_mont_array(t)) == []
    cases = C.corruptions(chip, h, t.shape[1])
    assert len(cases) >= 20 and cases[0][0] == 0 and cases[1][0] == h - 1
    rows_seen = set()
    for row, col, value in cases:
        bad = C.corrupt(t, row, col, value)
        res = check(chip, bad)
        want = M.failing_rows(chip, M.from_mont_array(bad))
        assert failing(res) == want and want in ([], [row]), (row, col, value)
        assert C.summary(res) == C.summary_from_rows(chip, res.first_fail_per_row)
        rows_seen.update(want)
    assert {0, h - 1} <= rows_seen  # the first and the last row were among the failing ones


def test_the_existing_single_cell_corruption():
    t = np.array(C.trace_of(ADDSUB, "+" * 17), dtype=np.uint32)
    t[3, 1] = O.to_mont((O.from_mont(int(t[3, 1])) + 1) % O.P)  # add_operation.value
    res = check(ADDSUB, t)
    assert failing(res) == M.failing_rows(ADDSUB, M.from_mont_array(t)) == [3]
    assert (res.failing_rows, res.first_row, res.num_constraints) == (1, 3, 8)
    # value + 1: overflow is -1, so the first non-zero constraint is is_real * overflow * (overflow - 256)
    assert res.first_constraint == 3
    assert str(res) == "AddSub: 1 failing row(s); first: row 3, AIR constraint 3 of 8"


@pytest.mark.parametrize("chip", sdk.UNI_STARK_CHIPS, ids=[sdk.CHIPS[c] for c in sdk.UNI_STARK_CHIPS])
def test_row_check_against_the_merged_checker(chip):
    """bfz_check_chip evaluates Chip::eval, the AIR constraints first: a row's first failing index
    below K_air is the AIR-only check's, anything else is a LogUp constraint the AIR-only check
    does not have.  The permutation trace is the oracle's true one for the corrupted main trace."""
    prog, stdin, h = C.SMALL[chip]
    t = C.trace_of(chip, prog, stdin)
    k_air = sdk.uni_stark_info(chip).num_constraints
    alpha, beta = D.challenges(29)
    visible = 0
    cases = C.corruptions(chip, h, t.shape[1])
    for row, col, value in cases:
        bad = C.corrupt(t, row, col, value)
        canon = np.array(M.from_mont_array(bad), dtype=np.uint32)
        perm, cs = D.perm(chip, canon, None, alpha, beta)
        full = D.check(chip, canon, None, perm, alpha, beta, cs).first_fail_per_row
        assert D.k_air(D.check(chip, canon, None, perm, alpha, beta, cs)) == k_air
        expected = np.where(full < k_air, full, -1).astype(np.int32)
        res = check(chip, bad)
        assert np.array_equal(res.first_fail_per_row, expected), (row, col, value)
        assert C.summary(res) == C.summary_from_rows(chip, expected)
        visible += bool((expected >= 0).any())
    assert 2 * visible >= len(cases), (visible, len(cases))  # not vacuous: the AIR sees them


def test_meminstrs_below_cell_zero_fails_and_one_row_cpu_passes():
    bad = C.trace_of(MEMINSTRS, "<+")
    res = check(MEMINSTRS, bad)
    assert res.failing_rows >= 1 and res.first_row == 0 and 0 <= res.first_constraint < res.num_constraints
    one = C.trace_of(CPU, "+")
    assert one.shape == (1, 31)
    assert C.summary(check(CPU, one)) == (CPU, 1, sdk.uni_stark_info(CPU).num_constraints, 0, -1, -1)


def test_refused_inputs():
    good = C.trace_of(ADDSUB, "+")
    assert C.uni_check_status(ADDSUB, good) == (0, "")
    for what, (rc, msg) in {
        "Program": C.uni_check_status(1, np.zeros((16, 1), dtype=np.uint32)),
        "Memory": C.uni_check_status(4, np.zeros((16, 12), dtype=np.uint32)),
        "Byte": C.uni_check_status(5, np.zeros((16, 2), dtype=np.uint32)),
        "chip 8": C.uni_check_status(8, good),
        "width": C.uni_check_status(ADDSUB, good[:, :6]),
        "height 12": C.uni_check_status(ADDSUB, good[:12]),
        "word >= p": C.uni_check_status(ADDSUB, np.full((16, 7), O.P, dtype=np.uint32)),
    }.items():
        assert rc < 0 and msg.startswith("uni_stark: "), (what, rc, msg)
    with pytest.raises(sdk.BfzError, match="width mismatch for AddSub"):
        sdk.uni_stark_check(ADDSUB, good[:, :6], on_device=False)
    with pytest.raises(sdk.BfzError, match=r"non-canonical field word \(>= p\) in AddSub"):
        sdk.uni_stark_check(ADDSUB, np.full((16, 7), O.P, dtype=np.uint32), on_device=False)
    # the record and batch calls refuse the same chips
    L = _lib.lib()
    out = _lib.VerifyOutcomeC()
    for chip in (1, 4, 5, 8):
        buf, n = _lib.u8buf(bytes.fromhex(FIXTURES[0]["proof"]))
        arr = (ctypes.POINTER(ctypes.c_uint8) * 1)(ctypes.cast(buf, ctypes.POINTER(ctypes.c_uint8)))
        ch = (sdk.Challenger * 1)()
        assert L.bfz_uni_verify_batch((ctypes.c_int * 1)(chip), ch, arr, (ctypes.c_size_t * 1)(n), 1, 0,
                                      ctypes.byref(out)) < 0
        assert b"uni_stark" in L.bfz_last_error()


# ---------------------------------------------------------------------------- batch verify
def by_queries():
    groups = {}
    for f in FIXTURES:
        groups.setdefault(f["num_queries"], []).append(f)
    return groups


@pytest.mark.parametrize("on_device,mask", [(False, 0), (True, 2)], ids=["host", "standin"])
def test_fixtures_are_accepted_in_a_batch(on_device, mask):
    assert len(FIXTURES) == 4
    accepted = 0
    for nq, fs in by_queries().items():
        sdk.set_num_queries(nq)
        chips = [f["chip"] for f in fs]
        proofs = [bytes.fromhex(f["proof"]) for f in fs]
        want = [C.verify_one(c, p) for c, p in zip(chips, proofs)]
        _lib.lib().bfz_set_fault_injection(mask)
        got = C.verify_batch(chips, proofs, on_device)
        _lib.lib().bfz_set_fault_injection(0)
        assert got == want
        assert all(o == (True, -1, "") for o, _ in got)
        accepted += len(got)
        if not on_device:  # the SDK call: outcomes, and the caller's challengers advanced
            chs = [sdk.Challenger() for _ in fs]
            outs = sdk.uni_stark_verify_batch(chips, proofs, on_device=False, chs=chs)
            assert [((o.ok, o.query, o.why), bytes(c)) for o, c in zip(outs, chs)] == want
    assert accepted == 4


def _poke(proof, off, f):
    (v,) = struct.unpack_from("<I", proof, off)
    return proof[:off] + struct.pack("<I", f(v)) + proof[off + 4:]


@pytest.mark.parametrize("on_device,mask", [(False, 0), (True, 2)], ids=["host", "standin"])
def test_rejections_outside_the_query_phase(on_device, mask):
    """BFU1 layout: magic, chip, log degree, the trace commitment at byte 12, the quotient
    commitment at 44, the length of trace_local at 76 and its first value at 80; the PoW witness
    is the last word."""
    fs = by_queries()[2]
    assert len(fs) == 3
    sdk.set_num_queries(2)
    good = [(f["chip"], bytes.fromhex(f["proof"])) for f in fs]
    chip, proof = good[0]
    other = next(c for c in sdk.UNI_STARK_CHIPS if c != chip)
    bad = {
        "cut short": (chip, proof[: len(proof) // 2]),
        "empty": (chip, b""),
        "wrong chip": (other, proof),
        "commit word": (chip, _poke(proof, 12, lambda v: v ^ 1)),
        "PoW witness": (chip, _poke(proof, len(proof) - 4, lambda v: v ^ 1)),
        "opened value": (chip, _poke(proof, 80, lambda v: (v + 1) % O.P)),
    }
    # bad proofs between good ones, one call
    batch = [good[1]]
    for item in bad.values():
        batch += [item, good[len(batch) % 3]]
    want = [C.verify_one(c, p) for c, p in batch]
    _lib.lib().bfz_set_fault_injection(mask)
    got = C.verify_batch([c for c, _ in batch], [p for _, p in batch], on_device)
    _lib.lib().bfz_set_fault_injection(0)
    assert got == want
    oks = [o[0] for o, _ in got]
    assert oks == [True] + [False, True] * len(bad)  # the neighbours are undisturbed
    whys = dict(zip(bad, [o[2] for o, _ in got[1::2]]))
    assert all(o[1] == -1 for o, _ in got)  # none of these is a query's rejection
    assert whys["wrong chip"] == "proof is for another chip"
    assert whys["PoW witness"] == "bad PoW witness"
    assert all(whys.values())


def test_empty_batch_null_arguments_and_no_device():
    L = _lib.lib()
    assert sdk.uni_stark_verify_batch([], [], on_device=False) == []
    assert L.bfz_uni_verify_batch(None, None, None, None, 0, 0, None) == 0
    assert L.bfz_uni_verify_batch(None, None, None, None, 0, 1, None) == 0
    f = FIXTURES[0]
    buf, n = _lib.u8buf(bytes.fromhex(f["proof"]))
    arr = (ctypes.POINTER(ctypes.c_uint8) * 1)(ctypes.cast(buf, ctypes.POINTER(ctypes.c_uint8)))
    ch = (sdk.Challenger * 1)()
    assert L.bfz_uni_verify_batch((ctypes.c_int * 1)(f["chip"]), ch, arr, (ctypes.c_size_t * 1)(n), 1, 0,
                                  None) < 0
    assert b"null argument" in L.bfz_last_error()
    with pytest.raises(ValueError):
        sdk.uni_stark_verify_batch([f["chip"]], [], on_device=False)
