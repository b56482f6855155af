"""Caller-defined AIRs as constraint programs on the device (bfz_air_prove, bfz_air_check): parity
with the compiled kernels on the built-in chips' exported programs (the same proof bytes but the
chip word, the same row-check results), two AIRs that are not chips against the host verifier and
the independent model of tests/uni_stark_model.py, invalid traces, and the refused inputs."""
import ctypes

import numpy as np
import pytest

import air_program_cases as A
import oracle_lib as O
import uni_device_cases as U
import uni_stark_model as M
from bfz import _lib, sdk

pytestmark = pytest.mark.gpu

QUERIES = A.QUERIES
CUSTOM = [("fib", h) for h in A.FIB_HEIGHTS] + [("mulgate", h) for h in A.MULGATE_HEIGHTS]
CUSTOM_IDS = [f"{k}-{h}" for k, h in CUSTOM]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.init(0)
    sdk.set_num_queries(QUERIES)
    yield
    sdk.set_num_queries(0)


def air_prove(prog, trace):
    ch = sdk.Challenger()
    return sdk.air_prove(prog, trace, ch), ch


def commit_root(trace):
    m = np.ascontiguousarray(trace, dtype=np.uint32)
    ptrs = (ctypes.POINTER(ctypes.c_uint32) * 1)(m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    hs, ws = (ctypes.c_size_t * 1)(m.shape[0]), (ctypes.c_size_t * 1)(m.shape[1])
    root = (ctypes.c_uint32 * 8)()
    _lib.check(_lib.lib().bfz_commit(ptrs, hs, ws, 1, root))
    return [O.from_mont(int(v)) for v in root]


# ---------------------------------------------------------------------------- parity
@pytest.mark.parametrize("name,chip,prog,stdin,height", A.CHIP_CASES, ids=[c[0] for c in A.CHIP_CASES])
def test_exported_program_proves_the_compiled_kernels_bytes(name, chip, prog, stdin, height):
    trace = U.trace_of(chip, prog, stdin)
    assert trace.shape == (height, A.WIDTHS[chip])
    ch_c = sdk.Challenger()
    want = sdk.uni_stark_prove(chip, trace, ch_c)
    got, ch_p = air_prove(A.export(chip), trace)
    assert got[4:8] == b"\xff\xff\xff\xff" and want[4:8] == chip.to_bytes(4, "little")
    assert got[:4] == want[:4] and got[8:] == want[8:]
    assert bytes(ch_p) == bytes(ch_c)
    (ok, _, why), ch_v = A.air_verify_one(A.export(chip), got)
    assert ok, why
    assert ch_v == bytes(ch_p)


@pytest.mark.parametrize("name,chip,prog,stdin,height", A.CHIP_CASES, ids=[c[0] for c in A.CHIP_CASES])
def test_exported_program_checks_as_the_compiled_kernel(name, chip, prog, stdin, height):
    trace = U.trace_of(chip, prog, stdin)
    traces = [trace] + [U.corrupt(trace, *c) for c in U.corruptions(chip, height, trace.shape[1])]
    for i, t in enumerate(traces):
        want = sdk.uni_stark_check(chip, t, on_device=True, per_row=True)
        got = sdk.air_check(A.export(chip), t, on_device=True, per_row=True)
        assert got.chip == -1
        assert A.summary(got)[1:] == A.summary(want)[1:], i
        assert np.array_equal(got.first_fail_per_row, want.first_fail_per_row), i


# ---------------------------------------------------------------------------- custom AIRs
@pytest.mark.parametrize("kind,height", CUSTOM, ids=CUSTOM_IDS)
def test_custom_air_proves_verifies_and_matches_the_model(kind, height, monkeypatch):
    prog, mirror, trace, rows = A.custom_case(kind, height)
    info = sdk.air_info(prog)
    assert not (A.mirror_rows(mirror, rows) >= 0).any()
    proof, ch_p = air_prove(prog, trace)
    (ok, _, why), ch_v = A.air_verify_one(prog, proof)
    assert ok, why
    assert ch_v == bytes(ch_p)
    assert air_prove(prog, trace)[0] == proof  # same inputs, same bytes
    sdk.air_verify(prog, proof)

    monkeypatch.setitem(M.AIRS, sdk.AIR_CHIP, mirror)
    monkeypatch.setitem(M.LOG_QUOTIENT_DEGREE, sdk.AIR_CHIP, info.log_quotient_degree)
    p = M.parse(proof)
    assert p["chip"] == sdk.AIR_CHIP and p["log_degree"] == height.bit_length() - 1
    assert len(p["queries"]) == QUERIES
    assert len(p["chunks"]) == 1 << info.log_quotient_degree
    t = M.check_transcript(p, M.challenger_words(ch_p))            # (a)
    assert p["trace_commit"] == commit_root(trace)                  # (b)
    if height <= 64:
        M.check_openings(p, rows, t["zeta"])                        # (c)
    M.check_quotient(p, t["alpha"], t["zeta"])                      # (d)

    # the device row check agrees that the trace is valid
    assert A.summary(sdk.air_check(prog, trace, on_device=True)) == \
        (-1, height, info.num_constraints, 0, -1, -1)
    # the compiled chips' verifier does not take it
    (ok, _, why), _ = U.verify_one(U.ADDSUB, proof)
    assert not ok and why == "proof is for another chip"


def test_another_program_rejects_the_proof():
    prog, _, trace, _ = A.mulgate_case(16)
    proof, _ = air_prove(prog, trace)
    (ok, _, why), _ = A.air_verify_one(A.mulgate_program(broken="square"), proof)
    assert not ok and why == "OOD evaluation mismatch on chip custom"
    with pytest.raises(sdk.BfzError, match="OOD evaluation mismatch on chip custom"):
        sdk.air_verify(A.mulgate_program(broken="square"), proof)
    # a b replaced by a + b is quadratic: one quotient chunk, so the shapes already differ
    assert sdk.air_info(A.mulgate_program(broken="sum")).log_quotient_degree == 0
    (ok, _, why), _ = A.air_verify_one(A.mulgate_program(broken="sum"), proof)
    assert not ok and why == "opened-value shape mismatch"


# ---------------------------------------------------------------------------- invalid traces
# fib: b + 1.  mulgate: s + 2 -- its zero rows are unconstrained while s is 0 or 1, and the last
# row is one of them.
@pytest.mark.parametrize("kind,height,col,delta", [("fib", 1024, 1, 1), ("mulgate", 512, 3, 2)],
                         ids=["fib-1024", "mulgate-512"])
def test_invalid_traces_are_located_prove_and_are_rejected(kind, height, col, delta):
    prog, mirror, trace, _ = A.custom_case(kind, height)
    k = sdk.air_info(prog).num_constraints
    for r in (0, height // 2 - 1, height - 1):
        bad = A.flip(trace, r, col, delta)
        want = A.mirror_rows(mirror, A.canonical(bad))
        assert want[r] >= 0, r
        dev = sdk.air_check(prog, bad, on_device=True, per_row=True)
        host = sdk.air_check(prog, bad, on_device=False, per_row=True)
        assert np.array_equal(dev.first_fail_per_row, want), r
        assert np.array_equal(host.first_fail_per_row, want), r
        assert A.summary(dev) == A.summary(host) == A.summary_from_rows(want, k), r
        proof, _ = air_prove(prog, bad)  # still proves
        (ok, _, why), _ = A.air_verify_one(prog, proof)
        assert not ok and why == "OOD evaluation mismatch on chip custom", r
        with pytest.raises(sdk.BfzError, match="violates the AIR"):
            sdk.air_prove(prog, bad, check=True)


# ---------------------------------------------------------------------------- refusals
def test_refused_inputs_carry_uni_proves_messages_and_leave_the_prover_usable():
    prog, _, good, _ = A.mulgate_case(16)
    want, _ = air_prove(prog, good)
    quartic = sdk.AirBuilder(4)
    x = quartic.local(0)
    quartic.assert_zero(x * x * x * x)
    for what, (rc, msg), needle in (
            ("width", A.air_prove_status(prog, good[:, :3]), "uni_stark: width mismatch for custom"),
            ("height 3", A.air_prove_status(prog, good[:3]),
             "uni_stark: height not a power of two in [1, 2^23] for custom"),
            ("word >= p", A.air_prove_status(prog, np.full((16, 4), O.P, dtype=np.uint32)),
             "uni_stark: non-canonical field word (>= p) in custom"),
            ("degree 4", A.air_prove_status(quartic.build(), good),
             "uni_stark: constraint degree above 3 is not supported")):
        assert rc < 0 and msg == needle, (what, rc, msg)
        assert air_prove(prog, good)[0] == want, what
    # the messages are bfz_uni_prove's, with the chip's name in place of "custom"
    t = U.trace_of(U.ADDSUB, "+")
    ch = sdk.Challenger()
    with pytest.raises(sdk.BfzError, match=r"uni_stark: width mismatch for AddSub"):
        sdk.uni_stark_prove(U.ADDSUB, t[:, :6], ch)
    with pytest.raises(sdk.BfzError, match=r"uni_stark: height not a power of two in \[1, 2\^23\] for AddSub"):
        sdk.uni_stark_prove(U.ADDSUB, t[:3], ch)
    with pytest.raises(sdk.BfzError, match=r"uni_stark: non-canonical field word \(>= p\) in AddSub"):
        sdk.uni_stark_prove(U.ADDSUB, np.full((16, 7), O.P, dtype=np.uint32), ch)
