"""AIR programs of constraint degree 4 and 9 on the device: 4 and 8 quotient chunks computed over
the coset slabs of 3 H_(4n) / 3 H_(8n) (k_quotient_prog_coset), against the host verifier and the
independent model of tests/uni_stark_model.py, which recomposes any number of chunks.

Heights: 1 and 2 are the degenerate domains (a slab of 2 or 4 points, the next row wraps); 16 is
one partial block; 512 leaves the one-launch LDE (n > 256) and a slab is 4 blocks; 4096 is many."""
import numpy as np
import pytest

import air_high_degree_cases as H
import air_program_cases as A
import uni_stark_model as M
from bfz import _lib, sdk
from test_air_program_gpu import air_prove, commit_root

pytestmark = pytest.mark.gpu

CASES = [(k, h) for k in ("chain4", "chain9") for h in (1, 2, 16, 512, 4096)]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.init(0)
    sdk.set_num_queries(A.QUERIES)
    sdk.set_air_max_degree(9)
    yield
    sdk.set_air_max_degree(0)
    sdk.set_num_queries(0)


@pytest.mark.parametrize("kind,height", CASES, ids=[f"{k}-{h}" for k, h in CASES])
def test_high_degree_air_proves_verifies_and_matches_the_model(kind, height, monkeypatch):
    prog, mirror, trace, rows = H.case(kind, height)
    info = sdk.air_info(prog)
    assert (info.degree, info.log_quotient_degree) == (H.POWER[kind], H.LQD[kind])
    assert not (A.mirror_rows(mirror, rows) >= 0).any()
    proof, ch_p = air_prove(prog, trace)
    assert air_prove(prog, trace)[0] == proof  # same inputs, same bytes
    (ok, _, why), ch_v = A.air_verify_one(prog, proof)
    assert ok, why
    assert ch_v == bytes(ch_p)

    monkeypatch.setitem(M.AIRS, sdk.AIR_CHIP, mirror)
    monkeypatch.setitem(M.LOG_QUOTIENT_DEGREE, sdk.AIR_CHIP, info.log_quotient_degree)
    p = M.parse(proof)
    assert p["log_degree"] == height.bit_length() - 1
    assert len(p["chunks"]) == 1 << H.LQD[kind]
    t = M.check_transcript(p, M.challenger_words(ch_p))
    assert p["trace_commit"] == commit_root(trace)
    if height <= 64:
        M.check_openings(p, rows, t["zeta"])
    M.check_quotient(p, t["alpha"], t["zeta"])

    assert A.summary(sdk.air_check(prog, trace, on_device=True)) == \
        (-1, height, info.num_constraints, 0, -1, -1)


@pytest.mark.parametrize("kind,height,other", [("chain4", 512, "chain9"), ("chain9", 16, "chain4")],
                         ids=["chain4-512", "chain9-16"])
def test_invalid_traces_other_programs_and_the_default_cap_are_rejected(kind, height, other):
    prog, mirror, trace, _ = H.case(kind, height)
    for r in (0, height // 2 - 1, height - 1):
        bad = A.flip(trace, r, 1)
        want = A.mirror_rows(mirror, A.canonical(bad))
        assert want[r] >= 0, r
        dev = sdk.air_check(prog, bad, on_device=True, per_row=True)
        host = sdk.air_check(prog, bad, on_device=False, per_row=True)
        assert np.array_equal(dev.first_fail_per_row, want), r
        assert np.array_equal(host.first_fail_per_row, want), r
        assert A.summary(dev) == A.summary(host) == A.summary_from_rows(want, 4), r
        counts_d = sdk.air_check_constraints(prog, bad, on_device=True)
        counts_h = sdk.air_check_constraints(prog, bad, on_device=False)
        assert [list(c) for c in counts_d[1:]] == [list(c) for c in counts_h[1:]], r
        proof, _ = air_prove(prog, bad)  # still proves
        (ok, _, why), _ = A.air_verify_one(prog, proof)
        assert not ok and why == "OOD evaluation mismatch on chip custom", r

    proof, _ = air_prove(prog, trace)
    (ok, _, why), _ = A.air_verify_one(H.program(other), proof)  # 4 chunks against 8
    assert not ok and why == "opened-value shape mismatch"
    sdk.set_air_max_degree(0)
    try:
        with pytest.raises(sdk.BfzError, match="constraint degree above 3 is not supported"):
            sdk.air_verify(prog, proof)
    finally:
        sdk.set_air_max_degree(9)
    sdk.air_verify(prog, proof)
