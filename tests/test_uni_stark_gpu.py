"""Per-chip uni-STARK proofs on the device (bfz_uni_prove) against the host verifier
(bfz_uni_verify) and the independent model of tests/uni_stark_model.py: all five chips with AIR
constraints, heights 1 .. 2^16, both quotient shapes (two chunks: Cpu, AddSub, Jump, MemoryInstrs;
one chunk: IO), determinism, the challenger hand-back, invalid traces, the query-count setting and
the refused inputs."""
import ctypes
import os

import numpy as np
import pytest

import oracle_lib as O
import uni_stark_model as M
from bfz import _lib, guests, sdk

pytestmark = pytest.mark.gpu

CPU, ADDSUB, JUMP, MEMINSTRS, IO = 0, 2, 3, 6, 7
QUERIES = 6  # all tests but test_query_counts: the protocol does not depend on the count

# (id, chip, program, stdin, height): heights confirmed with sdk.generate_traces on the CPU
CASES = [
    ("cpu-1", CPU, "+", [], 1),
    ("cpu-4", CPU, "+++.", [], 4),
    ("cpu-512", CPU, guests.HELLO, [], 512),
    ("cpu-65536", CPU, guests.FIBO, [17], 65536),
    ("addsub-16", ADDSUB, "+", [], 16),
    ("addsub-32", ADDSUB, "+" * 17, [], 32),
    ("addsub-256", ADDSUB, guests.HELLO, [], 256),
    ("addsub-16384", ADDSUB, guests.FIBO, [17], 16384),
    ("jump-32", JUMP, guests.HELLO, [], 32),
    ("jump-8192", JUMP, guests.FIBO, [17], 8192),
    ("meminstrs-16", MEMINSTRS, ">", [], 16),
    ("meminstrs-64", MEMINSTRS, guests.HELLO, [], 64),
    ("meminstrs-32768", MEMINSTRS, guests.FIBO, [17], 32768),
    ("io-16", IO, ".", [], 16),
    ("io-32", IO, "." * 17, [], 32),
]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.init(0)
    sdk.set_num_queries(QUERIES)
    yield
    sdk.set_num_queries(0)


_traces = {}


def trace_of(chip, prog, stdin):
    key = (prog, tuple(stdin))
    if key not in _traces:
        _traces[key] = {c: t for c, _, t in sdk.generate_traces(prog, stdin)}
    return _traces[key][chip]


def prove(chip, trace):
    ch = sdk.Challenger()
    proof = sdk.uni_stark_prove(chip, trace, ch)
    return proof, ch


def verify(chip, proof):
    """(ok, why, the verifier's ending challenger)"""
    ch = sdk.Challenger()
    buf, n = _lib.u8buf(proof)
    out = _lib.VerifyOutcomeC()
    _lib.check(_lib.lib().bfz_uni_verify(chip, ctypes.byref(ch), buf, n, ctypes.byref(out)))
    return bool(out.ok), out.why.decode(), ch


def commit_root(trace):
    """bfz_commit([trace]): the commitment test_commit_root_parity pins against the oracle."""
    m = np.ascontiguousarray(trace, dtype=np.uint32)
    ptrs = (ctypes.POINTER(ctypes.c_uint32) * 1)(m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    hs, ws = (ctypes.c_size_t * 1)(m.shape[0]), (ctypes.c_size_t * 1)(m.shape[1])
    root = (ctypes.c_uint32 * 8)()
    _lib.check(_lib.lib().bfz_commit(ptrs, hs, ws, 1, root))
    return [O.from_mont(int(v)) for v in root]


def model_checks(chip, trace, proof, ch_end):
    """Model checks (a), (b), and (c), (d) where they apply; returns which of c, d ran."""
    p = M.parse(proof)
    assert p["chip"] == chip and p["log_degree"] == trace.shape[0].bit_length() - 1
    assert len(p["queries"]) == QUERIES
    t = M.check_transcript(p, M.challenger_words(ch_end))          # (a)
    assert p["trace_commit"] == commit_root(trace)                  # (b)
    ran = ""
    if trace.shape[0] <= 64:
        M.check_openings(p, M.from_mont_array(trace), t["zeta"])    # (c)
        ran += "c"
    if chip in M.AIRS:
        M.check_quotient(p, t["alpha"], t["zeta"])                  # (d)
        ran += "d"
    return ran


@pytest.mark.parametrize("name,chip,prog,stdin,height", CASES, ids=[c[0] for c in CASES])
def test_prove_verify_and_model(name, chip, prog, stdin, height):
    trace = trace_of(chip, prog, stdin)
    assert trace.shape[0] == height
    proof, ch_p = prove(chip, trace)
    ok, why, ch_v = verify(chip, proof)
    assert ok, why
    assert bytes(ch_p) == bytes(ch_v)  # prover and verifier end in the same challenger state
    assert prove(chip, trace)[0] == proof  # same inputs, same bytes
    ran = model_checks(chip, trace, proof, ch_p)
    if chip in (ADDSUB, IO) and height <= 64:
        assert ran == "cd"  # never vacuous for either chunk shape


def test_chunk_counts_follow_the_air():
    for chip, chunks in ((CPU, 2), (ADDSUB, 2), (IO, 1)):
        c = next(c for c in CASES if c[1] == chip)
        proof, _ = prove(chip, trace_of(c[1], c[2], c[3]))
        assert len(M.parse(proof)["chunks"]) == chunks == 1 << sdk.uni_stark_info(chip).log_quotient_degree


@pytest.mark.parametrize("height", [1, 2])
def test_one_chunk_shape_at_the_smallest_heights(height):
    """IO traces are padded to 16 rows, so the one-chunk kernel's edge sizes (a quotient domain of
    1 and 2 points) are reached with IO's padding rows alone: all-zero rows satisfy its AIR."""
    trace = np.zeros((height, 5), dtype=np.uint32)
    assert M.failing_rows(IO, M.from_mont_array(trace)) == []
    proof, ch_p = prove(IO, trace)
    ok, why, ch_v = verify(IO, proof)
    assert ok, why
    assert bytes(ch_p) == bytes(ch_v)
    assert model_checks(IO, trace, proof, ch_p) == "cd"


@pytest.mark.parametrize("name,chip", [("io-zero-65536", IO), ("cpu-65536", CPU)])
def test_fused_fold_rounds_reproduce_the_recorded_proofs(name, chip):
    """2^16 rows is the smallest height whose first commit-phase round leaves a fold of
    2^15 >= FRI_FUSE_MIN outputs pending: the fused fold + leaf-hash round runs, then the unfused
    rounds and the single-launch tail.  One chunk (all-zero IO rows) and two chunks (Cpu).  The
    digests of tests/golden/uni_stark_fused.json were recorded before the uni-STARK prover took
    over the machine prover's PCS opening, from the build of the commit named there."""
    import hashlib
    import json
    if chip == IO:
        trace = np.zeros((1 << 16, 5), dtype=np.uint32)
    else:
        trace = trace_of(CPU, guests.FIBO, [17])
    assert trace.shape[0] == 1 << 16
    here = os.path.dirname(os.path.abspath(__file__))
    golden = json.load(open(os.path.join(here, "golden", "uni_stark_fused.json")))
    assert golden["num_queries"] == QUERIES
    proof, ch_p = prove(chip, trace)
    ok, why, ch_v = verify(chip, proof)
    assert ok, why
    assert bytes(ch_p) == bytes(ch_v)
    assert prove(chip, trace)[0] == proof
    p = M.parse(proof)
    assert len(p["queries"]) == QUERIES and p["log_degree"] == 16
    M.check_transcript(p, M.challenger_words(ch_p))
    want = golden["proofs"][name]
    assert len(proof) == want["bytes"]
    assert hashlib.sha256(proof).hexdigest() == want["sha256"]


def test_invalid_traces_prove_and_are_rejected():
    """One changed cell of a real AddSub row, and the MemoryInstrs trace of `<+` (the pointer steps
    below cell 0: the word range check fails): both still prove, and the verifier's out-of-domain
    identity fails."""
    trace = trace_of(ADDSUB, "+" * 17, []).copy()
    assert M.failing_rows(ADDSUB, M.from_mont_array(trace)) == []
    trace[3, 1] = O.to_mont((O.from_mont(int(trace[3, 1])) + 1) % O.P)  # add_operation.value
    assert M.failing_rows(ADDSUB, M.from_mont_array(trace)) == [3]
    proof, _ = prove(ADDSUB, trace)
    ok, why, _ = verify(ADDSUB, proof)
    assert not ok and why == "OOD evaluation mismatch on chip AddSub"
    # the model agrees: transcript and openings hold, the quotient identity does not
    p = M.parse(proof)
    t = M.check_transcript(p)
    M.check_openings(p, M.from_mont_array(trace), t["zeta"])
    assert M.folded_at_zeta(p, t["alpha"], t["zeta"]) != M.quotient_at_zeta(p, t["zeta"])
    with pytest.raises(sdk.BfzError, match="OOD evaluation mismatch"):
        sdk.uni_stark_verify(ADDSUB, proof)

    bad = trace_of(MEMINSTRS, "<+", [])
    proof, _ = prove(MEMINSTRS, bad)
    ok, why, _ = verify(MEMINSTRS, proof)
    assert not ok and why == "OOD evaluation mismatch on chip MemoryInstrs"


def test_query_counts():
    trace = trace_of(ADDSUB, guests.HELLO, [])
    default = int(os.environ.get("FRI_QUERIES", 84))  # kb31_poseidon2.rs:59-62
    try:
        for setting, want in ((1, 1), (0, default)):
            sdk.set_num_queries(setting)
            proof, _ = prove(ADDSUB, trace)
            sdk.uni_stark_verify(ADDSUB, proof)
            assert len(M.parse(proof)["queries"]) == want
        sdk.set_num_queries(default + 1)  # a verifier expecting another count rejects it
        with pytest.raises(sdk.BfzError, match="wrong number of queries"):
            sdk.uni_stark_verify(ADDSUB, proof)
    finally:
        sdk.set_num_queries(QUERIES)


def test_pcs_variant_is_honoured():
    trace = trace_of(IO, ".", [])
    try:
        sdk.set_pcs_variant(0)
        proof, _ = prove(IO, trace)
        sdk.uni_stark_verify(IO, proof)
        M.check_transcript(M.parse(proof), observe_openings=False)
        sdk.set_pcs_variant(1)
        assert prove(IO, trace)[0] != proof
        with pytest.raises(sdk.BfzError):
            sdk.uni_stark_verify(IO, proof)
    finally:
        sdk.set_pcs_variant(-1)


def test_refused_inputs_leave_the_prover_usable():
    good = trace_of(ADDSUB, "+", [])
    want, _ = prove(ADDSUB, good)
    L = _lib.lib()

    def status(chip, m, h=None, w=None):
        m = np.ascontiguousarray(m, dtype=np.uint32)
        ch = sdk.Challenger()
        ptr, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t()
        rc = L.bfz_uni_prove(chip, m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                             m.shape[0] if h is None else h, m.shape[1] if w is None else w,
                             ctypes.byref(ch), ctypes.byref(ptr), ctypes.byref(n), None)
        return rc, L.bfz_last_error().decode()

    for what, (rc, msg) in {
        "width": status(ADDSUB, good[:, :6]),
        "height 12": status(ADDSUB, good[:12]),
        "height 0": status(ADDSUB, good, h=0),
        "height 2^24": status(ADDSUB, good, h=1 << 24),  # refused before the trace is read
        "Program": status(1, np.zeros((16, 1), dtype=np.uint32)),
        "Memory": status(4, np.zeros((16, 12), dtype=np.uint32)),
        "Byte": status(5, np.zeros((16, 2), dtype=np.uint32)),
        "chip 8": status(8, good),
        "word >= p": status(ADDSUB, np.full((16, 7), O.P, dtype=np.uint32)),
    }.items():
        assert rc < 0 and msg, what
        assert prove(ADDSUB, good)[0] == want, what


def test_committed_fixtures_are_reproduced():
    """The fixture proofs of tests/golden/uni_stark.json (the host tests' input) are what the
    prover writes today, byte for byte."""
    import json
    here = os.path.dirname(os.path.abspath(__file__))
    try:
        for f in json.load(open(os.path.join(here, "golden", "uni_stark.json"))):
            sdk.set_num_queries(f["num_queries"])
            proof, _ = prove(f["chip"], trace_of(f["chip"], f["program"], f["stdin"]))
            assert proof.hex() == f["proof"], f["name"]
    finally:
        sdk.set_num_queries(QUERIES)
