"""Per-chip uni-STARK proofs without a device: the bfz_uni_info table, the model's own AIRs on
real traces, and the host verifier (bfz_uni_verify) on small fixture proofs written once by the
device prover (tests/golden/uni_stark.json: AddSub and Jump with two chunks, IO with one, the
1-row Cpu trace of a one-cycle program) -- accepted, rejected after any single-word change, for the
wrong chip and when cut short, and consistent with the independent model of
tests/uni_stark_model.py."""
import ctypes
import json
import os
import struct

import pytest

import uni_stark_model as M
from bfz import _lib, guests, sdk

CPU, ADDSUB, JUMP, MEMINSTRS, IO = 0, 2, 3, 6, 7
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = json.load(open(os.path.join(HERE, "golden", "uni_stark.json")))
IDS = [f["name"] for f in FIXTURES]


@pytest.fixture(autouse=True)
def default_queries():
    yield
    sdk.set_num_queries(0)


def verify(chip, proof, num_queries):
    """(ok, why, the verifier's ending challenger)"""
    sdk.set_num_queries(num_queries)
    ch = sdk.Challenger()
    buf, n = _lib.u8buf(proof)
    out = _lib.VerifyOutcomeC()
    _lib.check(_lib.lib().bfz_uni_verify(chip, ctypes.byref(ch), buf, n, ctypes.byref(out)))
    assert out.query >= -1
    return bool(out.ok), out.why.decode(), ch


def trace_of(f):
    return {c: t for c, _, t in sdk.generate_traces(f["program"], f["stdin"])}[f["chip"]]


# ---------------------------------------------------------------------------- bfz_uni_info
def test_info_table():
    for chip in (CPU, ADDSUB, JUMP, MEMINSTRS):
        i = sdk.uni_stark_info(chip)
        assert (i.degree, i.log_quotient_degree) == (3, 1), chip
    io = sdk.uni_stark_info(IO)
    assert (io.degree, io.log_quotient_degree) == (2, 0)
    assert sdk.uni_stark_info(ADDSUB).num_constraints == 8
    # K against a count of the model's own constraints
    for chip, width in ((ADDSUB, 7), (IO, 5)):
        row = [M.ZERO] * width
        assert sdk.uni_stark_info(chip).num_constraints == len(M.AIRS[chip](row, row, 0, 0, 0))
        assert sdk.uni_stark_info(chip).log_quotient_degree == M.LOG_QUOTIENT_DEGREE[chip]
    assert sdk.UNI_STARK_CHIPS == (CPU, ADDSUB, JUMP, MEMINSTRS, IO)


@pytest.mark.parametrize("chip", [1, 4, 5, -1, 8])
def test_chips_without_an_air_are_refused(chip):
    with pytest.raises(sdk.BfzError, match="uni_stark"):
        sdk.uni_stark_info(chip)
    out = _lib.VerifyOutcomeC()
    ch = sdk.Challenger()
    buf, n = _lib.u8buf(bytes.fromhex(FIXTURES[0]["proof"]))
    assert _lib.lib().bfz_uni_verify(chip, ctypes.byref(ch), buf, n, ctypes.byref(out)) < 0
    assert _lib.lib().bfz_last_error()


# ---------------------------------------------------------------------------- the model itself
@pytest.mark.parametrize("prog,stdin", [("+", []), ("+++.", []), (",.,.", [7, 9]), (guests.HELLO, []),
                                        (guests.FIBO, [9])], ids=["plus", "p3dot", "io2", "hello", "fibo9"])
def test_model_airs_vanish_on_real_traces(prog, stdin):
    seen = 0
    for chip, _, t in sdk.generate_traces(prog, stdin):
        if chip in M.AIRS:
            assert M.failing_rows(chip, M.from_mont_array(t)) == [], sdk.CHIPS[chip]
            seen += 1
    assert seen


def test_model_airs_see_a_changed_cell():
    t = M.from_mont_array(trace_of(FIXTURES[IDS.index("addsub16")]))
    t[0][2] = 1  # carry without an overflow
    assert M.failing_rows(ADDSUB, t) == [0]
    t = M.from_mont_array(trace_of(FIXTURES[IDS.index("io16")]))
    t[5][3] = 2  # is_input not a boolean, on a padding row
    assert M.failing_rows(IO, t) == [5]


# ---------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("f", FIXTURES, ids=IDS)
def test_fixture_accepted_and_model_checks(f):
    proof = bytes.fromhex(f["proof"])
    ok, why, ch = verify(f["chip"], proof, f["num_queries"])
    assert ok and why == ""
    p = M.parse(proof)
    assert (p["chip"], 1 << p["log_degree"], len(p["queries"])) == (f["chip"], f["height"], f["num_queries"])
    assert len(p["chunks"]) == 1 << sdk.uni_stark_info(f["chip"]).log_quotient_degree
    t = M.check_transcript(p, M.challenger_words(ch))                     # (a)
    trace = trace_of(f)
    assert trace.shape[0] == f["height"] <= 64
    M.check_openings(p, M.from_mont_array(trace), t["zeta"])              # (c)
    if f["chip"] in M.AIRS:
        M.check_quotient(p, t["alpha"], t["zeta"])                        # (d)
    with pytest.raises(sdk.BfzError, match="wrong number of queries"):
        sdk.set_num_queries(f["num_queries"] + 1)
        sdk.uni_stark_verify(f["chip"], proof)


def test_fixtures_cover_both_chunk_shapes_with_the_quotient_check():
    chips = {f["chip"] for f in FIXTURES}
    assert {ADDSUB, IO} <= chips and CPU in chips


def sections(proof):
    """(section, byte offset of one word in it) over the whole BFU1 layout; for a section of many
    words the first and the last."""
    r = M.Reader(proof)
    out = []

    def word(name):
        out.append((name, r.off))
        return r.u32()

    def span(name, nwords):
        if nwords:
            out.append((name + "[0]", r.off))
            out.append((name + "[-1]", r.off + 4 * (nwords - 1)))
        r.off += 4 * nwords

    word("magic"), word("chip"), word("log_degree")
    span("trace_commit", 8), span("quotient_commit", 8)
    span("trace_local", 4 * word("len trace_local"))
    span("trace_next", 4 * word("len trace_next"))
    for j in range(word("chunks")):
        span(f"chunk {j}", 4 * word(f"len chunk {j}"))
    for i in range(word("commit roots")):
        span(f"commit root {i}", 8)
    for q in range(word("queries")):
        for rr in range(word(f"q{q} rounds")):
            for m in range(word(f"q{q} r{rr} matrices")):
                span(f"q{q} r{rr} row {m}", word(f"q{q} r{rr} width {m}"))
            span(f"q{q} r{rr} path", 8 * word(f"q{q} r{rr} path length"))
        for s in range(word(f"q{q} steps")):
            span(f"q{q} step {s} sibling", 4)
            span(f"q{q} step {s} path", 8 * word(f"q{q} step {s} path length"))
    span("final_poly", 4)
    word("pow_witness")
    assert r.off == len(proof)
    return out


@pytest.mark.parametrize("f", FIXTURES, ids=IDS)
def test_every_single_word_change_is_rejected(f):
    proof = bytes.fromhex(f["proof"])
    secs = sections(proof)
    names = {name.split("[")[0] for name, _ in secs}
    assert {"magic", "chip", "log_degree", "trace_commit", "quotient_commit", "trace_local",
            "trace_next", "chunk 0", "q0 r0 row 0", "q0 r0 path", "q0 r1 row 0", "q0 r1 path",
            "final_poly", "pow_witness"} <= names
    if f["height"] > 1:  # a 1-row trace has no FRI round
        assert {"commit root 0", "q0 step 0 sibling", "q0 step 0 path"} <= names
    for name, off in secs:
        for flip in (1, 1 << 20):
            (v,) = struct.unpack_from("<I", proof, off)
            bad = proof[:off] + struct.pack("<I", v ^ flip) + proof[off + 4:]
            ok, why, _ = verify(f["chip"], bad, f["num_queries"])
            assert not ok and why, (name, flip)
    # a changed opened value is a transcript or opening failure, never a crash or an OOD surprise
    off = dict(secs)["trace_local[0]"]
    (v,) = struct.unpack_from("<I", proof, off)
    bad = proof[:off] + struct.pack("<I", (v + 1) % M.P) + proof[off + 4:]
    assert verify(f["chip"], bad, f["num_queries"])[1] in (
        "bad PoW witness", "input Merkle opening rejected", "FRI final value mismatch",
        "FRI commit-phase opening rejected")


@pytest.mark.parametrize("f", FIXTURES, ids=IDS)
def test_wrong_chip_truncated_and_extended(f):
    proof = bytes.fromhex(f["proof"])
    for other in sdk.UNI_STARK_CHIPS:
        if other != f["chip"]:
            ok, why, _ = verify(other, proof, f["num_queries"])
            assert not ok and why == "proof is for another chip"
    cuts = sorted({0, 3, 4, 11, 12, 76, len(proof) // 2, len(proof) - 4, len(proof) - 1}
                  | {off for _, off in sections(proof)})
    for cut in cuts:
        ok, why, _ = verify(f["chip"], proof[:cut], f["num_queries"])
        assert not ok and why, cut
    ok, why, _ = verify(f["chip"], proof + b"\0\0\0\0", f["num_queries"])
    assert not ok and why == "trailing bytes"


def test_same_width_chips_do_not_share_proofs():
    """The chip word is bound by the shapes, not trusted: an AddSub proof relabelled as IO fails on
    the opened-value shapes (7 columns against 5, two chunks against one)."""
    f = FIXTURES[IDS.index("addsub16")]
    proof = bytearray(bytes.fromhex(f["proof"]))
    struct.pack_into("<I", proof, 4, IO)
    ok, why, _ = verify(IO, bytes(proof), f["num_queries"])
    assert not ok and why == "opened-value shape mismatch"
