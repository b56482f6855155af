"""Caller-defined AIRs as constraint programs, without a device: the exporter against bfz_uni_info,
the extension-field evaluator against the model's AIRs and the Python mirrors, the host row check
against bfz_uni_check, the host verifier (bfz_air_verify) against bfz_uni_verify on the fixture
proofs of tests/golden/uni_stark.json and their single-word mutations, the validation of malformed
programs, and the AirBuilder round trip."""
import ctypes
import json
import os
import struct

import numpy as np
import pytest

import air_program_cases as A
import uni_device_cases as U
import uni_stark_model as M
from bfz import _lib, sdk

CPU, ADDSUB, JUMP, MEMINSTRS, IO = 0, 2, 3, 6, 7
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = json.load(open(os.path.join(HERE, "golden", "uni_stark.json")))
IDS = [f["name"] for f in FIXTURES]
P = M.P
MAGIC = 0x31414642
CONST, LOCAL, NEXT, FIRST, LAST, TRANS, ADD, SUB, MUL, NEG = range(10)


@pytest.fixture(autouse=True)
def default_queries():
    yield
    sdk.set_num_queries(0)


def raw(width, nodes, cons, n_nodes=None, n_cons=None):
    """BFA1 bytes from (op, a, b) triples and constraint node indices; the header counts can lie."""
    words = [MAGIC, width, len(nodes) if n_nodes is None else n_nodes,
             len(cons) if n_cons is None else n_cons]
    for n in nodes:
        words.extend(n)
    words.extend(cons)
    return struct.pack(f"<{len(words)}I", *words)


def ef_rows(rng, n):
    """n random canonical EF values as ([M.EF], (n, 4) Montgomery words)."""
    c = rng.integers(0, P, size=(n, 4))
    return [M.EF(r) for r in c.tolist()], A.mont(c)


def eval_both(prog, mirror, width, rng):
    """(air_eval of prog, the mirror) on one random EF frame, both as lists of canonical 4-tuples."""
    loc, loc_w = ef_rows(rng, width)
    nxt, nxt_w = ef_rows(rng, width)
    sel, sel_w = ef_rows(rng, 3)
    got = sdk.air_eval(prog, loc_w, nxt_w, sel_w[0], sel_w[1], sel_w[2])
    want = mirror(loc, nxt, sel[0], sel[1], sel[2])
    return [tuple(r) for r in M.from_mont_array(got)], [M._ef(v).c for v in want]


# ---------------------------------------------------------------------------- exporter, shape
@pytest.mark.parametrize("chip", sdk.UNI_STARK_CHIPS)
def test_exported_shape_is_the_chips(chip):
    want = sdk.uni_stark_info(chip)
    got = sdk.air_info(sdk.air_export(chip))
    assert (got.num_constraints, got.degree, got.log_quotient_degree) == \
        (want.num_constraints, want.degree, want.log_quotient_degree)
    assert got.width == A.WIDTHS[chip]
    assert 1 <= got.live_values <= 32
    assert got.instructions >= got.num_constraints


@pytest.mark.parametrize("chip", [1, 4, 5, -1, 8])
def test_export_refuses_the_chips_uni_info_refuses(chip):
    with pytest.raises(sdk.BfzError) as want:
        sdk.uni_stark_info(chip)
    with pytest.raises(sdk.BfzError) as got:
        sdk.air_export(chip)
    assert str(got.value) == str(want.value)


def test_custom_shapes():
    prog, _, _, _ = A.fib_case(4)
    i = sdk.air_info(prog)
    assert (i.width, i.num_constraints, i.degree, i.log_quotient_degree) == (2, 5, 2, 0)
    i = sdk.air_info(A.mulgate_program())
    assert (i.width, i.num_constraints, i.degree, i.log_quotient_degree) == (4, 3, 3, 1)
    assert NEG in [n[0] for n in struct.iter_unpack("<III", A.mulgate_program()[16:16 + 12 * i.num_nodes])]


# ---------------------------------------------------------------------------- bfz_air_eval
@pytest.mark.parametrize("chip", [ADDSUB, IO])
def test_eval_of_exported_programs_equals_the_model(chip):
    rng = np.random.default_rng([chip, 11])
    for _ in range(8):
        got, want = eval_both(A.export(chip), M.AIRS[chip], A.WIDTHS[chip], rng)
        assert got == want


def test_eval_of_custom_programs_equals_their_mirrors():
    rng = np.random.default_rng(12)
    for kind, height, width in (("fib", 4, 2), ("fib", 256, 2), ("mulgate", 16, 4)):
        prog, mirror, _, _ = A.custom_case(kind, height)
        for _ in range(8):
            got, want = eval_both(prog, mirror, width, rng)
            assert got == want, kind


def test_builder_round_trip_addsub():
    """AddSub written by hand from the model's expressions evaluates as the export does."""
    ab = sdk.AirBuilder(7)
    value, carry, a, b, is_add, is_sub = (ab.local(c) for c in (1, 2, 3, 4, 5, 6))
    is_real = is_add + is_sub
    boolc = lambda x: x * (x - 1)
    ab.assert_zero(boolc(is_add))
    ab.assert_zero(boolc(is_sub))
    ab.assert_zero(boolc(is_real))
    overflow = a + b - value
    ab.assert_zero(is_real * (overflow * (overflow - 256)))
    ab.assert_zero(is_real * (carry * (overflow - 256)))
    ab.assert_eq(is_real * ((carry - 1) * overflow), 0)
    ab.assert_zero(is_real * boolc(carry))
    ab.assert_zero(is_real * boolc(is_real))
    prog = ab.build()
    hand, exp = sdk.air_info(prog), sdk.air_info(A.export(ADDSUB))
    assert (hand.num_constraints, hand.degree, hand.log_quotient_degree) == \
        (exp.num_constraints, exp.degree, exp.log_quotient_degree)
    for seed in range(8):
        got, _ = eval_both(prog, M.AIRS[ADDSUB], 7, np.random.default_rng([seed, 13]))
        want, _ = eval_both(A.export(ADDSUB), M.AIRS[ADDSUB], 7, np.random.default_rng([seed, 13]))
        assert got == want


# ---------------------------------------------------------------------------- the host row check
@pytest.mark.parametrize("chip", sdk.UNI_STARK_CHIPS)
def test_host_check_equals_the_compiled_check(chip):
    prog_src, stdin, height = U.SMALL[chip]
    trace = U.trace_of(chip, prog_src, stdin)
    assert trace.shape == (height, A.WIDTHS[chip])
    traces = [trace] + [U.corrupt(trace, *c) for c in U.corruptions(chip, height, trace.shape[1])]
    failing = 0
    for t in traces:
        want = sdk.uni_stark_check(chip, t, on_device=False, per_row=True)
        got = sdk.air_check(A.export(chip), t, on_device=False, per_row=True)
        assert got.chip == -1
        assert A.summary(got)[1:] == A.summary(want)[1:]
        assert np.array_equal(got.first_fail_per_row, want.first_fail_per_row)
        failing += want.failing_rows > 0
    assert failing >= len(traces) // 2  # the corruptions are not vacuous


def test_host_check_of_custom_programs_equals_their_mirrors():
    for kind, height in (("fib", 1), ("fib", 4), ("fib", 256), ("mulgate", 1), ("mulgate", 16)):
        prog, mirror, trace, rows = A.custom_case(kind, height)
        k = sdk.air_info(prog).num_constraints
        got = sdk.air_check(prog, trace, on_device=False, per_row=True)
        assert A.summary(got) == (-1, height, k, 0, -1, -1), (kind, height)
        for r in sorted({0, height // 2, height - 1}):
            for col in range(trace.shape[1]):
                bad = A.flip(trace, r, col)
                want = A.mirror_rows(mirror, A.canonical(bad))
                got = sdk.air_check(prog, bad, on_device=False, per_row=True)
                assert np.array_equal(got.first_fail_per_row, want), (kind, height, r, col)
                assert A.summary(got) == A.summary_from_rows(want, k)


# ---------------------------------------------------------------------------- the host verifier
def uni_verify_one(chip, proof):
    return U.verify_one(chip, proof)


def sections(proof):
    """(section, byte offset of one word in it) over the whole BFU1 layout; for a section of many
    words the first and the last (the sample tests/test_uni_stark.py takes)."""
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
def test_fixtures_and_their_mutations_verify_as_the_chip_does(f):
    proof = bytes.fromhex(f["proof"])
    chip, prog = f["chip"], A.export(f["chip"])
    name = sdk.CHIPS[chip]
    sdk.set_num_queries(f["num_queries"])
    got, want = A.air_verify_one(prog, proof), uni_verify_one(chip, proof)
    assert got == want and got[0] == (True, -1, "")  # the same ending challenger too
    seen = set()
    for section, off in sections(proof):
        for bit in (1, 1 << 20):
            (v,) = struct.unpack_from("<I", proof, off)
            bad = proof[:off] + struct.pack("<I", v ^ bit) + proof[off + 4:]
            (ok, query, why), _ = A.air_verify_one(prog, bad)
            (ok_u, query_u, why_u), _ = uni_verify_one(chip, bad)
            if section == "chip" and why_u == "proof is for another chip":
                # the one word the two treat differently by design: for a program the chip word
                # is a label outside the transcript and is not interpreted
                assert ok and why == ""
                continue
            assert (ok, query) == (ok_u, query_u) and not ok, (section, bit)
            assert why == why_u.replace("chip " + name, "chip custom"), (section, bit)
            seen.add(why)
    assert len(seen) >= 4  # several stages of the verifier were reached
    # another chip's program of the same proof: the shapes or the identity fail, never a crash
    other = ADDSUB if chip != ADDSUB else IO
    (ok, _, why), _ = A.air_verify_one(A.export(other), proof)
    assert not ok and why in ("opened-value shape mismatch", "OOD evaluation mismatch on chip custom")


def test_uni_verify_rejects_a_program_proofs_label():
    f = FIXTURES[IDS.index("addsub16")]
    proof = bytearray(bytes.fromhex(f["proof"]))
    struct.pack_into("<I", proof, 4, sdk.AIR_CHIP)
    sdk.set_num_queries(f["num_queries"])
    assert uni_verify_one(ADDSUB, bytes(proof))[0] == (False, -1, "proof is for another chip")
    assert A.air_verify_one(A.export(ADDSUB), bytes(proof))[0] == (True, -1, "")


# ---------------------------------------------------------------------------- validation
L0 = (LOCAL, 0, 0)


def sum_of_squares(n):
    """n squares of distinct columns, all computed before the first is read: n live values."""
    nodes = [(LOCAL, c, 0) for c in range(n)]
    nodes += [(MUL, c, c) for c in range(n)]
    acc = n
    for c in range(1, n):
        nodes.append((ADD, acc, n + c))
        acc = len(nodes) - 1
    return raw(n, nodes, [acc])


MALFORMED = {
    "bad magic": (b"BFA2" + raw(1, [L0], [0])[4:], "word 0"),
    "short": (raw(1, [L0], [0])[:-4], "word"),
    "short header": (raw(1, [L0], [0])[:12], "word 0"),
    "odd length": (raw(1, [L0], [0]) + b"\0", "word"),
    "long": (raw(1, [L0], [0]) + b"\0\0\0\0", "word"),
    "forward operand": (raw(1, [L0, (ADD, 1, 0)], [1]), "word 8"),
    "forward operand b": (raw(1, [L0, (ADD, 0, 2), L0], [1]), "word 9"),
    "forward operand of neg": (raw(1, [(NEG, 0, 0)], [0]), "word 5"),
    "column = width": (raw(3, [(NEXT, 3, 0)], [0]), "word 5"),
    "constant = p": (raw(1, [(CONST, P, 0)], [0]), "word 5"),
    "unknown op": (raw(1, [(10, 0, 0)], [0]), "word 4"),
    "used unused operand": (raw(1, [(LOCAL, 0, 1)], [0]), "word 6"),
    "zero constraints": (raw(1, [L0], []), "word 3"),
    "constraint out of range": (raw(1, [L0], [1]), "word 7"),
    "degree 4": (raw(1, [L0, (MUL, 0, 0), (MUL, 1, 1)], [2]), "degree above 3"),
    "33 live values": (sum_of_squares(33), "33"),
    "width 0": (raw(0, [(FIRST, 0, 0)], [0]), "word 1"),
    "width 65": (raw(65, [L0], [0]), "word 1"),
    "4097 nodes": (raw(1, [L0] * 4097, [0]), "word 2"),
    "513 constraints": (raw(1, [L0], [0] * 513), "word 3"),
    "header counts beyond the bytes": (raw(1, [L0], [0], n_nodes=4096), "word"),
}


@pytest.mark.parametrize("what", list(MALFORMED))
def test_malformed_programs_are_refused(what):
    prog, needle = MALFORMED[what]
    rc, msg = A.air_info_status(prog)
    assert rc < 0 and needle in msg, (rc, msg)
    # every entry point validates first (the host ones need no device)
    out = _lib.VerifyOutcomeC()
    ch = sdk.Challenger()
    pbuf, pn = _lib.u8buf(prog)
    buf, n = _lib.u8buf(bytes.fromhex(FIXTURES[0]["proof"]))
    assert _lib.lib().bfz_air_verify(pbuf, pn, ctypes.byref(ch), buf, n, ctypes.byref(out)) < 0
    with pytest.raises(sdk.BfzError):
        sdk.air_check(prog, np.zeros((4, 1), dtype=np.uint32), on_device=False)


def test_the_limits_themselves_are_accepted():
    assert sdk.air_info(sum_of_squares(32)).live_values == 32
    assert sdk.air_info(raw(64, [(LOCAL, 63, 0)], [0])).width == 64
    assert sdk.air_info(raw(1, [L0] * 4096, [4095] * 512)).num_constraints == 512
    cubic = sdk.air_info(raw(1, [L0, (MUL, 0, 0), (MUL, 1, 0)], [2]))
    assert (cubic.degree, cubic.log_quotient_degree) == (3, 1)


def test_degree_rules():
    """is_transition and constants count 0, the other selectors and columns 1; add / sub take the
    maximum, mul the sum, neg nothing."""
    def degree(nodes):
        return sdk.air_info(raw(2, nodes, [len(nodes) - 1])).degree
    assert degree([(CONST, 5, 0)]) == 0
    assert degree([(TRANS, 0, 0)]) == 0
    assert degree([(FIRST, 0, 0)]) == degree([(LAST, 0, 0)]) == degree([(NEXT, 1, 0)]) == 1
    assert degree([L0, (TRANS, 0, 0), (MUL, 0, 1), (MUL, 2, 1)]) == 1
    assert degree([L0, (FIRST, 0, 0), (MUL, 0, 1), (NEG, 2, 0), (SUB, 3, 0), (ADD, 4, 1)]) == 2
    # an unreachable node does not count
    assert degree([L0, (MUL, 0, 0), (MUL, 1, 1), (ADD, 0, 0)]) == 1


def test_random_single_word_mutations_never_crash():
    base = A.export(JUMP)
    nwords = len(base) // 4
    info = sdk.air_info(base)
    zero = np.zeros((info.width, 4), dtype=np.uint32)
    rng = np.random.default_rng(2024)
    refused = valid = 0
    for k in range(2000):
        at = int(rng.integers(0, nwords))
        (old,) = struct.unpack_from("<I", base, 4 * at)
        new = old
        while new == old:  # small values hit live fields, large ones the range checks
            new = int(rng.integers(0, 16)) if k % 2 else int(rng.integers(0, 1 << 32))
        prog = base[:4 * at] + struct.pack("<I", new) + base[4 * at + 4:]
        rc, msg = A.air_info_status(prog)
        if rc != 0:
            assert rc < 0 and msg, at
            refused += 1
            continue
        got = sdk.air_info(prog)
        assert got.live_values <= 32 and got.degree <= 3
        z = np.zeros((got.width, 4), dtype=np.uint32)
        assert sdk.air_eval(prog, z, z, zero[0], zero[0], zero[0]).shape == (got.num_constraints, 4)
        valid += 1
    assert refused >= 200 and valid >= 200  # both outcomes are exercised
