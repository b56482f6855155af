"""CPU tests of bfz_verify_batch's host path (on_device = 0) and of its argument checks."""
import ctypes

import pytest

import bincode_ref as BR
import oracle_lib as O
from bfz import _lib, guests, sdk


def _vk(prog):
    return sdk.BfVerifyingKey(commit=[O.to_mont(x) for x in O.setup_root(prog)], elf=prog)


@pytest.fixture(scope="module")
def hello():
    return O.prove(guests.HELLO, [])


def _reason(pf, vk):
    """bfz_verify's reason for rejecting pf."""
    with pytest.raises(_lib.BfzError, match="verification failed: ") as e:
        sdk.ProverClient().verify(sdk.BfProofWithPublicValues(proof=pf, stdin=b""), vk)
    return str(e.value).split("verification failed: ", 1)[1]


def _tamper_query(pf, q):
    m = BR.parse_bfz1(pf)
    row = m["queries"][q]["inputs"][1]["rows"][0]
    row[0] = (row[0] + 1) % BR.P
    return BR.encode_bfz1(m)


def test_host_batch_reports_each_proof(hello):
    vk = _vk(guests.HELLO)
    bad = _tamper_query(hello, 5)
    out = sdk.ProverClient().verify_batch([hello, bad, hello], vk, on_device=False)
    assert [(o.ok, o.query, o.why) for o in out] == [
        (True, -1, ""), (False, 5, _reason(bad, vk)), (True, -1, "")]
    assert out[1].why == "input Merkle opening rejected"


def test_rejections_outside_the_query_loop_have_no_query(hello):
    vk = _vk(guests.HELLO)
    m = BR.parse_bfz1(hello)
    m["opened"][0]["cumsum"][0] = (m["opened"][0]["cumsum"][0] + 1) % BR.P
    bad = BR.encode_bfz1(m)
    o = sdk.ProverClient().verify_batch([bad], vk, on_device=False)[0]
    assert (o.ok, o.query) == (False, -1) and o.why == _reason(bad, vk)


def test_truncated_proof_does_not_affect_its_neighbours(hello):
    vk = _vk(guests.HELLO)
    cut = hello[: len(hello) // 3]
    out = sdk.ProverClient().verify_batch([hello, cut, b"", hello], vk, on_device=False)
    assert [o.ok for o in out] == [True, False, False, True]
    assert (out[1].query, out[1].why) == (-1, _reason(cut, vk))
    assert (out[2].query, out[2].why) == (-1, _reason(b"", vk))


def test_empty_batch_and_null_arguments(hello):
    L = _lib.lib()
    vk = _vk(guests.HELLO)
    commit = (ctypes.c_uint32 * 8)(*vk.commit)
    assert sdk.ProverClient().verify_batch([], vk, on_device=False) == []
    assert L.bfz_verify_batch(vk.elf.encode(), commit, None, None, 0, 0, None) == 0
    buf, n = _lib.u8buf(hello)
    arr = (ctypes.POINTER(ctypes.c_uint8) * 1)(ctypes.cast(buf, ctypes.POINTER(ctypes.c_uint8)))
    lens = (ctypes.c_size_t * 1)(n)
    out = (_lib.VerifyOutcomeC * 1)()
    assert L.bfz_verify_batch(vk.elf.encode(), commit, arr, lens, 1, 0, None) < 0
    assert b"null argument" in L.bfz_last_error()
    assert L.bfz_verify_batch(None, commit, arr, lens, 1, 0, out) < 0
    assert L.bfz_verify_batch(vk.elf.encode(), commit, arr, lens, 1, 0, out) == 0 and out[0].ok == 1


def test_honours_query_count_and_pcs_variant():
    prog = "+"
    vk = _vk(prog)
    c = sdk.ProverClient()
    pf5 = O.prove(prog, [], num_queries=5)
    pfv = O.prove(prog, [], observe_openings=False)
    assert [o.why for o in c.verify_batch([pf5, pfv], vk, on_device=False)] == [
        "wrong number of queries", _reason(pfv, vk)]
    try:
        sdk.set_num_queries(5)
        assert c.verify_batch([pf5], vk, on_device=False)[0].ok
    finally:
        sdk.set_num_queries(0)
    try:
        sdk.set_pcs_variant(0)
        assert c.verify_batch([pfv], vk, on_device=False)[0].ok
    finally:
        sdk.set_pcs_variant(-1)


def test_final_value_mismatch_is_what_a_tampered_one_row_opening_gives():
    """The mutation tests/test_verify_device.py sends through the device: with the opened values
    out of the transcript, a changed opened value of the 1-row Cpu trace reaches the fold chain's
    end through the height-2 reduced opening (D11) and nothing else."""
    prog = "+"
    m = BR.parse_bfz1(O.prove(prog, [], observe_openings=False))
    i = [k for k, o in enumerate(m["opened"]) if o["log_degree"] == 0][0]
    m["opened"][i]["main_local"][0][0] = (m["opened"][i]["main_local"][0][0] + 1) % BR.P
    try:
        sdk.set_pcs_variant(0)
        o = sdk.ProverClient().verify_batch([BR.encode_bfz1(m)], _vk(prog), on_device=False)[0]
    finally:
        sdk.set_pcs_variant(-1)
    assert (o.ok, o.query, o.why) == (False, 0, "FRI final value mismatch")


def test_device_path_without_a_device_is_an_error_not_a_fallback(hello):
    """on_device = 1 in a process that has bound no device fails; it does not quietly run the
    host verifier.  Whether a device is bound is the process's state, and another test of this
    session may have bound one, so the call is made in a fresh process that never calls bfz_init
    (the library loaded bare: it touches no GPU before bfz_init)."""
    import subprocess
    import sys
    import tempfile
    code = (
        "import ctypes, sys\n"
        "L = ctypes.CDLL(sys.argv[1]); pf = open(sys.argv[2], 'rb').read()\n"
        "L.bfz_last_error.restype = ctypes.c_char_p\n"
        "buf = (ctypes.c_uint8 * len(pf)).from_buffer_copy(pf)\n"
        "arr = (ctypes.c_void_p * 1)(ctypes.addressof(buf)); lens = (ctypes.c_size_t * 1)(len(pf))\n"
        "out = ctypes.create_string_buffer(b'\\x07' * 128, 128); vk = (ctypes.c_uint32 * 8)()\n"
        "rc = L.bfz_verify_batch(sys.argv[3].encode(), vk, arr, lens, ctypes.c_size_t(1), 1, out)\n"
        "print(rc, out.raw == b'\\x07' * 128, L.bfz_last_error().decode())\n")
    with tempfile.NamedTemporaryFile(suffix=".bfz1") as fh:
        fh.write(hello)
        fh.flush()
        r = subprocess.run([sys.executable, "-c", code, _lib.LIB_PATH, fh.name, guests.HELLO],
                           capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rc, untouched, msg = r.stdout.strip().split(" ", 2)
    assert int(rc) < 0 and untouched == "True" and "no device bound" in msg


def claimed_heights_mutation(pf):
    """The Program and Byte chips claim log degrees that are not their key's (and no other
    chip's).  The log degrees are not in the transcript, so every challenge and the PoW witness
    stay valid and the proof gets as far as the query loop -- with two more LDE heights than an
    honest proof can have, which the packed descriptor does not hold."""
    m = BR.parse_bfz1(pf)
    used = {o["log_degree"] for o in m["opened"]}
    free = [d for d in range(16, 0, -1) if d not in used]
    for name, d in zip(("Byte", "Program"), free):
        m["opened"][[BR.CHIPS[c] for c in m["chips"]].index(name)]["log_degree"] = d
    heights = {o["log_degree"] for o in m["opened"]} | used
    assert len(heights) > 8
    return BR.encode_bfz1(m)


def misshapen_cases(pf):
    """A query of another shape than the proof's (one path digest short) stops the packing: the
    queries before it go to the device, it and the later ones stay on the host.  (bytes, the
    host's outcome; a commit-phase sibling of query bump_q is changed as well.)"""
    def make(short_q, bump_q):
        m = BR.parse_bfz1(pf)
        m["queries"][short_q]["inputs"][1]["path"].pop()
        if bump_q is not None:
            sib = m["queries"][bump_q]["steps"][2]["sibling"]
            sib[1] = (sib[1] + 1) % BR.P
        return BR.encode_bfz1(m)
    return [(make(40, None), (False, 40, "bad path length")),
            (make(40, 10), (False, 10, "FRI commit-phase opening rejected")),  # fails on the device
            (make(40, 60), (False, 40, "bad path length")),  # a later query is never reached
            (make(0, None), (False, 0, "bad path length"))]  # nothing left for the device


def test_host_side_of_the_device_path_without_a_device(hello):
    """bfz_set_fault_injection bit 1 puts a stand-in that reports no failure in the kernels'
    place, so the device path's host side runs here: a proof whose packing is refused (more
    heights than a descriptor holds) is that proof's rejection with the host's reason, not an
    error of the call, and its neighbours keep their verdicts; queries from the first misshapen
    one on are checked on the host."""
    vk = _vk(guests.HELLO)
    c = sdk.ProverClient()
    crafted = claimed_heights_mutation(hello)
    shaped = misshapen_cases(hello)
    batch = [hello, crafted, hello] + [b for b, _ in shaped]
    host = [(o.ok, o.query, o.why) for o in c.verify_batch(batch, vk, on_device=False)]
    assert host[0] == host[2] == (True, -1, "")
    assert host[1][:2] == (False, 0) and host[1][2] in ("bad path length",
                                                        "input Merkle opening rejected")
    assert host[3:] == [want for _, want in shaped]
    L = _lib.lib()
    commit = (ctypes.c_uint32 * 8)(*vk.commit)
    bufs = [_lib.u8buf(x) for x in batch]
    arr = (ctypes.POINTER(ctypes.c_uint8) * len(batch))(
        *[ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)) for b, _ in bufs])
    lens = (ctypes.c_size_t * len(batch))(*[n for _, n in bufs])
    out = (_lib.VerifyOutcomeC * len(batch))()
    try:
        _lib.check(L.bfz_set_fault_injection(2))
        rc = L.bfz_verify_batch(vk.elf.encode(), commit, arr, lens, len(batch), 1, out)
    finally:
        _lib.check(L.bfz_set_fault_injection(0))
    assert rc == 0, L.bfz_last_error()
    got = [(bool(o.ok), o.query, o.why.decode()) for o in out]
    # the stand-in passes the queries the device would have failed: case (40, 10) reaches query 40
    want = list(host)
    want[4] = (False, 40, "bad path length")
    assert got == want
