"""The uni-STARK additions on the device: bfz_record_uni_prove against bfz_uni_prove on the host
trace (bytes and ending challenger), the row-check kernel (bfz_uni_check with on_device = 1,
bfz_record_uni_check) against its host path, and bfz_uni_verify_batch's device query phase
against the host verifier on a mixed batch of good and mutated proofs.

Each shape is the smallest at which the named thing can go wrong; 6 queries throughout."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import uni_device_cases as C
from bfz import _lib, guests, sdk
from uni_device_cases import ADDSUB, CPU, IO, JUMP, MEMINSTRS

pytestmark = pytest.mark.gpu

INPUT_REJECTED = "input Merkle opening rejected"
COMMIT_REJECTED = "FRI commit-phase opening rejected"
FINAL_MISMATCH = "FRI final value mismatch"
BAD_POW = "bad PoW witness"


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.init(0)
    sdk.set_num_queries(C.QUERIES)
    yield
    sdk.set_num_queries(0)
    sdk.set_pcs_variant(-1)


class Record:
    """bfz_setup + bfz_record_new of (program, stdin); freed on exit."""

    def __init__(self, prog, stdin=()):
        self.client = sdk.ProverClient()
        self.pk, _ = self.client.setup(prog)
        buf, n = _lib.u8buf(bytes(stdin))
        self.rec = ctypes.c_void_p()
        _lib.check(_lib.lib().bfz_record_new(ctypes.c_void_p(self.pk.handle), buf, n,
                                             ctypes.byref(self.rec), None))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _lib.lib().bfz_record_free(self.rec)

    def uni_prove(self, chip, timings=None):
        """(status, proof bytes or None, the ending challenger's bytes)"""
        ch = sdk.Challenger()
        ptr, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t()
        rc = _lib.lib().bfz_record_uni_prove(self.rec, chip, ctypes.byref(ch), ctypes.byref(ptr),
                                             ctypes.byref(n),
                                             ctypes.byref(timings) if timings is not None else None)
        return rc, (_lib.take_bytes(ptr, n.value) if rc == 0 else None), bytes(ch)

    def uni_check(self, chip):
        out = _lib.UniCheckC()
        rc = _lib.lib().bfz_record_uni_check(self.rec, chip, ctypes.byref(out))
        return rc, out

    def machine_proof(self):
        ptr, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t()
        _lib.check(_lib.lib().bfz_record_prove(ctypes.c_void_p(self.pk.handle), self.rec,
                                               ctypes.byref(ptr), ctypes.byref(n), None))
        return _lib.take_bytes(ptr, n.value)


def host_prove(chip, trace):
    ch = sdk.Challenger()
    return sdk.uni_stark_prove(chip, trace, ch), bytes(ch)


# ---------------------------------------------------------------------------- record prove
RECORD_CASES = [
    ("cpu-1", CPU, "+", (), 1),                 # no FRI round
    ("cpu-512", CPU, guests.HELLO, (), 512),
    ("addsub-32", ADDSUB, "+" * 17, (), 32),
    ("jump-32", JUMP, guests.HELLO, (), 32),
    ("meminstrs-16", MEMINSTRS, ">", (), 16),
    ("io-16", IO, ".", (), 16),                 # one chunk
    ("cpu-65536", CPU, guests.FIBO, (17,), 65536),  # the multi-pass LDE
]


@pytest.mark.parametrize("name,chip,prog,stdin,height", RECORD_CASES, ids=[c[0] for c in RECORD_CASES])
def test_record_prove_equals_host_trace_prove(name, chip, prog, stdin, height):
    trace = C.trace_of(chip, prog, stdin)
    assert trace.shape[0] == height
    want, ch_want = host_prove(chip, trace)
    with Record(prog, stdin) as r:
        before = r.machine_proof()
        rc, got, ch_got = r.uni_prove(chip)
        assert rc == 0 and got == want and ch_got == ch_want
        t = _lib.Timings()
        rc, again, ch_again = r.uni_prove(chip, t)  # a second call on the same record, timed
        assert rc == 0 and again == want and ch_again == ch_want
        assert t.trace_ms > 0 and t.total_ms >= t.trace_ms + t.main_commit_ms
        assert r.machine_proof() == before  # the record is as it was
    assert C.verify_one(chip, got)[0] == (True, -1, "")


def test_record_without_the_chip_and_refused_chips():
    with Record("+") as r:
        assert r.uni_prove(IO)[0] == 1
        assert r.uni_check(IO)[0] == 1
        for chip in (1, 4, 5, 8, -1):
            assert r.uni_prove(chip)[0] < 0 and b"uni_stark" in _lib.lib().bfz_last_error()
            assert r.uni_check(chip)[0] < 0 and b"uni_stark" in _lib.lib().bfz_last_error()
        assert r.uni_prove(CPU)[0] == 0


def test_sdk_prove_record():
    client = sdk.ProverClient()
    pk, _ = client.setup(guests.HELLO)
    proofs = client.uni_stark_prove_record(pk, [], check=True)
    assert sorted(proofs) == list(sdk.UNI_STARK_CHIPS)  # HELLO includes all five
    for chip, proof in proofs.items():
        assert proof == host_prove(chip, C.trace_of(chip, guests.HELLO))[0]
    pk, _ = client.setup("+")
    assert sorted(client.uni_stark_prove_record(pk, [])) == [CPU, ADDSUB]
    assert sorted(client.uni_stark_prove_record(pk, [], chips=(IO, ADDSUB))) == [ADDSUB]


# ---------------------------------------------------------------------------- row check
def both_checks(chip, trace):
    host = sdk.uni_stark_check(chip, trace, on_device=False, per_row=True)
    dev = sdk.uni_stark_check(chip, trace, on_device=True, per_row=True)
    assert np.array_equal(dev.first_fail_per_row, host.first_fail_per_row)
    assert C.summary(dev) == C.summary(host) == C.summary_from_rows(chip, host.first_fail_per_row)
    nosum = sdk.uni_stark_check(chip, trace, on_device=True)  # without the per-row array
    assert C.summary(nosum) == C.summary(host) and nosum.first_fail_per_row is None
    return host


CHECK_CASES = [(chip,) + C.SMALL[chip] + (C.N_CORRUPTIONS,) for chip in sdk.UNI_STARK_CHIPS] + [
    (CPU, "+", (), 1, 4),                    # the row is its own next row
    (IO, ".", (), 16, 8),
    (CPU, guests.HELLO, (), 512, 8),         # two blocks
    (CPU, guests.FIBO, (17,), 65536, 6),     # 256 blocks: the cross-block atomicMin, bit-reversed
]                                            # storage against natural-order output


@pytest.mark.parametrize("chip,prog,stdin,height,count", CHECK_CASES,
                         ids=[f"{sdk.CHIPS[c[0]]}-{c[3]}" for c in CHECK_CASES])
def test_device_row_check_equals_host(chip, prog, stdin, height, count):
    trace = C.trace_of(chip, prog, stdin)
    assert trace.shape[0] == height
    assert both_checks(chip, trace).failing_rows == 0
    cases = C.corruptions(chip, height, trace.shape[1], count=count)
    assert cases[1][0] == height - 1 and cases[2][0] >= height - 256  # row h-1, the last block
    if chip == CPU:  # is_real = 2 fails the row's own boolean constraint on any row, padding too:
        cases += [(height - 1, 30, 2), (max(height - 100, 0), 30, 2)]  # row h-1, the last block
    failed = 0
    for row, col, value in cases:
        res = both_checks(chip, C.corrupt(trace, row, col, value))
        rows = set(np.nonzero(res.first_fail_per_row >= 0)[0].tolist())
        assert rows <= {(row - 1) % height, row}
        assert row in rows or (col, value) != (30, 2)
        failed += res.failing_rows > 0
    assert failed  # some corruption is one the AIR sees
    # several failing rows in different blocks: the smallest row wins, the count adds up
    bad = np.array(trace, dtype=np.uint32)
    for row, col, value in cases:
        bad = C.corrupt(bad, row, col, value)
    both_checks(chip, bad)


def test_device_row_check_on_an_invalid_real_trace_and_refusals():
    res = both_checks(MEMINSTRS, C.trace_of(MEMINSTRS, "<+"))
    assert res.failing_rows >= 1 and res.first_row == 0
    good = C.trace_of(ADDSUB, "+")
    for what, (rc, msg) in {
        "Byte": C.uni_check_status(5, np.zeros((16, 2), dtype=np.uint32), 1),
        "width": C.uni_check_status(ADDSUB, good[:, :6], 1),
        "height 12": C.uni_check_status(ADDSUB, good[:12], 1),
        "word >= p": C.uni_check_status(ADDSUB, np.full((16, 7), O.P, dtype=np.uint32), 1),
    }.items():
        assert rc < 0 and msg.startswith("uni_stark: "), what
    assert C.uni_check_status(ADDSUB, good, 1) == (0, "")


def test_record_check_is_clean_on_fibo17():
    with Record(guests.FIBO, (17,)) as r:
        seen = []
        for chip in sdk.UNI_STARK_CHIPS:
            rc, out = r.uni_check(chip)
            assert rc == 0
            t = C.trace_of(chip, guests.FIBO, (17,))
            assert C.summary(out) == (chip, t.shape[0], sdk.uni_stark_info(chip).num_constraints, 0, -1, -1)
            seen.append(chip)
        assert seen == list(sdk.UNI_STARK_CHIPS)


# ---------------------------------------------------------------------------- batch verify
def mixed_batch():
    """[(chip, trace)]: Cpu h = 1, Cpu 512, AddSub 32, Jump 32, MemoryInstrs 64, IO 16 and IO h = 2
    on an all-zero trace (all-zero rows satisfy IO's AIR)."""
    return [(CPU, C.trace_of(CPU, "+")), (CPU, C.trace_of(CPU, guests.HELLO)),
            (ADDSUB, C.trace_of(ADDSUB, "+" * 17)), (JUMP, C.trace_of(JUMP, guests.HELLO)),
            (MEMINSTRS, C.trace_of(MEMINSTRS, guests.HELLO)), (IO, C.trace_of(IO, ".")),
            (IO, np.zeros((2, 5), dtype=np.uint32))]


def mutations(proof, seed, count=24):
    """count copies of the proof with one word ^= 1, one word from each of `count` equal
    stretches of the proof: spread over header, every query and the tail."""
    rng = np.random.default_rng([seed, len(proof)])
    words = len(proof) // 4
    out = []
    for k in range(count):
        lo, hi = k * words // count, (k + 1) * words // count
        off = 4 * int(rng.integers(lo, hi))
        out.append(proof[:off] + bytes([proof[off] ^ 1]) + proof[off + 1:])
    return out


def run_mixed(observe_openings, extra=()):
    """Proves the mixed batch under the given PCS variant and verifies good and mutated proofs,
    interleaved, in ONE call per mode; returns the host's reasons for the mutated proofs."""
    sdk.set_pcs_variant(observe_openings)
    try:
        heights = [t.shape[0] for _, t in mixed_batch()]
        assert heights == [1, 512, 32, 32, 64, 16, 2]
        chips, proofs, mutated, want_ch = [], [], [], []
        for i, (chip, trace) in enumerate(mixed_batch()):
            good, ch = host_prove(chip, trace)
            for bad in mutations(good, seed=5 + i):
                chips += [chip, chip]
                proofs += [good, bad]
                mutated += [False, True]
                want_ch += [ch, None]
        for chip, proof in extra:
            chips.append(chip)
            proofs.append(proof)
            mutated.append(True)
            want_ch.append(None)
        host = C.verify_batch(chips, proofs, on_device=False)
        dev = C.verify_batch(chips, proofs, on_device=True)
    finally:
        sdk.set_pcs_variant(-1)
    for i, (h, d) in enumerate(zip(host, dev)):
        assert d == h, (i, chips[i], mutated[i])  # (ok, query, why) and the ending challenger
        if mutated[i]:
            assert not h[0][0] and h[0][2], i  # the host rejects every mutated proof
        else:
            assert h == ((True, -1, ""), want_ch[i]), i  # accepted, the prover's challenger
    return [h[0] for h, m in zip(host, mutated) if m]


def test_mixed_batch_device_equals_host():
    """Which reasons single-word changes can reach.  Every word of a BFU1 proof outside the query
    openings is observed by the transcript before the PoW check (commitments, opened values under
    the default PCS variant, commit-phase roots, the final value, the witness itself), so changing
    one gives "bad PoW witness" except with probability 2^-16, and every word inside the query
    openings is bound by a Merkle path, so changing one gives one of the two opening reasons.
    "FRI final value mismatch" therefore needs opened values that stay out of the transcript --
    the other PCS variant (bfz_set_pcs_variant(0)), which the call must honour anyway -- and an
    out-of-domain mismatch needs a proof whose openings are consistent but whose trace is not
    valid: the proof of the corrupted AddSub trace, appended to the same call.  All five reasons
    are asserted over these runs, each compared between the two modes."""
    bad = np.array(C.trace_of(ADDSUB, "+" * 17), dtype=np.uint32)
    bad[3, 1] = O.to_mont((O.from_mont(int(bad[3, 1])) + 1) % O.P)
    invalid = host_prove(ADDSUB, bad)[0]
    seen = run_mixed(1, extra=[(ADDSUB, invalid)]) + run_mixed(0)
    whys = {w for _, _, w in seen}
    assert any(w == INPUT_REJECTED and q > 0 for _, q, w in seen)
    assert {COMMIT_REJECTED, FINAL_MISMATCH, BAD_POW, "OOD evaluation mismatch on chip AddSub"} <= whys


def test_invalid_trace_is_caught_by_the_check_and_by_both_verifiers():
    bad = np.array(C.trace_of(ADDSUB, "+" * 17), dtype=np.uint32)
    bad[3, 1] = O.to_mont((O.from_mont(int(bad[3, 1])) + 1) % O.P)
    with pytest.raises(sdk.BfzError, match=r"AddSub: 1 failing row\(s\); first: row 3, AIR constraint 3 of 8"):
        sdk.uni_stark_prove(ADDSUB, bad, check=True)
    good = C.trace_of(ADDSUB, "+" * 17)
    assert sdk.uni_stark_prove(ADDSUB, good, check=True) == host_prove(ADDSUB, good)[0]
    proof = sdk.uni_stark_prove(ADDSUB, bad)  # check=False: an invalid trace still proves
    for on_device in (False, True):
        outs = sdk.uni_stark_verify_batch([ADDSUB, ADDSUB], [proof, host_prove(ADDSUB, good)[0]],
                                          on_device=on_device)
        assert (outs[0].ok, outs[0].query, outs[0].why) == (False, -1, "OOD evaluation mismatch on chip AddSub")
        assert outs[1].ok
