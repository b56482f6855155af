"""GPU tests of the device verifier (bfz_verify_batch with on_device = 1): the query phase of a
batch of proofs in one device pass must give, proof by proof, exactly the host verifier's outcome
(ok, first failing query, reason).  The reference of every comparison is the host verifier
(on_device = 0) on the same bytes; for acceptance it is the oracle's own proofs, which no GPU code
produced."""
import random
import struct

import pytest

import bincode_ref as BR
import oracle_lib as O
from bfz import guests, sdk
from test_verify_batch import claimed_heights_mutation, misshapen_cases

pytestmark = pytest.mark.gpu

P = BR.P
INPUT_REJECTED = "input Merkle opening rejected"
COMMIT_REJECTED = "FRI commit-phase opening rejected"
FINAL_MISMATCH = "FRI final value mismatch"
QUERY_REASONS = (INPUT_REJECTED, COMMIT_REJECTED, FINAL_MISMATCH)


def _vk(prog):
    return sdk.BfVerifyingKey(commit=[O.to_mont(x) for x in O.setup_root(prog)], elf=prog)


def _both(proofs, vk):
    """[(ok, query, why)] of the host path and of the device path over the same bytes."""
    c = sdk.ProverClient()
    host = [(o.ok, o.query, o.why) for o in c.verify_batch(proofs, vk, on_device=False)]
    dev = [(o.ok, o.query, o.why) for o in c.verify_batch(proofs, vk, on_device=True)]
    return host, dev


def _bump(words, i):
    words[i] = (words[i] + 1) % P  # stays canonical, so the proof still decodes


@pytest.fixture(scope="module")
def hello():
    return O.prove(guests.HELLO, [])


# ------------------------------------------------------------------ 1. honest proofs
@pytest.mark.parametrize("prog,stdin", [("+", []), (guests.HELLO, []), (guests.FIBO, [17])],
                         ids=["one_row_cpu", "hello", "fibo17"])
def test_accepts_oracle_proofs(prog, stdin):
    pf = O.prove(prog, stdin)
    assert O.verify(prog, pf)
    host, dev = _both([pf], _vk(prog))
    assert host == [(True, -1, "")]
    assert dev == host


@pytest.mark.parametrize("nq", [1, 5])
def test_accepts_with_fewer_queries_than_a_wave(nq):
    prog = guests.HELLO
    pf = O.prove(prog, [], num_queries=nq)
    assert O.verify(prog, pf, num_queries=nq)
    try:
        sdk.set_num_queries(nq)
        host, dev = _both([pf], _vk(prog))
    finally:
        sdk.set_num_queries(0)
    assert host == [(True, -1, "")]
    assert dev == host
    # and the default query count refuses it on both paths, before any kernel
    host, dev = _both([pf], _vk(prog))
    assert host == [(False, -1, "wrong number of queries")] and dev == host


# ------------------------------------------------------------------ 2. a trace taller than Byte
def test_cpu_trace_taller_than_byte():
    """FIBO [40] runs 2^16 < cycles <= 2^18, so Byte's 2^16 rows join the main and permutation
    trees mid-path and log_max > 17.  Proved on the GPU; one bit of a Byte-height row is then
    flipped so the injected hash is what fails."""
    prog, stdin = guests.FIBO, [40]
    client = sdk.ProverClient()
    pk, vk = client.setup(prog)
    proof = client.prove(pk, stdin).run().proof
    m = BR.parse_bfz1(proof)
    logs = {BR.CHIPS[c]: o["log_degree"] for c, o in zip(m["chips"], m["opened"])}
    assert logs["Byte"] == 16 and logs["Cpu"] in (17, 18), logs
    assert len(m["commit_roots"]) + 1 == logs["Cpu"] + 1 > 17
    host, dev = _both([proof], vk)
    assert host == [(True, -1, "")] and dev == host
    byte_i = [i for i, c in enumerate(m["chips"]) if BR.CHIPS[c] == "Byte"][0]
    _bump(m["queries"][3]["inputs"][1]["rows"][byte_i], 0)
    host, dev = _both([BR.encode_bfz1(m)], vk)
    assert host == [(False, 3, INPUT_REJECTED)] and dev == host


# ------------------------------------------------------------------ 3. final value and D11
def test_final_value_and_late_reduced_opening():
    prog = "+"
    pf = O.prove(prog, [], observe_openings=False)
    m = BR.parse_bfz1(pf)
    one_row = [i for i, o in enumerate(m["opened"]) if o["log_degree"] == 0]
    assert len(one_row) == 1
    _bump(m["opened"][one_row[0]]["main_local"][0], 0)
    bad = BR.encode_bfz1(m)
    try:
        sdk.set_pcs_variant(0)  # the opened values stay out of the transcript
        host, dev = _both([pf, bad], _vk(prog))
    finally:
        sdk.set_pcs_variant(-1)
    assert host[0] == (True, -1, "")
    assert host[1] == (False, 0, FINAL_MISMATCH)
    assert dev == host


# ------------------------------------------------------------------ 4. targeted mutations
def targeted_mutations(pf, count=60, seed=7):
    """count proofs, each with one word of one query's opening bumped by 1 mod p, cycling through
    (a) an opened row, (b) an input path digest, (c) a commit-phase sibling, (d) a commit-phase
    path digest; in query 0, the last query or a random one."""
    rng = random.Random(seed)
    out = []
    nq = len(BR.parse_bfz1(pf)["queries"])
    for k in range(count):
        m = BR.parse_bfz1(pf)
        q = (0, nq - 1, rng.randrange(nq))[rng.randrange(3)]
        qp = m["queries"][q]
        kind = "abcd"[k % 4]
        if kind == "a":
            rows = qp["inputs"][rng.randrange(4)]["rows"]
            row = rows[rng.randrange(len(rows))]
            _bump(row, rng.randrange(len(row)))
        elif kind == "b":
            path = qp["inputs"][rng.randrange(4)]["path"]
            level = (0, len(path) - 1, rng.randrange(len(path)))[rng.randrange(3)]
            _bump(path[level], rng.randrange(8))
        elif kind == "c":
            _bump(qp["steps"][rng.randrange(len(qp["steps"]))]["sibling"], rng.randrange(4))
        else:
            path = qp["steps"][rng.randrange(len(qp["steps"]))]["path"]
            _bump(path[rng.randrange(len(path))], rng.randrange(8))
        out.append((kind, q, BR.encode_bfz1(m)))
    return out


def test_targeted_mutations_match_the_host(hello):
    cases = targeted_mutations(hello)
    host, dev = _both([b for _, _, b in cases], _vk(guests.HELLO))
    for (kind, q, _), h in zip(cases, host):
        # the condition of this test: the host rejects every case for the query-phase reason of
        # its kind, at the mutated query -- so the comparison below is of device verdicts
        assert h == (False, q, INPUT_REJECTED if kind in "ab" else COMMIT_REJECTED), (kind, q, h)
    assert dev == host


# ------------------------------------------------------------------ 5. the fuzz set
def fuzz_mutations(pf, count=300, seed=2024):
    """The generator of tests/test_abi.py test_verifier_fuzz_rejects_every_mutation."""
    rng = random.Random(seed)
    specials = [0, 1, 0x7F000000, 0x7F000001, 0x80000000, 0xFFFFFFFF]
    out = []
    while len(out) < count:
        b = bytearray(pf)
        kind = rng.randrange(5)
        if kind == 0:
            b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
        elif kind == 1:
            o = rng.randrange(len(b) // 4) * 4
            b[o:o + 4] = struct.pack("<I", rng.choice(specials + [rng.getrandbits(32)]))
        elif kind == 2:
            b = b[:rng.randrange(len(b))]
        elif kind == 3:
            o = rng.randrange(len(b) // 4) * 4
            b[o:o] = struct.pack("<I", rng.getrandbits(32))
        else:
            o = rng.randrange(min(len(b) // 4, 256)) * 4
            b[o:o + 4] = struct.pack("<I", rng.choice(specials + [2, 0x10000, rng.getrandbits(32)]))
        if bytes(b) == pf:
            continue
        out.append(bytes(b))
    return out


def test_fuzz_set_through_the_device(hello):
    cases = fuzz_mutations(hello)
    host, dev = _both(cases, _vk(guests.HELLO))
    assert not any(ok for ok, _, _ in host)
    in_queries = [h for h in host if h[2] in QUERY_REASONS]
    assert all(h[1] >= 0 for h in in_queries)
    assert len(in_queries) >= 80, len(in_queries)  # the kernels decided these
    assert dev == host


# ------------------------------------------------------------------ 6. a mixed batch
def test_mixed_batch_of_two_shapes():
    prog = guests.FIBO
    a, b = O.prove(prog, [3]), O.prove(prog, [17])
    shape = lambda pf: [o["log_degree"] for o in BR.parse_bfz1(pf)["opened"]]  # noqa: E731
    assert shape(a) != shape(b)
    rng = random.Random(11)
    batch = []
    for k in range(16):
        pf = (a, b)[k % 2]
        if k % 4 >= 2:  # valid, valid, tampered, tampered, ...
            pf = targeted_mutations(pf, count=4, seed=rng.randrange(1 << 30))[k % 4][2]
        batch.append(pf)
    batch[9] = batch[9][: len(batch[9]) // 2]  # and one truncated
    host, dev = _both(batch, _vk(prog))
    assert [h[0] for h in host] == [k % 4 < 2 and k != 9 for k in range(16)]
    assert host[9][:2] == (False, -1)  # a decode error, before any kernel
    assert dev == host


def test_misshapen_query_splits_the_work(hello):
    cases = misshapen_cases(hello)
    host, dev = _both([b for b, _ in cases], _vk(guests.HELLO))
    assert host == [want for _, want in cases]
    assert dev == host


def test_proof_the_packing_refuses_is_rejected_alone(hello):
    """Preprocessed chips that claim other log degrees than their key's give a proof more LDE
    heights than a descriptor holds.  The call still succeeds, that proof gets the host's reason
    (its queries run on the host) and its neighbours are verified on the device as usual."""
    bad = targeted_mutations(hello, count=1)[0][2]
    host, dev = _both([hello, claimed_heights_mutation(hello), bad, hello], _vk(guests.HELLO))
    assert [h[0] for h in host] == [True, False, False, True]
    assert host[1][:2] == (False, 0) and host[2][2] == INPUT_REJECTED
    assert dev == host


def test_verify_on_device_raises_like_the_host(hello):
    c = sdk.ProverClient()
    vk = _vk(guests.HELLO)
    c.verify(sdk.BfProofWithPublicValues(proof=hello, stdin=b""), vk, on_device=True)
    bad = targeted_mutations(hello, count=1)[0][2]
    with pytest.raises(sdk.BfzError, match="verification failed: " + INPUT_REJECTED):
        c.verify(sdk.BfProofWithPublicValues(proof=bad, stdin=b""), vk, on_device=True)
