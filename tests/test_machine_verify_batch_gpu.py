"""GPU tests of bfz_machine_verify_batch with on_device = 1: the query phase of machine proofs on
the device (csrc/verify_machine.hip) against the host verifier, Machine.verify.  Every comparison
is exact: (ok, query, why) and the ending challenger's bytes."""
import numpy as np
import pytest

import bincode_ref as BR
import chip_cases as C
import machine_cases as M
from bfz import guests, sdk

pytestmark = pytest.mark.gpu
QUERIES = 6
ELEVEN = (1, 2, 4, 8, 32, 64, 128, 256, 512, 1024)  # ten senders and the 16-row table


def _prove(m, traces, nq=QUERIES):
    sdk.set_num_queries(nq)
    try:
        return m.prove(traces, m.observe())
    finally:
        sdk.set_num_queries(0)


def _both(m, proofs, nq=QUERIES):
    """[((ok, query, why), challenger bytes)] of Machine.verify and of the device batch."""
    sdk.set_num_queries(nq)
    try:
        host = []
        for pf in proofs:
            ch = m.observe()
            o = m.verify(pf, ch)
            host.append(((o.ok, o.query, o.why), bytes(ch)))
        chs = [m.observe() for _ in proofs]
        out = m.verify_batch(proofs, chs, on_device=True)
        return host, [((o.ok, o.query, o.why), bytes(c)) for o, c in zip(out, chs)]
    finally:
        sdk.set_num_queries(0)


def test_builtin_parity():
    m = M.builtin_machine(guests.HELLO)
    proof = _prove(m, {name: main for _, name, main, _ in M.guest_traces(guests.HELLO)})
    host, dev = _both(m, [proof])
    assert dev == host and dev[0][0] == (True, -1, "")
    client = sdk.ProverClient()
    _, vk = client.setup(guests.HELLO)
    sdk.set_num_queries(QUERIES)
    try:
        o = client.verify_batch([proof], vk, on_device=True)[0]
    finally:
        sdk.set_num_queries(0)
    assert (o.ok, o.query, o.why) == dev[0][0]


@pytest.mark.parametrize("nq", [1, 70, 130])
def test_beyond_the_old_descriptors(nq):
    """11 chips, 11 LDE heights, 45 opened matrices, three rounds of 11 height groups; the 1-row
    sender's reduced opening joins after the last fold.  nq: fewer queries than a wave, more than
    one wave's turn per block, more than one pass of 128 queries through k_mverify_reduce."""
    m, traces = M.custom_machine(ELEVEN)
    host, dev = _both(m, [_prove(m, traces, nq)], nq)
    assert dev == host and dev[0][0] == (True, -1, "")


@pytest.mark.parametrize("nchips,nq", [(3, QUERIES), (8, QUERIES), (8, 130)])
def test_widest_rows(nchips, nq):
    """Main rows of 64 words and permutation rows of 68 (32 interactions: 16 batches and the sum),
    all chips in one height group.  Every interaction's multiplicity is column 0, which is zero.
    Eight chips are 1120 columns at one height: two coefficient tiles in k_mverify_reduce, and with
    130 queries the tiles are staged again for a second pass of queries."""
    b = sdk.LookupBuilder(64)
    for i in range(16):
        b.send(3, [b.main(1 + i)], b.main(0))
        b.receive(3, [b.main(17 + i)], b.main(0))
    lk = b.program()
    rows = np.arange(4 * 64, dtype=np.uint64).reshape(4, 64) * 7919 % C.P
    rows[:, 0] = 0
    names = [f"w{i}" for i in range(nchips)]
    m = sdk.Machine([(name, None, lk, None) for name in names])
    host, dev = _both(m, [_prove(m, {name: C.mont(rows) for name in names}, nq)], nq)
    assert dev == host and dev[0][0] == (True, -1, "")


@pytest.fixture(scope="module")
def eleven():
    m, traces = M.custom_machine(ELEVEN)
    return m, _prove(m, traces)


def _bump(words, i=0):
    words[i] = (words[i] + 1) % BR.P


MUTATIONS = [f"round{r}-{part}" for r in range(4) for part in ("tallest-row", "shortest-row", "path")]
MUTATIONS += ["first-sibling", "last-sibling", "step-path", "final-poly"]


def _mutate(model, which):
    """One word of the middle query (or the final polynomial) plus 1 mod p."""
    q = model["queries"][QUERIES // 2]
    if which == "final-poly":
        return _bump(model["final_poly"])
    if which == "first-sibling":
        return _bump(q["steps"][0]["sibling"])
    if which == "last-sibling":
        return _bump(q["steps"][-1]["sibling"], 2)
    if which == "step-path":
        return _bump(q["steps"][1]["path"][0], 5)
    opening = q["inputs"][int(which[5])]
    if which.endswith("path"):
        return _bump(opening["path"][len(opening["path"]) // 2], 3)
    logs = [o["log_degree"] for o in model["opened"]]
    chip = logs.index(max(logs) if "tallest" in which else min(logs))
    # every chip has the same number of matrices in a round (two quotient chunks each), so chip i's
    # first is i * per_chip; 0 in the preprocessed round: its one matrix
    per_chip = len(opening["rows"]) // len(logs)
    _bump(opening["rows"][chip * per_chip])


@pytest.mark.parametrize("which", MUTATIONS)
def test_mutations_name_what_the_host_names(eleven, which, monkeypatch):
    m, proof = eleven
    monkeypatch.setattr(BR, "CHIPS", tuple(n.decode() for n in m.names))
    model = BR.parse_bfz1(proof)
    _mutate(model, which)
    host, dev = _both(m, [proof, BR.encode_bfz1(model), proof])
    assert dev == host
    assert [d[0][0] for d in dev] == [True, False, True]


def test_misshapen_query_stays_on_the_host(eleven, monkeypatch):
    """Query 2 of 6 has a row one word short: queries 0 and 1 go to the device, the rest stay."""
    m, proof = eleven
    monkeypatch.setattr(BR, "CHIPS", tuple(n.decode() for n in m.names))
    model = BR.parse_bfz1(proof)
    model["queries"][2]["inputs"][1]["rows"][0].pop()
    host, dev = _both(m, [BR.encode_bfz1(model)])
    assert dev == host and dev[0][0][:2] == (False, 2)
