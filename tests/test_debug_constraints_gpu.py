"""The constraint checker on the device: k_check against the host path (same templates on the
CPU, tests/test_debug_constraints.py), and StarkMachine::debug_constraints
(crates/stark/src/machine.rs:288-387) on device records and host traces -- clean programs pass,
`<+` names its failing chip, an unbalanced Byte multiplicity shows in the balance table."""
import numpy as np
import pytest

import debug_cases as D
import oracle_lib as O
from bfz import _lib, guests, sdk

pytestmark = pytest.mark.gpu
P = O.P
K_BYTE = 7


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.init(0)
    yield


@pytest.fixture(scope="module")
def client():
    return sdk.ProverClient()


def same(dev, host):
    for f in ("chip", "height", "num_constraints", "num_batches", "failing_rows", "first_row",
              "first_constraint", "cumulative_sum"):
        assert getattr(dev, f) == getattr(host, f), (f, str(dev), str(host))
    assert (dev.first_fail_per_row == host.first_fail_per_row).all()


def both(chip, main, prep, perm, alpha, beta, cs):
    host = D.check(chip, main, prep, perm, alpha, beta, cs)
    dev = D.check(chip, main, prep, perm, alpha, beta, cs, on_device=True)
    same(dev, host)
    return host


@pytest.mark.parametrize("name,prog,stdin", [p for p in D.PROGRAMS if p[0] != "loop"],
                         ids=["hello", "fibo17", "plus"])
def test_device_equals_host_on_clean_and_random_traces(name, prog, stdin):
    """Every included chip (heights 1, 2, ... 2^16): the clean trace, and a uniformly random main
    of the same shape with its own permutation trace (nearly every row fails, at many indices)."""
    alpha, beta = D.challenges(23)
    rng = np.random.default_rng(29)
    heights = set()
    for chip in D.included(prog, stdin):
        main, prep = D.traces(prog, stdin, chip)
        heights.add(main.shape[0])
        perm, cs = D.perm(chip, main, prep, alpha, beta)
        assert both(chip, main, prep, perm, alpha, beta, cs).failing_rows == 0
        rnd = rng.integers(0, P, main.shape).astype(np.uint32)
        perm, cs = D.perm(chip, rnd, prep, alpha, beta)
        res = both(chip, rnd, prep, perm, alpha, beta, cs)
        if main.shape[0] >= 64 and chip not in (1, 4, 5):  # chips with AIR constraints
            assert res.failing_rows > main.shape[0] // 2
    assert (1 << 16) in heights
    if name == "plus":
        assert 1 in heights


CASES = D.corruption_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_device_equals_host_on_corruptions(case):
    """The CPU file's cases (a corruption in row 0 and one in the last row of a trace taller than
    256 rows among them: chip0_phi_first / chip0_phi_last), and what each must report."""
    name, chip, main, prep, perm, alpha, beta, cs, expect = case
    expect(both(chip, main, prep, perm, alpha, beta, cs))
    expect(D.check(chip, main, prep, perm, alpha, beta, cs, on_device=True))


def ef_sum(xs):
    return [sum(x[e] for x in xs) % P for e in range(4)]


def canon(words):
    return [O.from_mont(x) for x in words]


def check_clean_report(rep, prog, stdin):
    assert rep.ok, str(rep)
    ch = O.challenger([], 8)
    alpha, beta = ch[:4], ch[4:]
    assert canon(rep.alpha) == alpha and canon(rep.beta) == beta
    chips = D.included(prog, stdin)
    assert [c.chip for c in rep.chips] == chips
    for c in rep.chips:
        main, prep = D.traces(prog, stdin, c.chip)
        _, cs = D.perm(c.chip, main, prep, alpha, beta)
        assert canon(c.cumulative_sum) == cs, sdk.CHIPS[c.chip]
        assert c.failing_rows == 0 and c.height == main.shape[0]
    assert canon(rep.cumulative_sum) == [0, 0, 0, 0]
    assert ef_sum([canon(c.cumulative_sum) for c in rep.chips]) == [0, 0, 0, 0]
    assert rep.balance_valid
    for k in range(1, 8):  # every kind balances over the chips
        assert ef_sum([canon(rep.kind_sum[k][c]) for c in chips]) == [0, 0, 0, 0], sdk.KINDS[k]
        assert sum(rep.kind_net[k][c] for c in chips) == 0, sdk.KINDS[k]
    for c in rep.chips:    # a chip's sum over kinds is its cumulative sum
        assert ef_sum([canon(rep.kind_sum[k][c.chip]) for k in range(1, 8)]) == canon(c.cumulative_sum)


@pytest.mark.parametrize("name,prog,stdin", guests.REFERENCE_PROGRAMS + [("fibo17", guests.FIBO, [17])])
def test_clean_records_pass(client, name, prog, stdin):
    pk, _ = client.setup(prog)
    rep = client.debug_constraints(pk, stdin, flags=sdk.DEBUG_BALANCE)
    check_clean_report(rep, prog, tuple(stdin))
    plain = client.debug_constraints(pk, stdin)  # without the flag: no table for a zero sum
    assert plain.ok and not plain.balance_valid
    assert plain.chips == rep.chips


def test_challenger_is_advanced_by_two_extension_samples(client):
    pk, _ = client.setup(guests.LOOP)
    ch = sdk.CoreProver.new_challenger()
    rep = client.debug_constraints(pk, [], ch=ch)
    words = O.challenger([], 9)
    assert canon(rep.alpha) + canon(rep.beta) == words[:8]
    assert ch.n_output == 0  # the 8 outputs of the first duplexing are used up
    rep2 = client.debug_constraints(pk, [], ch=ch)  # the next samples differ: new challenges
    assert canon(rep2.alpha) + canon(rep2.beta) == O.challenger([], 16)[8:]
    assert rep2.ok


def test_invalid_execution_names_the_failing_chip(client):
    """`<+` (tests/test_gpu.py test_invalid_trace_rejected_by_verifiers): the memory pointer
    wraps below zero, which breaks MemoryInstrs' word range check."""
    pk, _ = client.setup("<+")
    rep = client.debug_constraints(pk, [])
    text = str(rep)
    assert not rep.ok, text
    failing = {c.chip: c for c in rep.failing()}
    assert 6 in failing, text  # MemoryInstrs
    mi = failing[6]
    assert 0 <= mi.first_row < mi.height and 0 <= mi.first_constraint < mi.num_constraints
    assert f"chip MemoryInstrs, row {mi.first_row}, constraint {mi.first_constraint} of " \
           f"{mi.num_constraints}" in text, text


def test_unbalanced_byte_lookup_shows_in_the_balance_table(client):
    prog = guests.HELLO
    pk, _ = client.setup(prog)
    traces = sdk.generate_traces(prog, [])
    clean = sdk.CoreProver().debug_constraints(pk, traces, flags=sdk.DEBUG_BALANCE)
    assert clean.ok and clean.balance_valid
    bad = [(c, n, t.copy()) for c, n, t in traces]
    byte = next(t for c, _, t in bad if c == 5)
    row = int(np.nonzero(byte[:, 0])[0][0])  # a byte that is looked up: one more receive
    byte[row, 0] = O.to_mont(O.from_mont(int(byte[row, 0])) + 1)
    rep = sdk.CoreProver().debug_constraints(pk, bad)
    text = str(rep)
    assert not rep.ok, text
    assert all(c.failing_rows == 0 for c in rep.chips), text  # every row check passes
    assert any(rep.cumulative_sum) and rep.balance_valid
    chips = [c.chip for c in rep.chips]
    for k in range(1, 8):
        total = ef_sum([canon(rep.kind_sum[k][c]) for c in chips])
        assert (total != [0, 0, 0, 0]) == (k == K_BYTE), (sdk.KINDS[k], text)
    assert sum(rep.kind_net[K_BYTE][c] for c in chips) == -1  # one more received than sent
    for k in range(1, 8):
        for c in chips:
            differs = (rep.kind_sum[k][c] != clean.kind_sum[k][c]
                       or rep.kind_net[k][c] != clean.kind_net[k][c])
            assert differs == (k == K_BYTE and c == 5), (sdk.KINDS[k], sdk.CHIPS[c])
    assert rep.kind_net[K_BYTE][5] == clean.kind_net[K_BYTE][5] - 1
    assert "Byte" in text and "NOT zero" in text and " *" in text


@pytest.mark.parametrize("prog,stdin", [(guests.HELLO, []), (guests.FIBO, [17]), ("+", []), ("<+", [])])
def test_record_and_host_trace_paths_agree(client, prog, stdin):
    pk, _ = client.setup(prog)
    a = client.debug_constraints(pk, stdin, flags=sdk.DEBUG_BALANCE)
    b = sdk.CoreProver().debug_constraints(pk, sdk.generate_traces(prog, stdin),
                                           flags=sdk.DEBUG_BALANCE)
    assert a == b


def test_bad_host_traces_are_errors(client):
    pk, _ = client.setup(guests.LOOP)
    traces = sdk.generate_traces(guests.LOOP, [])
    with pytest.raises(_lib.BfzError, match="Cpu chip is required"):
        sdk.CoreProver().debug_constraints(pk, [t for t in traces if t[0] != 0])
    short = [(c, n, t[: t.shape[0] // 2] if c == 5 else t) for c, n, t in traces]
    with pytest.raises(_lib.BfzError, match="preprocessed"):
        sdk.CoreProver().debug_constraints(pk, short)


def test_no_state_leaks_into_proofs(client):
    prog = guests.HELLO
    pk, _ = client.setup(prog)
    assert client.debug_constraints(pk, [], flags=sdk.DEBUG_BALANCE).ok
    assert client.prove(pk, []).run().proof == O.prove(prog, [])
