"""Per-key lookup discrepancies on the device (bfz_record_debug_interactions and
bfz_debug_interactions_traces with on_device = 1): the aggregation kernels of
csrc/lookup_debug.hip against the host path (the same Lookup tables over a std::map, checked
against the independent model in tests/test_debug_interactions.py), the record path, the
constraint checker's kind table, the multi-round path and a proof after a debug run."""
import pytest

import lookup_cases as C
import oracle_lib as O
from bfz import _lib, guests, sdk

pytestmark = pytest.mark.gpu
P = O.P
K_MEMORY, K_BYTE = 1, 7


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.init(0)
    yield


@pytest.fixture(scope="module")
def client():
    return sdk.ProverClient()


@pytest.fixture(scope="module")
def keys(client):
    return {name: client.setup(prog)[0] for name, (prog, _) in C.PROGS.items()}


def both(pk, traces, kinds=None, limit=256, all_records=False):
    run = C.run_all if all_records else (lambda *a, **k: C.run(*a, limit=limit, **k))
    host = run(pk, traces, kinds, on_device=False)
    dev = run(pk, traces, kinds, on_device=True)
    C.same_reports(dev, host)
    assert dev.rounds >= 1 and dev.table_bytes > 0 and host.table_bytes == 0
    return dev


def test_shapes_cover_one_row_part_of_a_block_and_many_blocks():
    """The heights the cases below run at: 1 (`+`), a Cpu trace shorter than one 256-thread block
    (loop: 32 rows), two blocks (hello: 512 rows), 2^16 (fibo17's Cpu trace and Byte)."""
    h = {name: {c: t[0].shape[0] for c, t in C.canonical_traces(name).items()} for name in C.PROGS}
    assert h["plus"][0] == 1
    assert h["loop"][0] < 256 < h["hello"][0]
    assert h["fibo17"][0] > 256 and h["fibo17"][5] == 1 << 16
    assert {x for v in h.values() for x in v.values()} >= {1, 16, 32, 64, 512, 1 << 16}


@pytest.mark.parametrize("name", ["hello", "loop", "fibo17", "plus"])
def test_device_equals_host_on_clean_traces(keys, name):
    rep = both(keys[name], C.canonical_traces(name))
    assert rep.balanced and rep.discrepancies == [] and rep.total_net == 0
    assert (rep.rounds, rep.tag_collisions) == (1, 0)


def test_device_equals_host_on_the_corruptions(keys):
    traces, value, _ = C.byte_case()
    rep = both(keys["hello"], traces)
    assert [(d.kind, d.values, d.net) for d in rep.discrepancies] == [(K_BYTE, [0, value, 0], -1)]
    traces, row = C.alu_key_case()
    rep = both(keys["fibo17"], traces)
    assert sorted(d.net for d in rep.discrepancies) == [-1, 1] and rep.total_net == 0
    assert (2, row) in [(d.first_chip, d.first_row) for d in rep.discrepancies]


@pytest.mark.parametrize("name", ["hello", "loop", "plus"])
def test_device_equals_host_on_random_mains(keys, name):
    """Every unbalanced key (cap = their number), then the truncation to 3."""
    traces = C.random_case(name)
    rep = both(keys[name], traces, all_records=True)
    assert len(rep.discrepancies) == rep.unbalanced_keys > rep.distinct_keys // 2
    cut = both(keys[name], traces, limit=3)
    assert cut.discrepancies == rep.discrepancies[:3] and cut.unbalanced_keys == rep.unbalanced_keys


def test_device_equals_host_on_a_tall_random_main(keys):
    """fibo17's shapes (2^16 Cpu rows, 16 interactions each): counters and the first records."""
    rep = both(keys["fibo17"], C.random_case("fibo17"), limit=64)
    assert len(rep.discrepancies) == 64 and rep.interactions > 1 << 20


@pytest.mark.parametrize("kind", [K_BYTE, K_MEMORY])
def test_device_equals_host_with_a_kind_filter(keys, kind):
    for traces in (C.canonical_traces("hello"), C.random_case("hello")):
        rep = both(keys["hello"], traces, kinds=[kind], all_records=True)
        assert all(d.kind == kind for d in rep.discrepancies)


@pytest.mark.parametrize("name,prog,stdin", guests.REFERENCE_PROGRAMS + [("fibo17", guests.FIBO, [17])])
def test_clean_records_balance_and_equal_the_host_trace_path(client, name, prog, stdin):
    pk, _ = client.setup(prog)
    rep = client.debug_interactions(pk, stdin)
    assert rep.balanced and rep.discrepancies == [] and rep.total_net == 0, str(rep)
    host = sdk.CoreProver().debug_interactions(pk, sdk.generate_traces(prog, stdin), on_device=False)
    C.same_reports(rep, host)


def test_invalid_execution_device_equals_host(client):
    """`<+`: no claim about its balance, only that both paths say the same."""
    pk, _ = client.setup("<+")
    rep = client.debug_interactions(pk, [])
    host = sdk.CoreProver().debug_interactions(pk, sdk.generate_traces("<+", []), on_device=False)
    C.same_reports(rep, host)


@pytest.mark.parametrize("prog,stdin", [(guests.HELLO, []), (guests.FIBO, [17])])
def test_counters_agree_with_the_constraint_checkers_kind_table(client, prog, stdin):
    pk, _ = client.setup(prog)
    rep = client.debug_interactions(pk, stdin)
    table = client.debug_constraints(pk, stdin, flags=sdk.DEBUG_BALANCE)
    assert table.balance_valid
    assert rep.interactions == sum(sum(row) for row in table.kind_count)
    assert (rep.total_net - sum(sum(row) for row in table.kind_net)) % P == 0
    for kind in range(1, 8):  # and kind by kind
        one = client.debug_interactions(pk, stdin, kinds=[kind])
        assert one.interactions == sum(table.kind_count[kind])


def test_unbalanced_traces_agree_with_the_kind_table(keys):
    traces, _, _ = C.byte_case()
    rep = C.run(keys["hello"], traces, on_device=True)
    table = sdk.CoreProver().debug_constraints(keys["hello"], C.lib_traces(traces), flags=sdk.DEBUG_BALANCE)
    assert rep.interactions == sum(sum(row) for row in table.kind_count)
    assert (rep.total_net - sum(sum(row) for row in table.kind_net)) % P == 0 and rep.total_net == -1


@pytest.mark.parametrize("case", ["hello", "random_hello"])
def test_multi_round_path_gives_the_same_report(keys, case):
    """Fault bit 2 cuts the key hash to 12 bits: distinct keys share tags, the rounds repeat, and
    verdicts, counters and records stay what they were."""
    traces = C.canonical_traces("hello") if case == "hello" else C.random_case("hello")
    plain = C.run_all(keys["hello"], traces, on_device=True)
    assert (plain.rounds, plain.tag_collisions) == (1, 0)
    try:
        _lib.check(_lib.lib().bfz_set_fault_injection(4))
        cut = C.run_all(keys["hello"], traces, on_device=True)
    finally:
        _lib.check(_lib.lib().bfz_set_fault_injection(0))
    assert cut.tag_collisions > 0 and cut.rounds >= 2
    C.same_reports(cut, plain)


def test_bad_arguments_are_errors_on_the_device_path(keys):
    traces = C.lib_traces(C.canonical_traces("loop"))
    with pytest.raises(_lib.BfzError, match="Cpu chip is required"):
        sdk.CoreProver().debug_interactions(keys["loop"], [t for t in traces if t[0] != 0])
    short = [(c, n, t[: t.shape[0] // 2] if c == 5 else t) for c, n, t in traces]
    with pytest.raises(_lib.BfzError, match="preprocessed"):
        sdk.CoreProver().debug_interactions(keys["loop"], short)
    with pytest.raises(_lib.BfzError, match="LookupKind"):
        sdk.CoreProver().debug_interactions(keys["loop"], traces, kinds=[8])
    with pytest.raises(_lib.BfzError, match="bfz_setup_host"):
        sdk.CoreProver().debug_interactions(C.host_key("loop"), traces)


def test_no_state_leaks_into_proofs(client):
    prog = guests.HELLO
    pk, _ = client.setup(prog)
    assert client.debug_interactions(pk, []).balanced
    traces, _, _ = C.byte_case()
    assert not C.run(pk, traces, on_device=True).balanced
    assert client.prove(pk, []).run().proof == O.prove(prog, [])
