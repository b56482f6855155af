"""Per-key lookup discrepancies, host path (bfz_debug_interactions_traces, on_device = 0): the
reference's debug_interactions_with_all_chips (crates/stark/src/lookup/debug.rs:59-196) on oracle
traces against the independent model of tests/lookup_model.py.  No device needed: the key is a
bfz_setup_host key."""
import numpy as np
import pytest

import debug_cases as D
import lookup_cases as C
import lookup_model as M
from bfz import sdk

K_MEMORY, K_ALU, K_BYTE = 1, 3, 7


@pytest.mark.parametrize("name", ["hello", "loop", "fibo17", "plus"])
def test_clean_traces_balance(name):
    traces = C.canonical_traces(name)
    rep = C.run(C.host_key(name), traces)
    want = C.model(name, traces)
    assert rep.balanced and rep.discrepancies == [] and rep.total_net == 0
    assert want["balanced"] and rep.interactions > 0
    C.assert_matches_model(rep, want)
    assert (rep.rounds, rep.tag_collisions, rep.table_bytes) == (0, 0, 0)  # host path
    text = str(rep)
    assert "All chips have the same number of sends and receives." in text
    assert f"Cpu chip has {want['chip_distinct'][0]} distinct events" in text


def test_one_byte_receive_too_many():
    traces, value, clean_mult = C.byte_case()
    rep = C.run(C.host_key("hello"), traces)
    want = C.model("byte_case", traces)
    C.assert_matches_model(rep, want)
    assert not rep.balanced and rep.unbalanced_keys == 1 and rep.total_net == -1
    d = rep.discrepancies[0]
    assert (d.kind, d.values, d.net) == (K_BYTE, [0, value, 0], -1)
    assert d.chip_net[5] == -clean_mult - 1           # one less than the clean net in Byte
    assert sum(d.chip_net) - d.chip_net[5] == clean_mult  # the senders are unchanged
    assert d.chip_count[5] == 1
    text = str(rep)
    assert f"Lookup key: Byte (0, {value}, 0) Send-Receive Discrepancy: -1" in text
    assert f" Byte chip's send-receive discrepancy for this key is {-clean_mult - 1}" in text
    assert "Total send-receive discrepancy: -1" in text
    assert "you're receiving more than you are sending" in text
    assert f"first seen at {sdk.CHIPS[d.first_chip]} row {d.first_row} interaction {d.first_interaction}" in text


def test_keys_wrong_totals_right():
    traces, row = C.alu_key_case()
    rep = C.run(C.host_key("fibo17"), traces)
    want = C.model("alu_key_case", traces)
    C.assert_matches_model(rep, want)
    assert not rep.balanced and rep.total_net == 0
    assert sorted(d.net for d in rep.discrepancies) == [-1, 1]
    assert all(d.kind == K_ALU for d in rep.discrepancies)
    recv = next(d for d in rep.discrepancies if d.net == -1)
    assert (recv.first_chip, recv.first_row) == (2, row)  # the AddSub row that was changed
    assert "the total number of sends and receives match, but the keys don't match" in str(rep)


@pytest.mark.parametrize("name", ["hello", "loop", "plus"])
def test_random_main_equals_model_record_for_record(name):
    """Nearly every interaction is unbalanced and the multiplicities are arbitrary field elements:
    field_to_int on both sides of p / 2, and the record order."""
    traces = C.random_case(name)
    want = C.model(("random", name), traces)
    rep = C.run_all(C.host_key(name), traces)
    assert want["unbalanced_keys"] > want["distinct_keys"] // 2
    C.assert_matches_model(rep, want)
    nets = [d.net for d in rep.discrepancies]
    if len(nets) > 100:
        assert min(nets) < -(M.P // 4) and max(nets) > M.P // 4
    keys = [(d.kind, d.values) for d in rep.discrepancies]
    assert keys == sorted(keys)


def test_truncation_keeps_the_first_records():
    traces = C.random_case("hello")
    want = C.model(("random", "hello"), traces)
    rep = C.run(C.host_key("hello"), traces, limit=3)
    assert len(rep.discrepancies) == 3
    C.assert_matches_model(rep, want, n=3)
    assert "more unbalanced keys" in str(rep)


@pytest.mark.parametrize("kind", [K_BYTE, K_MEMORY])
def test_kind_filter(kind):
    for key, traces in (("hello", C.canonical_traces("hello")),
                        (("random", "hello"), C.random_case("hello"))):
        want = C.model(key, traces, kinds=(kind,))
        rep = C.run_all(C.host_key("hello"), traces, kinds=[kind])
        C.assert_matches_model(rep, want)
        assert all(d.kind == kind for d in rep.discrepancies)
        assert 0 < rep.interactions < C.model(key, traces)["interactions"]
    assert sdk.kinds_mask(["Byte"]) == 1 << K_BYTE and sdk.kinds_mask() == 0xFE


def test_bad_arguments_are_errors():
    import ctypes
    from bfz import _lib
    pk = C.host_key("loop")
    traces = C.lib_traces(C.canonical_traces("loop"))

    def call(mask):
        _, chips, ptrs, hs, ws, k = keep = sdk._trace_args(traces)
        rep = _lib.LookupReportC()
        rc = _lib.lib().bfz_debug_interactions_traces(ctypes.c_void_p(pk.handle), chips, ptrs, hs, ws,
                                                     k, mask, 0, ctypes.byref(rep), None, 0)
        del keep
        return rc, _lib.lib().bfz_last_error().decode()

    assert call(0xFE)[0] == 0
    rc, msg = call(0)
    assert rc < 0 and "no LookupKind" in msg
    rc, msg = call(1 << 8)
    assert rc < 0 and "outside LookupKind 1..7" in msg
    assert call(1)[0] < 0  # bit 0 is no kind either
    # cap > 0 without an output array
    _, chips, ptrs, hs, ws, k = keep = sdk._trace_args(traces)
    rep = _lib.LookupReportC()
    assert _lib.lib().bfz_debug_interactions_traces(ctypes.c_void_p(pk.handle), chips, ptrs, hs, ws, k,
                                                    0xFE, 0, ctypes.byref(rep), None, 4) < 0
    del keep
    # the errors of bfz_debug_constraints_traces (tests/test_debug_constraints_gpu.py)
    with pytest.raises(sdk.BfzError, match="Cpu chip is required"):
        sdk.CoreProver().debug_interactions(pk, [t for t in traces if t[0] != 0], on_device=False)
    short = [(c, n, t[: t.shape[0] // 2] if c == 5 else t) for c, n, t in traces]
    with pytest.raises(sdk.BfzError, match="preprocessed"):
        sdk.CoreProver().debug_interactions(pk, short, on_device=False)
    bad = [(c, n, t.copy()) for c, n, t in traces]
    bad[0][2][0, 0] = M.P  # not a field word
    with pytest.raises(sdk.BfzError, match="non-canonical"):
        sdk.CoreProver().debug_interactions(pk, bad, on_device=False)


def test_host_key_is_refused_where_the_device_key_is_needed():
    pk = C.host_key("loop")
    with pytest.raises(sdk.BfzError, match="bfz_setup_host"):
        sdk.CoreProver().observe_into(pk, sdk.CoreProver.new_challenger())


def test_model_tables_cover_every_chip():
    """The model's interaction count per chip is the one the LogUp batches are sized by
    (debug_cases.N_LOOKUPS), and its traces have the chips' widths."""
    for c in range(8):
        prep = np.zeros((1, len(M.PREP_COLS[c])), dtype=np.uint32) if c in M.PREP_COLS else None
        assert len(M.interactions(c, np.zeros((1, M.WIDTHS[c]), dtype=np.uint32), prep)) == D.N_LOOKUPS[c]
