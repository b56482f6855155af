"""bfz_machine_check on the device: k_check_machine against the host path, across a segment
boundary, against the built-in machine's debug_constraints, and beyond the prover's height limit."""
import numpy as np
import pytest

import air_program_cases as A
import chip_cases as C
import machine_cases as M
import machine_check_cases as K
from bfz import guests, sdk

pytestmark = pytest.mark.gpu


def _both(m, traces):
    dev = m.check(traces, on_device=True, profile=True)
    K.same_report(dev, m.check(traces, on_device=False, profile=True))
    return dev


@pytest.mark.parametrize("flip", [None] + K.FLIPS, ids=["valid"] + K.FLIP_IDS)
def test_device_equals_host(flip):
    m, traces = M.custom_machine(K.HEIGHTS)
    rep = _both(m, K.flipped(traces, *flip) if flip else traces)
    assert rep.ok == (flip is None)


def test_segment_boundary():
    """Segments in layout order: m512 (two full blocks), then m256 from the next block.  A failure
    in the last row of m512 (the last thread of its last block) and one in row 0 of m256 (the
    first thread of its block) must each be credited to its own chip."""
    m, traces = M.custom_machine((256, 512))
    bad = K.flipped(K.flipped(traces, "m512", 511, 3, 2), "m256", 0, 2, 1)
    rep = _both(m, bad)
    got = {n: (c.failing_rows, c.first_row, c.first_constraint) for n, c in zip(rep.names, rep.chips)}
    # m512: s (s - 1) with s = 2; m256: c + 1 breaks the gate and the next row's a = c
    assert got == {"m512": (1, 511, 0), "m256": (1, 0, 1), "table": (0, -1, -1)}
    assert [int(x) for x in rep.counts[rep.names.index("m256")][:3]] == [0, 1, 1]


@pytest.mark.parametrize("broken", [False, True], ids=["valid", "cpu-flip"])
def test_builtin_yardstick(broken):
    guest = M.guest_traces(guests.HELLO)
    traces = {name: main for _, name, main, _ in guest}
    if broken:
        traces["Cpu"] = C.flip(traces["Cpu"], len(traces["Cpu"]) // 2, 0)
    m = M.builtin_machine(guests.HELLO)
    pk, _ = sdk.ProverClient().setup(guests.HELLO)
    ch = m.observe()
    want = sdk.CoreProver().debug_constraints(pk, [(c, name, traces[name]) for c, name, _, _ in guest],
                                              ch=sdk.Challenger.from_buffer_copy(ch))
    rep = m.check(traces, ch)
    assert (rep.ok, rep.alpha, rep.beta, rep.cumulative_sum) == (
        want.ok, want.alpha, want.beta, want.cumulative_sum) and rep.ok != broken
    by_chip = {c.chip: c for c in want.chips}
    for c in rep.chips:  # creation order is the built-in order: chip is the built-in id
        w = by_chip[c.chip]
        assert (c.num_constraints, c.num_batches, c.height, c.failing_rows, c.first_row,
                c.first_constraint, c.cumulative_sum) == (
            w.num_constraints, w.num_batches, w.height, w.failing_rows, w.first_row,
            w.first_constraint, w.cumulative_sum)


def test_no_same_height_limit():
    """Nine senders of 4 rows: the prover refuses them, the check (no tree) does not."""
    air, lk, tlk = A.mulgate_program(), M.sender_program(), M.table_lookups()
    sender = C.mont(np.array(M.sender_rows(4), dtype=np.uint64))
    keys = sorted({(int(a), int(b)) for a, b, _, s in M.sender_rows(4) if s})
    keys += [(k, 0) for k in range(2, 18)][:16 - len(keys)]
    prep = C.mont(np.array([[a] for a, _ in keys], dtype=np.uint64))
    main = C.mont(np.array([[0, b] for _, b in keys], dtype=np.uint64))
    main[:, 0] = sdk.lookups_multiplicities(tlk, main, prep, 0, [lk] * 9, [sender] * 9, [None] * 9).mult
    m = sdk.Machine([(f"s{i}", air, lk, None) for i in range(9)] + [("table", None, tlk, prep)])
    traces = dict({f"s{i}": sender for i in range(9)}, table=main)
    with pytest.raises(sdk.BfzError, match="9 chips of height 4"):
        m.prove(traces, m.observe())
    assert _both(m, traces).ok
