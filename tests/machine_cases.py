"""Shared by tests/test_machine.py and tests/test_machine_gpu.py: the built-in chips as a Machine
of exported programs and a custom machine of mulgate senders and a lookup-only table."""
import functools

import numpy as np

import chip_cases as C
import oracle_lib as O
from bfz import sdk

P = C.P


@functools.lru_cache(maxsize=None)
def guest_traces(prog, stdin=()):
    """[(chip, name, main, prep or None)] of the chips the guest includes, Montgomery words."""
    out = []
    for c, name in enumerate(sdk.CHIPS):
        m = O.trace(prog, list(stdin), c, False)
        if m is None:
            continue
        pr = O.trace(prog, list(stdin), c, True) if C.exported(c)[2].prep_width else None
        out.append((c, name, C.mont(m), None if pr is None else C.mont(pr)))
    return out


def builtin_machine(prog, stdin=(), verifier_only=False):
    """All eight exported chips in the built-in order (a proof's chip words are then the built-in
    chip ids), the guest's preprocessed traces -- or only their heights and the oracle's root."""
    prep = {c: pr for c, _, _, pr in guest_traces(prog, stdin)}
    chips = [(name, C.exported(c)[0], C.exported(c)[1], None if verifier_only else prep.get(c))
             for c, name in enumerate(sdk.CHIPS)]
    if not verifier_only:
        return sdk.Machine(chips)
    heights = {sdk.CHIPS[c]: len(pr) for c, pr in prep.items() if pr is not None}
    return sdk.Machine(chips, prep_root=[O.to_mont(x) for x in O.setup_root(prog)],
                       prep_heights=heights)


def table_lookups():
    """A lookup-only table chip: main (mult, b), one preprocessed column a; it receives (a, b)."""
    b = sdk.LookupBuilder(2, 1)
    b.receive(3, [b.prep(0), b.main(1)], b.main(0))
    return b.program()


def sender_program():
    """mulgate's AIR with a single send of (a, b) under its selector s."""
    b = sdk.LookupBuilder(4)
    b.send(3, [b.main(0), b.main(1)], b.main(3))
    return b.program()


def sender_rows(n):
    """A valid mulgate trace of n rows with at most 12 real rows (the table holds 16 keys)."""
    import air_program_cases as A
    rows = A.mulgate_canonical(min(n, 16))
    return rows + [(0, 0, 0, 0)] * (n - len(rows))


@functools.lru_cache(maxsize=None)
def custom_machine(heights):
    """(machine, traces): one mulgate sender per height, named m<height>, and the 16-row table
    whose rows hold every sent (a, b) (then fillers) and whose multiplicities come from
    sdk.lookups_multiplicities.  Traces are Montgomery words, read-only."""
    import air_program_cases as A
    air, lk, tlk = A.mulgate_program(), sender_program(), table_lookups()
    senders = {f"m{n}": C.mont(np.array(sender_rows(n), dtype=np.uint64)) for n in heights}
    keys = sorted({(int(a), int(b)) for n in heights for a, b, _, s in sender_rows(n) if s})
    keys += [(k, 0) for k in range(2, 18)][:16 - len(keys)]
    prep = C.mont(np.array([[a] for a, _ in keys], dtype=np.uint64))
    main = C.mont(np.array([[0, b] for _, b in keys], dtype=np.uint64))
    mult = sdk.lookups_multiplicities(tlk, main, prep, 0, [lk] * len(senders), list(senders.values()),
                                      [None] * len(senders))
    assert mult.unmatched == 0
    main[:, 0] = mult.mult
    m = sdk.Machine([(name, air, lk, None) for name in senders] + [("table", None, tlk, prep)])
    traces = dict(senders, table=main)
    for t in traces.values():
        t.setflags(write=False)
    return m, traces
