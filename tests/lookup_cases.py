"""Shared inputs of tests/test_debug_interactions.py (host path) and
tests/test_debug_interactions_gpu.py (device path): the traces of debug_cases.PROGRAMS, clean,
corrupted and random, each with the report the independent model (lookup_model.py) gives."""
from functools import lru_cache

import numpy as np

import debug_cases as D
import lookup_model as M
from bfz import sdk

P = D.P
PROGS = {name: (prog, tuple(stdin)) for name, prog, stdin in D.PROGRAMS}
RANDOM_SEED = 29


def canonical_traces(name):
    """{chip: (main, prep or None)} of a program of debug_cases.PROGRAMS (read-only arrays)."""
    prog, stdin = PROGS[name]
    return {c: D.traces(prog, stdin, c) for c in D.included(prog, stdin)}


def with_main(traces, chip, main):
    out = dict(traces)
    out[chip] = (main, traces[chip][1])
    return out


def byte_case():
    """hello with one Byte receive too many (the corruption of
    test_unbalanced_byte_lookup_shows_in_the_balance_table): (traces, byte value, clean
    multiplicity)."""
    t = canonical_traces("hello")
    main, prep = t[5]
    row = int(np.nonzero(main[:, 0])[0][0])
    bad = main.copy()
    bad[row, 0] = (int(bad[row, 0]) + 1) % P
    return with_main(t, 5, bad), int(prep[row, 0]), int(main[row, 0])


def alu_key_case():
    """fibo17 with the pc cell of a real AddSub row changed: its ALU receive no longer matches
    the Cpu's send, the totals still do.  (traces, row)."""
    t = canonical_traces("fibo17")
    main, _ = t[2]
    row = int(D.real_rows(2, main)[3])
    bad = main.copy()
    bad[row, 0] = (int(bad[row, 0]) + 1000) % P  # no instruction has this pc
    return with_main(t, 2, bad), row


@lru_cache(maxsize=None)
def random_case(name):
    """A uniformly random main of the same shape for every included chip (seeded as
    tests/test_debug_constraints_gpu.py does); the preprocessed traces stay the program's."""
    rng = np.random.default_rng(RANDOM_SEED)
    out = {}
    for c, (main, prep) in canonical_traces(name).items():
        out[c] = (rng.integers(0, P, main.shape).astype(np.uint32), prep)
    return out


_MODEL = {}


def model(key, traces, kinds=None):
    """lookup_model.debug_interactions, computed once per (case key, kinds)."""
    k = (key, None if kinds is None else tuple(kinds))
    if k not in _MODEL:
        _MODEL[k] = M.debug_interactions(traces, kinds)
    return _MODEL[k]


def lib_traces(traces):
    """The [(chip, name, Montgomery main)] list the SDK takes."""
    return [(c, sdk.CHIPS[c], D.mont(traces[c][0])) for c in sorted(traces)]


@lru_cache(maxsize=None)
def host_key(name):
    return sdk.host_key(PROGS[name][0])


def run(pk, traces, kinds=None, limit=256, on_device=False):
    return sdk.CoreProver().debug_interactions(pk, lib_traces(traces), kinds=kinds, limit=limit,
                                               on_device=on_device)


def run_all(pk, traces, kinds=None, on_device=False):
    """Every unbalanced key: cap = their number."""
    n = run(pk, traces, kinds, 0, on_device).unbalanced_keys
    return run(pk, traces, kinds, n, on_device)


def assert_counters(rep, want):
    for f in ("balanced", "total_net", "interactions", "distinct_keys", "unbalanced_keys",
              "chip_distinct"):
        assert getattr(rep, f) == want[f], (f, getattr(rep, f), want[f])


def assert_record(d, w):
    assert (d.kind, d.values, d.net) == (w["kind"], w["values"], w["net"]), (d, w)
    assert d.chip_net == w["chip_net"] and d.chip_count == w["chip_count"], (d, w)
    assert (d.first_chip, d.first_row, d.first_interaction) == w["first"], (d, w)
    assert (sum(d.chip_net) - d.net) % P == 0


def assert_matches_model(rep, want, n=None):
    """Counters and the first n (default: all) records equal the model's, in order."""
    assert_counters(rep, want)
    n = want["unbalanced_keys"] if n is None else n
    assert len(rep.discrepancies) == n
    for d, w in zip(rep.discrepancies, want["records"][:n]):
        assert_record(d, w)


def same_reports(a, b):
    """Device == host field by field, the device path's diagnostics aside."""
    for f in ("balanced", "total_net", "interactions", "distinct_keys", "unbalanced_keys",
              "chip_distinct", "discrepancies"):
        assert getattr(a, f) == getattr(b, f), f

