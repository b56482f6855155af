"""Shared by tests/test_lookups_debug.py (host path) and tests/test_lookups_debug_gpu.py (device):
the cases of bfz_lookups_debug / bfz_lookups_multiplicities and a plain Python-integer reference of
the per-key aggregation (lookup/debug.rs:59-196).  Canonical integers throughout; the library gets
Montgomery words."""
import functools
import struct

import numpy as np
import pytest

from bfz import sdk
from lookups_cases import P, R_INV, mont

HALF = (P - 1) // 2


def f2i(x):
    """field_to_int (lookup/debug.rs:46-54)."""
    x %= P
    return x - P if x > P // 2 else x


def ref_debug(chips, kinds=None):
    """chips: [(prog, main, prep)].  {(kind, nvals, values): [net, chip_net, chip_count, witness]}
    over Python integers, reading the BFL1 words itself; witness = (chip, row, interaction)."""
    agg = {}
    for k, (prog, main, prep) in enumerate(chips):
        w = struct.unpack(f"<{len(prog) // 4}I", prog)
        n, at, chain = w[3], 4, []
        for _ in range(n):
            kind, send, nv = w[at:at + 3]
            at += 3
            cols = []
            for _ in range(nv + 1):
                c, nt = w[at] * R_INV % P, w[at + 1]
                cols.append((c, [(w[at + 2 + 3 * i], w[at + 3 + 3 * i], w[at + 4 + 3 * i] * R_INV % P)
                                 for i in range(nt)]))
                at += 2 + 3 * nt
            chain.append((kind, send, cols))
        for r in range(len(main)):
            m, pr = [int(x) for x in main[r]], [int(x) for x in prep[r]] if prep is not None else None
            for j, (kind, send, cols) in enumerate(chain):
                if kinds is not None and kind not in kinds:
                    continue
                mu, *vals = [(c + sum(wt * (pr if s else m)[col] for s, col, wt in t)) % P for c, t in cols]
                if mu == 0:
                    continue
                e = agg.setdefault((kind, len(vals), tuple(vals)),
                                   [0, [0] * len(chips), [0] * len(chips), (k, r, j)])
                e[0] += f2i(mu) if send else -f2i(mu)
                e[1][k] += f2i(mu) if send else -f2i(mu)
                e[2][k] += 1
    return agg


def check_report(rep, agg, nchips, limit=None):
    """rep (sdk.LookupReport) against the reference: counts, then the records in key order."""
    bad = sorted(k for k, e in agg.items() if e[0] % P)
    assert rep.interactions == sum(sum(e[2]) for e in agg.values())
    assert rep.distinct_keys == len(agg) and rep.unbalanced_keys == len(bad)
    assert rep.balanced == (not bad) and rep.total_net == f2i(sum(e[0] for e in agg.values()))
    assert rep.chip_distinct == [sum(1 for e in agg.values() if e[2][c]) for c in range(nchips)]
    got = [((d.kind, len(d.values), tuple(d.values)), d.net, d.chip_net, d.chip_count,
            (d.first_chip, d.first_row, d.first_interaction)) for d in rep.discrepancies]
    want = [(k, f2i(agg[k][0]), [f2i(x) for x in agg[k][1]], agg[k][2], agg[k][3]) for k in bad]
    assert got == (want if limit is None else want[:limit])


@functools.lru_cache(maxsize=None)
def shapes(h):
    """Two chips of h rows (progs, mains, preps) where the walker can go wrong.  Chip A: 32
    interactions; B receives what A's interaction 2 sends.  Multiplicity main(0) is 0 in every
    third row."""
    rng = np.random.default_rng(h)
    a, b = sdk.LookupBuilder(9, 5), sdk.LookupBuilder(2)
    wide = sum((int(rng.integers(1, P)) * c for c in [a.main(1), a.prep(0), a.main(2), a.prep(4), a.main(8),
                                                      a.prep(2), a.main(5), a.prep(1)]), 11)  # 8 terms
    a.send(3, [], a.main(0))                                        # 0: no values
    a.send(4, [wide] + [a.main(c) for c in range(1, 7)], a.main(0))  # 1: 7 values
    a.send(5, [a.main(1), a.prep(3)], a.main(0))                    # 2: cancelled by B
    a.send(6, [a.main(7)], P - 1)                                   # 3: a 0-term VCOL, counts as -1
    a.send(7, [a.main(7)], a.main(0))                               # 4, 5: differ only in nvals
    a.send(7, [a.main(7), 0], a.main(0))
    a.send(8, [a.main(7)], a.main(0))                               # 6: differs from 4 only in kind
    for _ in range(7, 31):
        a.send(9, [a.main(4)], 0)                                   # multiplicity 0: never counted
    a.receive(10, [a.main(7)], a.main(0))                           # 31: the only carrier of kind 10
    b.receive(5, [b.main(1), 77], b.main(0))
    ma = rng.integers(0, P, size=(h, 9), dtype=np.uint32)
    ma[:, 7] = rng.integers(0, 4, size=h)  # few keys, many rows each
    ma[::3, 0] = 0
    pa = rng.integers(0, P, size=(h, 5), dtype=np.uint32)
    pa[:, 3] = 77
    mb = np.stack([ma[:, 0], ma[:, 1]], axis=1)[::-1].copy()  # the same multiset, other rows
    return [a.program(), b.program()], [ma, mb], [pa, None]


def run_debug(progs, mains, preps, on_device, **kw):
    return sdk.lookups_debug(progs, [mont(m) for m in mains],
                             [mont(p) if p is not None else None for p in preps], on_device=on_device, **kw)


def hot_key(on_device):
    """4096 rows, one key, multiplicity (p - 1) / 2 each: the net is the integer sum."""
    b = sdk.LookupBuilder(1)
    b.send(2, [5, 6], b.main(0))
    rep = run_debug([b.program()], [np.full((4096, 1), HALF, dtype=np.uint32)], [None], on_device)
    assert (rep.interactions, rep.distinct_keys, rep.unbalanced_keys) == (4096, 1, 1)
    d = rep.discrepancies[0]
    assert (d.kind, d.values, d.net, d.chip_net, d.chip_count) == (2, [5, 6], f2i(4096 * HALF), [f2i(4096 * HALF)], [4096])
    assert (d.first_chip, d.first_row, d.first_interaction) == (0, 0, 0)


def table_and_senders(seed=5):
    """A 256-row table with key (row) and a 1024-row chip with two sends per row in [0, 256)."""
    rng = np.random.default_rng(seed)
    t, s = sdk.LookupBuilder(2), sdk.LookupBuilder(2)
    t.receive(12, [t.main(0)], t.main(1))
    s.send(12, [s.main(0)], 1)
    s.send(12, [s.main(1)], 1)
    table = np.stack([np.arange(256), np.zeros(256)], axis=1).astype(np.uint32)
    return t.program(), table, s.program(), rng.integers(0, 256, size=(1024, 2), dtype=np.uint32)


def multiplicities(on_device):
    tp, table, sp, send = table_and_senders()
    run = lambda tb, sd: sdk.lookups_multiplicities(tp, mont(tb), None, 0, [sp], [mont(sd)], [None], on_device)
    counts = np.bincount(send.ravel(), minlength=256)
    got = run(table, send)
    assert np.array_equal(got.mult, mont(counts))
    assert (got.interactions, got.distinct_keys, got.unmatched) == (2048, np.count_nonzero(counts), 0)
    full = np.stack([table[:, 0], counts], axis=1)  # the column written into the table's trace
    one = [int(x) for x in mont([1, 0, 0, 0])]
    assert sdk.lookups_balance([tp, sp], [mont(full), mont(send)], [None, None], one, one, on_device).balanced
    rep = run_debug([tp, sp], [full, send], [None, None], on_device)
    assert rep.balanced and rep.discrepancies == []
    off = send.copy()
    off[700, 1] = 256  # sent, not in the table
    got = run(table, off)
    d = got.first_unmatched
    assert got.unmatched == 1 and (d.kind, d.values, d.net) == (12, [256], 1)
    assert (d.first_chip, d.first_row, d.first_interaction) == (0, 700, 1)
    dup = table.copy()
    dup[9, 0] = 3  # rows 3 and 9 hold the same key: the first takes everything
    got = run(dup, send)
    want = counts.copy()
    want[9] = 0
    assert np.array_equal(got.mult, mont(want)) and got.unmatched == (1 if counts[9] else 0)


def _big_kind():
    b = sdk.LookupBuilder(1)
    b.send(1, [], 1)
    b.send(1 << 24, [], 1)
    return b.program()


def refusal(case, on_device):
    """Each refusal: a negative status (sdk.BfzError) with the documented message."""
    tp, table, sp, send = table_and_senders()
    one = np.ones((4, 1), dtype=np.uint32)
    calls = {
        "kind": (r"kind 16777216 of chip 1, interaction 1 is not below 2\^24",
                 lambda: sdk.lookups_debug([sp, _big_kind()], [mont(send), one], [None, None], on_device=on_device)),
        "chips": (r"chip count not in \[1, 32\]",
                  lambda: sdk.lookups_debug([sp] * 33, [mont(send)] * 33, [None] * 33, on_device=on_device)),
        "word": (r"\(>= p\)",
                 lambda: sdk.lookups_debug([sp], [np.full((4, 2), P, dtype=np.uint32)], [None], on_device=on_device)),
        "height": (r"height not a power of two in \[1, 2\^23\]",
                   lambda: sdk.lookups_debug([sp], [mont(send[:768])], [None], on_device=on_device)),
        "interaction": (r"interaction 1 is not below the table program's 1",
                        lambda: sdk.lookups_multiplicities(tp, mont(table), None, 1, [sp], [mont(send)], [None],
                                                           on_device)),
    }
    msg, call = calls[case]
    with pytest.raises(sdk.BfzError, match=msg):
        call()


REFUSALS = ["kind", "chips", "word", "height", "interaction"]
