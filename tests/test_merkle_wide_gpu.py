"""Merkle commits whose launches hash more than 16 matrices (the column-table form of every
kernel, csrc/merkle.hip) and short trees (lane-mode leaves, k_hash_leaves_lanes): bfz_commit
against the oracle's root, bit for bit, and a machine with two chips at each of seven neighbouring
heights end to end.  Heights are trace heights n; the committed LDE has 2n rows."""
import numpy as np
import pytest

import air_program_cases as A
import chip_cases as C
import machine_cases as M
from bfz import sdk
from test_merkle_ends import T, commit_case, gpu  # noqa: F401  (gpu: the module's device fixture)

pytestmark = pytest.mark.gpu
CYCLE = (1, 7, 8, 9, 3)  # segment ends inside a chunk, on a chunk's end, twice in one chunk


def cycle(h, n=17):
    return [(h, CYCLE[i % 5]) for i in range(n)]


# 2^16 leaves by threads: k_hash_leaves_tab.  Width 1: every step is a segment's end.
@pytest.mark.parametrize("shapes", [cycle(T), [(T, 1)] * 17], ids=["cycle", "ones"])
def test_table_leaves(shapes):
    commit_case(shapes, 500 + len(shapes) + shapes[1][1])


# 2^15 nodes by threads: k_compress_tab.
def test_table_thread_layer():
    commit_case([(T, 8)] + cycle(T >> 1), 520)


# k_compress_top_tab: 21 segments over the seven layers of a subtree launch (a window that starts
# at a non-zero segment in every layer but the first), and 17 of one height between layers that
# inject nothing.
@pytest.mark.parametrize("small", [[(256 >> k, 3) for k in range(7) for _ in range(3)], [(16, 3)] * 17],
                         ids=["3-per-height", "17-at-16"])
def test_table_subtree(small):
    commit_case([(512, 3)] + small, 540 + len(small))


# Short trees (at most 2^14 leaves).  Below 64 columns the leaves stay with k_hash_leaves (the
# table form for 17 matrices); from 64 on they are hashed in lane mode: exactly full rounds, a
# last round of one column, of one chunk, of one chunk and a column; a segment's end inside a
# chunk, on a chunk's end, twice in one chunk; 17 matrices (the table form, ends inside every
# tile).  Heights: partial blocks (2, 4 rows), exactly one block (64 rows), two, and the largest
# tree that takes the path.
NARROW = [(1,), (7,), (8,), (9,), (16,), (17,), (31,), (5, 12), (8, 8), (3, 5, 9), (3,) * 17]
WIDE = [(64,), (65,), (72,), (73,), (80,), (60, 12), (64, 8), (40, 3, 5, 25), (5,) * 17]


@pytest.mark.parametrize("n,ws", [(32, ws) for ws in NARROW] +
                         [(n, ws) for n in (32, 1 << 13) for ws in WIDE] +
                         [(n, ws) for n in (1, 2, 64) for ws in ((65,), (5,) * 17)],
                         ids=lambda v: str(v) if isinstance(v, int) else f"w{'_'.join(map(str, v[:3]))}x{len(v)}")
def test_lane_leaves(n, ws):
    commit_case([(n, w) for w in ws], 600 + n + sum(ws))


def test_lane_leaves_many_rounds():
    commit_case([(32, 68)] * 8, 700)


def two_per_height_machine():
    """(machine, traces): two mulgate senders at each height 4 .. 256, one at 512 and the 16-row
    table; the quotient round commits 2 chips x 2 chunks x 7 heights in one subtree launch."""
    air, lk, tlk = A.mulgate_program(), M.sender_program(), M.table_lookups()
    senders = {f"m{n}{s}": C.mont(np.array(M.sender_rows(n), dtype=np.uint64))
               for n in (4, 8, 16, 32, 64, 128, 256, 512) for s in ("a", "b")[:1 + (n < 512)]}
    keys = sorted({(int(a), int(b)) for n in (4, 8, 16) for a, b, _, s in M.sender_rows(n) if s})
    keys += [(k, 0) for k in range(2, 18)][:16 - len(keys)]
    prep = C.mont(np.array([[a] for a, _ in keys], dtype=np.uint64))
    main = C.mont(np.array([[0, b] for _, b in keys], dtype=np.uint64))
    mult = sdk.lookups_multiplicities(tlk, main, prep, 0, [lk] * len(senders), list(senders.values()),
                                      [None] * len(senders))
    assert mult.unmatched == 0
    main[:, 0] = mult.mult
    m = sdk.Machine([(name, air, lk, None) for name in senders] + [("table", None, tlk, prep)])
    return m, dict(senders, table=main)


def test_machine_two_chips_per_height():
    m, traces = two_per_height_machine()
    sdk.set_num_queries(6)
    try:
        ch = m.observe()
        proof = m.prove(traces, ch, check=True)
        chv = m.observe()
        out = m.verify(proof, chv)
        assert out.ok, out.why
        chd = m.observe()
        dev = m.verify_batch([proof], [chd], on_device=True)[0]
        assert (dev.ok, dev.query, dev.why) == (out.ok, out.query, out.why) and bytes(chd) == bytes(chv)
        bad = m.prove(dict(traces, m8b=C.flip(traces["m8b"], 1, 2)), m.observe())
        out = m.verify(bad, m.observe())
        assert not out.ok and out.why == "OOD evaluation mismatch on chip m8b", out
    finally:
        sdk.set_num_queries(0)
