"""bfz_lookups_debug / bfz_lookups_multiplicities on the device: k_lookup_prog and the multiplicity
kernels (csrc/lookup_debug_prog.hip) against the compiled chips' k_lookup, word for word, and
against the Python-integer reference at the shapes where they can go wrong."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lookups_debug_cases as D
from bfz import _lib, guests, sdk
from test_lookups_gpu import _trace

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    _lib.init(0)
    yield


@pytest.mark.parametrize("corrupt", [False, True])
def test_exported_programs_equal_the_compiled_path(corrupt):
    """hello's traces: bfz_debug_interactions_traces (k_lookup<CHIP>) and bfz_lookups_debug on the
    exported programs, given the chips in another order, agree on everything."""
    have = [(c, _trace(c, 0)) for c in range(8)]
    have = [(c, m) for c, m in have if m is not None][::-1]  # caller's order: descending chip
    if corrupt:
        have[-1][1][5, 0] ^= 1  # one Cpu cell, read by several lookups
    pk = sdk.ProverClient().setup(guests.HELLO)[0]
    want = sdk.CoreProver().debug_interactions(pk, [(c, sdk.CHIPS[c], m) for c, m in have], limit=4096)
    progs = [sdk.lookups_export(c) for c, _ in have]
    preps = [_trace(c, 1) if sdk.lookups_info(p).prep_width else None for (c, _), p in zip(have, progs)]
    got = sdk.lookups_debug(progs, [m for _, m in have], preps, limit=4096)
    chips = [c for c, _ in have]
    assert want.balanced != corrupt and bool(want.discrepancies) == corrupt
    for f in ("balanced", "total_net", "interactions", "distinct_keys", "unbalanced_keys", "rounds"):
        assert getattr(got, f) == getattr(want, f), f
    assert got.chip_distinct == [want.chip_distinct[c] for c in chips]
    assert len(got.discrepancies) == len(want.discrepancies)
    for g, w in zip(got.discrepancies, want.discrepancies):
        assert (g.kind, g.values, g.net, g.first_row, g.first_interaction) == (
            w.kind, w.values, w.net, w.first_row, w.first_interaction)
        assert chips[g.first_chip] == w.first_chip
        assert g.chip_net == [w.chip_net[c] for c in chips]
        assert g.chip_count == [w.chip_count[c] for c in chips]


@pytest.mark.parametrize("h", [1, 2, 256, 512])
def test_shapes_where_the_walker_can_go_wrong(h):
    progs, mains, preps = D.shapes(h)
    D.check_report(D.run_debug(progs, mains, preps, True, limit=4096),
                   D.ref_debug(list(zip(progs, mains, preps))), 2)


def test_one_hot_key_with_large_multiplicities():
    """With the per-block LDS table and, in a child process (the variable is read once), without."""
    D.hot_key(True)
    code = "import lookups_debug_cases as D; from bfz import _lib; _lib.init(0); D.hot_key(True)"
    env = {**os.environ, "BFZ_LOOKUP_COMBINE": "0", "PYTHONPATH": os.pathsep.join(sys.path)}
    subprocess.run([sys.executable, "-c", code], check=True, env=env)


def test_grid_stride():
    """2^20 rows of one column: more than LK_MAX_BLOCKS x 256 threads' worth."""
    keys = np.random.default_rng(20).integers(0, 50000, size=(1 << 20, 1), dtype=np.uint32)
    b = sdk.LookupBuilder(1)
    b.send(1, [b.main(0)], 1)
    rep = D.run_debug([b.program()], [keys], [None], True, limit=1 << 16)
    vals, counts = np.unique(keys, return_counts=True)
    assert (rep.interactions, rep.distinct_keys, rep.unbalanced_keys) == (1 << 20, len(vals), len(vals))
    assert [d.values for d in rep.discrepancies] == [[int(v)] for v in vals]
    assert [d.net for d in rep.discrepancies] == counts.tolist()
    first = {int(v): i for i, v in reversed(list(enumerate(keys[:, 0].tolist())))}
    assert all(d.first_row == first[d.values[0]] for d in rep.discrepancies[::997])


def test_hash_cut_to_12_bits():
    progs, mains, preps = D.shapes(512)
    _lib.check(_lib.lib().bfz_set_fault_injection(4))
    try:
        rep = D.run_debug(progs, mains, preps, True, limit=4096)
        D.multiplicities(True)
    finally:
        _lib.check(_lib.lib().bfz_set_fault_injection(0))
    assert rep.rounds > 1 and rep.tag_collisions > 0
    D.check_report(rep, D.ref_debug(list(zip(progs, mains, preps))), 2)


def test_cap_below_the_number_of_unbalanced_keys():
    progs, mains, preps = D.shapes(256)
    rep = D.run_debug(progs, mains, preps, True, limit=3)
    assert len(rep.discrepancies) == 3 < rep.unbalanced_keys
    D.check_report(rep, D.ref_debug(list(zip(progs, mains, preps))), 2, limit=3)


def test_multiplicities():
    D.multiplicities(True)


@pytest.mark.parametrize("case", D.REFUSALS)
def test_refusals(case):
    D.refusal(case, True)
