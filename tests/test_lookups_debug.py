"""bfz_lookups_debug / bfz_lookups_multiplicities on the host path (on_device = 0, no GPU): the
compiled lists over a std::map against the Python-integer reference of lookups_debug_cases."""
import pytest

import lookups_debug_cases as D


@pytest.mark.parametrize("h", [1, 2, 256, 512])
def test_shapes_where_the_walker_can_go_wrong(h):
    progs, mains, preps = D.shapes(h)
    agg = D.ref_debug(list(zip(progs, mains, preps)))
    rep = D.run_debug(progs, mains, preps, False, limit=4096)
    D.check_report(rep, agg, 2)
    kinds = {d.kind for d in rep.discrepancies}
    assert 5 not in kinds and 9 not in kinds  # cancelled; multiplicity 0
    if h >= 256:  # every key of column 7 occurs in a row with a multiplicity
        assert {len(d.values) for d in rep.discrepancies if d.kind == 7} == {1, 2}
        assert any(d.kind == 6 and d.net < 0 for d in rep.discrepancies)
        assert all(d.first_interaction == 31 for d in rep.discrepancies if d.kind == 10)
    one = D.run_debug(progs, mains, preps, False, kinds=[10, 3])  # the witness keeps the chain index
    D.check_report(one, D.ref_debug(list(zip(progs, mains, preps)), kinds=[10, 3]), 2)


def test_one_hot_key_with_large_multiplicities():
    D.hot_key(False)


def test_cap_below_the_number_of_unbalanced_keys():
    progs, mains, preps = D.shapes(256)
    agg = D.ref_debug(list(zip(progs, mains, preps)))
    rep = D.run_debug(progs, mains, preps, False, limit=3)
    assert len(rep.discrepancies) == 3 < rep.unbalanced_keys
    D.check_report(rep, agg, 2, limit=3)


def test_multiplicities():
    D.multiplicities(False)


@pytest.mark.parametrize("case", D.REFUSALS)
def test_refusals(case):
    D.refusal(case, False)
