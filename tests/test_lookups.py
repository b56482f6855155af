"""Interaction programs (BFL1, bfz_lookups_*) on the host path: the exported programs' shapes, the
validation, and the single-threaded permutation trace against the Python-integer reference."""
import struct

import numpy as np
import pytest

import lookups_cases as LC
from bfz import _lib, sdk

# SURVEY section 2's chip table: (interactions, permutation width in EF columns)
CHIP_SHAPES = [(16, 9), (1, 2), (5, 4), (1, 2), (4, 3), (2, 2), (1, 2), (1, 2)]


@pytest.mark.parametrize("chip", range(8), ids=sdk.CHIPS)
def test_exported_programs_have_the_chip_tables_shapes(chip):
    info = sdk.lookups_info(sdk.lookups_export(chip))
    assert (info.n_interactions, info.perm_width) == CHIP_SHAPES[chip]
    assert info.sends + info.receives == info.n_interactions
    assert (info.prep_width > 0) == (chip in (1, 5))  # Program and Byte use their prep columns


def _base_words():
    """17 words: header 0-3, kind 4, direction 5, n_values 6, mult VCOL 7-11 (constant, n_terms,
    source, column, weight), one value VCOL 12-16."""
    b = sdk.LookupBuilder(3, 1)
    b.send(2, [b.prep(0) * 5 + 1], b.main(2))
    prog = b.program()
    return list(struct.unpack(f"<{len(prog) // 4}I", prog))


def _set(at, v):
    return lambda w: w[:at] + [v] + w[at + 1:]


@pytest.mark.parametrize("mutate,word", [
    (_set(0, 0x31414642), 0),          # bad magic ("BFA1")
    (_set(10, 3), 10),                 # a main column >= the width
    (_set(15, 1), 15),                 # a prep column >= the width
    (_set(11, LC.P), 11),              # a weight >= p
    (_set(3, 33), 3),                  # 33 interactions
    (_set(6, 8), 6),                   # 8 values
    (lambda w: w[:-1], 16),            # truncated
    (lambda w: w + [0], 17),           # trailing words
], ids=["magic", "main-column", "prep-column", "word-ge-p", "33-interactions", "8-values",
        "truncated", "trailing"])
def test_malformed_programs_name_the_word(mutate, word):
    w = _base_words()
    assert len(w) == 17 and sdk.lookups_info(struct.pack("<17I", *w)).n_interactions == 1
    bad = mutate(w)
    with pytest.raises(_lib.BfzError, match=rf"status -\d+: lookup program: .*\(word {word}\)"):
        sdk.lookups_info(struct.pack(f"<{len(bad)}I", *bad))


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_host_perm_trace_matches_the_integer_reference(name):
    rows, cumsum = LC.run_case(name, on_device=False)
    _, _, _, _, _, exp_rows, exp_cumsum = LC.case(name)
    assert np.array_equal(rows, exp_rows)
    assert cumsum == exp_cumsum


def test_host_path_refuses_words_not_below_p():
    prog, main, prep, alpha, beta, _, _ = LC.case("pair-h2")
    bad = LC.mont(main)
    bad[1, 4] = LC.P
    with pytest.raises(_lib.BfzError, match=r"non-canonical field word \(>= p\)"):
        sdk.lookups_perm_trace(prog, bad, LC.mont(prep), LC.mont(alpha), LC.mont(beta), False)
