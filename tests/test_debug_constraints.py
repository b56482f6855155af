"""The constraint checker's host path (bfz_check_chip, on_device = 0): the reference's debug mode
(crates/stark/src/debug.rs:24-105) on oracle traces -- clean traces pass, an independent numpy
model of AddSub's AIR agrees on every first failing index, and single-cell corruptions are
reported at the row and constraint index they break.  No device needed."""
import numpy as np
import pytest

import debug_cases as D
import oracle_lib as O
from bfz import guests, sdk

P = O.P


@pytest.mark.parametrize("name,prog,stdin", D.PROGRAMS, ids=[p[0] for p in D.PROGRAMS])
def test_clean_traces_pass(name, prog, stdin):
    alpha, beta = D.challenges(3)
    chips = D.included(prog, stdin)
    assert 0 in chips and 5 in chips
    for chip in chips:
        main, prep = D.traces(prog, stdin, chip)
        perm, cs = D.perm(chip, main, prep, alpha, beta)
        res = D.check(chip, main, prep, perm, alpha, beta, cs)
        assert res.failing_rows == 0, str(res)
        assert res.first_row == -1 and res.first_constraint == -1
        assert (res.first_fail_per_row == -1).all()
        assert res.height == main.shape[0] and res.chip == chip
        assert res.num_batches == (D.N_LOOKUPS[chip] + 1) // 2
        if chip == 2:
            assert res.num_constraints == 14
    if name == "plus":
        assert D.traces(prog, stdin, 0)[0].shape[0] == 1  # one cycle: a 1-row Cpu trace


def addsub_model(t):
    """First failing AIR index (or -1) per row of an AddSub trace, written from
    AddSubChip::eval (alu/mod.rs:159-176) and AddOperation::eval (operations/add.rs:49-67).
    Columns: pc, value, carry, operand_1, operand_2, is_add, is_sub.  Python integers mod p."""
    out = np.full(t.shape[0], -1, dtype=np.int32)
    for i, (pc, value, carry, a, b, is_add, is_sub) in enumerate(t.tolist()):
        is_real = (is_add + is_sub) % P
        overflow = (a + b - value) % P
        cons = [
            is_add * (is_add - 1),                    # assert_bool(is_add)
            is_sub * (is_sub - 1),                    # assert_bool(is_sub)
            is_real * (is_real - 1),                  # assert_bool(is_real)
            is_real * overflow * (overflow - 256),    # overflow is 0 or the base
            is_real * carry * (overflow - 256),       # carry = 1 -> overflow = base
            is_real * (carry - 1) * overflow,         # carry != 1 -> overflow = 0
            is_real * carry * (carry - 1),            # assert_bool(carry)
            is_real * is_real * (is_real - 1),        # assert_bool(is_real) under when(is_real)
        ]
        for k, c in enumerate(cons):
            if c % P:
                out[i] = k
                break
    return out


def test_addsub_agrees_with_independent_model():
    """Wherever the model says an AIR constraint fails, the library's first failing index is the
    model's (rows the model passes may still fail a LogUp constraint: not compared)."""
    alpha, beta = D.challenges(5)
    rng = np.random.default_rng(17)
    cases = [rng.integers(0, P, (1 << 10, 7)).astype(np.uint32)]
    # small values too, so that the bool and carry constraints hold on some rows and later
    # indices come first
    cases.append(rng.integers(0, 3, (1 << 10, 7)).astype(np.uint32))
    fibo, _ = D.traces(guests.FIBO, (17,), 2)
    for col in range(7):
        t = fibo.copy()
        t[:, col] = rng.integers(0, P, t.shape[0])
        cases.append(t)
        t = fibo.copy()
        t[:, col] = rng.integers(0, 3, t.shape[0])
        cases.append(t)
    seen = set()
    for t in cases:
        perm, cs = D.perm(2, t, None, alpha, beta)
        res = D.check(2, t, None, perm, alpha, beta, cs)
        want = addsub_model(t)
        rows = want >= 0
        assert (res.first_fail_per_row[rows] == want[rows]).all()
        # a row the model passes fails no AIR constraint
        assert not ((res.first_fail_per_row[~rows] >= 0) & (res.first_fail_per_row[~rows] < 8)).any()
        assert res.failing_rows == int((res.first_fail_per_row >= 0).sum())
        seen |= set(want[rows].tolist())
    assert len(seen) >= 4, seen  # not "always 0"


CASES = D.corruption_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_single_cell_corruptions(case):
    name, chip, main, prep, perm, alpha, beta, cs, expect = case
    expect(D.check(chip, main, prep, perm, alpha, beta, cs))


def test_report_text_names_chip_row_and_constraint():
    name, chip, main, prep, perm, alpha, beta, cs, _ = CASES[0]
    res = D.check(chip, main, prep, perm, alpha, beta, cs)
    text = str(res)
    assert "AddSub" in text and f"row {res.first_row}" in text
    assert "constraint 0 of 14 (AIR constraint 0)" in text
    assert sdk.constraint_name(8, 14, 3) == "LogUp batch 0"
    assert sdk.constraint_name(10, 14, 3) == "LogUp batch 2"
    assert [sdk.constraint_name(k, 14, 3) for k in (11, 12, 13)] == [
        "LogUp first-row", "LogUp transition", "LogUp last-row"]


def test_bad_arguments_are_errors_not_results():
    alpha, beta = D.challenges(3)
    main, _ = D.traces(guests.LOOP, (), 2)
    perm, cs = D.perm(2, main, None, alpha, beta)
    with pytest.raises(sdk.BfzError, match="power of two"):
        D.check(2, main[:3], None, perm[:3], alpha, beta, cs)
    with pytest.raises(sdk.BfzError, match="width"):
        D.check(2, main[:, :6], None, perm, alpha, beta, cs)
    bad = D.mont(main).copy()
    bad[0, 0] = P  # not a field word
    with pytest.raises(sdk.BfzError, match="non-canonical"):
        sdk.check_chip(2, bad, None, D.mont(perm), [O.to_mont(x) for x in alpha],
                       [O.to_mont(x) for x in beta], [O.to_mont(x) for x in cs])
    bmain, bprep = D.traces(guests.LOOP, (), 5)
    with pytest.raises(sdk.BfzError, match="preprocessed"):
        D.check(5, bmain, None, D.perm(5, bmain, bprep, alpha, beta)[0], alpha, beta, cs)
