"""Interaction programs on the device: k_perm_rows_prog against the compiled chips' kernels word
for word, against the Python-integer reference at the shapes where it can go wrong, and the
balance check of two caller-defined chips."""
import ctypes

import numpy as np
import pytest

import lookups_cases as LC
from bfz import _lib, guests, sdk

pytestmark = pytest.mark.gpu
P32 = ctypes.POINTER(ctypes.c_uint32)


def _trace(chip, prep):
    """bfz_trace of the hello guest (Montgomery words), or None when hello leaves the chip out."""
    out, h, w = P32(), ctypes.c_size_t(), ctypes.c_size_t()
    buf, n = _lib.u8buf(b"")
    st = _lib.lib().bfz_trace(guests.HELLO.encode(), buf, n, chip, prep, ctypes.byref(out),
                              ctypes.byref(h), ctypes.byref(w))
    if st == 1:
        return None
    _lib.check(st)
    m = np.ctypeslib.as_array(out, shape=(h.value, w.value)).copy()
    _lib.lib().bfz_free(out)
    return m


@pytest.mark.parametrize("chip", range(8), ids=sdk.CHIPS)
def test_exported_program_equals_the_compiled_chip(chip):
    _lib.init(0)
    prog = sdk.lookups_export(chip)
    info = sdk.lookups_info(prog)
    rng = np.random.default_rng(chip)
    main = _trace(chip, 0)
    if main is None:  # not in hello's proof: a random trace serves the comparison as well
        main = rng.integers(0, LC.P, size=(64, info.main_width), dtype=np.uint32)
    prep = _trace(chip, 1) if info.prep_width else None
    alpha, beta = (LC.mont(rng.integers(0, LC.P, 4)) for _ in range(2))
    out, w, cs = P32(), ctypes.c_size_t(), (ctypes.c_uint32 * 4)()
    _lib.check(_lib.lib().bfz_perm_trace(
        chip, main.ctypes.data_as(P32), prep.ctypes.data_as(P32) if prep is not None else None,
        main.shape[0], (ctypes.c_uint32 * 4)(*alpha), (ctypes.c_uint32 * 4)(*beta),
        ctypes.byref(out), ctypes.byref(w), cs))
    want = np.ctypeslib.as_array(out, shape=(main.shape[0], w.value)).copy()
    _lib.lib().bfz_free(out)
    got, got_cs = sdk.lookups_perm_trace(prog, main, prep, alpha, beta, on_device=True)
    assert np.array_equal(got, want)
    assert got_cs == list(cs)


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_device_perm_trace_matches_the_integer_reference(name):
    """The reference hits no zero denominator for these seeds (it asserts so).  The row-sum kernel
    of the balance check (no permutation trace) must give the same cumulative sum."""
    rows, cumsum = LC.run_case(name, on_device=True)
    prog, main, prep, alpha, beta, exp_rows, exp_cumsum = LC.case(name)
    assert np.array_equal(rows, exp_rows)
    assert cumsum == exp_cumsum
    bal = sdk.lookups_balance([prog], [LC.mont(main)], [LC.mont(prep)], LC.mont(alpha), LC.mont(beta))
    assert LC.unmont(bal.cumsums[0]).tolist() == exp_cumsum and not bal.balanced


def test_balance_of_two_chips():
    """Chip B receives, in permuted row order and padded to twice the height with multiplicity-0
    rows, exactly what chip A sends; then one value of one row changes."""
    rng = np.random.default_rng(77)
    a, b = sdk.LookupBuilder(3), sdk.LookupBuilder(4)
    a.send(5, [a.main(1), a.main(2) + 2 * a.main(1)], a.main(0))
    a.send(3, [], a.main(0))
    b.receive(5, [b.main(2), b.main(3) + 2 * b.main(2) + 0 * b.main(1)], b.main(0))
    b.receive(3, [], b.main(0))
    ma = rng.integers(0, LC.P, size=(256, 3), dtype=np.uint32)
    ma[::5, 0] = 0
    mb = rng.integers(0, LC.P, size=(512, 4), dtype=np.uint32)
    mb[:, 0] = 0
    perm = rng.permutation(512)[:256]
    mb[perm, 0], mb[perm, 2], mb[perm, 3] = ma[:, 0], ma[:, 1], ma[:, 2]
    alpha, beta = ([int(x) for x in rng.integers(0, LC.P, 4)] for _ in range(2))
    progs = [a.program(), b.program()]

    def both(ma, mb):
        got = sdk.lookups_balance(progs, [LC.mont(ma), LC.mont(mb)], [None, None], LC.mont(alpha),
                                  LC.mont(beta))
        exp = [LC.ref_perm_trace(p, m, None, alpha, beta)[1] for p, m in zip(progs, (ma, mb))]
        assert [LC.unmont(c).tolist() for c in got.cumsums] == exp
        assert LC.unmont(got.total).tolist() == LC.ef_add(*exp)
        return got

    ok = both(ma, mb)
    assert ok.balanced and ok.total == [0, 0, 0, 0]
    mb[perm[17], 3] = (int(mb[perm[17], 3]) + 1) % LC.P
    assert not both(ma, mb).balanced
