"""bfz_machine_check / Machine.check on the host path (on_device=False) against the per-chip host
calls and a recount in Python integers.  A proving machine commits its preprocessed traces on the
device when it is created, so the tests that build one are marked gpu although the check itself
touches no device; the verifier-only refusal runs anywhere."""
import numpy as np
import pytest

import chip_cases as C
import machine_cases as M
import machine_check_cases as K
import uni_stark_model as U
from bfz import _lib, guests, sdk

needs_machine = pytest.mark.gpu


def _copy(ch):
    return sdk.Challenger.from_buffer_copy(ch)


def _model_samples(m, count):
    """`count` extension samples (Montgomery words) after the machine's transcript head."""
    ch = U.Challenger()
    ch.observe_all([int(x) for x in C.unmont(np.array(m.prep_root, dtype=np.uint32))] + [0] * 7)
    return [C.mont(np.array(ch.sample_ef().c)).tolist() for _ in range(count)]


@needs_machine
def test_valid_traces():
    m, traces = M.custom_machine(K.HEIGHTS)
    ch = m.observe()
    rep = m.check(traces, ch, on_device=False, profile=True)
    assert rep.ok and rep.cumulative_sum == [0, 0, 0, 0] and rep.names == list(traces)
    want = _model_samples(m, 4)
    assert [rep.alpha, rep.beta] == want[:2]
    again = m.check(traces, ch, on_device=False)  # ch was advanced: the next two samples
    assert [again.alpha, again.beta] == want[2:] and again.ok
    for name, c, counts, firsts in zip(rep.names, rep.chips, rep.counts, rep.first_rows):
        _, cs = sdk.lookups_perm_trace(K.programs(name)[2], traces[name],
                                       m._check_preps.get(c.chip), rep.alpha, rep.beta, on_device=False)
        assert c.failing_rows == 0 and c.cumulative_sum == cs and c.chip == m.names.index(name.encode())
        assert not counts.any() and (firsts == -1).all()


@needs_machine
@pytest.mark.parametrize("flip", K.FLIPS, ids=K.FLIP_IDS)
def test_broken_traces(flip):
    m, traces = M.custom_machine(K.HEIGHTS)
    bad = K.flipped(traces, *flip)
    rep = m.check(bad, on_device=False, profile=True)
    assert not rep.ok
    for name, c, counts, firsts in zip(rep.names, rep.chips, rep.counts, rep.first_rows):
        air, mirror, lk = K.programs(name)
        prep = m._check_preps.get(c.chip)
        perm, cs = sdk.lookups_perm_trace(lk, bad[name], prep, rep.alpha, rep.beta, on_device=False)
        ref = sdk.chip_check(air, lk, bad[name], prep, perm, rep.alpha, rep.beta, cs, on_device=False)
        assert c.cumulative_sum == cs
        C.same_check(c, ref)  # (neither carries a per-row array)
        nz = K.recount(mirror, lk, bad[name], prep, perm, rep.alpha, rep.beta, cs)
        assert nz.shape == (c.height, c.num_constraints)
        assert np.array_equal(counts, nz.sum(axis=0))
        assert np.array_equal(firsts, np.where(nz.any(axis=0), nz.argmax(axis=0), -1))
        assert c.failing_rows == nz.any(axis=1).sum()
    if flip[0] == "table":  # every constraint intact: the total alone says no
        assert all(c.failing_rows == 0 for c in rep.chips) and any(rep.cumulative_sum)
    else:
        assert rep.chips[rep.names.index(flip[0])].first_row == flip[1]


@needs_machine
@pytest.mark.parametrize("case, match", [
    ("word", r"non-canonical field word \(>= p\) in m4"),
    ("repeat", "bad or repeated chip index"),
    ("height", "chip table is not at its preprocessed height"),
    ("counts", "counts and first_rows are given together or not at all"),
])
def test_refusals(case, match):
    import ctypes
    m, traces = M.custom_machine(K.HEIGHTS)
    t = {k: np.array(v) for k, v in traces.items()}
    if case == "word":
        t["m4"][2, 1] = C.P
    if case == "height":
        t["table"] = t["table"][:8]
    idx, ptrs, hs, k, _ = m._traces_c(t)
    if case == "repeat":
        idx[1] = idx[0]
    rep, per = _lib.MachineCheckReport(), (_lib.ChipCheck * k)()
    counts = (ctypes.c_uint64 * 64)() if case == "counts" else None
    status = _lib.lib().bfz_machine_check(m._h, idx, ptrs, hs, k, ctypes.byref(m.observe()), 0,
                                          ctypes.byref(rep), per, counts, None)
    assert status < 0
    with pytest.raises(sdk.BfzError, match=match):
        _lib.check(status)


def test_verifier_only_machine_refused():
    m = M.builtin_machine(guests.HELLO, verifier_only=True)
    t = {name: main for _, name, main, _ in M.guest_traces(guests.HELLO)}
    with pytest.raises(sdk.BfzError, match="verifier-only machine holds no preprocessed traces"):
        m.check(t, on_device=False)
