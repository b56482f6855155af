"""Shared inputs of tests/test_uni_device.py (host paths) and tests/test_uni_device_gpu.py (device
paths): the chips' traces, seeded single-cell corruptions and the raw calls of the AIR-only row
check and of the batch verifier.

Traces here are Montgomery words (the product's ABI) unless a name says canonical."""
import ctypes
from functools import lru_cache

import numpy as np

import oracle_lib as O
from bfz import _lib, guests, sdk

P = O.P
CPU, ADDSUB, JUMP, MEMINSTRS, IO = 0, 2, 3, 6, 7
QUERIES = 6
N_CORRUPTIONS = 24
# one small real trace per chip for the corruption tests: (program, stdin, height)
SMALL = {CPU: (guests.LOOP, (), 32), ADDSUB: ("+" * 17, (), 32), JUMP: (guests.HELLO, (), 32),
         MEMINSTRS: (guests.HELLO, (), 64), IO: (",.,.", (7, 9), 16)}
# Seeds of corruptions(): chosen on the CPU so that at least half of each chip's corruptions fail
# an AIR constraint (test_row_check_against_the_merged_checker asserts it).
SEEDS = {CPU: 1, ADDSUB: 3, JUMP: 3, MEMINSTRS: 2, IO: 1}  # 12, 15, 20, 17, 12 of 24 on SMALL


def mont(a):
    return ((np.asarray(a, dtype=np.uint64) << np.uint64(32)) % np.uint64(P)).astype(np.uint32)


@lru_cache(maxsize=None)
def _traces(prog, stdin):
    out = {}
    for c, _, t in sdk.generate_traces(prog, list(stdin)):
        t.setflags(write=False)  # shared between tests: corrupt a copy
        out[c] = t
    return out


def trace_of(chip, prog, stdin=()):
    """The chip's Montgomery trace (read-only), or None when the program does not include it."""
    return _traces(prog, tuple(stdin)).get(chip)


def corruptions(chip, height, width, seed=None, count=N_CORRUPTIONS):
    """[(row, column, canonical value)]: `count` seeded single-cell changes, the first in row 0,
    the second in row height - 1 (whose next row wraps to row 0), the third in the last 256-row
    block; the rest anywhere."""
    rng = np.random.default_rng([chip, height, SEEDS[chip] if seed is None else seed])
    out = []
    for k in range(count):
        row = (0, height - 1, height - 1 - int(rng.integers(0, min(height, 256))))[k] if k < 3 \
            else int(rng.integers(0, height))
        out.append((row, int(rng.integers(0, width)), int(rng.integers(0, P))))
    return out


def corrupt(trace, row, col, value):
    """A copy of the Montgomery trace with one cell set to the canonical `value` (or to the
    cell's value + 1 when that is what the cell already holds)."""
    bad = np.array(trace, dtype=np.uint32)
    new = O.to_mont(value)
    if int(bad[row, col]) == new:
        new = O.to_mont((value + 1) % P)
    bad[row, col] = new
    return bad


def summary(res):
    return (res.chip, res.height, res.num_constraints, res.failing_rows, res.first_row,
            res.first_constraint)


def summary_from_rows(chip, rows):
    """What the summary of a check must be, given its per-row array."""
    bad = np.nonzero(rows >= 0)[0]
    k = sdk.uni_stark_info(chip).num_constraints
    if not len(bad):
        return (chip, len(rows), k, 0, -1, -1)
    return (chip, len(rows), k, len(bad), int(bad[0]), int(rows[bad[0]]))


def uni_check_status(chip, m, on_device=0, h=None, w=None):
    """(status, message) of a raw bfz_uni_check call."""
    m = np.ascontiguousarray(m, dtype=np.uint32)
    out = _lib.UniCheckC()
    L = _lib.lib()
    rc = L.bfz_uni_check(chip, m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                         m.shape[0] if h is None else h, m.shape[1] if w is None else w,
                         on_device, ctypes.byref(out), None)
    return rc, L.bfz_last_error().decode() if rc else ""


def verify_one(chip, proof):
    """bfz_uni_verify: ((ok, query, why), the ending challenger's bytes); None for a refused call."""
    ch = sdk.Challenger()
    buf, n = _lib.u8buf(proof)
    out = _lib.VerifyOutcomeC()
    _lib.check(_lib.lib().bfz_uni_verify(chip, ctypes.byref(ch), buf, n, ctypes.byref(out)))
    return (bool(out.ok), out.query, out.why.decode()), bytes(ch)


def verify_batch(chips, proofs, on_device):
    """bfz_uni_verify_batch from fresh challengers: [((ok, query, why), challenger bytes)].  The
    raw call: sdk.uni_stark_verify_batch binds a device for on_device = 1, which the stand-in of
    fault-injection bit 1 does not need."""
    k = len(proofs)
    bufs = [_lib.u8buf(p) for p in proofs]
    arr = (ctypes.POINTER(ctypes.c_uint8) * k)(
        *[ctypes.cast(b, ctypes.POINTER(ctypes.c_uint8)) for b, _ in bufs])
    lens = (ctypes.c_size_t * k)(*[n for _, n in bufs])
    chs = (sdk.Challenger * k)()
    out = (_lib.VerifyOutcomeC * k)()
    _lib.check(_lib.lib().bfz_uni_verify_batch((ctypes.c_int * k)(*chips), chs, arr, lens, k,
                                               int(bool(on_device)), out))
    return [((bool(o.ok), o.query, o.why.decode()), bytes(c)) for o, c in zip(out, chs)]
