#!/usr/bin/env python3
"""The constraint profile against the first-fail row check of the same build, in one process, on
the headline record's traces (FIBO_X4 stdin [255]): Cpu 2^22 x 31 and Jump 2^19 x 45
(profiles/r12/check_constraints.json).

  uni   bfz_uni_check  against  bfz_uni_check_constraints       k_check_air<CHIP> / k_profile_air<CHIP>
  air   bfz_air_check  against  bfz_air_check_constraints       k_check_prog / k_profile_prog
        (the chip's exported program)
  rec   bfz_record_uni_check  against  bfz_record_uni_check_constraints   (no upload; valid only)

on a valid trace and on a trace with one column wrong on every row (every lane fails the
constraints that read it).  on_device = 1; wall clock around the whole C call, which for uni / air
includes the upload and the transpose of the host trace; the four calls of a trace alternate;
median and min-max of --runs warm calls after --warmups.  No threshold: the first-fail kernels are
the yardstick.

  python scripts/check_constraints_time.py [--out FILE] [--runs 6] [--warmups 3]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zkvm-brainfuck_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# (chip, name, a column that constraints without a selector read)
CHIPS = ((0, "Cpu", 23), (3, "Jump", 43))
P = 0x7F000001
P32 = ctypes.POINTER(ctypes.c_uint32)


def alternate(calls, runs, warmups):
    """calls: {name: f}; every f is timed whole, the calls taking turns."""
    from uni_stark_time import spread
    for f in calls.values():
        for _ in range(warmups):
            f()
    ms = {k: [] for k in calls}
    for _ in range(runs):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: spread(v) for k, v in ms.items()}


def trace_calls(lib, L, chip, prog, t, k, expect):
    """The four calls on one trace; expect(failing_rows, counts or None) checks each result."""
    out = lib.UniCheckC()
    counts, first = (ctypes.c_uint64 * k)(), (ctypes.c_int64 * k)()
    buf, n = lib.u8buf(prog)
    tp, h, w = t.ctypes.data_as(P32), t.shape[0], t.shape[1]

    def done(rc, tables):
        lib.check(rc)
        expect(out.failing_rows, list(counts) if tables else None)
    return {
        "uni_first_fail": lambda: done(L.bfz_uni_check(chip, tp, h, w, 1, ctypes.byref(out), None), False),
        "uni_profile": lambda: done(L.bfz_uni_check_constraints(chip, tp, h, w, 1, ctypes.byref(out),
                                                                counts, first), True),
        "air_first_fail": lambda: done(L.bfz_air_check(buf, n, tp, h, w, 1, ctypes.byref(out), None), False),
        "air_profile": lambda: done(L.bfz_air_check_constraints(buf, n, tp, h, w, 1, ctypes.byref(out),
                                                                counts, first), True),
    }


def timings(runs, warmups):
    import numpy as np
    from bfz import _lib, guests, sdk
    from uni_stark_time import trace
    L = _lib.lib()
    res = {"program": "FIBO_X4", "stdin": [255], "runs": runs, "warmups": warmups,
           "method": "wall clock around the whole C call, on_device = 1; the calls of a trace "
                     "alternate in one process; ms", "chips": {}}
    client = sdk.ProverClient()
    pk, _ = client.setup(guests.FIBO_X4)
    buf, n = _lib.u8buf(bytes([255]))
    rec = ctypes.c_void_p()
    _lib.check(L.bfz_record_new(ctypes.c_void_p(pk.handle), buf, n, ctypes.byref(rec), None))
    try:
        for chip, name, col in CHIPS:
            t = trace(chip)
            h = t.shape[0]
            k = sdk.uni_stark_info(chip).num_constraints
            prog = sdk.air_export(chip)
            bad = t.copy()  # canonical value + 2 in every row of the column
            bad[:, col] = (bad[:, col].astype(np.uint64) + np.uint64((2 << 32) % P)) % np.uint64(P)

            def valid(rows, counts):
                assert rows == 0 and not (counts and any(counts))

            def wrong(rows, counts):
                assert rows == h and (counts is None or max(counts) == h)
            out = _lib.UniCheckC()
            counts, first = (ctypes.c_uint64 * k)(), (ctypes.c_int64 * k)()
            res["chips"][name] = {
                "height": int(h), "width": int(t.shape[1]), "constraints": k, "wrong_column": col,
                "valid": alternate(trace_calls(_lib, L, chip, prog, t, k, valid), runs, warmups),
                "column_wrong": alternate(trace_calls(_lib, L, chip, prog, bad, k, wrong), runs, warmups),
                "record_valid": alternate({
                    "first_fail": lambda: _lib.check(L.bfz_record_uni_check(rec, chip, ctypes.byref(out))),
                    "profile": lambda: _lib.check(L.bfz_record_uni_check_constraints(
                        rec, chip, ctypes.byref(out), counts, first))}, runs, warmups)}
    finally:
        L.bfz_record_free(rec)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--warmups", type=int, default=3)
    a = ap.parse_args()
    from bfz import _lib
    _lib.init(0)
    text = json.dumps(timings(a.runs, a.warmups), indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
