#!/usr/bin/env python3
"""Times the device constraint checker against a proof of the same record, in one process:
bfz_record_debug_constraints without and with the balance table, and bfz_record_prove (whose
stage events give the quotient stage: the same constraints on twice as many points).  Every call
is warmed once, then the three are timed alternately `--reps` times on a host clock around the
call (each call ends in a stream synchronize).  Prints one JSON line; DESIGN.md quotes it.

  python scripts/debug_constraints_time.py [--program fibo_x4|fibo17|hello] [--reps 5]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zkvm-brainfuck_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--program", default="fibo_x4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    from bfz import _lib, guests, sdk
    prog, stdin = {"fibo_x4": (guests.FIBO_X4, bytes([255])),
                   "fibo17": (guests.FIBO, bytes([17])),
                   "hello": (guests.HELLO, b"")}[args.program]
    L = _lib.lib()
    _lib.init(args.device)
    client = sdk.ProverClient(device=args.device)
    pk, _ = client.setup(prog)
    rec = ctypes.c_void_p()
    cycles = ctypes.c_uint64()
    buf, n = _lib.u8buf(stdin)
    _lib.check(L.bfz_record_new(ctypes.c_void_p(pk.handle), buf, n, ctypes.byref(rec),
                                ctypes.byref(cycles)))

    def debug(flags):
        ch = _lib.Challenger()
        out = _lib.DebugReportC()
        t0 = time.perf_counter()
        _lib.check(L.bfz_record_debug_constraints(ctypes.c_void_p(pk.handle), rec, ctypes.byref(ch),
                                                  flags, ctypes.byref(out)))
        ms = (time.perf_counter() - t0) * 1e3
        if not out.ok:
            raise SystemExit("debug_constraints_time: the record does not satisfy its constraints")
        return ms, out

    def prove(timings=None):
        ptr = ctypes.POINTER(ctypes.c_uint8)()
        plen = ctypes.c_size_t()
        t0 = time.perf_counter()
        _lib.check(L.bfz_record_prove(ctypes.c_void_p(pk.handle), rec, ctypes.byref(ptr),
                                      ctypes.byref(plen), timings))
        ms = (time.perf_counter() - t0) * 1e3
        L.bfz_free(ptr)
        return ms

    _, rep = debug(0)
    debug(1)
    prove()
    t = {"check": [], "check_balance": [], "prove": []}
    for _ in range(args.reps):
        t["check"].append(debug(0)[0])
        t["check_balance"].append(debug(1)[0])
        t["prove"].append(prove())
    tm = _lib.Timings()
    prove(ctypes.byref(tm))  # stage events (slower than an untimed proof: not in the list above)
    L.bfz_record_free(rec)

    # algorithmic bytes of the row check: every main, preprocessed and permutation cell is read
    # as a local and as a next row
    main_w, prep_w, perm_w = sdk._MAIN_W, sdk._PREP_W, sdk._PERM_W
    cells = sum(c.height * (main_w[c.chip] + prep_w[c.chip] + perm_w[c.chip])
                for c in (rep.chips[i] for i in range(rep.n_chips)))
    med = {k: statistics.median(v) for k, v in t.items()}
    print(json.dumps({
        "program": args.program, "cycles": cycles.value, "reps": args.reps,
        "heights": {sdk.CHIPS[rep.chips[i].chip]: rep.chips[i].height for i in range(rep.n_chips)},
        "check_ms": [round(x, 3) for x in t["check"]],
        "check_balance_ms": [round(x, 3) for x in t["check_balance"]],
        "prove_ms": [round(x, 3) for x in t["prove"]],
        "median_ms": {k: round(v, 3) for k, v in med.items()},
        "check_over_prove": round(med["check"] / med["prove"], 3),
        "check_balance_over_prove": round(med["check_balance"] / med["prove"], 3),
        "timed_proof_stage_ms": {"trace": round(tm.trace_ms, 3), "perm_rows": round(tm.perm_rows_ms, 3),
                                 "quotient": round(tm.quotient_ms, 3)},
        "check_cells": cells, "check_algorithmic_bytes": 8 * cells,
    }), flush=True)


if __name__ == "__main__":
    main()
