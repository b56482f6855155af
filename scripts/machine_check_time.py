#!/usr/bin/env python3
"""Machine.check (bfz_machine_check: one upload, k_perm_rows_machine, the running sums, one
k_check_machine launch per class of chips) against the loop Machine.prove(check=True) runs
(lookups_perm_trace + chip_check per chip: the permutation trace down and up again, one
k_check_chip_prog launch per chip), host wall clock around the whole calls, alternating after a
warm-up of each (profiles/r20/machine_check.json).  The public interface has no entry point that
times the check launches alone, so the launch-level comparison is the same two forms with the
per-chip permutation traces computed beforehand: chip_check per chip (upload + one launch each)
beside the whole Machine.check.  Two machines: 31 mulgate senders of 2^10 rows and their table
(32 chips, the limit), and
the eight exported chips on FIBO stdin [255]'s traces (a 2^20-row Cpu trace).

  python scripts/machine_check_time.py [--out FILE] [--runs 10]"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zkvm-brainfuck_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def guest_trace(prog, chip, prep):
    import numpy as np
    from bfz import _lib
    L = _lib.lib()
    buf, n = _lib.u8buf(bytes([255]))
    p, h, w = ctypes.POINTER(ctypes.c_uint32)(), ctypes.c_size_t(), ctypes.c_size_t()
    _lib.check(L.bfz_trace(prog.encode(), buf, n, chip, prep, ctypes.byref(p), ctypes.byref(h),
                           ctypes.byref(w)))
    a = np.ctypeslib.as_array(p, shape=(h.value * w.value,)).copy().reshape(h.value, w.value)
    L.bfz_free(p)
    return a


def senders_machine(count, rows):
    """`count` mulgate senders of `rows` rows (12 real rows each, the same keys) and the 16-row
    table that receives them."""
    import numpy as np
    from bfz import sdk
    P = 0x7F000001

    def mont(x):
        return ((np.asarray(x, dtype=np.uint64) << 32) % P).astype(np.uint32)

    ab = sdk.AirBuilder(4)
    a, b, c, s = (ab.local(i) for i in range(4))
    ab.assert_zero(s * (s - 1))
    ab.assert_zero(s * (c + -(a * b)))
    lb = sdk.LookupBuilder(4)
    lb.send(3, [lb.main(0), lb.main(1)], lb.main(3))
    tb = sdk.LookupBuilder(2, 1)
    tb.receive(3, [tb.prep(0), tb.main(1)], tb.main(0))
    air, lk, tlk = ab.build(), lb.program(), tb.program()
    real = [(k + 2, k + 3, (k + 2) * (k + 3), 1) for k in range(12)]
    sender = mont(real + [(0, 0, 0, 0)] * (rows - len(real)))
    keys = [(x, y) for x, y, _, _ in real] + [(100 + k, 0) for k in range(4)]
    prep, main = mont([[x] for x, _ in keys]), mont([[0, y] for _, y in keys])
    main[:, 0] = sdk.lookups_multiplicities(tlk, main, prep, 0, [lk] * count, [sender] * count,
                                            [None] * count).mult
    names = [f"c{i:02d}" for i in range(count)]
    m = sdk.Machine([(n, air, lk, None) for n in names] + [("table", None, tlk, prep)])
    return m, dict({n: sender for n in names}, table=main)


def compare(m, traces, runs):
    from air_program_time import spread
    from bfz import sdk
    items = [(m.names.index(n.encode()), n, t) for n, t in traces.items()]

    def loop():  # what Machine.prove(check=True) runs
        for i, _, t in items:
            air, lk = m.programs[i]
            prep = m._check_preps.get(i)
            perm, cs = sdk.lookups_perm_trace(lk, t, prep, sdk._CHECK_ALPHA, sdk._CHECK_BETA)
            sdk.chip_check(air, lk, t, prep, perm, sdk._CHECK_ALPHA, sdk._CHECK_BETA, cs)

    perms = {}
    for i, n, t in items:
        perms[n] = sdk.lookups_perm_trace(m.programs[i][1], t, m._check_preps.get(i), sdk._CHECK_ALPHA,
                                          sdk._CHECK_BETA)

    def checks_only():  # per chip: upload, one k_check_chip_prog launch
        for i, n, t in items:
            air, lk = m.programs[i]
            sdk.chip_check(air, lk, t, m._check_preps.get(i), perms[n][0], sdk._CHECK_ALPHA,
                           sdk._CHECK_BETA, perms[n][1])

    forms = {"Machine.check": lambda: m.check(traces), "prove_check_loop": loop,
             "chip_check_per_chip_given_perm": checks_only}
    assert m.check(traces).ok
    ms = {k: [] for k in forms}
    for r in range(-2, runs):  # two warm-up rounds, then alternating
        for k, f in forms.items():
            t0 = time.perf_counter()
            f()
            if r >= 0:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    out = {k: spread(v) for k, v in ms.items()}
    out["check_ahead_of_loop_beyond_overlap"] = out["Machine.check"]["max"] < out["prove_check_loop"]["min"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=10)
    a = ap.parse_args()
    from bfz import _lib, guests, sdk
    _lib.init(0)
    res = {"timer": "time.perf_counter around whole calls (each call ends synchronized), ms; "
                    "forms alternate after two warm-up rounds"}
    m, traces = senders_machine(31, 1024)  # 31 + the table: the 32-chip limit
    res["31_senders_2^10_and_table"] = compare(m, traces, a.runs)
    del m, traces
    mains = {c: guest_trace(guests.FIBO, c, 0) for c in range(8)}
    chips = [(name, None if c in (1, 4, 5) else sdk.air_export(c), sdk.lookups_export(c),
              guest_trace(guests.FIBO, c, 1) if c in (1, 5) else None)
             for c, name in enumerate(sdk.CHIPS)]
    m = sdk.Machine(chips)
    traces = {sdk.CHIPS[c]: t for c, t in mains.items()}
    res["exported_chips_FIBO"] = {"heights": {k: int(v.shape[0]) for k, v in traces.items()},
                                  **compare(m, traces, max(3, a.runs // 2))}
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
