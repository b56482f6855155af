#!/usr/bin/env python3
"""The segmented chip kernels against the per-chip launches they replace
(profiles/r16/machine_prove.json): k_perm_rows_machine / k_quotient_machine, one launch over every
chip of a machine, against the loop of k_perm_rows_prog<1> / k_quotient_chip_prog launches, on the
same device inputs: single launches (or loops) bracketed by HIP events (bfz_machine_time),
alternating after one warm-up of each, whose words the library compares.  Two machines: the eight
exported chips on FIBO_X4 stdin [255]'s traces (one 2^22 chip among small ones), and 32 copies of
a small custom chip at 2^10 rows.  For the first, the whole Machine.prove call beside
bfz_prove_traces on the same traces (host wall clock, after warm-up).

  python scripts/machine_prove_time.py [--out FILE] [--runs 20]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zkvm-brainfuck_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def prep_trace(chip):
    import numpy as np
    from bfz import _lib, guests
    L = _lib.lib()
    buf, n = _lib.u8buf(bytes([255]))
    p, h, w = ctypes.POINTER(ctypes.c_uint32)(), ctypes.c_size_t(), ctypes.c_size_t()
    _lib.check(L.bfz_trace(guests.FIBO_X4.encode(), buf, n, chip, 1, ctypes.byref(p), ctypes.byref(h),
                           ctypes.byref(w)))
    a = np.ctypeslib.as_array(p, shape=(h.value * w.value,)).copy().reshape(h.value, w.value)
    L.bfz_free(p)
    return a


def small_chip():
    """width 4 (a, b, c, s): s boolean, s (c - a b) = 0; one send and one receive."""
    from bfz import sdk
    ab = sdk.AirBuilder(4)
    a, b, c, s = (ab.local(i) for i in range(4))
    ab.assert_zero(s * (s - 1))
    ab.assert_zero(s * (c + -(a * b)))
    lb = sdk.LookupBuilder(4)
    lb.send(3, [lb.main(0), lb.main(1)], lb.main(3))
    lb.receive(3, [lb.main(2)], lb.main(3))
    return ab.build(), lb.program()


def forms(t):
    from air_program_time import spread
    out = {}
    for step, (seg, loop) in t.items():
        a, b = spread(seg), spread(loop)
        out[step] = {"segmented_ms": a, "per_chip_loop_ms": b,
                     "segmented_ahead_beyond_overlap": a["max"] < b["min"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    from air_program_time import trace, warm_calls
    from bfz import _lib, guests, sdk
    _lib.init(0)
    res = {"timer": "hipEventElapsedTime around one segmented launch / one loop of per-chip "
                    "launches, alternating; the two forms' words are compared in the warm-up round"}
    mains = {c: trace(c) for c in range(8)}
    chips = [(name, None if c in (1, 4, 5) else sdk.air_export(c), sdk.lookups_export(c),
              prep_trace(c) if c in (1, 5) else None) for c, name in enumerate(sdk.CHIPS)]
    m = sdk.Machine(chips)
    traces = {sdk.CHIPS[c]: t for c, t in mains.items()}
    res["exported_chips_FIBO_X4"] = {"heights": {k: int(v.shape[0]) for k, v in traces.items()},
                                     **forms(m.time(traces, a.runs))}
    core = sdk.CoreProver()
    pk, _ = sdk.ProverClient().setup(guests.FIBO_X4)
    tr = [(c, sdk.CHIPS[c], t) for c, t in mains.items()]
    res["whole_prove_ms"] = {
        "Machine.prove": warm_calls(lambda: m.prove(traces, m.observe()), 5),
        "bfz_prove_traces": warm_calls(lambda: core.prove(pk, tr), 5)}
    del m, mains, traces, tr
    air, lk = small_chip()
    rng = np.random.default_rng(16)
    t = ((rng.integers(0, 0x7F000001, size=(1024, 4)).astype(np.uint64) << 32) % 0x7F000001).astype(np.uint32)
    m32 = sdk.Machine([(f"c{i:02d}", air, lk, None) for i in range(32)])
    res["32_small_chips_2^10"] = forms(m32.time({f"c{i:02d}": t for i in range(32)}, a.runs))
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
