#!/usr/bin/env python3
"""Machine proofs whose tall chip has AIR degree 3, 4 and 9 (2, 4 and 8 quotient chunks):
Machine.prove (host wall clock around the call, which ends synchronized) and the quotient stage
(bfz_machine_time: HIP events on the proof's stream around slab 0 and, from degree 4, the slab
LDEs, k_quotient_machine_coset and the chunk LDEs), the three machines alternating, median and
range of `--runs` after two warm-up rounds.  Then the segmented slab launches against the per-chip
loop (both inside bfz_machine_time's quotient figures) on a machine of 8 small chips of degree 4
to 9 (profiles/r21/machine_high_degree.json).

  python scripts/machine_high_degree_time.py [--out FILE] [--runs 5] [--log-rows 20]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zkvm-brainfuck_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
P = 0x7F000001


def mont(x):
    import numpy as np
    return ((np.asarray(x, dtype=np.uint64) << 32) % P).astype(np.uint32)


def pow_chip(k):
    """main (x, y, s): y = x^k on every row, s boolean, (x, y) sent under s."""
    from bfz import sdk
    ab = sdk.AirBuilder(3)
    x, y, s = (ab.local(i) for i in range(3))
    xk = x
    for _ in range(k - 1):
        xk = xk * x
    ab.assert_zero(y - xk)
    ab.assert_zero(s * (s - 1))
    lb = sdk.LookupBuilder(3)
    lb.send(3, [lb.main(0), lb.main(1)], lb.main(2))
    return ab.build(), lb.program()


def pow_trace(k, n, seed):
    """n valid rows; the first two are sent."""
    import numpy as np
    x = np.random.default_rng([k, n, seed]).integers(2, P, n).astype(np.uint64)
    y = x.copy()
    for _ in range(k - 1):
        y = y * x % P
    s = np.zeros(n, dtype=np.uint64)
    s[:2] = 1
    return np.stack([x, y, s], axis=1)


def machine(chips):
    """chips: [(name, degree, rows)].  The machine with the 32-row table of every sent key."""
    import numpy as np
    from bfz import sdk
    tb = sdk.LookupBuilder(2, 1)
    tb.receive(3, [tb.prep(0), tb.main(1)], tb.main(0))
    tlk = tb.program()
    progs = {name: pow_chip(k) for name, k, _ in chips}
    canon = {name: pow_trace(k, n, i) for i, (name, k, n) in enumerate(chips)}
    keys = [(int(t[r, 0]), int(t[r, 1])) for t in canon.values() for r in range(2)]
    keys += [(k, 0) for k in range(2, 34)][:32 - len(keys)]
    traces = {name: mont(t) for name, t in canon.items()}
    prep, main = mont([[a] for a, _ in keys]), mont([[0, b] for _, b in keys])
    main[:, 0] = sdk.lookups_multiplicities(tlk, main, prep, 0, [progs[n][1] for n in traces],
                                            list(traces.values()), [None] * len(traces)).mult
    m = sdk.Machine([(n, *progs[n], None) for n in traces] + [("table", None, tlk, prep)])
    return m, dict(traces, table=main)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--log-rows", type=int, default=20)
    a = ap.parse_args()
    from air_program_time import spread
    from bfz import _lib, sdk
    _lib.init(0)
    sdk.set_chip_max_degree(9)
    res = {"timer": "prove: time.perf_counter around Machine.prove, ms; quotient: bfz_machine_time's "
                    "HIP events (segmented form), ms; machines alternate after two warm-up rounds",
           "tall_rows": 1 << a.log_rows}
    tall = {f"degree_{k}": machine([("tall", k, 1 << a.log_rows)]) for k in (3, 4, 9)}
    prove = {k: [] for k in tall}
    quot = {k: [] for k in tall}
    for r in range(-2, a.runs):
        for k, (m, traces) in tall.items():
            t0 = time.perf_counter()
            proof = m.prove(traces, m.observe())
            dt = (time.perf_counter() - t0) * 1e3
            q = m.time(traces, runs=1)["quotient"][0][0]
            if r < 0:
                assert m.verify(proof, m.observe()).ok
            else:
                prove[k].append(dt)
                quot[k].append(q)
    res["tall"] = {k: {"prove_ms": spread(prove[k]), "quotient_ms": spread(quot[k])} for k in tall}
    del tall
    m, traces = machine([(f"c{i}", 4 + i % 6, 16 << i) for i in range(8)])  # degrees 4..9, 2^4..2^11 rows
    seg, loop = m.time(traces, runs=4 * a.runs)["quotient"]
    res["8_small_chips"] = {"quotient_segmented_ms": spread(seg), "quotient_per_chip_loop_ms": spread(loop)}
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
