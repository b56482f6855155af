#!/usr/bin/env python3
"""The chip-program quotient kernel against the compiled one (profiles/r14/chip_quotient.json):
k_quotient_chip_prog<1> on Cpu's two exported programs against k_quotient<0>, and
k_quotient_chip_prog<0> on Memory's exported interactions against k_quotient<4>, on FIBO_X4 stdin
[255]'s traces (Cpu: 2^22 x 31): single launches bracketed by HIP events
(bfz_chip_quotient_time), alternating after a warm-up launch of each.  The two kernels' outputs
are compared word for word first, on the first 2^16 rows of the trace.

  python scripts/chip_quotient_time.py [--out FILE] [--runs 20]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zkvm-brainfuck_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
CHIPS = {"Cpu": 0, "Memory": 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    from air_program_time import spread, trace
    from bfz import _lib, sdk
    _lib.init(0)
    rng = np.random.default_rng(14)
    p = 0x7F000001
    alpha, beta, qa = ([int(x) for x in rng.integers(0, p, 4)] for _ in range(3))
    res = {"program": "FIBO_X4", "stdin": [255],
           "timer": "hipEventElapsedTime around one launch; launches alternate prog, compiled"}
    ok = True
    for name, chip in CHIPS.items():
        t = trace(chip)
        air = sdk.air_export(chip) if name == "Cpu" else None
        lk = sdk.lookups_export(chip)
        info = sdk.chip_info(air, lk)
        # results must not differ: the programs' quotient against the compiled chip's
        head = t[:min(len(t), 1 << 16)]
        got, cs = sdk.chip_quotient(air, lk, head, None, alpha, beta, qa)
        want, cs_c = sdk.chip_quotient(None, None, head, None, alpha, beta, qa, chip=chip)
        same = bool(np.array_equal(got, want)) and cs == cs_c
        ok = ok and same
        pm, cm = sdk.chip_quotient_time(chip, air, lk, t, None, alpha, beta, qa, a.runs)
        kp, kc = f"k_quotient_chip_prog<{int(air is not None)}>_ms", f"k_quotient<{chip}>_ms"
        res[name] = {"height": int(t.shape[0]), "width": int(t.shape[1]),
                     "air_constraints": info.air_constraints, "num_constraints": info.num_constraints,
                     "interactions": info.n_interactions, "words_equal_compiled": same,
                     kp: spread(pm), kc: spread(cm),
                     "ratio_prog_over_compiled": round(spread(pm)["median"] / spread(cm)["median"], 3)}
        del t, got, want
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    if not ok:
        sys.exit("a program's quotient differs from the compiled chip's")


if __name__ == "__main__":
    main()
