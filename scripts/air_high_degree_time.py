#!/usr/bin/env python3
"""bfz_air_prove of one AIR family at log quotient degree 1, 2 and 3 (2, 4 and 8 quotient chunks)
on the same trace shape: wall time and the stage times of bfz_timings (HIP events on the proof's
stream), ranges over repeated runs that alternate the three degrees, 84 queries
(profiles/r19/air_high_degree.json).

  python scripts/air_high_degree_time.py [--out FILE] [--runs 5]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
      python scripts/air_high_degree_time.py --workload      # the quotient kernels alone
  python scripts/air_high_degree_time.py --kernels DIR/run_kernel_trace.csv --out kernels.json
  python scripts/air_high_degree_time.py --merge new.json kernels.json --out FILE

The AIR: for every column c, next((c + 1) mod w) - local(c)^k with k = 3, 4, 9 -- w constraints
that read every column at both rows.  The traces are seeded random words (a trace that violates the
AIR proves all the same): a tall narrow 2^21 x 2 (the tallest 8 chunks allow) and a Cpu-like
2^20 x 31."""
import argparse
import csv
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("tall-narrow", 21, 2), ("cpu-like", 20, 31))
POWERS = ((1, 3), (2, 4), (3, 9))  # (log quotient degree, k)
STAGES = ("main_commit_ms", "quotient_ms", "open_ms", "fri_ms", "total_ms")
P = 0x7F000001


def program(width, k):
    from bfz import sdk
    ab = sdk.AirBuilder(width)
    for c in range(width):
        x = p = ab.local(c)
        for _ in range(k - 1):
            p = p * x
        ab.assert_zero(ab.next((c + 1) % width) - p)
    return ab.build()


def random_trace(log_h, width):
    import numpy as np
    rng = np.random.default_rng([log_h, width])
    return rng.integers(0, P, size=(1 << log_h, width), dtype=np.uint32)  # words < p


def prove(prog, trace):
    """One bfz_air_prove: (wall ms, the stage times)."""
    from bfz import _lib, sdk
    L = _lib.lib()
    ch, tm = sdk.Challenger(), _lib.Timings()
    ptr, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t()
    pbuf, pn = _lib.u8buf(prog)
    t0 = time.perf_counter()
    _lib.check(L.bfz_air_prove(pbuf, pn, trace.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                               trace.shape[0], trace.shape[1], ctypes.byref(ch), ctypes.byref(ptr),
                               ctypes.byref(n), ctypes.byref(tm)))
    wall = (time.perf_counter() - t0) * 1e3
    L.bfz_free(ptr)
    return wall, {s: getattr(tm, s) for s in STAGES}


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
            "runs": len(v)}


def timings(runs):
    from bfz import sdk
    sdk.set_air_max_degree(9)
    out = {"queries": 84, "shapes": {}}
    for name, log_h, width in SHAPES:
        t = random_trace(log_h, width)
        progs = {lqd: program(width, k) for lqd, k in POWERS}
        for lqd in progs:
            assert sdk.air_info(progs[lqd]).log_quotient_degree == lqd
        samples = {lqd: {"wall_ms": [], **{s: [] for s in STAGES}} for lqd in progs}
        for rep in range(2 + runs):  # two warm-up rounds: tables, the lane's pool
            for lqd in progs:  # alternating: every round takes the three degrees in turn
                wall, st = prove(progs[lqd], t)
                if rep >= 2:
                    samples[lqd]["wall_ms"].append(wall)
                    for s in STAGES:
                        samples[lqd][s].append(st[s])
        shape = {"height": 1 << log_h, "width": width, "lqd": {}}
        for lqd, k in POWERS:
            info = sdk.air_info(progs[lqd])
            c = {"power": k, "chunks": 1 << lqd, "instructions": info.instructions}
            c.update({key: spread(v) for key, v in samples[lqd].items()})
            c["rest_ms"] = spread([a - b for a, b in zip(samples[lqd]["total_ms"],
                                                         samples[lqd]["quotient_ms"])])
            shape["lqd"][str(lqd)] = c
        out["shapes"][name] = shape
    return out


def workload():
    from bfz import sdk
    sdk.set_air_max_degree(9)
    for _, log_h, width in SHAPES:
        t = random_trace(log_h, width)
        for _ in range(4):
            for _, k in POWERS:
                prove(program(width, k), t)


def kernels(path):
    """Per-launch times of the two quotient kernels, keyed by name and grid (the LDE's height)."""
    rows = {}
    for r in csv.DictReader(open(path)):
        nm = r["Kernel_Name"]
        if "k_quotient_prog" not in nm:
            continue
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        grid = int(r.get("Grid_Size") or r.get("Grid_Size_X") or 0)
        kind = "k_quotient_prog_coset" if "coset" in nm else "k_quotient_prog<1>"
        rows.setdefault(f"{kind} grid {grid}", []).append(us)
    return {k: {"launches": len(v), "median_us": round(statistics.median(v), 1),
                "min_us": round(min(v), 1), "max_us": round(max(v), 1)} for k, v in rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--workload", action="store_true")
    ap.add_argument("--kernels", metavar="KERNEL_TRACE_CSV")
    ap.add_argument("--merge", nargs=2, metavar="JSON")
    a = ap.parse_args()
    if a.kernels:
        res = kernels(a.kernels)
    elif a.merge:
        res = json.load(open(a.merge[0]))
        res["kernels"] = json.load(open(a.merge[1]))
    else:
        sys.path.insert(0, os.path.join(ROOT, "zkvm-brainfuck_amd"))
        from bfz import _lib
        _lib.init(0)
        if a.workload:
            workload()
            return
        res = timings(a.runs)
    text = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
