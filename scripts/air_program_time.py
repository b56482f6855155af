#!/usr/bin/env python3
"""Constraint programs (bfz_air_prove / bfz_air_check on a chip's exported AIR) against the
compiled chips (bfz_uni_prove / bfz_uni_check) on the headline record's traces: median (min-max)
wall time of 6 warm calls each, 84 queries (profiles/r11/air_program.json).

  python scripts/air_program_time.py [--out FILE] [--runs 6]
  python scripts/air_program_time.py --pkg PARENT/zkvm-brainfuck_amd --out parent.json
      # the same bfz_uni_* calls from another checkout's build (the parent commit), same box
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
      python scripts/air_program_time.py --workload   # k_quotient_prog beside k_quotient_air
  python scripts/air_program_time.py --kernels DIR/run_kernel_trace.csv --out kernels.json
  python scripts/air_program_time.py --merge new.json parent.json kernels.json --out FILE

The traces are FIBO_X4 stdin [255]'s Cpu (2^22 x 31) and Jump (2^19 x 45), generated on the host."""
import argparse
import csv
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHIPS = ((0, "Cpu"), (3, "Jump"))


def trace(chip):
    import numpy as np
    from bfz import _lib, guests
    L = _lib.lib()
    buf, n = _lib.u8buf(bytes([255]))
    p, h, w = ctypes.POINTER(ctypes.c_uint32)(), ctypes.c_size_t(), ctypes.c_size_t()
    _lib.check(L.bfz_trace(guests.FIBO_X4.encode(), buf, n, chip, 0, ctypes.byref(p), ctypes.byref(h),
                           ctypes.byref(w)))
    a = np.ctypeslib.as_array(p, shape=(h.value * w.value,)).copy().reshape(h.value, w.value)
    L.bfz_free(p)
    return a


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
            "runs": len(v)}


def warm_calls(f, runs):
    for _ in range(3):  # warm-up: tables, the lane's pool (a new buffer shape settles in the pool)
        f()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        f()
        out.append((time.perf_counter() - t0) * 1e3)
    return spread(out)


def timings(runs):
    from bfz import sdk
    programs = hasattr(sdk, "air_prove")  # a parent checkout has the compiled chips only
    out = {"program": "FIBO_X4", "stdin": [255], "queries": 84, "chips": {}}
    for chip, name in CHIPS:
        t = trace(chip)
        c = {"height": int(t.shape[0]), "width": int(t.shape[1])}
        c["uni_prove_ms"] = warm_calls(lambda: sdk.uni_stark_prove(chip, t), runs)
        c["uni_check_ms"] = warm_calls(lambda: sdk.uni_stark_check(chip, t, on_device=True), runs)
        if programs:
            prog = sdk.air_export(chip)
            assert sdk.air_prove(prog, t)[8:] == sdk.uni_stark_prove(chip, t)[8:]
            assert sdk.air_check(prog, t, on_device=True).failing_rows == 0
            info = sdk.air_info(prog)
            c["program"] = {"bytes": len(prog), "nodes": info.num_nodes,
                            "constraints": info.num_constraints, "instructions": info.instructions,
                            "live_values": info.live_values}
            c["air_prove_ms"] = warm_calls(lambda: sdk.air_prove(prog, t), runs)
            c["air_check_ms"] = warm_calls(lambda: sdk.air_check(prog, t, on_device=True), runs)
            c["prove_ratio"] = round(c["air_prove_ms"]["median"] / c["uni_prove_ms"]["median"], 3)
            c["check_ratio"] = round(c["air_check_ms"]["median"] / c["uni_check_ms"]["median"], 3)
        out["chips"][name] = c
    return out


def workload():
    from bfz import sdk
    for chip, _ in CHIPS:
        t = trace(chip)
        prog = sdk.air_export(chip)
        for _ in range(4):
            sdk.uni_stark_prove(chip, t)
            sdk.air_prove(prog, t)


def kernels(path):
    """Per-launch times: the launches alternate Cpu x 8 then Jump x 8 for each kernel family; the
    chip of a k_quotient_prog launch is known from its grid (the trace's height)."""
    rows = {}
    for r in csv.DictReader(open(path)):
        nm = r["Kernel_Name"]
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if "k_quotient_prog" in nm:
            grid = int(r.get("Grid_Size") or r.get("Grid_Size_X") or 0)
            rows.setdefault(f"k_quotient_prog<1> grid {grid}", []).append(us)
        elif "k_quotient_air<0, 1>" in nm or "k_quotient_air<3, 1>" in nm:
            rows.setdefault("k_quotient_air<0, 1>" if "<0, 1>" in nm else "k_quotient_air<3, 1>", []).append(us)
    return {k: {"launch_us": [round(x, 1) for x in v], "median_us": round(statistics.median(v), 1),
                "min_us": round(min(v), 1), "max_us": round(max(v), 1)} for k, v in rows.items()}


def merge(new_path, parent_path, kernels_path):
    new, parent = json.load(open(new_path)), json.load(open(parent_path))
    new["parent"] = {"note": "bfz_uni_prove / bfz_uni_check of the parent commit's build, same box, "
                             "same session", "chips": parent["chips"]}
    ok = True
    for name, c in new["chips"].items():
        for key in ("uni_prove_ms", "uni_check_ms"):
            p = parent["chips"][name][key]
            inside = p["min"] <= c[key]["median"] <= p["max"]
            c[key + "_within_parent_spread"] = inside
            ok = ok and (inside or c[key]["median"] < p["min"])
    new["uni_calls_not_slower_than_parent"] = ok
    if kernels_path:
        new["kernels"] = json.load(open(kernels_path))
    return new


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "zkvm-brainfuck_amd"))
    ap.add_argument("--workload", action="store_true")
    ap.add_argument("--kernels", metavar="KERNEL_TRACE_CSV")
    ap.add_argument("--merge", nargs="+", metavar="JSON")
    a = ap.parse_args()
    if a.kernels:
        res = kernels(a.kernels)
    elif a.merge:
        res = merge(a.merge[0], a.merge[1], a.merge[2] if len(a.merge) > 2 else None)
    else:
        sys.path.insert(0, a.pkg)
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
