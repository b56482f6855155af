#!/usr/bin/env python3
"""Per-chip uni-STARK proofs (bfz_uni_prove / bfz_uni_verify) on the headline record's traces:
wall time and stage split of the prover, host verifier time (profiles/r09/uni_stark.json).

  python scripts/uni_stark_time.py [--out FILE] [--runs 6]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \
      python scripts/uni_stark_time.py --workload      # k_quotient<0> beside k_quotient_air<0, 1>
  python scripts/uni_stark_time.py --kernels DIR/run_kernel_trace.csv   # per-launch times of both

The traces are FIBO_X4 stdin [255]'s Cpu (2^22 x 31) and Jump chips, generated on the host."""
import argparse
import csv
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zkvm-brainfuck_amd"))


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


def timings(runs):
    from bfz import _lib, sdk
    out = {"program": "FIBO_X4", "stdin": [255], "queries": 84, "chips": {}}
    for chip, name in ((0, "Cpu"), (3, "Jump")):
        t = trace(chip)
        proof = sdk.uni_stark_prove(chip, t)  # warm-up: tables, the lane's pool
        walls, stages, ver = [], [], []
        for _ in range(runs):
            t0 = time.perf_counter()
            again = sdk.uni_stark_prove(chip, t)
            walls.append((time.perf_counter() - t0) * 1e3)
            assert again == proof
        for _ in range(3):
            tm = _lib.Timings()
            sdk.uni_stark_prove(chip, t, timings=tm)
            stages.append({k: round(getattr(tm, k), 3) for k in
                           ("main_commit_ms", "quotient_ms", "open_ms", "fri_ms", "total_ms")})
        for _ in range(runs):
            t0 = time.perf_counter()
            sdk.uni_stark_verify(chip, proof)
            ver.append((time.perf_counter() - t0) * 1e3)
        out["chips"][name] = {
            "height": int(t.shape[0]), "width": int(t.shape[1]), "proof_bytes": len(proof),
            "prove_wall_ms": spread(walls),
            "stage_ms_runs": stages,
            "stage_note": "HIP events on the prover stream; main_commit_ms includes the host-to-device "
                          "copy and transpose of the trace, quotient_ms the chunk LDEs and their commit",
            "verify_host_ms": spread(ver)}
    return out


def workload():
    from bfz import sdk
    from bfz import guests
    t = trace(0)
    client = sdk.ProverClient()
    pk, _ = client.setup(guests.FIBO_X4)
    for _ in range(4):
        client.prove(pk, [255]).run()
        sdk.uni_stark_prove(0, t)


def kernels(path):
    rows = {}
    for r in csv.DictReader(open(path)):
        nm = r["Kernel_Name"]
        if "k_quotient<0>" in nm or "k_quotient_air<0, 1>" in nm:
            key = "k_quotient<0>" if "k_quotient<0>" in nm else "k_quotient_air<0, 1>"
            rows.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"launch_us": [round(x, 1) for x in v], "median_us": round(statistics.median(v), 1),
                "min_us": round(min(v), 1), "max_us": round(max(v), 1)} for k, v in rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--workload", action="store_true")
    ap.add_argument("--kernels", metavar="KERNEL_TRACE_CSV")
    a = ap.parse_args()
    if a.kernels:
        res = kernels(a.kernels)
    else:
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
