#!/usr/bin/env python3
"""Times the per-key lookup debugger (bfz_record_debug_interactions, csrc/lookup_debug.hip):

  headline  FIBO_X4 with stdin [255], all kinds: device time, table_bytes and the counters, and
            bfz_record_debug_constraints (without / with the kind table) on the same record;
  headline_no_combine  the same with BFZ_LOOKUP_COMBINE=0 (no per-block LDS table);
  mid       FIBO with stdin [60] (a 2^16..2^18-row Cpu trace): device time, the host path's time
            (bfz_debug_interactions_traces, on_device = 0, over host traces) and the constraint
            checker on the same record.

Without --step it runs each step as a process of its own under `timeout`, one after the other,
stops at the first that fails, and writes profiles/r08/debug_interactions.json (DESIGN.md and
the README quote it).  Every call is warmed once and timed `--reps` times on a host clock around
the call (each call ends in a stream synchronize).

  python scripts/debug_interactions_time.py [--reps 3] [--out profiles/r08/debug_interactions.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zkvm-brainfuck_amd"))
STEPS = {"headline": 420, "headline_no_combine": 420, "mid": 300}  # seconds each step may take


def step(name, reps, device):
    from bfz import _lib, guests, sdk
    prog, stdin = {"headline": (guests.FIBO_X4, bytes([255])),
                   "headline_no_combine": (guests.FIBO_X4, bytes([255])),
                   "mid": (guests.FIBO, bytes([60]))}[name]
    L = _lib.lib()
    _lib.init(device)
    client = sdk.ProverClient(device=device)
    pk, _ = client.setup(prog)
    rec = ctypes.c_void_p()
    cycles = ctypes.c_uint64()
    buf, n = _lib.u8buf(stdin)
    _lib.check(L.bfz_record_new(ctypes.c_void_p(pk.handle), buf, n, ctypes.byref(rec),
                                ctypes.byref(cycles)))

    def interactions():
        rep = _lib.LookupReportC()
        out = (_lib.LookupDiscrepancyC * 16)()
        t0 = time.perf_counter()
        _lib.check(L.bfz_record_debug_interactions(ctypes.c_void_p(pk.handle), rec, 0xFE,
                                                   ctypes.byref(rep), out, 16))
        return (time.perf_counter() - t0) * 1e3, rep

    def constraints(flags):
        ch = _lib.Challenger()
        out = _lib.DebugReportC()
        t0 = time.perf_counter()
        _lib.check(L.bfz_record_debug_constraints(ctypes.c_void_p(pk.handle), rec, ctypes.byref(ch),
                                                  flags, ctypes.byref(out)))
        return (time.perf_counter() - t0) * 1e3, out

    _, rep = interactions()
    _, chk = constraints(1)
    t = {"interactions": [], "constraints": [], "constraints_balance": []}
    for _ in range(reps):
        t["interactions"].append(interactions()[0])
        t["constraints"].append(constraints(0)[0])
        t["constraints_balance"].append(constraints(1)[0])
    L.bfz_record_free(rec)
    res = {
        "step": name, "cycles": cycles.value, "reps": reps,
        "heights": {sdk.CHIPS[chk.chips[i].chip]: chk.chips[i].height for i in range(chk.n_chips)},
        "balanced": bool(rep.balanced), "interactions": rep.interactions,
        "distinct_keys": rep.distinct_keys, "rounds": rep.rounds,
        "tag_collisions": rep.tag_collisions, "table_bytes": rep.table_bytes,
        "device_ms": [round(x, 3) for x in t["interactions"]],
        "debug_constraints_ms": [round(x, 3) for x in t["constraints"]],
        "debug_constraints_balance_ms": [round(x, 3) for x in t["constraints_balance"]],
        "median_ms": {k: round(statistics.median(v), 3) for k, v in t.items()},
    }
    if name == "mid":
        traces = sdk.generate_traces(prog, stdin)
        t0 = time.perf_counter()
        host = sdk.CoreProver().debug_interactions(pk, traces, limit=16, on_device=False)
        res["host_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        res["host_equals_device"] = (
            host.balanced == bool(rep.balanced) and host.interactions == rep.interactions
            and host.distinct_keys == rep.distinct_keys
            and host.chip_distinct == list(rep.chip_distinct))
        res["host_over_device"] = round(res["host_ms"] / res["median_ms"]["interactions"], 2)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "debug_interactions.json"))
    args = ap.parse_args()
    if args.step:
        return step(args.step, args.reps, args.device)
    results = {}
    for name in ("headline", "headline_no_combine", "mid"):  # chained: a failing step ends the run
        # the A/B of the account phase's per-block LDS table (csrc/lookup_debug.hip)
        env = dict(os.environ, BFZ_LOOKUP_COMBINE="0" if name == "headline_no_combine" else "1")
        r = subprocess.run(["timeout", "-k", "10", str(STEPS[name]), sys.executable, __file__,
                            "--step", name, "--reps", str(args.reps), "--device", str(args.device)],
                           capture_output=True, text=True, env=env)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"debug_interactions_time: step {name} ended with status {r.returncode}")
        results[name] = json.loads(r.stdout.strip().splitlines()[-1])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(results, fh, indent=1)
        fh.write("\n")
    print(json.dumps(results), flush=True)


if __name__ == "__main__":
    main()
