#!/usr/bin/env python3
"""Times the per-key lookup debugger of caller-defined chips (bfz_lookups_debug,
csrc/lookup_debug_prog.hip) with the compiled chips' path as the yardstick:

  combine        FIBO_X4 with stdin [255], its eight host traces: the whole of bfz_lookups_debug on
                 the eight exported programs against the whole of bfz_debug_interactions_traces,
                 alternating after one warm-up of each (both calls upload the traces);
  no_combine     the same with BFZ_LOOKUP_COMBINE=0 (no per-block LDS table in either kernel);
  multiplicities bfz_lookups_multiplicities of a 2^18-row table (key = row) from a 2^18-row chip
                 with two sends per row.

Without --step it runs each step as a process of its own under `timeout`, one after the other,
stops at the first that fails, and writes profiles/r15/lookups_debug.json (DESIGN.md and the README
quote it).  Times are host clocks around the calls (each ends in a stream synchronize), in ms.

  python scripts/lookups_debug_time.py [--reps 5] [--out profiles/r15/lookups_debug.json]
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
STEPS = {"combine": 420, "no_combine": 420, "multiplicities": 120}  # seconds each step may take


def spread(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def headline(reps, device):
    import numpy as np
    from bfz import _lib, guests, sdk
    _lib.init(device)
    elf, stdin = guests.FIBO_X4, bytes([255])
    traces = sdk.generate_traces(elf, stdin)
    pk, _ = sdk.ProverClient(device=device).setup(elf)
    progs = [sdk.lookups_export(c) for c, _, _ in traces]
    preps = []
    for (c, _, m), p in zip(traces, progs):
        w = sdk.lookups_info(p).prep_width
        if not w:
            preps.append(None)
            continue
        out, h, ww = ctypes.POINTER(ctypes.c_uint32)(), ctypes.c_size_t(), ctypes.c_size_t()
        buf, n = _lib.u8buf(stdin)
        _lib.check(_lib.lib().bfz_trace(elf.encode(), buf, n, c, 1, ctypes.byref(out), ctypes.byref(h),
                                        ctypes.byref(ww)))
        preps.append(np.ctypeslib.as_array(out, shape=(h.value, ww.value)).copy())
        _lib.lib().bfz_free(out)
    mains = [m for _, _, m in traces]

    def timed(f):
        t0 = time.perf_counter()
        r = f()
        return (time.perf_counter() - t0) * 1e3, r

    prog = lambda: sdk.lookups_debug(progs, mains, preps, limit=16)
    chip = lambda: sdk.CoreProver().debug_interactions(pk, traces, limit=16)
    (_, a), (_, b) = timed(prog), timed(chip)  # warm-up
    t = {"programs": [], "compiled": []}
    for _ in range(reps):
        t["programs"].append(timed(prog)[0])
        t["compiled"].append(timed(chip)[0])
    return {
        "reps": reps, "heights": {name: int(m.shape[0]) for _, name, m in traces},
        "interactions": a.interactions, "distinct_keys": a.distinct_keys, "rounds": a.rounds,
        "same_counts": (a.balanced, a.interactions, a.distinct_keys, a.unbalanced_keys) ==
                       (b.balanced, b.interactions, b.distinct_keys, b.unbalanced_keys),
        "programs_ms": spread(t["programs"]), "compiled_ms": spread(t["compiled"]),
        "ratio": round(statistics.median(t["programs"]) / statistics.median(t["compiled"]), 3),
    }


def multiplicities(reps, device):
    import numpy as np
    from bfz import _lib, sdk
    _lib.init(device)
    n = 1 << 18
    mont = lambda a: ((np.asarray(a, dtype=np.uint64) << np.uint64(32)) % np.uint64(0x7F000001)).astype(np.uint32)
    t, s = sdk.LookupBuilder(2), sdk.LookupBuilder(2)
    t.receive(12, [t.main(0)], t.main(1))
    s.send(12, [s.main(0)], 1)
    s.send(12, [s.main(1)], 1)
    table = mont(np.stack([np.arange(n), np.zeros(n)], axis=1))
    vals = np.random.default_rng(18).integers(0, n, size=(n, 2))
    send = mont(vals)
    ms = []
    for r in range(reps + 1):  # the first call warms up
        t0 = time.perf_counter()
        got = sdk.lookups_multiplicities(t.program(), table, None, 0, [s.program()], [send], [None])
        if r:
            ms.append((time.perf_counter() - t0) * 1e3)
    ok = bool(np.array_equal(got.mult, mont(np.bincount(vals.ravel(), minlength=n))))
    return {"reps": reps, "rows": n, "interactions": got.interactions, "equals_bincount": ok, "ms": spread(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "lookups_debug.json"))
    args = ap.parse_args()
    if args.step:
        f = multiplicities if args.step == "multiplicities" else headline
        print(json.dumps(f(args.reps, args.device)), flush=True)
        return
    results = {}
    for name in ("combine", "no_combine", "multiplicities"):  # chained: a failing step ends the run
        env = dict(os.environ, BFZ_LOOKUP_COMBINE="0" if name == "no_combine" else "1")
        r = subprocess.run(["timeout", "-k", "10", str(STEPS[name]), sys.executable, __file__,
                            "--step", name, "--reps", str(args.reps), "--device", str(args.device)],
                           capture_output=True, text=True, env=env)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"lookups_debug_time: step {name} ended with status {r.returncode}")
        results[name] = json.loads(r.stdout.strip().splitlines()[-1])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(results, fh, indent=1)
        fh.write("\n")
    print(json.dumps(results), flush=True)


if __name__ == "__main__":
    main()
