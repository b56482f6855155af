#!/usr/bin/env python3
"""The device verifier of machine proofs against the host verifier
(profiles/r17/machine_verify.json): bfz_machine_verify_batch with on_device = 0 and 1 on the same
bytes, whole-call wall clock, alternating after one warm-up of each, median (min-max) of `runs`.
  1. the eight exported chips on FIBO_X4 stdin [255], 84 queries, 1 and 8 proofs; beside it
     bfz_verify_batch(on_device=1) on the same bytes (a machine of the exported chips writes the
     built-in proof bytes)
  2. a wide custom machine proved on the device: 12 lookup-only chips of main width 64 with 32
     interactions each (68-word permutation rows), one per height from 2^16 rows down to 2^5
  3. for both: HIP-event times of the device pass's launches (bfz_machine_verify_time), and the
     host side alone of each device path (bfz_set_fault_injection bit 1: stages and packing with a
     stand-in for the kernels), so that whole call - host side = upload, kernels and synchronise

  python scripts/machine_verify_time.py [--out FILE] [--runs 20] [--bench FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zkvm-brainfuck_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def alternate(calls, runs):
    """{name: spread of `runs` wall-clock ms}, the calls taken in turn after one warm-up of each."""
    from air_program_time import spread
    for f in calls.values():
        f()
    ms = {k: [] for k in calls}
    for _ in range(runs):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: spread(v) for k, v in ms.items()}


def host_side(f):
    """f under the stand-in for the kernels: the device path's host side alone."""
    from bfz import _lib

    def run():
        _lib.check(_lib.lib().bfz_set_fault_injection(2))
        try:
            f()
        finally:
            _lib.check(_lib.lib().bfz_set_fault_injection(0))
    return run


def kernel_ms(times):
    from air_program_time import spread
    return {k: spread(v) for k, v in times.items()}


def accepted(outs):
    assert all(o.ok for o in outs), [o.why for o in outs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--bench", help="JSON of the alternating bench.py runs, copied into the result")
    a = ap.parse_args()
    import numpy as np
    from air_program_time import trace
    from machine_prove_time import prep_trace
    from bfz import _lib, guests, sdk
    _lib.init(0)
    res = {"timer": "time.perf_counter around the whole verify_batch call, host and device "
                    "alternating after one warm-up of each; ms"}
    mains = {c: trace(c) for c in range(8)}
    m = sdk.Machine([(name, None if c in (1, 4, 5) else sdk.air_export(c), sdk.lookups_export(c),
                      prep_trace(c) if c in (1, 5) else None) for c, name in enumerate(sdk.CHIPS)])
    proof = m.prove({sdk.CHIPS[c]: t for c, t in mains.items()}, m.observe())
    client = sdk.ProverClient()
    _, vk = client.setup(guests.FIBO_X4)
    for n in (1, 8):
        res[f"exported_chips_FIBO_X4_{n}_proofs"] = alternate({
            "machine_host_ms": lambda: accepted(m.verify_batch([proof] * n, on_device=False)),
            "machine_device_ms": lambda: accepted(m.verify_batch([proof] * n, on_device=True)),
            "builtin_device_ms": lambda: accepted(client.verify_batch([proof] * n, vk, on_device=True)),
            "machine_device_host_side_ms": host_side(lambda: m.verify_batch([proof] * n, on_device=True)),
            "builtin_device_host_side_ms": host_side(lambda: client.verify_batch([proof] * n, vk, on_device=True)),
        }, a.runs)
        res[f"exported_chips_FIBO_X4_{n}_proofs"]["machine_kernels_ms"] = kernel_ms(
            m.verify_time([proof] * n, a.runs))
    del m, mains
    b = sdk.LookupBuilder(64)
    for i in range(16):
        b.send(3, [b.main(1 + i)], b.main(0))
        b.receive(3, [b.main(17 + i)], b.main(0))
    lk = b.program()
    names = [f"w{i:02d}" for i in range(12)]
    rng = np.random.default_rng(17)
    traces = {}
    for i, nm in enumerate(names):
        t = ((rng.integers(0, 0x7F000001, size=(1 << (16 - i), 64)).astype(np.uint64) << 32)
             % 0x7F000001).astype(np.uint32)
        t[:, 0] = 0  # every interaction's multiplicity
        traces[nm] = t
    wide = sdk.Machine([(nm, None, lk, None) for nm in names])
    wproof = wide.prove(traces, wide.observe())
    res["wide_machine_12_chips_2^16_to_2^5"] = {
        "proof_bytes": len(wproof),
        **alternate({"machine_host_ms": lambda: accepted(wide.verify_batch([wproof], on_device=False)),
                     "machine_device_ms": lambda: accepted(wide.verify_batch([wproof], on_device=True)),
                     "machine_device_host_side_ms": host_side(lambda: wide.verify_batch([wproof], on_device=True))},
                    a.runs),
        "machine_kernels_ms": kernel_ms(wide.verify_time([wproof], a.runs))}
    if a.bench:
        res["bench_flagship_ms"] = json.load(open(a.bench))
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
