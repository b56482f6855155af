#!/usr/bin/env python3
"""A/B of the host verifier against the device verifier on the headline proof.

Builds bench.py's workload proof (FIBO_X4, stdin [255]: a 2^22-row Cpu trace, 84 queries, 23 FRI
rounds) on the GPU, warms both paths, then times bfz_verify_batch with on_device = 0 and 1,
alternating them in one process: wall clock around the whole call (host stages, packing, upload,
kernels and the final synchronise included).  One proof first, then a batch of --batch copies.
The host verifier is code this comparison does not change, so its time is the baseline.

    python scripts/verify_ab.py [--reps 12] [--batch 8] [--out profiles/r07/verify_ab.json]

Needs a GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zkvm-brainfuck_amd"))

from bfz import _lib, guests, sdk  # noqa: E402


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3),
            "max_ms": round(max(ms), 3), "runs": len(ms)}


def ab(client, proofs, vk, reps):
    times = {False: [], True: []}
    for _ in range(reps):
        for dev in (False, True):
            t = time.perf_counter()
            out = client.verify_batch(proofs, vk, on_device=dev)
            times[dev].append((time.perf_counter() - t) * 1e3)
            if not all(o.ok for o in out):
                raise SystemExit(f"verify_ab: on_device={dev} rejected the proof: {out[0].why}")
    host, dev = stats(times[False]), stats(times[True])
    spread = max(host["max_ms"] - host["min_ms"], dev["max_ms"] - dev["min_ms"])
    return {"host": host, "device": dev, "spread_ms": round(spread, 3),
            "host_over_device": round(host["median_ms"] / dev["median_ms"], 2),
            "device_faster_by_more_than_spread": host["median_ms"] - dev["median_ms"] > spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "verify_ab.json"))
    a = ap.parse_args()
    if a.reps < 10:
        raise SystemExit("verify_ab: at least 10 repetitions per path")
    _lib.init(0)
    client = sdk.ProverClient()
    pk, vk = client.setup(guests.FIBO_X4)
    proof = client.prove(pk, [255]).run().proof
    tampered = bytearray(proof)
    tampered[len(tampered) // 2] ^= 1
    for dev in (False, True):  # warm both paths (code objects, pool buffers, page faults)
        for _ in range(2):
            got = client.verify_batch([proof, bytes(tampered)], vk, on_device=dev)
            if [o.ok for o in got] != [True, False]:
                raise SystemExit(f"verify_ab: warm-up outcomes wrong on_device={dev}: {got}")
    import ctypes
    name = ctypes.create_string_buffer(256)
    _lib.check(_lib.lib().bfz_device_name(name, 256))
    res = {
        "what": "bfz_verify_batch wall clock, host verifier (on_device=0, one thread; unchanged "
                "code, i.e. the parent commit's figure) against the device query phase "
                "(on_device=1), alternated in one process",
        "workload": "FIBO_X4 stdin [255]: 2^22-row Cpu trace, 84 queries, 23 FRI rounds",
        "proof_bytes": len(proof),
        "device": name.value.decode(),
        "one_proof": ab(client, [proof], vk, a.reps),
        "batch": dict(ab(client, [proof] * a.batch, vk, a.reps), proofs=a.batch),
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
