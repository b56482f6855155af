#!/usr/bin/env python3
"""Merkle leaf and layer kernels in their new forms (profiles/r18/merkle_wide.json), single launches
bracketed by HIP events on the same generated device matrices, alternating after one warm-up of
each (bfz_merkle_time; the library compares the two forms' digests):

  lane-mode leaves (k_hash_leaves_lanes) against one thread per row (k_hash_leaves) at the three
  short-tree shapes of DESIGN.md's routing rule;
  the column-table form against the kernel-argument form of k_hash_leaves and k_compress at a
  16-segment list, the longest both can take.

Then the whole Machine.prove call (host wall clock after warm-up) of two machines that the commit
refused before: two senders at each height 4 .. 256 (tests/test_merkle_wide_gpu.py), and 8 small
chips at each of three neighbouring heights.

  python scripts/merkle_wide_time.py [--out FILE] [--runs 20]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("zkvm-brainfuck_amd", "scripts", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
            "runs": len(v)}


def pair(rows, widths, kind_a, kind_b, runs):
    from bfz import _lib
    ws = (ctypes.c_int * len(widths))(*widths)
    a, b = (ctypes.c_float * runs)(), (ctypes.c_float * runs)()
    _lib.check(_lib.lib().bfz_merkle_time(rows, ws, len(widths), kind_a, kind_b, runs, a, b))
    return spread(list(a)), spread(list(b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    from air_program_time import warm_calls
    from machine_prove_time import small_chip
    from bfz import _lib, sdk
    _lib.init(0)
    res = {"timer": "hipEventElapsedTime around one launch, the two kernels alternating on the same "
                    "device matrices after one warm-up of each; their digests are compared",
           "lane_leaves": {}, "table_form": {}}
    for name, rows, widths in (("2^11x8", 1 << 11, [8]), ("2^11x544_in_8", 1 << 11, [68] * 8),
                               ("2^14x31", 1 << 14, [31]), ("2^11x31", 1 << 11, [31]),
                               ("2^14x8", 1 << 14, [8]), ("2^11x9", 1 << 11, [9]), ("2^14x9", 1 << 14, [9]),
                               ("2^11x16", 1 << 11, [16]), ("2^14x16", 1 << 14, [16]),
                               ("2^11x17", 1 << 11, [17]), ("2^14x17", 1 << 14, [17]),
                               ("2^11x24", 1 << 11, [24]), ("2^14x24", 1 << 14, [24]),
                               ("2^11x64", 1 << 11, [64]), ("2^14x64", 1 << 14, [64]),
                               ("2^11x128", 1 << 11, [128]), ("2^14x128", 1 << 14, [128]),
                               ("2^11x256", 1 << 11, [256]), ("2^14x256", 1 << 14, [256]),
                               ("2^14x544_in_8", 1 << 14, [68] * 8), ("2^6x544_in_8", 1 << 6, [68] * 8)):
        th, ln = pair(rows, widths, 0, 2, a.runs)
        res["lane_leaves"][name] = {"k_hash_leaves_ms": th, "k_hash_leaves_lanes_ms": ln,
                                    "lanes_at_or_below_threads": ln["max"] <= th["max"] and ln["min"] <= th["min"]}
    for name, rows, kind in (("k_hash_leaves_2^16x16_of_3", 1 << 16, 0), ("k_compress_2^15x16_of_3", 1 << 15, 4),
                             ("k_hash_leaves_lanes_2^11x16_of_3", 1 << 11, 2)):
        arg, tab = pair(rows, [3] * 16, kind, kind + 1, a.runs)
        res["table_form"][name] = {"kernel_arguments_ms": arg, "column_table_ms": tab,
                                   "ranges_overlap": tab["min"] <= arg["max"] and arg["min"] <= tab["max"]}
    sdk.set_num_queries(0)
    from test_merkle_wide_gpu import two_per_height_machine
    m, traces = two_per_height_machine()
    res["whole_prove_ms"] = {"two_senders_per_height_4..256": warm_calls(lambda: m.prove(traces, m.observe()), 5)}
    air, lk = small_chip()
    rng = np.random.default_rng(18)
    names = [f"c{h}_{i}" for h in (256, 512, 1024) for i in range(8)]
    t = {nm: ((rng.integers(0, 0x7F000001, size=(int(nm[1:].split("_")[0]), 4)).astype(np.uint64) << 32)
              % 0x7F000001).astype(np.uint32) for nm in names}
    m24 = sdk.Machine([(nm, air, lk, None) for nm in names])
    res["whole_prove_ms"]["8_chips_at_each_of_2^8_2^9_2^10"] = warm_calls(lambda: m24.prove(t, m24.observe()), 5)
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
