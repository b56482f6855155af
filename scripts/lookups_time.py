#!/usr/bin/env python3
"""The interaction-program row kernel against the compiled one (profiles/r13/lookups_program.json):
k_perm_rows_prog<1> on the exported Cpu program and k_perm_rows<0> on the same trace, FIBO_X4
stdin [255]'s Cpu (2^22 x 31), single launches bracketed by HIP events (bfz_lookups_time),
alternating after a warm-up launch of each; the two calls' outputs are compared word for word
first.

  python scripts/lookups_time.py [--out FILE] [--runs 20]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zkvm-brainfuck_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
CHIP = 0  # Cpu


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
            "runs": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    from air_program_time import trace
    from bfz import _lib, sdk
    _lib.init(0)
    L = _lib.lib()
    t = trace(CHIP)
    prog = sdk.lookups_export(CHIP)
    info = sdk.lookups_info(prog)
    rng = np.random.default_rng(13)
    p = 0x7F000001
    alpha, beta = ((ctypes.c_uint32 * 4)(*[int(x) for x in rng.integers(0, p, 4)]) for _ in range(2))
    u32p = ctypes.POINTER(ctypes.c_uint32)
    # results must not differ: the program's trace against the compiled chip's, at the timed size
    out, w, cs = u32p(), ctypes.c_size_t(), (ctypes.c_uint32 * 4)()
    _lib.check(L.bfz_perm_trace(CHIP, t.ctypes.data_as(u32p), None, t.shape[0], alpha, beta,
                                ctypes.byref(out), ctypes.byref(w), cs))
    want = np.ctypeslib.as_array(out, shape=(t.shape[0], w.value)).copy()
    L.bfz_free(out)
    got, got_cs = sdk.lookups_perm_trace(prog, t, None, list(alpha), list(beta), on_device=True)
    same = bool(np.array_equal(got, want)) and got_cs == list(cs)
    del got, want
    pm, cm = (ctypes.c_float * a.runs)(), (ctypes.c_float * a.runs)()
    buf, n = _lib.u8buf(prog)
    _lib.check(L.bfz_lookups_time(buf, n, CHIP, t.ctypes.data_as(u32p), None, t.shape[0], alpha, beta,
                                  a.runs, pm, cm))
    # the bytes the algorithm needs: the main columns read once, the batch columns and row sums written
    need = t.shape[0] * 4 * (info.main_width + 4 * (info.perm_width - 1) + 4)
    res = {"program": "FIBO_X4", "stdin": [255], "chip": "Cpu", "height": int(t.shape[0]),
           "width": int(t.shape[1]), "interactions": info.n_interactions,
           "list_words": info.list_words, "words_equal_compiled": same,
           "k_perm_rows_prog<1>_ms": spread(list(pm)), "k_perm_rows<0>_ms": spread(list(cm)),
           "algorithmic_bytes": int(need),
           "k_perm_rows_prog<1>_GBps": round(need / statistics.median(pm) / 1e6, 1),
           "k_perm_rows<0>_GBps": round(need / statistics.median(cm) / 1e6, 1),
           "ratio_prog_over_compiled": round(statistics.median(pm) / statistics.median(cm), 3),
           "timer": "hipEventElapsedTime around one launch; launches alternate prog, compiled"}
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    if not same:
        sys.exit("the program's permutation trace differs from the compiled chip's")


if __name__ == "__main__":
    main()
