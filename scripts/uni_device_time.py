#!/usr/bin/env python3
"""The uni-STARK device paths against their host counterparts on the headline record (FIBO_X4
stdin [255]) at 84 queries (profiles/r10/uni_device.json):

  prove    bfz_uni_prove from the host trace   against  bfz_record_uni_prove     Cpu 2^22, Jump 2^19
  verify   bfz_uni_verify_batch on_device = 0  against  on_device = 1            1 proof, then 8
  check    bfz_uni_check on_device = 0         against  on_device = 1            Cpu 2^22

One process, everything warmed, the calls of each pair alternate, wall clock around the whole C
call, median and min-max of --runs calls.  A device figure counts as faster only when its range
lies wholly below the host figure's range ("device_faster").

  python scripts/uni_device_time.py [--out FILE] [--runs 6]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \\
      python scripts/uni_device_time.py --workload      # k_check_air and the verify kernels
  python scripts/uni_device_time.py --kernels DIR/run_kernel_trace.csv"""
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

CHIPS = ((0, "Cpu"), (3, "Jump"))
P32 = ctypes.POINTER(ctypes.c_uint32)


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
            "runs": len(v)}


def pair(host, device, runs):
    """host() and device() alternate; each returns nothing and is timed whole."""
    host(), device()  # warm-up of both
    h, d = [], []
    for _ in range(runs):
        for f, into in ((host, h), (device, d)):
            t0 = time.perf_counter()
            f()
            into.append((time.perf_counter() - t0) * 1e3)
    out = {"host_ms": spread(h), "device_ms": spread(d)}
    out["device_faster"] = max(d) < min(h)
    out["ranges_overlap"] = not (max(d) < min(h) or max(h) < min(d))
    return out


class Calls:
    """The raw C calls on the headline record, arguments prepared once."""

    def __init__(self):
        from bfz import _lib, guests, sdk
        from uni_stark_time import trace
        self.lib, self.L = _lib, _lib.lib()
        self.traces = {chip: trace(chip) for chip, _ in CHIPS}
        client = sdk.ProverClient()
        self.pk, _ = client.setup(guests.FIBO_X4)
        buf, n = _lib.u8buf(bytes([255]))
        self.rec = ctypes.c_void_p()
        _lib.check(self.L.bfz_record_new(ctypes.c_void_p(self.pk.handle), buf, n, ctypes.byref(self.rec), None))
        self.last = None

    def close(self):
        self.L.bfz_record_free(self.rec)

    def _take(self, ptr, n):
        self.last = self.lib.take_bytes(ptr, n.value)

    def prove_host(self, chip, timings=None):
        t = self.traces[chip]
        ch = self.lib.Challenger()
        ptr, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t()
        self.lib.check(self.L.bfz_uni_prove(chip, t.ctypes.data_as(P32), t.shape[0], t.shape[1],
                                            ctypes.byref(ch), ctypes.byref(ptr), ctypes.byref(n),
                                            ctypes.byref(timings) if timings is not None else None))
        self._take(ptr, n)

    def prove_record(self, chip, timings=None):
        ch = self.lib.Challenger()
        ptr, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_size_t()
        self.lib.check(self.L.bfz_record_uni_prove(self.rec, chip, ctypes.byref(ch), ctypes.byref(ptr),
                                                   ctypes.byref(n),
                                                   ctypes.byref(timings) if timings is not None else None))
        self._take(ptr, n)

    def verifier(self, chip, proof, count, on_device):
        buf, n = self.lib.u8buf(proof)
        arr = (ctypes.POINTER(ctypes.c_uint8) * count)(
            *[ctypes.cast(buf, ctypes.POINTER(ctypes.c_uint8))] * count)
        lens = (ctypes.c_size_t * count)(*[n] * count)
        chips = (ctypes.c_int * count)(*[chip] * count)
        out = (self.lib.VerifyOutcomeC * count)()

        def run():
            chs = (self.lib.Challenger * count)()
            self.lib.check(self.L.bfz_uni_verify_batch(chips, chs, arr, lens, count, on_device, out))
            assert all(out[i].ok for i in range(count)), out[0].why
        run.keep = (buf, arr, lens, chips, out)
        return run

    def checker(self, chip, on_device):
        t = self.traces[chip]
        out = self.lib.UniCheckC()

        def run():
            self.lib.check(self.L.bfz_uni_check(chip, t.ctypes.data_as(P32), t.shape[0], t.shape[1],
                                                on_device, ctypes.byref(out), None))
            assert out.failing_rows == 0
        return run


def timings(runs):
    c = Calls()
    res = {"program": "FIBO_X4", "stdin": [255], "queries": 84, "runs": runs,
           "method": "wall clock around the whole C call; the calls of a pair alternate in one process",
           "prove": {}, "verify": {}}
    try:
        for chip, name in CHIPS:
            t = c.traces[chip]
            c.prove_host(chip)
            proof = c.last
            c.prove_record(chip)
            assert c.last == proof  # byte-identical
            r = pair(lambda: c.prove_host(chip), lambda: c.prove_record(chip), runs)
            r = {"from_host_trace_ms": r.pop("host_ms"), "from_record_ms": r.pop("device_ms"), **r}
            tm = c.lib.Timings()
            c.prove_record(chip, tm)
            r["record_stage_ms"] = {k: round(getattr(tm, k), 3) for k in
                                    ("trace_ms", "main_commit_ms", "quotient_ms", "open_ms", "fri_ms", "total_ms")}
            r.update(height=int(t.shape[0]), width=int(t.shape[1]), proof_bytes=len(proof))
            res["prove"][name] = r
            res["verify"][name] = {
                f"{k}_proof": pair(c.verifier(chip, proof, k, 0), c.verifier(chip, proof, k, 1), runs)
                for k in (1, 8)}
        res["check"] = {"Cpu": dict(pair(c.checker(0, 0), c.checker(0, 1), runs),
                                    height=int(c.traces[0].shape[0]))}
    finally:
        c.close()
    return res


def workload():
    c = Calls()
    try:
        for chip, _ in CHIPS:
            c.prove_record(chip)
            for k in (1, 8):
                run = c.verifier(chip, c.last, k, 1)
                for _ in range(3):
                    run()
            run = c.checker(chip, 1)
            for _ in range(3):
                run()
    finally:
        c.close()


def kernels(path):
    rows = {}
    for r in csv.DictReader(open(path)):
        nm = r["Kernel_Name"]
        for key in ("k_check_air", "k_verify_fold", "k_verify_fri_paths", "k_verify_inputs"):
            if key in nm:
                if key == "k_check_air":
                    key = nm[nm.index(key):].split("(")[0]
                rows.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"launches": len(v), "median_us": round(statistics.median(v), 1),
                "min_us": round(min(v), 1), "max_us": round(max(v), 1)} for k, v in sorted(rows.items())}


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
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
