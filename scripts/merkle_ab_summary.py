"""Merkle hashing time per proof of one rocprofv3 --kernel-trace run of bench.py, for same-box
A/Bs of csrc/merkle.hip builds (profiles/r07/).

A proof starts at a k_trace_cpu dispatch; proofs before the last `timed` ones are warm-up.  Per
timed proof: the summed time of k_hash_leaves, k_compress and k_hash_rows8, and one launch of each
as G permutations / s: the proof's first full-grid k_hash_leaves (the main trace, 2^23 rows x 31
columns = 33.6 M permutations), the longest k_compress (the 2^22-node layer that injects the
41-column matrix = 33.6 M) and the longest k_hash_rows8 (the first FRI layer = 4.19 M).

usage: python3 scripts/merkle_ab_summary.py run_kernel_trace.csv <label> [timed proofs, default 5]
"""
import statistics
import sys

from kernel_outliers import load

KERNELS = {"k_hash_leaves": 33.554432e6, "k_compress": 33.554432e6, "k_hash_rows8": 4.194304e6}


def main():
    rows = load(sys.argv[1])
    label = sys.argv[2]
    timed = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    starts = [i for i, r in enumerate(rows) if r["name"] == "k_trace_cpu"]
    if not starts:
        sys.exit("no k_trace_cpu dispatch in the trace: not a bench.py run")
    bounds = starts + [len(rows)]
    proofs = [rows[bounds[k]:bounds[k + 1]] for k in range(len(starts))][-timed:]
    out = {"label": label, "proofs": len(proofs)}
    for name, perms in KERNELS.items():
        tot, longest = [], []
        for p in proofs:
            ls = [r for r in p if r["name"] == name]
            d = [r["end"] - r["start"] for r in ls]
            if d:
                tot.append(sum(d) / 1e6)
                if name == "k_hash_leaves":
                    full = max(r["wgs"] for r in ls)
                    d = [[r["end"] - r["start"] for r in ls if r["wgs"] == full][0]]
                longest.append(max(d) / 1e3)
        if not tot:
            continue
        us = statistics.median(longest)
        out[name] = {"ms_per_proof": round(statistics.mean(tot), 4),
                     "launch_us": round(us, 1),
                     "gperms_per_s": round(perms / us / 1e3, 3)}
    both = out["k_hash_leaves"]["ms_per_proof"] + out["k_compress"]["ms_per_proof"]
    print(f"{label:10s} leaves+compress {both:7.3f} ms/proof | " + " | ".join(
        f"{k} {v['ms_per_proof']:.3f} ms, launch {v['launch_us']:.0f} us = "
        f"{v['gperms_per_s']:.2f} G/s" for k, v in out.items() if isinstance(v, dict)))


if __name__ == "__main__":
    main()
