#!/usr/bin/env python3
"""Regenerate tests/golden/reference_rs_lines.json from a checkout of the reference workspace:

    python tests/golden/make_reference_index.py PATH_TO_REFERENCE

The file lists every .rs file of the reference (path relative to the workspace) with its number
of lines -- names and counts only, nothing of the files' text.  tests/test_citations.py checks
each `file.rs:N-M` citation of this repository against it, so that test needs no checkout.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ref = sys.argv[1]
    rs_lines = {}
    for d, dirs, fs in os.walk(ref):
        dirs[:] = sorted(x for x in dirs if x not in (".git", "target"))
        for f in sorted(fs):
            if f.endswith(".rs"):
                p = os.path.join(d, f)
                with open(p, errors="replace") as fh:
                    rs_lines[os.path.relpath(p, ref)] = sum(1 for _ in fh)
    with open(os.path.join(HERE, "reference_rs_lines.json"), "w") as f:
        json.dump(rs_lines, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote reference_rs_lines.json: {len(rs_lines)} .rs files")


if __name__ == "__main__":
    main()
