#!/usr/bin/env python3
"""Derives K of tests/test_gpu_long_fp64.py from the reference alone (CPU only, a few minutes).

D_ref = |fp32 oracle - double oracle| per compared quantity on the headline net (39 -> 3 x blstm250 -> 183, PS 50, 48 sequences
U[240,300], longest 300) for three seeds x two slot orders (the same sequences with the slots reversed: the same mathematics,
another fp32 summation order).  s = the largest max/min of any quantity over the six runs; K = max(4, 2 s).  Prints the table
that the test module's K_DERIVATION and DESIGN.md section 3 quote."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import __graft_entry__ as ge  # noqa: E402
from helpers import fp64_distances, oracle_reference  # noqa: E402
from test_gpu_long_fp64 import build_case  # noqa: E402


def main():
    pkg, orc = ge.load_package(), ge.load_oracle()
    o64 = orc.real64()
    n = min(16, len(os.sched_getaffinity(0)))
    orc.set_threads(n); o64.set_threads(n)
    runs = {}
    for seed in (70, 71, 72):
        for rev in (False, True):
            case = build_case(pkg, "a", seed=seed, reverse=rev, lo=240, hi=300)
            args = (case["layers"], case["weights"], case["frac"], case["PS"])
            d = fp64_distances(oracle_reference(orc, *args), oracle_reference(o64, *args), case["T"], case["slot"])
            runs[(seed, rev)] = d
            print("seed %d %s: %s" % (seed, "reversed" if rev else "in order", {k: float("%.3g" % v) for k, v in sorted(d.items())}), flush=True)
    s = 0.0
    print("%-14s %10s %10s %8s" % ("quantity", "min D_ref", "max D_ref", "max/min"))
    for k in sorted(next(iter(runs.values()))):
        v = [r[k] for r in runs.values()]
        s = max(s, max(v) / min(v))
        print("%-14s %10.3g %10.3g %8.2f" % (k, min(v), max(v), max(v) / min(v)))
    print("s = %.2f, K = max(4, 2 s) = %.2f" % (s, max(4.0, 2 * s)))


if __name__ == "__main__":
    main()
