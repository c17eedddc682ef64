#!/usr/bin/env python3
"""Times Context.window_var (hb_ctx_window_var, hibayes_amd/csrc/hb_pve.hip) against Context.matmul of the same records — the same products, and
the nearest thing the library had before — at the benchmark's shape.

    python tools/pve_timing.py [--n 50000] [--m 500000] [--window 100] [--reps 5] [--out profiles/pve_timing.txt]

Genotypes from Context.generate, windows of --window consecutive markers, on the int8 and the 2-bit layout, two cases: 64 records with 1 % of the
effects non-zero (a point-mass model's stored samples) and 8 dense records. Per case and layout the two calls alternate --reps times after one
untimed round; the table holds the median and the least wall time of each (host clock around calls that end in a synchronise, so the host's
packing of the batches and the copies are in both), their ratio, and how far the totals are from the variance of matmul's columns. The numbers
are reported, nothing asserts them."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--m", type=int, default=500000)
    ap.add_argument("--window", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pve_timing.txt"))
    a = ap.parse_args()
    from hibayes_amd import Context
    n, m = a.n, a.m
    rng = np.random.default_rng(8)
    w = (np.arange(m) // a.window + 1).astype(np.uint32)
    sparse = np.asfortranarray(rng.standard_normal((m, 64)) * (rng.random((m, 64)) < 0.01))
    dense = np.asfortranarray(rng.standard_normal((m, 8)))
    cases = (("64 records, 1 % non-zero", sparse), ("8 dense records", dense))
    lines = ["# tools/pve_timing.py: n = %d, m = %d, %d windows of %d markers; seconds per call, median (least) of %d alternating repeats" % (n, m, int(w.max()), a.window, a.reps),
             "# %-26s %6s %19s %19s %8s %12s" % ("case", "layout", "window_var", "matmul", "ratio", "total_relerr")]
    print("\n".join(lines), flush=True)
    with Context(n, m) as c:
        c.generate(20240901)
        for bits in (8, 2):
            if bits == 2:
                c.set_layout(2)
            for name, A in cases:
                tw, tm = [], []
                for rep in range(a.reps + 1):
                    t0 = time.perf_counter()
                    var, tot = c.window_var(A, w)
                    t1 = time.perf_counter()
                    g = c.matmul(A)
                    t2 = time.perf_counter()
                    if rep:   # (the first round loads the code objects)
                        tw.append(t1 - t0)
                        tm.append(t2 - t1)
                rel = float(np.max(np.abs(tot - g.var(axis=0, ddof=1)) / g.var(axis=0, ddof=1)))
                del g
                line = "  %-26s %6d %9.3f (%7.3f) %9.3f (%7.3f) %8.2f %12.2e" % (name, bits, np.median(tw), min(tw), np.median(tm), min(tm),
                                                                                np.median(tw) / np.median(tm), rel)
                print(line, flush=True)
                lines.append(line)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
