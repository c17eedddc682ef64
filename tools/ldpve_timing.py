#!/usr/bin/env python3
"""Times LDMatrix.window_var (hb_ldm_window_var, hibayes_amd/csrc/hb_ldquad.hip) on the two loaders at the sizes they exist for.

    python tools/ldpve_timing.py [--m-sparse 100000] [--half-width 500] [--m-dense 20000] [--n 1000] [--window 100] [--reps 5]
                                 [--out profiles/ldpve_timing.txt]

Shape 1: the sparse sampler's shape, a band of --half-width around the diagonal of --m-sparse markers handed over by
LDMatrix.from_scipy (the device CSC). Shape 2: a dense handle of --m-dense markers built by ldmat() from generated genotypes of --n individuals
(the dense device copy). Two cases each: 64 records with 5 % of the effects non-zero (a point-mass model's stored samples) and 8 dense records;
windows of --window consecutive markers. Per case the call is repeated --reps times after one untimed round; the table holds the median and the
least wall time (host clock around a call that ends in a copy back, so the host's plan of every batch and its copies are in it) and the counted
bytes of matrix entries the call reads per second of the median: per batch and listed column, its stored entries at 12 B (value and row index)
in the CSC or its m entries at 8 B in the dense copy. The numbers are reported, nothing asserts them."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def band_csc(m, hw):
    """V_ij = 0.98^|i - j| (1 + 0.1 sin(i + j)) for |i - j| <= hw: from |i - j| and i + j alone, so (i, j) and (j, i) hold the same bits"""
    import scipy.sparse as sp
    off = np.arange(-hw, hw + 1)
    decay = 0.98 ** np.abs(off)
    indptr, ind, dat = np.zeros(m + 1, dtype=np.int64), [], []
    for j0 in range(0, m, 8192):
        j = np.arange(j0, min(m, j0 + 8192))
        rows = j[:, None] + off[None, :]
        ok = (rows >= 0) & (rows < m)
        vals = decay[None, :] * (1.0 + 0.1 * np.sin((rows + j[:, None]).astype(np.float64)))
        indptr[j + 1] = ok.sum(axis=1)
        ind.append(rows[ok].astype(np.int32))
        dat.append(vals[ok])
    np.cumsum(indptr, out=indptr)
    return sp.csc_matrix((np.concatenate(dat), np.concatenate(ind), indptr), shape=(m, m))


def counted_bytes(A, per_column, entry_bytes):
    """the entries read: per batch of 8 records, the columns with a non-zero effect in any of them"""
    total = 0
    for r0 in range(0, A.shape[1], 8):
        listed = np.any(A[:, r0:r0 + 8] != 0.0, axis=1)
        total += int(per_column[listed].sum()) * entry_bytes
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m-sparse", type=int, default=100000)
    ap.add_argument("--half-width", type=int, default=500)
    ap.add_argument("--m-dense", type=int, default=20000)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--window", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ldpve_timing.txt"))
    a = ap.parse_args()
    from hibayes_amd import Context, LDMatrix
    lines = ["# tools/ldpve_timing.py: windows of %d markers; seconds per call, median (least) of %d repeats; GB/s = counted bytes of entries read / median" % (a.window, a.reps),
             "# %-34s %-26s %8s %12s %19s %9s" % ("matrix", "case", "windows", "entries", "window_var", "GB/s")]
    print("\n".join(lines), flush=True)

    def run(name, ld, per_column, entry_bytes):
        m = ld.shape[0]
        rng = np.random.default_rng(8)
        w = (np.arange(m) // a.window + 1).astype(np.uint32)
        sparse = np.asfortranarray(rng.standard_normal((m, 64)) * (rng.random((m, 64)) < 0.05))
        dense = np.asfortranarray(rng.standard_normal((m, 8)))
        for case, A in (("64 records, 5 % non-zero", sparse), ("8 dense records", dense)):
            ts = []
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                ld.window_var(A, w)
                t1 = time.perf_counter()
                if rep:   # (the first round loads the code objects and makes the device copy)
                    ts.append(t1 - t0)
            nbytes = counted_bytes(A, per_column, entry_bytes)
            line = "  %-34s %-26s %8d %12d %9.4f (%7.4f) %9.1f" % (name, case, int(w.max()), nbytes // entry_bytes, np.median(ts), min(ts),
                                                                 1e-9 * nbytes / np.median(ts))
            print(line, flush=True)
            lines.append(line)

    V = band_csc(a.m_sparse, a.half_width)
    with LDMatrix.from_scipy(V) as ld:
        run("band +-%d, m = %d (CSC)" % (a.half_width, a.m_sparse), ld, np.diff(V.indptr), 12)
    del V
    with Context(a.n, a.m_dense) as c:
        c.generate(20240901)
        ld = c.ldmat()
    with ld:
        assert ld.kind == "dense"
        run("ldmat(), m = %d (dense)" % a.m_dense, ld, np.full(a.m_dense, a.m_dense, dtype=np.int64), 8)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
