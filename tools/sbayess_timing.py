#!/usr/bin/env python3
"""Milliseconds per sweep of the sparse summary-level sampler (SBayesS, hb_sbayes_run_sparse) for BayesCpi and BayesRR at two
shapes, one JSON line:
  band   m = 100 000, a symmetric band of half-width 500 (about 1e8 stored entries; the dense matrix would be 80 GB);
  demo   the demo's genome-wide dense LD matrix (m = 1000, every entry stored), next to SBayesD on the same handle.
A sweep is loop_seconds / iters_done of the run's own timing: set-up and the CSC's upload are outside it, the graph capture is
inside the first sweep, so the runs are long enough to drown it. profiles/sbayess_timing.json is its output on an MI355X.

    python tools/sbayess_timing.py [--m 100000] [--halfwidth 500] [--sweeps 40]
"""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hibayes_amd as H  # noqa: E402


def band(m, hw, rho=0.97):
    """csc of rho^|i - j| for |i - j| <= hw, built column by column without a COO detour"""
    off = np.arange(-hw, hw + 1)
    vals = rho ** np.abs(off)
    indptr = np.zeros(m + 1, dtype=np.int64)
    lo, hi = np.maximum(0, np.arange(m) - hw), np.minimum(m - 1, np.arange(m) + hw)
    indptr[1:] = np.cumsum(hi - lo + 1)
    indices, data = np.empty(indptr[-1], dtype=np.int32), np.empty(indptr[-1])
    for j0 in range(0, m, 8192):
        j = np.arange(j0, min(m, j0 + 8192))
        rows = j[:, None] + off[None, :]
        ok = (rows >= 0) & (rows < m)
        indices[indptr[j[0]]:indptr[j[-1] + 1]] = rows[ok]
        data[indptr[j[0]]:indptr[j[-1] + 1]] = np.broadcast_to(vals, rows.shape)[ok]
    return sp.csc_matrix((data, indices, indptr), shape=(m, m))


def ms_per_sweep(res):
    t = res["timing"]
    return round(1e3 * t["loop_seconds"] / max(1, t["iters_done"]), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=100000)
    ap.add_argument("--halfwidth", type=int, default=500)
    ap.add_argument("--sweeps", type=int, default=40)
    a = ap.parse_args()
    out = {"device": H.lib().hb_version().decode(), "sweeps": a.sweeps}
    rng = np.random.default_rng(1)
    kw = dict(niter=a.sweeps, nburn=0, thin=a.sweeps, verbose=False, store_alpha=False, seed=3)

    m = a.m
    b = rng.normal(0, 0.02, m)
    b[rng.choice(m, max(1, m // 500), replace=False)] += rng.normal(0, 0.5, max(1, m // 500))
    ss = np.column_stack([np.full(m, 0.3), b, np.full(m, 0.03), np.full(m, 1000.0)])
    with H.LDMatrix.from_scipy(band(m, a.halfwidth)) as ld:
        shape = {"m": m, "halfwidth": a.halfwidth, "nnz": int(ld.nnz), "launches_per_sweep": 2 * ((m + 511) // 512) + 3}
        for model in ("BayesCpi", "BayesRR"):
            r = H.SBayesS(ss, ld, model, [0.95, 0.05], **kw)
            shape[model + "_ms_per_sweep"] = ms_per_sweep(r)
            shape[model + "_moves_per_sweep"] = round(r["timing"]["mean_events"], 1)
    out["band"] = shape

    d = os.path.join(ROOT, "tests", "golden", "demo", "demo")
    geno = H.read_plink(d)["geno"]
    rows = [ln.split() for ln in open(d + ".ma")][1:]
    f = lambda x: float(x) if x != "NA" else np.nan
    ssd = np.array([[f(r[3]), f(r[4]), f(r[5]), f(r[7])] for r in rows])
    kw["niter"] = kw["thin"] = 10 * a.sweeps
    with H.ldmat(geno, keep_on_device=True) as ld:
        shape = {"m": int(ld.shape[0]), "nnz": int(ld.nnz), "launches_per_sweep": 2 * ((ld.shape[0] + 511) // 512) + 3}
        for model in ("BayesCpi", "BayesRR"):
            shape[model + "_ms_per_sweep"] = ms_per_sweep(H.SBayesS(ssd, ld, model, [0.95, 0.05], **kw))
            shape[model + "_ms_per_sweep_SBayesD"] = ms_per_sweep(H.SBayesD(ssd, ld, model, [0.95, 0.05], **kw))
    out["demo"] = shape
    print(json.dumps(out))


if __name__ == "__main__":
    main()
