#!/usr/bin/env python
"""Time per iteration and bytes per second of the conjugate-gradient solve (hibayes_amd/cg.py, hb_cg.hip) on a synthetic
symmetric LD-like matrix: dense (conjgt_den on the host array) and chi^2-sparsified (conjgt_spa on its handle), beside the
streaming-read rate bench.py quotes as roofline.measured_copy_GBps (Context.time_stream_read). Needs a GPU.

    python tools/cg_time.py [--m 20000] [--out profiles/cg_timing.txt]

The time is the solve's own loop_seconds over the passes it ran: the whole loop as a caller sees it — three launches per pass,
one synchronise and read-back per chunk of `--chunk` passes, and the empty launches between the pass that stops and the end of
its chunk — not a kernel time. Bytes per pass are what the algorithm must read: the matrix once (m * m * 8 dense; 12 per stored
entry plus 8 (m + 1) of column pointers sparse) plus the vectors (p, ap, x, r read and written: 11 m * 8)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hibayes_amd as H  # noqa: E402


def synthetic(m, rank, seed):
    """V = U diag(c^2) U' / rank + 0.05 I with c log-spaced over two decades: symmetric to the bit, positive definite"""
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((m, rank)) * np.logspace(0, -2, rank)
    V = U @ U.T
    V /= rank
    V[np.diag_indices(m)] += 0.05
    V = np.triu(V)
    V += np.triu(V, 1).T
    return np.asfortranarray(V)


def sparsify(V, n, chisq):
    import scipy.sparse as sp
    d = np.sqrt(np.diag(V))
    keep = np.empty(V.shape, dtype=bool)
    for j0 in range(0, V.shape[0], 1024):          # the correlations by column strips; np.where below still makes one more m x m array
        r = V[:, j0:j0 + 1024] / np.outer(d, d[j0:j0 + 1024])
        keep[:, j0:j0 + 1024] = r * r * n > chisq
    A = sp.csc_matrix(np.where(keep, V, 0.0))
    A.sort_indices()
    return A


def run(label, fit, ss, ldm, lam, esp, chunk, bytes_per_pass, min_seconds, say):
    fit(ss, ldm, lam, esp=esp, outfreq=chunk, verbose=False)                       # warm-up: code objects, the handle's device copies
    secs, its, runs, per = 0.0, 0, 0, []
    while secs < min_seconds and runs < 20:
        r = fit(ss, ldm, lam, esp=esp, outfreq=chunk, verbose=False)
        secs += r["timing"]["loop_seconds"]
        its += r["iterations"]
        per.append(r["timing"]["loop_seconds"] / r["iterations"])
        runs += 1
    say("%s: %d solves, %d passes each (converged: %s, err %.3g), %.4f ms per pass (per solve: min %.4f, max %.4f), "
        "%.1f MB per pass -> %.0f GB/s" % (label, runs, r["iterations"], r["converged"], r["err"], 1e3 * secs / its, 1e3 * min(per),
                                          1e3 * max(per), bytes_per_pass / 1e6, bytes_per_pass * its / secs / 1e9))
    return bytes_per_pass * its / secs / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=20000)
    ap.add_argument("--rank", type=int, default=200)
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--chisq", type=float, default=5.0)
    ap.add_argument("--lam", type=float, default=0.05)
    ap.add_argument("--esp", type=float, default=1e-8)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if H.lib().hb_device_count() < 1:
        raise SystemExit("cg_time.py: no HIP device visible")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("command: python tools/cg_time.py " + " ".join(sys.argv[1:]))
    m = a.m
    t = time.time()
    V = synthetic(m, a.rank, 11)
    rng = np.random.default_rng(12)
    ss = np.column_stack([np.full(m, 0.3), rng.normal(0, 0.1, m), np.full(m, 0.02), np.full(m, float(a.n))])
    lam = np.full(m, a.lam)
    say("m = %d, synthetic matrix of rank %d + 0.05 I made in %.1f s; lambda = %g, esp = %g, chunks of %d passes" %
        (m, a.rank, time.time() - t, a.lam, a.esp, a.chunk))
    with H.Context(20000, 20000) as ctx:                                            # bench.py's ceiling: a plain streaming read of 400 MB
        ctx.generate(5)
        ms, nb = ctx.time_stream_read(reps=3)
    copy = nb / (ms * 1e-3) / 1e9
    say("streaming read of %.0f MB of resident genotypes (bench.py's roofline.measured_copy_GBps): %.0f GB/s" % (nb / 1e6, copy))
    vec = 11 * m * 8
    d = run("dense", H.conjgt_den, ss, V, lam, a.esp, a.chunk, m * m * 8 + vec, a.min_seconds, say)
    say("dense: %.3f of the streaming-read rate" % (d / copy))
    t = time.time()
    A = sparsify(V, a.n, a.chisq)
    del V
    per = np.diff(A.indptr)
    say("chi^2 > %g at n = %d keeps %.2f %% of the entries (%d; per column mean %.0f, max %d), made in %.1f s" %
        (a.chisq, a.n, 100.0 * A.nnz / m / m, A.nnz, per.mean(), per.max(), time.time() - t))
    with H.LDMatrix.from_scipy(A) as ld:
        # the thresholded matrix is indefinite: a ridge that keeps V + Lambda positive definite (Gershgorin would do; this is a timing)
        lam_s = np.full(m, a.lam + 0.1 * float(abs(A).sum(axis=0).max()))
        s = run("sparse", H.conjgt_spa, ss, ld, lam_s, a.esp, a.chunk, A.nnz * 12 + (m + 1) * 8 + vec, a.min_seconds, say)
    say("sparse: %.3f of the streaming-read rate" % (s / copy))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
