#!/usr/bin/env python3
"""Times hibayes_amd.eigh's stages against numpy.linalg.eigh (LAPACK dsyevd on the host's cores: make_grm's default route) on the same matrix.

    python tools/eig_timing.py [--n 2000 8000 20000] [--out profiles/eig_timing.txt] [--no-host-above N] [--tridiagonal host|device] [--append]

Per n: reduce (hb_eig_reduce, device) / tridiagonal (dstemr, host) / upload + back-transform (hb_eig_vectors: Z over the bus, K = Q Z on the device) /
total, numpy.linalg.eigh beside it, and the two error measures of tests/eig_restatement.py on the device's pair where n allows. One untimed small
run first loads the code objects. --tridiagonal device times the leg with the middle stage on the device (hb_eig_tridiagonal: Z never leaves it,
"vectors" is then the back-transformation alone) and adds that stage's phases — leaves, gather + deflation scan, rotations + secular equation +
vector work, U strips + GEMM, copies + ordering — with the GEMM's operations over the GEMM phase's seconds as its achieved rate; --append adds
the rows to the file instead of replacing it. The matrix is a GRM-like G = Z Z' / mean(diag) + 0.01 I with m = 2 n random 0..2 codes, formed on the host."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def matrix(n):
    rng = np.random.default_rng(n)
    M = rng.integers(0, 3, size=(n, 2 * n)).astype(np.float32)
    M -= M.mean(axis=0, keepdims=True)
    G = (M @ M.T).astype(np.float64)
    G = 0.5 * (G + G.T)
    G /= np.mean(np.diag(G))
    G[np.diag_indices(n)] += 0.01
    return np.asfortranarray(G)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2000, 8000, 20000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eig_timing.txt"))
    ap.add_argument("--no-host-above", type=int, default=1 << 30, help="skip numpy.linalg.eigh (and the error measures) above this n")
    ap.add_argument("--tridiagonal", choices=["host", "device"], default="host", help="where the tridiagonal stage runs")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    a = ap.parse_args()
    import hibayes_amd as H
    from hibayes_amd import eig as HE
    import eig_restatement as E
    dev = a.tridiagonal == "device"
    H.eigh(matrix(300), tridiagonal=a.tridiagonal)
    lines = ["# tools/eig_timing.py%s: seconds per stage, one run each; host = numpy.linalg.eigh on %s threads"
             % (" --tridiagonal device" if dev else "", os.environ.get("OMP_NUM_THREADS", "all")),
             "# %6s %9s %9s %9s %9s %9s %9s %9s %10s %10s" % ("n", "upload_G", "reduce", "tridiag", "vectors", "download", "total", "host_eigh", "res_eps", "orth_eps")]
    if dev:
        lines[-1] += " | %8s %8s %8s %8s %8s %10s" % ("leaves", "scan", "secular", "gemm", "copies", "gemm_TF/s")
    print("\n".join(lines), flush=True)
    for n in a.n:
        G = matrix(n)
        st = {}
        t0 = time.perf_counter()
        A = HE.upload(G)
        t1 = time.perf_counter()
        Kh = HE.eigh_device(A, keep_on_device=True, stats=st, tridiagonal=a.tridiagonal)
        t2 = time.perf_counter()
        K = Kh.toarray()
        t3 = time.perf_counter()
        w = Kh.values
        Kh.close()
        host = res = orth = float("nan")
        if n <= a.no_host_above:
            t4 = time.perf_counter()
            np.linalg.eigh(G)
            host = time.perf_counter() - t4
            res, orth = E.res_eps(G, w, K), E.orth_eps(K)
        line = "  %6d %9.3f %9.3f %9.3f %9.3f %9.3f %9.3f %9.3f %10.1f %10.1f" % (n, t1 - t0, st["reduce"], st["tridiagonal"], st["vectors"], t3 - t2,
                                                                                t2 - t0, host, res, orth)
        if dev:
            ph = HE.stedc_stats()
            line += " | %8.3f %8.3f %8.3f %8.3f %8.3f %10.2f" % (ph["leaves"], ph["scan"], ph["secular"], ph["gemm"], ph["copies"],
                                                               1e-12 * ph["gemm_flops"] / max(ph["gemm"], 1e-9))
        print(line, flush=True)
        lines.append(line)
        del G, K
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
