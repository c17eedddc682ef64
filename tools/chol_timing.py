#!/usr/bin/env python3
"""Times the stages of hibayes_amd's device inverse (hb_chol_factor, hb_chol_invert_factor, hb_spd_inverse; hibayes_amd/csrc/hb_chol.hip) against
LAPACK's dpotrf + dpotri through scipy on the host's cores, on the same matrix.

    python tools/chol_timing.py [--n 2000 8000 20000] [--out profiles/chol_timing.txt] [--no-host-above N] [--no-residual-above N]

Per n: the factorisation (dpotrf), the factor's inverse (dtrtri) — each timed on a device copy of its own input — the whole hb_spd_inverse, and the
product stage as what is left of the whole after the other two (dlauum, with the copy into the work buffer); scipy's dpotrf + dpotri beside them; the
achieved rate n^3 / seconds of the whole call and of the host (n^3 / 3 operations each for the factor, its inverse and the product); resR of
tests/chol_restatement.py for both up to --no-residual-above (its 2-norms are singular value decompositions). One untimed small run first loads
the code objects. The matrix is GRM-like, G = Z Z' / mean(diag) + 0.01 I with m = n / 8 random 0..2 codes, formed on the host. The numbers are
reported, nothing asserts them."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def matrix(n):
    rng = np.random.default_rng(n)
    M = rng.integers(0, 3, size=(n, max(n // 8, 16))).astype(np.float32)
    M -= M.mean(axis=0, keepdims=True)
    G = (M @ M.T).astype(np.float64)
    G = 0.5 * (G + G.T)
    G /= np.mean(np.diag(G))
    G[np.diag_indices(n)] += 0.01
    return np.asfortranarray(G)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2000, 8000, 20000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chol_timing.txt"))
    ap.add_argument("--no-host-above", type=int, default=1 << 30, help="skip scipy's dpotrf + dpotri (and the residuals) above this n")
    ap.add_argument("--no-residual-above", type=int, default=4000, help="skip the residuals above this n")
    a = ap.parse_args()
    import hibayes_amd as H
    from hibayes_amd import eig as HE
    from hibayes_amd._lib import check
    from scipy.linalg import lapack
    import chol_restatement as R
    L = H.lib()
    H.spd_inverse(matrix(300))
    lines = ["# tools/chol_timing.py: seconds per stage, one run each; host = scipy dpotrf + dpotri on %s threads; rates are n^3 / seconds"
             % os.environ.get("OMP_NUM_THREADS", "all"),
             "# %6s %9s %9s %9s %9s %9s %9s %11s %11s %9s %9s" % ("n", "factor", "invert", "product", "total", "download", "host", "dev_TF/s", "host_TF/s",
                                                                   "resR_dev", "resR_host")]
    print("\n".join(lines), flush=True)
    for n in a.n:
        G = matrix(n)
        info = C.c_int32()
        with HE.upload(G) as D:
            t0 = time.perf_counter()
            check(L.hb_chol_factor(D.ptr, D.ld, n, 0, 0.0, C.byref(info)))
            t1 = time.perf_counter()
            assert info.value == 0
            check(L.hb_chol_invert_factor(D.ptr, D.ld, n, 0))
            t2 = time.perf_counter()
        with HE.upload(G) as D:
            t3 = time.perf_counter()
            check(L.hb_spd_inverse(D.ptr, D.ld, n, 0, 0.0, C.byref(info)))
            t4 = time.perf_counter()
            assert info.value == 0
            X = D.toarray()
            t5 = time.perf_counter()
        fac, inv, tot = t1 - t0, t2 - t1, t4 - t3
        host = rd = rh = float("nan")
        if n <= a.no_host_above:
            t6 = time.perf_counter()
            c, i1 = lapack.dpotrf(G, lower=1)
            xh, i2 = lapack.dpotri(c, lower=1, overwrite_c=1)
            host = time.perf_counter() - t6
            assert i1 == 0 and i2 == 0
            xh = np.tril(xh)
            xh = xh + np.tril(xh, -1).T
            if n <= a.no_residual_above:
                rd, rh = R.res_right(G, X), R.res_right(G, xh)
            del c, xh
        line = "  %6d %9.3f %9.3f %9.3f %9.3f %9.3f %9.3f %11.3f %11.3f %9.2f %9.2f" % (n, fac, inv, tot - fac - inv, tot, t5 - t4, host,
                                                                                       1e-12 * float(n) ** 3 / tot, 1e-12 * float(n) ** 3 / host, rd, rh)
        print(line, flush=True)
        lines.append(line)
        del G, X
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
