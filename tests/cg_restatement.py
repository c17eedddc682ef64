"""A numpy fp64 restatement of the reference's conjugate-gradient fitter: CG() (src/solver.cpp:54-115) and the set-up and
epilogue of conjgt_den() / conjgt_spa() (src/cg.cpp:12-53, :77-116) — a helper for the CG tests, not a test. Written from the
algorithm. The one thing the reference leaves open is the order in which `A * p` is summed (it is whatever BLAS R links), so
the product is an argument: `matvec_plain` is A @ v, `matvec_reversed_chunks` adds the columns' contributions chunk by chunk
from the last chunk to the first. Two legal orders; how far their trajectories part is the measure of what a third legal order
— the device's — may differ by (tests/test_gpu_cg.py)."""
import math

import numpy as np

from sbayess_restatement import arma_sum


def matvec_plain(A):
    return lambda v: np.asarray(A @ v, dtype=np.float64).ravel()


def matvec_reversed_chunks(A, chunk=64):
    """sum over column chunks, last chunk first: A[:, c] @ v[c] added in reversed order"""
    m = A.shape[0]
    starts = list(range(0, m, chunk))[::-1]
    A = A.tocsc() if hasattr(A, "tocsc") else A

    def mv(v):
        out = np.zeros(m)
        for s in starts:
            out += np.asarray(A[:, s:s + chunk] @ v[s:s + chunk], dtype=np.float64).ravel()
        return out
    return mv


def cg(matvec, b, lam=None, esp=1e-6):
    """CG() with x0 = NULL. Returns x, the number of passes of the loop (i + 1 at the `break`, m without one), whether
    err < esp at the end, and err of every pass."""
    b = np.asarray(b, dtype=np.float64)
    m = b.size
    x = np.zeros(m)
    r = b - matvec(x)                                   # :73
    if lam is not None:
        r = r - x * lam                                 # :81
    p = r.copy()
    r2 = float(np.sum(r * r))                           # :84
    hist, err = [], math.nan
    with np.errstate(all="ignore"):
        for _ in range(m):
            ap = matvec(p)                              # :89
            if lam is not None:
                ap = ap + p * lam                       # :91
            alpha = r2 / float(np.sum(p * ap))          # :93
            x = x + alpha * p
            r = r - alpha * ap
            r2update = float(np.sum(r * r))             # :96
            err = math.sqrt(r2update) if r2update >= 0 else math.nan
            hist.append(err)
            if err < esp:                               # :102
                break
            beta = r2update / r2
            p = r + beta * p
            r2 = r2update
    return x, len(hist), bool(err < esp), np.array(hist)


def setup(sumstat, diag):
    """src/cg.cpp:12-41 / :77-103: n, b = xy / n, yy, count_y. Raises the reference's texts."""
    ss = np.asarray(sumstat, dtype=np.float64)
    diag = np.asarray(diag, dtype=np.float64)
    if ss.shape[0] != diag.size:
        raise ValueError("Number of SNPs not equals.")
    N = ss[:, 3]
    n = int(np.mean(N[np.isfinite(N)]))                 # :13
    xpx = diag * n
    xy = xpx * ss[:, 1]                                 # a NaN BETA is not filtered
    has = ~np.isnan(ss[:, 2])
    yyi = np.where(has, xpx * (ss[:, 1] * ss[:, 1] + (N - 2) * ss[:, 2] * ss[:, 2]), 0.0)
    count_y = int(has.sum())
    if count_y == 0:
        raise ValueError("Lack of SE.")
    return n, xy / n, arma_sum(yyi) / count_y, count_y


def conjgt_restatement(sumstat, A, lam=None, esp=1e-6, matvec=None):
    """conjgt_den() / conjgt_spa() on a numpy array or a scipy sparse matrix A; matvec: a factory A -> (v -> A v)."""
    diag = A.diagonal() if hasattr(A, "diagonal") else np.diag(A)
    n, b, yy, count_y = setup(sumstat, np.asarray(diag).ravel())
    mv = (matvec or matvec_plain)(A)
    lam = None if lam is None else np.asarray(lam, dtype=np.float64)
    g, its, conv, hist = cg(mv, b, lam, esp)
    vg = n * float(g @ mv(g)) / (n - 1)                 # :52, :115
    return {"vg": vg, "ve": yy / (n - 1) - vg, "g": g, "n": n, "count_y": count_y, "iterations": its, "converged": conv,
            "err": hist[-1], "err_hist": hist, "b": b, "yy": yy}


# ---- the fixtures the CPU and the GPU tests share (tests/test_cg_host.py asserts their conditions) ----
_FIX = {}


def demo_fixtures():
    """From the committed demo (tests/golden/demo): the 950 markers of demo.ma that have statistics (n = 300), their LD matrix
    cov(geno[:, ok], ddof=0) made exactly symmetric, its leading 333 x 333 block (odd m: every other column starts 8 bytes off a
    16-byte boundary) and its host chi^2 <= 5 thresholding (9 % of the entries stored)."""
    if _FIX:
        return _FIX
    import os

    import scipy.sparse as sp

    import hibayes_amd as H
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "demo", "demo")
    geno = H.read_plink(d)["geno"]
    rows = [l.split() for l in open(d + ".ma")][1:]
    f = lambda x: float(x) if x != "NA" else np.nan
    ss = np.array([[f(r[3]), f(r[4]), f(r[5]), f(r[7])] for r in rows])
    ok = ~np.isnan(ss).any(axis=1)
    ss = ss[ok]
    ld = np.cov(geno[:, ok].astype(np.float64), rowvar=False, ddof=0)
    ld = np.asfortranarray(np.triu(ld) + np.triu(ld, 1).T)          # (exactly symmetric whatever the BLAS did)
    dg = np.sqrt(np.diag(ld))
    with np.errstate(all="ignore"):
        r = ld / np.outer(dg, dg)
        A = sp.csc_matrix(np.where(r * r * 300 <= 5.0, 0.0, ld))
    A.sort_indices()
    m = ld.shape[0]
    _FIX.update(geno=geno, ok=ok, ss=ss, ld=ld, ss333=ss[:333], ld333=np.asfortranarray(ld[:333, :333]), sp=A,
                lamvec=np.random.default_rng(5).uniform(1.0, 2.0, m))
    return _FIX


def trajectory_cases():
    """name -> (sumstat, matrix, lambda): the cases whose whole trajectory the device must reproduce"""
    F = demo_fixtures()
    m = F["ld"].shape[0]
    return {"dense950_lambda1": (F["ss"], F["ld"], np.full(m, 1.0)),
            "dense950_lambda950": (F["ss"], F["ld"], np.full(m, float(m))),       # lambda = m (1 / h2 - 1), h2 = 0.5
            "dense950_lambda_vector": (F["ss"], F["ld"], F["lamvec"]),
            "dense333_lambda1": (F["ss333"], F["ld333"], np.full(333, 1.0)),
            "sparse950_lambda1": (F["ss"], F["sp"], np.full(m, 1.0))}


def both_orders(name):
    """the restatement of a trajectory case under its two summation orders, computed once"""
    key = "traj_" + name
    if key not in _FIX:
        ss, A, lam = trajectory_cases()[name]
        _FIX[key] = (conjgt_restatement(ss, A, lam, matvec=matvec_plain), conjgt_restatement(ss, A, lam, matvec=matvec_reversed_chunks))
    return _FIX[key]


def spread(r0, r1):
    """the largest relative difference between two runs' err_hist, g, vg and ve (relative to the largest |.| of each)"""
    if r0["iterations"] != r1["iterations"]:
        return math.inf
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(np.asarray(a))))
    return max(float(np.max(np.abs(r0["err_hist"] - r1["err_hist"]) / np.abs(r0["err_hist"]))), rel(r0["g"], r1["g"]),
               rel([r0["vg"]], [r1["vg"]]), rel([r0["ve"]], [r1["ve"]]))
