"""A numpy restatement of the reference's ldmat() arithmetic (BigStat, tXXmat_Geno, tXXmat_Chr: src/tXXmat.cpp:43-77, :100-206,
:504-626) for the LD-matrix tests — a helper, not a test. Every operation is one IEEE fp64 operation on whole arrays, in the
reference's order, so the result equals a literal loop's in every bit (test_ldmat_host.py checks that):
  * xx = sqrt(sum_k (x_k - mean)^2) with the squares added one row at a time;
  * `p12 -= sum1 * m2 + sum2 * m1 - ind * m1 * m2` with the marker of the SMALLER index in the sum1 / m1 role — (ind * m1) * m2 is
    not symmetric in the two markers;
  * dense results carry xx * xx / ind on the diagonal, sparse ones send the diagonal through the formula and the threshold;
  * `r * r * ind <= chisq` drops an entry, so a NaN r (monomorphic marker) keeps it.
Returns the dense m x m array with zeros where the reference stores nothing."""
import numpy as np


def big_stat(X):
    Xd = np.asarray(X, dtype=np.float64)
    n, m = Xd.shape
    s = Xd.sum(axis=0)                 # small integers: exact in any order
    mean = s / n
    p1 = np.zeros(m)
    for k in range(n):                 # serial in k, as the reference's inner loop
        d = Xd[k] - mean
        p1 += d * d
    return s, mean, np.sqrt(p1)


def ldmat_restatement(X, chisq=None, chr=None):
    """chr None: tXXmat_Geno (sparse iff chisq > 0); chr given: tXXmat_Chr (sparse iff chisq is not None)."""
    Xd = np.asarray(X, dtype=np.float64)
    n, m = Xd.shape
    ind = float(n)
    s, mean, xx = big_stat(Xd)
    G = Xd.T @ Xd                      # integer cross-products below 2^53: exact
    idx = np.arange(m)
    lo, hi = np.minimum.outer(idx, idx), np.maximum.outer(idx, idx)
    sj, mj, xj, si, mi, xi = s[lo], mean[lo], xx[lo], s[hi], mean[hi], xx[hi]
    p12 = G - (((sj * mi) + (si * mj)) - ((ind * mj) * mi))
    val = p12 / ind
    sparse = (chisq is not None) if chr is not None else (chisq is not None and chisq > 0)
    if sparse:
        with np.errstate(invalid="ignore", divide="ignore"):
            r = p12 / (xj * xi)
            drop = (r * r) * ind <= chisq          # False for NaN: kept
        val = np.where(drop, 0.0, val)
    else:
        np.fill_diagonal(val, (xx * xx) / ind)
    if chr is not None:
        c = np.asarray(chr)
        val[c[:, None] != c[None, :]] = 0.0
    return np.asfortranarray(val)
