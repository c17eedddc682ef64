"""The device imputation's algorithm (hibayes_amd/csrc/hb_impute.hip) restated in numpy: a batched conjugate-gradient solve
of A_nn X = -A_ng M with the Jacobi preconditioner, all columns advancing in lockstep, a column frozen where it stops. It defines what the
device computes — the set-up, the stop rule, the freeze, the errors, the true residual — and calls no product code.

Every per-column quantity is formed from that column alone, by operations whose order does not depend on the block: the sparse products add a
row's stored entries in storage order, the dot products reduce one contiguous copy of the column. So a column has the same bits alone, in any
block and at any position, as on the device."""
import numpy as np
import scipy.sparse as sp


class NotPositiveDefinite(ValueError):
    pass


class NotConverged(RuntimeError):
    def __init__(self, live, cols, max_iter):
        super().__init__("%d of %d columns did not converge within %d iterations" % (live, cols, max_iter))
        self.live = live


def coldot(a, b):
    """per-column a . b of two q x k blocks: each column reduced on its own, as one contiguous vector"""
    return np.add.reduce(np.ascontiguousarray((a * b).T), axis=1)


def pcg_batched(A_nn, A_ng, M, tol, max_iter):
    """Returns dict(x, iterations (until every column had stopped), col_iterations, residual (per column, true, relative 2-norm),
    max_residual, bnorm). A_nn: q x q symmetric CSC; A_ng: q x n_g CSR; M: n_g x k."""
    A = sp.csr_matrix(A_nn)  # (symmetric: the rows are the CSC columns)
    A.sort_indices()
    G = sp.csr_matrix(A_ng)
    G.sort_indices()
    M = np.asarray(M, dtype=np.float64)
    if M.ndim == 1:
        M = M[:, None]
    M = np.ascontiguousarray(M)
    if not (0.0 < tol < 1.0):
        raise ValueError("tol must lie inside (0, 1)")
    if max_iter < 1:
        raise ValueError("max_iter must be at least 1")
    k = M.shape[1]
    dinv = (1.0 / A.diagonal())[:, None]
    b = -(G @ M)
    x = np.zeros_like(b)
    r = b.copy()
    p = dinv * r
    bb = coldot(b, b)
    rz = coldot(r, p)
    tol2 = tol * tol
    live = ~(bb <= tol2 * bb)  # a zero column stops before the first iteration, x = 0: no 0 / 0 is formed
    col_it = np.zeros(k, dtype=np.int64)
    it = 0
    while live.any():
        if it >= max_iter:
            raise NotConverged(int(live.sum()), k, max_iter)
        L = np.flatnonzero(live)
        Ap = A @ np.ascontiguousarray(p[:, L])
        pAp = coldot(p[:, L], Ap)
        if not np.all(pAp > 0.0):
            raise NotPositiveDefinite("p'Ap <= 0 at iteration %d: the matrix is not positive definite" % it)
        alpha = rz[L] / pAp
        x[:, L] = x[:, L] + alpha * p[:, L]
        rL = r[:, L] - alpha * Ap
        r[:, L] = rL
        zL = dinv * rL
        rr = coldot(rL, rL)
        rz_new = coldot(rL, zL)
        it += 1
        stop = rr <= tol2 * bb[L]
        col_it[L[stop]] = it
        live[L[stop]] = False  # frozen: x of these columns is never touched again
        go = ~stop
        beta = rz_new[go] / rz[L[go]]
        p[:, L[go]] = zL[:, go] + beta * p[:, L[go]]
        rz[L] = rz_new
    res = b - A @ x
    rn, bn = np.sqrt(coldot(res, res)), np.sqrt(bb)
    rel = np.where(bn > 0, rn / np.where(bn > 0, bn, 1.0), 0.0)
    return {"x": x, "iterations": int(col_it.max()) if k else 0, "col_iterations": col_it, "residual": rel, "max_residual": float(rel.max()) if k else 0.0,
            "bnorm": bn}


def pedigree(generations, family, size, seed):
    """(s, d): 1-based parents (0 = unknown), parents first. `size` founders, then `generations` generations of `size` individuals each: every
    generation's sires are size / family individuals of the previous one with `family` offspring each, its dams are drawn at random from the
    REST of the previous generation. (An individual that is sire and dam of the same offspring must not occur: make_Ainv() writes the
    reference's rule for that case, 1.5 instead of 2 on the parent's diagonal, and 19 such offspring among 20 000 leave A^-1_nn with an
    eigenvalue of -6e-4 — conjugate gradients then meet p'Ap <= 0.)"""
    rng = np.random.default_rng(seed)
    s, d = [np.zeros(size, dtype=np.int64)], [np.zeros(size, dtype=np.int64)]
    first = 0
    for _ in range(generations):
        prev = np.arange(first, first + size) + 1
        sires = rng.choice(prev, max(1, size // family), replace=False)
        s.append(np.resize(np.repeat(sires, family), size))
        d.append(rng.choice(np.setdiff1d(prev, sires), size))
        first += size
    return np.concatenate(s), np.concatenate(d)


def split(Ai, genotyped):
    """(A_nn as CSC, A_ng as CSR, n_indx) of A^-1 for the genotyped individuals' positions"""
    Ai = sp.csr_matrix(Ai)
    is_g = np.zeros(Ai.shape[0], dtype=bool)
    is_g[genotyped] = True
    n_indx = np.flatnonzero(~is_g)
    Ann = Ai[n_indx][:, n_indx].tocsc()
    Ang = Ai[n_indx][:, np.asarray(genotyped)].tocsr()
    for X in (Ann, Ang):
        X.sum_duplicates()
        X.sort_indices()
    return Ann, Ang, n_indx
