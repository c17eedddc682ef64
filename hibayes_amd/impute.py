"""ssbrm()'s imputation on the device (reference R/ssbayes.r:295-307): Mn = solve(A^-1_nn, -A^-1_ng M) without a factor.

`impute_device()`  a batched conjugate-gradient solve with the Jacobi preconditioner (hb_impute.hip): every marker column
                   is a right-hand side, the columns of a block advance in lockstep, a column that has converged is frozen.
`ImputeSystem`     the two matrices on the device, for several solves of one system
"""
import ctypes as ct
import time

import numpy as np

from . import _lib

STAT_FIELDS = ("width", "iterations", "blocks", "parts", "cached", "looks", "max_residual", "seconds", "product_seconds", "product_bytes")


def _compressed(A, fmt, name):
    """(indptr int64, indices int32, data float64, shape) of a scipy sparse matrix in canonical CSC / CSR, or of a
    (indptr, indices, data, shape) tuple passed on as it is — the library validates it."""
    if isinstance(A, (tuple, list)) and len(A) == 4:
        indptr, indices, data, shape = A
    else:
        import scipy.sparse as sp
        if not sp.issparse(A):
            A = sp.csr_matrix(np.asarray(A, dtype=np.float64))
        A = (sp.csc_matrix if fmt == "csc" else sp.csr_matrix)(A, dtype=np.float64, copy=True)
        A.sum_duplicates()
        A.sort_indices()
        indptr, indices, data, shape = A.indptr, A.indices, A.data, A.shape
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    data = np.ascontiguousarray(data, dtype=np.float64)
    major = shape[1] if fmt == "csc" else shape[0]
    if indptr.size != major + 1 or indices.size != data.size or indices.size < int(indptr[-1]):
        raise _lib.HibayesError(1, "%s: indptr, indices and data do not describe a %d x %d matrix" % (name, shape[0], shape[1]))
    return indptr, indices, data, (int(shape[0]), int(shape[1]))


class ImputeSystem:
    """A^-1_nn (q x q, symmetric, both triangles) and A^-1_ng (q x n_g) on the device: hb_impute_create / _solve / _destroy."""

    def __init__(self, Ai_nn, Ai_ng, device=0):
        self._h = ct.c_void_p()
        nn = _compressed(Ai_nn, "csc", "A_nn")
        ng = _compressed(Ai_ng, "csr", "A_ng")
        if nn[3][0] != nn[3][1]:
            raise _lib.HibayesError(1, "hb_impute_create: A_nn must be square")
        self.q, self.n_g = nn[3][0], ng[3][1]
        L = _lib.lib()
        _lib.check(L.hb_impute_create(self.q, nn[0].ctypes.data, nn[1].ctypes.data, nn[2].ctypes.data, ng[3][0], self.n_g, ng[0].ctypes.data,
                                      ng[1].ctypes.data, ng[2].ctypes.data, int(device), ct.byref(self._h)))

    def solve(self, M, tol=1e-12, max_iter=10000, out=None):
        """M: n_g x k (a column-major array is taken as it is). Returns (Mn, stats): Mn q x k column-major (`out`, when given)."""
        M = np.asarray(M, dtype=np.float64)
        if M.ndim == 1:
            M = M[:, None]
        if M.ndim != 2 or M.shape[0] != self.n_g or M.shape[1] < 1:
            raise _lib.HibayesError(1, "hb_impute_solve: M must have n_g = %d rows and at least one column" % self.n_g)
        if not M.flags.f_contiguous:
            M = np.asfortranarray(M)
        k = M.shape[1]
        if out is None:
            out = np.empty((self.q, k), dtype=np.float64, order="F")
        if out.shape != (self.q, k) or out.dtype != np.float64 or not out.flags.f_contiguous:
            raise _lib.HibayesError(1, "hb_impute_solve: the output must be a column-major q x k array of doubles")
        st = _lib.ImputeStats()
        ld, ld_out = (M.strides[1] // 8, out.strides[1] // 8) if k > 1 else (self.n_g, self.q)  # (a single column's stride says nothing)
        rc = _lib.lib().hb_impute_solve(self._h, M.ctypes.data, ld, k, float(tol), int(max_iter), out.ctypes.data, ld_out, ct.byref(st))
        _lib.check(rc)
        return out, {f: getattr(st, f) for f in STAT_FIELDS}

    def close(self):
        if self._h:
            _lib.lib().hb_impute_destroy(self._h)
            self._h = ct.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def impute_device(Ai_nn, Ai_ng, M, tol=1e-12, max_iter=None, chunk=512, device=0):
    """Mn = solve(Ai_nn, -Ai_ng M) on the device. Ai_nn: q x q symmetric positive definite (scipy sparse, both triangles), Ai_ng: q x n_g,
    M: n_g x m (or one column). A column stops at ||r|| <= tol ||b||; a zero column comes back exactly zero. `chunk`: marker columns per call
    of the library (the host copies one chunk at a time; the library cuts it into its own blocks). `max_iter` (default 10000): a column still
    live then raises HibayesError — a partial result is never returned.
    Returns (Mn, stats): stats = width, iterations (the slowest block's), blocks, parts, cached, looks, max_residual (the largest true
    relative residual, from one more product after the stop), seconds, setup_seconds, product_seconds, product_bytes."""
    if max_iter is None:
        max_iter = 10000
    M = np.asarray(M, dtype=np.float64)
    one = M.ndim == 1
    if one:
        M = M[:, None]
    t0 = time.perf_counter()
    with ImputeSystem(Ai_nn, Ai_ng, device) as S:
        setup = time.perf_counter() - t0
        m = M.shape[1] if M.ndim == 2 else 0
        Mn = np.empty((S.q, m), dtype=np.float64, order="F")
        total = None
        for c0 in range(0, max(m, 1), max(1, int(chunk))):
            c1 = min(m, c0 + max(1, int(chunk)))
            _, st = S.solve(M[:, c0:c1], tol, max_iter, out=Mn[:, c0:c1])
            if total is None:
                total = st
            else:
                for f in ("iterations", "max_residual", "product_seconds"):
                    total[f] = max(total[f], st[f])
                for f in ("blocks", "looks", "seconds"):
                    total[f] += st[f]
    total["setup_seconds"] = setup
    return (Mn[:, 0] if one else Mn), total
