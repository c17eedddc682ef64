"""spd_inverse() / grm_inverse(): the inverse make_grm(inverse=TRUE) returns (reference src/rm.cpp:39-42: solve(), src/solver.cpp:251-259) with
its O(n^3) work on the device (hb_chol_*, hb_spd_inverse; hibayes_amd/csrc/hb_chol.hip):

    hb_chol_factor          dpotrf('L'): a right-looking blocked Cholesky, panels of 64 columns        device
    hb_chol_invert_factor   dtrtri('L', 'N'): the factor's inverse in place                            device
    (inside hb_spd_inverse) dlauum and the mirror: X = L^-T L^-1, both triangles                       device

solve() first tries solver_chol() (:159-202) and, where dpotrf reports a minor that is not positive definite, solver_lu() (:204-249). The first is
hb_spd_inverse; the second stays on the host (solver_lu() below, LAPACK through scipy) and raises the reference's texts.

grm_inverse() builds G with hb_grm_build and inverts it where it lies: on the Cholesky route G never visits the host."""
import ctypes as C

import numpy as np

from ._lib import check, lib
from .eig import DeviceMatrix, upload

EPS = float(np.finfo(np.float64).eps)  # arma::datum::eps
_HINT = "try to specify parameter 'lambda' with a small value, eg: 0.001 or bigger"


def chol_plan(n):
    """hb_chol_plan (hb_cholplan.hpp; needs no device): dict(nb, ldw, factor_bytes, invert_bytes, inverse_bytes, steps [(k0, width, row_tiles,
    tri_tiles)])"""
    cap = max((int(n) + 63) // 64, 1)
    a = [np.zeros(cap, dtype=np.int32) for _ in range(3)]
    tt = np.zeros(cap, dtype=np.int64)
    nb, ns, ldw, by = C.c_int32(), C.c_int32(), C.c_int64(), np.zeros(3, dtype=np.int64)
    check(lib().hb_chol_plan(int(n), cap, C.addressof(nb), C.addressof(ldw), by.ctypes.data, C.addressof(ns), a[0].ctypes.data, a[1].ctypes.data,
                             a[2].ctypes.data, tt.ctypes.data))
    return dict(nb=nb.value, ldw=ldw.value, factor_bytes=int(by[0]), invert_bytes=int(by[1]), inverse_bytes=int(by[2]),
                steps=[(int(a[0][s]), int(a[1][s]), int(a[2][s]), int(tt[s])) for s in range(ns.value)])


def solver_lu(A, lambda_=0.0):
    """solver_lu() of the reference (src/solver.cpp:204-249) on the host: the inverse of A + lambda I by dgetrf, dlange('1'), dgecon and dgetri,
    with its exception texts as ValueError. Needs no device."""
    from scipy.linalg import lapack
    A = np.array(A, dtype=np.float64, order="F")
    if A.ndim != 2 or A.shape[0] != A.shape[1]:
        raise ValueError("solver_lu: A must be a square matrix")
    if lambda_:
        A[np.diag_indices_from(A)] += float(lambda_)
    lu, piv, info = lapack.dgetrf(A, overwrite_a=1)
    if info:
        raise ValueError("matrix is not invertible, " + _HINT)
    anorm = lapack.dlange("1", lu)  # (of the factors, as :226 computes it)
    rcond, info = lapack.dgecon(lu, anorm, norm="1")
    if rcond <= EPS:
        raise ValueError("system is computationally singular: reciprocal condition number = %.6e,\n%s" % (rcond, _HINT))
    inv, info = lapack.dgetri(lu, piv, overwrite_lu=1)
    if info:
        raise ValueError("U matrix of LU decomposition is singular.")
    return np.asfortranarray(inv)


def _device_inverse(D, lambda_):
    """hb_spd_inverse on the DeviceMatrix D, in place; the reported info"""
    D._live("spd_inverse")
    info = C.c_int32()
    check(lib().hb_spd_inverse(D.ptr, D.ld, D.n, D.device, float(lambda_), C.byref(info)))
    return info.value


def _finish(D, own, lambda_, keep_on_device):
    """solve() on the DeviceMatrix D: hb_spd_inverse, or with info > 0 solver_lu() on the untouched matrix"""
    try:
        info = _device_inverse(D, lambda_)
        if info == 0:
            if keep_on_device:
                own = False
                return D
            return D.toarray()
        X = solver_lu(D.toarray(), lambda_)
        if not keep_on_device:
            return X
        new = upload(X, D.device)
        if own:
            return new
        lib_free = getattr(lib(), D._free)
        lib_free(D.ptr)  # the caller's handle now owns the inverse, as on the Cholesky route
        D.ptr, D.ld, D._free = new.ptr, new.ld, new._free
        new.ptr = None
        return D
    finally:
        if own:
            D.close()


def spd_inverse(A, lambda_=0.0, *, device=0, keep_on_device=False):
    """Mirror of solve() (reference src/solver.cpp:251-259): (A + lambda_ I)^-1. `A` is a symmetric host matrix, of which only the lower triangle
    is read on the Cholesky route, or an eig.DeviceMatrix, which is overwritten with the inverse. hb_spd_inverse does the work on the device; where
    it reports a leading minor that is not positive definite, the matrix is untouched and goes through solver_lu() on the host, which raises
    ValueError with the reference's texts for a singular matrix. Returns a Fortran-ordered array equal to its transpose bit for bit (Cholesky
    route), or with keep_on_device=True an eig.DeviceMatrix (A itself where A is one)."""
    if isinstance(A, DeviceMatrix):
        return _finish(A, False, lambda_, keep_on_device)
    return _finish(upload(A, device), True, lambda_, keep_on_device)


def chol_factor(A, lambda_=0.0, *, device=0):
    """(L, info) of hb_chol_factor: dpotrf('L') of A + lambda_ I on the device. L is lower triangular (zeros above); info = 0, or k > 0 where
    the leading minor of order k is not positive definite — L is then what the factorisation left. log|A| = 2 sum(log(diag(L)))."""
    with upload(A, device) as D:
        info = C.c_int32()
        check(lib().hb_chol_factor(D.ptr, D.ld, D.n, D.device, float(lambda_), C.byref(info)))
        return np.asfortranarray(np.tril(D.toarray())), info.value


def grm_inverse(M, lambda_=0.0, verbose=True, *, device=0, keep_on_device=False):
    """What make_grm(Z, lambda, inverse=TRUE) returns (reference src/rm.cpp:5-42): (G + lambda_ I)^-1 for the relationship matrix G of the
    genotypes `M` (n x m, int8 preferred, or an engine.Context that holds them). hb_grm_build leaves G on the device and hb_spd_inverse inverts it
    there; keep_on_device=True returns the eig.DeviceMatrix instead of a Fortran-ordered array."""
    from .engine import Context
    from .grm import grm_build_device
    own = not isinstance(M, Context)
    if own:
        M = np.asarray(M)
        if M.ndim != 2:
            raise ValueError("grm_inverse: M must be an n x m matrix")
        ctx = Context(M.shape[0], M.shape[1], device=device)
    else:
        ctx = M
    try:
        if own:
            ctx.upload(M)
        if verbose:
            print("Start construct G matrix for %d individuals using %d markers" % (ctx.n, ctx.m))
            print("Compute Z * Z'")
        G = grm_build_device(ctx, 0.0)
    finally:
        if own:
            ctx.close()
    if verbose:
        print("Invert the G matrix")
    return _finish(G, True, lambda_, keep_on_device)
