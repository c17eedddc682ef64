"""make_grm(): the genomic relationship matrix of the reference (src/rm.cpp:5-53) from genotypes resident on the device.

The n x n matrix G = Z Z' / mean(diag(Z Z')), Z the column-centred genotypes, is built by hb_grm_build (hand-written gfx950 kernels:
exact int8 cross-products on the matrix cores, one fixed fp64 expression per entry). The eigen-decomposition
ibrm()'s BSLMM needs (R/bayes.r:292-294) is numpy.linalg.eigh — LAPACK's dsyevd, the routine the reference calls (eigen_sym_dc) — by
default, or with eigen_solver="device" hibayes_amd.eig: the matrix then stays where hb_grm_build left it and only the tridiagonal stage
runs on the host.
"""
import ctypes as C

import numpy as np

from ._lib import check, lib

HB_GRM_RAW = 1


def grm_build(ctx, lambda_=0.0, raw=False):
    """hb_grm_build on an engine.Context that holds int8 columns: the n x n matrix as a Fortran-ordered array."""
    G = np.zeros((ctx.n, ctx.n), order="F")
    check(lib().hb_grm_build(ctx.h, float(lambda_), HB_GRM_RAW if raw else 0, G.ctypes.data, None))
    return G


def grm_build_device(ctx, lambda_=0.0):
    """hb_grm_build with the matrix left on the device: an eig.DeviceMatrix (leading dimension n)"""
    from .eig import DeviceMatrix
    p = C.c_void_p()
    check(lib().hb_grm_build(ctx.h, float(lambda_), 0, None, C.byref(p)))
    return DeviceMatrix(p.value, ctx.n, ctx.n, ctx.device, free="hb_grm_free")


def make_grm(M, lambda_=0.0, inverse=False, eigen=False, verbose=True, *, device=0, eigen_solver="host", keep_on_device=False, tridiagonal="host"):
    """Mirror of make_grm() (reference src/rm.cpp:5-53). `M` is the n x m genotype matrix (int8 preferred, or integer-valued floats)
    or an engine.Context with the genotypes already resident. Returns G, or with eigen=True the pair (eigenvalues, eigenvectors) in
    numpy.linalg.eigh's ascending order. As in the reference, `lambda_` is added to the diagonal before the decomposition (:46) and
    is not part of the plain G. inverse=True (solve(), :39-42) is not routed through make_grm(): grm_inverse() (hibayes_amd/chol.py) returns it.
    eigen_solver: "host" (default) decomposes G with numpy.linalg.eigh; "device" with hibayes_amd.eig — G goes from hb_grm_build straight
    into the reduction and never visits the host. keep_on_device=True (eigen_solver="device" only) returns an eig.EigVectors handle
    (.values, .toarray(), .close()) instead of the pair, for Context.poly_setup(). tridiagonal (eigen_solver="device" only): "host" (default)
    solves the tridiagonal stage with LAPACK dstemr on one host thread; "device" with the device's divide and conquer (eig.tridiagonal_eigh_device),
    so that no n x n matrix crosses the bus."""
    if eigen_solver not in ("host", "device"):
        raise ValueError("make_grm: eigen_solver must be \"host\" or \"device\", not %r" % (eigen_solver,))
    from .eig import check_tridiagonal
    check_tridiagonal("make_grm", tridiagonal, eigen_solver)
    if keep_on_device and not (eigen and eigen_solver == "device"):
        raise ValueError("make_grm: keep_on_device=True goes with eigen=True, eigen_solver=\"device\"")
    if inverse:
        raise NotImplementedError("make_grm(inverse=True) (solve(), src/rm.cpp:39-42) is not routed through make_grm(): call grm_inverse()")
    from .engine import Context
    own = not isinstance(M, Context)
    if own:
        M = np.asarray(M)
        if M.ndim != 2:
            raise ValueError("make_grm: M must be an n x m matrix")
        ctx = Context(M.shape[0], M.shape[1], device=device)
    else:
        ctx = M
    try:
        if own:
            ctx.upload(M)
        if verbose:
            print("Start construct G matrix for %d individuals using %d markers" % (ctx.n, ctx.m))
            print("Compute Z * Z'")
        if eigen and eigen_solver == "device":
            G = grm_build_device(ctx, lambda_)
        else:
            G = grm_build(ctx, lambda_ if eigen else 0.0)
    finally:
        if own:
            ctx.close()
    if not eigen:
        return G
    if verbose:
        print("Eigen decomposition on G matrix")
    if eigen_solver == "device":
        from .eig import eigh_device
        return eigh_device(G, keep_on_device, tridiagonal=tridiagonal)
    ev, K = np.linalg.eigh(G)
    return ev, np.asfortranarray(K)
