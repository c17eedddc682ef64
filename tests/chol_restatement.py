"""LAPACK's own pipeline for the inverse of a symmetric positive definite matrix — dpotrf(lower) -> dpotri(lower) -> mirror, what solver_chol()
(reference src/solver.cpp:159-202) runs — and the measures tests/test_gpu_chol.py compares the device's stages with, all in units of eps.
A helper, not a test file."""
import numpy as np
from scipy.linalg import lapack

EPS = np.finfo(np.float64).eps


def shifted(A, lam=0.0):
    B = np.array(A, dtype=np.float64, order="F")
    if lam:
        B[np.diag_indices_from(B)] += lam
    return B


def lapack_factor(B):
    """(L, info) of dpotrf('L'): L lower triangular with zeros above"""
    c, info = lapack.dpotrf(np.asfortranarray(B), lower=1, clean=1)
    return np.asfortranarray(np.tril(c)), int(info)


def lapack_invert_factor(L):
    """dtrtri('L', 'N')"""
    x, info = lapack.dtrtri(np.asfortranarray(L), lower=1, unitdiag=0)
    assert info == 0
    return np.asfortranarray(np.tril(x))


def lapack_inverse(B):
    """dpotrf -> dpotri -> the mirror of src/solver.cpp:194-198; (X, info)"""
    c, info = lapack.dpotrf(np.asfortranarray(B), lower=1, clean=0)
    if info:
        return None, int(info)
    x, info = lapack.dpotri(c, lower=1)
    assert info == 0
    x = np.tril(x)
    return np.asfortranarray(x + np.tril(x, -1).T), 0


def norm2(M):
    return float(np.linalg.norm(M, 2))


def res_right(B, X):
    """max|B X - I| / (||B||_2 ||X||_2), in eps"""
    n = B.shape[0]
    return float(np.abs(B @ X - np.eye(n)).max() / (norm2(B) * norm2(X)) / EPS)


def res_left(B, X):
    return res_right(X, B)


def fac(B, L):
    """max|L L' - B| over the lower triangle / ||B||_2, in eps (B: symmetric, or only its lower triangle meaningful)"""
    Bl = np.tril(B)
    Bs = Bl + np.tril(Bl, -1).T
    Lt = np.tril(L)
    return float(np.abs(np.tril(Lt @ Lt.T - Bs)).max() / norm2(Bs) / EPS)


def tri(L, Li):
    """max|L L^-1 - I| / (||L||_2 ||L^-1||_2), in eps"""
    n = L.shape[0]
    Lt, Xt = np.tril(L), np.tril(Li)
    return float(np.abs(Lt @ Xt - np.eye(n)).max() / (norm2(Lt) * norm2(Xt)) / EPS)


def bound(lapack_value, n):
    """the accuracy rule of tests/test_gpu_eig.py: 4 x LAPACK's measure on the same matrix + n, in eps"""
    return 4.0 * lapack_value + n


# ---- the matrices ----
def well_conditioned(n, seed):
    """B B' / n + I from a seeded normal B: condition number about 5"""
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, n))
    return np.asfortranarray(B @ B.T / n + np.eye(n))


def graded(n, seed):
    """Q diag(logspace(0, -10, n)) Q', symmetrised: condition number 1e10"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.logspace(0.0, -10.0, n)) @ Q.T
    return np.asfortranarray(0.5 * (A + A.T))


def grm_host(M):
    """make_grm()'s G (reference src/rm.cpp:17-37) in plain numpy, for the tests that run without a device"""
    Z = np.asarray(M, dtype=np.float64)
    Z = Z - Z.mean(axis=0)
    G = Z @ Z.T
    return np.asfortranarray(G / np.mean(np.diag(G)))
