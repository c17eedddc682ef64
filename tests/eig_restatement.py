"""Plain-numpy restatement of the device eigensolver's two stages (hibayes_amd/csrc/hb_eig.hip) in LAPACK dsytrd's convention for uplo = 'L', the
comparison pipeline "LAPACK all the way", and the error measures both are judged by. A helper: no tests here.

Convention: reflector k is H_k = I - tau_k v_k v_k' with v_k[:k + 1] = 0, v_k[k + 1] = 1; for x = A[k + 1:, k] (A as updated by the reflectors before
it), alpha = x[0]: beta = -sign(alpha) ||x||, tau = (beta - alpha) / beta, v[k + 2:] = x[1:] / (alpha - beta); x[1:] exactly zero gives tau = 0, beta =
alpha. Q = H_0 H_1 ... H_{n-2} and Q' A Q = T = tridiag(e, d, e)."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)


def householder_tridiagonal(A):
    """Unblocked reduction (dsytd2, lower). Returns d (n), e (n - 1), V (n x (n - 1), explicit reflector vectors) and tau (n - 1)."""
    A = np.array(A, dtype=np.float64)
    A = np.tril(A) + np.tril(A, -1).T          # only the lower triangle is read
    n = A.shape[0]
    d, e, tau = np.zeros(n), np.zeros(max(n - 1, 0)), np.zeros(max(n - 1, 0))
    V = np.zeros((n, max(n - 1, 0)))
    for k in range(n - 1):
        x = A[k + 1:, k].copy()
        alpha = x[0]
        xn2 = float(np.sum(x[1:] * x[1:]))
        v = np.zeros(n)
        v[k + 1] = 1.0
        if xn2 == 0.0:
            beta, t = alpha, 0.0
        else:
            beta = -np.copysign(np.sqrt(alpha * alpha + xn2), alpha)
            t = (beta - alpha) / beta
            v[k + 2:] = x[1:] / (alpha - beta)
        d[k], e[k], tau[k] = A[k, k], beta, t
        V[:, k] = v
        if t != 0.0:
            # A <- H A H on the trailing square, as dsytd2: w = tau A v - (tau / 2) (tau v'A v) v, A -= v w' + w v'
            p = t * (A @ v)
            w = p - 0.5 * t * (p @ v) * v
            A -= np.outer(v, w) + np.outer(w, v)
    d[n - 1] = A[n - 1, n - 1]
    return d, e, V, tau


def back_transform(V, tau, Z=None):
    """Q Z, reflector by reflector from the last to the first (Z = None: Q itself)."""
    n = V.shape[0]
    K = np.eye(n) if Z is None else np.array(Z, dtype=np.float64)
    for k in range(V.shape[1] - 1, -1, -1):
        if tau[k] != 0.0:
            v = V[:, k]
            K -= tau[k] * np.outer(v, v @ K)
    return K


def tridiagonal_eigh(d, e):
    """The stage both pipelines share: dstemr (scipy.linalg.eigh_tridiagonal), eigenvalues ascending."""
    if len(d) == 1:
        return np.array(d, dtype=np.float64), np.ones((1, 1))
    from scipy.linalg import eigh_tridiagonal
    return eigh_tridiagonal(np.asarray(d, dtype=np.float64), np.asarray(e, dtype=np.float64), lapack_driver="stemr")


def restatement_eigh(A):
    d, e, V, tau = householder_tridiagonal(A)
    w, Z = tridiagonal_eigh(d, e)
    return w, back_transform(V, tau, Z)


def reflectors_from_packed(Ap, tau):
    """The explicit V of a matrix as dsytrd (uplo = 'L') leaves it: column k below the subdiagonal holds v_k[k + 2:]."""
    n = Ap.shape[0]
    V = np.zeros((n, max(n - 1, 0)))
    for k in range(n - 1):
        V[k + 1, k] = 1.0
        V[k + 2:, k] = Ap[k + 2:, k]
    return V


def lapack_tridiagonal(A):
    """scipy.linalg.lapack.dsytrd (lower): (packed matrix, d, e, tau)"""
    from scipy.linalg.lapack import dsytrd
    A = np.asfortranarray(A, dtype=np.float64)
    if A.shape[0] == 1:
        return A.copy(), np.array([A[0, 0]]), np.zeros(0), np.zeros(0)
    c, d, e, tau, info = dsytrd(A, lower=1)
    assert info == 0
    return c, d, e, tau


def lapack_back_transform(c, tau, Z):
    """What dormtr does for side = 'L', uplo = 'L', trans = 'N': dormqr with the n - 1 reflectors stored in c[1:, :n - 1] on the rows 1: of Z
    (scipy wraps dormqr, not dormtr itself)."""
    from scipy.linalg.lapack import dormqr
    n = c.shape[0]
    K = np.array(Z, dtype=np.float64, order="F")
    if n < 2:
        return K
    a = np.asfortranarray(c[1:, :n - 1])
    sub = np.asfortranarray(K[1:, :])
    lwork = max(1, int(dormqr("L", "N", a, tau, sub, -1)[1][0]))
    out, _, info = dormqr("L", "N", a, tau, sub, lwork)
    assert info == 0
    K[1:, :] = out
    return K


def lapack_eigh(A):
    """LAPACK all the way: dsytrd -> the same dstemr -> dormtr. Returns (w, K)."""
    c, d, e, tau = lapack_tridiagonal(A)
    w, Z = tridiagonal_eigh(d, e)
    return w, lapack_back_transform(c, tau, Z)


def norm2(G):
    return float(np.max(np.abs(np.linalg.eigvalsh(G)))) if G.shape[0] > 1 else float(abs(G[0, 0]))


def res_eps(G, w, K):
    """max |G K - K diag(w)| / ||G||_2, in units of eps"""
    return float(np.max(np.abs(G @ K - K * w[None, :]))) / max(norm2(G), 1e-300) / EPS


def orth_eps(K):
    """max |K'K - I|, in units of eps"""
    return float(np.max(np.abs(K.T @ K - np.eye(K.shape[0])))) / EPS


def grm_case(n, m, lam, seed=None):
    """G = Z Z' / mean(diag) + lambda I from random codes 0..2, Z column-centred (make_grm's matrix, formed on the host)"""
    rng = np.random.default_rng(1000 * n + m if seed is None else seed)
    M = rng.integers(0, 3, size=(n, m)).astype(np.float64)
    Z = M - M.mean(axis=0, keepdims=True)
    G = Z @ Z.T
    G = 0.5 * (G + G.T)
    mu = np.mean(np.diag(G))                   # (n = 1: the centred row is zero; the matrix is lambda alone)
    return np.asfortranarray(G / (mu if mu > 0 else 1.0) + lam * np.eye(n))


def grm_cases(nb):
    return [(1, 5, .01), (2, 5, .01), (3, 7, .01), (17, 63, .01), (nb - 1, 200, .01), (nb, 200, .01), (nb + 1, 200, .01), (129, 64, .25),
            (300, 1000, .01), (300, 120, .01), (300, 1000, 0.0), (513, 700, .01)]
