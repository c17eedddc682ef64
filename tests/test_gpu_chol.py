"""The device Cholesky inverse (hibayes_amd/csrc/hb_chol.hip, hibayes_amd/chol.py): the factorisation, the factor's inverse and the whole inverse,
stage by stage; matrices that are not positive definite; grm_inverse() end to end. Every error measure is asserted against the same measure of
LAPACK's own pipeline (dpotrf -> dtrtri / dpotri -> mirror, tests/chol_restatement.py) on the same matrix, computed here, by the rule of
tests/test_gpu_eig.py: device <= MARGIN * LAPACK + n, in units of eps. Both pipelines are the same backward-stable algorithm and differ in
blocking and summation order only, hence MARGIN = 4; the floor n is there because LAPACK's value can be luckily small (its resR is 0.5-2.5 eps on
the well-conditioned matrices and 0.02-0.1 eps on the graded and demo ones). HB_CHOL_ACCURACY_OUT=<file> appends every measured pair to it
(profiles/chol_accuracy.txt was written that way)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import hibayes_amd as H
from hibayes_amd import eig as HE

import chol_restatement as R

pytestmark = pytest.mark.gpu
MARGIN = 4
NB = 64  # HB_CHOL_NB of hb_cholplan.hpp, the tile edge as well
SB = 256  # HB_CHOL_SB: the factor's inverse goes by super-blocks of four panels
# one block short of full, exactly one, a one-row panel with a 1 x 1 trailing matrix, ragged last tiles, several tiles over several panels; and the
# same edges of a super-block: one short of full, exactly one, a second one of a single row, a ragged second one of several panels
SIZES = (1, 2, NB - 1, NB, NB + 1, 2 * NB + 1, SB - 1, SB, SB + 1, 6 * NB + 7)
KINDS = ("well", "graded")
SENTINEL = 777.25


def judge(case, n, measures):
    """measures: {name: (device, LAPACK)} in eps. Prints and records every pair, then asserts all of them."""
    lines = ["%-34s n=%-4d %-5s device %10.3f eps   LAPACK %10.3f eps   bound %9.2f" % (case, n, k, a, b, MARGIN * b + n) for k, (a, b) in measures.items()]
    print("\n".join(lines))
    out = os.environ.get("HB_CHOL_ACCURACY_OUT")
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")
    bad = {k: v for k, v in measures.items() if not v[0] <= MARGIN * v[1] + n}
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def matrix(kind, n):
    A = R.well_conditioned(n, 1000 + n) if kind == "well" else R.graded(n, 2000 + n)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def reference(kind, n):
    """LAPACK's stages on matrix(kind, n) and their measures, computed once"""
    B = matrix(kind, n)
    L, info = R.lapack_factor(B)
    assert info == 0
    Li = R.lapack_invert_factor(L)
    X, info = R.lapack_inverse(B)
    assert info == 0
    return {"fac": R.fac(B, L), "tri": R.tri(L, Li), "resR": R.res_right(B, X), "resL": R.res_left(B, X)}


def bits(M):
    return np.ascontiguousarray(M).view(np.int64)


class Dev:
    """An n x n matrix on the device with any leading dimension lda >= n: a flat device buffer (an even-sided square of the upload interface) that holds
    entry (i, j) at j * lda + i. Everything else in the buffer is a sentinel that no call may change."""

    def __init__(self, A, lda):
        A = np.asarray(A, dtype=np.float64)
        self.n, self.lda = A.shape[0], int(lda)
        m = int(np.ceil(np.sqrt(self.lda * self.n)))
        m += m & 1
        flat = np.full(m * m, SENTINEL)
        flat[:self.lda * self.n].reshape((self.lda, self.n), order="F")[:self.n, :] = A
        self.flat = flat.copy()
        self.D = HE.upload(flat.reshape((m, m), order="F"))
        assert self.D.ld == m
        self.ptr = self.D.ptr

    def get(self):
        """the matrix; asserts the buffer's other entries are untouched"""
        flat = self.D.toarray().ravel(order="F")
        body = flat[:self.lda * self.n].reshape((self.lda, self.n), order="F")
        want = self.flat[:self.lda * self.n].reshape((self.lda, self.n), order="F")
        assert np.array_equal(body[self.n:, :], want[self.n:, :]) and np.array_equal(flat[self.lda * self.n:], self.flat[self.lda * self.n:])
        return np.asfortranarray(body[:self.n, :])

    def factor(self, lam=0.0):
        info = C.c_int32(-1)
        HE.check(H.lib().hb_chol_factor(self.ptr, self.lda, self.n, 0, float(lam), C.byref(info)))
        return info.value

    def invert_factor(self):
        HE.check(H.lib().hb_chol_invert_factor(self.ptr, self.lda, self.n, 0))

    def inverse(self, lam=0.0):
        info = C.c_int32(-1)
        HE.check(H.lib().hb_spd_inverse(self.ptr, self.lda, self.n, 0, float(lam), C.byref(info)))
        return info.value

    def close(self):
        self.D.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def ldas(n):
    return (n + (n & 1), n + 6)


def with_nan_above(A):
    B = np.array(A, order="F")
    B[np.triu_indices_from(B, 1)] = np.nan
    return B


# ---- stage by stage ----
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_factor_then_invert_factor(kind, n):
    """hb_chol_factor: fac against dpotrf's; the strict upper triangle is neither read (NaN there changes no bit of L) nor written (it is still
    NaN). hb_chol_invert_factor on the result: tri against dtrtri's, and the upper triangle is still NaN."""
    B, ref = matrix(kind, n), reference(kind, n)
    up = np.triu_indices(n, 1)
    for lda in ldas(n):
        with Dev(B, lda) as clean, Dev(with_nan_above(B), lda) as d:
            assert clean.factor() == 0 and d.factor() == 0
            Lc, Ln = clean.get(), d.get()
            assert np.isnan(Ln[up]).all()
            assert np.array_equal(bits(np.tril(Ln)), bits(np.tril(Lc)))
            assert np.array_equal(bits(Lc[up]), bits(B[up]))  # (not written either)
            L = np.tril(Ln)
            d.invert_factor()
            Xn = d.get()
            assert np.isnan(Xn[up]).all()
            X = np.tril(Xn)
        judge("%s lda=%d" % (kind, lda), n, {"fac": (R.fac(B, L), ref["fac"]), "tri": (R.tri(L, X), ref["tri"])})


def test_factor_applies_lambda_as_the_host_would():
    n, lam = 2 * NB + 1, 0.375
    B = matrix("well", n)
    with Dev(B, n + 1) as a, Dev(R.shifted(B, lam), n + 1) as b:
        assert a.factor(lam) == 0 and b.factor(0.0) == 0
        assert np.array_equal(bits(a.get()), bits(b.get()))
    L, info = H.chol_factor(B, lam)
    assert info == 0 and not L[np.triu_indices(n, 1)].any()
    sign, logdet = np.linalg.slogdet(R.shifted(B, lam))
    assert sign == 1.0 and abs(2.0 * np.log(np.diag(L)).sum() - logdet) <= 1e-12 * abs(logdet) + 1e-12


# ---- the inverse ----
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_spd_inverse(kind, n):
    """resR and resL against LAPACK's; X equals its transpose bit for bit; a second run gives the same bits; only the lower triangle is read"""
    B, ref = matrix(kind, n), reference(kind, n)
    first = None
    for lda in ldas(n):
        with Dev(B, lda) as d, Dev(with_nan_above(B), lda) as e:
            assert d.inverse() == 0 and e.inverse() == 0
            X, X2 = d.get(), e.get()
        assert np.array_equal(bits(X), bits(X.T))
        assert np.array_equal(bits(X), bits(X2))
        if first is None:
            first = X
        assert np.array_equal(bits(X), bits(first))  # (nor do the bits depend on the leading dimension)
        judge("%s lda=%d" % (kind, lda), n, {"resR": (R.res_right(B, X), ref["resR"]), "resL": (R.res_left(B, X), ref["resL"])})


@pytest.mark.parametrize("n", (1, NB + 1, 4 * NB + 1))
def test_spd_inverse_applies_lambda_as_the_host_would(n):
    lam = 0.25
    A = matrix("graded", n)
    B = R.shifted(A, lam)
    with Dev(A, n + 6) as a, Dev(B, n + 6) as b:
        assert a.inverse(lam) == 0 and b.inverse(0.0) == 0
        X = a.get()
        assert np.array_equal(bits(X), bits(b.get()))
    Xl, info = R.lapack_inverse(B)
    assert info == 0
    judge("graded + %.2f I" % lam, n, {"resR": (R.res_right(B, X), R.res_right(B, Xl)), "resL": (R.res_left(B, X), R.res_left(B, Xl))})
    assert np.array_equal(bits(H.spd_inverse(A, lam)), bits(X))


@pytest.fixture(scope="module")
def demo_grm(demo):
    X = np.ascontiguousarray(demo["plink"]["geno"])
    G = H.make_grm(X, verbose=False)
    assert G.shape == (600, 600)
    return {"X": X, "G": G}


@pytest.mark.parametrize("lam", (0.01, 1e-6))
def test_spd_inverse_of_the_demo_grm(demo_grm, lam):
    G = demo_grm["G"]
    B = R.shifted(G, lam)
    Xl, info = R.lapack_inverse(B)
    assert info == 0
    X = H.spd_inverse(G, lam)
    assert X.flags.f_contiguous and np.array_equal(bits(X), bits(X.T))
    judge("demo GRM + %g I" % lam, 600, {"resR": (R.res_right(B, X), R.res_right(B, Xl)), "resL": (R.res_left(B, X), R.res_left(B, Xl))})


def test_spd_inverse_of_a_device_matrix_in_place():
    B = matrix("well", NB + 1)
    want = H.spd_inverse(B)
    with HE.upload(B) as D:
        got = H.spd_inverse(D, keep_on_device=True)
        assert got is D and np.array_equal(bits(D.toarray()), bits(want))


# ---- not positive definite ----
@pytest.mark.parametrize("p", (0, NB - 1, NB, 2 * NB + 1))
def test_a_minor_that_is_not_positive_definite_is_reported_not_raised(p):
    """info is LAPACK's: the order of the leading minor. A NaN pivot counts (asserted of the device alone: the OpenBLAS behind scipy lets it
    pass). hb_spd_inverse then leaves the matrix as it was, and spd_inverse() takes solver_lu()'s route."""
    n = 2 * NB + 2
    for bad in (-1.0, np.nan):
        E = np.eye(n, order="F")
        E[p, p] = bad
        if bad < 0:
            assert R.lapack_factor(E)[1] == p + 1
        for lda in ldas(n):
            with Dev(E, lda) as d:
                assert d.factor() == p + 1
            with Dev(E, lda) as d:
                assert d.inverse() == p + 1
                assert np.array_equal(bits(d.get()), bits(E))
        L, info = H.chol_factor(E)
        assert info == p + 1
    E = np.eye(n)
    E[p, p] = -1.0
    X = H.spd_inverse(E)
    assert np.array_equal(X, E)  # diag(+-1) is its own inverse
    with HE.upload(E) as D:
        assert H.spd_inverse(D, keep_on_device=True) is D and np.array_equal(D.toarray(), E)
    with pytest.raises(ValueError, match="matrix is not invertible"):
        H.spd_inverse(np.zeros((3, 3)))


def test_a_work_buffer_that_does_not_fit_is_out_of_memory():
    """the second n x n matrix of n = 10^6 is 8 TB: refused when it is allocated, before any kernel is launched on the (tiny) matrix"""
    with HE.upload(np.eye(2)) as D:
        info = C.c_int32(-1)
        rc = H.lib().hb_spd_inverse(D.ptr, 1000000, 1000000, 0, 0.0, C.byref(info))
        assert rc == 3 and "out of memory" in H.lib().hb_last_error().decode()
        assert np.array_equal(D.toarray(), np.eye(2))


# ---- end to end ----
def test_grm_inverse_end_to_end(demo_grm):
    X, G, lam = demo_grm["X"], demo_grm["G"], 0.01
    B = R.shifted(G, lam)
    Xl, info = R.lapack_inverse(B)
    assert info == 0
    Gi = H.grm_inverse(X, lam, verbose=False)
    assert Gi.flags.f_contiguous and Gi.shape == (600, 600) and np.array_equal(bits(Gi), bits(Gi.T))
    judge("grm_inverse(demo, %g)" % lam, 600, {"resR": (R.res_right(B, Gi), R.res_right(B, Xl)), "resL": (R.res_left(B, Gi), R.res_left(B, Xl))})
    assert np.array_equal(bits(Gi), bits(H.spd_inverse(G, lam)))  # G went from hb_grm_build to hb_spd_inverse with the bits make_grm() downloads
    with H.Context(X.shape[0], X.shape[1]) as ctx:
        ctx.upload(X)
        assert np.array_equal(bits(H.grm_inverse(ctx, lam, verbose=False)), bits(Gi))
        with H.grm_inverse(ctx, lam, verbose=False, keep_on_device=True) as D:
            assert isinstance(D, HE.DeviceMatrix) and D.shape == (600, 600)
            assert np.array_equal(bits(D.toarray()), bits(Gi))
