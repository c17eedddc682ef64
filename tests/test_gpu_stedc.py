"""The device's tridiagonal divide and conquer (hibayes_amd/csrc/hb_stedc.hip, eig.tridiagonal_eigh_device) alone, through eigh(), make_grm()
and ibrm(), its determinism and its refusals.

The accuracy rule is tests/test_gpu_eig.py's. Every measure is computed for the device's pair and for LAPACK's divide and conquer on the same T —
numpy.linalg.eigh(tri(d, e)): dsytrd of a tridiagonal matrix is the identity, so that is dstedc on (d, e) — and asserted: device <= 4 * LAPACK + n,
in eps. The algorithm and its first-order bound are the same, only the leaf solver, the secular iteration and the summation order differ, hence
the project's margin of 4; the floor n eps is there because the reference can be luckily small. Measures: res = max|T Z - Z diag(w)| / ||T||_2,
orth = max|Z'Z - I|, values = max|w - w_sterf| / max|w| with w_sterf from dsterf. HB_EIG_ACCURACY_OUT=<file> appends every measured pair to it
(profiles/eig_accuracy.txt was written that way). tests/stedc_restatement.py builds the matrices, each the smallest that forces its case."""
import functools

import numpy as np
import pytest

import hibayes_amd as H
from hibayes_amd import eig as HE

import bslmm_restatement as B
import eig_restatement as E
import stedc_restatement as S
import test_gpu_eig as TG

pytestmark = pytest.mark.gpu
LAMBDA = TG.LAMBDA
KW = TG.KW


@functools.lru_cache(maxsize=None)
def matrices():
    return S.matrices()


@functools.lru_cache(maxsize=None)
def reference(name):
    """LAPACK's measures on the named matrix, computed once"""
    d, e = matrices()[name]
    wl, Zl = S.lapack_dc(d, e)
    return wl, S.measures(d, e, wl, Zl)


def device_pair(d, e):
    w, Zh = HE.tridiagonal_eigh_device(d, e)
    with Zh:
        assert Zh.ld % 64 == 0 and Zh.ld >= len(d) and Zh.shape == (len(d), len(d))
        return w, Zh.toarray()


@pytest.mark.parametrize("name", S.MATRIX_NAMES)
def test_matrices_against_lapacks_divide_and_conquer(name):
    d, e = matrices()[name]
    n = len(d)
    w, Z = device_pair(d, e)
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(Z)) and np.all(np.diff(w) >= 0)
    wl, ref = reference(name)
    m = {k: (v, ref[k]) for k, v in S.measures(d, e, w, Z).items()}
    if name.startswith("toeplitz"):
        exact = S.toeplitz_values(n)
        m["closed form"] = tuple(float(np.max(np.abs(x - exact))) / float(np.max(exact)) / S.EPS for x in (w, wl))      # 2 - 2 cos(k pi / (n + 1))
    TG.judge("stedc " + name, n, m)


def is_permutation(Z):
    return np.all((Z == 0) | (Z == 1)) and np.all(Z.sum(axis=0) == 1) and np.all(Z.sum(axis=1) == 1)


def test_exact_cases():
    d = np.random.default_rng(11).uniform(0.5, 2.0, 131)              # e = 0, d unsorted: every part is 1 x 1
    w, Z = device_pair(d, np.zeros(130))
    assert np.array_equal(w, np.sort(d)) and is_permutation(Z) and np.array_equal(Z.T @ d, w)
    w, Z = device_pair(np.zeros(40), np.zeros(39))
    assert np.all(w == 0) and np.array_equal(Z, np.eye(40))
    w, Z = device_pair(np.full(70, 1.75), np.full(69, 1e-20))         # all splits
    assert np.all(w == 1.75) and is_permutation(Z)


@pytest.mark.parametrize("n,m,lam", E.grm_cases(TG.NB))
def test_eigh_with_the_tridiagonal_stage_on_the_device(n, m, lam):
    """the public route on the project's relationship matrices — n > m among them, where the cluster of n - m equal eigenvalues is what BSLMM
    meets with fewer markers than individuals — judged by test_gpu_eig's pair measures against LAPACK all the way"""
    G = E.grm_case(n, m, lam)
    w, K = H.eigh(G, tridiagonal="device")
    assert K.shape == (n, n) and K.flags.f_contiguous and np.all(np.diff(w) >= 0)
    _, ref = TG.lapack_all(G)
    TG.judge("eigh/stedc grm m=%d lambda=%g" % (m, lam), n, {k: (v, ref[k]) for k, v in TG.pair_measures(G, w, K).items()})


@pytest.mark.parametrize("n,m", [(129, 64), (300, 120)])
def test_make_grm_keeps_everything_on_the_device(n, m):
    M = TG.codes(n, m)
    with H.Context(n, m) as c:
        c.upload(M)
        G = c.grm(lambda_=LAMBDA)
        with H.make_grm(c, LAMBDA, eigen=True, verbose=False, eigen_solver="device", tridiagonal="device", keep_on_device=True) as Kh:
            assert Kh.shape == (n, n) and Kh.ld % 2 == 0 and Kh.ld >= n
            w, K = Kh.values, Kh.toarray()
    assert np.all(np.diff(w) >= 0)
    _, ref = TG.lapack_all(G)
    TG.judge("make_grm/stedc m=%d" % m, n, {k: (v, ref[k]) for k, v in TG.pair_measures(G, w, K).items()})


def test_ibrm_is_the_restatements_chain_on_the_downloaded_pair(demo):
    import test_gpu_bslmm as TB
    pl, phe = demo["plink"], demo["phe"]
    fit = H.ibrm("T1 ~ 1", data=phe, M=pl["geno"], M_id=demo["ids"], method="BSLMM", lambda_=LAMBDA, verbose=False, eigen_solver="device",
                 tridiagonal="device", **KW)
    Kval, K = H.make_grm(demo["M"], LAMBDA, eigen=True, verbose=False, eigen_solver="device", tridiagonal="device")   # (bit for bit ibrm()'s pair)
    a = B.bslmm(demo["y"], demo["M"], [0.95, 0.05], Kival=Kval, Ki=K, order="blas", **KW)
    b = B.bslmm(demo["y"], demo["M"], [0.95, 0.05], Kival=Kval, Ki=K, order="rev", **KW)
    got = dict(fit)
    got["e"] = fit["e"]["e"]
    TB.compare_chain(got, a, b)
    assert fit["n_records"] == 20 and len(fit["g"]["gebv"]) == 600 and np.all(np.isfinite(fit["g"]["gebv"]))


@pytest.mark.parametrize("n", [129, 300])
def test_two_runs_agree_bit_for_bit(n):
    d, e = S.random_pair(n)
    (w1, Z1), (w2, Z2) = device_pair(d, e), device_pair(d, e)
    assert np.array_equal(w1, w2) and np.array_equal(Z1, Z2)
    G = E.grm_case(n, 200, LAMBDA)
    (v1, K1), (v2, K2) = H.eigh(G, tridiagonal="device"), H.eigh(G, tridiagonal="device")
    assert np.array_equal(v1, v2) and np.array_equal(K1, K2)


def test_refusals():
    d, e = S.random_pair(40)
    bad = d.copy()
    bad[17] = np.nan
    with pytest.raises(H.HibayesError, match="the tridiagonal matrix holds a non-finite value") as ex:
        HE.tridiagonal_eigh_device(bad, e)
    assert ex.value.status == 1
    G = E.grm_case(40, 90, LAMBDA)
    with HE.Reduction(HE.upload(G)) as red:
        w, Zh = HE.tridiagonal_eigh_device(red.d, red.e)
        Zh.close()
        with pytest.raises(H.HibayesError, match="has been closed") as ex:       # a closed Z
            red.vectors_dev(Zh, w)
        assert ex.value.status == 1
        w, Zh = HE.tridiagonal_eigh_device(red.d, red.e)
        Zh.ld += 2                                                              # a wrong leading dimension
        with pytest.raises(H.HibayesError, match="leading dimension of Z must be n rounded up to 64") as ex:
            red.vectors_dev(Zh, w)
        assert ex.value.status == 1
        Zh.ld -= 2
        with red.vectors_dev(Zh, w) as Kh:                                      # the buffer stayed the caller's, and is taken over now
            assert Zh.ptr is None
            assert E.res_eps(G, w, Kh.toarray()) <= 64 * 40
        red.A.close()
    w, K = H.eigh(G, tridiagonal="device")                                      # and the device is still fine
    assert E.res_eps(G, w, K) <= 64 * 40
