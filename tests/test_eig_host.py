"""The device eigensolver's host side (hibayes_amd/eig.py, hb_eig_*): the numpy restatement of its convention against LAPACK's own pipeline, the
additive C ABI, and the refusals that need no device. Runs without a GPU."""
import inspect
import os

import numpy as np
import pytest

import hibayes_amd as H
from hibayes_amd import _lib

import eig_restatement as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIG_SYMBOLS = ["hb_eig_upload", "hb_eig_reduce", "hb_eig_tau", "hb_eig_vectors", "hb_eig_download", "hb_eig_release", "hb_eig_destroy"]
CASES = E.grm_cases(64) + E.grm_cases(32)[4:7]
NO_DEVICE = H.lib().hb_device_count() < 1


def crafted():
    rng = np.random.default_rng(11)
    G = E.grm_case(40, 90, .01)
    G[:, 7] = G[:, 3]
    G[7, :] = G[3, :]
    G[7, 7] = G[3, 3]
    return {"diagonal": np.diag(rng.uniform(0.5, 2.0, 37)), "multiple of I": 1.75 * np.eye(33), "two identical rows": np.asfortranarray(G)}


@pytest.mark.parametrize("n,m,lam", CASES)
def test_restatement_agrees_with_the_lapack_pipeline(n, m, lam):
    """Same convention, so d, e, tau and the reflectors are LAPACK's to rounding — dsytrd is blocked (dlatrd) from n = 33 on, the restatement is
    not, so they differ by the backward error of either: a small multiple of n eps ||G||. Then the pair, by both error measures."""
    G = E.grm_case(n, m, lam)
    d, e, V, tau = E.householder_tridiagonal(G)
    c, dl, el, taul = E.lapack_tridiagonal(G)
    scale, tol = E.norm2(G), 64 * n * E.EPS
    # (n > m: G - lambda I has rank m, the subdiagonal falls to rounding level after m columns and what follows reduces rounding noise — d and e
    # are then no continuous function of G, and only Q' G Q = T and the eigenvalues below can be compared)
    if n <= m:
        assert np.max(np.abs(d - dl), initial=0.0) <= tol * scale
    if 1 < n <= m:
        assert np.max(np.abs(np.abs(e) - np.abs(el))) <= tol * scale
        # the signs too where the subdiagonal is not at rounding level (there the sign of alpha is rounding's)
        big = np.abs(el) > 1e-6 * scale
        assert np.array_equal(np.sign(e[big]), np.sign(el[big]))
        assert np.all((tau >= 0) & (tau <= 2)) and tau[-1] == 0.0 and taul[-1] == 0.0
    Q = E.back_transform(V, tau)
    T = Q.T @ G @ Q
    assert E.orth_eps(Q) <= 8 * n
    assert np.max(np.abs(T - (np.diag(d) + np.diag(e, 1) + np.diag(e, -1)))) <= tol * scale
    w, K = E.restatement_eigh(G)
    wl, Kl = E.lapack_eigh(G)
    wr = np.linalg.eigvalsh(G)
    assert np.all(np.diff(w) >= 0)
    assert np.max(np.abs(w - wr)) <= tol * scale and np.max(np.abs(wl - wr)) <= tol * scale
    for name, f in (("res", lambda KK, ww: E.res_eps(G, ww, KK)), ("orth", lambda KK, ww: E.orth_eps(KK))):
        mine, ref = f(K, w), f(Kl, wl)
        print("%s n=%d m=%d: restatement %.1f eps, LAPACK %.1f eps" % (name, n, m, mine, ref))
        assert mine <= 4 * ref + n, (name, mine, ref)


@pytest.mark.parametrize("name", ["diagonal", "multiple of I", "two identical rows"])
def test_restatement_on_the_crafted_inputs(name):
    G = crafted()[name]
    n = G.shape[0]
    d, e, V, tau = E.householder_tridiagonal(G)
    if name != "two identical rows":
        assert np.all(tau == 0) and np.all(e == 0) and np.array_equal(d, np.diag(G))      # every reflector is the identity
    w, K = E.restatement_eigh(G)
    assert E.res_eps(G, w, K) <= 64 * n and E.orth_eps(K) <= 64 * n
    np.testing.assert_allclose(w, np.linalg.eigvalsh(G), rtol=0, atol=64 * n * E.EPS * E.norm2(G))


def test_lapack_back_transform_is_q_times_z():
    G = E.grm_case(17, 63, .01)
    c, d, e, tau = E.lapack_tridiagonal(G)
    V = E.reflectors_from_packed(c, tau)
    Z = np.random.default_rng(3).normal(size=(17, 17))
    np.testing.assert_allclose(E.lapack_back_transform(c, tau, Z), E.back_transform(V, tau, Z), rtol=0, atol=1e-13)


def test_new_symbols_are_declared_exported_and_the_abi_is_still_6():
    lib = H.lib()
    hdr = open(os.path.join(ROOT, "include", "hibayes_gpu.h")).read()
    for s in EIG_SYMBOLS:
        assert s in _lib.SYMBOLS and hasattr(lib, s) and (s + "(") in hdr, s
    assert "typedef struct hb_eig hb_eig;" in hdr and "src/rm.cpp:46-52" in hdr and "R/bayes.r:292-294" in hdr
    assert lib.hb_abi_version() == 6


def test_eigh_is_exported_and_the_defaults_are_the_host_route():
    assert "eigh" in H.__all__ and callable(H.eigh)
    for f in (H.make_grm, H.ibrm):
        assert inspect.signature(f).parameters["eigen_solver"].default == "host"
    assert inspect.signature(H.make_grm).parameters["keep_on_device"].default is False
    assert inspect.signature(H.eigh).parameters["keep_on_device"].default is False


def test_a_bad_eigen_solver_is_a_value_error():
    M = np.zeros((4, 6), dtype=np.int8)
    with pytest.raises(ValueError, match="eigen_solver"):
        H.make_grm(M, eigen=True, eigen_solver="gpu", verbose=False)
    with pytest.raises(ValueError, match="eigen_solver"):
        H.ibrm("T1 ~ 1", data={"id": ["a"], "T1": [1.0]}, M=M[:1], M_id=["a"], method="BSLMM", eigen_solver="lapack")
    with pytest.raises(ValueError, match="keep_on_device"):
        H.make_grm(M, eigen=True, keep_on_device=True, verbose=False)


def test_arguments_are_refused_before_any_device_is_asked_for():
    import ctypes as C
    lib = H.lib()
    A = np.eye(3, order="F")
    d, e, h = np.zeros(3), np.zeros(2), C.c_void_p()
    for lda, n, text in ((2, 3, "leading dimension smaller than n"), (3, 0, "n < 1")):
        assert lib.hb_eig_reduce(A.ctypes.data, lda, n, 0, d.ctypes.data, e.ctypes.data, C.byref(h)) == 1   # (never dereferenced: refused first)
        assert text in lib.hb_last_error().decode() and not h.value
    K, ldk = C.c_void_p(), C.c_int64()
    assert lib.hb_eig_vectors(None, None, 0, C.byref(K), C.byref(ldk)) == 1 and "null handle" in lib.hb_last_error().decode()
    lib.hb_eig_destroy(None)
    lib.hb_eig_release(None)


@pytest.mark.skipif(not NO_DEVICE, reason="a HIP device is visible: the no-device refusals cannot be seen here")
def test_without_a_device_the_compute_entries_say_so():
    G = E.grm_case(17, 63, .01)
    with pytest.raises(H.HibayesError, match="no HIP device available") as ex:
        H.eigh(G)
    assert ex.value.status == 2
    with pytest.raises(H.HibayesError, match="no HIP device available") as ex:
        H.make_grm(np.ones((5, 7), dtype=np.int8), 0.01, eigen=True, eigen_solver="device", verbose=False)
    assert ex.value.status == 2
