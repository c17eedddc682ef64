"""sbrm()'s method = "CG" without a GPU: the numpy restatement the GPU tests compare against (tests/cg_restatement.py) is checked
against numpy.linalg.solve, the conditions that keep a GPU test from passing by luck are asserted on the fixtures, and the
refusals of sbrm_cg() / conjgt_den() / conjgt_spa() / hb_cg_run* that need no device carry the reference's texts."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import hibayes_amd as H
from hibayes_amd import _lib
import cg_restatement as R

ESP = 1e-6
CASES = list(R.trajectory_cases())


def dense_of(A):
    return A.toarray() if sp.issparse(A) else np.asarray(A)


@pytest.mark.parametrize("name", CASES)
def test_restatement_solves_the_ridge_system(name):
    """Both summation orders stop with a true residual within 2 esp (the recursive residual is below esp at the break; the two
    part by rounding only), and g is then within 2 esp / lambda_min(V + Lambda) of numpy's direct solve."""
    ss, A, lam = R.trajectory_cases()[name]
    M = dense_of(A) + np.diag(lam)
    lmin = np.linalg.eigvalsh(M)[0]
    assert lmin > 0.4
    for r in R.both_orders(name):
        assert r["converged"] and r["iterations"] < M.shape[0] and r["n"] == 300 and r["count_y"] == M.shape[0]
        assert np.linalg.norm(r["b"] - M @ r["g"]) <= 2 * ESP
        assert np.linalg.norm(r["g"] - np.linalg.solve(M, r["b"])) <= 2 * ESP / lmin
        assert r["vg"] == pytest.approx(300 * (r["g"] @ (dense_of(A) @ r["g"])) / 299, rel=1e-12)
        assert r["ve"] == pytest.approx(r["yy"] / 299 - r["vg"], rel=1e-12)


def test_fixtures_are_what_the_gpu_tests_say_they_are():
    F = R.demo_fixtures()
    assert F["ld"].shape == (950, 950) and np.array_equal(F["ld"], F["ld"].T) and F["ld333"].shape == (333, 333)
    per = np.diff(F["sp"].indptr)
    assert 0.085 < F["sp"].nnz / 950 ** 2 < 0.095 and (abs(F["sp"] - F["sp"].T)).nnz == 0 and 16 <= per.mean() < 256
    its = {k: R.both_orders(k)[0]["iterations"] for k in CASES}
    assert its == {"dense950_lambda1": 22, "dense950_lambda950": 3, "dense950_lambda_vector": 22, "dense333_lambda1": 15,
                   "sparse950_lambda1": 24}


@pytest.mark.parametrize("name", CASES)
def test_trajectory_cases_cannot_pass_by_luck(name):
    """The two orders agree on the iteration count, no err sits within 1e-6 (relative) of esp — a third legal order, the
    device's, cannot stop an iteration earlier or later — and the spread between the orders, whose 1000-fold is the GPU test's
    tolerance, is at most 1e-9."""
    a, b = R.both_orders(name)
    assert a["iterations"] == b["iterations"] and a["converged"] and b["converged"]
    for r in (a, b):
        assert np.min(np.abs(r["err_hist"] - ESP) / ESP) >= 1e-6
    s = R.spread(a, b)
    print(name, "spread between the two orders:", s, "closest err to esp:", np.min(np.abs(a["err_hist"] - ESP) / ESP))
    assert s <= 1e-9


def test_ill_conditioned_case_reaches_its_residual_under_both_orders():
    ss, A, _ = R.trajectory_cases()["dense950_lambda1"]
    lam = np.full(950, 0.005)
    M = A + np.diag(lam)
    for mv in (R.matvec_plain, R.matvec_reversed_chunks):
        r = R.conjgt_restatement(ss, A, lam, matvec=mv)
        res = np.linalg.norm(r["b"] - M @ r["g"])
        print("iterations", r["iterations"], "true residual", res, "max|g - solve|", np.max(np.abs(r["g"] - np.linalg.solve(M, r["b"]))))
        assert r["converged"] and r["iterations"] <= 950 and res <= 1.1 * ESP
        assert np.max(np.abs(r["g"] - np.linalg.solve(M, r["b"]))) <= 2 * ESP / 0.005


def test_device_built_sparse_matrix_has_no_reproducible_trajectory_at_lambda_1():
    """What test_gpu_cg.py's test of ldmat(geno[:, ok], chisq=5.0, keep_on_device=True) rests on, asserted here on the matrix's
    bit-exact restatement (tests/ldmat_restatement.py): it is thresholded at the genotypes' own n = 600, keeps 23 % of the
    entries, and at lambda = 1 the two summation orders part by 3e-7 over their 28 passes — beyond the 1e-9 a trajectory case may
    have — so the GPU test checks that case by its result, for which both orders must reach a true residual within 1.1 esp."""
    from ldmat_restatement import ldmat_restatement
    F = R.demo_fixtures()
    A = ldmat_restatement(F["geno"][:, F["ok"]], chisq=5.0)
    assert np.array_equal(A, A.T) and 0.20 < (A != 0).mean() < 0.25
    lam, M = np.ones(950), A + np.eye(950)
    assert np.linalg.eigvalsh(M)[0] > 0.4
    a = R.conjgt_restatement(F["ss"], sp.csc_matrix(A), lam)
    b = R.conjgt_restatement(F["ss"], sp.csc_matrix(A), lam, matvec=R.matvec_reversed_chunks)
    s = R.spread(a, b)
    print("iterations", a["iterations"], b["iterations"], "spread", s)
    assert a["iterations"] == b["iterations"] == 28 and 1e-9 < s < 1e-5
    for r in (a, b):
        assert r["converged"] and np.linalg.norm(r["b"] - M @ r["g"]) <= 1.1 * ESP


def test_iteration_limit_case_runs_all_four_passes():
    V, b = np.diag([1.0, 2.0, 3.0, 4.0]) + 0.1, np.array([1.0, -2.0, 3.0, 0.5])
    x, its, conv, hist = R.cg(R.matvec_plain(V), b, None, 1e-20)
    assert its == 4 and not conv and np.isfinite(x).all() and hist[-1] < 1e-12
    np.testing.assert_allclose(x, np.linalg.solve(V, b), rtol=0, atol=1e-12)


def tiny_ss(m, n=100.0):
    return np.column_stack([np.full(m, 0.3), np.linspace(-1, 1, m) + 0.05, np.full(m, 0.1), np.full(m, n)])


def test_argument_errors_that_need_no_device():
    ss = tiny_ss(5)
    with pytest.raises(ValueError, match="length of lambda should be equal to the number of SNPs."):
        H.sbrm_cg(ss, np.eye(5), lambda_=[1.0, 2.0])
    with pytest.raises(ValueError, match="length of lambda should be equal to the number of SNPs."):
        H.conjgt_den(ss, np.eye(5), np.ones(4))
    with pytest.raises(ValueError, match="Unrecognized type of ldm."):
        H.sbrm_cg(ss, "ldm")
    with pytest.raises(ValueError, match="sparse_ld=True needs a scipy sparse ldm or an LDMatrix"):
        H.sbrm_cg(ss, np.eye(5), sparse_ld=True)
    with pytest.raises(ValueError, match="goes to conjgt_spa"):
        H.conjgt_den(ss, sp.identity(5, format="csc"))
    with pytest.raises(ValueError, match="goes to conjgt_den"):
        H.conjgt_spa(ss, np.eye(5))
    with pytest.raises(H.HibayesError, match="Number of SNPs not equals."):
        H.sbrm_cg(ss, np.eye(4), lambda_=1.0, verbose=False)
    with pytest.raises(ValueError, match="Number of SNPs not equals."):
        H.conjgt_spa(ss, sp.identity(4, format="csc"), verbose=False)
    nose = ss.copy()
    nose[:, 2] = np.nan
    with pytest.raises(H.HibayesError, match="Lack of SE."):
        H.conjgt_den(nose, np.eye(5), np.ones(5), verbose=False)
    # the COJO table's columns 4, 5, 6, 8 are the ones kept (R/sbayes.r:209): with SE in column 6 missing -> "Lack of SE."
    cojo = np.zeros((5, 8))
    cojo[:, [3, 4, 7]] = ss[:, [0, 1, 3]]
    cojo[:, 5] = np.nan
    with pytest.raises(H.HibayesError, match="Lack of SE."):
        H.sbrm_cg(cojo, np.eye(5), lambda_=1.0, verbose=False)
    # a sparse matrix that differs from its transpose is refused when its handle is made
    bad = sp.csc_matrix(np.array([[1.0, 0.5, 0.0], [0.25, 1.0, 0.0], [0.0, 0.0, 1.0]]))
    with pytest.raises(H.HibayesError, match="must equal its transpose"):
        H.conjgt_spa(tiny_ss(3), bad, verbose=False)
    with pytest.raises(H.HibayesError, match="must equal its transpose"):
        H.sbrm_cg(tiny_ss(3), bad, lambda_=1.0, verbose=False)


def test_c_abi_refusals_and_struct_layout():
    L = H.lib()
    ss, ld, g = np.asfortranarray(tiny_ss(5)), np.asfortranarray(np.eye(5)), np.zeros(5)
    a, o = _lib.CGArgs(), _lib.CGOut()
    a.m, a.sumstat, a.ld_sumstat, a.ldm, a.ld_ldm, a.esp, a.outfreq = 5, ss.ctypes.data, 5, ld.ctypes.data, 4, 1e-6, 100
    o.g = g.ctypes.data
    def err(rc):
        return rc, L.hb_last_error().decode()
    assert err(L.hb_cg_run(C.byref(a), C.byref(o))) == (1, "Number of SNPs not equals.")          # ld_ldm < m
    a.ld_ldm, a.ld_sumstat = 5, 4
    assert err(L.hb_cg_run(C.byref(a), C.byref(o))) == (1, "Number of SNPs not equals.")
    a.ld_sumstat, a.ldm = 5, None
    assert err(L.hb_cg_run(C.byref(a), C.byref(o))) == (1, "Number of SNPs not equals.")          # no matrix at all
    assert err(L.hb_cg_run_ldm(C.byref(a), None, C.byref(o))) == (1, "hb_cg_run_ldm: null LD matrix handle")
    assert err(L.hb_cg_run_sparse(C.byref(a), None, C.byref(o))) == (1, "hb_cg_run_sparse: null LD matrix handle")
    assert err(L.hb_cg_run(None, C.byref(o))) == (1, "hb_cg_run: null argument")
    if L.hb_device_count() == 0:                                              # valid arguments, no device: refused loudly
        with pytest.raises(H.HibayesError, match="no HIP device available"):
            H.conjgt_den(tiny_ss(5), np.eye(5), np.ones(5), verbose=False)
    # the ctypes mirrors have the C layout
    import os
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "sz.c"), os.path.join(d, "sz")
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "hibayes_gpu.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n",'
                             'sizeof(hb_cg_args),sizeof(hb_cg_out),offsetof(hb_cg_args,lambda),offsetof(hb_cg_args,log),'
                             'offsetof(hb_cg_out,g),offsetof(hb_cg_out,loop_seconds));return 0;}\n')
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), src, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    A, O = _lib.CGArgs, _lib.CGOut
    assert got == [C.sizeof(A), C.sizeof(O), A.lambda_.offset, A.log.offset, O.g.offset, O.loop_seconds.offset]
    assert L.hb_abi_version() == 6                                            # additive: no existing struct changed


def test_sbrm_itself_still_refuses_cg_and_names_the_way():
    ss8 = np.zeros((5, 8))
    with pytest.raises(NotImplementedError, match="sbrm_cg"):
        H.sbrm(ss8, np.eye(5), "CG")
    with pytest.raises(NotImplementedError, match="CG"):
        H.sbrm(ss8, sp.identity(5, format="csc"), "CG", sparse_ld=True)
