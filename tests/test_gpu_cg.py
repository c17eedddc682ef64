"""sbrm()'s method = "CG" on the MI355X (hb_cg.hip: k_cg_matvec_dense, k_cg_matvec_csc, k_cg_step1, k_cg_step2, k_cg_symcheck;
reference CG(), src/solver.cpp:54-115, conjgt_den / conjgt_spa, src/cg.cpp) against the numpy restatement
(tests/cg_restatement.py, checked on the CPU by test_cg_host.py).

The method has no RNG, so a well-conditioned solve is compared pass for pass. The one freedom is the order in which A * p is
summed (unpinned in the reference too: it is its BLAS's). The trajectory test therefore measures, per case, the largest relative
difference between the restatement's own two orders (A @ v, and column chunks added last to first) and allows the device — a
third legal order — 1000 times that, with a floor of 1e-12 relative. Measured on a CPU: spread 6.1e-14 (dense, lambda = 1),
3.5e-14 (per-marker lambda), 2.5e-15 (lambda = 950), 1.0e-15 (m = 333), 2.0e-14 (sparse), so tolerances of 6.1e-11, 3.5e-11,
2.5e-12, 1e-12 and 2.0e-11; the test prints both. test_cg_host.py asserts what keeps this from passing by luck: both orders stop
at the same pass, no err within 1e-6 (relative) of esp, spread <= 1e-9."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import hibayes_amd as H
from hibayes_amd import _lib
import cg_restatement as R
from test_gpu_sbayess import bits, same_run
from test_sbayess_host import full_csc

pytestmark = pytest.mark.gpu
ESP = 1e-6


@pytest.fixture(scope="module")
def handles():
    """handles of the fixtures' matrices, made once: the dense ones stored in full (so that hb_cg_run_ldm's device copy and
    hb_cg_run_sparse's CSC hold exactly the host matrix), the thresholded one as it is"""
    F = R.demo_fixtures()
    hs = {"dense950": H.LDMatrix.from_scipy(full_csc(F["ld"])), "dense333": H.LDMatrix.from_scipy(full_csc(F["ld333"])),
          "sparse950": H.LDMatrix.from_scipy(F["sp"])}
    yield hs
    for h in hs.values():
        h.close()


def dense_of(A):
    return A.toarray(order="F") if sp.issparse(A) else A


def agree(dev, ref, tol, what):
    """iterations and converged exactly; err_hist elementwise, g (against its largest entry), vg and ve within tol, relative"""
    assert dev["iterations"] == ref["iterations"] and dev["converged"] == ref["converged"], what
    assert dev["n"] == ref["n"] and dev["count_y"] == ref["count_y"]
    d = {"err_hist": float(np.max(np.abs(dev["err_hist"] - ref["err_hist"]) / np.abs(ref["err_hist"]))),
         "g": float(np.max(np.abs(dev["g"] - ref["g"])) / np.max(np.abs(ref["g"]))),
         "vg": abs(dev["vg"] - ref["vg"]) / abs(ref["vg"]), "ve": abs(dev["ve"] - ref["ve"]) / abs(ref["ve"])}
    print(what, "device against restatement:", d, "allowed:", tol)
    assert max(d.values()) <= tol, (what, d)
    assert dev["err"] == dev["err_hist"][-1]


def solves(dev, ss, V, lam, what, esp=ESP):
    """the result alone: converged within m passes, the true residual within 2 esp, g within 2 esp / lambda_min(V + Lambda) of
    numpy's direct solve (the recursive residual is below esp at the break), vg and ve the reference's formulas of that g"""
    m = V.shape[0]
    n, b, yy, count_y = R.setup(ss, np.diag(V))
    M = V + np.diag(lam if lam is not None else np.zeros(m))
    lmin = np.linalg.eigvalsh(M)[0]
    res = np.linalg.norm(b - M @ dev["g"])
    off = np.max(np.abs(dev["g"] - np.linalg.solve(M, b)))
    print(what, "iterations", dev["iterations"], "true residual", res, "max|g - solve|", off, "lambda_min", lmin)
    assert lmin > 0 and dev["converged"] and 1 <= dev["iterations"] <= m and dev["err"] < esp
    assert res <= 2 * esp and off <= 2 * esp / lmin
    vg = n * (dev["g"] @ (V @ dev["g"])) / (n - 1)
    assert dev["n"] == n and dev["count_y"] == count_y
    assert dev["vg"] == pytest.approx(vg, rel=1e-9) and dev["ve"] == pytest.approx(yy / (n - 1) - vg, rel=1e-9, abs=1e-9 * abs(vg))


@pytest.mark.parametrize("name", list(R.trajectory_cases()))
def test_trajectory_equals_the_restatement_through_all_three_entry_points(handles, name):
    ss, A, lam = R.trajectory_cases()[name]
    ref, other = R.both_orders(name)
    spread = R.spread(ref, other)
    tol = max(1000 * spread, 1e-12)
    print(name, "spread between the restatement's two orders:", spread, "-> tolerance", tol, "iterations", ref["iterations"])
    h = handles[name.split("_")[0]]
    agree(H.conjgt_den(ss, dense_of(A), lam, verbose=False), ref, tol, name + " hb_cg_run")
    agree(H.conjgt_den(ss, h, lam, verbose=False), ref, tol, name + " hb_cg_run_ldm")
    agree(H.conjgt_spa(ss, h, lam, verbose=False), ref, tol, name + " hb_cg_run_sparse")


def test_sparse_matrix_built_on_the_device_runs_from_its_own_csc():
    """.bed -> ldmat(chisq, keep_on_device=True) -> CG with no host matrix. The device-built matrix is not the host fixture (it
    is thresholded at the genotypes' own n = 600 and keeps 23 % of the entries), and at lambda = 1 its trajectory is not
    reproducible — the restatement's own two orders part by 3e-7 over their 28 passes, which
    test_cg_host.py::test_device_built_sparse_matrix_has_no_reproducible_trajectory_at_lambda_1 asserts on the CPU — so, as for
    the ill-conditioned solve, the result is checked; the same matrix through LDMatrix.from_scipy walks the same CSC and must
    agree bit for bit."""
    F = R.demo_fixtures()
    lam = np.ones(950)
    with H.ldmat(F["geno"][:, F["ok"]], chisq=5.0, keep_on_device=True) as ld:
        assert ld.kind == "sparse"
        r = H.sbrm_cg(F["ss"], ld, lambda_=1.0, verbose=False, sparse_ld=True)
        A = ld.tocsc()
    solves(r, F["ss"], A.toarray(), lam, "ldmat -> sbrm_cg")
    assert r["model"] == "Summary level Bayesian model fit by [CG]" and "gwas" not in r
    assert same_run(r, H.sbrm_cg(F["ss"], A, lambda_=1.0, verbose=False))


def test_ill_conditioned_solve_reaches_the_answer():
    """lambda = 0.005: 207 passes in the restatement, and trajectories are not reproducible here (with lambda = 0.05 the
    restatement's own two orders stop at 80 and 81), so only the result is checked."""
    F = R.demo_fixtures()
    lam = np.full(950, 0.005)
    solves(H.conjgt_den(F["ss"], F["ld"], lam, verbose=False), F["ss"], F["ld"], lam, "lambda = 0.005")


def tiny():
    V, b = np.asfortranarray(np.diag([1.0, 2.0, 3.0, 4.0]) + 0.1), np.array([1.0, -2.0, 3.0, 0.5])
    return np.column_stack([np.full(4, 0.3), b / np.diag(V), np.full(4, 0.1), np.full(4, 100.0)]), V


def test_iteration_limit_and_its_console_line():
    """esp = 1e-20 cannot be met: all m = 4 passes run, the state stays finite, not converged. err_hist is compared where it
    exceeds 1e-9 of its first entry, to 1e-12 of that entry: the residual is a recurrence on numbers of the size of b, so its
    rounding is a few 1e-16 of err_hist[0] whatever its own size — four orders below the bound; a wrong alpha or beta moves it
    by its own size."""
    ss, V = tiny()
    ref = R.conjgt_restatement(ss, V, None, esp=1e-20)
    assert ref["iterations"] == 4 and not ref["converged"] and ref["err"] < 1e-12
    lines = []
    runs = [H.conjgt_den(ss, V, None, esp=1e-20, outfreq=2, log=lines.append), H.conjgt_spa(ss, sp.csc_matrix(V), None, esp=1e-20, verbose=False)]
    for r in runs:
        assert r["iterations"] == 4 and not r["converged"] and r["err_hist"].shape == (4,) and np.isfinite(r["g"]).all()
        np.testing.assert_allclose(r["g"], np.linalg.solve(V, ref["b"]), rtol=0, atol=1e-12)
        big = ref["err_hist"] > 1e-9 * ref["err_hist"][0]
        assert big[:3].all()
        np.testing.assert_allclose(r["err_hist"][big], ref["err_hist"][big], rtol=0, atol=1e-12 * ref["err_hist"][0])
    assert lines[:4] == ["Prior parameters:", "    Model fitted at [Conjugate Gradient]", "    Maximum iteration number: 4",
                         "    Phenotypic var %.4f" % (ref["yy"] / 99)]
    assert lines[4] == "Iter No.1, err = %.6f" % runs[0]["err_hist"][1] and lines[5] == "Iter No.3, err = %.6f" % runs[0]["err_hist"][3]
    assert lines[6:] == ["Convergence: NO[try to adjust lambda]", "Prior parameters:", "    Genetic var %.4f" % runs[0]["vg"],
                         "    Residual var %.4f" % runs[0]["ve"]]


def test_a_nan_beta_propagates_as_in_the_reference():
    ss, V = tiny()
    ss[1, 1] = np.nan
    ref = R.conjgt_restatement(ss, V, np.ones(4))
    assert np.isnan(ref["g"]).all() and ref["iterations"] == 4 and not ref["converged"]
    for r in (H.conjgt_den(ss, V, np.ones(4), verbose=False), H.conjgt_spa(ss, sp.csc_matrix(V), np.ones(4), verbose=False)):
        assert np.isnan(r["g"]).all() and r["iterations"] == 4 and not r["converged"] and np.isnan(r["err"])
        assert np.isnan(r["err_hist"]).all() and np.isnan(r["vg"]) and r["count_y"] == 4
    # a matrix larger than one chunk of iterations: the host stops launching once err is NaN
    F = R.demo_fixtures()
    ss = F["ss333"].copy()
    ss[7, 1] = np.nan
    r = H.conjgt_den(ss, F["ld333"], np.ones(333), verbose=False)
    assert np.isnan(r["g"]).all() and r["iterations"] == 333 and not r["converged"] and np.isnan(r["err_hist"]).all()


def test_two_runs_agree_bit_for_bit(handles):
    """fixed-order reductions, no floating-point atomics"""
    ss, A, lam = R.trajectory_cases()["dense950_lambda1"]
    assert same_run(H.conjgt_den(ss, A, lam, verbose=False), H.conjgt_den(ss, A, lam, verbose=False))
    ss, A, lam = R.trajectory_cases()["sparse950_lambda1"]
    assert same_run(H.conjgt_spa(ss, handles["sparse950"], lam, verbose=False), H.conjgt_spa(ss, A, lam, verbose=False))


def test_paths_agree(handles):
    """One dense kernel behind the host array and both kinds of handle: bit for bit. The sparse kernel on the same matrix stored
    in full sums in another order: within the trajectory test's tolerance."""
    ss, A, lam = R.trajectory_cases()["dense950_lambda1"]
    host = H.conjgt_den(ss, A, lam, verbose=False)
    assert same_run(host, H.conjgt_den(ss, handles["dense950"], lam, verbose=False))
    tol = max(1000 * R.spread(*R.both_orders("dense950_lambda1")), 1e-12)
    agree(H.conjgt_spa(ss, full_csc(A), lam, verbose=False), host, tol, "conjgt_spa on the matrix stored in full, against conjgt_den")
    F = R.demo_fixtures()
    with H.ldmat(F["geno"][:, F["ok"]], keep_on_device=True) as ld:                 # the genome-wide dense kind, built on the device
        assert ld.kind == "dense"
        a = H.conjgt_den(ss, ld, lam, verbose=False)
        assert same_run(a, H.conjgt_den(ss, ld.toarray(), lam, verbose=False))
        assert a["iterations"] == host["iterations"]
        np.testing.assert_allclose(a["g"], host["g"], rtol=0, atol=1e-9 * np.max(np.abs(host["g"])))   # (np.cov's last bits)


def small_case(m, seed):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 3, (40, m)).astype(np.float64)
    V = np.atleast_2d(np.cov(X, rowvar=False, ddof=0)) + np.eye(m)              # well-conditioned, positive definite
    V = np.asfortranarray(np.triu(V) + np.triu(V, 1).T)
    ss = np.column_stack([X.mean(0) / 2, rng.normal(0, 0.3, m), np.full(m, 0.05), np.full(m, 40.0)])
    return ss, V


@pytest.mark.parametrize("m", [1, 3, 65])
def test_small_sizes_with_and_without_lambda(m):
    """m = 1 and 3: less than one 16-byte pair per lane and an odd leading dimension, so peeled heads and tails only; m = 65: half
    a wave of pairs plus the peeled or the tail element, 17 workgroups of the dense mat-vec, the CSC at 4 and at 16 lanes per
    column. Checked by their result: a product that drops or repeats an entry solves another system."""
    ss, V = small_case(m, 40 + m)
    for lam in (None, np.linspace(0.5, 1.5, m)):
        solves(H.conjgt_den(ss, V, lam, verbose=False), ss, V, lam, "dense m = %d" % m)
        solves(H.conjgt_spa(ss, sp.csc_matrix(V), lam, verbose=False), ss, V, lam, "sparse m = %d" % m)


def test_padded_leading_dimension_through_ctypes():
    """ld_ldm = m + 1 with poisoned padding rows: the result of the unpadded call, bit for bit"""
    F = R.demo_fixtures()
    m, ss, lam = 333, np.asfortranarray(F["ss333"]), np.ones(333)
    pad = np.full((m + 1, m), np.nan, order="F")
    pad[:m, :] = F["ld333"]
    g, hist = np.zeros(m), np.zeros(m)
    a, o = _lib.CGArgs(), _lib.CGOut()
    a.m, a.sumstat, a.ld_sumstat, a.ldm, a.ld_ldm, a.lambda_ = m, ss.ctypes.data, m, pad.ctypes.data, m + 1, lam.ctypes.data
    a.esp, a.outfreq, a.verbose = ESP, 100, 0
    o.g, o.err_hist = g.ctypes.data, hist.ctypes.data
    assert H.lib().hb_cg_run(C.byref(a), C.byref(o)) == 0, H.lib().hb_last_error()
    ref = H.conjgt_den(ss, F["ld333"], lam, verbose=False)
    assert o.iterations == ref["iterations"] == 15 and o.converged == 1
    assert np.array_equal(bits(g), bits(ref["g"])) and np.array_equal(bits(hist[:15]), bits(ref["err_hist"])) and not hist[15:].any()
    assert bits(o.vg) == bits(ref["vg"]) and bits(o.ve) == bits(ref["ve"]) and bits(o.err) == bits(ref["err"])


def test_empty_columns_and_a_long_column():
    F = R.demo_fixtures()
    ss, lam = F["ss"], np.ones(950)
    # 30 markers without any stored entry: ap[j] = lambda[j] p[j] there, g[j] = b[j] / lambda[j] = 0 (their diagonal is gone)
    drop = np.arange(7, 950, 32)[:30]
    V = F["sp"].toarray()
    V[drop, :] = 0.0
    V[:, drop] = 0.0
    A = sp.csc_matrix(V)
    assert (np.diff(A.indptr)[drop] == 0).all()
    r = H.conjgt_spa(ss, A, lam, verbose=False)
    solves(r, ss, V, lam, "30 empty columns")
    assert not r["g"][drop].any()
    # one marker in LD with everybody: a column (and row) of 950 > 512 stored entries among columns of 87 on average
    V = F["sp"].toarray()
    V[0, :] = F["ld"][0, :]
    V[:, 0] = F["ld"][:, 0]
    A = sp.csc_matrix(V)
    per = np.diff(A.indptr)
    assert per[0] > 512 and per.mean() < 256
    lam = np.full(950, 950.0)
    solves(H.conjgt_spa(ss, A, lam, verbose=False), ss, V, lam, "a column of %d entries" % per[0])


def test_a_host_matrix_that_differs_from_its_transpose_is_refused():
    F = R.demo_fixtures()
    V = F["ld333"].copy(order="F")
    V[10, 300] = np.nextafter(V[10, 300], np.inf)
    V[5, 200] = np.nextafter(V[5, 200], np.inf)       # one bit; the first differing pair in column-major order
    with pytest.raises(H.HibayesError, match=r"must equal its transpose in value bits: ldm\[5\]\[200\] differs from ldm\[200\]\[5\]") as e:
        H.conjgt_den(F["ss333"], V, np.ones(333), verbose=False)
    assert e.value.status == 1                        # HB_ERR_INVALID


def test_console_lines_of_a_converged_run():
    ss, A, lam = R.trajectory_cases()["dense950_lambda1"]
    lines = []
    r = H.sbrm_cg(ss, A, lambda_=1.0, printfreq=10, log=lines.append)
    assert lines[:3] == ["Prior parameters:", "    Model fitted at [Conjugate Gradient]", "    Maximum iteration number: 950"]
    assert lines[3].startswith("    Phenotypic var ")
    assert lines[4:6] == ["Iter No.9, err = %.6f" % r["err_hist"][9], "Iter No.19, err = %.6f" % r["err_hist"][19]]
    assert lines[6:] == ["Convergence: YES", "Prior parameters:", "    Genetic var %.4f" % r["vg"], "    Residual var %.4f" % r["ve"]]
    assert r["iterations"] == 22 and r["call"] == "b ~ nD^{-1}V alpha + e"
