"""ssbrm()'s imputation on the device (hibayes_amd/csrc/hb_impute.hip): the batched conjugate-gradient solve against dense algebra on the demo,
its determinism and the independence of a column from its block, a deep generated pedigree, the non-convergence error, and the route through
ssbrm_prepare() and ssbrm()."""
import re

import numpy as np
import pytest

import hibayes_amd as H
from hibayes_amd.impute import ImputeSystem

import impute_restatement as R
from test_impute_host import deep, ss_demo  # noqa: F401  (the module-scoped systems: built once here too)

pytestmark = pytest.mark.gpu
TOL = 1e-12


@pytest.fixture(scope="module")
def system(ss_demo):  # noqa: F811
    with ImputeSystem(ss_demo["Ann"], ss_demo["Ang"]) as S:
        yield S


def bounds(Ann, Ang, M, x, tol, lmin=None, star=None):
    """per column: the true residual recomputed here within 2 tol ||b|| (the restatement stays within 1.5, tests/test_impute_host.py), and the
    distance from the reference solution within 2 tol ||b|| / lambda_min"""
    b = -(Ang @ M)
    bn = np.linalg.norm(b, axis=0)
    res = np.linalg.norm(b - Ann @ x, axis=0)
    assert np.all(res <= 2 * tol * bn), np.max(res[bn > 0] / (tol * bn[bn > 0]))
    if star is not None:
        err = np.linalg.norm(x - star, axis=0)
        assert np.all(err <= 2 * tol * bn / lmin), np.max(err[bn > 0] / (2 * tol * bn[bn > 0] / lmin))
    return res, bn


def test_demo_columns_and_J_against_dense_algebra(ss_demo, system):  # noqa: F811
    """131 columns: two full groups of 64 lanes and a ragged one — the plan takes them as one block of W = 192 with 61 padding columns, and
    impute_device(chunk=50) as three blocks of W = 64 with 14 and 33; q = 900 is a multiple of neither 64 nor 256, and its last run of 16 rows
    has 4"""
    M = ss_demo["M"]
    assert M.shape == (600, 131) and np.all(M[:, 130] == -1.0)
    x, st = system.solve(M, TOL, 2000)
    ref = R.pcg_batched(ss_demo["Ann"], ss_demo["Ang"], M, TOL, 2000)
    print("demo: device %d iterations (W = %d, %d parts, %d looks), restatement %d; reported residual %.3g"
          % (st["iterations"], st["width"], st["parts"], st["looks"], ref["iterations"], st["max_residual"]))
    assert x.shape == (900, 131) and x.flags.f_contiguous and np.all(np.isfinite(x))
    res, bn = bounds(ss_demo["Ann"], ss_demo["Ang"], M, x, TOL, ss_demo["lmin"], ss_demo["dense"])
    true = np.max(res[bn > 0] / bn[bn > 0])
    assert abs(st["max_residual"] - true) <= 0.01 * true + 1e-16
    zero = np.flatnonzero(~M.any(axis=0))
    assert zero.size >= 1 and np.all(x[:, zero] == 0.0)
    assert 1 <= st["iterations"] <= 2000 and st["width"] % 64 == 0 and st["blocks"] == 1
    assert np.linalg.norm(x[:, 130] - ss_demo["dense"][:, 130]) <= 2 * TOL * bn[130] / ss_demo["lmin"] and bn[130] > 0   # Jn
    # the function form, in chunks: 50 + 50 + 31 columns through three calls
    x2, st2 = H.impute_device(ss_demo["Ann"], ss_demo["Ang"], M, tol=TOL, chunk=50)
    assert np.array_equal(x2, x) and st2["blocks"] == 3 and st2["setup_seconds"] > 0


def test_the_same_call_twice_gives_the_same_bits(ss_demo, system):  # noqa: F811
    a, sa = system.solve(ss_demo["M"], TOL, 2000)
    b, sb = system.solve(ss_demo["M"], TOL, 2000)
    assert np.array_equal(a, b) and sa["iterations"] == sb["iterations"] and sa["max_residual"] == sb["max_residual"]


def test_a_columns_bits_do_not_depend_on_its_block(ss_demo, system):  # noqa: F811
    M = ss_demo["M"]
    block, _ = system.solve(M[:, :64], TOL, 2000)
    for c in (0, 17, 63):
        alone, st = system.solve(M[:, c], TOL, 2000)
        assert st["width"] == 64 and np.array_equal(alone[:, 0], block[:, c]), c
    rev, _ = system.solve(M[:, :64][:, ::-1], TOL, 2000)
    assert np.array_equal(rev[:, ::-1], block)
    wide, st = system.solve(M, TOL, 2000)          # another width, another lane, another group
    assert st["width"] == 192 and np.array_equal(wide[:, :64], block)
    # columns that stop at different iterations: zero columns, a single non-zero genotype, full columns
    mix = np.zeros((600, 7))
    mix[3, 1] = 1.0
    mix[:, 2] = M[:, 0]
    mix[599, 4] = 2.0
    mix[:, 5] = M[:, 17]
    mix[:, 6] = M[:, 130]
    ref = R.pcg_batched(ss_demo["Ann"], ss_demo["Ang"], mix, TOL, 2000)
    assert len(set(ref["col_iterations"].tolist())) >= 4
    together, st = system.solve(mix, TOL, 2000)
    assert np.all(together[:, [0, 3]] == 0.0)
    bounds(ss_demo["Ann"], ss_demo["Ang"], mix, together, TOL)
    for c in range(7):
        alone, _ = system.solve(mix[:, c], TOL, 2000)
        assert np.array_equal(alone[:, 0], together[:, c]), c
    assert np.array_equal(together[:, 2], block[:, 0]) and np.array_equal(together[:, 5], block[:, 17])


def test_deep_generated_pedigree(deep):  # noqa: F811
    """q = 19 897 in 415 runs of 48 rows, tol = 1e-10 (tests/test_impute_host.py says why not 1e-12)"""
    tol = 1e-10
    x, st = H.impute_device(deep["Ann"], deep["Ang"], deep["M"], tol=tol, max_iter=5000)
    ref = R.pcg_batched(deep["Ann"], deep["Ang"], deep["M"], tol, 5000)
    print("deep pedigree: device %d iterations in %d looks (%d parts), restatement %d; reported residual %.3g; %.3f s"
          % (st["iterations"], st["looks"], st["parts"], ref["iterations"], st["max_residual"], st["seconds"]))
    res, bn = bounds(deep["Ann"], deep["Ang"], deep["M"], x, tol)
    true = np.max(res / bn)
    assert abs(st["max_residual"] - true) <= 0.01 * true + 1e-16
    assert st["looks"] >= 4 and st["iterations"] > 96 and st["parts"] == 415


def test_non_convergence_is_an_error_that_names_the_columns(ss_demo, system):  # noqa: F811
    M = ss_demo["M"]
    live = int(np.count_nonzero(M.any(axis=0)))
    with pytest.raises(H.HibayesError, match="did not converge") as e:
        system.solve(M, TOL, 5)
    assert re.search(r"\b%d of 131 columns" % live, str(e.value)) and "within 5 iterations" in str(e.value), str(e.value)
    with pytest.raises(H.HibayesError, match="did not converge"):
        H.impute_device(ss_demo["Ann"], ss_demo["Ang"], M, tol=TOL, max_iter=5)
    x, _ = system.solve(M[:, :3], TOL, 2000)      # the handle is good for the next solve
    bounds(ss_demo["Ann"], ss_demo["Ang"], M[:, :3], x, TOL)


def test_ssbrm_prepare_on_the_device_route(ss_demo):  # noqa: F811
    host = ss_demo["pr"]
    # chunk = 2000: the 1000 markers and J in ONE call of the library, which cuts them into two blocks of W = 512, the second ragged (489)
    dev = H.ssbrm_prepare("T1 ~ 1", ss_demo["phe"], ss_demo["geno"], ss_demo["M_id"], ss_demo["ped"], impute="device", chunk=2000)
    for key in ("M_id", "Mn_id", "y_id", "y_id_comb", "n_genotyped_records", "n_other_records"):
        assert dev[key] == host[key], key
    for key in ("index", "y_indx", "y", "M", "J"):
        assert np.array_equal(dev[key], host[key]), key
    ng = host["n_genotyped_records"]
    assert np.array_equal(dev["y_J"][:ng], host["y_J"][:ng]) and np.array_equal(dev["y_M"][:ng], host["y_M"][:ng])
    assert dev["Mn"].shape == host["Mn"].shape == (900, 1000) and dev["Jn"].shape == host["Jn"].shape == (900,)
    st = dev["impute_stats"]
    assert "impute_stats" not in host and st["blocks"] == 2 and st["width"] == 512 and 1 <= st["iterations"] <= 10000
    Mall = np.column_stack([dev["M"], dev["J"]])
    xall = np.column_stack([dev["Mn"], dev["Jn"]])
    res, bn = bounds(dev["Ai_nn"], dev["Ai_ng"], Mall, xall, TOL)
    # against the dense solution on the columns that have one, against the host's factor on all (its own error: 1e-10 of the terms)
    err = np.linalg.norm(np.column_stack([dev["Mn"][:, :130], dev["Jn"]]) - ss_demo["dense"], axis=0)
    assert np.all(err <= 2 * TOL * bn[list(range(130)) + [1000]] / ss_demo["lmin"])
    assert np.max(np.abs(dev["Mn"] - host["Mn"])) < 1e-9 and np.max(np.abs(dev["Jn"] - host["Jn"])) < 1e-9
    zero = np.flatnonzero(~dev["M"].any(axis=0))
    assert zero.size == 54 and np.all(dev["Mn"][:, zero] == 0.0)
    n_rec = dev["index"] - 1
    assert np.array_equal(dev["y_M"][ng:], dev["Mn"][n_rec]) and np.array_equal(dev["y_J"][ng:], dev["Jn"][n_rec])


def test_ssbrm_on_the_device_route_is_Bayes_on_its_prepared_data(ss_demo):  # noqa: F811
    kw = dict(niter=60, nburn=20, thin=5, seed=20261020)
    fit = H.ssbrm("T1 ~ 1", ss_demo["phe"], ss_demo["geno"], ss_demo["M_id"], ss_demo["ped"], method="BayesCpi", verbose=False, impute="device", **kw)
    pr = H.ssbrm_prepare("T1 ~ 1", ss_demo["phe"], ss_demo["geno"], ss_demo["M_id"], ss_demo["ped"], impute="device")
    direct = H.Bayes(pr["y"], pr["y_M"], "BayesCpi", [0.95, 0.05], epsl_y_J=pr["y_J"], epsl_Gi=pr["Ai_nn"], epsl_index=pr["index"], genotype_bits=64,
                     verbose=False, **kw)
    assert fit["timing"]["impute_stats"]["iterations"] == pr["impute_stats"]["iterations"] >= 1
    for key in ("alpha", "Vg", "Ve", "mu", "pi", "Veps", "J"):
        np.testing.assert_array_equal(fit[key], direct[key], err_msg=key)
    np.testing.assert_array_equal(fit["epsilon"]["epsilon"], direct["epsilon"])
    for key in ("alpha", "epsilon", "Veps", "J"):
        np.testing.assert_array_equal(fit["MCMCsamples"][key], direct["MCMCsamples"][key], err_msg=key)
    assert fit["g"]["id"] == pr["M_id"] + pr["Mn_id"] and np.all(np.isfinite(fit["g"]["gebv"]))
