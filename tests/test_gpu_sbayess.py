"""The summary-level sampler on a SPARSE LD matrix (SBayesS(), hb_sbayes_run_sparse: k_ss_pre, k_ss_group, k_ss_update; reference
src/SBayesS.cpp:277-600) on the MI355X, draw for draw against the Python restatement (tests/sbayess_restatement.py, pinned to
the C oracle by test_sbayess_host.py) under the same Philox counters. Tolerances are the dense sampler's own
(test_gpu_sbayes.py::_compare): inclusion pattern identical, alpha rtol 1e-9 (1e-6 for BayesL), PIP atol 1e-12, r_hat
1e-7 max|r_hat|."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import hibayes_amd as H
from oracle import oracle as O
from sbayess_restatement import sbayess_restatement
from test_gpu_sbayes import _compare
from test_oracle_sbayes import MODELS, sdemo  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CPI = ("BayesCpi", [0.95, 0.05], None)
BR = ("BayesR", [0.95, 0.02, 0.02, 0.01], [0, 1e-4, 1e-3, 1e-2])


def bits(x):
    """the bit patterns of floating-point data (so that a NaN equals the same NaN and -0.0 differs from 0.0), anything else as it is"""
    x = np.asarray(x)
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64) if x.dtype.kind == "f" else x


def same_run(a, b):
    """everything two runs return except their timings, bit for bit"""
    for k in a:
        if k == "timing":
            continue
        if k == "MCMCsamples":
            for q in a[k]:
                assert np.array_equal(bits(a[k][q]), bits(b[k][q])), "MCMCsamples." + q
        else:
            assert np.array_equal(bits(a[k]), bits(b[k])), k
    return True


@pytest.fixture(scope="module")
def geno():
    X = H.read_plink(os.path.join(G, "demo", "demo"))["geno"]
    assert X.shape == (600, 1000) and X.dtype == np.int8
    return X


@pytest.fixture(scope="module")
def sp5(geno):
    """the genome-wide chi^2-sparsified matrix of the demo on the device: 20.8 % of the entries, 30 empty columns, two groups"""
    with H.ldmat(geno, chisq=5.0, keep_on_device=True) as ld:
        A = ld.tocsc()
        per = np.diff(A.indptr)
        assert ld.kind == "sparse" and 0.15 < A.nnz / 1e6 < 0.25 and (per == 0).sum() == 30 and per.max() < 512
        yield {"ld": ld, "csc": A}


@pytest.fixture(scope="module")
def strong():
    """test_gpu_sbayes.py's generator of many candidates under strong LD (m = 1700: three groups of 512 and a tail of 164, LD
    blocks of 32), the matrix thresholded on the host: r^2 n <= 5 -> 0"""
    rng = np.random.default_rng(31)
    n, m = 600, 1700
    p = np.repeat(rng.uniform(0.1, 0.5, (m + 31) // 32), 32)[:m]
    X = np.empty((n, m))
    for j in range(m):
        fresh = (rng.random(n) < p[j]).astype(float) + (rng.random(n) < p[j])
        X[:, j] = fresh if j % 32 == 0 else np.where(rng.random(n) < 0.92, X[:, j - 1], fresh)
    ld = np.cov(X, rowvar=False, ddof=0)
    ld = np.triu(ld) + np.triu(ld, 1).T                   # (exactly symmetric whatever the BLAS did)
    beta = np.zeros(m)
    causal = rng.choice(m, 120, replace=False)
    beta[causal] = rng.normal(0, 0.5, causal.size)
    y = X @ beta + rng.normal(0, 1.0, n)
    Xc = X - X.mean(0)
    xx = (Xc ** 2).sum(0)
    b = (Xc * (y - y.mean())[:, None]).sum(0) / xx
    se = np.sqrt(((y - y.mean()) ** 2).sum() / (n - 2) / xx)
    ss = np.column_stack([X.mean(0) / 2, b, se, np.full(m, float(n))])
    d = np.sqrt(np.diag(ld))
    r = ld / np.outer(d, d)
    A = sp.csc_matrix(np.where(r * r * n <= 5.0, 0.0, ld))
    A.sort_indices()
    assert 0.01 < A.nnz / m ** 2 < 0.5
    return {"ss": ss, "csc": A}


@pytest.mark.parametrize("model,Pi,fold", MODELS)
def test_demo_from_the_handle_draw_for_draw_and_from_scipy_bit_for_bit(sdemo, sp5, model, Pi, fold):
    """Five of these chains leave the region where a variance is a variance, and the device has to follow the reference there.
    Thresholding at chisq = 5 leaves the demo's LD matrix indefinite (smallest eigenvalue -0.559), so g' ldm g can be negative and
    with it the sweep's genetic variance (src/SBayesS.cpp:531); `vare_ < 0 -> vare_ = vara_ * 0.5` (:538) then makes the residual
    variance negative too. In the next sweep varei < 0: the inclusion inequality turns round for the markers whose v * varei is
    negative, log(varg * lhs + 1) (:376) and sqrt(varei / v) (:387) are NaN for others, which the reference INCLUDES with a NaN
    effect, and from the sweep after that everything a stored entry reaches is NaN. Under seed 97 the first negative Vg comes in
    sweep 0 (BayesL: -417.6), 12 (BayesCpi: -1897.7), 15 (BayesC: -169.9), 18 (BayesBpi: -427.4) and 57 (BayesRR: -425.5) of the
    60. The comparison is the same as everywhere: NaN where the reference has NaN, the PIPs of the sweeps in between exact, the
    rows of r_hat no stored entry reaches finite and equal. BayesA, BayesB and BayesR keep positive variances here."""
    kw = dict(fold=fold, niter=60, nburn=20, thin=4, seed=97)
    r = H.SBayesS(sdemo["ss"], sp5["ld"], model, Pi, verbose=False, **kw)
    assert same_run(r, H.SBayesS(sdemo["ss"], sp5["csc"], model, Pi, verbose=False, **kw))      # through hb_ldm_from_csc
    ref = sbayess_restatement(sdemo["ss"], sp5["csc"], model, Pi, **kw)
    print(model, "restatement's Vg records:", ref["s_Vg"], "device's:", r["MCMCsamples"]["Vg"][0])
    _compare(r, ref, 1e-6 if model == "BayesL" else 1e-9)
    np.testing.assert_allclose(r["MCMCsamples"]["Vg"][0], ref["s_Vg"], rtol=1e-6 if model == "BayesL" else 1e-9)
    assert np.any(ref["s_alpha"] != 0)


@pytest.mark.parametrize("model,Pi,fold", [CPI, BR])
def test_per_chromosome_handle_with_interleaved_ids_and_windows(geno, sdemo, model, Pi, fold):
    chrs = ["X" if j in (5, 333, 334, 999) else str(j * 7 % 3 + 1) for j in range(1000)]     # test_gpu_ldmat.py's `ref`
    mp = [["snp%d" % j, c, 1000 + j] for j, c in enumerate(chrs)]
    wind = (np.arange(1000) // 20 + 1).astype(np.uint32)
    kw = dict(fold=fold, niter=60, nburn=20, thin=4, seed=97, windindx=wind)
    with H.ldmat(geno, mp, chisq=5.0, ldchr=False, keep_on_device=True) as ld:
        assert ld.kind == "block-sparse"
        A = ld.tocsc()
        r = H.SBayesS(sdemo["ss"], ld, model, Pi, verbose=False, **kw)
    coo = A.tocoo()
    assert (np.abs(coo.row - coo.col) > 512).any()             # every group's rows scatter over the whole range
    ref = sbayess_restatement(sdemo["ss"], A, model, Pi, **kw)
    _compare(r, ref)
    np.testing.assert_allclose(r["gwas"], ref["gwas"], rtol=0, atol=1e-12)
    assert r["nw"] == 50 and ref["gwas"].any()


@pytest.mark.parametrize("model,Pi,fold", [("BayesCpi", [0.7, 0.3], None), ("BayesB", [0.5, 0.5], None),
                                           ("BayesR", [0.6, 0.2, 0.15, 0.05], [0, 1e-3, 1e-2, 1e-1]), ("BayesRR", [0.95, 0.05], None)])
def test_groups_with_many_candidates_under_strong_ld(strong, model, Pi, fold):
    kw = dict(fold=fold, niter=12, nburn=4, thin=2, seed=77)
    ref = sbayess_restatement(strong["ss"], strong["csc"], model, Pi, **kw)
    assert (ref["s_alpha"][:, -1] != 0).sum() > 200       # (the regime the test is about)
    _compare(H.SBayesS(strong["ss"], strong["csc"], model, Pi, verbose=False, **kw), ref, 1e-8)


@pytest.mark.parametrize("model,Pi,fold", MODELS)
def test_all_models_on_the_strong_ld_matrix(strong, model, Pi, fold):
    """every model where the reference's chain holds (Vg and Ve stay positive over these 24 sweeps on this matrix, though it is
    indefinite too: smallest eigenvalue -0.293)"""
    kw = dict(fold=fold, niter=24, nburn=8, thin=4, seed=77)
    ref = sbayess_restatement(strong["ss"], strong["csc"], model, Pi, **kw)
    assert np.isfinite(ref["s_Vg"]).all() and (ref["s_Vg"] > 0).all() and (ref["s_Ve"] > 0).all()
    r = H.SBayesS(strong["ss"], strong["csc"], model, Pi, verbose=False, **kw)
    _compare(r, ref, 1e-6 if model == "BayesL" else 1e-8)
    np.testing.assert_allclose(r["MCMCsamples"]["Vg"][0], ref["s_Vg"], rtol=1e-6 if model == "BayesL" else 1e-8)


@pytest.mark.parametrize("model,Pi,fold", [("BayesCpi", [0.9, 0.1], None), ("BayesR", [0.875, 0.0625, 0.03125, 0.03125], [0, 1e-4, 1e-3, 1e-2])])
def test_truncation_redraws_and_the_effect_set_to_zero_after_101(model, Pi, fold):
    rng = np.random.default_rng(5)
    n, m = 400, 203                                        # test_gpu_sbayes.py's ragged generator
    p = rng.uniform(0.1, 0.5, m)
    X = ((rng.random((n, m)) < p).astype(float) + (rng.random((n, m)) < p).astype(float))
    ld = np.cov(X, rowvar=False, ddof=0)
    ld = np.triu(ld) + np.triu(ld, 1).T
    beta = np.zeros(m)
    causal = rng.choice(m, 10, replace=False)
    beta[causal] = rng.normal(0, 1, 10)
    y = X @ beta + rng.normal(0, 1.0, n)
    Xc = X - X.mean(0)
    b = (Xc * (y - y.mean())[:, None]).sum(0) / (Xc ** 2).sum(0)
    se = np.sqrt(((y - y.mean()) ** 2).sum() / (n - 2) / (Xc ** 2).sum(0))
    big = causal[np.argmax(np.abs(b[causal]))]
    b[big] *= 3.0                                          # vary is a mean over m markers: one outlier has b^2 vx > vary
    ss = np.column_stack([p, b, se, np.full(m, float(n))])
    ss[17, 1] = np.nan
    d = np.sqrt(np.diag(ld))
    A = sp.csc_matrix(np.where((ld / np.outer(d, d)) ** 2 * n <= 5.0, 0.0, ld))
    A.sort_indices()
    kw = dict(fold=fold, niter=80, nburn=30, thin=5, seed=11)
    ref = sbayess_restatement(ss, A, model, Pi, **kw)
    print("marker-sweeps that redrew: %d, ended at zero after 101: %d" % (ref["redraws"], ref["zeroed"]))
    assert ref["redraws"] > ref["zeroed"] >= 1        # redraws that succeed, and redraws that give up
    r = H.SBayesS(ss, A, model, Pi, verbose=False, **kw)
    _compare(r, ref)
    np.testing.assert_allclose(r["MCMCsamples"]["Vg"][0], ref["s_Vg"], rtol=1e-9)          # (they see the restart of the sum of squares)
    np.testing.assert_allclose(r["MCMCsamples"]["Ve"][0], ref["s_Ve"], rtol=1e-9)


@pytest.mark.parametrize("model,Pi,fold", [CPI, ("BayesRR", [0.95, 0.05], None)])
def test_full_matrix_against_the_c_oracle(geno, sdemo, model, Pi, fold):
    """independent of the Python restatement: on the genome-wide dense kind every entry is stored (varediff = 0) and the demo
    redraws nothing, so SBayesS() is SBayesD()"""
    kw = dict(fold=fold, niter=60, nburn=20, thin=4, seed=97)
    with H.ldmat(geno, keep_on_device=True) as ld:
        assert ld.kind == "dense"
        D = ld.toarray()
        r = H.SBayesS(sdemo["ss"], ld, model, Pi, verbose=False, **kw)
    _compare(r, O.sbayes(sdemo["ss"], D, model, Pi, rng=O.RNG_PHILOX, store_alpha=True, **kw))


def test_the_markers_own_residual_variance_is_live(sdemo, sp5):
    kw = dict(niter=12, nburn=4, thin=2, seed=2468, verbose=False)
    a = H.SBayesS(sdemo["ss"], sp5["ld"], "BayesCpi", [0.95, 0.05], **kw)
    b = H.SBayesD(sdemo["ss"], sp5["ld"], "BayesCpi", [0.95, 0.05], **kw)
    assert not np.array_equal(a["MCMCsamples"]["alpha"], b["MCMCsamples"]["alpha"])
    assert np.any(a["MCMCsamples"]["alpha"] != 0) and np.any(b["MCMCsamples"]["alpha"] != 0)


def test_two_runs_of_one_call_agree_bit_for_bit(strong):
    kw = dict(niter=12, nburn=4, thin=2, seed=77, verbose=False)
    with H.LDMatrix.from_scipy(strong["csc"]) as ld:
        a = H.SBayesS(strong["ss"], ld, "BayesRR", [0.95, 0.05], **kw)
        b = H.SBayesS(strong["ss"], ld, "BayesRR", [0.95, 0.05], **kw)
    assert same_run(a, b) and np.any(a["MCMCsamples"]["alpha"] != 0)


def test_a_quarter_of_a_million_markers_without_a_dense_copy():
    """m = 250 000, a symmetric band of half-width 5: the dense copy would be 500 GB, so the run succeeds only without one"""
    m, hw = 250000, 5
    rng = np.random.default_rng(3)
    A = sp.diags([np.full(m - abs(k), 0.6 ** abs(k)) for k in range(-hw, hw + 1)], list(range(-hw, hw + 1)), format="csc")
    A.sort_indices()
    assert A.nnz == m * (2 * hw + 1) - hw * (hw + 1)
    b = rng.normal(0, 0.02, m)
    b[rng.choice(m, 500, replace=False)] += rng.normal(0, 0.5, 500)
    ss = np.column_stack([np.full(m, 0.3), b, np.full(m, 0.03), np.full(m, 1000.0)])
    r = H.SBayesS(ss, A, "BayesCpi", [0.95, 0.05], niter=3, nburn=0, thin=1, seed=5, verbose=False)
    xy = r["n"] * A.diagonal() * b
    np.testing.assert_allclose(r["r_hat"], xy - r["n"] * (A @ r["g_last"]), rtol=0, atol=1e-9 * np.abs(xy).max())
    assert np.any(r["g_last"] != 0) and r["n_records"] == 3 and r["n"] == 1000


def test_refusals_and_sbrm_on_the_sparse_route(strong):
    ss, A = strong["ss"], strong["csc"]
    rows, cols = A.nonzero()
    k = np.flatnonzero(rows != cols)[0]
    B = A.tolil(copy=True)
    B[rows[k], cols[k]] = A[rows[k], cols[k]] * 2          # one entry above the diagonal, its mirror left alone
    with pytest.raises(H.HibayesError, match="must equal its transpose") as ei:
        H.SBayesS(ss, B.tocsc(), "BayesCpi", [0.95, 0.05], niter=4, nburn=2, thin=1, verbose=False)
    assert ei.value.status == 1
    with H.LDMatrix.from_scipy(A[:100, :100]) as small:
        assert small.kind == "sparse" and small.shape == (100, 100)
        with pytest.raises(H.HibayesError, match="Number of SNPs not equals."):
            H.SBayesS(ss, small, "BayesCpi", [0.95, 0.05], niter=4, nburn=2, thin=1, verbose=False)
    m = ss.shape[0]
    full = np.column_stack([np.zeros((m, 3)), ss[:, 0], ss[:, 1], ss[:, 2], np.zeros(m), ss[:, 3]])
    f = H.sbrm(full, A, method="BayesCpi", niter=40, nburn=10, verbose=False, sparse_ld=True)
    assert f["n_records"] == 6 and f["model"] == "Summary level Bayesian model fit by [BayesCpi]" and np.isfinite(f["h2"])
    assert f["call"] == "b ~ nD^{-1}V alpha + e"
    with H.LDMatrix.from_scipy(A) as ld:
        g = H.sbrm(full, ld, method="BayesCpi", niter=40, nburn=10, verbose=False, sparse_ld=True)
    assert np.array_equal(f["alpha"], g["alpha"])
