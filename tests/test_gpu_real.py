"""The fp64 resident layout (genotype_bits = 64): real-valued genotypes — imputed dosages — from the kernels up to Bayes() and ibrm().
The round trip, the statistics, the mat-vec and the Gram blocks alone against higher-precision products, the chain draw for draw
against the live oracle (which takes a double X), against the integer engine on integer input, with the host blocks and the GWAS
windows, and the refusals."""
import functools
import math

import numpy as np
import pytest

import hibayes_amd as H
from hibayes_amd.engine import Context
from oracle import oracle as O

pytestmark = pytest.mark.gpu

MODELS = [("BayesCpi", [0.95, 0.05], None), ("BayesC", [0.9, 0.1], None), ("BayesRR", [0.95, 0.05], None),
          ("BayesA", [0.95, 0.05], None), ("BayesBpi", [0.95, 0.05], None), ("BayesB", [0.9, 0.1], None),
          ("BayesL", [0.95, 0.05], None), ("BayesR", [0.95, 0.02, 0.02, 0.01], [0, 1e-4, 1e-3, 1e-2])]   # tests/test_gpu_parity.py::MODELS
EPS = 2.0 ** -52
WIDE = np.longdouble if np.finfo(np.longdouble).nmant > 52 else None


def genotypes012(rng, n, m):
    p = rng.uniform(0.05, 0.5, m)
    return (rng.random((n, m)) < p).astype(np.float64) + (rng.random((n, m)) < p)


def dosages(rng, n, m):
    """0/1/2 genotypes with a third of the rows replaced by imputed-looking ones: half of those the average of two genotyped rows
    (multiples of 0.5), half convex combinations of three with irrational weights."""
    G = genotypes012(rng, n, m)
    X = G.copy()
    imp = rng.choice(n, n // 3, replace=False)
    for i in imp[: imp.size // 2]:
        a, b = rng.choice(n, 2, replace=False)
        X[i] = 0.5 * (G[a] + G[b])
    w = np.array([1.0 / math.sqrt(2.0), 1.0 / math.pi, 0.0])
    w[2] = 1.0 - w[0] - w[1]
    for i in imp[imp.size // 2:]:
        a, b, c = rng.choice(n, 3, replace=False)
        X[i] = w[0] * G[a] + w[1] * G[b] + w[2] * G[c]
    return X


@functools.lru_cache(maxsize=None)
def problem():
    """n = 300, m = 200 from a fixed seed; columns 3 and 130 constant (one of them fractional)."""
    rng = np.random.default_rng(20251020)
    n, m = 300, 200
    X = dosages(rng, n, m)
    X[:, 3] = 0.37
    X[:, 130] = 1.0
    beta = np.zeros(m)
    beta[rng.choice(m, 12, replace=False)] = rng.normal(0, 1, 12)
    y = X @ beta + rng.normal(0, 1.0, n)
    X.setflags(write=False)
    y.setflags(write=False)
    return y, X


@functools.lru_cache(maxsize=None)
def oracle_fit(model):
    y, X = problem()
    _, Pi, fold = [q for q in MODELS if q[0] == model][0]
    return O.bayes(y, X, model, Pi, fold=fold, niter=16, nburn=6, thin=2, seed=424242, rng=O.RNG_PHILOX, store_alpha=True)


def wide_dot(A, B):
    """A' B in the widest arithmetic here: 80-bit long doubles, or exactly rounded sums (math.fsum) of the double products"""
    if WIDE is not None:
        return (A.astype(WIDE).T @ B.astype(WIDE)).astype(np.float64)
    out = np.zeros((A.shape[1], B.shape[1]))
    for i in range(A.shape[1]):
        for j in range(B.shape[1]):
            out[i, j] = math.fsum(A[:, i] * B[:, j])
    return out


# ---- 1. round trip ----
def test_round_trip_is_bit_exact_and_a_nan_is_refused():
    rng = np.random.default_rng(1)
    n, m = 300, 70
    X = dosages(rng, n, m)
    X[5, 7] = -0.0
    X[6, 8] = 1e-310          # a denormal travels too
    with Context(n, m, panel=64) as c:
        c.upload_real(X)
        assert c.layout()[0] == 64
        back = c.download_real()
        assert back.tobytes() == np.asfortranarray(X).tobytes()
        assert c.pipeline()[:3] == (0, 0, 1) and "fp64 resident layout" in c.pipeline_note()
        c.set_pipeline(1, 2, 7)
        assert c.pipeline()[:3] == (0, 0, 1)
        bad = X.copy()
        bad[17, 3] = np.nan
        with pytest.raises(H.HibayesError) as ei:
            c.upload_real(bad)
        assert ei.value.status == 1 and str(ei.value) == "NAs are not allowed in genotype."
        bad[17, 3] = np.inf
        with pytest.raises(H.HibayesError) as ei:
            c.upload_real(bad)
        assert ei.value.status == 1
    y = X @ rng.normal(0, 0.1, m) + rng.normal(0, 1, n)
    r = H.Bayes(y, X, "BayesCpi", [0.95, 0.05], niter=6, nburn=2, thin=2, verbose=False)   # auto, the default precise = 2
    assert r["timing"]["resident_bits"] == 64
    r = H.Bayes(y, np.rint(X), "BayesCpi", [0.95, 0.05], niter=6, nburn=2, thin=2, verbose=False)
    assert r["timing"]["resident_bits"] in (8, 2)   # an integer-valued float matrix keeps today's route


# ---- 2. statistics ----
def test_statistics_two_pass_and_constant_fractional_column():
    rng = np.random.default_rng(2)
    n, m = 300, 70
    X = dosages(rng, n, m)
    X[:, 11] = 0.37
    with Context(n, m, panel=64) as c:
        c.upload_real(X)
        xpx, vx, sumvx, nvar0 = c.marker_stats()
    np.testing.assert_allclose(xpx, (X * X).sum(0), rtol=1e-13)
    others = np.arange(m) != 11
    np.testing.assert_allclose(vx[others], X[:, others].var(0, ddof=1), rtol=1e-13, atol=0)
    assert vx[11] == 0.0 and nvar0 == 1     # (numpy's own two-pass variance of that column is 1.6e-30, not 0)
    y = X @ rng.normal(0, 0.1, m) + rng.normal(0, 1, n)
    r = H.Bayes(y, X, "BayesRR", [0.95, 0.05], niter=10, nburn=4, thin=2, verbose=False, genotype_bits=64)
    a = r["MCMCsamples"]["alpha"]
    assert np.all(a[11] == 0.0) and np.all(a[np.arange(m) != 11] != 0.0)


# ---- 3. the mat-vec alone ----
@pytest.mark.parametrize("panel", [64, 512])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4096, 4097])
def test_matvec_alone_against_a_wider_product(n, panel):
    """hb_ctx_dot on the real layout; per column |d - exact| <= n 2^-52 sum |x_i r_i|. n = 4097 crosses one 256 x 16-row chunk (two row splits),
    the ragged m a column tile and a panel edge. A context needs two individuals: n = 1 is refused when it is created, on every layout."""
    if n == 1:
        with pytest.raises(H.HibayesError) as ei:
            Context(1, 5, panel=panel)
        assert ei.value.status == 1
        return
    rng = np.random.default_rng(1000 * n + panel)
    for m in (1, 63, 64, 65, 513):
        X = dosages(rng, n, m) if n >= 6 else rng.random((n, m))
        r = rng.normal(0, 3.0, n)
        with Context(n, m, panel=panel, precise=2) as c:
            c.upload_real(X)
            c.set_residual(r, np.zeros(n))
            d = c.dot()
            d2 = c.dot()
        want = wide_dot(X, r[:, None])[:, 0]
        bound = n * EPS * (np.abs(X) * np.abs(r)[:, None]).sum(0)
        err = np.abs(d - want)
        print("n=%d m=%d panel=%d: max err / bound = %.3g" % (n, m, panel, np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound), (n, m, panel)
        assert d.tobytes() == d2.tobytes()


# ---- 4. the Gram blocks ----
@pytest.mark.parametrize("m,panel", [(65, 64), (513, 64), (513, 512)])
def test_gram_blocks_symmetric_with_xpx_on_the_diagonal(m, panel):
    rng = np.random.default_rng(m + panel)
    n = 257
    X = dosages(rng, n, m)
    with Context(n, m, panel=panel) as c:
        c.upload_real(X)
        xpx = c.marker_stats()[0]
        c.build_gram()
        P = c.panel
        npan = (m + P - 1) // P
        Gs = [c.gram_real(p) for p in range(npan)]
        c.build_gram()
        assert all(c.gram_real(p).tobytes() == Gs[p].tobytes() for p in range(npan))   # built the same twice
        with pytest.raises(H.HibayesError):
            c.gram(0)
    Xp = np.zeros((n, npan * P))
    Xp[:, :m] = X
    xp = np.zeros(npan * P)
    xp[:m] = xpx
    for p, G in enumerate(Gs):
        B = Xp[:, p * P:(p + 1) * P]
        want = wide_dot(B, B)
        bound = n * EPS * (np.abs(B).T @ np.abs(B))
        assert np.all(np.abs(G - want) <= bound), (m, panel, p)
        assert G.tobytes() == np.ascontiguousarray(G.T).tobytes()
        assert np.diag(G).tobytes() == xp[p * P:(p + 1) * P].tobytes()


# ---- 5. draw for draw against the live oracle ----
@pytest.mark.parametrize("model,Pi,fold", MODELS)
@pytest.mark.parametrize("panel", [64, 512])
def test_draw_for_draw_against_the_live_oracle(model, Pi, fold, panel):
    y, X = problem()
    ref = oracle_fit(model)
    assert ref["vx"][3] == 0.0 and ref["vx"][130] == 0.0
    r = H.Bayes(y, X, model, Pi, fold=fold, niter=16, nburn=6, thin=2, seed=424242, verbose=False, panel=panel)   # auto layout, default precise
    assert r["timing"]["resident_bits"] == 64
    tol = 1e-6 if model == "BayesL" else 1e-9
    a, b = r["MCMCsamples"]["alpha"], ref["s_alpha"]
    assert np.array_equal(a != 0, b != 0)
    np.testing.assert_allclose(a, b, rtol=tol, atol=1e-12)
    np.testing.assert_allclose([r["Vg"], r["Ve"], r["h2"], r["mu"]], [ref["Vg"], ref["Ve"], ref["h2"], ref["mu"]], rtol=tol)
    np.testing.assert_allclose(r["pi"], ref["pi"], rtol=tol, atol=1e-14)
    np.testing.assert_allclose(r["pip"], ref["pip"], rtol=0, atol=1e-12)
    assert r["alpha"][3] == 0 and r["alpha"][130] == 0


# ---- 6. the same chain as the integer engine ----
@pytest.mark.parametrize("model,Pi", [("BayesCpi", [0.95, 0.05]), ("BayesR", [0.95, 0.02, 0.02, 0.01]), ("BayesRR", [0.95, 0.05])])
def test_integer_input_runs_the_integer_engines_chain(model, Pi):
    rng = np.random.default_rng(6)
    n, m = 300, 200
    X8 = genotypes012(rng, n, m).astype(np.int8)
    y = X8 @ rng.normal(0, 0.1, m) + rng.normal(0, 1, n)
    fold = [0, 1e-4, 1e-3, 1e-2] if model == "BayesR" else None
    kw = dict(fold=fold, niter=16, nburn=6, thin=2, seed=99, verbose=False)
    a = H.Bayes(y, X8, model, Pi, genotype_bits=64, **kw)     # int8 input converted on the device
    b = H.Bayes(y, X8, model, Pi, genotype_bits=8, precise=1, **kw)
    assert a["timing"]["resident_bits"] == 64 and b["timing"]["resident_bits"] == 8
    sa, sb = a["MCMCsamples"]["alpha"], b["MCMCsamples"]["alpha"]
    assert np.array_equal(sa != 0, sb != 0)
    np.testing.assert_allclose(sa, sb, rtol=1e-9, atol=1e-12)
    c = H.Bayes(y, X8.astype(np.float64), model, Pi, genotype_bits=64, **kw)   # ... and uploaded as doubles: the same columns
    assert c["MCMCsamples"]["alpha"].tobytes() == sa.tobytes()


# ---- 7. the host blocks through ibrm() ----
def test_ibrm_full_formula_on_fractional_genotypes(demo, monkeypatch):
    pl, phe = demo["plink"], demo["phe"]
    rng = np.random.default_rng(7)
    M = pl["geno"].astype(np.float64)
    quarter = rng.choice(M.shape[0], M.shape[0] // 4, replace=False)
    for i in quarter:
        a, b = rng.choice(M.shape[0], 2, replace=False)
        M[i] = 0.5 * (pl["geno"][a].astype(np.float64) + pl["geno"][b]) if i % 2 else (pl["geno"][a] / math.sqrt(2.0) + (1 - 1 / math.sqrt(2.0)) * pl["geno"][b])
    seen = {}
    import hibayes_amd.bayes as HB
    inner = HB.Bayes

    def spy(**kw):
        seen.update(kw)
        return inner(**kw)

    monkeypatch.setattr(HB, "Bayes", spy)
    kw = dict(niter=300, nburn=100, thin=5, seed=666666)
    fit = H.ibrm("T1 ~ season + bwt + (1 | loc) + (1 | dam)", data=phe, M=M, M_id=demo["ids"], method="BayesCpi", Pi=[0.98, 0.02],
                 verbose=False, **kw)
    assert fit["timing"]["resident_bits"] == 64
    ref = O.bayes(seen["y"], seen["X"], "BayesCpi", [0.98, 0.02], Cmat=seen["C_"], R=seen["R"], rng=O.RNG_PHILOX, **kw)
    assert fit["beta_names"] == ["seasonSpring", "seasonSummer", "seasonWinter", "bwt"]
    np.testing.assert_allclose(fit["beta"], ref["beta"], rtol=1e-7)
    np.testing.assert_allclose(fit["Vr"], ref["Vr"], rtol=1e-7)
    np.testing.assert_allclose(fit["r"]["Estimation"], ref["r"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(fit["alpha"], ref["alpha"], rtol=1e-6, atol=1e-10)
    np.testing.assert_allclose(fit["e"]["e"], ref["e"], rtol=1e-7, atol=1e-8)
    assert len(fit["g"]["gebv"]) == 600 and len(fit["e"]["id"]) == 300
    np.testing.assert_allclose(fit["g"]["gebv"], M @ fit["alpha"], rtol=1e-10, atol=1e-12)
    gs = fit["MCMCsamples"]["g"]
    assert gs.shape == (600, 40)
    np.testing.assert_allclose(gs, M @ fit["MCMCsamples"]["alpha"], rtol=1e-12, atol=1e-12)


# ---- 8. GWAS windows ----
def test_gwas_windows_on_the_real_layout():
    y, X = problem()
    wind = (np.arange(X.shape[1]) // 20 + 1).astype(np.uint32)
    kw = dict(niter=60, nburn=20, thin=5, seed=7)
    r = H.Bayes(y, X, "BayesCpi", [0.95, 0.05], windindx=wind, verbose=False, **kw)
    ref = O.bayes(y, X, "BayesCpi", [0.95, 0.05], windindx=wind, rng=O.RNG_PHILOX, **kw)
    assert r["timing"]["resident_bits"] == 64 and r["gwas"].size == wind.max()
    np.testing.assert_allclose(r["gwas"], ref["gwas"], rtol=0, atol=1e-12)


# ---- 9. refusals ----
def test_refusals_name_the_layout():
    y, X = problem()
    kw = dict(niter=4, nburn=2, thin=1, verbose=False)

    def refused(**more):
        a = dict(kw)
        a.update(more)
        model = a.pop("model", "BayesCpi")
        with pytest.raises(H.HibayesError) as ei:
            H.Bayes(y, X, model, [0.95, 0.05], **a)
        assert ei.value.status == 4, str(ei.value)
        return str(ei.value)

    assert "fp64 resident layout" in refused(shard_rows=True, genotype_bits=64)
    assert "fp64 resident layout" in refused(shard_rows=True)                      # auto would choose it
    n = y.size
    assert "fp64 resident layout" in refused(model="BSLMM", Kival=np.ones(n), Ki=np.eye(n), genotype_bits=64)
    assert "hb_ctx_upload_genotype_real" in refused(genotype_bits=8)
    assert "hb_ctx_upload_genotype_real" in refused(genotype_bits=2)
    with Context(n, X.shape[1]) as c:
        c.upload_real(X)
        for call in (c.ldmat, c.grm, lambda: c.set_layout(2)):
            with pytest.raises(H.HibayesError) as ei:
                call()
            assert ei.value.status == 4 and "fp64 resident layout" in str(ei.value)
        c.upload(np.rint(X).astype(np.int8))      # integer genotypes put the context back on the int8 columns
        assert c.layout()[0] == 8
