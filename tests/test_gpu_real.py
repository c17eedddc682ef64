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
from real_restatement import fma, stats_real

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


# ---- 10. the statistics at the edges of their row pairs ----
def vx_bound(X, var_ref):
    """What k_stats_real may be off by, per column, from its two passes (u = eps / 2 the unit roundoff, eps below absorbs second-order terms).
    Pass one gives mean_d = mean + dm with |dm| <= n u mean|x|: n - 1 additions in some order and the division. Pass two forms t_i = fl(mean_d -
    x_i), a2 = sum t_i^2 and a3 = sum t_i, and for ANY mean_d the identity sum (x_i - mean_d)^2 - (sum (x_i - mean_d))^2 / n = S = sum (x_i - mean)^2
    holds exactly: dm itself cancels, only roundings remain. With T = S + n dm^2 = sum (mean_d - x_i)^2: the roundings of the t_i (2 u T), a2's n
    fused terms in some order (n u T), a3's sum ((n + 1) u sum |t_i| <= (n + 1) u sqrt(n T), which enters as 2 |dm| times that) and the three
    operations of the last line (3 u T) — together below 8 n eps (T + |dm| sqrt(n T)), over n - 1. T / (n - 1) is the variance plus mean^2
    (n eps)^2-sized terms."""
    n = X.shape[0]
    dm = n * EPS * np.abs(X).mean(0)
    T = (n - 1) * var_ref + n * dm * dm
    return 8 * n * EPS * (T + dm * np.sqrt(n * T)) / (n - 1)


@pytest.mark.parametrize("n", [2, 3, 255, 257, 511, 513])
def test_statistics_at_odd_n_constant_columns_and_a_large_mean(n):
    """k_stats_real reads pairs of rows; at odd n the second element of the last pair is the zero padding row, which both passes guard with
    r0 + 1 < n. Without the second guard a (mean - 0)^2 enters the variance: caught here at every odd n. Without the first the padding's 0
    would be among the extremes of a constant column and the rule mn == mx would not fire — but that cannot be seen from outside: the correction
    term then brings the variance of a constant column to exactly 0 by itself (all t_i are one number; a host emulation of the kernel's order
    of sums found no constant and no odd n below 3 100 where it does not), and the extremes go nowhere else on this layout. The assertion on
    the constant columns therefore pins the result, not the guard. n = 511, 513 are either side of one trip of the 512-row loop. Columns: a constant 0.37 and a
    constant 1.0 (vx == 0.0 exactly, counted in nvar0), 1e6 + N(0, 1e-3) (the two-pass bound holds; the one-pass n S2 - S1^2 formula, evaluated
    here in doubles, misses the variance by orders of magnitude more than that bound), and a column that differs from 0.37 in its last row only.
    xpx: n fused terms in some order, n eps sum x^2."""
    rng = np.random.default_rng(n)
    m = 70
    X = dosages(rng, n, m) if n >= 6 else rng.uniform(0, 2, (n, m))
    for j in range(m):
        if X[:, j].min() == X[:, j].max():
            X[0, j] += 0.25
    X[:, 11] = 0.37
    X[:, 12] = 1.0
    X[:, 13] = 1e6 + rng.normal(0, 1e-3, n)
    X[:, 14] = 0.37
    X[n - 1, 14] = 0.38
    with Context(n, m, panel=64) as c:
        c.upload_real(X)
        xpx, vx, sumvx, nvar0 = c.marker_stats()
    rx, rv = stats_real(X)
    assert np.all(np.abs(xpx - rx) <= n * EPS * (X * X).sum(0))
    assert vx[11] == 0.0 and vx[12] == 0.0 and nvar0 == 2 and rv[11] == 0.0 and rv[12] == 0.0
    bound = vx_bound(X, rv)
    err = np.abs(vx - rv)
    print("n=%d: max vx err / bound = %.3g; column 1e6 + N(0, 1e-3): rel err %.3g, bound %.3g" % (n, np.max(err / np.maximum(bound, 1e-300)),
                                                                                          err[13] / rv[13], bound[13] / rv[13]))
    assert np.all(err <= bound), (n, np.flatnonzero(err > bound).tolist())
    assert vx[14] > 0 and bound[13] < 1e-9 * rv[13]
    s1, s2 = X[:, 13].sum(), (X[:, 13] * X[:, 13]).sum()
    onepass = (n * s2 - s1 * s1) / (n * (n - 1.0))
    assert abs(onepass - rv[13]) > 1e3 * bound[13]


# ---- 11. X alpha and the GEBV sample matrix on the layout ----
@pytest.mark.parametrize("n", [2, 255, 257])
def test_matvec_and_matmul_on_the_real_layout(n):
    """hb_ctx_matvec (k_xalpha_real) and Context.matmul (k_xmat_real) at m = 300: 320 padded columns, two column blocks of k_xalpha_real, whose
    block sums meet in atomics — a bound, nnz eps sum |x| |a| (a chain of at most nnz fused terms, then one addition). k_xmat_real has no atomics:
    per record acc = 0; acc = fma(x_j, a_j, acc) over the columns that carry an effect in any of the pass's eight records, in ascending column
    order — bit for bit at every n here (n = 257: a second workgroup with one live pair of rows), and the same bound. alpha with 0, 1, 5, 6,
    7, 8 and 40 non-zeros; 1, 8, 9 and 17 records, record sets of 5, 6, 7, 41 and 3 columns (nnz % 4 = 1, 2, 3, 1, 3: the last batch of four
    reads its columns through min(e0 + k, nnz - 1) and skips the moves at or past nnz), and at 17 records a whole pass of eight empty ones."""
    rng = np.random.default_rng(n)
    m = 300
    X = dosages(rng, n, m) if n >= 6 else rng.uniform(0, 2, (n, m))
    X[0, 7] = 1e-310
    X[n - 1, 290] = -0.0
    absX = np.abs(X)
    with Context(n, m, panel=64) as c:
        c.upload_real(X)
        assert c.layout()[0] == 64
        for nnz in (0, 1, 5, 6, 7, 8, 40):
            alpha = np.zeros(m)
            cols = np.sort(np.concatenate([rng.choice(256, nnz // 2, replace=False), 256 + rng.choice(m - 256, nnz - nnz // 2, replace=False)]))
            alpha[cols] = rng.normal(size=nnz)
            out = np.full(n, np.nan)
            H._lib.check(c.L.hb_ctx_matvec(c.h, alpha.ctypes.data, out.ctypes.data))
            want = wide_dot(X.T.copy(), alpha[:, None])[:, 0]
            lim = nnz * EPS * (absX @ np.abs(alpha))
            assert np.all(np.abs(out - want) <= lim), (n, nnz)
            if nnz == 0:
                assert not out.any()
        for R, sizes in ((1, [5]), (8, [6]), (9, [7, 8]), (17, [41, 0, 3])):
            A = np.zeros((m, R))
            for b, k in enumerate(sizes):
                cols = rng.choice(m, k, replace=False)
                recs = np.arange(8 * b, min(R, 8 * b + 8))
                for j in cols:                                  # every column of the pass's set in one of its records at least, in half of the others
                    on = rng.random(recs.size) < 0.5
                    on[rng.integers(recs.size)] = True
                    A[j, recs[on]] = rng.normal(size=int(on.sum()))
                assert (np.abs(A[:, recs]).sum(1) != 0).sum() == k
            out = c.matmul(A)
            out2 = c.matmul(A)
            assert out.tobytes() == out2.tobytes()
            for b in range(len(sizes)):
                recs = np.arange(8 * b, min(R, 8 * b + 8))
                support = np.flatnonzero(np.abs(A[:, recs]).sum(1) != 0)
                for r in recs:
                    acc = np.zeros(n)
                    for j in support:
                        acc = fma(X[:, j], A[j, r], acc)
                    assert out[:, r].tobytes() == acc.tobytes(), (n, R, int(r), "k_xmat_real in list order")
                    want = wide_dot(X.T.copy(), A[:, r:r + 1])[:, 0]
                    assert np.all(np.abs(out[:, r] - want) <= max(1, len(support)) * EPS * (absX @ np.abs(A[:, r]))), (n, R, int(r))
            if R == 17:
                assert not out[:, 8:16].any()


# ---- 12. genotype_bits = 64 from int8 input ----
def test_int8_columns_converted_on_the_device_at_odd_n():
    """k_i8_to_real: every code -128 .. 127 at n = 257 becomes the same number as a double, and the padding rows stay out of the statistics: a
    constant column of 5s and one of -3s have vx == 0.0 exactly (a padding 0 among the extremes would give them a variance), xpx is the exact
    integer, vx holds the two-pass bound."""
    rng = np.random.default_rng(12)
    n, m = 257, 70
    X8 = rng.integers(-128, 128, size=(n, m)).astype(np.int8)
    X8[:256, 0] = np.arange(-128, 128)
    X8[:, 9] = 5
    X8[:, 10] = -3
    X8 = np.asfortranarray(X8)
    with Context(n, m, panel=64) as c:
        c.upload(X8)
        c.set_layout(64)
        assert c.layout()[0] == 64
        back = c.download_real()
        xpx, vx, _, nvar0 = c.marker_stats()
    Xf = X8.astype(np.float64)
    assert back.tobytes() == np.asfortranarray(Xf).tobytes()
    assert np.array_equal(xpx, (X8.astype(np.int64) ** 2).sum(0).astype(np.float64))
    assert vx[9] == 0.0 and vx[10] == 0.0 and nvar0 == 2
    rx, rv = stats_real(Xf)
    assert np.all(np.abs(vx - rv) <= vx_bound(Xf, rv))
