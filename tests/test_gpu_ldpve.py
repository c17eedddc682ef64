"""The window pass on the LD matrix on the device (hibayes_amd/csrc/hb_ldquad.hip through LDMatrix.window_var, ld_window_pve, sbrm(pve=True);
ssbrm(pve=True) through the genotype pass) against numpy in longdouble, within the bound derived in ldpve_restatement.py, its bit-for-bit
properties, and against the two independent routes to the same quantity: the genotype pass and the sampler's own r_hat."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import hibayes_amd as H
from hibayes_amd import Context, LDMatrix
from hibayes_amd import pve as HP

import ldpve_restatement as R
import pve_restatement as RG
from test_gpu_pve import window_maps   # one, own, interleaved, spare ids, a zeroed window

pytestmark = pytest.mark.gpu

N = 40                                  # individuals behind every built matrix
MS = (1, 2, 63, 64, 65, 513, 1025)      # the wave edge and the 512-marker group of HB_LDM_GS
RS = (1, 8, 9)                          # one batch, a full one, two
KINDS = ("dense", "sparse", "block", "band", "odd")
DEMO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "demo", "demo")


@functools.lru_cache(maxsize=None)
def genotypes(m, n=N):
    X = np.asfortranarray(np.random.default_rng(1000 * n + m).integers(0, 3, (n, m)).astype(np.int8))
    X.setflags(write=False)
    return X


def effects(m, R_, seed=0):
    rng = np.random.default_rng(77 * m + R_ + seed)
    A = rng.standard_normal((m, R_)) * (rng.random((m, R_)) < 0.6)
    if m > 1:
        A[rng.integers(0, m), :] = 0.0
    return np.asfortranarray(A)


def mirrored(m, seed):
    Uq = np.triu(np.random.default_rng(seed).standard_normal((m, m)))
    return Uq + np.triu(Uq, 1).T


def from_mask(V, S):
    rows, cols = np.nonzero(S)
    A = sp.csc_matrix((V[rows, cols], (rows, cols)), shape=V.shape)
    A.sort_indices()
    return A


def band(m, hw=5):
    i, j = np.indices((m, m))
    return from_mask(mirrored(m, 5 * m + 1), np.abs(i - j) <= hw)


def odd(m):
    """a diagonal with neighbours at distance 1 and 3; marker 0 tied to the first 303 markers (a column of several passes of a wave); an empty
    column; and a column whose only entries are its two neighbours — outside its window wherever neighbours lie in other windows"""
    i, j = np.indices((m, m))
    S = np.isin(np.abs(i - j), (0, 1, 3))
    hub = min(m, 303)
    S[0, :hub] = S[:hub, 0] = True
    if m >= 3:
        e = m // 3
        S[e, :] = S[:, e] = False
    if m >= 8:
        d = 2 * m // 3
        S[d, :] = S[:, d] = False
        S[d, d - 1] = S[d - 1, d] = S[d, d + 1] = S[d + 1, d] = True
    return from_mask(mirrored(m, 7 * m + 2), S)


def open_handle(kind, m):
    """(the handle, the matrix it holds as the reference reads it: a dense array for the dense kind, CSC for every other)"""
    if kind in ("dense", "sparse", "block"):
        with Context(N, m) as c:
            c.upload(genotypes(m))
            ld = c.ldmat() if kind == "dense" else c.ldmat(chisq=5.0) if kind == "sparse" else c.ldmat(chr=(np.arange(m) % 3 + 1).astype(np.int32))
        assert ld.kind == {"dense": "dense", "sparse": "sparse", "block": "block-dense"}[kind]
        return ld, (ld.toarray() if kind == "dense" else ld.tocsc())
    V = band(m) if kind == "band" else odd(m)
    ld = LDMatrix.from_scipy(V)
    assert ld.kind == "sparse" and ld.nnz == V.nnz
    return ld, V


def check_within_bound(got, ref, bound, what):
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    assert np.all(err <= bound), (what, float(err.max()), np.argwhere(err > bound)[:4].tolist())
    assert np.all(got[bound == 0.0] == 0.0), what   # (no pair of effects on a stored entry: 0.0 exactly)
    return float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0


def batch_bound(V, A, w, nw):
    """ld_var_bound per batch of 8 records, as the device takes them: k, the columns of a window with an effect, is the batch's own"""
    parts = [R.ld_var_bound(V, A[:, r0:r0 + 8], w, nw) for r0 in range(0, A.shape[1], 8)]
    return np.hstack([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("kind", KINDS)
def test_window_forms_meet_the_derived_bound(kind, m):
    worst, negative = 0.0, 0
    ld, V = open_handle(kind, m)
    with ld:
        for wname, (w, nw, zero) in window_maps(m).items():
            A = effects(m, max(RS))
            if zero is not None:
                A[w == zero + 1] = 0.0
            var, tot = R.ld_window_var_ref(V, A, w, nw)      # (once for the 9 records: a record's reference does not depend on the others)
            for R_ in RS:
                gv, gt = ld.window_var(A[:, :R_], w, nw=nw)
                assert gv.shape == (nw, R_) and gt.shape == (R_,)
                what = (kind, m, R_, wname)
                bv, bt = batch_bound(V, A[:, :R_], w, nw)    # (k counts the columns its own batch lists, not those of the 9 records)
                worst = max(worst, check_within_bound(gv, var[:, :R_], bv, what), check_within_bound(gt, tot[:R_], bt, what + ("total",)))
                negative += int((gv < 0).sum())
                if zero is not None:
                    assert not gv[zero].any(), what
                if wname == "spare_ids":
                    assert not gv[3:].any(), what
    print("kind %s, m %d: worst error / bound = %.3g; %d negative forms" % (kind, m, worst, negative))
    assert worst <= 1.0
    if kind in ("band", "odd") and m >= 63:
        assert negative > 0      # (random symmetric values: indefinite, and stored as computed)


# ---- bit for bit ----
@pytest.fixture(scope="module", params=[("dense", 513), ("odd", 1025), ("sparse", 1025)], ids=lambda p: "%s-%d" % p)
def bits(request):
    kind, m = request.param
    R_ = 9
    A = effects(m, R_, seed=5)
    w = (np.arange(m) // 7 + 1).astype(np.uint32)
    nw = int(w.max())
    out = {"A": A, "w": w, "nw": nw, "m": m}
    ld, V = open_handle(kind, m)
    with ld:
        out["first"] = ld.window_var(A, w)
        out["again"] = ld.window_var(A, w)
        out["alone"] = {r: ld.window_var(A[:, r], w) for r in (0, 3, 7, 8)}
        out["batch8"] = ld.window_var(A[:, :8], w)
        B = A.copy()
        B[w != 4] *= -1.75
        B[(w == 9) | (w == 10)] = 0.0
        out["others_changed"] = ld.window_var(B, w)
        perm = np.random.default_rng(3).permutation(nw) + 1
        out["perm"] = perm
        out["renumbered"] = ld.window_var(A, perm[w - 1].astype(np.uint32))
        out["diag"] = ld.diagonal()
        out["closed"] = H.ld_window_pve(ld, A)
        out["pve"] = H.ld_window_pve(ld, A, w)
        out["pve_y"] = H.ld_window_pve(ld, A, w, vary=2.5, threshold=0.02)
    out["V"] = V
    out["by_matrix"] = H.ld_window_pve(V, A, w)      # a dense array through its CSC, a scipy matrix as it is
    return out


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_two_calls_give_the_same_bits(bits):
    assert same(bits["first"], bits["again"]) and np.isfinite(bits["first"][0]).all() and bits["first"][0].any()


def test_a_record_does_not_depend_on_the_batch_it_travels_in(bits):
    var, tot = bits["first"]       # 9 records: a batch of 8 and a batch of 1
    for r, (v1, t1) in bits["alone"].items():
        assert np.array_equal(v1[:, 0], var[:, r]) and t1[0] == tot[r], r
    assert np.array_equal(bits["batch8"][0], var[:, :8]) and np.array_equal(bits["batch8"][1], tot[:8])


def test_a_window_does_not_depend_on_the_other_windows_or_on_its_id(bits):
    var, tot = bits["first"]
    assert np.array_equal(bits["others_changed"][0][3], var[3])
    assert not bits["others_changed"][0][8:10].any() and bits["others_changed"][0][0].any()
    assert np.array_equal(bits["renumbered"][0][bits["perm"] - 1], var)
    assert np.array_equal(bits["renumbered"][1], tot)      # (the total's order depends on m alone)


def test_diagonal_closed_form_and_the_stated_arithmetic(bits):
    V, A, m = bits["V"], bits["A"], bits["m"]
    d = V.diagonal() if sp.issparse(V) else np.diag(V)
    assert np.array_equal(bits["diag"], d)
    got = bits["closed"]
    assert np.array_equal(got["var"], d[:, None] * A * A) and np.array_equal(got["total"], bits["first"][1]) and got["threshold"] == 1.0 / m
    var, tot = bits["first"]
    p, q = bits["pve"], bits["pve_y"]
    assert np.array_equal(p["var"], var) and np.array_equal(p["total"], tot) and np.all(tot != 0)
    assert np.array_equal(p["pve"], var / tot[None, :]) and np.array_equal(p["mean"], (var / tot[None, :]).mean(axis=1))
    assert p["threshold"] == 1.0 / bits["nw"] and np.array_equal(p["wppa"], (var / tot[None, :] > 1.0 / bits["nw"]).mean(axis=1))
    assert np.array_equal(q["pve"], var / 2.5) and np.array_equal(q["wppa"], (var / tot[None, :] > 0.02).mean(axis=1))
    assert sorted(p) == sorted(H.window_pve(genotypes(9), np.ones((9, 2)), np.ones(9, dtype=np.uint32)))      # window_pve()'s keys
    # the same matrix by value: a scipy matrix is the same CSC; a dense array loses nothing but exact zeros, which add 0.0
    if sp.issparse(V):
        assert same((bits["by_matrix"]["var"], bits["by_matrix"]["total"]), bits["first"])
    else:
        ref, rt = R.ld_window_var_ref(V, A, bits["w"], bits["nw"])
        bv, bt = batch_bound(V, A, bits["w"], bits["nw"])
        check_within_bound(bits["by_matrix"]["var"], ref, bv, "array")
        check_within_bound(bits["by_matrix"]["total"], rt, bt, "array total")


# ---- two independent routes to the same quantity ----
def test_against_the_genotype_pass():
    """alpha_w' V_ww alpha_w n / (n - 1) on ldmat()'s dense matrix is var(X_w alpha_w): hb_ldquad.hip against hb_pve.hip, within the sum of their
    derived bounds and of what the matrix's diagonal xx * xx / n may be off by"""
    m, R_ = 130, 9
    X = genotypes(m)
    A = effects(m, R_, seed=2)
    w = (np.arange(m) // 7 + 1).astype(np.uint32)
    nw = int(w.max())
    f = N / (N - 1.0)
    with Context(N, m) as c:
        c.upload(X)
        gv, gt = c.window_var(A, w)
        with c.ldmat() as ld:
            assert ld.kind == "dense"
            V = ld.toarray()
            lv, lt = ld.window_var(A, w)
    bgv, bgt = RG.var_bound(X, A, w, nw)
    blv, blt = batch_bound(V, A, w, nw)
    bdv, bdt = R.ld_diag_bound(np.diag(V), A, w, nw, N)
    tv, tt = bgv + f * (blv + bdv), bgt + f * (blt + bdt)
    ev, et = np.abs(lv * f - gv), np.abs(lt * f - gt)
    some = gv > 0     # (a short window can be without an effect in a record: 0.0 on both sides)
    print("LD pass x n / (n - 1) against the genotype pass: worst difference / tolerance = %.3g (windows), %.3g (total); relative %.3g"
          % (float((ev[some] / tv[some]).max()), float((et / tt).max()), float((ev[some] / gv[some]).max())))
    assert some.sum() > 150 and np.all(gt > 0) and np.all(ev <= tv) and np.all(et <= tt)
    assert not lv[~some].any() and not gv[~some].any()


@pytest.fixture(scope="module")
def sdemo():
    pl = H.read_plink(DEMO)
    rows = [l.split() for l in open(DEMO + ".ma")][1:]
    f = lambda x: float(x) if x != "NA" else np.nan
    return {"ss": np.array([[f(r[3]), f(r[4]), f(r[5]), f(r[7])] for r in rows]), "geno": pl["geno"], "map": pl["map"]}


def test_against_the_sampler(sdemo):
    """SBayesD keeps r_hat = xy - n V g: g_last' V g_last is g_last . (xy - r_hat) / n. Tolerance: the pass's bound and gamma_m on the dot."""
    ss = sdemo["ss"]
    m = ss.shape[0]
    with H.ldmat(sdemo["geno"], keep_on_device=True) as ld:
        r = H.SBayesD(ss, ld, "BayesCpi", [0.95, 0.05], niter=12, nburn=4, thin=2, seed=2468, verbose=False)
        g = r["g_last"]
        _, tot = ld.window_var(g, np.ones(m, dtype=np.uint32))
        V, d = ld.toarray(), ld.diagonal()
    est = ~np.isnan(ss[:, 1:]).any(axis=1)
    xy = np.where(est, d * r["n"] * np.where(est, ss[:, 1], 0.0), 0.0)
    terms = g.astype(np.longdouble) * (xy.astype(np.longdouble) - r["r_hat"]) / r["n"]
    _, bt = R.ld_var_bound(V, g, np.ones(m, dtype=int), 1)
    tol = bt[0] + R.gamma(m) * float(np.abs(terms).sum())
    err = abs(float(tot[0] - terms.sum()))
    print("total(g_last) %.17g against g_last . (xy - r_hat) / n: difference %.3g, tolerance %.3g" % (tot[0], err, tol))
    assert np.count_nonzero(g) > 5 and tot[0] > 0 and err <= tol


# ---- what is stored as computed ----
def test_a_negative_form_stays_negative_and_nan_needs_two_effects():
    V = sp.csc_matrix(np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 3.0]]))
    with LDMatrix.from_scipy(V) as ld:
        var, tot = ld.window_var(np.array([1.0, -1.0, 0.5]), np.array([1, 1, 2]))
        assert var[0, 0] == -2.0 and var[1, 0] == 0.75 and tot[0] == -1.25
        p = H.ld_window_pve(ld, np.array([1.0, -1.0, 0.5]), np.array([1, 1, 2]))
        assert p["var"][0, 0] == -2.0 and p["pve"][0, 0] == 1.6
    m = 70
    D = mirrored(m, 11)
    D[2, 2] = np.nan                      # a monomorphic marker's diagonal
    D[1, 40] = D[40, 1] = np.nan
    D[5, 69] = D[69, 5] = np.inf
    w = (np.arange(m) // 35 + 1).astype(np.uint32)
    A = np.ones((m, 4))
    A[[2, 40, 69], 0] = 0.0               # record 0: no NaN or Inf between two effects
    A[[2, 5], 1] = 0.0                    # record 1: (1, 40) across the windows: the total alone
    A[[40, 69], 2] = 0.0                  # record 2: (2, 2) inside window 1
    A[[2, 40], 3] = 0.0                   # record 3: the Inf across the windows
    ref, rt = R.ld_window_var_ref(sp.csc_matrix(D), A, w, 2)
    bv, bt = R.ld_var_bound(sp.csc_matrix(D), A, w, 2)
    with LDMatrix.from_scipy(sp.csc_matrix(D)) as ld:
        var, tot = ld.window_var(A, w)
    assert np.isfinite(var[:, 0]).all() and np.isfinite(tot[0])
    assert np.isfinite(var[:, 1]).all() and np.isnan(tot[1])
    assert np.isnan(var[0, 2]) and np.isfinite(var[1, 2]) and np.isnan(tot[2])
    assert np.isfinite(var[:, 3]).all() and np.isinf(tot[3])
    fin = np.isfinite(ref.astype(np.float64))
    assert np.array_equal(fin, np.isfinite(var)) and np.all(np.abs(var[fin] - ref[fin]) <= bv[fin])
    assert abs(tot[0] - rt[0]) <= bt[0]


def test_a_monomorphic_marker_on_the_dense_loader():
    """The dense kind stores no NaN: ldmat()'s dense arm divides by n alone (src/tXXmat.cpp:168, :179), so a monomorphic marker's diagonal is an
    exact zero there and the rest of its row zero or a rounding of it (the sparse arms divide by xx_i xx_j and keep the NaN). The dense loader's
    select on such a column: the column listed with an effect, everything finite and inside the bound; and a positive semi-definite matrix
    gives no negative form."""
    m = 130
    X = np.array(genotypes(m))
    X[:, 7] = 1
    X[:, 64] = 2
    A = effects(m, 9, seed=3)
    A[7], A[64, :4] = 1.5, -2.0
    w = (np.arange(m) // 7 + 1).astype(np.uint32)
    nw = int(w.max())
    with Context(N, m) as c:
        c.upload(np.asfortranarray(X))
        with c.ldmat() as ld:
            assert ld.kind == "dense"
            V = ld.toarray()
            var, tot = ld.window_var(A, w)
            d = ld.diagonal()
            own = ld.window_var(A, np.arange(1, m + 1, dtype=np.uint32))[0]
    assert np.isfinite(V).all() and np.abs(V[7]).max() < 1e-14 and np.abs(V[:, 64]).max() < 1e-14 and d[7] == 0.0 and d[64] == 0.0
    assert np.array_equal(d, np.diag(V))
    assert not own[7].any() and not own[64].any() and own[8].any()
    ref, rt = R.ld_window_var_ref(V, A, w, nw)
    bv, bt = batch_bound(V, A, w, nw)
    print("dense handle with two monomorphic markers: worst error / bound = %.3g" % max(check_within_bound(var, ref, bv, "mono"), check_within_bound(tot, rt, bt, "mono total")))
    assert np.isfinite(var).all() and np.all(var >= 0) and np.all(tot > 0)


# ---- sbrm(pve=True), ssbrm(pve=True) ----
def equal_apart_from(a, b, skip):
    assert sorted(k for k in a if k not in skip) == sorted(k for k in b if k not in skip)
    for k in a:
        if k in skip:
            continue
        if isinstance(a[k], dict):
            equal_apart_from(a[k], b[k], skip)
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k
        else:
            assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), k


@pytest.mark.parametrize("route", ["dense", "dense_handle", "sparse"])
def test_sbrm_returns_the_windows_pve(sdemo, route):
    """dense: a host matrix through SBayesD() (the pass on its CSC); dense_handle: ldmat(keep_on_device=True) -> sbrm() on the handle of kind dense
    (the sampler and the pass on its dense device copy); sparse: ldmat(chisq = 5, keep_on_device=True) -> sbrm(sparse_ld=True) on the handle and on its CSC
    by value. (BayesR there: thresholded at chisq = 5 the demo's matrix is indefinite, and under it BayesCpi's chain leaves the finite numbers —
    test_gpu_sbayess.py —, which ld_window_pve() refuses like any non-finite effect.)"""
    ss, mp = sdemo["ss"], sdemo["map"]
    w = H.cutwind_by_num(*H.bayes._map_columns(mp), 50)
    nw = int(w.max())
    if route == "dense":
        kw = dict(method="BayesCpi", niter=40, nburn=10, thin=5, seed=7, verbose=False)
        with H.ldmat(sdemo["geno"], keep_on_device=True) as full:
            mat = full.toarray()
        hand_ld = LDMatrix.from_scipy(sp.csc_matrix(mat))
        first = mat
    elif route == "dense_handle":
        kw = dict(method="BayesCpi", niter=40, nburn=10, thin=5, seed=7, verbose=False)
        hand_ld = first = mat = H.ldmat(sdemo["geno"], keep_on_device=True)
        assert hand_ld.kind == "dense"
    else:
        kw = dict(method="BayesR", niter=60, nburn=20, thin=4, seed=97, verbose=False, sparse_ld=True)
        hand_ld = first = H.ldmat(sdemo["geno"], chisq=5.0, keep_on_device=True)
        assert hand_ld.kind == "sparse"
        mat = hand_ld.tocsc()
    nrec = (kw["niter"] - kw["nburn"]) // kw["thin"]
    with hand_ld:
        if route == "dense_handle":     # (the last check below, while the handle is open)
            mean_fit = H.sbrm(ss, mat, pve=True, store_alpha=False, **kw)
        plain = H.sbrm(ss, first, map=mp, windnum=50, **kw)
        fit = H.sbrm(ss, first, map=mp, windnum=50, pve=True, **kw)
        assert "pve" not in plain
        equal_apart_from(fit, plain, ("pve", "timing"))
        samples = fit["MCMCsamples"]["alpha"]
        assert samples.shape == (ss.shape[0], nrec) and np.isfinite(samples).all() and samples.any()
        d = hand_ld.diagonal()
        vary = HP.sbayes_vary(ss, d)
        hand = H.ld_window_pve(hand_ld, samples, w, vary=vary)
    loop_vary, n, count_y = R.sbayes_vary_loop(ss, d)
    assert (n, count_y) == (fit["n"], fit["count_y"]) and abs(vary - loop_vary) <= 2 * R.gamma(len(d)) * loop_vary
    p = fit["pve"]
    assert p["var"].shape == (nw, nrec) and p["var"].any()
    for k in ("var", "total", "pve", "mean", "wppa", "threshold"):
        assert np.array_equal(p[k], hand[k]), k
    assert np.array_equal(p["pve"], p["var"] / vary)
    assert p["WIND"] == fit["gwas"]["WIND"] == ["wind%d" % (k + 1) for k in range(nw)] and p["NUM"] == [int((w == k + 1).sum()) for k in range(nw)]
    assert len(p["CHR"]) == len(p["START"]) == len(p["END"]) == nw and all(a <= b for a, b in zip(p["START"], p["END"]))
    if route == "sparse":     # the matrix by value: the handle is made once and swept
        equal_apart_from(H.sbrm(ss, mat, map=mp, windnum=50, pve=True, **kw), fit, ("timing",))
    # without the samples: the posterior mean, one record; without windows: every marker its own
    if route != "dense_handle":
        mean_fit = H.sbrm(ss, mat, pve=True, store_alpha=False, **kw)
    q = mean_fit["pve"]
    assert q["var"].shape == (ss.shape[0], 1) and "wppa" not in q and "WIND" not in q
    assert np.array_equal(q["var"][:, 0], d * mean_fit["alpha"] * mean_fit["alpha"])


def test_ssbrm_returns_the_windows_pve(sdemo):
    phe = H.read_table(DEMO + ".phe")
    ped = np.array([l.split() for l in open(DEMO + ".ped")][1:], dtype=object)
    M_id = [r[1] for r in H.read_plink(DEMO)["fam"]]
    kw = dict(method="BayesCpi", map=sdemo["map"], windnum=50, niter=40, nburn=10, thin=5, seed=7, verbose=False)
    plain = H.ssbrm("T1 ~ 1", phe, sdemo["geno"], M_id, ped, **kw)
    fit = H.ssbrm("T1 ~ 1", phe, sdemo["geno"], M_id, ped, pve=True, **kw)
    assert "pve" not in plain
    # every other key bit for bit, but one: e = y - ... - X alpha comes from hb_ctx_matvec, which on the fp64 layout adds a row's partial sums
    # with atomics (k_xalpha_real) in an order that differs from run to run, with or without pve. Each run's sum of the m products is within
    # gamma_m of the exact one whatever its order: two runs are within 2 gamma_m sum_j |x_ij alpha_j| of each other.
    equal_apart_from(fit, plain, ("pve", "timing", "e"))
    again = H.ssbrm("T1 ~ 1", phe, sdemo["geno"], M_id, ped, **kw)
    equal_apart_from(again, plain, ("timing", "e"))
    print("e of two runs without pve: %d of %d entries differ, by at most %.3g; with pve against without: %d, %.3g"
          % (int(np.sum(again["e"]["e"] != plain["e"]["e"]) - np.isnan(plain["e"]["e"]).sum()), len(plain["e"]["e"]),
             float(np.nanmax(np.abs(again["e"]["e"] - plain["e"]["e"]))),
             int(np.sum(fit["e"]["e"] != plain["e"]["e"]) - np.isnan(plain["e"]["e"]).sum()), float(np.nanmax(np.abs(fit["e"]["e"] - plain["e"]["e"])))))
    pr = H.ssbrm_prepare("T1 ~ 1", phe, sdemo["geno"], M_id, ped)
    m = len(fit["alpha"])
    room = 2 * R.gamma(m) * float((np.abs(np.vstack([pr["M"], pr["Mn"]])) @ np.abs(fit["alpha"])).max())
    assert fit["e"]["id"] == plain["e"]["id"] and np.array_equal(np.isnan(fit["e"]["e"]), np.isnan(plain["e"]["e"]))
    assert np.nanmax(np.abs(fit["e"]["e"] - plain["e"]["e"])) <= room and np.nanmax(np.abs(again["e"]["e"] - plain["e"]["e"])) <= room
    w = H.cutwind_by_num(*H.bayes._map_columns(sdemo["map"]), 50)
    hand = H.window_pve(np.vstack([pr["M"], pr["Mn"]]), fit["MCMCsamples"]["alpha"], w, vary=float(np.var(pr["y"], ddof=1)))
    p = fit["pve"]
    assert p["var"].shape == (int(w.max()), 6) and np.all(p["total"] > 0)
    for k in ("var", "total", "pve", "mean", "wppa", "threshold"):
        assert np.array_equal(p[k], hand[k]), k
    assert p["Wind"] == fit["gwas"]["Wind"] and p["N"] == fit["gwas"]["N"]


# ---- refusals ----
def test_refusals_of_the_entry():
    m = 6
    L = H.lib()
    with LDMatrix.from_scipy(band(m, 1)) as ld:
        var, tot, w = np.zeros((2, 3), order="F"), np.zeros(3), np.array([1, 1, 2, 2, 1, 2], dtype=np.uint32)

        def call(A, rows, R_, wi, nw):
            A = np.asfortranarray(A, dtype=np.float64)
            return L.hb_ldm_window_var(ld._handle(), A.ctypes.data, max(rows, 1), rows, R_, wi.ctypes.data, nw, var.ctypes.data, 2, tot.ctypes.data), L.hb_last_error().decode()

        assert call(np.ones((m, 1)), m, 1, w, 2)[0] == 0
        rc, text = call(np.ones((m + 1, 1)), m + 1, 1, w, 2)
        assert rc == 1 and "one row per marker of the matrix (6)" in text
        rc, text = call(np.ones((m, 1)), m, 0, w, 2)
        assert rc == 1 and "R must be >= 1" in text
        for bad in (np.inf, -np.inf, np.nan):
            A = np.ones((m, 2))
            A[4, 1] = bad
            rc, text = call(A, m, 2, w, 2)
            assert rc == 1 and "the effects must be finite (marker 5, record 2)" in text
        for wid in (0, 3):
            w2 = w.copy()
            w2[3] = wid
            rc, text = call(np.ones((m, 1)), m, 1, w2, 2)
            assert rc == 1 and "window ids in 1 .. nw (marker 4 has %d)" % wid in text
        assert text.startswith("hb_ldm_window_var: ")
        # and through the Python surface
        with pytest.raises(H.HibayesError, match="one row per marker") as e:
            ld.window_var(np.ones(m + 1), w)
        assert e.value.status == 1
        with pytest.raises(H.HibayesError, match="R must be >= 1"):
            ld.window_var(np.ones((m, 0)), w)
        with pytest.raises(ValueError, match="window ids in 1 .. nw"):
            ld.window_var(np.ones(m), w, nw=1)
        v0, t0 = ld.window_var(np.zeros((m, 2)), w)
        assert v0.shape == (2, 2) and not v0.any() and not t0.any()
    with pytest.raises(ValueError, match="was closed"):
        ld.window_var(np.ones(m), w)
    with pytest.raises(H.HibayesError, match="must equal its transpose"):
        H.ld_window_pve(np.array([[1.0, 0.5], [0.25, 1.0]]), np.ones(2))
