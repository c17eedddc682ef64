"""The window-variance pass on the device (hibayes_amd/csrc/hb_pve.hip through Context.window_var, window_pve and ibrm(pve=True)) against
numpy in longdouble, within the bound derived in pve_restatement.py, and its bit-for-bit properties."""
import functools

import numpy as np
import pytest

import hibayes_amd as H
from hibayes_amd import Context
from hibayes_amd import pve as HP

import pve_restatement as R

pytestmark = pytest.mark.gpu

NS, MS, RS = (2, 5, 257, 1025), (1, 9, 130), (1, 8, 9)   # the 4-row thread, the wave and the 1024-row block edges; one batch, a full one, two
CODES = {"012": (0, 2), "-101": (-1, 1), "pm127": (-127, 127)}


@functools.lru_cache(maxsize=None)
def genotypes(n, m, codes):
    lo, hi = CODES[codes]
    rng = np.random.default_rng(1000 * n + m + (hi - lo))
    X = rng.integers(lo, hi + 1, (n, m)).astype(np.int8)
    if codes == "pm127" and n > 1:
        X[0, :], X[1, :] = 127, -127
    X = np.asfortranarray(X)
    X.setflags(write=False)
    return X


def effects(m, R_, seed=0):
    rng = np.random.default_rng(77 * m + R_ + seed)
    A = rng.standard_normal((m, R_)) * (rng.random((m, R_)) < 0.6)
    if m > 1:
        A[rng.integers(0, m), :] = 0.0
    return np.asfortranarray(A)


def window_maps(m):
    """name -> (windindx, nw, the 0-based window whose effects are set to zero or None)"""
    blocks = (np.arange(m) * 4 // m + 1).astype(np.uint32)
    return {"one": (np.ones(m, dtype=np.uint32), 1, None), "own": (np.arange(1, m + 1, dtype=np.uint32), m, None),
            "interleaved": ((np.arange(m) % 3 + 1).astype(np.uint32), min(m, 3), None), "spare_ids": ((np.arange(m) % 3 + 1).astype(np.uint32), 7, None),
            "zero_window": (blocks, int(blocks.max()), int(blocks[m // 2]) - 1)}


@functools.lru_cache(maxsize=None)
def reference(n, m, R_, codes, wname):
    """(A, windindx, nw, zeroed window, var_ref, total_ref, var_bound, total_bound): computed once, shared by the layouts"""
    X = genotypes(n, m, codes)
    w, nw, zero = window_maps(m)[wname]
    A = effects(m, R_)
    if zero is not None:
        A[w == zero + 1] = 0.0
    var, tot = R.window_var_ref(X, A, w, nw)
    bv, bt = R.var_bound(X, A, w, nw)
    for a in (A, w):
        a.setflags(write=False)
    return A, w, nw, zero, var, tot, bv, bt


def open_context(X, layout):
    c = Context(X.shape[0], X.shape[1])
    if layout == 64:
        c.upload_real(X.astype(np.float64))
    else:
        c.upload(X)
        if layout == 2:
            c.set_layout(2, keep_int8=False)
    assert c.layout()[0] == layout
    return c


def check_within_bound(got, ref, bound, what):
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    assert np.all(err <= bound), (what, float(err.max()), np.argwhere(err > bound)[:4].tolist())
    assert np.all(got[bound == 0.0] == 0.0), what   # (no effect in the window: never visited, 0.0 exactly)
    return float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0


@pytest.mark.parametrize("layout,codes", [(8, "012"), (8, "-101"), (8, "pm127"), (2, "012"), (64, "012"), (64, "-101")])
def test_window_variances_meet_the_derived_bound(layout, codes):
    worst = 0.0
    for n in NS:
        for m in MS:
            with open_context(genotypes(n, m, codes), layout) as c:
                for R_ in RS:
                    for wname in window_maps(m):
                        A, w, nw, zero, var, tot, bv, bt = reference(n, m, R_, codes, wname)
                        gv, gt = c.window_var(A, w, nw=nw)
                        assert gv.shape == (nw, R_) and gt.shape == (R_,)
                        what = (layout, codes, n, m, R_, wname)
                        worst = max(worst, check_within_bound(gv, var, bv, what), check_within_bound(gt, tot, bt, what + ("total",)))
                        if zero is not None:
                            assert not gv[zero].any(), what
                        if wname == "spare_ids":
                            assert not gv[3:].any(), what
    print("layout %d, codes %s: worst error / bound = %.3g" % (layout, codes, worst))
    assert worst <= 1.0


def test_the_two_bit_layout_takes_no_negative_codes():
    """codes -1..1 have no 2-bit form: the layout itself refuses them (status 4), so there is no such case of the pass to run"""
    with Context(5, 9) as c:
        c.upload(genotypes(5, 9, "-101"))
        with pytest.raises(H.HibayesError, match=r"needs genotype codes 0\.\.3") as e:
            c.set_layout(2)
        assert e.value.status == 4


def test_a_case_that_needs_the_shift():
    """fp64 columns 1000 + noise: the one-pass formula without a shift loses what the bound keeps"""
    n, m = 1025, 9
    rng = np.random.default_rng(12)
    X = 1000.0 + 0.1 * rng.standard_normal((n, m))
    A = np.asfortranarray(rng.standard_normal((m, 2)))
    w = (np.arange(m) % 3 + 1).astype(np.uint32)
    var, tot = R.window_var_ref(X, A, w, 3)
    bv, bt = R.var_bound(X, A, w, 3, real=True)
    with Context(n, m) as c:
        c.upload_real(X)
        gv, gt = c.window_var(A, w)
    worst = max(check_within_bound(gv, var, bv, "windows"), check_within_bound(gt, tot, bt, "total"))
    naive = np.array([[R.onepass_uncentred(X[:, w == k + 1], A[w == k + 1, r]) for r in range(2)] for k in range(3)])
    nerr = np.abs(naive.astype(np.longdouble) - var).astype(np.float64)
    print("worst error / bound = %.3g; the uncentred one-pass formula: %.3g" % (worst, float(np.max(nerr / bv))))
    assert np.all(bv < 1e-9 * var.astype(np.float64)) and np.all(nerr > bv)


# ---- bit for bit ----
@pytest.fixture(scope="module")
def bits():
    n, m, R_ = 1025, 130, 9
    X = genotypes(n, m, "012")
    A = effects(m, R_, seed=5)
    w = (np.arange(m) // 7 + 1).astype(np.uint32)    # 19 windows, the last one short
    out = {"X": X, "A": A, "w": w, "nw": int(w.max())}
    with open_context(X, 8) as c:
        out["vx"] = c.marker_stats()[1]
        out["first"] = c.window_var(A, w)
        out["again"] = c.window_var(A, w)
        out["alone"] = {r: c.window_var(A[:, r], w) for r in (0, 3, 7, 8)}
        out["batch8"] = c.window_var(A[:, :8], w)
        B = A.copy()
        B[w != 4] *= -1.75
        B[(w == 9) | (w == 10)] = 0.0
        out["others_changed"] = c.window_var(B, w)
        perm = np.random.default_rng(3).permutation(out["nw"]) + 1
        out["perm"] = perm
        out["renumbered"] = c.window_var(A, perm[w - 1].astype(np.uint32))
        out["single"] = c.window_var(A, np.arange(1, m + 1, dtype=np.uint32))
        out["closed"] = H.window_pve(c, A)
        out["pve"] = H.window_pve(c, A, w)
        out["pve_y"] = H.window_pve(c, A, w, vary=2.5, threshold=0.02)
        out["pve_one"] = H.window_pve(c, A[:, 0], w)
    with open_context(X, 2) as c:
        out["two_bit"] = c.window_var(A, w)
    with open_context(X, 64) as c:
        out["fp64"] = c.window_var(A, w)
    out["matrix"] = H.window_pve(np.array(X), A, w)
    out["matrix_real"] = H.window_pve(X.astype(np.float64) + 0.25, A[:, :2], w)
    with Context(n, m) as c:
        c.upload_real(X.astype(np.float64) + 0.25)
        out["context_real"] = c.window_var(A[:, :2], w)
    return out


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_two_calls_and_the_layouts_give_the_same_bits(bits):
    assert same(bits["first"], bits["again"])
    assert same(bits["first"], bits["two_bit"])
    assert same(bits["first"], bits["fp64"])     # (the same integers as doubles: the same chains, four rows to a thread on every layout)


def test_a_record_does_not_depend_on_the_batch_it_travels_in(bits):
    var, tot = bits["first"]
    for r, (v1, t1) in bits["alone"].items():
        assert np.array_equal(v1[:, 0], var[:, r]) and t1[0] == tot[r], r
    assert np.array_equal(bits["batch8"][0], var[:, :8]) and np.array_equal(bits["batch8"][1], tot[:8])


def test_a_window_does_not_depend_on_the_other_windows_or_on_its_id(bits):
    var = bits["first"][0]
    assert np.array_equal(bits["others_changed"][0][3], var[3])
    assert not bits["others_changed"][0][8:10].any() and bits["others_changed"][0][0].any()
    assert np.array_equal(bits["renumbered"][0][bits["perm"] - 1], var)


def test_one_marker_windows_are_the_closed_form(bits):
    A, vx = bits["A"], bits["vx"]
    closed = vx[:, None] * A * A
    ref, _ = R.window_var_ref(bits["X"], A, np.arange(1, 131), 130)
    bv, _ = R.var_bound(bits["X"], A, np.arange(1, 131), 130)
    print("one-marker windows: worst error / bound = %.3g" % check_within_bound(bits["single"][0], ref, bv, "single"))
    assert np.all(np.abs(closed.astype(np.longdouble) - ref) <= bv + 4 * R.U * np.abs(closed))   # (vx is exact on integers: three roundings)
    got = bits["closed"]
    assert np.array_equal(got["var"], closed) and np.array_equal(got["total"], bits["first"][1])
    assert got["threshold"] == 1.0 / 130


def test_pve_mean_and_wppa_are_the_stated_arithmetic(bits):
    var, tot = bits["first"]
    p = bits["pve"]
    assert np.array_equal(p["var"], var) and np.array_equal(p["total"], tot) and np.all(tot > 0)
    assert np.array_equal(p["pve"], var / tot[None, :]) and np.array_equal(p["mean"], (var / tot[None, :]).mean(axis=1))
    assert p["threshold"] == 1.0 / 19 and np.array_equal(p["wppa"], (var / tot[None, :] > 1.0 / 19).mean(axis=1))
    assert 0 < p["wppa"].max() <= 1 and p["wppa"].min() < 1
    q = bits["pve_y"]
    assert np.array_equal(q["pve"], var / 2.5) and np.array_equal(q["mean"], (var / 2.5).mean(axis=1))
    assert np.array_equal(q["wppa"], (var / tot[None, :] > 0.02).mean(axis=1))
    one = bits["pve_one"]
    assert "wppa" not in one and one["var"].shape == (19, 1) and np.array_equal(one["var"][:, 0], var[:, 0])


def test_a_matrix_goes_the_way_of_a_context(bits):
    assert np.array_equal(bits["matrix"]["var"], bits["first"][0]) and np.array_equal(bits["matrix"]["total"], bits["first"][1])
    assert np.array_equal(bits["matrix_real"]["var"], bits["context_real"][0]) and np.array_equal(bits["matrix_real"]["total"], bits["context_real"][1])
    assert not np.array_equal(bits["matrix_real"]["total"], bits["first"][1][:2])


def test_refusals_on_the_device():
    with Context(8, 4) as c:   # no genotypes yet
        with pytest.raises(H.HibayesError, match="no genotypes on the device") as e:
            c.window_var(np.ones(4), np.ones(4, dtype=np.uint32))
        assert e.value.status == 1
        c.upload(np.ones((8, 4), dtype=np.int8))
        with pytest.raises(H.HibayesError, match="effects must be finite"):
            c.window_var(np.array([1.0, np.inf, 0, 0]), np.ones(4, dtype=np.uint32))
        var, tot = c.window_var(np.ones(4), np.array([1, 1, 2, 2], dtype=np.uint32))
        assert not var.any() and not tot.any()      # (constant columns: nothing varies)
        var, tot = c.window_var(np.zeros((4, 2)), np.array([1, 1, 2, 2], dtype=np.uint32))
        assert var.shape == (2, 2) and not var.any() and not tot.any()


# ---- ibrm(pve=True) ----
KW = dict(niter=60, nburn=20, thin=5, seed=11, verbose=False)


def test_ibrm_returns_the_windows_pve(demo):
    pl, phe = demo["plink"], demo["phe"]
    args = dict(data=phe, M=pl["geno"], M_id=demo["ids"], method="BayesCpi", map=pl["map"], windnum=50, **KW)
    plain = H.ibrm("T1 ~ 1", **args)
    fit = H.ibrm("T1 ~ 1", pve=True, **args)
    assert "pve" not in plain and np.array_equal(fit["gwas"], plain["gwas"]) and np.array_equal(fit["alpha"], plain["alpha"])
    samples = fit["MCMCsamples"]["alpha"]
    m = pl["geno"].shape[1]
    w = H.cutwind_by_num(*H.bayes._map_columns(pl["map"]), 50)
    nw = int(w.max())
    hand = H.window_pve(pl["geno"], samples, w, vary=float(np.var(demo["y"], ddof=1)))
    p = fit["pve"]
    assert samples.shape == (m, 8) and p["var"].shape == (nw, 8) and fit["gwas"].shape == (nw,)
    for k in ("var", "total", "pve", "mean", "wppa"):
        assert np.array_equal(p[k], hand[k]), k
    assert p["WIND"] == ["wind%d" % (k + 1) for k in range(nw)] and p["NUM"] == [int((w == k + 1).sum()) for k in range(nw)]
    assert len(p["CHR"]) == len(p["START"]) == len(p["END"]) == nw and all(a <= b for a, b in zip(p["START"], p["END"]))
    assert np.all(p["total"] > 0) and np.all(p["pve"] >= 0) and np.all(p["var"].sum(axis=0) > 0)
    # without the samples: the posterior mean, one record
    mean_fit = H.ibrm("T1 ~ 1", pve=True, store_alpha=False, **args)
    q = mean_fit["pve"]
    assert q["var"].shape == (nw, 1) and "wppa" not in q
    hand1 = H.window_pve(pl["geno"], mean_fit["alpha"], w, vary=float(np.var(demo["y"], ddof=1)))
    assert np.array_equal(q["var"], hand1["var"]) and np.array_equal(q["pve"], hand1["pve"])
