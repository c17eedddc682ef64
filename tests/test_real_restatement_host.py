"""tests/real_restatement.py against plain formulations, without a GPU: the one-rounding fma against exact rational arithmetic on
adversarial operands, chain_panel against a sequential sampler that recomputes x_t . r from an explicitly updated residual in long doubles,
update_real against r - X[:, cols] @ deltas, stats_real against numpy's variance."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import real_restatement as R

EPS = 2.0 ** -52
WIDE = np.longdouble


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------------------
# fma
# ------------------------------------------------------------------------------------------------------------------------
def adversarial_triples():
    rng = np.random.default_rng(52)
    A, B, C = [], [], []

    def add(a, b, c):
        A.extend(np.atleast_1d(a).tolist())
        B.extend(np.atleast_1d(b).tolist())
        C.extend(np.atleast_1d(c).tolist())

    k = 1500
    add(rng.normal(size=k), rng.normal(size=k), rng.normal(size=k))                                   # ordinary
    add(rng.normal(size=k) * 1e8, rng.normal(size=k), rng.normal(size=k) * 1e-8)                      # c far below the product
    add(rng.normal(size=k) * 1e-9, rng.normal(size=k), rng.normal(size=k) * 1e9)                      # the product far below c
    a, b = rng.normal(size=k), rng.normal(size=k)                                                   # cancellation: the result is the product's error
    add(a, b, -(a * b))
    a, b = rng.integers(-1000, 1000, k).astype(float), rng.integers(-1000, 1000, k).astype(float)   # ... and to an exact zero
    add(a, b, -(a * b))
    # near-ties: a b + c within a rounding of c of the midpoint between two doubles, on either side, also next to a power of two
    a, b = rng.uniform(0.5, 2.0, k), rng.uniform(0.5, 2.0, k)
    base = np.where(rng.random(k) < 0.2, 2.0 ** rng.integers(-3, 4, k).astype(float), rng.uniform(0.1, 8.0, k))
    base = np.where(rng.random(k) < 0.5, base, np.nextafter(base, 0.0))
    for ai, bi, r0 in zip(a, b, base):
        mid = (Fraction(float(r0)) + Fraction(float(np.nextafter(r0, np.inf)))) / 2
        add(ai, bi, float(mid - Fraction(float(ai)) * Fraction(float(bi))))
        add(-ai, bi, -float(mid - Fraction(float(ai)) * Fraction(float(bi))))
    # exact ties: the product is a multiple of 2^-53 that lands on a midpoint above c = 1, 2, 1 - 2^-53
    for c0 in (1.0, 2.0, 1.0 - 2.0 ** -53, -1.0, 4.0):
        for mult in range(-9, 10):
            add(float(mult), 2.0 ** -53, c0)
            add(float(mult), 2.0 ** -54, c0)
            add(float(mult) * 2.0 ** -27, 2.0 ** -27, c0)
    # denormals: operands, products and sums below 2^-1022; products that underflow altogether
    tiny = np.array([5e-324, 1e-310, 2.2250738585072014e-308, 1e-300, 3e-162, 1e-160, 2.0 ** -537, 2.0 ** -538])
    for x in tiny:
        for y in (1.0, 0.5, 3.0, 1e-10, 1e10, 2.0 ** -537, 1.5 * 2.0 ** -537, 1e-160):
            for z in (0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 1e-300, 1.0):
                add(x, y, z)
                add(-x, y, z)
    add(rng.normal(size=300) * 1e-155, rng.normal(size=300) * 1e-155, rng.normal(size=300) * 1e-310)
    # signed zeros
    for x in (0.0, -0.0, 1.0, -1.0):
        for y in (0.0, -0.0, 2.0, -2.0):
            for z in (0.0, -0.0, 2.0, -2.0):
                add(x, y, z)
    # large operands: the split would overflow
    add([2.0 ** 995, 2.0 ** 1000, -2.0 ** 1010, 3.0], [2.0 ** -10, 2.0 ** -1000, 2.0 ** 10, 2.0 ** 1000], [1.0, 2.0 ** -1070, 2.0 ** 1020, -2.0 ** 1001])
    return np.array(A), np.array(B), np.array(C)


def test_fma_is_one_rounding_on_adversarial_operands():
    a, b, c = adversarial_triples()
    assert a.size > 5000
    got = R.fma(a, b, c)
    want = np.array([R.fma_fraction(x, y, z) for x, y, z in zip(a, b, c)])
    diff = np.flatnonzero(bits(got) != bits(want))
    assert diff.size == 0, [(a[i].hex(), b[i].hex(), c[i].hex(), got[i].hex(), want[i].hex()) for i in diff[:5]]
    # the set is adversarial: a naive a * b + c misses a good part of it (else the test tests nothing)
    with np.errstate(all="ignore"):
        naive = a * b + c
    assert (bits(naive) != bits(want)).sum() > 500
    # signed zeros as IEEE 754 has them
    assert math.copysign(1.0, R.fma_fraction(-0.0, 1.0, -0.0)) < 0 and math.copysign(1.0, R.fma_fraction(0.0, 1.0, -0.0)) > 0
    assert math.copysign(1.0, R.fma_fraction(3.0, 2.0, -6.0)) > 0
    assert math.copysign(1.0, float(R.fma(-0.0, 1.0, -0.0))) < 0
    # broadcasting, as update_real and chain_panel call it
    x = np.arange(5.0)
    assert np.array_equal(R.fma(x, 0.1, x), np.array([R.fma_fraction(v, 0.1, v) for v in x]))


# ------------------------------------------------------------------------------------------------------------------------
# chain_panel
# ------------------------------------------------------------------------------------------------------------------------
def panel_problem(seed, n=101, P=64):
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.5, P)
    X = (rng.random((n, P)) < p).astype(np.float64) + (rng.random((n, P)) < p)
    X[::3] = 0.5 * (X[::3] + X[1::3][: X[::3].shape[0]]) / math.sqrt(2.0) + 0.1
    X[:, 7] = 0.37                                           # a constant column: skipped
    # markers in LD, so that a move matters to the next marker
    X[:, 20] = X[:, 19]
    X[5, 20] += 0.5
    beta = np.zeros(P)
    beta[[3, 19, 40, 63]] = [0.8, -0.6, 0.5, 0.7]
    r = X @ beta + rng.normal(size=n)
    g_old = np.zeros(P)
    hot = rng.choice(np.setdiff1d(np.arange(P), [7]), 12, replace=False)
    g_old[hot] = rng.normal(size=12) * 0.1
    return rng, X, r, g_old


def pre_for(rng, model, X, vare):
    """thresholds, 1/v and sd z as k_pre would leave them, from formulas of the right shape and the host's own deviates"""
    P = X.shape[1]
    xx = (X * X).sum(0)
    z = rng.normal(size=P)
    if model in ("BayesCpi", "BayesBpi"):
        vv = xx + vare / 0.05
        thr = (np.abs(rng.normal(size=P)) * 2.0 * np.sqrt(vv * vare)) ** 2
        return thr[None], (1.0 / vv)[None], (np.sqrt(vare / vv) * z)[None]
    if model in ("BayesRR", "BayesA", "BayesL"):
        vv = xx + vare / 0.05
        return np.full((1, P), -np.inf), (1.0 / vv)[None], (np.sqrt(vare / vv) * z)[None]
    K1 = 3 if model == "BayesR4" else 7
    real = 3 if model == "BayesR4" else 5
    thr, iv, sz = np.full((K1, P), np.inf), np.zeros((K1, P)), np.zeros((K1, P))
    t0 = (np.abs(rng.normal(size=P)) * 1.5 * np.sqrt(xx)) ** 2
    for c in range(real):
        vv = xx + vare / (0.05 * 10.0 ** (c - real + 1))
        thr[c] = t0 * (1.0 + 0.6 * c)                        # nested
        iv[c], sz[c] = 1.0 / vv, np.sqrt(vare / vv) * z
    return thr, iv, sz


def plain_chain(X, r, vx, g_old, thr, invv, sdz, model):
    """the sampler as the reference writes it: one marker after the other, x_t . r recomputed from the residual, which every move updates"""
    n, P = X.shape
    Xw, rw = X.astype(WIDE), r.astype(WIDE)
    moves, cls_out = [], np.zeros(P, dtype=np.int64)
    for t in range(P):
        if vx[t] == 0.0:
            continue
        rhs = Xw[:, t] @ rw + (Xw[:, t] @ Xw[:, t]) * WIDE(g_old[t])
        q = rhs * rhs
        if not (g_old[t] != 0.0 or q >= thr[0, t]):
            continue
        cls = int(sum(q >= thr[c, t] for c in range(thr.shape[0])))
        gn = rhs * WIDE(invv[cls - 1, t]) + WIDE(sdz[cls - 1, t]) if cls else WIDE(0.0)   # (nested thresholds: the last one passed is the cls-th)
        if model == "BayesL" and abs(gn) < 1e-6:
            gn = WIDE(1e-6)
        cls_out[t] = cls
        d = gn - WIDE(g_old[t])
        if d != 0:
            moves.append((t, float(d)))
            rw = rw - Xw[:, t] * d
    return moves, cls_out, rw


@pytest.mark.parametrize("model", ["BayesCpi", "BayesBpi", "BayesRR", "BayesA", "BayesL", "BayesR4", "BayesR6"])
def test_chain_panel_against_a_sequential_sampler_on_an_explicit_residual(model):
    rng, X, r, g_old = panel_problem(sum(map(ord, model)))
    n, P = X.shape
    vare = 1.0
    thr, invv, sdz = pre_for(rng, model, X, vare)
    vx = X.var(0, ddof=1)
    vx[7] = 0.0
    if model == "BayesL":                                      # one installed effect that the draw takes inside (-1e-6, 1e-6): marker 0 sees no move before it
        xx0 = float(X[:, 0] @ X[:, 0])
        g_old[0] = (-sdz[0, 0] / invv[0, 0] - float(X[:, 0] @ r)) / xx0
    Xw = X.astype(WIDE)
    G = (Xw.T @ Xw).astype(np.float64)
    dots = (Xw.T @ r.astype(WIDE)).astype(np.float64)
    fold = [0.0, 1e-4, 1e-3, 1e-2, 0.1, 1.0]
    name = "BayesR" if model.startswith("BayesR") and model != "BayesRR" else model
    idx, dl, g_new, cls, sum_w = R.chain_panel(G, np.diag(G).copy(), vx, g_old, dots, thr, invv, sdz, name, fold)
    moves, cls_want, rw = plain_chain(X, r, vx, g_old, thr, invv, sdz, model)
    assert idx.tolist() == [t for t, _ in moves], model
    assert np.array_equal(cls, cls_want), model
    np.testing.assert_allclose(dl, [d for _, d in moves], rtol=1e-12, atol=1e-12)
    assert len(idx) >= 12 and 7 not in idx and g_new[7] == 0.0
    # what the kernel writes back, and its sum
    moved = np.zeros(P, dtype=bool)
    moved[idx] = True
    assert np.array_equal(bits(dl), bits(g_new[idx] - g_old[idx]))   # delta = g_new - g_old, one rounding
    assert not g_new[~moved & (g_old == 0)].any()
    w = g_new[cls > 0] ** 2 / (np.array(fold)[cls[cls > 0]] if name == "BayesR" else 1.0)
    assert abs(sum_w - w.sum()) <= 64 * EPS * w.sum()
    if model == "BayesL":
        assert g_new[0] == 1e-6 and idx[0] == 0
    if model in ("BayesRR", "BayesA", "BayesL"):
        assert len(idx) == P - 1                               # every polymorphic marker moves
    if model == "BayesR6":
        assert set(cls.tolist()) >= {0, 1, 5}
    # the updated residual: update_real on the chain's list against the sampler's own
    r1, u1, r32 = R.update_real(X, r, np.zeros(n), idx, dl)
    np.testing.assert_allclose(r1, rw.astype(np.float64), rtol=0, atol=1e-11)


# ------------------------------------------------------------------------------------------------------------------------
# update_real, stats_real
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 8, 9, 40])
def test_update_real_within_the_dot_product_bound(k):
    """a is a chain of k fused multiply-adds: |a - sum x d| <= k u sum |x d| (u = eps / 2), and r - a, u + a round once more."""
    rng = np.random.default_rng(k)
    n, m = 257, 50
    X = rng.normal(size=(n, m))
    X[3, :] = 1e-310
    r, u = rng.normal(size=n), rng.normal(size=n)
    cols = rng.choice(m, k, replace=False)
    dl = rng.normal(size=k)
    r1, u1, r32 = R.update_real(X, r, u, cols, dl)
    if k == 0:
        assert r1.tobytes() == r.tobytes() and u1.tobytes() == u.tobytes()
    a = X[:, cols].astype(WIDE) @ dl.astype(WIDE)
    absa = np.abs(X[:, cols]) @ np.abs(dl)
    lim = k * EPS * absa
    assert np.all(np.abs(r1 - (r - a).astype(np.float64)) <= lim + EPS * np.abs(r1))
    assert np.all(np.abs(u1 - (u + a).astype(np.float64)) <= lim + EPS * np.abs(u1))
    assert np.array_equal(r32.view(np.uint32), r1.astype(np.float32).view(np.uint32))
    # ... and each step IS the exact fma
    if 0 < k <= 9:
        acc = np.zeros(n)
        for j, d in zip(cols, dl):
            acc = np.array([R.fma_fraction(x, d, v) for x, v in zip(X[:, j], acc)])
        assert np.array_equal(bits(r1), bits(r - acc))


@pytest.mark.parametrize("n", [2, 3, 255, 257])
def test_stats_real_against_numpy(n):
    rng = np.random.default_rng(n)
    X = rng.uniform(0, 2, size=(n, 9))
    X[:, 2] = 0.37
    X[:, 3] = 1.0
    X[:, 4] = 1e6 + rng.normal(0, 1e-3, n)
    X[:, 5] = 0.37
    X[n - 1, 5] = 0.38
    xpx, vx = R.stats_real(X)
    np.testing.assert_allclose(xpx, (X * X).sum(0), rtol=1e-13)
    assert vx[2] == 0.0 and vx[3] == 0.0
    keep = [0, 1, 5, 6, 7, 8]
    np.testing.assert_allclose(vx[keep], X[:, keep].var(0, ddof=1), rtol=1e-12)
    # mean 1e6, spread 1e-3: numpy's two passes in doubles carry the mean's rounding; exact rational arithmetic decides
    col = [Fraction(float(v)) for v in X[:, 4]]
    mean = sum(col) / n
    exact = float(sum((v - mean) ** 2 for v in col) / (n - 1))
    assert abs(vx[4] - exact) <= 1e-13 * exact
