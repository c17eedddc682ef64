"""Level 0 for the floating-point kernels that run once per sweep: k_pre, k_bayesl_post, k_reduce_ru and k_sum_vec alone,
each against the reference's own formula evaluated in higher precision — np.longdouble (64-bit mantissa) where whole arrays are
evaluated, mpmath at 50 digits where a formula cancels, exact sums (mpmath.fsum) for the reductions. No chain is compared: every test
reads one product of the sweep boundary and says which one is off, and by how many eps.

The references are src/Bayes.cpp:595 / :617 / :640-648 / :683-691 / :726 / :759-784 (the conditionals as the reference writes them:
class scores s_j, then probabilities) and src/stats.cpp:55-67, never the kernels' restated algebra (closed-form threshold, Newton
search on a log-sum-exp with shortcuts). Deviates come from the oracle's Philox layer at the addresses of hb_rng.hpp:
sub = (1 << 56) | iter, blk = (m_offset + j) * 64 + b.

The constants C_* below are 4 x the largest figure measured on an MI355X with the seeds named here (DESIGN.md §7 has the table; every
test prints its figures before it asserts), under the caps the tests were written for: 16 eps S for a threshold, 8 ulp for 1/v and
sd z, 16 eps kappa for the inverse Gaussian."""
import functools
import math

import mpmath
import numpy as np
import pytest

import hibayes_amd as H
from oracle import oracle as O

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
SEED = 20240901
N = 300
INF = float("inf")

# 4 x measured on the MI355X, capped at 16 / 8 / 8 / 16. Measured: thresholds B 1.69, C 0.71, R 1.52 eps S; 1/v RR 0.62, A 7.97, B 6.47, C 0.64,
# L 1.74, R 1.70 ulp; sd z RR 2.95, A 3.56, B 4.97, C 3.16, L 3.22, R 3.94 ulp (so every sd z and A / B's 1/v stand at the cap: the device's
# Box-Muller normal is a few ulp from the oracle's, and A / B's chi-square cubes it); inverse Gaussian 1.28 eps kappa.
C_THR = {"BayesB": 6.8, "BayesC": 2.9, "BayesR": 6.1}             # threshold residual, in eps * S
C_INVV = {"BayesRR": 2.5, "BayesA": 8.0, "BayesB": 8.0, "BayesC": 2.6, "BayesL": 7.0, "BayesR": 6.8}   # ulp of 1/v
C_SDZ = {"BayesRR": 8.0, "BayesA": 8.0, "BayesB": 8.0, "BayesC": 8.0, "BayesL": 8.0, "BayesR": 8.0}    # ulp of sd z
C_IG = 5.2                                                        # inverse Gaussian, in eps * kappa_j
assert max(C_THR.values()) <= 16 and max(C_INVV.values()) <= 8 and max(C_SDZ.values()) <= 8 and C_IG <= 16


def test_the_high_precision_type_is_wide_enough():
    assert np.finfo(LD).eps < 2e-19
    mpmath.mp.dps = 50
    assert mpmath.mpf(1) + mpmath.mpf(2) ** -160 != 1


# ------------------------------------------------------------------------------------------------------------------------
# shared inputs
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def geno(n, m):
    """codes 0/1/2 with allele frequencies from 0.002 to 0.998; column 0 a single 1 (xpx = 1), column 1 all 2 but one 1 (xpx = 4 n - 3),
    columns 2 and 3 monomorphic (all 2: xpx = 4 n; all 0)."""
    rng = np.random.default_rng(1000 + m)
    p = np.geomspace(0.002, 0.5, m)
    p[1::2] = 1.0 - p[1::2]
    X = rng.binomial(2, p, size=(n, m)).astype(np.int8)
    X[:, 0] = 0
    X[17, 0] = 1
    X[:, 1] = 2
    X[n - 1, 1] = 1
    X[:, 2] = 2
    X[:, 3] = 0
    X = np.asfortranarray(X)
    X.setflags(write=False)
    return X


def marker_sub(it):
    return (1 << 56) | it


def deviates(it, m_offset, m, b, normal):
    f = O.lib().hbo_philox_normal if normal else O.lib().hbo_philox_uniform
    sub = marker_sub(it)
    return np.array([f(SEED, sub, (m_offset + j) * 64 + b) for j in range(m)])


def ulps(got, ref):
    """|got - ref| in units of the double spacing at ref (ref: longdouble)"""
    sp = np.spacing(np.abs(ref).astype(np.float64)).astype(LD)
    return (np.abs(got.astype(LD) - ref) / sp).astype(np.float64)


def lse(s):
    """log-sum-exp down the rows of a (k, m) longdouble array; -inf where every term is -inf"""
    mx = s.max(axis=0)
    fin = np.isfinite(mx)
    safe = np.where(fin, mx, LD(0))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return np.where(fin, safe + np.log(np.exp(s - safe).sum(axis=0)), mx)


def bits(*arrays):
    return [np.ascontiguousarray(a).view(np.uint64).copy() for a in arrays]


# ------------------------------------------------------------------------------------------------------------------------
# 1. k_pre
# ------------------------------------------------------------------------------------------------------------------------
TYP_PI, TYP_FOLD = [0.95, 0.02, 0.02, 0.01], [0.0, 1e-4, 1e-3, 1e-2]


def _r(pi, fold, vare=1.0, varg=0.5):
    with np.errstate(divide="ignore"):
        return dict(model="BayesR", vare=vare, varg=varg, logpi=[float(v) for v in np.log(np.asarray(pi, dtype=np.float64))], fold=list(fold))


PRE_CASES = {
    "RR": dict(model="BayesRR", vare=1.0, varg=0.01),
    "A": dict(model="BayesA", vare=1.0, s2varg_df=0.05, dfvara=4.0),
    "L": dict(model="BayesL", vare=1.0, lam=1.5, lam2=2.25),
    "L-vare1e2": dict(model="BayesL", vare=1e2, lam=1.5, lam2=2.25),
    "B": dict(model="BayesB", vare=1.0, s2varg_df=0.05, dfvara=4.0, logpi=[math.log(0.95), math.log(0.05)]),
    "B-vare1e-2": dict(model="BayesB", vare=1e-2, s2varg_df=0.05, dfvara=4.0, logpi=[math.log(0.95), math.log(0.05)]),
    "C": dict(model="BayesC", vare=1.0, varg=0.01, logpi=[math.log(0.95), math.log(0.05)]),
    "C-vare1e-2": dict(model="BayesC", vare=1e-2, varg=0.01, logpi=[math.log(0.95), math.log(0.05)]),
    "C-vare1e2": dict(model="BayesC", vare=1e2, varg=0.01, logpi=[math.log(0.95), math.log(0.05)]),
    "C-pi1-zero": dict(model="BayesC", vare=1.0, varg=0.01, logpi=[0.0, -INF]),
    "C-pi0-zero": dict(model="BayesC", vare=1.0, varg=0.01, logpi=[-INF, 0.0]),
    "R-K2": _r([0.95, 0.05], [0.0, 1e-2]),
    "R-K3": _r([0.9, 0.07, 0.03], [0.0, 1e-3, 1e-2]),
    "R-K4": _r(TYP_PI, TYP_FOLD),
    "R-K5": _r([0.9, 0.04, 0.03, 0.02, 0.01], [0.0, 1e-5, 1e-4, 1e-3, 1e-2]),
    "R-K8": _r([0.86, 0.02, 0.02, 0.02, 0.02, 0.02, 0.02, 0.02], [0.0, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1.0]),
    "R-vare1e-2": _r(TYP_PI, TYP_FOLD, vare=1e-2),
    "R-vare1e2": _r(TYP_PI, TYP_FOLD, vare=1e2),
    "R-pi-zero-middle": _r([0.95, 0.0, 0.03, 0.02], TYP_FOLD),
    "R-pi-zero-end": _r([0.95, 0.03, 0.02, 0.0], TYP_FOLD),
    "R-pi-zero-class0": _r([0.0, 0.5, 0.3, 0.2], TYP_FOLD),
    "R-fold1e-8": _r(TYP_PI, [0.0, 1e-8, 1e-6, 1e-4]),
    "R-fold-near-equal": _r([0.9, 0.05, 0.05], [0.0, 1e-3, 1.0000001e-3]),
    "R-K8-fold-near-equal": _r([0.86, 0.02, 0.02, 0.02, 0.02, 0.02, 0.02, 0.02], [0.0, 1e-8, 1e-6, 1e-4, 1e-3, 1.0000001e-3, 1e-2, 1e-1]),
}
ADDRESSES = [(0, 0), (7, 0), (0, 1000000), (7, 1000000)]   # (iter, m_offset), dealt round the cases


def pre_state(m):
    rng = np.random.default_rng(77)
    g = np.zeros(m)
    g[0::2] = rng.choice([-1.0, 1.0], size=g[0::2].size) * 10.0 ** rng.uniform(-4, 0, size=g[0::2].size)
    vargL = rng.permutation(np.geomspace(1e-8, 1e2, m))
    return g, vargL


def run_pre(case, it, m_offset, m, g, vargL, pipeline):
    """one sweep, then what k_pre left: (thr, invv, sdz, xpx, vx)"""
    X = geno(N, m)
    kw = {k: v for k, v in case.items() if k not in ("model", "vare")}
    if case["model"] == "BayesR":
        kw["vara_fold"] = [case["varg"] * f for f in case["fold"]]
    with H.Context(N, m, panel=64, precise=2, m_offset=m_offset, seed=SEED) as c:
        c.upload(X)
        xpx, vx, _, _ = c.marker_stats()
        c.set_pipeline(*pipeline)
        c.set_residual(np.zeros(N), np.zeros(N))          # (little for the chain to do: only k_pre's products are read)
        c.set_effects(g, (g != 0).astype(np.uint8), vargL)
        c.sweep(case["model"], it, case["vare"], **kw)
        thr, invv, sdz = c.pre()
    return thr, invv, sdz, xpx, vx


@pytest.mark.parametrize("name", list(PRE_CASES))
def test_k_pre_against_the_reference_conditionals(name):
    """thr, 1/v and sd z of one sweep, every marker and every row. At the device's own threshold q the reference's class probabilities
    (evaluated in longdouble from s_j of :643 / :686 / :762) must put P(class > c | q) at 1 - U: |logit P - log((1-U)/U)| <= C eps S with
    S = 1 + |logT| + max |a_i| + max b_i |q|, the sizes of the terms that are added (a_i the score at q = 0, b_i its slope). So an error in
    the Newton search, in the log-sum-exp shortcuts or in the closed form shows as a residual; no root is searched here."""
    case = PRE_CASES[name]
    model = case["model"]
    it, m_offset = ADDRESSES[list(PRE_CASES).index(name) % 4]
    m = 1024 + 37 if model == "BayesR" else 4096 + 37
    g, vargL = pre_state(m)
    thr, invv, sdz, xpx, vx = run_pre(case, it, m_offset, m, g, vargL, (1, 2, 2))
    thr0, invv0, sdz0, _, _ = run_pre(case, it, m_offset, m, g, vargL, (0, 0, 1))
    for a, b in zip(bits(thr, invv, sdz), bits(thr0, invv0, sdz0)):       # the two launch sites of k_pre
        assert np.array_equal(a, b)

    X = geno(N, m).astype(np.int64)
    assert np.array_equal(xpx, (X * X).sum(0)) and np.array_equal(vx == 0, (X == X[0]).all(0))
    act = vx != 0
    assert act[0] and act[1] and not act[2] and not act[3] and xpx[0] == 1 and xpx[1] == 4 * N - 3
    K = len(case["logpi"]) if model == "BayesR" else 2
    kp = 1 if model != "BayesR" or K == 2 else (3 if K <= 4 else 7)
    m_pad = -(-m // 64) * 64
    assert thr.shape == invv.shape == sdz.shape == (kp, m_pad)
    nrow = K - 1 if model == "BayesR" else 1
    idle = np.ones((kp, m_pad), dtype=bool)                               # pad columns, monomorphic markers, unused rows
    idle[:nrow, :m] = ~act
    assert (thr[idle] == INF).all() and not invv[idle].any() and not sdz[idle].any()
    assert np.isfinite(invv[:nrow, :m][:, act]).all() and np.isfinite(sdz[:nrow, :m][:, act]).all() and not np.isnan(thr).any()

    vare, xx = LD(case["vare"]), xpx.astype(LD)
    z = deviates(it, m_offset, m, 1, True).astype(LD)
    sub = marker_sub(it)
    # vf[c]: the variance of class c's effects — the shared one, BayesA / BayesB's own draw (:613 / :636), or varg * fold (:749)
    if model in ("BayesA", "BayesB"):
        chi = np.array([O.Stream(O.RNG_PHILOX, SEED, sub, (m_offset + j) * 64 + 4).chisq(case["dfvara"] + 1.0) for j in range(m)])
        vf = [None, (g.astype(LD) ** 2 + LD(case["s2varg_df"])) / chi.astype(LD)]
    elif model == "BayesR":
        vf = [None] + [LD(case["varg"] * f) * np.ones(m, dtype=LD) for f in case["fold"][1:]]
    else:
        vf = [None, LD(case.get("varg", 0.0)) * np.ones(m, dtype=LD)]
    worst_v = worst_s = 0.0
    for c in range(1, nrow + 1):
        vv = xx + 1 / vargL.astype(LD) if model == "BayesL" else xx + vare / vf[c]          # :595 :617 :648 :691 :726 :761
        e1 = ulps(invv[c - 1, :m], 1 / vv)[act].max()
        e2 = ulps(sdz[c - 1, :m], np.sqrt(vare / vv) * z)[act].max()
        worst_v, worst_s = max(worst_v, e1), max(worst_s, e2)
    print("k_pre %-22s 1/v %.2f ulp, sd z %.2f ulp" % (name, worst_v, worst_s))
    assert worst_v <= C_INVV[model] and worst_s <= C_SDZ[model]

    if model not in C_THR:
        assert (thr[0, :m][act] == -INF).all()         # RR / A / L: every polymorphic marker is sampled
        return
    U = deviates(it, m_offset, m, 0, False).astype(LD)
    logT = np.log((1 - U) / U)
    logpi = np.array(case["logpi"], dtype=LD)
    a = np.empty((K, m), dtype=LD)
    b = np.zeros((K, m), dtype=LD)
    a[0] = logpi[0]
    with np.errstate(divide="ignore"):
        for c in range(1, K):
            a[c] = -0.5 * np.log(vf[c] * (xx / vare) + 1) + logpi[c]           # s_c at rhs = 0 (:641-643, :760-762)
            b[c] = 0.5 / ((xx + vare / vf[c]) * vare)                          # rhs * uhat / vare = rhs^2 / ((xx + vare / vf) vare)
    amax = np.where(np.isfinite(a), np.abs(a), 0).max(axis=0)
    Ctol = C_THR[model] * EPS
    worst = 0.0
    for c in range(K - 1):
        t = thr[c, :m]

        def residual(q):
            with np.errstate(invalid="ignore"):
                h = lse(a[c + 1:] + b[c + 1:] * q) - lse(a[:c + 1] + b[:c + 1] * q) - logT
            return h, 1 + np.abs(logT) + amax + (b * np.abs(q)).max(axis=0)

        h0, S0 = residual(np.zeros(m, dtype=LD))
        fin = act & np.isfinite(t) & ((t != 0) if model == "BayesR" else np.ones(m, dtype=bool))
        hq, Sq = residual(np.where(fin, t, 0).astype(LD))
        ratio = np.where(fin, np.abs(hq) / (EPS * Sq), 0).astype(np.float64)
        worst = max(worst, ratio.max())
        assert (ratio <= C_THR[model]).all(), (name, c, int(ratio.argmax()), ratio.max())
        if model == "BayesR":
            assert (t[act] >= 0).all()
            if c:
                assert (t[act] >= thr[c - 1, :m][act]).all()                   # nested boundaries
        low = act & (t <= 0)                            # "included whatever rhs is": only where the reference says so at q = 0
        assert (h0[low] >= -Ctol * S0[low]).all(), (name, c)
        # never crossed: only where the reference's P(class > c | q) is 0 for every q, i.e. every class above c has pi = 0
        never = bool(np.isneginf(logpi[c + 1:]).all())
        assert ((t[act] == INF) == never).all(), (name, c)
        seen = fin | low | (t == INF)
        assert seen[act].all()                          # no marker is left out
    print("k_pre %-22s threshold residual %.2f eps S" % (name, worst))


# ------------------------------------------------------------------------------------------------------------------------
# 2. k_bayesl_post
# ------------------------------------------------------------------------------------------------------------------------
def test_bayesl_post_against_the_inverse_gaussian_formula():
    """vargL_j = 1 / InvGauss(sqrt(vare) lambda / |g_j|, lambda^2) (:729, stats.cpp:55-67) from the device's own g_j after one sweep: against
    the oracle's stream in double and against the same formula at 50 digits on the same deviates. The root
    x = mu + mu^2 y / 2L - (mu / 2L) sqrt(4 mu L y + mu^2 y^2) cancels, so the bound per marker is C eps kappa_j with
    kappa_j = (|mu| + |mu^2 y / 2L| + |(mu / 2L) sqrt(...)|) / |x|, the condition number of that sum, from the 50-digit evaluation. (The
    oracle's double is allowed the same error, hence 2 C between the two doubles.) No marker lies within 1e-12 of the branch
    u <= mu / (mu + x) at this seed, so none is excused."""
    m, it, m_offset = 4096 + 37, 3, 1000000
    vare, lam, lam2 = 1.3, 1.5, 2.25
    X = geno(N, m)
    rng = np.random.default_rng(5)
    g0 = rng.choice([-1.0, 1.0], size=m) * 10.0 ** rng.uniform(-7, 1, size=m)
    v0 = rng.permutation(np.geomspace(1e-8, 1e2, m))
    with H.Context(N, m, panel=64, precise=2, m_offset=m_offset, seed=SEED) as c:
        c.upload(X)
        _, vx, _, _ = c.marker_stats()
        c.set_residual(rng.normal(size=N), np.zeros(N))
        c.set_effects(g0, np.ones(m, dtype=np.uint8), v0)
        c.sweep("BayesL", it, vare, lam=lam, lam2=lam2)
        g, _, v = c.get_effects()
    act = vx != 0
    assert np.array_equal(v[~act], v0[~act]) and not act[2] and not act[3]
    assert np.abs(g[act]).min() > 0 and np.log10(np.abs(g[act]).max() / np.abs(g[act]).min()) > 3     # mu over decades
    sub = marker_sub(it)
    L = O.lib()
    mpmath.mp.dps = 50
    mpf = mpmath.mpf
    worst = worst_o = kmax = 0.0
    near = 0
    for j in np.flatnonzero(act):
        blk = (m_offset + int(j)) * 64 + 2
        mu_d = math.sqrt(vare) * lam / abs(g[j])
        want_d = 1.0 / O.Stream(O.RNG_PHILOX, SEED, sub, blk).invgauss(mu_d, lam2)
        zz, u = mpf(L.hbo_philox_normal(SEED, sub, blk)), mpf(L.hbo_philox_uniform(SEED, sub, blk + 1))
        mu, lm = mpmath.sqrt(mpf(vare)) * mpf(lam) / abs(mpf(float(g[j]))), mpf(lam2)
        y = zz * zz
        t1, t2 = mu * mu * y / (2 * lm), (mu / (2 * lm)) * mpmath.sqrt(4 * mu * lm * y + mu * mu * y * y)
        x = mu + t1 - t2
        kappa = float((mu + t1 + t2) / x)
        margin = abs(u - mu / (mu + x))
        near += margin < mpf("1e-12")
        want = 1 / (x if u <= mu / (mu + x) else mu * mu / x)
        e = float(abs(mpf(float(v[j])) - want) / want) / (EPS * kappa)
        eo = abs(float(v[j]) - want_d) / abs(want_d) / (EPS * kappa)
        worst, worst_o, kmax = max(worst, e), max(worst_o, eo), max(kmax, kappa)
        assert e <= C_IG and eo <= 2 * C_IG, (int(j), float(g[j]), float(v[j]), float(want), want_d, kappa)
    print("k_bayesl_post: %.2f eps kappa against 50 digits, %.2f against the oracle's double; largest kappa %.3g" % (worst, worst_o, kmax))
    assert near == 0


# ------------------------------------------------------------------------------------------------------------------------
# 3. end-of-sweep reductions
# ------------------------------------------------------------------------------------------------------------------------
def exact_sums(r, u):
    mpmath.mp.dps = 50
    n = len(r)
    sr, sr2, su = mpmath.fsum(r.tolist()), mpmath.fsum(r.tolist(), squared=True), mpmath.fsum(u.tolist())
    mean = su / n
    ss = mpmath.fsum([(mpmath.mpf(x) - mean) ** 2 for x in u.tolist()])       # two-pass, as arma::var (:819)
    return sr, sr2, ss / (n - 1), float(np.abs(r).sum()), float((r * r).sum())


@pytest.mark.parametrize("n", [2, 63, 64, 65, 1023, 1024, 1025, 28671, 28672, 28673, 57343, 57344, 57345])
def test_reduce_ru_at_the_loop_edges(n):
    """k_reduce_ru's passes step by 28 * 1024 and 56 * 1024 elements; sixteen waves of 64 lanes. A BayesC sweep with pi_1 = 0 moves
    nothing, so hb_sweep_out's sums are pure reductions of what set_residual installed: r = 1e3 + N(0, 1), u likewise, the last element
    the largest. Bound from the kernel's shape — ceil(n / 1024) serial adds per lane, six shuffle levels, sixteen wave sums:
    (ceil(n / 1024) + 22) eps sum |term|; var(u) by the same factor relative to the two-pass value. A second sweep on the same context
    gives the same bits (the tickets in ru_ws were reset)."""
    rng = np.random.default_rng(n)
    X = np.asfortranarray(rng.integers(0, 3, size=(n, 64)).astype(np.int8))
    r, u = 1e3 + rng.normal(size=n), 1e3 + rng.normal(size=n)
    r[n - 1], u[n - 1] = 1007.5, 1009.25
    assert np.abs(r).argmax() == n - 1 and np.abs(u).argmax() == n - 1
    with H.Context(n, 64, panel=64, precise=2, seed=SEED) as c:
        c.upload(X)
        c.marker_stats()
        c.set_residual(r, u)
        kw = dict(vare=1.0, varg=0.01, logpi=[0.0, -INF])
        s1 = c.sweep("BayesC", 0, **kw)
        a1 = c.residual_sums()
        s2 = c.sweep("BayesC", 0, **kw)
        a2 = c.residual_sums()
        r1, u1 = c.get_residual()
    assert s1["n_events"] == 0 and np.array_equal(r1, r) and np.array_equal(u1, u)
    for k in ("sum_r", "sum_r2", "var_u"):
        assert np.float64(s1[k]).view(np.uint64) == np.float64(s2[k]).view(np.uint64), k
    assert a1 == a2 == (s1["sum_r"], s1["sum_r2"])
    sr, sr2, var, abs_r, abs_r2 = exact_sums(r, u)
    f = (-(-n // 1024) + 22) * EPS
    e = [float(abs(mpmath.mpf(s1["sum_r"]) - sr)) / (f * abs_r), float(abs(mpmath.mpf(s1["sum_r2"]) - sr2)) / (f * abs_r2),
         float(abs(mpmath.mpf(s1["var_u"]) - var) / var) / f]
    print("k_reduce_ru n = %5d: sum r %.3f, sum r^2 %.3f, var u %.3f of the bound" % (n, e[0], e[1], e[2]))
    assert max(e) <= 1.0, e


@pytest.mark.parametrize("m", [64, 1023, 1025, 4133])
def test_sum_vargl_at_the_block_edges(m):
    """k_sum_vec (one workgroup of 1024) behind hb_sweep_out.sum_vargL: against the exact sum of the vargL the same sweep left, same bound."""
    X = geno(N, 4133)[:, :m]
    rng = np.random.default_rng(m)
    with H.Context(N, m, panel=64, precise=2, seed=SEED) as c:
        c.upload(X)
        c.marker_stats()
        c.set_residual(rng.normal(size=N), np.zeros(N))
        c.set_effects(np.zeros(m), np.zeros(m, dtype=np.uint8), rng.permutation(np.geomspace(1e-6, 1e2, m)))
        s = c.sweep("BayesL", 1, 1.0, lam=1.5, lam2=2.25)
        _, _, v = c.get_effects()
    mpmath.mp.dps = 50
    e = float(abs(mpmath.mpf(s["sum_vargL"]) - mpmath.fsum(v.tolist()))) / ((-(-m // 1024) + 22) * EPS * float(np.abs(v).sum()))
    print("k_sum_vec m = %4d: %.3f of the bound" % (m, e))
    assert (v > 0).all() and e <= 1.0
