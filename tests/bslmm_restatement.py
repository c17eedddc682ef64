"""numpy restatement of the reference's BSLMM: the loop of src/Bayes.cpp:477-917 for model_index 4 (BayesC / BayesCpi / BSLMM) with the
polygenic block of :518-552, the posterior of :919-1040 with the back-projection of :955-972, and make_grm's arithmetic (src/rm.cpp:5-53)
in the integer form the device evaluates. Test infrastructure: no GPU, no product code.

Draws are addressed Philox draws (hibayes_amd/csrc/hb_rng.hpp): the host stream (purpose 2) through oracle.oracle.Stream, the marker
stream (purpose 1: block marker * 64 + 0 the inclusion uniform, + 1 the effect normal) and the polygenic block's normals (purpose 5:
block j) through the oracle's addressed normal / uniform. The summation order of the three products with K is pluggable (`tdot`:
K'v, `kdot`: K w), which is how the tests measure what the order alone does to a chain.
"""
import ctypes as C

import numpy as np

from oracle import oracle as O

PURPOSE_MARKER, PURPOSE_HOST, PURPOSE_POLY = 1, 2, 5
NOT_PD = "matrix is not positive definite, try to specify parameter 'lambda' with a small value, eg: 0.001 or bigger"


def sub(purpose, it):
    return (purpose << 56) | int(it)


def normal_blk(seed, s, blk):
    return O.lib().hbo_philox_normal(C.c_uint64(seed), C.c_uint64(s), C.c_uint64(blk))


def uniform_blk(seed, s, blk):
    return O.lib().hbo_philox_uniform(C.c_uint64(seed), C.c_uint64(s), C.c_uint64(blk))


def poly_normals(seed, it, n):
    s = sub(PURPOSE_POLY, it)
    return np.array([normal_blk(seed, s, j) for j in range(n)])


def arma_sum(v):
    v = np.asarray(v, dtype=np.float64)
    n = v.size
    h = n // 2
    a1 = float(np.sum(v[0:2 * h:2])) if h else 0.0
    a2 = float(np.sum(v[1:2 * h:2])) if h else 0.0
    if n % 2:
        a1 += float(v[-1])
    return a1 + a2


def var_n1(v):
    v = np.asarray(v, dtype=np.float64)
    n = v.size
    if n < 2:
        return 0.0
    mean = arma_sum(v) / n
    t = mean - v
    return (float(t @ t) - float(t.sum()) ** 2 / n) / (n - 1)


# ---- the orders of summation ----
def tdot_blas(K, v):
    return K.T @ v


def kdot_blas(K, w):
    return K @ w


def tdot_rev(K, v):
    return K[::-1].T @ v[::-1]


def kdot_rev(K, w):
    return K[:, ::-1] @ w[::-1]


ORDERS = {"blas": (tdot_blas, kdot_blas), "rev": (tdot_rev, kdot_rev)}


def poly_block(K, Kval, yadj, u, k_old, vare, vb, z, chis, s2_df, tdot=tdot_blas, kdot=kdot_blas):
    """src/Bayes.cpp:518-552 on arrays of any float dtype (float64, or numpy.longdouble for the kernel tests' reference). Returns the new
    state; raises ValueError with the reference's text when the check of :533 fails."""
    t = tdot(K, yadj + k_old)                                   # :519, :532
    ev = (Kval * vare) / (Kval + vare / vb)                     # :531
    if not np.all(ev >= -1e-06 * np.max(np.abs(ev))):           # :533
        raise ValueError(NOT_PD)
    w = (ev / vare) * t + np.sqrt(np.maximum(ev, 0)) * z        # :532, :534-535 (the two products as one)
    k_new = kdot(K, w)
    d = k_old - k_new                                           # :537-538
    Kg = tdot(K, k_new)                                         # :543
    q = (Kg * Kg / Kval).sum()                                  # :544
    return {"t": t, "eval": ev, "w": w, "k": k_new, "yadj": yadj + d, "u": u - d, "Kg": Kg, "q": q, "vb": (q + s2_df) / chis}


def bslmm(y, X, Pi, niter, nburn, thin, seed, Kival=None, Ki=None, Cmat=None, R=None, order="blas", fixpi=False):
    """Bayes(y, X, "BayesCpi" | "BSLMM", Pi, Kival, Ki, C, R, niter, nburn, thin) of the reference with its defaults."""
    tdot, kdot = ORDERS[order]
    y = np.asarray(y, dtype=np.float64)
    Xf = np.asfortranarray(X, dtype=np.float64)
    n, m = Xf.shape
    Pi = np.array(Pi, dtype=np.float64)
    nk = 0 if Ki is None else n
    if nk:
        K = np.asarray(Ki, dtype=np.float64)
        Kval = np.asarray(Kival, dtype=np.float64)
    # covariates and random effects (:126-201)
    Cm = np.zeros((n, 0)) if Cmat is None else np.asarray(Cmat, dtype=np.float64).reshape(n, -1, order="F")
    nc = Cm.shape[1]
    cpc = np.array([float(Cm[:, i] @ Cm[:, i]) for i in range(nc)])
    Rm = np.zeros((n, 0), dtype=object) if R is None else np.asarray(R, dtype=object).reshape(n, -1)
    nr = Rm.shape[1]
    zid, zz, estR = [], [], []
    for t in range(nr):
        lev = sorted(set(str(v) for v in Rm[:, t]))
        ix = {l: q for q, l in enumerate(lev)}
        zi = np.array([ix[str(v)] for v in Rm[:, t]])
        zid.append(zi)
        zz.append(np.bincount(zi, minlength=len(lev)).astype(np.float64))
        estR.append(np.zeros(len(lev)))
    # marker statistics and prior defaults (:310-374)
    xpx = np.array([float(Xf[:, j] @ Xf[:, j]) for j in range(m)])
    vx = np.array([var_n1(Xf[:, j]) for j in range(m)])
    sumvx = arma_sum(vx)
    nvar0 = int(np.sum(vx == 0))
    vary = var_n1(y)
    h2, dfvara, dfvare, s2vare, dfr, s2r = 0.5, 4.0, -2.0, 0.0, -1.0, 0.0
    vara = ((dfvara - 2) / dfvara) * vary * h2
    vare = vary * (1 - h2) / (nr + 1)
    s2vara = vara * (dfvara - 2) / dfvara
    varg = vara / ((1 - Pi[0]) * sumvx)
    s2varg = s2vara / ((1 - Pi[0]) * sumvx)
    vrtmp = np.full(nr, vary * (1 - h2) / (nr + 1))
    vr = np.zeros(nr)
    vbtmp = vara                                                # :333
    va = vb = 0.0
    # chain state (:469-472)
    mu = arma_sum(y) / n
    yadj = y - mu
    u = np.zeros(n)
    g = np.zeros(m)
    beta = np.zeros(nc)
    k_est = np.zeros(n)
    nrec = max((niter - nburn) // thin, 0)
    st = {k: np.zeros(nrec) for k in ("mu", "Vg", "Ve", "h2", "Va", "Vb")}
    s_alpha, s_pi, s_beta = np.zeros((m, nrec)), np.zeros((2, nrec)), np.zeros((nc, nrec))
    s_Vr = np.zeros((nr, nrec))
    s_r = [np.zeros((len(e), nrec)) for e in estR]
    k_store = np.zeros(n)
    traj = {"k": [], "vb": []}
    count = 0
    poly = [j for j in range(m) if vx[j] != 0]
    for it in range(niter):
        hs = O.Stream(O.RNG_PHILOX, seed, sub(PURPOSE_HOST, it), 0)
        msub = sub(PURPOSE_MARKER, it)
        mu_ = -(arma_sum(yadj) / n + np.sqrt(vare / n) * hs.norm())     # :479-482
        mu -= mu_
        yadj = yadj + mu_
        for i in range(nc):                                             # :484-494
            ci = Cm[:, i]
            rhs = float(ci @ yadj) + cpc[i] * beta[i]
            gi = rhs / cpc[i] + np.sqrt(vare / cpc[i]) * hs.norm()
            yadj = yadj + (beta[i] - gi) * ci
            beta[i] = gi
        for t in range(nr):                                             # :496-516
            rr = np.bincount(zid[t], weights=yadj, minlength=len(zz[t])) + zz[t] * estR[t]
            lhs = zz[t] + vare / vrtmp[t]
            new = np.array([rr[q] / lhs[q] + np.sqrt(vare / lhs[q]) * hs.norm() for q in range(len(lhs))])
            yadj = yadj + (estR[t] - new)[zid[t]]
            vrtmp[t] = (float(new @ new) + s2r * dfr) / hs.chisq(len(new) + dfr)
            vr[t] = var_n1(new)
            estR[t] = new
        if nk:                                                          # :518-552
            z = poly_normals(seed, it, n)
            chis = hs.chisq(dfvara + nk)
            pb = poly_block(K, Kval, yadj, u, k_est, vare, vbtmp, z, chis, s2vara * dfvara, tdot, kdot)
            yadj, u, k_est, vbtmp = pb["yadj"], pb["u"], pb["k"], pb["vb"]
            vb = vbtmp
            traj["k"].append(k_est.copy())
            traj["vb"].append(vb)
        # BayesC / BayesCpi sweep (:671-717)
        logpi = np.log(Pi)
        vargi = 0.0
        nnz = 0
        for i in poly:
            x = Xf[:, i]
            xx = xpx[i]
            old = g[i]
            rhs = float(x @ yadj)
            if old:
                rhs += xx * old
            logdetV = np.log(varg * (xx / vare) + 1)
            uhat = rhs / (xx + vare / varg)
            s1 = -0.5 * (logdetV - (rhs * uhat / vare)) + logpi[1]
            accept = 1 / (1.0 + np.exp(s1 - logpi[0]))
            if uniform_blk(seed, msub, i * 64 + 0) < accept:
                gi = 0.0
                if old:
                    yadj = yadj + old * x
                    u = u - old * x
            else:
                v = xx + vare / varg
                gi = rhs / v + np.sqrt(vare / v) * normal_blk(seed, msub, i * 64 + 1)
                yadj = yadj + (old - gi) * x
                u = u - (old - gi) * x
                vargi += gi * gi
                nnz += 1
            g[i] = gi
        varg = (vargi + s2varg * dfvara) / hs.chisq(dfvara + nnz)       # :713
        if nk:
            va = varg                                                   # :715
        if not fixpi:                                                   # :716, src/stats.cpp:69-76
            xn = np.array([hs.gamma(m - nvar0 - nnz + 1, 1.0), hs.gamma(nnz + 1, 1.0)])
            Pi = xn / arma_sum(xn)
        vara = var_n1(u)                                                # :819
        vare = (float(yadj @ yadj) + s2vare * dfvare) / hs.chisq(n + dfvare)   # :823
        if it >= nburn and (it + 1 - nburn) % thin == 0 and count < nrec:       # :848-882
            st["mu"][count], st["Vg"][count], st["Ve"][count] = mu, vara, vare
            s_pi[:, count] = Pi
            if nk:
                st["Va"][count], st["Vb"][count] = va, vb
                k_store += k_est
            s_alpha[:, count] = g
            s_beta[:, count] = beta
            s_Vr[:, count] = vr
            for t in range(nr):
                s_r[t][:, count] = estR[t]
            st["h2"][count] = vara / (vara + vare + vr.sum())
            count += 1
    # posterior (:919-1040)
    res = {"Vg": st["Vg"].mean(), "Ve": st["Ve"].mean(), "h2": st["h2"].mean(), "mu": st["mu"].mean(), "pi": s_pi.mean(axis=1),
           "s_Vg": st["Vg"], "s_Ve": st["Ve"], "s_mu": st["mu"], "s_h2": st["h2"], "s_pi": s_pi, "s_beta": s_beta, "s_Vr": s_Vr,
           "g": u.copy(), "traj": traj, "sumvx": sumvx}
    e = y - res["mu"]
    if nc:
        res["beta"] = s_beta.mean(axis=1)
        e = e - Cm @ res["beta"]
    if nk:                                                              # :955-969
        k_mean = k_store / count
        Kg = tdot(K, k_mean) / Kval / sumvx
        ghat = Xf.T @ kdot(K, Kg)
        ghat = ghat - arma_sum(ghat) / m
        s_alpha = s_alpha + ghat[:, None]
        res.update(k=k_mean, ghat=ghat, Va=st["Va"].mean(), Vb=st["Vb"].mean(), s_Va=st["Va"], s_Vb=st["Vb"])
    res["s_alpha"] = s_alpha
    res["alpha"] = s_alpha.mean(axis=1)
    e = e - Xf @ res["alpha"]                                           # :971
    for t in range(nr):
        e = e - s_r[t].mean(axis=1)[zid[t]]
    if nr:
        res["Vr"] = s_Vr.mean(axis=1)
    res["e"] = e
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# make_grm (src/rm.cpp:5-53) in the integer form of hb_grm_build
# ---------------------------------------------------------------------------------------------------------------------------------
EPS = float(np.finfo(np.float64).eps)


def grm_integers(M):
    """S = M M', a_i = sum_k c_k M_ik (int64 arrays) and C = sum_k c_k^2 (a Python integer), c the column sums: all exact."""
    M64 = np.asarray(M).astype(np.int64)
    c = M64.sum(axis=0)
    return M64 @ M64.T, M64 @ c, sum(int(v) ** 2 for v in c)


def grm_expression(M):
    """The fixed fp64 expression: raw_ij = (S_ij - (a_i + a_j) / n) + C / n^2 with every conversion and operation rounded to nearest."""
    S, a, Cc = grm_integers(M)
    n = S.shape[0]
    cn2 = float(Cc) / (float(n) * float(n))
    return (S.astype(np.float64) - (a[:, None] + a[None, :]).astype(np.float64) / float(n)) + cn2


def grm_raw_error(M, raw):
    """(err, bound): the exact |raw_ij - value_ij| of an n x n float matrix against the rational n^2 value = n^2 S - n (a_i + a_j) + C,
    as floats rounded up a hair, and the stated bound 4 eps (|S_ij| + |a_i + a_j| / n + C / n^2)."""
    S, a, Cc = grm_integers(M)
    n = S.shape[0]
    err, bound = np.zeros((n, n)), np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            N = n * n * int(S[i, j]) - n * (int(a[i]) + int(a[j])) + Cc
            p, q = float(raw[i, j]).as_integer_ratio()
            err[i, j] = abs(p * n * n - N * q) / (q * n * n)
            bound[i, j] = 4 * EPS * (abs(int(S[i, j])) + abs(int(a[i]) + int(a[j])) / n + Cc / (n * n))
    return err, bound


def grm_scaled_bound(M, lambda_=0.0):
    """(G, bound): G_ij = raw_ij / mean(diag raw) (+ lambda on the diagonal) in numpy.longdouble from the exact integers, and the bound on
    the device's fp64 entry that follows from the stated one: with T_ij = |S_ij| + |a_i + a_j| / n + C / n^2 every raw entry is off by at
    most 4 eps T_ij, so the mean of the diagonal — n such entries (all >= 0) added in some order and divided — by at most
    Em = 4 eps mean(T_ii) + (n + 1) eps mean(raw_ii); the quotient and the added lambda round once more each."""
    S, a, Cc = grm_integers(M)
    n = S.shape[0]
    ld = np.longdouble
    rawx = (S.astype(ld) - (a[:, None] + a[None, :]).astype(ld) / ld(n)) + ld(Cc) / (ld(n) * ld(n))
    T = np.abs(S).astype(np.float64) + np.abs(a[:, None] + a[None, :]) / n + Cc / (n * n)
    mean = float(np.trace(rawx) / n)
    Em = 4 * EPS * float(np.trace(T)) / n + (n + 1) * EPS * mean
    G = rawx / ld(mean)
    bound = 1.01 * (4 * EPS * T + np.abs(rawx).astype(np.float64) * Em / mean) / mean + EPS * np.abs(G).astype(np.float64)
    G = G + ld(lambda_) * np.eye(n, dtype=ld)
    bound = bound + EPS * np.abs(np.diag(np.diag(G))).astype(np.float64)
    return G, bound
