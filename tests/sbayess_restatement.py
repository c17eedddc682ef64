"""A Python restatement of the reference's summary-level sampler on a SPARSE LD matrix, SBayesS() (src/SBayesS.cpp:109-141 set-up
and varediff, :277-600 the MCMC loop), on a scipy CSC matrix — a helper for the sparse sampler's tests, not a test. Written from
the algorithm, in the words of the C oracle of SBayesD() (oracle/hb_sbayes_oracle.c), with what SBayesS() has beyond it:
  * varediff[i] = (m - nnz(column i)) / m and the marker's own residual variance varei = varediff[i] * vara_ + vare_ (:131-141, :285);
  * a move updates r_hat at the stored rows of the marker's column only (:292-296);
  * BayesC / BayesCpi / BayesR: an effect with gi * gi * vx[i] > vary is redrawn until it is not; the 101st redraw is followed by
    gi = 0, which ends the loop with the marker still counted as included (:388-398, :489-499). `vargi = gi * gi` inside that loop
    (:392) starts BayesC's sum of squared effects again at that marker (the sum the sweep's varg is drawn from, :414); in BayesR
    the same statement writes a variable nobody reads.
Every floating-point operation is the scalar IEEE operation of the C oracle in the same order (math.log / exp / sqrt are the C
library's; the dot products are summed left to right), so on a matrix that stores every entry — varediff = 0, varei = vare_
exactly — and with no redraw the records equal O.sbayes(..., rng=RNG_PHILOX) in every bit (test_sbayess_host.py pins that).

Draws come from the oracle's Philox functions: marker i's blocks 64 i + 0 / 1 / 2 / 4 under sub = (1 << 56) | iter exactly as
oracle/hb_sbayes_oracle.c:61-84, the host stream as Stream(RNG_PHILOX, seed, (2 << 56) | iter), and — purpose 4, new with this
sampler — the normal of redraw k = 1, 2, ... of marker i in sweep iter from block 128 i + k under sub = (4 << 56) | iter.

Returns what O.sbayes returns, plus "redraws" (marker-sweeps that redrew at least once) and "zeroed" (those that ended at 0).

`trace`: a list that receives one record per sweep, four m-long arrays taken from this sequential chain (nothing here simulates
the device's rounds; `group` is the number of consecutive markers one chain launch of the device holds, SB_GS = SS_GS = 512):
  g_before  the effects when the sweep began;
  entry_in  the decision the marker would get, with its own draws, from r_hat as it stood when the sweep reached the first
            marker of the marker's block of `group` (true for every marker with statistics under BayesRR / BayesA / BayesL);
  turn_in   the decision at the marker's own turn;
  moved     the marker's effect changed.
Each model's decision is a function of (marker, right-hand side) for that; with trace=None nothing else differs, and the records
are the same in every bit with the trace on or off (test_sbayes_rounds_host.py)."""
import math

import numpy as np

from oracle import oracle as O

PURPOSE_MARKER, PURPOSE_HOST, PURPOSE_REDRAW = 1, 2, 4
BLK_PER_MARKER, REDRAW_BLK = 64, 128


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def _log(x):
    """C's log: -inf at 0, NaN below (math.log raises)"""
    return math.log(x) if x > 0 else (-math.inf if x == 0 else math.nan)


def _sqrt(x):
    return math.sqrt(x) if x >= 0 else math.nan


def seq_sum(v):
    """left-to-right sum, as a C loop `s += v[i]`"""
    return float(np.add.accumulate(np.asarray(v, dtype=np.float64))[-1]) if len(v) else 0.0


def arma_sum(v):
    """Armadillo's accumulate: two interleaved accumulators (oracle/hb_sbayes_oracle.c:29-39)"""
    v = np.asarray(v, dtype=np.float64)
    return seq_sum(v[0::2]) + seq_sum(v[1::2])


def varediff_of(csc):
    m = csc.shape[0]
    return (m - np.diff(csc.indptr).astype(np.float64)) / m          # :140


def sbayess_restatement(sumstat, csc, model, Pi, fold=None, niter=50000, nburn=20000, thin=5, vg=None, dfvg=None, s2vg=None,
                        ve=None, dfve=None, s2ve=None, windindx=None, seed=666666, trace=None, group=512):
    L = O.lib()
    ss = np.asarray(sumstat, dtype=np.float64)
    m = csc.shape[0]
    if ss.shape[0] != m:
        raise RuntimeError("Number of SNPs not equals.")
    indptr, indices, data = csc.indptr, csc.indices, csc.data
    for j in (0, m // 2, m - 1):
        assert np.all(np.diff(indices[indptr[j]:indptr[j + 1]]) > 0), "rows must be sorted inside a column"
    mi = {"BayesRR": 1, "BayesA": 2, "BayesB": 3, "BayesBpi": 3, "BayesC": 4, "BayesCpi": 4, "BayesL": 5}.get(model, 6)
    N = ss[:, 3]
    n = int(N[np.isfinite(N)].sum() / max(1, int(np.isfinite(N).sum())))
    fixpi = model in ("BayesB", "BayesC")
    Pi = [float(p) for p in Pi]
    n_fold = len(Pi)
    fold_ = [0.0] * n_fold if fold is None else [float(f) for f in fold]
    assert len(fold_) == n_fold and (fold is not None or model != "BayesR")
    n_records = (niter - nburn) // thin
    always_in = mi in (1, 2, 5)
    NnzSnp = 0
    if always_in:
        NnzSnp, Pi[0], Pi[1], fixpi = m, 0.0, 1.0, True
    snptracker, nzrate = np.zeros(m), np.zeros(m)
    vx = np.asarray(csc.diagonal(), dtype=np.float64)
    xpx = vx * n
    b, se = ss[:, 1], ss[:, 2]
    ifest = ~(np.isnan(b) | np.isnan(se) | np.isnan(N))
    nvar0, count_y = int((~ifest).sum()), int(ifest.sum())
    xy = np.where(ifest, xpx * np.nan_to_num(b), 0.0)
    r_hat = xy.copy()
    with np.errstate(invalid="ignore"):
        yyi = np.where(ifest, xpx * (b * b + (N - 2) * se * se), 0.0)
    varediff = varediff_of(csc)
    yy = arma_sum(yyi) / count_y
    vary = yy / (n - 1)
    h2 = 0.5
    dfvara_ = 4.0 if dfvg is None else float(dfvg)
    vara_ = ((dfvara_ - 2) / dfvara_) * vary * h2 if vg is None else float(vg)
    vare_ = vary * (1 - h2) if ve is None else float(ve)
    dfvare_ = -2.0 if dfve is None else float(dfve)
    s2vara_ = vara_ * (dfvara_ - 2) / dfvara_ if s2vg is None else float(s2vg)
    sumvx = arma_sum(vx)
    varg = vara_ / ((1 - Pi[0]) * sumvx)
    s2varg_ = s2vara_ / ((1 - Pi[0]) * sumvx)
    s2vare_ = 0.0 if s2ve is None else float(s2ve)
    R2 = (dfvara_ - 2) / dfvara_
    lambda2 = 2 * (1 - R2) / (R2) * sumvx
    lam = _sqrt(lambda2)
    shape0 = 1.1
    rate0 = (shape0 - 1) / lambda2
    vargL = np.full(m, varg)
    vara_fold = [(vara_ / ((1 - Pi[0]) * sumvx)) * f for f in fold_]
    fold_snp_num = [0.0] * n_fold
    nw = 0
    if windindx is not None:
        wi = np.asarray(windindx, dtype=np.int64)
        nw = int(wi.max())
        wppai = np.zeros(nw)
    g = np.zeros(m)
    s_alpha, s_pi = np.zeros((m, n_records), order="F"), np.zeros((n_fold, n_records), order="F")
    s_Vg, s_Ve, s_h2 = np.zeros(n_records), np.zeros(n_records), np.zeros(n_records)
    pi_sum, g_sum = [0.0] * n_fold, np.zeros(m)
    vara_sum = vare_sum = hsq_sum = 0.0
    count = nzct = 0
    redraws = zeroed = 0
    est = np.flatnonzero(ifest)
    cols = [(indices[indptr[i]:indptr[i + 1]], data[indptr[i]:indptr[i + 1]]) for i in range(m)]

    def move(i, gi):
        rows, vals = cols[i]
        r_hat[rows] += ((g[i] - gi) * n) * vals                      # gi_ = (g[i] - gi) * n; r_hat[row] += gi_ * value
        g[i] = gi

    for it in range(niter):
        glob = O.Stream(O.RNG_PHILOX, seed, (PURPOSE_HOST << 56) | it)
        sub, subr = (PURPOSE_MARKER << 56) | it, (PURPOSE_REDRAW << 56) | it
        unif = lambda i: L.hbo_philox_uniform(seed, sub, i * BLK_PER_MARKER + 0)
        norm = lambda i: L.hbo_philox_normal(seed, sub, i * BLK_PER_MARKER + 1)
        chisq = lambda i, df: O.Stream(O.RNG_PHILOX, seed, sub, i * BLK_PER_MARKER + 4).chisq(df)

        rec, nxt = None, 0
        if trace is not None:
            rec = {"g_before": g.copy(), "entry_in": np.zeros(m, dtype=bool), "turn_in": np.zeros(m, dtype=bool),
                   "moved": np.zeros(m, dtype=bool)}
            trace.append(rec)

        def enter(i, included):
            """before marker i's turn: every block of `group` the sweep has reached gets its markers' decisions from r_hat as it is"""
            nonlocal nxt
            while i >= nxt:
                for j in est[(est >= nxt) & (est < nxt + group)]:
                    j = int(j)
                    rhs = r_hat[j]
                    if g[j]:
                        rhs += xpx[j] * g[j]
                    rec["entry_in"][j] = included(j, rhs)
                nxt += group

        def truncated(i, gi, rhs, v, varei):
            """:388-398 / :489-499; returns (gi, redrew, last draw squared)"""
            nonlocal redraws, zeroed
            if not (gi * gi * vx[i]) > vary:
                return gi, False, 0.0
            ii, last2 = 0, 0.0
            while (gi * gi * vx[i]) > vary:
                ii += 1
                gi = rhs / v + _sqrt(varei / v) * L.hbo_philox_normal(seed, subr, i * REDRAW_BLK + ii)
                last2 = gi * gi
                if ii > 100:
                    gi = 0.0
            redraws += 1
            zeroed += ii > 100
            return gi, True, last2

        if mi in (1, 2, 5):
            for i in est:
                i = int(i)
                if rec is not None:
                    enter(i, lambda j, rhs: True)
                    rec["turn_in"][i] = True
                xx, gi = xpx[i], g[i]
                varei = varediff[i] * vara_ + vare_
                if mi == 2:
                    varg = (gi * gi + s2varg_ * dfvara_) / chisq(i, dfvara_ + 1)
                rhs = r_hat[i]
                if gi:
                    rhs += xx * gi
                v = xx + 1 / vargL[i] if mi == 5 else xx + varei / varg
                gi = rhs / v + _sqrt(varei / v) * norm(i)
                if mi == 5:
                    if abs(gi) < 1e-6:
                        gi = 1e-6
                    vargi = 1 / O.Stream(O.RNG_PHILOX, seed, sub, i * BLK_PER_MARKER + 2).invgauss(_sqrt(varei) * lam / abs(gi), lambda2)
                    if vargi > 0:
                        vargL[i] = vargi
                    if gi != g[i]:
                        move(i, gi)
                else:
                    move(i, gi)
                if rec is not None:
                    rec["moved"][i] = g[i] != rec["g_before"][i]
            if mi == 1:
                varg = (seq_sum(g * g) + s2varg_ * dfvara_) / glob.chisq(dfvara_ + count_y)
            if mi == 5:
                lambda2 = glob.gamma(shape0 + count_y, 1 / (rate0 + arma_sum(vargL) / 2))
                lam = _sqrt(lambda2)
        elif mi in (3, 4):
            logpi = [_log(p) for p in Pi]
            s0 = logpi[0]
            vargi = 0.0

            def decide(i, rhs):
                """marker i's class from its right-hand side, with its own draws (g[i] is the effect it entered the sweep with
                until its turn is over); also the variance of its effect"""
                xx, gi = xpx[i], g[i]
                varei = varediff[i] * vara_ + vare_
                vgi = (gi * gi + s2varg_ * dfvara_) / chisq(i, dfvara_ + 1) if mi == 3 else varg
                lhs = xx / varei
                logdetV = _log(vgi * lhs + 1)
                uhat = rhs / (xx + varei / vgi)
                s1 = -0.5 * (logdetV - (rhs * uhat / varei)) + logpi[1]
                acceptProb = 1 / (_exp(s0 - s0) + _exp(s1 - s0))
                return (0 if unif(i) < acceptProb else 1), vgi

            for i in est:
                i = int(i)
                if rec is not None:
                    enter(i, lambda j, rhs: decide(j, rhs)[0] != 0)
                xx, gi = xpx[i], g[i]
                varei = varediff[i] * vara_ + vare_
                rhs = r_hat[i]
                if gi:
                    rhs += xx * gi
                flag, vgi = decide(i, rhs)
                if mi == 3:
                    varg = vgi
                snptracker[i] = flag
                if flag == 0:
                    gi = 0.0
                else:
                    v = xx + varei / varg
                    gi = rhs / v + _sqrt(varei / v) * norm(i)
                    if mi == 4:
                        gi, redrew, last2 = truncated(i, gi, rhs, v, varei)
                        if redrew:
                            vargi = last2                           # :392
                        vargi += gi * gi
                if gi != g[i]:
                    move(i, gi)
                if rec is not None:
                    rec["turn_in"][i] = flag != 0
                    rec["moved"][i] = g[i] != rec["g_before"][i]
            fold_snp_num[1] = float(snptracker.sum())
            fold_snp_num[0] = m - nvar0 - fold_snp_num[1]
            NnzSnp = int(fold_snp_num[1])
            if mi == 4:
                varg = (vargi + s2varg_ * dfvara_) / glob.chisq(dfvara_ + NnzSnp)
            if not fixpi:
                xn = [glob.gamma(c + 1, 1.0) for c in fold_snp_num]
                sx = arma_sum(xn)
                Pi = [x / sx for x in xn]
        else:
            logpi = [_log(p) for p in Pi]
            varg = 0.0

            def decide(i, rhs):
                """marker i's class from its right-hand side, with its own draw"""
                xx = xpx[i]
                varei = varediff[i] * vara_ + vare_
                lhs = xx / varei
                s = [logpi[0]] + [0.0] * (n_fold - 1)
                for j in range(1, n_fold):
                    logdetV = _log(vara_fold[j] * lhs + 1)
                    uhat = rhs / (xx + varei / vara_fold[j])
                    s[j] = -0.5 * (logdetV - (rhs * uhat / varei)) + logpi[j]
                stemp = []
                for j in range(n_fold):
                    temp = 0.0
                    for k in range(n_fold):
                        temp += _exp(s[k] - s[j])
                    stemp.append(1 / temp)
                acceptProb, flag, rval = 0.0, 0, unif(i)
                for j in range(n_fold):
                    acceptProb += stemp[j]
                    if rval < acceptProb:
                        flag = j
                        break
                return flag

            for i in est:
                i = int(i)
                if rec is not None:
                    enter(i, lambda j, rhs: decide(j, rhs) != 0)
                xx, gi = xpx[i], g[i]
                varei = varediff[i] * vara_ + vare_
                rhs = r_hat[i]
                if gi:
                    rhs += xx * gi
                flag = decide(i, rhs)
                snptracker[i] = flag
                if flag == 0:
                    gi = 0.0
                else:
                    v = xx + varei / vara_fold[flag]
                    gi = rhs / v + _sqrt(varei / v) * norm(i)
                    gi, _, _ = truncated(i, gi, rhs, v, varei)
                    varg += gi * gi / fold_[flag]
                if gi != g[i]:
                    move(i, gi)
                if rec is not None:
                    rec["turn_in"][i] = flag != 0
                    rec["moved"][i] = g[i] != rec["g_before"][i]
            fold_snp_num = [float((snptracker == j).sum()) for j in range(n_fold)]
            NnzSnp = int(m - fold_snp_num[0])
            varg = (varg + s2varg_ * dfvara_) / glob.chisq(dfvara_ + NnzSnp)
            vara_fold = [varg * f for f in fold_]
            fold_snp_num[0] -= nvar0
            if not fixpi:
                xn = [glob.gamma(c + 1, 1.0) for c in fold_snp_num]
                sx = arma_sum(xn)
                Pi = [x / sx for x in xn]
        vara_ = (seq_sum(g * (xy - r_hat)) + s2vara_ * dfvara_) / glob.chisq(n + dfvara_)      # :529-531
        vare_ = (yy - seq_sum(g * (xy + r_hat)) + s2vare_ * dfvare_) / glob.chisq(n + dfvare_)  # :536-537
        if vare_ < 0:
            vare_ = vara_ * 0.5
        if it >= nburn:
            if not always_in:
                nzrate[snptracker != 0] += 1
            if nw:
                wf = np.zeros(nw)
                wf[wi[snptracker != 0] - 1] = 1
                wppai += wf
            nzct += 1
        if it >= nburn and (it + 1 - nburn) % thin == 0:
            if not fixpi:
                for j in range(n_fold):
                    s_pi[j, count] = Pi[j]
                    pi_sum[j] += Pi[j]
            s_Vg[count], s_Ve[count], s_h2[count] = vara_, vare_, vara_ / (vara_ + vare_)
            vara_sum += vara_
            vare_sum += vare_
            hsq_sum += vara_ / (vara_ + vare_)
            s_alpha[:, count] = g
            g_sum += g
            count += 1
        if count == n_records:
            break
    Rn = float(n_records)
    if not fixpi:
        Pi = [p / Rn for p in pi_sum]
    else:
        s_pi[0, :], s_pi[1, :] = Pi[0], Pi[1]
    if always_in:
        pip = np.ones(m)
    else:
        pip = nzrate / nzct
        pip[pip == 1] = (nzct - 1) / float(nzct)
    res = {"Vg": vara_sum / Rn, "Ve": vare_sum / Rn, "h2": hsq_sum / Rn, "alpha": g_sum / Rn, "pi": np.array(Pi), "pip": pip,
           "s_Vg": s_Vg, "s_Ve": s_Ve, "s_h2": s_h2, "s_alpha": s_alpha, "s_pi": s_pi, "r_hat": r_hat, "g_last": g.copy(),
           "n_records": n_records, "nzct": nzct, "nw": nw, "n": n, "count_y": count_y, "vary": vary,
           "redraws": redraws, "zeroed": zeroed}
    if nw:
        gw = wppai / nzct
        gw[gw == 1] = (nzct - 1) / float(nzct)
        res["gwas"] = gw
    return res
