"""Host restatement of the fp64 resident layout's sweep (hb_real.hip and k_chain of hb_chain_panel.hpp), one kernel per function, in the
arithmetic the kernels use, so that tests/test_gpu_real_sweep.py can ask for equal bits. No GPU in here; tests/test_real_restatement_host.py
checks every function against a plain formulation.

What is exact, and why. Given what k_pre left (thresholds, 1/v, sd z: Context.pre()), the panel's mat-vec (Context.dot(): k_sum_partials adds the
row splits 0 + ps[0] + ps[1] + ..., the chain adds them in the same order) and the panel's Gram block (Context.gram_real()), k_chain draws
nothing and sums nothing in an order of its own: every lane's right-hand side is one chain of fused multiply-adds, one per move before its
marker, in the order of the move list. chain_panel() is that chain. k_update_real's lanes are a = 0; a = fma(x_e, d_e, a) in list order, then
r - a and u + a: update_real(). Both need fl(a b + c) in ONE rounding, which numpy does not have: fma() below.

What is a bound. stats_real() evaluates k_stats_real's formula in wider arithmetic: the kernel's block sums have an order (threads, shuffle
tree) that a test should not restate, so the kernel is held to the bound of any order, derived in tests/test_gpu_real.py."""
import math
from fractions import Fraction

import numpy as np

WIDE = np.longdouble if np.finfo(np.longdouble).nmant > 52 else None
_SPLIT = 134217729.0            # 2^27 + 1: Veltkamp's splitter
_BIG, _TINY = 2.0 ** 990, 2.0 ** -960


# ------------------------------------------------------------------------------------------------------------------------
# fl(a b + c), one rounding
# ------------------------------------------------------------------------------------------------------------------------
def fma_fraction(a, b, c):
    """fl(a b + c) of three finite doubles through exact rational arithmetic (float(Fraction) rounds to nearest even). An exact zero
    takes IEEE's sign: -0.0 only where the product and c are both negative zeros."""
    a, b, c = float(a), float(b), float(c)
    s = Fraction(a) * Fraction(b) + Fraction(c)
    if s == 0:
        if (a == 0.0 or b == 0.0) and c == 0.0:
            pneg = (math.copysign(1.0, a) < 0) != (math.copysign(1.0, b) < 0)
            return -0.0 if pneg and math.copysign(1.0, c) < 0 else 0.0
        return 0.0
    return float(s)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    """Dekker's product: a b = p + e exactly while nothing overflows in the split and no partial product underflows (the caller checks)"""
    p = a * b
    ca = _SPLIT * a
    ah = ca - (ca - a)
    al = a - ah
    cb = _SPLIT * b
    bh = cb - (cb - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def fma(a, b, c):
    """fl(a b + c) elementwise (broadcasting), one rounding. Vectorised error-free transformations where they are provably one rounding,
    Fraction arithmetic elsewhere.

    a b = p + e (Dekker), p + c = s + t and t + e = v + w (Knuth's two-sum, exact for any doubles): a b + c = s + v + w exactly, with
    |v| <= ulp(s) and |w| <= ulp(v) / 2. r = fl(s + v) = s + v - z with z exact too. If v = w = 0 the answer is s, signed zeros included.
    If w = 0 then r IS the rounding of the exact value. Otherwise r is the rounding of s + v + w unless w carries s + v across the
    midpoint that r's interval ends in, i.e. unless |z| + |w| reaches the half gap on r's narrower side (a quarter of spacing(r) at a
    power of two, half of it elsewhere); fl(|z| + |w|) is never below a float that the exact sum reaches, so testing the rounded sum
    errs to the safe side. Those elements (a near-tie, a cancellation down to w), the ones whose product is below 2^-960 without being an
    exact zero (Dekker's partial products may underflow) and operands above 2^990 (the split overflows) go through fma_fraction."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    shape = a.shape
    a, b, c = a.ravel(), b.ravel(), c.ravel()
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        p, e = _two_prod(a, b)
        s, t = _two_sum(p, c)
        v, w = _two_sum(t, e)
        r, z = _two_sum(s, v)
        plain = (v == 0.0) & (w == 0.0)
        r = np.where(plain, s, r)
        ar = np.abs(r)
        gap = np.spacing(ar) * np.where(np.frexp(ar)[0] == 0.5, 0.25, 0.5)
        near = (w != 0.0) & ~(np.abs(z) + np.abs(w) < gap)
        zero_prod = (a == 0.0) | (b == 0.0)
        unsafe = near | ~(np.abs(a) < _BIG) | ~(np.abs(b) < _BIG) | ~(np.abs(c) < _BIG) | ~(np.abs(p) < _BIG) | ((np.abs(p) < _TINY) & ~zero_prod)
    bad = np.flatnonzero(unsafe)
    if bad.size:
        r = r.copy()
        r[bad] = [fma_fraction(a[i], b[i], c[i]) for i in bad]
    return r.reshape(shape)


# ------------------------------------------------------------------------------------------------------------------------
# k_update_real
# ------------------------------------------------------------------------------------------------------------------------
def update_real(X, r, u, cols, deltas):
    """k_update_real for one panel's move list: a = 0; a = fma(x_e, d_e, a) in list order; r - a, u + a, r32 = float32(r). X: the columns
    as the device holds them (doubles, or int8 codes, which convert exactly). An empty list touches nothing. Returns (r, u, r32)."""
    r, u = np.array(r, dtype=np.float64), np.array(u, dtype=np.float64)
    if len(cols):
        a = np.zeros(len(r))
        for j, d in zip(cols, deltas):
            a = fma(np.asarray(X[:, int(j)], dtype=np.float64), float(d), a)
        r, u = r - a, u + a
    return r, u, r.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------
# k_chain<K1, GT>, one panel
# ------------------------------------------------------------------------------------------------------------------------
MODEL_INDEX = {"BayesRR": 1, "BayesA": 2, "BayesB": 3, "BayesBpi": 3, "BayesC": 4, "BayesCpi": 4, "BayesL": 5, "BayesR": 6}


def chain_panel(G, xpx, vx, g_old, dots, thr, invv, sdz, model, fold=None):
    """k_chain on one panel of P markers. G: the panel's P x P Gram block (doubles, or the exact integers of the int8 layouts), xpx, vx,
    g_old, dots: P values each (dots: the panel's mat-vec on the residual the panel sees), thr, invv, sdz: K1 x P as k_pre left them, model: a
    name or hb_sweep_in's index, fold: BayesR's. Returns (idx, deltas, g_new, cls, sum_w): the move list in the kernel's order, the effects
    and classes it writes back (0 for a marker with vx == 0) and the sum of w = g^2 (BayesR: g^2 / fold[cls]) over the markers with a class.

    The order of a lane's corrections: wave s applies its own moves to its later lanes one by one, in marker order; a later wave takes the
    moves of wave s from the list, in list order, which is marker order again. So marker t' sees every move of a marker t < t' in ascending
    t, each one fused multiply-add on its right-hand side: the loop below, vectorised over t'."""
    model = MODEL_INDEX[model] if isinstance(model, str) else int(model)
    G = np.asarray(G, dtype=np.float64)
    P = len(dots)
    thr, invv, sdz = (np.asarray(x, dtype=np.float64).reshape(-1, P) for x in (thr, invv, sdz))
    K1 = thr.shape[0]
    g_old = np.asarray(g_old, dtype=np.float64)
    rhs = np.array(dots, dtype=np.float64)
    nz = g_old != 0.0
    rhs[nz] = fma(np.asarray(xpx, dtype=np.float64)[nz], g_old[nz], rhs[nz])
    g_new, cls_out = np.zeros(P), np.zeros(P, dtype=np.int64)
    idx, deltas = [], []
    sum_w = 0.0
    for t in range(P):
        if vx[t] == 0.0:
            continue
        q = rhs[t] * rhs[t]
        if not (g_old[t] != 0.0 or q >= thr[0, t]):
            continue
        cls, iv, sz = 0, 0.0, 0.0
        for c in range(K1):
            if q >= thr[c, t]:
                cls += 1
                iv, sz = invv[c, t], sdz[c, t]
        gn = float(fma(rhs[t], iv, sz)) if cls > 0 else 0.0
        if model == 5 and abs(gn) < 1e-6:
            gn = 1e-6
        g_new[t], cls_out[t] = gn, cls
        if cls > 0:
            sum_w += gn * gn / fold[cls] if model == 6 else gn * gn
        delta = gn - g_old[t]
        if delta != 0.0:
            idx.append(t)
            deltas.append(delta)
            if t + 1 < P:
                rhs[t + 1:] = fma(-G[t, t + 1:], delta, rhs[t + 1:])
    return np.array(idx, dtype=np.int64), np.array(deltas, dtype=np.float64), g_new, cls_out, sum_w


# ------------------------------------------------------------------------------------------------------------------------
# k_stats_real
# ------------------------------------------------------------------------------------------------------------------------
def stats_real(X):
    """(xpx, vx) of the columns of X as k_stats_real forms them — xpx = sum x^2; vx = (a2 - a3^2 / n) / (n - 1) with a2, a3 the sums of
    (mean - x)^2 and of (mean - x), arma::var's two passes with its correction term; exactly 0 for a column whose minimum is its maximum (and
    for n < 2) — evaluated in long doubles, or with exactly rounded sums (math.fsum) where a long double is a double. Returned as doubles."""
    X = np.asarray(X, dtype=np.float64)
    n, m = X.shape
    xpx, vx = np.zeros(m), np.zeros(m)
    for j in range(m):
        x = X[:, j]
        if WIDE is not None:
            xw = x.astype(WIDE)
            xpx[j] = float((xw * xw).sum())
            if n < 2 or x.min() == x.max():
                continue
            mean = xw.sum() / n
            t = mean - xw
            a2, a3 = (t * t).sum(), t.sum()
            vx[j] = float((a2 - a3 * a3 / n) / (n - 1))
        else:
            xpx[j] = math.fsum(x * x)          # (x x rounded once: half an ulp a term, far inside the kernel's bound)
            if n < 2 or x.min() == x.max():
                continue
            mean = math.fsum(x) / n
            t = mean - x
            a2, a3 = math.fsum(t * t), math.fsum(t)
            vx[j] = (a2 - a3 * a3 / n) / (n - 1)
    return xpx, vx
