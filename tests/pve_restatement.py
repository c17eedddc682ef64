"""Restatement of the window-variance pass (hibayes_amd/csrc/hb_pve.hip, hb_pveplan.hpp) for its tests: the plan by brute force, the reference
in numpy longdouble, and the bound the device is held to.

The bound (var_bound), computed from the inputs and the reference only. u = 2^-53, gamma_k = k u / (1 - k u). For one (window, record) pair let
k be the window's list entries, g_i = sum_j x_ij alpha_j the window's breeding value of individual i, a_i = sum_j |x_ij alpha_j|, gbar the mean of
g and SS = sum (g_i - gbar)^2 = ||P g||^2 (P: the centring projection), so that the quantity is SS / (n - 1). The device
  1. forms ghat_i by k fused multiply-adds in list order: |ghat_i - g_i| <= gamma_k a_i (an entry whose effect is 0.0 in this record adds
     x * 0.0 exactly: k counts every marker of the window that has an effect in any record, which only loosens gamma_k);
  2. subtracts the shift c, the window's mean breeding value as the plan computed it: that == (g_i - c) + e_i with
     |e_i| <= gamma_k a_i + u |ghat_i - c|, and |ghat_i - c| <= |g_i - gbar| + dc + gamma_k a_i, where dc >= |gbar - c| is the shift's own error:
     gamma_(k+2) sum_j |mean_j alpha_j| for the division, the product and the sum of each term, plus, on the fp64 layout, what the column sums
     s1_j are off by, gamma_n sum_j mean|x_j| |alpha_j| (the integer layouts' sums are exact);
  3. sums that and that^2. For ANY c, sum (g_i - c)^2 - (sum (g_i - c))^2 / n == SS exactly: c itself cancels, and with the e_i in, the centred sum of
     squares of that moves by at most 2 ||P g|| ||e|| + ||e||^2;
  4. the roundings of the two sums and of the last line: with T = sum that_i^2 = SS + n (gbar - c)^2 (to first order; |gbar - c| <= dc), S2 is
     off by at most gamma_n T whatever the order of its n terms, S1^2 / n by 2 gamma_n T (|S1| and sum |that_i| are both <= sqrt(n T)) and the square, the
     division by n, the subtraction and the division by n - 1 add 4 u T: together (3 gamma_n + 4 u) T;
  5. everything is divided by n - 1.
The first-order sum of 3. and 4. is allowed a constant 2 for the second-order terms left out (gamma_k a_i inside |ghat_i - c|, T taken at g
instead of that). A result the device rounds up from below zero to 0.0 only moves towards the non-negative truth."""
import numpy as np

U = 2.0 ** -53
RB = 8          # records per batch (HB_PVE_RB)
ROWS = 1024     # rows of a workgroup (HB_PVE_ROWS)
FILL = 4        # workgroups per compute unit the chunks aim for (HB_PVE_FILL)


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- the plan, by brute force ----
def plan(A, windindx, nw, s1, n, num_cus):
    """A: m x nr (nr <= 8). Returns dict(idx, val (nnz x 8), segs [(window0, first, count)], shift (nseg x 8), total_shift (8), row_blocks) — the
    chunks are checked by their properties, not restated."""
    A = np.asarray(A, dtype=np.float64).reshape(len(windindx), -1)
    m, nr = A.shape
    keys = sorted((int(windindx[j]), j) for j in range(m) if np.any(A[j] != 0.0))
    idx = [j for _, j in keys]
    val = np.zeros((len(idx), RB))
    for e, j in enumerate(idx):
        val[e, :nr] = A[j]
    segs, shift = [], []
    e = 0
    while e < len(keys):
        w, f = keys[e][0], e
        while e < len(keys) and keys[e][0] == w:
            e += 1
        segs.append((w - 1, f, e - f))
        c = np.zeros(RB, dtype=np.longdouble)
        for q in range(f, e):
            c += np.longdouble(s1[idx[q]]) / np.longdouble(n) * val[q].astype(np.longdouble)
        shift.append(c)
    tot = np.zeros(RB, dtype=np.longdouble)
    for q, j in enumerate(idx):
        tot += np.longdouble(s1[j]) / np.longdouble(n) * val[q].astype(np.longdouble)
    return {"idx": idx, "val": val, "segs": segs, "shift": np.array(shift, dtype=np.longdouble).reshape(len(segs), RB), "total_shift": tot,
            "row_blocks": (n + ROWS - 1) // ROWS}


def shift_bound(A, windindx, s1, n, seg, idx):
    """gamma_(k + 2) sum_e |mean_j alpha_j| per record, for the list entries idx[first : first + count] of seg"""
    _, f, k = seg
    js = idx[f:f + k]
    return gamma(k + 2) * (np.abs(np.asarray(s1)[js, None] / n) * np.abs(np.asarray(A).reshape(len(windindx), -1)[js])).sum(0)


# ---- the reference and the bound ----
def window_var_ref(X, A, windindx, nw):
    """(var nw x R, total R) in longdouble: g = X_w alpha_w, var(g, ddof = 1)"""
    Xl = np.asarray(X).astype(np.longdouble)
    A = np.asarray(A, dtype=np.float64).reshape(Xl.shape[1], -1).astype(np.longdouble)
    w = np.asarray(windindx)
    var = np.zeros((nw, A.shape[1]), dtype=np.longdouble)
    for k in range(nw):
        js = np.flatnonzero(w == k + 1)
        if js.size:
            var[k] = (Xl[:, js] @ A[js]).var(axis=0, ddof=1)
    return var, (Xl @ A).var(axis=0, ddof=1)


def _bound_one(Xw, Aw, real):
    """Xw: n x k columns of the window (only those with an effect in any record), Aw: k x R. The bound per record, R."""
    n, k = Xw.shape
    Xl, Al = Xw.astype(np.longdouble), Aw.astype(np.longdouble)
    g = Xl @ Al
    a = np.abs(Xl) @ np.abs(Al)
    gc = g - g.mean(axis=0)
    SS = (gc * gc).sum(axis=0)
    dc = gamma(k + 2) * (np.abs(Xl.mean(axis=0))[:, None] * np.abs(Al)).sum(axis=0)
    if real:
        dc = dc + gamma(n) * (np.abs(Xl).mean(axis=0)[:, None] * np.abs(Al)).sum(axis=0)
    e = gamma(k) * a + U * (np.abs(gc) + dc[None, :])
    en = np.sqrt((e * e).sum(axis=0))
    T = SS + n * dc * dc
    first = 2.0 * np.sqrt(SS) * en + en * en + (3.0 * gamma(n) + 4.0 * U) * T
    return (2.0 * first / (n - 1)).astype(np.float64)


def var_bound(X, A, windindx, nw, real=False):
    """(bound nw x R, bound of the total R); see the module's docstring"""
    X = np.asarray(X)
    A = np.asarray(A, dtype=np.float64).reshape(X.shape[1], -1)
    w = np.asarray(windindx)
    used = np.any(A != 0.0, axis=1)
    out = np.zeros((nw, A.shape[1]))
    for k in range(nw):
        js = np.flatnonzero((w == k + 1) & used)
        if js.size:
            out[k] = _bound_one(X[:, js], A[js], real)
    js = np.flatnonzero(used)
    tot = _bound_one(X[:, js], A[js], real) if js.size else np.zeros(A.shape[1])
    return out, tot


def onepass_uncentred(X, alpha):
    """what the one-pass formula gives in double WITHOUT a shift, its sums taken row by row: (S2 - S1^2 / n) / (n - 1) of g = X alpha"""
    g = np.asarray(X, dtype=np.float64) @ np.asarray(alpha, dtype=np.float64)
    s1 = s2 = 0.0
    for v in g.tolist():
        s1 += v
        s2 += v * v
    n = len(g)
    return (s2 - s1 * s1 / n) / (n - 1)
