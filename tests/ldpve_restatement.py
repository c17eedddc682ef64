"""Restatement of the LD matrix's window pass (hibayes_amd/csrc/hb_ldquad.hip, hb_ldqplan.hpp) for its tests: the reference in numpy longdouble
and the bound the device is held to.

The quantities, for a record alpha (one column of A) and a window w, over the STORED entries of V (a dense array stores all of them, a scipy
sparse matrix the entries of its CSC, explicit zeros and NaN included):
    var[w]  = sum_{j in w} alpha_j t_j,   t_j = sum_{i in w, (i, j) stored} V_ij alpha_i
    total   = sum_j alpha_j T_j,          T_j = sum_{i, (i, j) stored} V_ij alpha_i
with every term SELECTED, (alpha_i != 0 ? V_ij alpha_i : 0.0) and likewise for the outer factor: an entry meets a result only where both of its
effects are non-zero, so the reference sums over the markers with a non-zero effect and never touches the other entries (a NaN there stays out).

The bound (ld_var_bound), derived, not measured. u = 2^-53, gamma_k = k u / (1 - k u). For one (window, record) pair the device
  1. rounds each product V_ij alpha_i once and adds the column's in-window terms — at most c of them are stored, every other addend is an exact
     0.0 — in some fixed order (a lane's entries in column order, the 64 lanes by a shuffle tree): t_j is off by at most gamma_c sum_i |V_ij alpha_i|,
     whatever the order;
  2. multiplies by alpha_j: one more rounding, gamma_(c + 1);
  3. adds the window's k listed columns (the columns with an effect in any record of the batch; the ones without one in this record add an
     exact 0.0): k - 1 more roundings at most.
So |device - exact| <= gamma_L sum_{i, j in w} |alpha_i| |V_ij| |alpha_j| with L = c + k + 2, c = the largest number of stored in-window
entries of a column of w; for the total the same with all stored rows of a column and all listed columns (the total's sum runs over all m
markers in an order that depends on m alone; the markers that are not listed add an exact 0.0)."""
import numpy as np

U = 2.0 ** -53


def gamma(k):
    return k * U / (1.0 - k * U)


def _dense_and_stored(V):
    """(V as a dense longdouble array with 0 where nothing is stored, the stored mask)"""
    try:
        import scipy.sparse as sp
        sparse = sp.issparse(V)
    except ImportError:
        sparse = False
    if sparse:
        C = V.tocsc()
        m = C.shape[0]
        D, S = np.zeros((m, m), dtype=np.longdouble), np.zeros((m, m), dtype=bool)
        for j in range(m):
            rows = C.indices[C.indptr[j]:C.indptr[j + 1]]
            D[rows, j] = C.data[C.indptr[j]:C.indptr[j + 1]]
            S[rows, j] = True
        return D, S
    D = np.asarray(V, dtype=np.float64).astype(np.longdouble)
    return D, np.ones(D.shape, dtype=bool)


def _forms(D, A, js):
    """alpha_js' D[js, js] alpha_js for every column of A under the select rule: per record, over the markers of js with a non-zero effect"""
    R = A.shape[1]
    out = np.zeros(R, dtype=np.longdouble)
    if js.size == 0:
        return out
    Dw, Aw = D[np.ix_(js, js)], A[js]
    if np.isfinite(Dw).all():       # (x * 0 is an exact 0 for finite x: the plain product is the selected one)
        return (Aw * (Dw @ Aw)).sum(axis=0)
    for r in range(R):
        nz = Aw[:, r] != 0
        a = Aw[nz, r]
        out[r] = a @ (Dw[np.ix_(nz, nz)] @ a) if a.size else 0.0
    return out


def ld_window_var_ref(V, A, w, nw):
    """(var nw x R, total R) in longdouble. V: a square ndarray or a scipy sparse matrix; A: m x R; w: m window ids in 1 .. nw."""
    D, _ = _dense_and_stored(V)
    m = D.shape[0]
    A = np.asarray(A, dtype=np.float64).reshape(m, -1).astype(np.longdouble)
    w = np.asarray(w)
    var = np.zeros((nw, A.shape[1]), dtype=np.longdouble)
    for k in range(nw):
        var[k] = _forms(D, A, np.flatnonzero(w == k + 1))
    return var, _forms(D, A, np.arange(m))


def ld_var_bound(V, A, w, nw):
    """(bound nw x R, bound of the total R); see the module's docstring. A non-finite entry that meets two non-zero effects makes its bound
    non-finite, as it makes the result."""
    D, S = _dense_and_stored(V)
    m = D.shape[0]
    A = np.asarray(A, dtype=np.float64).reshape(m, -1)
    absA, absD = np.abs(A).astype(np.longdouble), np.abs(D)
    w = np.asarray(w)
    used = np.any(A != 0.0, axis=1)
    out = np.zeros((nw, A.shape[1]))
    for k in range(nw):
        js = np.flatnonzero(w == k + 1)
        cols = int(used[js].sum())
        if cols:
            L = int(S[np.ix_(js, js)].sum(axis=0).max()) + cols + 2
            out[k] = (gamma(L) * _forms(absD, absA, js)).astype(np.float64)
    cols = int(used.sum())
    tot = np.zeros(A.shape[1])
    if cols:
        tot = (gamma(int(S.sum(axis=0).max()) + cols + 2) * _forms(absD, absA, np.arange(m))).astype(np.float64)
    return out, tot


def ld_diag_bound(vdiag, A, w, nw, n):
    """What ldmat()'s dense diagonal may be off by, carried into the window forms: V_jj = xx * xx / n with xx = sqrt(sum_k (x_kj - mean_j)^2)
    (src/tXXmat.cpp:67-75, :168). Each term rounds three times (the difference, the square, its addition), the sum of n terms adds n - 1, the
    square root, the product and the division one each and the root enters twice: V_jj (1 + theta), |theta| <= gamma_(n + 8) (the mean's own
    rounding moves the sum by n (mean error)^2, second order). Returns (nw x R, R): gamma_(n + 8) sum_{j in w} alpha_j^2 |V_jj|."""
    A = np.asarray(A, dtype=np.float64).reshape(len(vdiag), -1)
    terms = gamma(n + 8) * np.abs(np.asarray(vdiag, dtype=np.float64))[:, None] * A * A
    w = np.asarray(w)
    out = np.zeros((nw, A.shape[1]))
    for k in range(nw):
        out[k] = terms[w == k + 1].sum(axis=0)
    return out, terms.sum(axis=0)


def sbayes_vary_loop(sumstat, diag):
    """src/SBayesD.cpp:33-34 and :93-115 as literal loops: (vary, n, count_y)"""
    ss = np.asarray(sumstat, dtype=np.float64)
    m = ss.shape[0]
    fin = [ss[k, 3] for k in range(m) if np.isfinite(ss[k, 3])]
    n = int(sum(fin) / len(fin))
    vx, xpx = [0.0] * m, [0.0] * m
    for i in range(m):
        vx[i] = float(diag[i])
        xpx[i] = vx[i] * n
    count_y, yyi = 0, [0.0] * m
    for k in range(m):
        if np.isnan(ss[k, 1]) or np.isnan(ss[k, 2]) or np.isnan(ss[k, 3]):
            continue
        yyi[k] = xpx[k] * (ss[k, 1] * ss[k, 1] + (ss[k, 3] - 2) * ss[k, 2] * ss[k, 2])
        count_y += 1
    yy = sum(yyi) / count_y
    return yy / (n - 1), n, count_y
