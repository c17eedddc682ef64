"""window_pve(): the phenotypic or genetic variance explained by single markers or by windows of markers — item (8) of the reference README's
list of what hibayes estimates. The reference leaves it to the R session after ibrm()'s GEBV step (R/bayes.r:303-308), as
apply(geno, 2, var) * alpha^2 / var(pheno): right for one marker, wrong for a window of markers in LD, where the quantity is var(X_w alpha_w).
Here the window variances of every stored record come from the resident genotypes in one pass (Context.window_var, hb_pve.hip), and with
them the posterior mean PVE of a window and the variance-based WPPA of Fernando et al.: the share of records in which the window explains more
than a threshold of the genetic variance.

ld_window_pve(): the same for the summary-level model, where there are no genotypes. sbrm() (R/sbayes.r:231-234) returns the windows' WPPA and
stops there; the variance a window explains is the quadratic form alpha_w' V_ww alpha_w on the LD matrix the sampler swept, taken from the
handle's device copy in one pass per batch of records (LDMatrix.window_var, hb_ldquad.hip)."""
import numpy as np

from .engine import Context


def _is_integer_codes(M):
    M = np.asarray(M)
    if M.dtype.kind in "iu":
        return M.size == 0 or (M.min() >= -128 and M.max() <= 127)
    if M.dtype.kind != "f" or not np.isfinite(M).all():
        return False
    return bool(np.all(M == np.rint(M)) and (M.size == 0 or (M.min() >= -128 and M.max() <= 127)))


def check_pve_args(m, alpha, windindx, vary, threshold):
    """The argument checks of window_pve() that need no device: (alpha as m x R, windindx as uint32 or None, nw)."""
    a = np.asarray(alpha, dtype=np.float64)
    if a.ndim == 1:
        a = a.reshape(-1, 1)
    if a.ndim != 2 or a.shape[0] != m:
        raise ValueError("alpha must be (m,) or (m, R) with m = %d markers" % m)
    if a.shape[1] < 1:
        raise ValueError("alpha holds no record")
    if not np.isfinite(a).all():
        raise ValueError("alpha must be finite")
    if vary is not None and not (np.isfinite(vary) and vary > 0):
        raise ValueError("vary must be a positive number")
    if threshold is not None and not (np.isfinite(threshold) and threshold >= 0):
        raise ValueError("threshold must be a non-negative number")
    if windindx is None:
        return np.asfortranarray(a), None, m
    w = np.asarray(windindx)
    if w.shape != (m,) or w.dtype.kind not in "iu":
        raise ValueError("windindx must hold one integer window id per marker")
    if w.size and w.min() < 1:
        raise ValueError("windindx must hold window ids in 1 .. nw")
    return np.asfortranarray(a), np.ascontiguousarray(w, dtype=np.uint32), int(w.max())


def pve_plan(A, windindx, nw, s1, n, ld=None, num_cus=256):
    """hb_pve_plan (hb_pveplan.hpp; needs no device) of one batch, A: m x nr with nr <= 8: dict(idx, val (entries x 8), segs [(window 0-based,
    first entry, count)], shift (segments x 8), total_shift (8), chunks [(first segment, count)], row_blocks). Refusals raise HibayesError."""
    import ctypes as C
    from ._lib import check, lib
    windindx = np.ascontiguousarray(windindx, dtype=np.uint32)
    m = windindx.size
    A = np.asfortranarray(np.asarray(A, dtype=np.float64).reshape(m, -1))
    s1 = np.ascontiguousarray(s1, dtype=np.float64)
    if s1.size != m:
        raise ValueError("s1 must hold one column sum per marker")
    ld = (int(n) + 255) // 256 * 256 if ld is None else int(ld)
    counts = np.zeros(4, dtype=np.int32)
    idx, segs, chunks = np.zeros(m, dtype=np.int32), np.zeros(3 * m, dtype=np.int32), np.zeros(2 * m, dtype=np.int32)
    val, shift, tot = np.zeros(8 * m), np.zeros(8 * m), np.zeros(8)
    check(lib().hb_pve_plan(A.ctypes.data, m, m, A.shape[1], windindx.ctypes.data, int(nw), s1.ctypes.data, int(n), ld, int(num_cus),
                            counts.ctypes.data, idx.ctypes.data, val.ctypes.data, segs.ctypes.data, shift.ctypes.data, tot.ctypes.data, chunks.ctypes.data))
    nnz, nseg, nch, nrb = (int(v) for v in counts)
    return {"idx": idx[:nnz].tolist(), "val": val[:8 * nnz].reshape(nnz, 8), "segs": [tuple(int(v) for v in segs[3 * s:3 * s + 3]) for s in range(nseg)],
            "shift": shift[:8 * nseg].reshape(nseg, 8), "total_shift": tot, "chunks": [tuple(int(v) for v in chunks[2 * k:2 * k + 2]) for k in range(nch)],
            "row_blocks": nrb}


def pve_summary(var, total, vary=None, threshold=None):
    """The host arithmetic on the device's numbers: pve = var / vary, or var / total (0 where total is 0); mean = its row means; wppa (R > 1) =
    the share of records with var / total > threshold (default 1 / nw)."""
    var, total = np.asarray(var, dtype=np.float64), np.asarray(total, dtype=np.float64)
    nw, R = var.shape
    share = np.zeros_like(var)
    np.divide(var, total[None, :], out=share, where=total[None, :] != 0.0)
    pve = share if vary is None else var / float(vary)
    out = {"var": var, "total": total, "pve": pve, "mean": pve.mean(axis=1)}
    if R > 1:
        thr = 1.0 / nw if threshold is None else float(threshold)
        out["wppa"] = (share > thr).mean(axis=1)
        out["threshold"] = thr
    return out


def window_pve(M, alpha, windindx=None, *, vary=None, threshold=None, device=0):
    """M: the n x m genotypes (integer codes are uploaded as int8 columns, anything else as real-valued ones) or a Context that holds them;
    alpha: (m,) or (m, R), one column per record (MCMCsamples["alpha"] or the posterior mean); windindx: m window ids in 1 .. nw as
    cutwind_by_bp / cutwind_by_num give them, or None: every marker its own window — the reference's closed form vx_j * alpha_j^2, from
    Context.marker_stats(), which launches nothing beyond them.
    Returns a dict: var (nw x R, var(X_w alpha_w)), total (R, var(X alpha)), pve (var / vary when vary — var(y), say — is given, else
    var / total, 0 where total is 0), mean (the posterior mean PVE, row means of pve) and, for R > 1, wppa: the share of records with
    var / total > threshold (default 1 / nw), and that threshold."""
    own = not isinstance(M, Context)
    if own:
        M = np.asarray(M)
        if M.ndim != 2:
            raise ValueError("M must be an n x m matrix or a Context")
        n, m = M.shape
    else:
        n, m = M.n, M.m
    a, w, nw = check_pve_args(m, alpha, windindx, vary, threshold)
    if n < 2:
        raise ValueError("a variance needs n >= 2 individuals")
    ctx = M
    if own:
        ctx = Context(n, m, device=device)
    try:
        if own:
            if _is_integer_codes(M):
                ctx.upload(M if M.dtype == np.int8 else M.astype(np.int8))
            else:
                ctx.upload_real(M)
        if w is None:
            vx = ctx.marker_stats()[1]
            var = vx[:, None] * a * a
            total = ctx.window_var(a, np.ones(m, dtype=np.uint32))[1]
        else:
            var, total = ctx.window_var(a, w)
    finally:
        if own:
            ctx.close()
    return pve_summary(var, total, vary, threshold)


def sbayes_vary(sumstat, diag):
    """var(y) as SBayesD() and SBayesS() take it from the summary statistics (src/SBayesD.cpp:93-115): sumstat m x 4 (MAF, BETA, SE, NMISS; NaN =
    NA), diag the LD matrix's diagonal. n = the mean of the finite NMISS cut to an integer (:33-34), xpx_k = diag_k n, and over the markers with
    BETA, SE and NMISS all present yy_k = xpx_k (BETA^2 + (NMISS - 2) SE^2); vary = (sum yy_k / their count) / (n - 1)."""
    ss = np.asarray(sumstat, dtype=np.float64)
    if ss.ndim != 2 or ss.shape[1] != 4:
        raise ValueError("sumstat must have the four columns MAF, BETA, SE, NMISS")
    d = np.asarray(diag, dtype=np.float64)
    if d.shape != (ss.shape[0],):
        raise ValueError("diag must hold one entry per marker")
    nm = ss[:, 3]
    if not np.isfinite(nm).any():
        raise ValueError("Lack of NMISS.")
    n = int(nm[np.isfinite(nm)].mean())
    est = ~(np.isnan(ss[:, 1]) | np.isnan(ss[:, 2]) | np.isnan(ss[:, 3]))
    if not est.any():
        raise ValueError("Lack of SE.")
    yyi = (d[est] * n) * (ss[est, 1] * ss[est, 1] + (ss[est, 3] - 2.0) * ss[est, 2] * ss[est, 2])
    return float(yyi.sum() / int(est.sum()) / (n - 1))


def ld_window_pve(ldm, alpha, windindx=None, *, vary=None, threshold=None, device=0):
    """ldm: an LDMatrix (ldmat(..., keep_on_device=True), LDMatrix.from_scipy), a scipy sparse matrix, or a square ndarray — the last two are
    handed over as CSC (LDMatrix.from_scipy; an ndarray with its exact zeros dropped), so they must equal their transpose; alpha, windindx,
    vary and threshold as in window_pve(). Returns window_pve()'s dict, with var[w, r] = alpha_w,r' V_ww alpha_w,r and
    total[r] = alpha_r' V alpha_r over the stored entries. windindx=None: every marker its own window, var = diag(V) alpha^2 as the closed
    form, and only the total comes from the pass. A thresholded LD matrix is indefinite: a negative var or total is a finding and is
    returned as computed."""
    from .ldm import LDMatrix
    own = None
    if not isinstance(ldm, LDMatrix):
        import scipy.sparse as sp
        if not sp.issparse(ldm):
            V = np.asarray(ldm, dtype=np.float64)
            if V.ndim != 2 or V.shape[0] != V.shape[1]:
                raise ValueError("ldm must be an LDMatrix, a scipy sparse matrix or a square array")
            ldm = sp.csc_matrix(V)
        elif ldm.ndim != 2 or ldm.shape[0] != ldm.shape[1]:
            raise ValueError("ldm must be an LDMatrix, a scipy sparse matrix or a square array")
    m = ldm.shape[0]
    a, w, nw = check_pve_args(m, alpha, windindx, vary, threshold)
    if not isinstance(ldm, LDMatrix):
        ldm = own = LDMatrix.from_scipy(ldm, device=device)
    try:
        if w is None:
            var = ldm.diagonal()[:, None] * a * a
            # (the total alone is wanted: the pass with one window, whose form — the total once more, added per column — is dropped. A total's bits
            # do not depend on the window map, so this is the total every other map gives.)
            total = ldm.window_var(a, np.ones(m, dtype=np.uint32))[1]
        else:
            var, total = ldm.window_var(a, w)
    finally:
        if own is not None:
            own.close()
    return pve_summary(var, total, vary, threshold)
