"""Host mirror of the reference's conjugate-gradient fitter: conjgt_den() on a dense LD matrix (src/cg.cpp:68-129), conjgt_spa()
on a sparse one (src/cg.cpp:4-65) and sbrm()'s method = "CG" arm that leads to them (R/sbayes.r:206-229, :235-236). The solve
(V + diag(lambda)) g = b runs on the device through hb_cg_run / hb_cg_run_ldm / hb_cg_run_sparse (include/hibayes_gpu.h); there
is no CPU fallback."""
import ctypes as C

import numpy as np

from ._lib import LOG_FN, CGArgs, CGOut, check, lib
from .ldm import LDMatrix


def _issparse(ldm):
    try:
        import scipy.sparse as sp
    except ImportError:
        return False
    return sp.issparse(ldm)


def conjgt_den(sumstat, ldm, lambda_=None, esp=1e-6, outfreq=100, verbose=True, *, device=0, log=None):
    """sumstat: m x 4 (MAF, BETA, SE, NMISS; NaN = NA); ldm: m x m dense, which must equal its transpose bit for bit, or an
    LDMatrix (ldmat(..., keep_on_device=True)): the run then reads the handle's dense device copy on the handle's device.
    lambda_: None or m values. Returns vg, ve, g as the reference does, and n, count_y, iterations (passes of the loop),
    converged, err, err_hist (err of every pass) and timing."""
    if _issparse(ldm):
        raise ValueError("conjgt_den needs a dense ldm or an LDMatrix (a scipy sparse matrix goes to conjgt_spa)")
    return _run(False, sumstat, ldm, lambda_, esp, outfreq, verbose, device, log)


def conjgt_spa(sumstat, ldm, lambda_=None, esp=1e-6, outfreq=100, verbose=True, *, device=0, log=None):
    """conjgt_den()'s arguments and results on a sparse LD matrix: an LDMatrix of any kind, or a scipy sparse matrix, which must
    equal its transpose (LDMatrix.from_scipy). The products walk the stored entries of the handle's device CSC: no m x m array
    exists on either side."""
    own = None
    if not isinstance(ldm, LDMatrix):
        if not _issparse(ldm):
            raise ValueError("conjgt_spa needs an LDMatrix or a scipy sparse ldm (a dense array goes to conjgt_den)")
        if ldm.ndim != 2 or ldm.shape[0] != ldm.shape[1] or ldm.shape[0] != np.shape(sumstat)[0]:
            raise ValueError("Number of SNPs not equals.")
        ldm = own = LDMatrix.from_scipy(ldm, device=device)
    try:
        return _run(True, sumstat, ldm, lambda_, esp, outfreq, verbose, device, log)
    finally:
        if own is not None:
            own.close()


def _run(sparse, sumstat, ldm, lambda_, esp, outfreq, verbose, device, log):
    L = lib()
    ss = np.asfortranarray(sumstat, dtype=np.float64)
    handle = ldm if isinstance(ldm, LDMatrix) else None
    ld = None if handle is not None else np.asfortranarray(ldm, dtype=np.float64)
    if ss.ndim != 2 or ss.shape[1] != 4:
        raise ValueError("sumstat must have the four columns MAF, BETA, SE, NMISS")
    m = ss.shape[0]
    a = CGArgs()
    if handle is not None:
        a.m = m if handle.shape[0] == m else -1                                   # -> "Number of SNPs not equals."
        a.sumstat, a.ld_sumstat, a.ldm, a.ld_ldm = ss.ctypes.data, m, None, 0
        device = handle.device
    else:
        a.m = m if ld.ndim == 2 and ld.shape[0] == m and ld.shape[1] == m else -1
        a.sumstat, a.ld_sumstat, a.ldm, a.ld_ldm = ss.ctypes.data, m, ld.ctypes.data, (ld.shape[0] if ld.ndim == 2 else 0)
    keep = [ss, ld]
    if lambda_ is not None:
        lam = np.ascontiguousarray(lambda_, dtype=np.float64).ravel()
        if lam.size != m:
            raise ValueError("length of lambda should be equal to the number of SNPs.")
        a.lambda_ = lam.ctypes.data
        keep.append(lam)
    a.esp, a.outfreq, a.verbose, a.device = float(esp), int(outfreq), int(bool(verbose)), int(device)
    if log is not None:
        cb = LOG_FN(lambda line, _u: log(line.decode("utf-8", "replace")))
        a.log = cb
        keep.append(cb)
    mm = max(m, 1)
    g, hist = np.zeros(mm), np.zeros(mm)
    o = CGOut()
    o.g, o.err_hist = g.ctypes.data, hist.ctypes.data
    if handle is not None:
        check((L.hb_cg_run_sparse if sparse else L.hb_cg_run_ldm)(C.byref(a), handle._handle(), C.byref(o)))
    else:
        check(L.hb_cg_run(C.byref(a), C.byref(o)))
    del keep
    return {"vg": o.vg, "ve": o.ve, "g": g[:m], "n": o.n, "count_y": o.count_y, "iterations": o.iterations,
            "converged": bool(o.converged), "err": o.err, "err_hist": hist[:o.iterations].copy(),
            "timing": {"setup_seconds": o.setup_seconds, "loop_seconds": o.loop_seconds}}


def sbrm_cg(sumstat, ldm, lambda_=None, printfreq=100, verbose=True, sparse_ld=False, **kw):
    """The method = "CG" arm of the reference's sbrm() (R/sbayes.r:206-229, :235-236): the column selection
    sumstat[, c(4, 5, 6, 8)] of the 8-column COJO table (:209), a scalar lambda repeated for every marker (:219-220), then
    conjgt_den() for a dense array or an LDMatrix and conjgt_spa() for a scipy sparse matrix — or, with sparse_ld=True, for an
    LDMatrix (:225-229). The result carries `call` and `model` and, like the reference's, no `gwas`. sbrm(method="CG") itself
    does not come here yet."""
    ss = np.asarray(sumstat, dtype=np.float64)
    if ss.ndim == 2 and ss.shape[1] >= 8:      # the COJO table; a 4-column matrix is taken as MAF, BETA, SE, NMISS already
        ss = ss[:, [3, 4, 5, 7]]
    sparse = _issparse(ldm)
    if sparse_ld and not (sparse or isinstance(ldm, LDMatrix)):
        raise ValueError("sparse_ld=True needs a scipy sparse ldm or an LDMatrix")
    if not (sparse or isinstance(ldm, (np.ndarray, LDMatrix)) or hasattr(ldm, "__array__")):
        raise ValueError("Unrecognized type of ldm.")
    if lambda_ is not None:
        lam = np.atleast_1d(np.asarray(lambda_, dtype=np.float64)).ravel()
        if lam.size == 1:
            lam = np.repeat(lam, ss.shape[0])
        elif lam.size != ss.shape[0]:
            raise ValueError("length of lambda should be equal to the number of SNPs.")
        lambda_ = lam
    if printfreq <= 0:
        verbose = False
    fit = conjgt_spa if (sparse or sparse_ld) else conjgt_den
    res = fit(ss, ldm, lambda_, outfreq=printfreq, verbose=verbose, **kw)
    res["call"] = "b ~ nD^{-1}V alpha + e"
    res["model"] = "Summary level Bayesian model fit by [CG]"
    return res
