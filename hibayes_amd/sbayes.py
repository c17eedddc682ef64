"""Host mirror of the reference's summary-level interface: SBayesD() on a dense LD matrix (src/SBayesD.cpp:5-26, the generated
wrapper R/RcppExports.R:8-10), SBayesS() on a sparse one (src/SBayesS.cpp:21-40) and the slice of sbrm() (R/sbayes.r:101-239)
that leads to them. Everything computes on the device through hb_sbayes_run / hb_sbayes_run_ldm / hb_sbayes_run_sparse
(include/hibayes_gpu.h); there is no CPU fallback."""
import ctypes as C

import numpy as np

from ._lib import LOG_FN, HibayesError, SBayesArgs, SBayesOut, check, lib
from .ldm import LDMatrix


def SBayesD(sumstat, ldm, model, Pi, niter=50000, nburn=20000, thin=5, fold=None, windindx=None, vg=None, dfvg=None, s2vg=None,
            ve=None, dfve=None, s2ve=None, outfreq=100, threads=0, verbose=True, *, seed=666666, device=0, store_alpha=True, log=None):
    """sumstat: m x 4 (MAF, BETA, SE, NMISS — what sbrm() keeps of the COJO file, R/sbayes.r:207; NaN = NA); ldm: m x m dense,
    or an LDMatrix (ldmat(..., keep_on_device=True)): the run then reads the handle's device copy (hb_sbayes_run_ldm; a sparse
    or per-chromosome handle as the dense matrix with zeros where it stores nothing) on the handle's device."""
    return _run(False, sumstat, ldm, model, Pi, niter, nburn, thin, fold, windindx, vg, dfvg, s2vg, ve, dfve, s2ve, outfreq, threads,
                verbose, seed, device, store_alpha, log)


def SBayesS(sumstat, ldm, model, Pi, niter=50000, nburn=20000, thin=5, fold=None, windindx=None, vg=None, dfvg=None, s2vg=None,
            ve=None, dfve=None, s2ve=None, outfreq=100, threads=0, verbose=True, *, seed=666666, device=0, store_alpha=True, log=None):
    """SBayesS() of the reference (src/SBayesS.cpp): the sampler on a sparse LD matrix, SBayesD()'s arguments and results. ldm: an
    LDMatrix of any kind (ldmat(..., chisq=..., keep_on_device=True)) or a scipy sparse matrix, which must equal its transpose and
    is handed over as CSC with sorted indices (LDMatrix.from_scipy). The run walks the stored entries from the handle's device CSC
    (hb_sbayes_run_sparse): no m x m array exists on either side. Not SBayesD() with zeros — every marker has its own residual
    variance varediff[i] * Vg + Ve, varediff[i] the share of column i that is not stored, and BayesC / BayesCpi / BayesR effects
    with g^2 * vx > var(y) are redrawn."""
    own = None
    if not isinstance(ldm, LDMatrix):
        try:
            import scipy.sparse as sp
        except ImportError:
            sp = None
        if sp is None or not sp.issparse(ldm):
            raise ValueError("SBayesS needs an LDMatrix or a scipy sparse ldm (a dense array goes to SBayesD)")
        ldm = own = LDMatrix.from_scipy(ldm, device=device)
    try:
        return _run(True, sumstat, ldm, model, Pi, niter, nburn, thin, fold, windindx, vg, dfvg, s2vg, ve, dfve, s2ve, outfreq,
                    threads, verbose, seed, device, store_alpha, log)
    finally:
        if own is not None:
            own.close()


def _run(sparse, sumstat, ldm, model, Pi, niter, nburn, thin, fold, windindx, vg, dfvg, s2vg, ve, dfve, s2ve, outfreq, threads,
         verbose, seed, device, store_alpha, log):
    L = lib()
    ss = np.asfortranarray(sumstat, dtype=np.float64)
    handle = ldm if isinstance(ldm, LDMatrix) else None
    ld = None if handle is not None else np.asfortranarray(ldm, dtype=np.float64)
    if ss.ndim != 2 or ss.shape[1] != 4:
        raise ValueError("sumstat must have the four columns MAF, BETA, SE, NMISS")
    m = ss.shape[0]
    a = SBayesArgs()
    if handle is not None:
        a.m = m if handle.shape[0] == m else -1
        a.sumstat, a.ld_sumstat, a.ldm, a.ld_ldm = ss.ctypes.data, m, None, 0
        device = handle.device
    else:
        a.m = m if ld.ndim == 2 and ld.shape[0] == m and ld.shape[1] == m else -1   # -> "Number of SNPs not equals."
        a.sumstat, a.ld_sumstat, a.ldm, a.ld_ldm = ss.ctypes.data, m, ld.ctypes.data, (ld.shape[0] if ld.ndim == 2 else 0)
    a.model = model.encode()
    pv = np.ascontiguousarray(Pi, dtype=np.float64)
    a.Pi, a.n_pi = pv.ctypes.data, pv.size
    keep = [ss, ld, pv]
    if fold is not None:
        fv = np.ascontiguousarray(fold, dtype=np.float64)
        a.fold, a.n_fold = fv.ctypes.data, fv.size
        keep.append(fv)
    a.niter, a.nburn, a.thin = int(niter), int(nburn), int(thin)
    nw = 0
    if windindx is not None:
        w = np.ascontiguousarray(windindx, dtype=np.uint32)
        a.windindx, nw = w.ctypes.data, int(w.max())
        keep.append(w)
    for name, val in (("vg", vg), ("dfvg", dfvg), ("s2vg", s2vg), ("ve", ve), ("dfve", dfve), ("s2ve", s2ve)):
        if val is not None:
            setattr(a, "has_" + name, 1)
            setattr(a, name, float(val))
    a.outfreq, a.threads, a.verbose = int(outfreq), int(threads), int(bool(verbose))
    a.seed, a.device, a.store_alpha = int(seed), int(device), int(bool(store_alpha))
    if log is not None:
        cb = LOG_FN(lambda line, _u: log(line.decode("utf-8", "replace")))
        a.log = cb
        keep.append(cb)
    nrec = max((a.niter - a.nburn) // max(a.thin, 1), 0)
    o, res, mc = SBayesOut(), {}, {}

    def buf(d, name, shape):
        arr = np.zeros(shape, order="F")
        d[name] = arr
        return arr.ctypes.data

    mm = max(m, 1)
    o.alpha, o.pi, o.pip = buf(res, "alpha", mm), buf(res, "pi", pv.size), buf(res, "pip", mm)
    o.gwas = buf(res, "gwas", nw) if nw else None
    o.s_Vg, o.s_Ve, o.s_h2 = buf(mc, "Vg", (1, nrec)), buf(mc, "Ve", (1, nrec)), buf(mc, "h2", (1, nrec))
    o.s_alpha = buf(mc, "alpha", (mm, nrec)) if store_alpha else None
    o.s_pi = buf(mc, "pi", (pv.size, nrec))
    o.r_hat, o.g_last = buf(res, "r_hat", mm), buf(res, "g_last", mm)
    if handle is not None:
        check((L.hb_sbayes_run_sparse if sparse else L.hb_sbayes_run_ldm)(C.byref(a), handle._handle(), C.byref(o)))
    else:
        check(L.hb_sbayes_run(C.byref(a), C.byref(o)))
    for k in ("Vg", "Ve", "h2", "n_records", "nzct", "nw", "n", "count_y"):
        res[k] = getattr(o, k)
    res["MCMCsamples"] = mc
    res["timing"] = {"setup_seconds": o.setup_seconds, "loop_seconds": o.loop_seconds, "iters_done": o.iters_done, "mean_events": o.mean_events}
    del keep
    return res


def sbrm(sumstat, ldm, method="BayesB", map=None, Pi=None, fold=None, niter=None, nburn=None, thin=5, windsize=None, windnum=None,
         windindx=None, vg=None, dfvg=None, s2vg=None, ve=None, dfve=None, s2ve=None, printfreq=100, seed=666666, threads=4, verbose=True,
         sparse_ld=False, pve=False, **kw):
    """sbrm() of the reference (R/sbayes.r:101-239): the ldm type check (:126-132), GWAS windows cut from `map` by windsize /
    windnum (:135-187; res["gwas"] then carries WIND / CHR / NUM / START / END / WPPA like the reference's data frame, :231-234),
    defaults (:189-203), the column selection sumstat[, c(4, 5, 6, 8)] of the 8-column COJO table (:207), then SBayesD() — or, with
    sparse_ld=True and a scipy sparse `ldm` or an LDMatrix, SBayesS(), as :213 does for a dgCMatrix: .bed -> ldmat(chisq=...,
    keep_on_device=True) -> sbrm(sparse_ld=True) with no dense matrix on either side. Without sparse_ld a scipy sparse `ldm` is
    refused, and an LDMatrix runs through SBayesD() as the dense matrix. method = "CG" is refused here: its arm of sbrm() is
    sbrm_cg() (hibayes_amd/cg.py).
    `pve`: also return res["pve"] = ld_window_pve(...) — the variance explained by every window (windindx, or the windows cut by windsize /
    windnum; without either, by every marker) in every stored record of the effects (without store_alpha: in their posterior mean), as the
    quadratic form on the LD matrix the sampler ran on, relative to the sampler's own var(y) (src/SBayesD.cpp:93-115); see
    hibayes_amd.ld_window_pve. Where the windows were cut here, the table WIND / CHR / NUM / START / END comes with it. A host matrix is
    handed to the library once, as a handle, before the fit — it must equal its transpose in value bits, and one that does not is refused
    before anything is fitted. A sparse one is swept from that same handle; a dense one is swept as it was passed, and the handle holds the
    same values as CSC (12 B per stored entry in pinned memory: pass an LDMatrix from ldmat(keep_on_device=True) to avoid the copy)."""
    is_sparse = False
    try:
        import scipy.sparse as sp
        is_sparse = sp.issparse(ldm)
    except ImportError:
        pass
    if is_sparse and not sparse_ld:
        raise NotImplementedError("a sparse ldm (dgCMatrix: SBayesS, src/SBayesS.cpp) runs with sparse_ld=True; without it pass the dense LD matrix")
    if sparse_ld and not (is_sparse or isinstance(ldm, LDMatrix)):
        raise ValueError("sparse_ld=True needs a scipy sparse ldm or an LDMatrix")
    if not (is_sparse or isinstance(ldm, (np.ndarray, LDMatrix)) or hasattr(ldm, "__array__")):
        raise ValueError("Unrecognized type of ldm.")
    if method == "CG":
        raise NotImplementedError("method = 'CG' (conjgt_den / conjgt_spa) is not routed through sbrm(): call sbrm_cg()")
    windinfo = None
    if windsize is not None or windnum is not None:
        if method in ("BayesA", "BayesRR", "BayesL"):
            raise ValueError("can not implement GWAS analysis for the method: " + method)
        if map is None:
            raise ValueError("map information must be provided.")
        from .bayes import _map_columns
        from .windows import cutwind_by_bp, cutwind_by_num
        chrom, bp = _map_columns(map)          # R/sbayes.r:140-172, the same checks as ibrm()
        if windnum is not None:
            if len(chrom) < windnum:
                raise ValueError("Number of markers specified in a window is larger than the total number of markers.")
            windindx = cutwind_by_num(chrom, bp, windnum)
        else:
            if bp.max() < windsize:
                raise ValueError("Maximum of physical position is smaller than wind size.")
            windindx = cutwind_by_bp(chrom, bp, windsize)
        nwin = int(windindx.max())
        windinfo = {"WIND": ["wind%d" % (w + 1) for w in range(nwin)],
                    "CHR": [chrom[np.flatnonzero(windindx == w + 1)[0]] for w in range(nwin)],
                    "NUM": [int((windindx == w + 1).sum()) for w in range(nwin)],
                    "START": [float(bp[windindx == w + 1].min()) for w in range(nwin)],
                    "END": [float(bp[windindx == w + 1].max()) for w in range(nwin)]}
    if niter is None:
        niter = 50000 if method == "BayesR" else 20000
    if nburn is None:
        nburn = 30000 if method == "BayesR" else 12000
    if thin >= (niter - nburn):
        raise ValueError("bad setting for collecting frequency 'thin'.")
    if printfreq <= 0:
        verbose = False
    if Pi is None:
        if method == "BayesR":
            Pi = [0.95, 0.02, 0.02, 0.01]
            if fold is None:
                fold = [0, 0.0001, 0.001, 0.01]
        else:
            Pi = [0.95, 0.05]
    ss = np.asarray(sumstat, dtype=np.float64)
    if ss.ndim == 2 and ss.shape[1] >= 8:      # the COJO table (:207); a 4-column matrix is taken as MAF, BETA, SE, NMISS already
        ss = ss[:, [3, 4, 5, 7]]
    own = None
    try:
        pve_ld = ldm
        if pve and not isinstance(ldm, LDMatrix):
            # a host matrix becomes a handle once, BEFORE the fit: hb_ldm_from_csc refuses one that does not equal its transpose in value bits, and
            # that must not cost a finished chain. A sparse matrix is then swept from this handle (SBayesS() would make the same one for itself);
            # a dense one is swept by SBayesD() as it was passed and the handle, its CSC with the exact zeros dropped, serves the pass alone.
            import scipy.sparse as sp
            try:
                pve_ld = own = LDMatrix.from_scipy(ldm if is_sparse else sp.csc_matrix(np.asarray(ldm, dtype=np.float64)), device=kw.get("device", 0))
            except HibayesError as e:
                raise HibayesError(e.status, "sbrm(pve=True): %s (the variance explained is a quadratic form on the matrix; nothing was fitted)" % e) from None
            if sparse_ld:
                ldm = pve_ld
        res = (SBayesS if sparse_ld else SBayesD)(ss, ldm, method, Pi, niter=niter, nburn=nburn, thin=thin, fold=fold, windindx=windindx, vg=vg, dfvg=dfvg, s2vg=s2vg,
                      ve=ve, dfve=dfve, s2ve=s2ve, outfreq=printfreq, threads=threads, verbose=verbose, seed=seed, **kw)
        if pve:  # README item (8), on the matrix the sampler ran on; relative to the sampler's own var(y)
            from .pve import ld_window_pve, sbayes_vary
            samples = res["MCMCsamples"].get("alpha")
            res["pve"] = ld_window_pve(pve_ld, res["alpha"] if samples is None else samples, windindx, vary=sbayes_vary(ss, pve_ld.diagonal()))
            if windinfo is not None:
                res["pve"].update(windinfo)
    finally:
        if own is not None:
            own.close()
    if windinfo is not None:
        res["gwas"] = dict(windinfo, WPPA=res["gwas"])
    res["call"] = "b ~ nD^{-1}V alpha + e"
    res["model"] = "Summary level Bayesian model fit by [%s]" % method
    return res
