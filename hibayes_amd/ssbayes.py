"""The single-step model's front end (reference R/ssbayes.r:115-351, make_ped / make_Ainv src/rm.cpp:56-206).

`make_ped()`, `make_Ainv()`  the pedigree in parents-first order and the inverse of its numerator relationship matrix
`ssbrm_prepare()`            everything ssbrm() does before the sampler, on the host (set-up, once): no device needed
`ssbrm()`                    the fit: Bayes() on fp64 columns with the epsilon block on the device (hb_epsl.hip), then the GEBV bookkeeping
`epsl_descriptor()`          a scipy sparse matrix or an (indptr, indices, data) triple as the library's hb_epsl_gi
"""
import ctypes as ct
import warnings

import numpy as np

from . import _lib
from .bayes import METHODS, _RAND, Bayes, _column, _first_column_name, _isna, _map_columns, _model_matrix

NA_POOL = frozenset(["NA", "Na", ".", "-", "NaN", "NAN", "nan", "na", "N/A", "n/a", "<NA>"])  # src/rm.cpp:64
SS_METHODS = tuple(m for m in METHODS if m != "BSLMM")  # R/ssbayes.r:122


def epsl_descriptor(Gi, index):
    """(hb_epsl_gi, index as uint32, the arrays both point into). A scipy sparse matrix is brought to canonical CSC (duplicates summed, row
    indices sorted); a triple (indptr, indices, data) is passed on as it is — the library validates it."""
    if isinstance(Gi, (tuple, list)) and len(Gi) == 3:
        indptr, indices, data = Gi
    else:
        import scipy.sparse as sp
        if not sp.issparse(Gi):
            Gi = sp.csc_matrix(np.asarray(Gi, dtype=np.float64))
        if Gi.shape[0] != Gi.shape[1]:
            raise _lib.HibayesError(1, "variance-covariance matrix should be in square.")
        G = sp.csc_matrix(Gi, dtype=np.float64, copy=True)
        G.sum_duplicates()
        G.sort_indices()
        indptr, indices, data = G.indptr, G.indices, G.data
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    data = np.ascontiguousarray(data, dtype=np.float64)
    idx = np.asarray(index).ravel()
    if idx.size and (np.any(idx < 0) or np.any(idx > 0xFFFFFFFF)):
        raise _lib.HibayesError(1, "epsl_index: an index is outside 1 .. q (the columns of epsl_Gi)")
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    if indptr.size < 2 or indices.size != data.size or indices.size < int(indptr[-1]):
        raise _lib.HibayesError(1, "epsl_Gi: an empty descriptor (q, indptr, indices, data)")
    gi = _lib.EpslGi(indptr.size - 1, idx.size, indptr.ctypes.data, indices.ctypes.data, data.ctypes.data)
    return gi, idx, (indptr, indices, data)


def epsl_check(Gi, index, n):
    """The library's validation of the block's arguments alone (no device): raises HibayesError with its text."""
    gi, idx, keep = epsl_descriptor(Gi, index)
    _lib.check(_lib.lib().hb_epsl_check(ct.byref(gi), idx.ctypes.data, int(n)))
    del keep


def epsl_plan(Gi, sched_mode=0, row_mode=0):
    """The schedule of the Gibbs pass for a pattern (hb_epslplan.hpp; no device): dict of level, rows, steps (level, lane0, nlane, wave0, nwave),
    launches (kind, s0, s1), levels, max_col."""
    gi, _idx, keep = epsl_descriptor(Gi, [])
    q = gi.q
    level, rows = np.zeros(q, dtype=np.int32), np.zeros(q, dtype=np.int32)
    steps, launches, cnt = np.zeros((q, 5), dtype=np.int32), np.zeros((q, 3), dtype=np.int32), np.zeros(4, dtype=np.int32)
    _lib.check(_lib.lib().hb_epsl_plan(q, keep[0].ctypes.data, keep[1].ctypes.data, int(sched_mode), int(row_mode), level.ctypes.data, rows.ctypes.data,
                                       steps.ctypes.data, launches.ctypes.data, cnt.ctypes.data))
    return {"level": level, "rows": rows, "steps": steps[:cnt[0]].copy(), "launches": launches[:cnt[1]].copy(), "levels": int(cnt[2]),
            "max_col": int(cnt[3])}


# --------------------------------------------------------------------------------------------
# make_ped(), src/rm.cpp:56-170
# --------------------------------------------------------------------------------------------
def make_ped(id, sire, dam, verbose=False):
    """The pedigree in an order in which parents come before their offspring. Rows whose id is an NA token are dropped, NA parents become
    "0", parents that have no row of their own are added as founders where they are first met. Returns (ids, s, d): s / d are the 1-based
    positions of sire and dam in ids, 0 = unknown."""
    pid, ps, pd = [], [], []
    for p, s, d in zip(id, sire, dam):
        p, s, d = str(p), str(s), str(d)
        if p in NA_POOL:
            continue
        pid.append(p)
        ps.append("0" if s in NA_POOL else s)
        pd.append("0" if d in NA_POOL else d)
    ped_1 = set(pid)
    if len(ped_1) != len(pid):
        raise ValueError("repeated records are not allowed in the first column of pedigree file.")
    n = len(pid)
    todo = [True] * n
    idset = {"0"}
    ids, ss, dd = [], [], []

    def add(i_, s_, d_):
        idset.add(i_)
        ids.append(i_)
        ss.append(s_)
        dd.append(d_)

    for i in range(n):
        if ps[i] == "0" and pd[i] == "0":
            add(pid[i], "0", "0")
            todo[i] = False
        else:
            for par in (ps[i], pd[i]):
                if par != "0" and par not in ped_1 and par not in idset:
                    add(par, "0", "0")
    left = sum(todo)
    while left:
        loopin = 0
        for i in range(n):
            if todo[i] and ps[i] in idset and pd[i] in idset:
                add(pid[i], ps[i], pd[i])
                todo[i] = False
                loopin += 1
        if not loopin:
            for i in range(n):
                if todo[i] and (ps[i] in idset or pd[i] in idset):
                    add(pid[i], ps[i], pd[i])
                    todo[i] = False
                    loopin += 1
        if not loopin:
            for i in range(n):
                if todo[i]:
                    add(pid[i], ps[i], pd[i])
                    todo[i] = False
        left = sum(todo)
    if not ids:
        raise ValueError("no individuals detected;")
    if verbose:
        print("%d unique individuals have been detected in pedigree" % len(ids))
    pos = {"0": 0}
    for j, v in enumerate(ids):
        pos.setdefault(v, j + 1)
    return ids, [pos[v] for v in ss], [pos[v] for v in dd]


# --------------------------------------------------------------------------------------------
# make_Ainv(), src/rm.cpp:173-206
# --------------------------------------------------------------------------------------------
def make_Ainv(s, d, one_parent="reference"):
    """Henderson's rules for the inverse of the numerator relationship matrix without inbreeding, as a scipy CSC matrix: 1 for a founder;
    2 / -1 / 0.5 for an individual with both parents known.

    `one_parent`: the reference writes the one-known-parent contributions as the C++ expressions 4/3, 2/3 and 1/3 — integer divisions, 1, 0
    and 0 — so it adds 1 to the individual's diagonal and nothing else. "reference" (default) reproduces that, so that ssbrm() fits the model
    the reference fits; "henderson" gives the rule itself: 4/3 on the diagonal, -2/3 against the parent, 1/3 on the parent's diagonal.
    (The contributions are added up; the reference SETS a founder's diagonal to 1, the same thing wherever parents precede their offspring,
    which is the order make_ped() returns.)"""
    import scipy.sparse as sp
    if one_parent not in ("reference", "henderson"):
        raise ValueError("make_Ainv: one_parent must be \"reference\" or \"henderson\", not %r" % (one_parent,))
    s = np.asarray(s, dtype=np.int64).ravel()
    d = np.asarray(d, dtype=np.int64).ravel()
    n = s.size
    if d.size != n or np.any(s < 0) or np.any(d < 0) or np.any(s > n) or np.any(d > n):
        raise ValueError("make_Ainv: s and d hold positions 1 .. n, 0 for an unknown parent")
    x = np.arange(n)
    R, Cc, V = [], [], []

    def put(r, c, v):
        R.append(np.asarray(r))
        Cc.append(np.asarray(c))
        V.append(np.full(len(r), v, dtype=np.float64))

    f = x[(s == 0) & (d == 0)]
    put(f, f, 1.0)
    b = x[(s > 0) & (d > 0)]
    sb, db = s[b] - 1, d[b] - 1
    put(b, b, 2.0)
    put(b, sb, -1.0), put(sb, b, -1.0)
    put(db, b, -1.0), put(b, db, -1.0)
    put(sb, sb, 0.5)
    diff = sb != db
    put(sb[diff], db[diff], 0.5), put(db[diff], sb[diff], 0.5)
    put(sb[~diff], sb[~diff], 0.5)  # (sire == dam: the reference writes the same element once, 0.5 more)
    put(db, db, 0.5)
    for par in (s, d):
        o = x[(par > 0) & ((s == 0) | (d == 0))]
        po = par[o] - 1
        if one_parent == "reference":
            put(o, o, 1.0)
        else:
            put(o, o, 4.0 / 3.0)
            put(o, po, -2.0 / 3.0), put(po, o, -2.0 / 3.0)
            put(po, po, 1.0 / 3.0)
    A = sp.coo_matrix((np.concatenate(V), (np.concatenate(R), np.concatenate(Cc))), shape=(n, n)).tocsc()
    A.sum_duplicates()
    A.sort_indices()
    return A


# --------------------------------------------------------------------------------------------
# ssbrm(), R/ssbayes.r:115-351
# --------------------------------------------------------------------------------------------
def ssbrm_prepare(formula, data=None, M=None, M_id=None, pedigree=None, maf=0.01, one_parent="reference", chunk=512, verbose=False, *,
                  impute="host", impute_tol=1e-12, device=0):
    """ssbrm() up to the call of Bayes() (R/ssbayes.r:225-319): the formula, the ids, the pedigree, A^-1, the imputation
    Mn = solve(A^-1_nn, -A^-1_ng M) in chunks of `chunk` marker columns, Jn, and the stacking — genotyped records first, then the
    non-genotyped ones. Returns a dict.
    `impute="host"` (default): one sparse LU factor on the host; nothing touches a device. `impute="device"`: a batched conjugate-gradient
    solve on `device` (impute_device(), hb_impute.hip) to the relative residual `impute_tol`, J as one more column of the last chunk — no
    factor, so it reaches pedigrees whose factor does not fit; the dict then also has "impute_stats"."""
    import re
    if impute not in ("host", "device"):
        raise ValueError("impute must be \"host\" or \"device\", not %r" % (impute,))
    import scipy.sparse as sp
    from scipy.sparse.linalg import splu
    if data is None:
        raise ValueError("no data assigned.")
    names_all = list(data.columns) if hasattr(data, "columns") else list(data)
    if len(names_all) < 2:
        raise ValueError("the first column in 'data' should be the individual id.")
    if M is None:
        raise ValueError("no genotype data.")
    if M_id is None:
        raise ValueError("please assign the individuals id to 'M.id'.")
    M = np.array(M, dtype=np.float64, order="F")  # (a copy: the MAF filter below writes into it)
    M_id = [str(v) for v in M_id]
    if len(M_id) != M.shape[0]:
        raise ValueError("number of individuals mismatched in 'M' and 'M.id'.")
    if pedigree is None:
        raise ValueError("pedigree should be provided for single-step bayesian model.")

    # ---- the formula, :225-258 (ibrm()'s conventions) ----
    lhs, rhs = [t.strip() for t in formula.split("~", 1)]
    rand_terms = _RAND.findall(rhs)
    fixed = _RAND.sub("", rhs)
    fixed_terms = [t.strip() for t in re.split(r"\+", fixed) if t.strip() and t.strip() != "1"]
    for t in fixed_terms:
        if "|" in t or "(" in t:
            raise ValueError("Invalid random effects expression '%s',\n  it should be in the format "
                             "'(1 | x)' or '+ (1 | x1:x2:...:xn)'." % t)
        if ":" in t or "*" in t:
            raise NotImplementedError("interaction terms in the fixed part are not supported")
    idcol = _first_column_name(data)
    names = set([lhs] + fixed_terms + [c for r in rand_terms for c in r.split(":")])
    cols = {nm: _column(data, nm) for nm in names}
    ids_all = [str(v) for v in _column(data, idcol)]
    nrow = len(ids_all)
    yNA = np.zeros(nrow, dtype=bool)
    for nm in names:
        yNA |= np.array([_isna(v) for v in cols[nm]])
    if yNA.all():
        raise ValueError("no effective data left.")

    # ---- MAF, :263-264 ----
    p = M.mean(axis=0) / 2.0
    p = np.minimum(p, 1.0 - p)
    M[:, p < maf] = 0.0

    # ---- ids, :265-289 ----
    ped = np.asarray(pedigree.values if hasattr(pedigree, "values") else pedigree, dtype=object)
    if ped.ndim != 2 or ped.shape[1] != 3:
        raise ValueError("3 columns ('id', 'sir', 'dam') are required in pedigree.")
    ped = [[str(v) for v in ped[:, j]] for j in range(3)]
    ped_set = set(ped[0]) | set(ped[1]) | set(ped[2])
    msub = [v for v in M_id if v not in ped_set]
    if len(msub) == len(M_id):
        raise ValueError("no shared individuals between 'M.id' and 'pedigree'.")
    if msub:
        ped[0] += msub
        ped[1] += ["0"] * len(msub)
        ped[2] += ["0"] * len(msub)
        ped_set |= set(msub)
    M_set = set(M_id)
    if all(v in M_set for v in ped_set):
        raise ValueError("all individuals have been genotyped, no necessaries to fit single-step bayes model.")
    y_id = [ids_all[i] for i in range(nrow) if not yNA[i]]
    ysub = [v for v in y_id if v not in ped_set]
    if len(ysub) == len(y_id):
        raise ValueError("no shared individuals between 'data' and 'pedigree'.")
    if ysub:  # (they are in neither block of the stacking below, :310-313: they leave the fit)
        if verbose:
            print("%d individuals cannot be found in genotype or pedigree" % len(ysub))
        drop = set(ysub)
        for i in range(nrow):
            if ids_all[i] in drop:
                yNA[i] = True
    rows = np.flatnonzero(~yNA)
    y_id = [ids_all[i] for i in rows]
    y = np.array([float(cols[lhs][i]) for i in rows])
    Xfix, fixed_names = _model_matrix(cols, fixed_terms, rows)
    R = None
    if rand_terms:
        R = np.array([[":".join(str(cols[c][i]) for c in r.split(":")) for i in rows] for r in rand_terms], dtype=object).T

    # ---- pedigree, A^-1 and the imputation, :291-309 ----
    ped_id, s, d = make_ped(ped[0], ped[1], ped[2], verbose)
    Ai = make_Ainv(s, d, one_parent)
    pos = {}
    for j, v in enumerate(ped_id):
        pos.setdefault(v, j)
    g_indx = np.array([pos[v] for v in M_id], dtype=np.int64)
    is_g = np.zeros(len(ped_id), dtype=bool)
    is_g[g_indx] = True
    n_indx = np.flatnonzero(~is_g)
    Mn_id = [ped_id[j] for j in n_indx]
    Ai = Ai.tocsr()
    Ai_nn = Ai[n_indx][:, n_indx].tocsc()
    Ai_ng = Ai[n_indx][:, g_indx].tocsr()
    Ai_nn.sum_duplicates()
    Ai_nn.sort_indices()
    import time
    t0 = time.perf_counter()
    m = M.shape[1]
    Mn = np.empty((len(Mn_id), m), dtype=np.float64, order="F")
    J = np.full(len(M_id), -1.0)
    impute_stats = None
    if impute == "host":
        # (A^-1_nn is symmetric positive definite: a minimum-degree ordering of its own pattern and pivots on the diagonal keep the factor sparse)
        lu = splu(Ai_nn, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
        for c0 in range(0, m, int(chunk)):
            c1 = min(m, c0 + int(chunk))
            Mn[:, c0:c1] = lu.solve(-(Ai_ng @ M[:, c0:c1]))
        Jn = lu.solve(-(Ai_ng @ J))
    else:
        from .impute import ImputeSystem
        ck = max(1, int(chunk))
        starts = list(range(0, m, ck)) or [0]
        with ImputeSystem(Ai_nn, Ai_ng, device) as S:
            for c0 in starts:
                c1 = min(m, c0 + ck)
                if c0 != starts[-1]:
                    _, st = S.solve(M[:, c0:c1], impute_tol, out=Mn[:, c0:c1])
                else:  # the last chunk takes J with it
                    last, st = S.solve(np.asfortranarray(np.column_stack([M[:, c0:c1], J])), impute_tol)
                    Mn[:, c0:c1] = last[:, :c1 - c0]
                    Jn = np.ascontiguousarray(last[:, c1 - c0])
                if impute_stats is None:
                    impute_stats = st
                else:
                    for f in ("iterations", "max_residual", "product_seconds"):
                        impute_stats[f] = max(impute_stats[f], st[f])
                    for f in ("blocks", "looks", "seconds"):
                        impute_stats[f] += st[f]
    impute_seconds = time.perf_counter() - t0

    # ---- the stacking, :310-319 ----
    y_set = set(y_id)
    g_rec = [i for i, v in enumerate(M_id) if v in y_set]
    n_rec = [i for i, v in enumerate(Mn_id) if v in y_set]
    comb = [M_id[i] for i in g_rec] + [Mn_id[i] for i in n_rec]
    ypos = {}
    for i, v in enumerate(y_id):
        ypos.setdefault(v, i)
    y_indx = np.array([ypos[v] for v in comb], dtype=np.int64)
    return {
        "y": y[y_indx], "X": None if Xfix is None else np.asfortranarray(Xfix[y_indx]), "R": None if R is None else R[y_indx],
        "y_M": np.asfortranarray(np.vstack([M[g_rec], Mn[n_rec]])), "y_J": np.concatenate([J[g_rec], Jn[n_rec]]),
        "Ai_nn": Ai_nn, "Ai_ng": Ai_ng, "index": np.array(n_rec, dtype=np.int64) + 1,
        "M": M, "Mn": Mn, "J": J, "Jn": Jn, "M_id": M_id, "Mn_id": Mn_id, "y_id": y_id, "y_id_comb": comb, "y_indx": y_indx,
        "n_genotyped_records": len(g_rec), "n_other_records": len(n_rec), "fixed_names": fixed_names, "rand_terms": list(rand_terms),
        "lhs": lhs, "rhs": rhs, "impute_seconds": impute_seconds,
        **({} if impute_stats is None else {"impute_stats": impute_stats}),
    }


def ssbrm(formula, data=None, M=None, M_id=None, pedigree=None, method="BayesCpi", map=None, Pi=None, fold=None, niter=None, nburn=None, thin=5,
          windsize=None, windnum=None, maf=0.01, dfvr=None, s2vr=None, vg=None, dfvg=None, s2vg=None, ve=None, dfve=None, s2ve=None,
          printfreq=100, seed=666666, threads=4, verbose=True, *, windindx=None, device=0, panel=0, store_alpha=True, store_epsilon=True,
          gebv_samples=False, one_parent="reference", chunk=512, impute="host", impute_tol=1e-12, pve=False):
    """Mirror of ssbrm() (reference R/ssbayes.r:115-351), with ibrm()'s conventions for `formula`, `data` and the keyword extras: the
    single-step model for a population of which only a part is genotyped. `pedigree`: three columns (id, sire, dam). The non-genotyped
    individuals' genotypes are imputed from the pedigree in the set-up — on the host through a sparse factor, or with `impute="device"` by a
    batched conjugate-gradient solve on the device (ssbrm_prepare()) —, the fit runs on the fp64 resident layout with the epsilon
    block — J, the Gibbs pass over the non-genotyped individuals, the variance of epsilon — on the device.
    Returns Bayes()'s fields plus Veps, J, epsilon {"id", "epsilon"}, g {"id", "gebv"} over the genotyped, then the non-genotyped
    individuals (the linear form of :325 applied to the posterior means; `gebv_samples=True` also returns the full MCMCsamples["g"]) and
    e {"id", "e"}. `one_parent`: make_Ainv()'s — the default reproduces the reference's A^-1.
    `pve`: also return res["pve"] = window_pve(...) — the variance explained by every window (or, without windows, by every marker) in every
    stored record of the effects (without store_alpha: in their posterior mean) over all individuals, genotyped and imputed, relative to
    var(y) of the fit; see hibayes_amd.window_pve. Where the windows were cut here, their table comes with it."""
    if method not in SS_METHODS:
        raise ValueError("'arg' should be one of " + ", ".join(SS_METHODS))
    windinfo = None
    if (windsize is not None or windnum is not None) and windindx is None:
        if method in ("BayesA", "BayesRR", "BayesL"):
            raise ValueError("can not implement GWAS analysis for the method: " + method)
        chrom, bp = _map_columns(map)
        from .windows import cutwind_by_bp, cutwind_by_num
        if windnum is not None:
            if len(chrom) < windnum:
                raise ValueError("Number of markers specified in a window is larger than the total number of markers.")
            windindx = cutwind_by_num(chrom, bp, windnum)
        else:
            if bp.max() < windsize:
                raise ValueError("Maximum of physical position is smaller than wind size.")
            windindx = cutwind_by_bp(chrom, bp, windsize)
        # the windows' table, R/ssbayes.r:200-204: chromosome, markers and range of every window
        w = np.asarray(windindx, dtype=np.int64)
        wins = range(1, int(w.max()) + 1)
        windinfo = {"Wind": ["wind%d" % k for k in wins], "Chr": [chrom[w == k][0] for k in wins], "N": [int(np.sum(w == k)) for k in wins],
                    "Start": [float(bp[w == k].min()) for k in wins], "End": [float(bp[w == k].max()) for k in wins]}
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
    pr = ssbrm_prepare(formula, data, M, M_id, pedigree, maf=maf, one_parent=one_parent, chunk=chunk, verbose=verbose, impute=impute,
                       impute_tol=impute_tol, device=device)
    has_eps = pr["n_other_records"] > 0
    kw = dict(y=pr["y"], X=pr["y_M"], model=method, Pi=Pi, fold=fold, C_=pr["X"], R=pr["R"], niter=niter, nburn=nburn, thin=thin, windindx=windindx,
              dfvr=dfvr, s2vr=s2vr, vg=vg, dfvg=dfvg, s2vg=s2vg, ve=ve, dfve=dfve, s2ve=s2ve, outfreq=printfreq, threads=threads, verbose=verbose,
              seed=seed, device=device, panel=panel, store_alpha=store_alpha, genotype_bits=64)
    if has_eps:
        res = Bayes(epsl_y_J=pr["y_J"], epsl_Gi=pr["Ai_nn"], epsl_index=pr["index"], store_epsilon=store_epsilon, **kw)
    else:  # (:329: the reference's Bayes() skips the block when no record belongs to it)
        warnings.warn("all phenotypic individuals have genotype information, thus can't fit imputation errors.")
        res = Bayes(**kw)
    if "beta" in res:
        res["beta_names"] = pr["fixed_names"]
    if "Vr" in res:
        res["Vr_names"] = pr["rand_terms"]
    # GEBV, :325 and :337: g = [J; Jn] J + [M alpha; Mn alpha + epsilon], on the device (hb_ctx_matmul on the fp64 columns)
    from .engine import Context
    Mall = np.vstack([pr["M"], pr["Mn"]])
    Jall = np.concatenate([pr["J"], pr["Jn"]])
    ng = len(pr["M_id"])
    with Context(Mall.shape[0], Mall.shape[1], device=device, panel=panel) as cg:
        cg.upload_real(Mall)
        gebv = cg.matmul(res["alpha"])[:, 0]
        if has_eps:
            gebv = gebv + Jall * res["J"]
            gebv[ng:] += res["epsilon"]
        mc = res["MCMCsamples"]
        if gebv_samples and "alpha" in mc and (not has_eps or "epsilon" in mc):
            gs = cg.matmul(mc["alpha"])
            if has_eps:
                gs = gs + np.outer(Jall, mc["J"].ravel())
                gs[ng:] += mc["epsilon"]
            mc["g"] = gs
        if pve:  # README item (8), on the context that holds all individuals; relative to var(y) of the fit
            from .pve import window_pve
            samples = mc.get("alpha") if store_alpha else None
            res["pve"] = window_pve(cg, res["alpha"] if samples is None else samples, windindx, vary=float(np.var(pr["y"], ddof=1)))
            if windinfo is not None:
                res["pve"].update(windinfo)
    if has_eps:
        res["epsilon"] = {"id": list(pr["Mn_id"]), "epsilon": res["epsilon"]}
    res["u_last"] = res["g"]
    res["g"] = {"id": list(pr["M_id"]) + list(pr["Mn_id"]), "gebv": gebv}
    e = np.full(len(pr["y_id"]), np.nan)
    e[pr["y_indx"]] = res["e"]
    res["e"] = {"id": list(pr["y_id"]), "e": e}
    if windinfo is not None and "gwas" in res:  # :343-346
        res["gwas"] = dict(windinfo, WPPA=res["gwas"])
    res["call"] = "%s ~ %s + J + M[pedigree]" % (pr["lhs"], pr["rhs"])
    res["model"] = "Single-step Bayesian model fit by [%s]" % method
    res["timing"]["impute_seconds"] = pr["impute_seconds"]
    if "impute_stats" in pr:
        res["timing"]["impute_stats"] = pr["impute_stats"]
    return res
