"""Plain-numpy restatement of the device's symmetric tridiagonal eigensolver (hibayes_amd/csrc/hb_stedc.hip): Cuppen's
divide and conquer with Gu-Eisenstat vectors, step by step as the library does it — the same scaling and splitting, the same merge tree
(hb_stedcplan.hpp), the same rank-one tearing, the same cyclic Jacobi on the leaves, dlaed2's deflation rule, roots held as (origin pole, offset)
with every difference formed as (d_j - d_origin) - tau, the Loewner product ratio by ratio. A helper: no tests here.

EPS_L is LAPACK's dlamch('Epsilon') = 2^-53: the thresholds below are dstedc's, dlaed2's and dlaed4's with that value."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
EPS_L = 0.5 * EPS
LEAF = 32          # STEDC_LEAF of hb_stedcplan.hpp
MAXIT = 100        # STEDC_MAXIT
SWEEPS = 30        # STEDC_SWEEPS


def tri(d, e):
    d, e = np.asarray(d, dtype=np.float64), np.asarray(e, dtype=np.float64)
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


def plan(n, splits, leaf=LEAF):
    """(leaves [(lo, hi)], merges [(lo, mid, hi, level)], levels): `splits` are the indices i whose e_i is negligible. A part of more than `leaf`
    rows is halved (the first half gets the smaller share); a merge's level is one more than the higher of its children's (leaves: 0)."""
    leaves, merges = [], []

    def build(lo, hi):
        if hi - lo <= leaf:
            leaves.append((lo, hi))
            return 0
        mid = lo + (hi - lo) // 2
        a = build(lo, mid)
        b = build(mid, hi)
        merges.append((lo, mid, hi, 1 + max(a, b)))
        return 1 + max(a, b)

    bounds = [0] + [int(i) + 1 for i in splits] + [n]
    levels = 0
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        levels = max(levels, build(lo, hi))
    return leaves, merges, levels


def round_robin(step):
    """the 16 disjoint pairs of step 0 .. 30 of a sweep over 32 indices"""
    pairs = [(31, step)]
    for k in range(1, 16):
        pairs.append(((step + k) % 31, (step - k) % 31))
    return [(min(p, q), max(p, q)) for p, q in pairs]


def jacobi_leaf(d, e):
    """Cyclic Jacobi on the leaf's block padded to 32 x 32 with zeros, 16 disjoint rotations per step. A rotation is skipped where |a_pq| <=
    EPS_L max|T| / 32. Returns (eigenvalues in the diagonal's order, V, sweeps)."""
    s = len(d)
    A = np.zeros((32, 32))
    A[:s, :s] = tri(d, e)
    V = np.eye(32)
    thr = EPS_L * float(np.max(np.abs(A))) / 32.0
    for sweep in range(SWEEPS):
        rotated = False
        for step in range(31):
            pr = round_robin(step)
            p, q = np.array([a for a, _ in pr]), np.array([b for _, b in pr])
            apq, app, aqq = A[p, q], A[p, p], A[q, q]
            on = np.abs(apq) > thr
            if not np.any(on):
                continue
            rotated = True
            safe = np.where(on, apq, 1.0)
            theta = (aqq - app) / (2.0 * safe)
            with np.errstate(over="ignore"):
                t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            r = np.sqrt(t * t + 1.0)
            c = 1.0 - t * t / (r * (1.0 + r))       # (not 1 / r: r's rounding above 1 is one-sided for small t and the columns' norms would drift)
            sn = t * c
            c, sn, t = np.where(on, c, 1.0), np.where(on, sn, 0.0), np.where(on, t, 0.0)
            cp, cq = A[:, p].copy(), A[:, q].copy()
            A[:, p], A[:, q] = c * cp - sn * cq, sn * cp + c * cq
            rp, rq = A[p, :].copy(), A[q, :].copy()
            A[p, :], A[q, :] = c[:, None] * rp - sn[:, None] * rq, sn[:, None] * rp + c[:, None] * rq
            vp, vq = V[:, p].copy(), V[:, q].copy()
            V[:, p], V[:, q] = c * vp - sn * vq, sn * vp + c * vq
            A[p, p] = np.where(on, app - t * apq, A[p, p])
            A[q, q] = np.where(on, aqq + t * apq, A[q, q])
            A[p, q] = np.where(on, 0.0, A[p, q])
            A[q, p] = np.where(on, 0.0, A[q, p])
        if not rotated:
            break
    else:
        raise RuntimeError("stedc: a leaf's Jacobi sweeps did not converge")
    return np.diag(A)[:s].copy(), V[:s, :s].copy(), sweep


def deflate(dd, zraw, rho0, k1):
    """dlaed2 on one merge: dd the children's eigenvalues by position (k1 of the first child), zraw the gathered rows, rho0 = |e_k|.
    Returns dict(rho, keep, defl, rots, typ, d, z): positions kept in ascending d, positions deflated, rotations (pj, nj, c, s) in order."""
    k = len(dd)
    dd = np.array(dd, dtype=np.float64)
    z = np.asarray(zraw, dtype=np.float64) / np.sqrt(2.0)
    rho = 2.0 * rho0
    typ = np.where(np.arange(k) < k1, 1, 3)
    order = np.argsort(dd, kind="stable")
    tol = 8.0 * EPS_L * max(float(np.max(np.abs(dd))), float(np.max(np.abs(z))))
    keep, defl, rots = [], [], []
    if rho * float(np.max(np.abs(z))) <= tol:
        return dict(rho=rho, keep=keep, defl=[int(j) for j in order], rots=rots, typ=typ, d=dd, z=z)
    pj = -1
    for j in order:
        j = int(j)
        if rho * abs(z[j]) <= tol:
            defl.append(j)
            continue
        if pj < 0:
            pj = j
            continue
        s, c = z[pj], z[j]
        tau = float(np.hypot(c, s))
        t = dd[j] - dd[pj]
        c, s = c / tau, -s / tau
        if abs(t * c * s) <= tol:
            z[j], z[pj] = tau, 0.0
            rots.append((pj, j, c, s))
            if typ[pj] != typ[j]:
                typ[j] = 2
            t2 = dd[pj] * c * c + dd[j] * s * s
            dd[j] = dd[pj] * s * s + dd[j] * c * c
            dd[pj] = t2
            defl.append(pj)
        else:
            keep.append(pj)
        pj = j
    keep.append(pj)
    return dict(rho=rho, keep=keep, defl=defl, rots=rots, typ=typ, d=dd, z=z)


def bisect(lo, hi):
    if hi <= 0.0:
        return -bisect(-hi, -lo)
    if lo == 0.0:
        return hi * 2.0 ** -10
    if hi > 16.0 * lo:
        return np.sqrt(lo) * np.sqrt(hi)
    return lo + 0.5 * (hi - lo)


def secular_root(i, dl, zl, rho):
    """Root i of 1 / rho + sum_j z_j^2 / (d_j - x) as (origin, tau, iterations): x = d[origin] + tau, the origin the nearer pole."""
    kk = len(dl)
    rhoinv = 1.0 / rho
    if kk == 1:
        return 0, rho * zl[0] * zl[0], 0
    last = i == kk - 1
    pa, pb = (i - 1, i) if last else (i, i + 1)

    def evaluate(org, tau):
        delta = (dl - dl[org]) - tau
        t = zl / delta
        lo_terms, hi_terms = zl[:pa + 1] * t[:pa + 1], zl[pb:] * t[pb:]
        psi = dpsi = 0.0
        for j in range(pa + 1):
            psi += lo_terms[j]
            dpsi += t[j] * t[j]
        phi = dphi = 0.0
        for j in range(kk - 1, pb - 1, -1):
            phi += hi_terms[j - pb]
            dphi += t[j] * t[j]
        err = 8.0 * (float(np.sum(np.abs(lo_terms))) + float(np.sum(np.abs(hi_terms)))) + 2.0 * rhoinv + abs(tau) * (dpsi + dphi)
        return rhoinv + psi + phi, psi, dpsi, phi, dphi, err, delta[pa], delta[pb]

    if last:
        org, lo, hi = i, 0.0, rho * float(np.sum(zl * zl))
        tau = hi
    else:
        half = 0.5 * (dl[i + 1] - dl[i])
        if evaluate(i, half)[0] >= 0.0:
            org, lo, hi, tau = i, 0.0, half, half
        else:
            org, lo, hi, tau = i + 1, -half, 0.0, -half
    for it in range(1, MAXIT + 1):
        w, psi, dpsi, phi, dphi, err, da, db = evaluate(org, tau)
        if abs(w) <= EPS_L * err:
            return org, tau, it
        if w < 0.0:
            lo = tau
        else:
            hi = tau
        mid = bisect(lo, hi)
        if not lo < mid < hi:                    # the bracket holds no number between its ends: the end that is no pole
            return org, (hi if lo == 0.0 else lo if hi == 0.0 else tau), it
        c = w - da * dpsi - db * dphi
        a = (da + db) * w - da * db * (dpsi + dphi)
        b = da * db * w
        with np.errstate(all="ignore"):
            if c == 0.0:
                r1 = r2 = b / a
            else:
                sq = np.sqrt(abs(a * a - 4.0 * b * c))
                if a >= 0.0:
                    r1, r2 = (a + sq) / (2.0 * c), 2.0 * b / (a + sq)
                else:
                    r1, r2 = (a - sq) / (2.0 * c), 2.0 * b / (a - sq)
        new = mid
        for eta in (r1, r2):
            if lo < tau + eta < hi:
                new = tau + eta
                break
        tau = new
    raise RuntimeError("stedc: the secular equation's iteration did not converge in %d steps" % MAXIT)


def merge(Zold, Znew, lam, lo, mid, hi, e_k, stats):
    """One merge, in place in lam[lo:hi]; Znew's block [lo:hi, lo:hi] is written."""
    k, k1 = hi - lo, mid - lo
    sgn = 1.0 if e_k >= 0 else -1.0
    zraw = np.concatenate([Zold[mid - 1, lo:mid], sgn * Zold[mid, mid:hi]])
    D = deflate(lam[lo:hi], zraw, abs(e_k), k1)
    for pj, nj, c, s in D["rots"]:
        x, y = Zold[lo:hi, lo + pj].copy(), Zold[lo:hi, lo + nj].copy()
        Zold[lo:hi, lo + pj], Zold[lo:hi, lo + nj] = c * x + s * y, c * y - s * x
    keep, defl, rho = D["keep"], D["defl"], D["rho"]
    kk = len(keep)
    stats["deflated"] = stats.get("deflated", 0) + len(defl)
    stats["rotations"] = stats.get("rotations", 0) + len(D["rots"])
    newlam = np.zeros(k)
    if kk:
        dl, zl = D["d"][keep], D["z"][keep]
        org, tau = np.zeros(kk, dtype=np.int64), np.zeros(kk)
        for i in range(kk):
            org[i], tau[i], it = secular_root(i, dl, zl, rho)
            stats["maxit"] = max(stats.get("maxit", 0), it)
        # Loewner: zhat_j^2 = -(d_j - x_j) prod_{i != j} (d_j - x_i) / (d_j - d_i), ratio by ratio
        zh = np.zeros(kk)
        for j in range(kk):
            wj = (dl[j] - dl[org[j]]) - tau[j]
            for i in range(kk):
                if i != j:
                    wj *= ((dl[j] - dl[org[i]]) - tau[i]) / (dl[j] - dl[i])
            zh[j] = np.copysign(np.sqrt(-wj), zl[j])
        U = np.zeros((kk, kk))
        for i in range(kk):
            u = zh / ((dl - dl[org[i]]) - tau[i])
            nrm = 0.0
            for j in range(kk):
                nrm += u[j] * u[j]
            U[:, i] = u * (1.0 / np.sqrt(nrm))
        src = np.array([lo + j for j in keep])
        typ = D["typ"][keep]
        top, bot = typ <= 2, typ >= 2
        Znew[lo:mid, lo:lo + kk] = Zold[lo:mid, src[top]] @ U[top, :]
        Znew[mid:hi, lo:lo + kk] = Zold[mid:hi, src[bot]] @ U[bot, :]
        newlam[:kk] = dl[org] + tau
    for t, j in enumerate(defl):
        Znew[lo:hi, lo + kk + t] = Zold[lo:hi, lo + j]
        newlam[kk + t] = D["d"][j]
    lam[lo:hi] = newlam


def stedc(d, e, stats=None):
    """(w ascending, Z) of tridiag(e, d, e)"""
    d = np.array(d, dtype=np.float64)
    n = d.size
    e = np.zeros(0) if n == 1 else np.array(e, dtype=np.float64)
    stats = {} if stats is None else stats
    sigma = max(float(np.max(np.abs(d))), float(np.max(np.abs(e), initial=0.0)))
    if sigma == 0.0:
        return np.zeros(n), np.eye(n)
    ds, es = d / sigma, e / sigma
    splits = [i for i in range(n - 1) if abs(es[i]) <= EPS_L * np.sqrt(abs(ds[i])) * np.sqrt(abs(ds[i + 1]))]
    leaves, merges, levels = plan(n, splits)
    dt = ds.copy()
    for lo, mid, hi, _ in merges:
        rho = abs(es[mid - 1])
        dt[mid - 1] -= rho
        dt[mid] -= rho
    lam, Z, W = np.zeros(n), np.zeros((n, n)), np.zeros((n, n))
    single = np.zeros(n, dtype=bool)
    for lo, hi in leaves:
        lam[lo:hi], Z[lo:hi, lo:hi], sw = jacobi_leaf(dt[lo:hi], es[lo:hi - 1])
        stats["sweeps"] = max(stats.get("sweeps", 0), sw)
        if hi - lo == 1 and (lo == 0 or lo - 1 in splits) and (hi == n or hi - 1 in splits):
            single[lo] = True
    blo, bhi = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)      # the finished node that holds each column
    for lo, hi in leaves:
        blo[lo:hi], bhi[lo:hi] = lo, hi
    for level in range(1, levels + 1):
        busy = np.zeros(n, dtype=bool)
        for lo, mid, hi, lv in merges:
            if lv == level:
                merge(Z, W, lam, lo, mid, hi, es[mid - 1], stats)
                busy[lo:hi] = True
                blo[lo:hi], bhi[lo:hi] = lo, hi
        for p in np.flatnonzero(~busy):          # a node that waits for a later level moves to the other buffer as it is
            W[blo[p]:bhi[p], p] = Z[blo[p]:bhi[p], p]
        Z, W = W, Z
    w = np.where(single, d, lam * sigma)      # a 1 x 1 part's eigenvalue is its entry, untouched by the scaling
    order = np.argsort(w, kind="stable")
    return w[order], np.asfortranarray(Z[:, order])


# ---------------------------------------------------------------------------------------------------------------------------------
# the matrices both test files use, each the smallest that forces its case, and the measures they are judged by
# ---------------------------------------------------------------------------------------------------------------------------------
def wilkinson(m):
    h = (m - 1) // 2
    return np.abs(np.arange(-h, h + 1)).astype(np.float64), np.ones(m - 1)


def glued(copies, glue, m=21):
    d, e = wilkinson(m)
    ee = []
    for i in range(copies):
        ee.extend(e)
        if i < copies - 1:
            ee.append(glue)
    return np.tile(d, copies), np.array(ee)


def toeplitz(n):
    return np.full(n, 2.0), np.full(n - 1, -1.0)


def toeplitz_values(n):
    return 2.0 - 2.0 * np.cos(np.arange(1, n + 1) * np.pi / (n + 1))


def random_pair(n, seed=None):
    rng = np.random.default_rng(n if seed is None else seed)
    return rng.normal(size=n), rng.normal(size=n - 1)


def matrices():
    out = {}
    for n in (1, 2, 3, 32, 33, 65, 129, 300, 513):
        out["random %d" % n] = random_pair(n)
    for n in (33, 257, 500):
        out["toeplitz %d" % n] = toeplitz(n)
    for m in (21, 201):
        out["wilkinson %d" % m] = wilkinson(m)
    out["glued 5 x 1e-8"] = glued(5, 1e-8)
    out["glued 10 x 1e-14"] = glued(10, 1e-14)
    d = np.logspace(0, -12, 200)
    out["graded"] = (d, 0.1 * np.sqrt(d[:-1] * d[1:]))
    rng = np.random.default_rng(5)
    out["clustered"] = (1.0 + 1e-15 * rng.normal(size=120), 1e-15 * rng.normal(size=119))
    # (there the split test already leaves no part longer than a leaf; with a subdiagonal well above eps the merges run and deflate nearly all)
    out["clustered 1e-12"] = (1.0 + 1e-15 * rng.normal(size=120), 1e-12 * rng.normal(size=119))
    d, e = random_pair(150, seed=6)
    e[40] = e[41] = 0.0
    e[100] = 1e-300
    out["splits"] = (d, e)
    d, e = random_pair(97, seed=7)
    out["scaled 2^500"] = (d * 2.0 ** 500, e * 2.0 ** 500)
    out["scaled 2^-500"] = (d * 2.0 ** -500, e * 2.0 ** -500)
    return out


MATRIX_NAMES = list(matrices())


def sterf(d, e):
    """the eigenvalues alone by LAPACK dsterf (root-free QL): the yardstick for `values`"""
    if len(d) == 1:
        return np.array(d, dtype=np.float64)
    from scipy.linalg.lapack import dsterf
    w, info = dsterf(np.asarray(d, dtype=np.float64), np.asarray(e, dtype=np.float64))
    assert info == 0
    return w


def lapack_dc(d, e):
    """LAPACK's divide and conquer on (d, e): dsytrd of a tridiagonal matrix is the identity, so numpy.linalg.eigh(tri(d, e)) is dstedc"""
    return np.linalg.eigh(tri(d, e))


def measures(d, e, w, Z):
    """res = max|T Z - Z diag(w)| / ||T||_2, orth = max|Z'Z - I|, values = max|w - w_sterf| / max|w_sterf|, in units of EPS"""
    T, n = tri(d, e), len(d)
    ws = sterf(d, e)
    scale = max(float(np.max(np.abs(ws))), 1e-300)
    return {"res": float(np.max(np.abs(T @ Z - Z * w[None, :]))) / scale / EPS, "orth": float(np.max(np.abs(Z.T @ Z - np.eye(n)))) / EPS,
            "values": float(np.max(np.abs(w - ws))) / scale / EPS}
