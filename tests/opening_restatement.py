"""Plain numpy restatements of what the chain kernels of a sweep are handed at their opening (tests/test_opening_host.py tests them on the
CPU for their own properties, tests/test_gpu_opening.py compares the device's arrays with them):

  cert_reference     the group chain's certificate (hb_gram.hip: k_g16_ab, k_gcmax): G[k][j] = ga[k] gB[j] + c[k][j], |c[k][j]| <= gcmax[k]
  filter_reference   the opening filter and the 16-byte opening records (hb_chain_persist.hpp: k_hotlist)
  hotlist_reference  the row-cache lists of the per-panel chain (k_hotlist), with check_lists(), what the chain needs of ANY such list

Everything is exact integer or IEEE arithmetic: the comparisons are equalities."""
import numpy as np

INT32_MAX = 2147483647
HS = 256            # ints per panel in the packed list: four header words, then up to LIST_MAX markers
LIST_MAX = HS - 4


def padded(X, P):
    """X (n x m) as int64 with zero columns up to whole panels"""
    n, m = X.shape
    m_pad = -(-m // P) * P
    Xp = np.zeros((n, m_pad), dtype=np.int64)
    Xp[:, :m] = X
    return Xp


def cross(A, B):
    """A' B of two integer matrices, exactly: every partial sum stays far below 2^53, so the fp64 product is the integer one"""
    assert float(np.abs(A).max(initial=0)) * float(np.abs(B).max(initial=0)) * A.shape[0] < 2.0 ** 53
    return np.rint(A.astype(np.float64).T @ B.astype(np.float64)).astype(np.int64)


def cert_reference(X, P, Lg, n):
    """(ga, gB, gcmax), m_pad int64 each, of the genotypes X (n x m, any integer coding) at panel P over a band of Lg blocks.
    s = column sums; ga = rint(s / 256), gB = rint(s 256 / n) in fp64, ties to even (the kernel's operations one for one: s 256 is exact);
    gcmax[k] = max |G[k][j] - ga[k] gB[j]| in int64 over the columns j of the panels p(k) .. p(k) + Lg that exist, k itself left out,
    clamped at INT32_MAX."""
    Xp = padded(X, P)
    m_pad = Xp.shape[1]
    s = Xp.sum(axis=0).astype(np.float64)
    ga = np.rint(s / 256.0).astype(np.int64)
    gB = np.rint(s * 256.0 / float(n)).astype(np.int64)
    gcmax = np.zeros(m_pad, dtype=np.int64)
    for p in range(m_pad // P):
        j0, j1 = p * P, min(m_pad, (p + Lg + 1) * P)
        c = np.abs(cross(Xp[:, j0:j0 + P], Xp[:, j0:j1]) - ga[j0:j0 + P, None] * gB[None, j0:j1])
        c[np.arange(P), np.arange(P)] = 0          # x_k . x_k is no pair
        gcmax[j0:j0 + P] = c.max(axis=1)
    return ga, gB, np.minimum(gcmax, INT32_MAX)


def float_below(x):
    """the largest float not above each double of x (+inf stays, a double beyond the floats' range gives the largest float)"""
    with np.errstate(over="ignore"):
        f = np.asarray(x, dtype=np.float64).astype(np.float32)
    up = f.astype(np.float64) > x
    return np.where(up, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def filter_reference(thr0, vx, g, candf, gB):
    """(thr0f, opn): the filter word per marker — NaN monomorphic (vx == 0), -inf in the model (g != 0), else the entry threshold thr0 rounded
    DOWN to float — and the records as m x 4 int32: the candidate threshold (-1 in the model, else candf * (double) word, NaN for a monomorphic
    marker) as a double, low word first, the filter word, gB."""
    thr0, vx, g = (np.asarray(a, dtype=np.float64) for a in (thr0, vx, g))
    f = float_below(thr0)
    f = np.where(g != 0.0, np.float32(-np.inf), f)
    f = np.where(vx == 0.0, np.float32(np.nan), f).astype(np.float32)
    with np.errstate(invalid="ignore"):
        thc = np.where(np.isneginf(f), -1.0, float(candf) * f.astype(np.float64))
    opn = np.zeros((thr0.size, 4), dtype=np.int32)
    opn[:, 0:2] = np.ascontiguousarray(thc).view(np.int32).reshape(-1, 2)
    opn[:, 2] = f.view(np.int32)
    opn[:, 3] = gB
    return f, opn


def hot_flags(vx, g, thr0, xpx, kappa, vare):
    """(active, hot) as k_hotlist decides them: polymorphic; and in the model or predicted to enter, thr0 <= kappa xpx vare"""
    active = np.asarray(vx) != 0.0
    return active, active & ((np.asarray(g) != 0.0) | (np.asarray(thr0) <= kappa * np.asarray(xpx) * vare))


def _geometry(P):
    U = max(P >> 6, 1)                 # a whole row, in units of 64 ints
    return U, U >> 1, P == 512         # ... a half row; panel 512 keeps a row of the second half as its second piece alone


def hotlist_reference(active, hot, P, nslot):
    """(slot_of, lists, head) of the flags active / hot (m_pad each, whole panels): slot_of[j] = where marker j's Gram row sits in the row cache
    of nslot rows, in units of 64 ints (-1: no place, -2: monomorphic); lists[p] = the hot markers of panel p in marker order, LIST_MAX at the
    most; head[p] = [rows that fit, rows listed, whole rows among those that fit, the shift in pieces].
    The layout, as the comment above k_hotlist has it, walked with a cursor: whole rows first — at panel 512 the hot rows of the first half, else
    all of them —, then the second pieces of the second half's rows, each with its base one piece before the piece; when no whole row precedes
    them the cursor starts one piece in, so that no base is negative. A row that ends beyond the cache has no place; the cursor moves on."""
    active, hot = np.asarray(active, dtype=bool), np.asarray(hot, dtype=bool)
    U, Uh, tri = _geometry(P)
    cap = nslot * U
    npan = active.size // P
    slot_of = np.where(active, -1, -2).astype(np.int32)
    lists, head = [], np.zeros((npan, 4), dtype=np.int32)
    for p in range(npan):
        hp = np.flatnonzero(hot[p * P:(p + 1) * P])
        whole = hp[hp < P // 2] if tri else hp
        halves = hp[hp >= P // 2] if tri else hp[:0]
        shift = Uh if (tri and whole.size == 0) else 0
        cursor, fit, fit_whole = shift, 0, 0
        for t in whole:
            if cursor + U <= cap:
                slot_of[p * P + t] = cursor
                fit, fit_whole = fit + 1, fit_whole + 1
            cursor += U
        for t in halves:
            if cursor + Uh <= cap:
                slot_of[p * P + t] = cursor - Uh
                fit += 1
            cursor += Uh
        count = min(fit, LIST_MAX)
        head[p] = [count, min(hp.size, LIST_MAX), min(fit_whole, count), 1 if shift else 0]
        lists.append(hp[:LIST_MAX].astype(np.int32))
    return slot_of, lists, head


def check_lists(slot_of, lists, head, active, hot, P, nslot):
    """What the per-panel chain needs of any row-cache list, as a list of violations (empty: none):
      1. the cache pieces [off, off + len) of the markers with a slot are pairwise disjoint and inside [0, nslot P / 64);
      2. no base is negative (nothing below the two sentinels -1 and -2);
      3. every marker with a slot stands in the packed list at a position below head[0] — the cache is filled from those entries;
      4. head[1], head[2], head[3] are what the layout says: rows listed, whole rows among those that fit, the shift;
      5. monomorphic markers, and only they, have -2; only hot markers have a slot."""
    U, Uh, tri = _geometry(P)
    cap = nslot * U
    bad = []
    slot_of, active, hot = np.asarray(slot_of), np.asarray(active, dtype=bool), np.asarray(hot, dtype=bool)
    for p in range(active.size // P):
        sl, ac, ho = slot_of[p * P:(p + 1) * P], active[p * P:(p + 1) * P], hot[p * P:(p + 1) * P]
        if sl.min(initial=0) < -2:
            bad.append("panel %d: 2. a base below the sentinels" % p)
        if not np.array_equal(sl == -2, ~ac):
            bad.append("panel %d: 5. -2 is not exactly the monomorphic markers" % p)
        if (sl[~ho] >= 0).any():
            bad.append("panel %d: 5. a marker that is not hot has a slot" % p)
        used = np.zeros(max(cap, 1), dtype=np.int32)
        for t in np.flatnonzero(sl >= 0):
            half = tri and t >= P // 2
            off, ln = (int(sl[t]) + Uh, Uh) if half else (int(sl[t]), U)
            if off < 0 or off + ln > cap:
                bad.append("panel %d marker %d: 1. piece [%d, %d) outside [0, %d)" % (p, t, off, off + ln, cap))
            else:
                used[off:off + ln] += 1
        if used.max(initial=0) > 1:
            bad.append("panel %d: 1. cache pieces overlap" % p)
        lst, h = np.asarray(lists[p]), [int(v) for v in head[p]]
        for t in np.flatnonzero(sl >= 0):
            pos = np.flatnonzero(lst == t)
            if pos.size != 1 or pos[0] >= h[0]:
                bad.append("panel %d marker %d: 3. a slot, but not among the first %d of the list" % (p, t, h[0]))
                break
        hp = np.flatnonzero(ho)
        n_whole = int((hp < P // 2).sum()) if tri else hp.size
        fit_whole = int(((sl >= 0) & ((np.arange(P) < P // 2) | (not tri))).sum())
        want = [min(hp.size, LIST_MAX), min(fit_whole, h[0]), 1 if (tri and n_whole == 0) else 0]
        if h[1:] != want:
            bad.append("panel %d: 4. head words [1..3] %r, the layout says %r" % (p, h[1:], want))
        if not np.array_equal(lst[:h[1]], hp[:h[1]]):
            bad.append("panel %d: 4. the list is not the hot markers in marker order" % p)
        if not (0 <= h[0] <= h[1] <= LIST_MAX):
            bad.append("panel %d: 4. head[0] = %d rows to fill from a list of %d" % (p, h[0], h[1]))
    return bad


def hot_patterns(P, nslot):
    """The hot patterns of one panel at which the layout takes another path, as {name: P flags}: none; one marker at 0, P/2 - 1, P/2, P - 1;
    the second half only (panel 512: the shifted layout), a few and all of it; exactly nslot, nslot + 1 and all P; more than LIST_MAX (from
    panel 256 on)."""
    rng = np.random.default_rng(1000 * P + nslot)

    def flags(ix):
        f = np.zeros(P, dtype=bool)
        f[np.asarray(ix, dtype=np.int64)] = True
        return f

    pat = {"none": flags([]), "at-0": flags([0]), "at-half-1": flags([P // 2 - 1]), "at-half": flags([P // 2]), "at-last": flags([P - 1]),
           "second-half-few": flags(P // 2 + np.array([1, 2, 11, P // 2 - 6])), "second-half-all": flags(np.arange(P // 2, P)),
           "nslot": flags(rng.choice(P, min(nslot, P), replace=False)), "nslot+1": flags(rng.choice(P, min(nslot + 1, P), replace=False)),
           "all": flags(np.arange(P))}
    if P > LIST_MAX:
        few = np.ones(P, dtype=bool)
        few[[5, P // 2 + 9, P - 2]] = False
        if P == 512:
            few[3::3] = False                       # 341 hot: beyond the list in both halves together, within it in each
        assert few.sum() > LIST_MAX
        pat["beyond-the-list"] = few
    return pat


def lists_from_pack(hotpack):
    """(lists, head) of the device's packed array (npanels x HS): the entries behind the header, head[1] of them"""
    hotpack = np.asarray(hotpack)
    return [hotpack[p, 4:4 + max(0, min(int(hotpack[p, 1]), LIST_MAX))] for p in range(hotpack.shape[0])], hotpack[:, :4].copy()


def fits_the_list(P, nslot):
    """the list (LIST_MAX entries) can name every row a cache of nslot rows holds: whole rows elsewhere, up to 2 nslot - 1 half rows at panel 512.
    The device's nslot always does: it is capped at 250, and at panel 512 the 160 KiB of LDS hold 80 rows of 2 KiB, before anything else."""
    return (2 * nslot - 1 if P == 512 else nslot) <= LIST_MAX
