"""The residual's writers alone: the update rows of hb_update.hpp bit for bit with their digit planes, and the helper
kernels of hb_blocks.hpp at their loop edges.

Update rows. update_rows (move list, four rows per lane) and update_rows_dense (LDS-DMA slab, one row per lane) are deterministic: per
launch group a = 0; a = fma(x_e, d_e, a) for each move in list order; yadj -= a; u += a where the list is non-empty. emulate_update()
restates exactly that on the host (a + x d in numpy is the fma while x d is exact, i.e. for codes -1..2; entries with code 3 go through
fractions.Fraction, whose float() rounds correctly), so every assertion on yadj, u, r32 and the digits is an equality; the bounds mb[] are
checked as bounds and the exponent as hb_fix_exp of the bound behind it. The list actually applied is read back with Context.events()
and cross-checked against the effects bit for bit (delta = g_after - g_before in the point-mass chains; k_chain_dense draws the step and
stores g + step, so there g_after = g_before + delta); a BayesC sweep with pi_1 = 0 removes exactly the markers the test installed, with
pi_0 = 0 or BayesRR every polymorphic marker moves. Context.mirrors() (hb_ctx_debug_get_mirrors) reads the version the last executed update rows
wrote, hb_ctx_sweep_range stops a sweep after a prefix of its groups so that versions in mid-sweep are read as well.

Not tested: the load path without 32-bit offsets (update_rows' `wide_off == false`). It needs the genotypes of one launch group to span
4 GB — a million individuals at 4096 columns — and no test here allocates that. k_delta_unpack (the sharded run's exchange) has no entry
point on a single context and is not driven here either."""
import math
from fractions import Fraction

import mpmath
import numpy as np
import pytest

import hibayes_amd as H

pytestmark = pytest.mark.gpu

HB_ND = 7
INF = float("inf")
SEED = 20240901
EPS = float(np.finfo(np.float64).eps)


# ------------------------------------------------------------------------------------------------------------------------
# host restatements (tests/test_update_reference.py checks them without a GPU)
# ------------------------------------------------------------------------------------------------------------------------
def digits_of(q):
    """Balanced base-256 digits of the integer q as hb_store_digits splits it: HB_ND - 1 digits in [-128, 127], lowest first, and
    whatever is left as the top one (in [-128, 127] exactly when |q| fits the planes)."""
    d = []
    for _ in range(HB_ND - 1):
        lo = ((q & 0xff) ^ 0x80) - 0x80
        d.append(lo)
        q = (q - lo) >> 8
    return d + [q]


def fix_exp(bound):
    """hb_fix_exp: E with bound * 2^E < 2^54; 0 for a zero or non-finite bound"""
    if not (bound > 0.0) or not (bound < 1e300):
        return 0
    return min(max(53 - (math.frexp(bound)[1] - 1), -900), 900)


def emulate_update(X, r, u, groups):
    """The update rows on the host. groups: [(columns, deltas)] per launch group, in application order. Returns (r, u, versions) with
    versions[h] the residual after group h."""
    r, u = np.array(r, dtype=np.float64), np.array(u, dtype=np.float64)
    versions = []
    for cols, deltas in groups:
        a = np.zeros(len(r))
        for j, d in zip(cols, deltas):
            x = X[:, int(j)]
            t = a + x.astype(np.float64) * float(d)        # x d exact for x in {-1, 0, 1, 2}: one rounding, the fma's
            three = np.flatnonzero(x == 3)
            if len(three):
                d3 = 3 * Fraction(float(d))
                t[three] = [float(Fraction(float(v)) + d3) for v in a[three]]
            a = t
        r = r - a
        if len(cols):
            u = u + a
        versions.append(r)
    return r, u, versions


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def quantised_dots(X, r):
    """X' q 2^-E with q = rint(r 2^E), E = hb_fix_exp(max |r|), in exact integers: (values, |exact integer| < 2^61)"""
    E = fix_exp(float(np.abs(r).max()))
    q = np.rint(np.ldexp(r, E)).astype(np.int64)
    assert np.abs(q).max() < 2 ** 54
    lo = q & ((1 << 27) - 1)
    hi = (q - lo) >> 27
    Xt = X.T.astype(np.int64)
    a, b = Xt @ hi, Xt @ lo                                # each below 3 n 2^28
    exact = [(int(v) << 27) + int(w) for v, w in zip(a, b)]
    return np.array([math.ldexp(float(v), -E) for v in exact]), np.array([abs(v) < 2 ** 61 for v in exact])


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------
def geno(rng, n, m, codes):
    """codes "012", "-101" (int8 layout only) or "0123": the last with a 3 at each of the 16 positions of column 0's first packed word
    and column 1 all 3 but its last row (an all-3 column is monomorphic and never moves). Every column is polymorphic."""
    p = rng.uniform(0.05, 0.5, m)
    X = sum((rng.random((n, m)) < p).astype(np.int8) for _ in range(3 if codes == "0123" else 2))
    if codes == "-101":
        X = X - 1
    if codes == "0123":
        X[:16, 0] = 3
        X[16:, 0] = np.where(X[16:, 0] == 3, 2, X[16:, 0])
        X[:, 1] = 3
        X[n - 1, 1] = 0
        assert all((X[k::16] == 3).any() for k in range(16))
    X = np.asfortranarray(X.astype(np.int8))
    assert (X.astype(np.float64).var(0) > 0).all() and X.min() == {"012": 0, "-101": -1, "0123": 0}[codes] and X.max() == int(codes[-1])
    return X


def install(rng, m, P, D, counts, gmag, must=()):
    """Effects that a BayesC sweep with pi_1 = 0 removes: counts[h] markers of launch group h (D panels), those of the last group all in
    the last, ragged panel; |g| in [gmag / 10, gmag] with gmag itself among them."""
    npan = -(-m // P)
    G = -(-npan // D)
    assert len(counts) == G, (len(counts), G)
    g = np.zeros(m)
    for h, k in enumerate(counts):
        lo, hi = h * D * P, min(m, (h + 1) * D * P)
        if h == G - 1:
            lo = (npan - 1) * P
        forced = [j for j in must if lo <= j < hi]
        free = np.setdiff1d(np.arange(lo, hi), forced)
        assert len(forced) <= k <= hi - lo
        pick = np.concatenate([np.array(forced, dtype=np.int64), rng.choice(free, k - len(forced), replace=False)]).astype(np.int64)
        g[pick] = rng.choice([-1.0, 1.0], size=k) * rng.uniform(0.1, 1.0, size=k) * gmag
        if k:
            g[pick[0]] = gmag
    return g


CLASSES = ("0", "1..8", "9..32", "33..64", "65..448", "449..896", ">=897")


def move_class(k):
    """which batches and staging passes a group of k moves takes: one batch of 8 | of 32 | of 64 | several, one pass | two passes | three"""
    return CLASSES[sum(k > t for t in (0, 8, 32, 64, 448, 896))]


# ------------------------------------------------------------------------------------------------------------------------
# one sweep on one context, checked range by range
# ------------------------------------------------------------------------------------------------------------------------
def run_sweep(name, X, r0, u0, g0, *, panel, geo, precise, model, logpi, layout=8, nblocks=1, memo=None):
    """One sweep of `model` in `nblocks` ranges. After every range: assertions a-d of the module on what the update rows left; after the
    sweep: e. Returns the bits that another layout or form must reproduce. memo: emulations by range, shared between the variants of a case
    (reused only where the move lists are the same bits)."""
    n, m = X.shape
    out = {"ranges": []}
    with H.Context(n, m, panel=panel, precise=precise, seed=SEED) as c:
        c.upload(X)
        if layout == 2:
            c.set_layout(2, keep_int8=False)
        assert c.layout() == ((2, False) if layout == 2 else (8, True)), name
        c.set_pipeline(*geo)
        pl, Lv, D, _ = c.pipeline()
        assert pl == geo[0] and (not pl or D == geo[2]), (name, "the geometry asked for is not the one that runs", (pl, Lv, D))
        P, ld = c.panel, c.ld
        assert P == panel and ld == -(-n // 256) * 256
        npan = -(-m // P)
        gp = D if pl else 1                                 # panels per launch group
        G = -(-npan // gp)
        nb = min(nblocks, G) if pl else 1
        c.set_effects(g0, (g0 != 0).astype(np.uint8), np.ones(m))
        c.set_residual(r0, u0)
        kw = dict(vare=1.0, varg=0.01, logpi=logpi)
        r_cur, u_cur, g_cur = r0, u0, g0
        versions = {}
        total = 0
        for b in range(nb):
            c.sweep_range(b, nb, model, 0, **kw)
            g_lo, g_hi = (G * b // nb, G * (b + 1) // nb) if pl else (0, G)
            cnt, lists = c.events()
            groups = []
            for h in range(g_lo, g_hi):
                ps = range(h * gp, min(npan, (h + 1) * gp))
                assert all(cnt[p] >= 0 for p in ps), (name, h, cnt[list(ps)])
                groups.append((np.concatenate([p * P + lists[p][0] for p in ps]).astype(np.int64), np.concatenate([lists[p][1] for p in ps])))
                k = len(groups[-1][0])
                total += k
                out.setdefault("counts", []).append(k)
            cols = np.concatenate([g_[0] for g_ in groups])
            dls = np.concatenate([g_[1] for g_ in groups])
            # the list is what happened to the effects: each marker at most once, delta = g_after - g_before bit for bit — or, in
            # k_chain_dense, which draws the STEP and stores g + step, g_after = g_before + delta bit for bit
            g_new = c.get_effects()[0]
            assert len(np.unique(cols)) == len(cols) and (cols < m).all(), name
            if model == "BayesRR":
                assert np.array_equal(u64(g_new[cols]), u64(g_cur[cols] + dls)), (name, "g_before + move list against g_after")
            else:
                assert np.array_equal(u64(dls), u64(g_new[cols] - g_cur[cols])), (name, "move list against g_after - g_before")
            rest = np.ones(m, dtype=bool)
            rest[cols] = False
            assert np.array_equal(u64(g_new[rest]), u64(g_cur[rest])), (name, "an effect changed without a move")
            g_cur = g_new
            key = (b, nb, u64(cols).tobytes(), u64(dls).tobytes())
            if memo is not None and memo.get(b, (None,))[0] == key:
                r_cur, u_cur, vs = memo[b][1]
            else:
                r_cur, u_cur, vs = emulate_update(X, r_cur, u_cur, groups)
                if memo is not None:
                    memo[b] = (key, (r_cur, u_cur, vs))
            r_start = versions[g_lo - 1] if g_lo else r0
            for h, v in zip(range(g_lo, g_hi), vs):
                versions[h] = v
            # a. the residual and u
            rr, uu = c.get_residual()
            assert np.array_equal(u64(rr), u64(r_cur)), (name, "yadj after range %d" % b, int((u64(rr) != u64(r_cur)).sum()))
            assert np.array_equal(u64(uu), u64(u_cur)), (name, "u after range %d" % b, int((u64(uu) != u64(u_cur)).sum()))
            mir = c.mirrors()
            h_last = g_hi - 1
            assert mir["bound_index"] == h_last and mir["slot"] == (((g_hi - g_lo) & 1) if pl else npan % (Lv + 1)), (name, mir["slot"], mir["bound_index"])
            assert np.array_equal(u64(mir["r"][:n]), u64(r_cur)), (name, "the version slot's residual")
            # b. the padding rows
            assert not mir["r"][n:].any() and not mir["r32"][n:].any(), (name, "rows [n, ld)")
            # c. the fp32 mirror
            assert np.array_equal(mir["r32"].view(np.uint32), mir["r"].astype(np.float32).view(np.uint32)), (name, "r32")
            # d. bounds, exponent, digits
            if precise == 2:
                mb = mir["mb"]
                assert mb[0] == np.abs(r_start).max(), (name, "mb[0]", mb[0], np.abs(r_start).max())
                for h in range(g_hi):
                    assert mb[1 + h] >= np.abs(versions[h]).max(), (name, "bound of group %d" % h, mb[1 + h], np.abs(versions[h]).max())
                E = fix_exp(float(mb[1 + h_last]))
                assert mir["vexp"] == E, (name, "vexp", mir["vexp"], E)
                q = np.zeros(ld, dtype=np.int64)
                for k in range(HB_ND):
                    q += mir["rq"][k].astype(np.int64) << (8 * k)
                want = np.rint(np.ldexp(mir["r"], E))
                assert np.abs(want).max() < 2.0 ** 54, (name, "|q| >= 2^54")
                assert np.array_equal(q, want.astype(np.int64)), (name, "digit planes", int((q != want.astype(np.int64)).sum()))
                for i in (0, n // 2, n - 1):                # ... and plane by plane as digits_of splits
                    assert [int(mir["rq"][k][i]) for k in range(HB_ND)] == digits_of(int(want[i])), (name, i)
            else:
                assert mir["rq"] is None and mir["vexp"] is None
            out["ranges"].append({"r": u64(rr).copy(), "u": u64(uu).copy(), "r32": mir["r32"].view(np.uint32).copy(), "cols": cols, "dls": u64(dls).copy(),
                                  "rq": None if mir["rq"] is None else mir["rq"].copy(), "vexp": mir["vexp"], "mb": u64(mir["mb"][:1 + g_hi]).copy()})
        s = c.sweep_end()
        assert s["n_events"] == total, (name, s["n_events"], total)
        # e. the read-out left the context alone: the mat-vec of the final residual
        d = c.dot()
        if precise == 2:
            want, small = quantised_dots(X, rr)
            assert np.array_equal(d[small], want[small]), (name, "dot after the sweep")
            assert (np.abs(d[~small] - want[~small]) <= np.spacing(np.abs(want[~small]))).all(), (name, "dot after the sweep")
        else:                                                  # fp64 / fp32 accumulation of n terms in some order (fp32: of the rounded residual)
            Xf = np.abs(X.astype(np.float64))
            exact = np.array([math.fsum(col) for col in (X.astype(np.float64) * rr[:, None]).T])
            lim = 1.01 * n * (2.0 ** -53 if precise == 1 else 2.0 ** -24) * (Xf.T @ np.abs(rr))
            assert (np.abs(d - exact) <= lim).all(), (name, "dot after the sweep", float(np.max(np.abs(d - exact) / lim)))
        out["dot"] = u64(d).copy()
    return out


def same_bits(name, a, b, what):
    assert len(a["ranges"]) == len(b["ranges"])
    for ra, rb in zip(a["ranges"], b["ranges"]):
        for k in ("cols", "dls", "r", "u", "r32", "rq", "vexp", "mb"):
            assert (ra[k] is None and rb[k] is None) or np.array_equal(ra[k], rb[k]), (name, what, k)
    assert np.array_equal(a["dot"], b["dot"]), (name, what, "dot")


def ragged_panel(panel):
    """markers in the last panel"""
    return 100 if panel == 512 else 5


def residuals(rng, n, small_r):
    """small_r: r = 1e-3 N(0, 1) against |g| up to 1e3 — the bound decides the exponent, not the start value; else r of order 1, |g| ~ 1e-6"""
    r = rng.normal(size=n) * (1e-3 if small_r else 1.0)
    return r, rng.normal(size=n), (1e3 if small_r else 1e-6)


# (name, n, panel, geometry, codes, layouts, precise, counts per launch group, nblocks to try, small_r)
# Groups are D panels under the pipeline and single panels under the per-panel kernels (geometry (0, Lv, 1): Lv = 0 keeps one residual
# version, r_in == r). The last group's moves all sit in its last, ragged panel. P = 64 with eight panels per launch runs with one group of
# look-ahead (the band of two would be 23 blocks).
LIST_CASES = [
    ("p64-D8", 300, 64, (1, 1, 8), "012", (8, 2), 2, [8, 1, 0, 9, 32, 33, 64, 65, 447, 448, 449, 0, 3], (1, 3), True),
    ("p128-D8-code3", 1000, 128, (1, 1, 8), "0123", (8, 2), 2, [1024, 0, 449, 897, 2], (1, 2), False),
    ("p128-D7-signed", 1300, 128, (1, 2, 7), "-101", (8,), 2, [65, 447, 0, 896, 1], (1, 2), True),
    ("p64-D1", 1300, 64, (1, 2, 1), "012", (8, 2), 2, [0, 1, 8, 9, 32, 33, 64, 0, 1, 2], (1, 3), True),
    ("p64-D1-fp64", 1300, 64, (1, 2, 1), "012", (8,), 1, [0, 1, 8, 9, 32, 33, 64, 0, 1, 2], (1,), False),
    ("p64-D1-fp32", 300, 64, (1, 2, 1), "-101", (8,), 0, [0, 1, 8, 9, 32, 33, 64, 0, 1, 2], (1,), True),
    ("p128-D2-code3", 1000, 128, (1, 2, 2), "0123", (8, 2), 2, [2, 33, 0, 64, 65, 256, 8, 4], (1, 2), True),
    ("p64-D2", 300, 64, (1, 2, 2), "012", (8, 2), 2, [9, 128, 0, 32, 5], (2,), False),
    ("p64-serial-one-version", 300, 64, (0, 0, 1), "012", (8, 2), 2, [0, 1, 8, 9, 32, 33, 64, 0, 2], (1,), True),
    ("p128-serial-three-versions", 1000, 128, (0, 2, 1), "0123", (8, 2), 2, [2, 0, 128, 65, 0, 9, 3], (1,), False),
    ("p64-serial-fp64", 1300, 64, (0, 0, 1), "-101", (8,), 1, [0, 64, 8, 0, 33, 2], (1,), True),
    ("p512-D1", 300, 512, (1, 2, 1), "012", (8, 2), 2, [449, 0, 512, 7], (1, 2), True),
    ("p512-D2", 1000, 512, (1, 2, 2), "0123", (8, 2), 2, [1024, 449, 60], (1, 2), False),
    ("p512-D2-fp64", 1300, 512, (1, 2, 2), "012", (8,), 1, [897, 100], (1,), True),
]


@pytest.mark.parametrize("case", LIST_CASES, ids=[c[0] for c in LIST_CASES])
def test_update_rows_apply_a_chosen_move_list_bit_for_bit(case):
    """BayesC with pi_1 = 0: the installed effects are removed and nothing else moves, so the test chooses each group's number of moves —
    every batch size and staging pass of update_rows (move_class), groups without a move with and without a second residual version, a
    group whose moves sit in its ragged last panel — on the int8 and the 2-bit layout (the two load paths with 32-bit offsets), which must
    also agree bit for bit (f)."""
    name, n, panel, geo, codes, layouts, precise, counts, blocks, small_r = case
    D = geo[2] if geo[0] else 1
    m = (len(counts) - 1) * D * panel + (panel if D > 1 else 0) + ragged_panel(panel)
    rng = np.random.default_rng(sum(map(ord, name)))
    X = geno(rng, n, m, codes)
    r0, u0, gmag = residuals(rng, n, small_r)
    g0 = install(rng, m, panel, D, counts, gmag, must=(0, 1) if codes == "0123" else ())
    for nblocks in blocks:
        memo, first = {}, None
        for layout in layouts:
            tag = "%s layout=%d nblocks=%d" % (name, layout, nblocks)
            got = run_sweep(tag, X, r0, u0, g0, panel=panel, geo=geo, precise=precise, model="BayesC", logpi=[0.0, -INF], layout=layout,
                            nblocks=nblocks, memo=memo)
            assert got["counts"] == counts, (tag, "the installed pattern is not the list's", got["counts"], counts)
            assert set(np.concatenate([rg["cols"] for rg in got["ranges"]]).tolist()) == set(np.flatnonzero(g0).tolist()), tag
            if first is None:
                first = got
            else:
                same_bits(tag, first, got, "2-bit against int8")


def test_the_cases_cover_every_move_count_class_on_both_layouts():
    """Every case above asserts that the counts events() reported are the ones listed for it, so what ran is what the table says: each
    class of move_class with the counts at its edges on the int8 and on the 2-bit load path, and both ends also without digit planes."""
    for layout in (8, 2):
        every = set().union(*[set(c[7]) for c in LIST_CASES if layout in c[5] and c[6] == 2])
        assert {move_class(k) for k in every} == set(CLASSES), (layout, sorted(every))
        assert {0, 1, 8, 9, 32, 33, 64, 65, 447, 448, 449, 897, 1024} <= every, (layout, sorted(every))
        assert any(c[3][0] == 0 and c[3][1] == 0 and 0 in c[7] for c in LIST_CASES if layout in c[5])      # no move and one version: r_in == r
        assert any(c[3][0] == 1 and 0 in c[7] for c in LIST_CASES if layout in c[5])                        # no move under look-ahead
    plain = set().union(*[set(c[7]) for c in LIST_CASES if c[6] != 2])
    assert {move_class(k) for k in plain} >= {"0", ">=897"}


# ------------------------------------------------------------------------------------------------------------------------
# every marker moves: the dense form, the list form on the same data, three staging passes
# ------------------------------------------------------------------------------------------------------------------------
DENSE_CASES = [(n, D, 2) for n in (300, 1000, 1300) for D in (1, 2)] + [(1300, 2, 1), (1000, 1, 1), (1300, 2, 0)]


@pytest.mark.parametrize("n,D,precise", DENSE_CASES)
def test_dense_update_rows_against_the_list_form_and_the_emulation(n, D, precise, monkeypatch):
    """BayesRR at panel 512 runs k_chain_dense: with int8 columns its update is update_rows_dense (a grid row of the fixed-point mat-vec,
    k_update_dense beside the fp64 / fp32 one and for the groups no later launch carries). ld = 512, 1024, 1536 is 8, 16, 24 blocks of 64
    rows — all in the unpermuted tail, all permuted, sixteen permuted and eight not; a group is four (D = 1) or eight 128-column chunks
    through the two buffers, the ragged last panel's changes behind the 100th are zero. The same sweep with HB_DENSE_UPD set (the list
    form: 512 or 1024 moves, two or three staging passes) and on the 2-bit layout gives the same bits (f), all of them the emulation's."""
    name = "dense n=%d D=%d precise=%d" % (n, D, precise)
    m = 512 * 3 + 100
    rng = np.random.default_rng(n + D)
    codes = "-101" if precise != 2 and D == 2 else ("0123" if n == 1000 else "012")
    X = geno(rng, n, m, codes)
    r0, u0, gmag = residuals(rng, n, n != 1000)
    g0 = rng.normal(size=m) * gmag
    memo, got = {}, {}
    variants = [("dense", 8, False), ("list", 8, True)] + ([("2-bit", 2, False)] if precise == 2 and codes != "-101" else [])
    for what, layout, env in variants:
        if env:
            monkeypatch.setenv("HB_DENSE_UPD", "0")
        else:
            monkeypatch.delenv("HB_DENSE_UPD", raising=False)
        for nblocks in ((1, 2) if what == "dense" and D == 1 else (1,)):
            res = run_sweep("%s %s nblocks=%d" % (name, what, nblocks), X, r0, u0, g0, panel=512, geo=(1, 2, D), precise=precise, model="BayesRR",
                            logpi=[0.0, 0.0], layout=layout, nblocks=nblocks, memo=memo if nblocks == 1 else None)
            if nblocks == 1:
                got[what] = res
        npan = 4
        want = [min(m, (h + 1) * D * 512) - h * D * 512 for h in range(-(-npan // D))]
        assert got[what]["counts"] == want, (name, what, "every marker moves", got[what]["counts"])
        if what != "dense":
            same_bits(name, got["dense"], got[what], what + " against dense")


def test_three_staging_passes_where_every_marker_of_a_point_mass_model_moves():
    """BayesC with pi_0 = 0 (every polymorphic marker drawn afresh) at panel 128, eight panels per launch: 1024 moves a group, three
    passes of 448, 448 and 128, from effects of order 1e3 on a residual of order 1e-3; int8 against 2-bit."""
    n, P, D = 300, 128, 8
    m = 2 * P * D + P + 5
    rng = np.random.default_rng(77)
    X = geno(rng, n, m, "012")
    r0, u0, gmag = residuals(rng, n, True)
    g0 = rng.normal(size=m) * gmag
    memo, first = {}, None
    for layout in (8, 2):
        got = run_sweep("all-move layout=%d" % layout, X, r0, u0, g0, panel=P, geo=(1, 1, D), precise=2, model="BayesC", logpi=[-INF, 0.0],
                        layout=layout, nblocks=1, memo=memo)
        assert got["counts"] == [P * D, P * D, P + 5], got["counts"]
        if first is None:
            first = got
        else:
            same_bits("all-move", first, got, "2-bit against int8")


# ------------------------------------------------------------------------------------------------------------------------
# the other writers of the residual at their loop edges
# ------------------------------------------------------------------------------------------------------------------------
def fma_exact(a, x, r):
    """fl(a x + r) elementwise, one rounding"""
    fa = Fraction(float(a))
    return np.array([float(fa * Fraction(float(xi)) + Fraction(float(ri))) for xi, ri in zip(x, r)])


def mirror_ok(c, n, r_want, what):
    rr, _ = c.get_residual()
    mir = c.mirrors()
    assert mir["slot"] == 0 and np.array_equal(u64(mir["r"][:n]), u64(rr)) and not mir["r"][n:].any(), what
    assert np.array_equal(mir["r32"].view(np.uint32), mir["r"].astype(np.float32).view(np.uint32)), (what, "r32 is not the float cast of the residual")
    if r_want is not None:
        assert np.array_equal(u64(rr), u64(r_want)), (what, int((u64(rr) != u64(r_want)).sum()))
    return rr


C_SCALAR = 4     # roundings of the scalar tail of a step, each half an eps relative on a term it touches: fewer than 2 * C_SCALAR of them
LEVELS = (1, 2, 1024, 1025, 1500)
WORST = {}


def test_a_context_needs_two_individuals():
    """n = 1 is below what hb_ctx_create takes (the variances divide by n - 1): refused, not run. n = 2 is the smallest case below."""
    with pytest.raises(H._lib.HibayesError):
        H.Context(1, 64)


@pytest.mark.parametrize("n", [2, 63, 1023, 1024, 1025, 2049])
def test_helper_kernels_at_their_loop_edges(n):
    """k_shift, k_axpy, k_level_sums, k_level_axpy, k_cov_step and k_lev_step, one kernel per step, each from the state read back before
    it — so an error says which kernel made it. n around the 1024 threads of the one-workgroup kernels and the 256 of the others; 1, 2,
    1024, 1025 and 1500 levels, level 1 always empty (zz = 0) where there are two or more.

    Exact steps (one rounding per row, restated with numpy or Fraction): k_shift r + a, k_axpy fma(a, x, r), k_level_axpy r + delta[z],
    the rows of k_cov_step fma(old - g_i, c, r) and of k_lev_step r + (estR_old - estR_new)[z] given the coefficients read back.

    Derived bounds (eps = 2^-52, twice the unit roundoff, which absorbs the second-order terms):
    - a dot product (hb_ctx_cov_dot, k_cov_step's C_i . yadj): every thread chains ceil(n / 1024) fmas, a block reduction of ten levels
      (six shuffles, sixteen wave sums) follows: |err| <= (ceil(n / 1024) + 12) eps sum |c_k r_k|.
    - a level sum (k_level_sums, k_lev_step's Z' yadj): atomic adds in no fixed order, c_q - 1 of them into a level of c_q rows, each one
      rounding of a partial sum that is at most sum |r_k|: |err| <= (c_q - 1) eps sum_{k in q} |r_k| — the same shape, the chain being c_q
      long. An empty level is exactly 0.
    - the coefficient of k_cov_step, g_i = (s + v old) / v + sqrt(vare / v) z: the error of s over v, plus C_SCALAR eps on each of
      |s| / v, |old| and |sqrt(vare / v) z| for the six roundings behind them.
    - the coefficients of k_lev_step, e_q = (w_q + zz_q estR_q) / l_q + sqrt(vare / l_q) z_q with l_q = zz_q + vare / vrtmp: the error of w_q
      over l_q plus C_SCALAR eps (|w_q| / l_q + zz_q |estR_q| / l_q + |sqrt(vare / l_q) z_q|) (nine roundings, at most five behind a term).
    - vrtmp = (sum e_q^2 + s2r dfr) / chisq and vr = the two-pass variance of the e_q read back (its correction term cancels the error of
      the mean): (ceil(levels / 1024) + 16) eps relative, the dot product's chain and reduction plus the few scalar operations.
    The measured multiples of eps are printed before each assertion (DESIGN.md §7 holds the MI355X figures)."""
    rng = np.random.default_rng(n)
    X = np.asfortranarray(rng.integers(0, 3, size=(n, 64)).astype(np.int8))
    r = rng.normal(size=n)
    Cm = np.asfortranarray(rng.normal(size=(n, 2)))
    K = -(-n // 1024) + 12
    mpmath.mp.dps = 50
    worst = WORST.setdefault(n, {})

    def note(k, v):
        worst[k] = max(worst.get(k, 0.0), float(v))

    with H.Context(n, 64, panel=64, precise=2, seed=SEED) as c:
        c.upload(X)
        c.set_residual(r, np.zeros(n))
        mirror_ok(c, n, r, "set_residual")
        c.residual_shift(0.3125 + 2.0 ** -40)
        r = mirror_ok(c, n, r + (0.3125 + 2.0 ** -40), "k_shift")
        c.set_covariates(Cm)
        for i in range(2):                                    # the dot product alone
            got = c.cov_dot(i)
            t = Cm[:, i] * r
            e = float(abs(mpmath.mpf(got) - mpmath.fdot(Cm[:, i].tolist(), r.tolist())))
            note("dot", e / (EPS * float(np.abs(t).sum())))
            assert e <= K * EPS * float(np.abs(t).sum()), ("k_dot_vec", i, e)
        c.cov_axpy(1, -0.7)
        r = mirror_ok(c, n, fma_exact(-0.7, Cm[:, 1], r), "k_axpy")
        # ---- k_cov_step: one covariate per step ----
        cpc = (Cm * Cm).sum(0)
        for i in range(2):
            c.set_covariates(Cm[:, i:i + 1])
            c.blocks_setup(cpc[i:i + 1], [], [])
            old = 0.0
            for step, vare in enumerate((1.3, 0.9)):
                z = rng.normal(size=1)
                c.blocks_step(vare, z, [], [], -1.0, 0.0)
                gi = c.blocks_state()[0][0]
                ci, v = Cm[:, i], float(cpc[i])
                s = mpmath.fdot(ci.tolist(), r.tolist())
                sabs = float(np.abs(ci * r).sum())
                sd_z = mpmath.sqrt(mpmath.mpf(vare) / v) * float(z[0])
                want = (s + mpmath.mpf(v) * old) / v + sd_z
                bound = K * EPS * sabs / v + C_SCALAR * EPS * (float(abs(s)) / v + abs(old) + float(abs(sd_z)))
                e = float(abs(mpmath.mpf(gi) - want))
                note("cov g_i (of its bound)", e / bound)
                note("cov g_i", e / (EPS * (sabs / v + abs(old) + float(abs(sd_z)))))
                assert e <= bound, ("k_cov_step coefficient", i, step, e, bound)
                r = mirror_ok(c, n, fma_exact(old - gi, ci, r), "k_cov_step rows")
                old = gi
        # ---- the level kernels, one term per context state ----
        H._lib.check(c.L.hb_ctx_set_covariates(c.h, None, 0))
        for nlev in LEVELS:
            zid = rng.integers(0, nlev, size=n)
            if nlev >= 2:
                zid[zid == 1] = 0                             # level 1 is empty
            c.set_levels(zid, [nlev])
            cq = np.bincount(zid, minlength=nlev)

            def level_sums_exact(rv):
                order = np.argsort(zid, kind="stable")
                ends = np.cumsum(cq)
                vals = rv[order].tolist()
                ex = [mpmath.fsum(vals[e - k:e]) for e, k in zip(ends, cq)]
                ab = np.bincount(zid, weights=np.abs(rv), minlength=nlev)
                return ex, ab

            got = c.level_sums(0)
            ex, ab = level_sums_exact(r)
            err = np.array([float(abs(mpmath.mpf(float(gq)) - eq)) for gq, eq in zip(got, ex)])
            lim = np.maximum(cq - 1, 0) * EPS * ab
            note("level sums", (err / np.maximum(EPS * ab, 1e-300)).max())
            assert (err <= lim).all(), ("k_level_sums", nlev, float((err - lim).max()))
            assert not got[cq == 0].any()
            delta = rng.normal(size=nlev)
            c.level_axpy(0, delta)
            r = mirror_ok(c, n, r + delta[zid], "k_level_axpy %d levels" % nlev)
            # k_lev_step, twice: the second step starts from coefficients that are not zero
            zz = cq.astype(np.float64)
            vrtmp, dfr, s2r = 0.3, 4.0, 0.05
            c.blocks_setup([], zz, [vrtmp])
            est = np.zeros(nlev)
            for step, vare in enumerate((1.3, 0.9)):
                zl = rng.normal(size=nlev)
                chis = float(rng.chisquare(nlev + dfr))
                c.blocks_step(vare, [], zl, [chis], dfr, s2r)
                _, en, vt, vr = c.blocks_state()
                ex, ab = level_sums_exact(r)
                lam = mpmath.mpf(vare) / vrtmp
                worst_e = worst_b = 0.0
                for q in range(nlev):
                    l = zz[q] + lam
                    sd_z = mpmath.sqrt(mpmath.mpf(vare) / l) * float(zl[q])
                    want = (ex[q] + zz[q] * mpmath.mpf(float(est[q]))) / l + sd_z
                    scal = float(abs(ex[q]) / l) + float(zz[q] * abs(est[q]) / l) + float(abs(sd_z))
                    bound = max(cq[q] - 1, 0) * EPS * ab[q] / float(l) + C_SCALAR * EPS * scal
                    e = float(abs(mpmath.mpf(float(en[q])) - want))
                    worst_b = max(worst_b, e / bound)
                    worst_e = max(worst_e, e / (EPS * (ab[q] / float(l) + scal)))
                    assert e <= bound, ("k_lev_step coefficient", nlev, step, q, e, bound)
                note("lev e_q (of its bound)", worst_b)
                note("lev e_q", worst_e)
                r = mirror_ok(c, n, r + (est - en)[zid], "k_lev_step rows, %d levels" % nlev)
                Kq = -(-nlev // 1024) + 16
                ss = mpmath.fsum(en.tolist(), squared=True)
                want_vt = (ss + s2r * dfr) / chis
                e = float(abs(mpmath.mpf(float(vt[0])) - want_vt) / want_vt)
                note("vrtmp", e / EPS)
                assert e <= Kq * EPS, ("vrtmp", nlev, e / EPS)
                if nlev > 1:
                    mean = mpmath.fsum(en.tolist()) / nlev
                    var = mpmath.fsum([(mpmath.mpf(x) - mean) ** 2 for x in en.tolist()]) / (nlev - 1)
                    e = float(abs(mpmath.mpf(float(vr[0])) - var) / var)
                    note("vr", e / EPS)
                    assert e <= Kq * EPS, ("vr", nlev, e / EPS)
                else:
                    assert vr[0] == 0.0
                est, vrtmp = en, float(vt[0])
    print("helper kernels n = %4d (dot bound %d eps): " % (n, K) + ", ".join("%s %.2f" % kv for kv in sorted(worst.items())))
