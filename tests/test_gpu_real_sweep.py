"""The fp64 resident layout's sweep (genotype_bits = 64) kernel by kernel: k_dot_real's row splits as the chain sums them, k_chain<K1, double>
(hb_chain_panel.hpp) and k_update_real (hb_real.hip), one sweep at a time, each step checked from the state read back before it — so a
failure names the kernel. tests/real_restatement.py holds the host restatements (tests/test_real_restatement_host.py checks them without a GPU).

What is exact, and why.
- The chain. Context.pre() returns what k_pre left (thresholds on rhs^2, 1 / v, sd z — the sweep's uniform and normal draws are in them), so
  k_chain has no randomness left, and no sum in it has an order of its own: a lane's right-hand side starts from the panel's mat-vec, 0 + ps[0] +
  ps[1] + ... over the row splits (the order of k_sum_partials, so Context.dot() on a second context that holds the emulated residual gives
  the chain's own starting bits for any number of splits), takes fma(xpx, g_old, .) and then one fma(-G[t][t'], delta_t, .) per move of an
  earlier marker t in ascending t. real_restatement.chain_panel is that; the device's move list (Context.events()) must be its list, indices
  and deltas, bit for bit, and so g, the tracker, the class counts and n_events.
- The update. k_update_real's lanes are a = 0; a = fma(x_e, d_e, a) in list order, r - a, u + a, r32 = (float)r:
  real_restatement.update_real, applied panel by panel; r, u, the mirror's rows [0, n), its padding rows [n, ld) (zero) and r32 are equalities.
  The fma is vectorised on the host (an error-free product and sums, exact rational arithmetic where those are not provably one rounding), so
  the update is restated exactly at n = 65 537 too, where exact rational arithmetic alone would take minutes; the dot-product bound of a
  panel's update, |r_after - (r_before - sum_e x_e d_e)| <= k eps sum_e |x_e d_e| + eps |r_after| (k moves: a chain of k fmas is within k u
  sum |x d|, u = eps / 2, and r - a rounds once), summed over the sweep's panels, is asserted there as well.

What is a bound.
- A panel's mat-vec against a long-double product: n eps sum |x_i r_i| (any order of n fused terms; tests/test_gpu_real.py uses the same).
- sum_g2 is an fp64 atomic over the panels of a block sum over at most 512 markers (a shuffle tree: nine levels and the sixteen wave
  sums): (panels + 10) eps sum w.

The fixed-point mirrors (rq, vexp, mb) do not exist on this layout: mirrors() reports none (asserted).

Not tested: the fp64 layout under row or column shards and under BSLMM (Bayes() refuses both: tests/test_gpu_real.py), and n beyond 65 537
(17 row splits: the chain's first sixteen in registers and one trip of its tail loop; more trips are the same loop)."""
import math

import numpy as np
import pytest

import hibayes_amd as H
from hibayes_amd.engine import Context
from real_restatement import chain_panel, update_real
from test_gpu_real import dosages

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
INF = float("inf")
SEED = 20251101
WIDE = np.longdouble if np.finfo(np.longdouble).nmant > 52 else None


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def wide_matvec(X, r):
    if WIDE is not None:
        return (X.astype(WIDE).T @ r.astype(WIDE)).astype(np.float64)
    return np.array([math.fsum(X[:, j] * r) for j in range(X.shape[1])])


def nslot_real(P):
    """chain_nslot(P, 8) of hb_kernels.hip: the Gram rows of P doubles that fit in 158 KiB of LDS beside the event lists (16 P bytes) and the
    reduction words (320 bytes): 37 at P = 512, 76 at P = 256, the whole panel at 128 and 64"""
    return (158 * 1024 - (P * 16 + 128 + 128 + 64)) // (P * 8)


def special_dosages(rng, n, m, const_col, den_col, negz_col):
    """dosages() of tests/test_gpu_real.py (halves and irrational convex weights) with a constant fractional column (never moves), a column
    with a denormal entry and one with a -0.0"""
    X = dosages(rng, n, m) if n >= 6 else rng.random((n, m))
    for j in range(m):                                       # every other column polymorphic, whatever the draw
        if X[:, j].min() == X[:, j].max():
            X[0, j] += 0.25
    X[:, const_col] = 0.37
    X[0, den_col] = 1e-310
    X[n - 1, negz_col] = -0.0
    assert X[:, den_col].min() != X[:, den_col].max() and X[:, negz_col].min() != X[:, negz_col].max()
    return np.asfortranarray(X)


# ------------------------------------------------------------------------------------------------------------------------
# one or two sweeps on one context, checked panel by panel
# ------------------------------------------------------------------------------------------------------------------------
def run_sweeps(name, X, model, kw, g0, r0, u0, P, sweeps=1, int8=False, bound_too=False):
    """X: doubles for the fp64 layout, int8 codes with int8=True (precise = 1 on the per-panel kernels: k_dot's partials, k_chain<1>, k_update).
    Returns per sweep the lists and what the chain wrote, after asserting everything the module's docstring lists."""
    n, m = X.shape
    Xd = X.astype(np.float64)
    fold = kw.get("fold")
    res = []

    def make():
        if int8:
            c = Context(n, m, panel=P, precise=1, seed=SEED)
            c.upload(X)
            c.set_pipeline(0, 0, 1)
            assert c.layout()[0] == 8 and c.pipeline()[:3] == (0, 0, 1), name
        else:
            c = Context(n, m, panel=P, seed=SEED)           # the default precise
            c.upload_real(X)
            assert c.layout()[0] == 64 and c.pipeline()[:3] == (0, 0, 1), name
        return c

    with make() as c, make() as d:
        assert c.panel == P and c.ld == -(-n // 256) * 256, name
        ld, npan = c.ld, -(-m // P)
        m_pad = npan * P
        xpx, vx, _, _ = c.marker_stats()
        c.build_gram()
        grams = [(c.gram(p) if int8 else c.gram_real(p)) for p in range(npan)]
        pad = lambda a: np.concatenate([a, np.zeros(m_pad - m)])
        xpx_p, vx_p = pad(xpx), pad(vx)
        c.set_effects(g0, (g0 != 0).astype(np.uint8), np.ones(m))
        c.set_residual(r0, u0)
        g_cur, r_cur, u_cur = g0.copy(), r0.copy(), u0.copy()
        for it in range(sweeps):
            out = c.sweep(model, it, 1.0, **kw)
            thr, invv, sdz = c.pre()
            cnt, lists = c.events()
            g_dev, trk_dev, _ = c.get_effects()
            r_dev, u_dev = c.get_residual()
            mir = c.mirrors()
            K1 = thr.shape[0]
            g_want, cls_want = np.zeros(m_pad), np.zeros(m_pad, dtype=np.int64)
            g_cur_p = pad(g_cur)
            sum_w, total, per_panel = 0.0, 0, []
            for p in range(npan):
                tag = (name, "sweep %d" % it, "panel %d" % p)
                sl = slice(p * P, (p + 1) * P)
                cols = min(P, m - p * P)
                # ---- the panel's input mat-vec: the chain's own starting bits ----
                d.set_residual(r_cur, np.zeros(n))
                dots = np.zeros(P)
                dots[:cols] = d.dot(p * P, cols)
                want = wide_matvec(Xd[:, p * P:p * P + cols], r_cur)
                lim = n * EPS * (np.abs(Xd[:, p * P:p * P + cols]) * np.abs(r_cur)[:, None]).sum(0)
                assert np.all(np.abs(dots[:cols] - want) <= lim), tag + ("k_dot_real / k_dot", float(np.max(np.abs(dots[:cols] - want) / np.maximum(lim, 1e-300))))
                # ---- the chain ----
                idx, dl, g_new, cls, sw = chain_panel(grams[p], xpx_p[sl], vx_p[sl], g_cur_p[sl], dots, thr[:, sl], invv[:, sl], sdz[:, sl], model, fold)
                assert cnt[p] == len(idx), tag + ("moves", int(cnt[p]), len(idx), lists[p][0][:8].tolist(), idx[:8].tolist())
                assert np.array_equal(lists[p][0], idx), tag + ("the move list's markers", np.flatnonzero(lists[p][0] != idx)[:4].tolist())
                assert np.array_equal(u64(lists[p][1]), u64(dl)), tag + ("the move list's deltas", np.flatnonzero(u64(lists[p][1]) != u64(dl))[:4].tolist())
                g_want[sl], cls_want[sl] = g_new, cls
                sum_w += sw
                total += len(idx)
                # ---- the update ----
                gcols = p * P + idx
                r_before = r_cur
                r_cur, u_cur, _ = update_real(X, r_cur, u_cur, gcols, dl)
                per_panel.append((gcols, dl, r_before))
            # ---- after the sweep: what the chain wrote ----
            tag = (name, "sweep %d" % it)
            assert np.array_equal(u64(g_dev), u64(g_want[:m])), tag + ("g", np.flatnonzero(u64(g_dev) != u64(g_want[:m]))[:8].tolist())
            assert np.array_equal(trk_dev.astype(np.int64), cls_want[:m]), tag + ("tracker",)
            allc = np.concatenate([pp[0] for pp in per_panel]).astype(np.int64)
            rest = np.ones(m, dtype=bool)
            rest[allc] = False
            assert len(np.unique(allc)) == len(allc)
            assert np.array_equal(u64(g_dev[rest]), u64(g_cur[rest])), tag + ("an effect changed without a move",)
            active = vx != 0.0
            cc = np.zeros(len(out["class_count"]))
            for k in range(K1 + 1):
                if k < len(cc):
                    cc[k] = np.sum(active & (cls_want[:m] == k))
            assert np.array_equal(out["class_count"], cc), tag + ("class_count", out["class_count"], cc)
            assert out["n_events"] == total, tag + ("n_events", out["n_events"], total)
            print("%s sweep %d: sum_g2 off by %.2f eps sum w" % (name, it, abs(out["sum_g2"] - sum_w) / max(EPS * sum_w, 1e-300)))
            assert abs(out["sum_g2"] - sum_w) <= (npan + 10) * EPS * sum_w, tag + ("sum_g2", out["sum_g2"], sum_w)
            # ---- ... and the update rows ----
            assert np.array_equal(u64(r_dev), u64(r_cur)), tag + ("yadj", int((u64(r_dev) != u64(r_cur)).sum()))
            assert np.array_equal(u64(u_dev), u64(u_cur)), tag + ("u", int((u64(u_dev) != u64(u_cur)).sum()))
            assert mir["slot"] == 0 and np.array_equal(u64(mir["r"][:n]), u64(r_cur)), tag + ("the mirror's residual",)
            assert not mir["r"][n:].any() and not mir["r32"][n:].any(), tag + ("rows [n, ld)",)
            assert np.array_equal(mir["r32"].view(np.uint32), mir["r"].astype(np.float32).view(np.uint32)), tag + ("r32",)
            assert mir["rq"] is None and mir["vexp"] is None, tag + ("digit planes on a layout that keeps none",)
            if bound_too:                                    # the dot-product bound of the update, from the device's own lists and residual
                rr = r0 if it == 0 else res[-1]["r"]
                acc, absacc, k = np.zeros(n, dtype=WIDE or np.float64), np.zeros(n), 0
                for gcols, dl, _ in per_panel:
                    for j, dv in zip(gcols, dl):
                        acc = acc + Xd[:, j].astype(acc.dtype) * dv
                        absacc += np.abs(Xd[:, j] * dv)
                    k = max(k, len(gcols))
                err = np.abs((r_dev.astype(acc.dtype) - (rr.astype(acc.dtype) - acc)).astype(np.float64))
                lim = len(per_panel) * (k * EPS * absacc + EPS * (np.abs(rr) + absacc))
                assert np.all(err <= lim), tag + ("the update's dot-product bound", float(np.max(err / np.maximum(lim, 1e-300))))
            res.append({"lists": [(pp[0], pp[1]) for pp in per_panel], "counts": [len(pp[0]) for pp in per_panel], "g_before": g_cur.copy(),
                        "g": g_dev.copy(), "cls": cls_want[:m].copy(), "r": r_dev.copy(), "kpad": K1, "thr": thr})
            g_cur = g_dev
    return res


def install_counts(rng, X, P, counts, gmag, must=()):
    """counts[p] installed effects in panel p (the last panel ragged, its moves all inside it), on polymorphic columns only"""
    n, m = X.shape
    g = np.zeros(m)
    poly = X.min(0) != X.max(0)
    for p, k in enumerate(counts):
        lo, hi = p * P, min(m, (p + 1) * P)
        forced = [j for j in must if lo <= j < hi]
        free = np.setdiff1d(np.flatnonzero(poly[lo:hi]) + lo, forced)
        assert len(forced) <= k <= len(forced) + len(free), (p, k, len(free))
        pick = np.concatenate([np.array(forced, dtype=np.int64), rng.choice(free, k - len(forced), replace=False)]).astype(np.int64)
        g[pick] = rng.choice([-1.0, 1.0], size=k) * rng.uniform(0.1, 1.0, size=k) * gmag
    return g


# ------------------------------------------------------------------------------------------------------------------------
# 1. the move counts of k_update_real
# ------------------------------------------------------------------------------------------------------------------------
COUNT_CASES = [
    ("p64", 301, 64, [0, 1, 7, 8, 9, 16, 17, 63, 64, 3], 5),
    ("p512", 301, 512, [511, 512, 0, 100], 100),
    ("n2", 2, 64, [9], 40),
    ("n255", 255, 64, [9], 40),
    ("n257", 257, 64, [9], 40),
]


@pytest.mark.parametrize("case", COUNT_CASES, ids=[c[0] for c in COUNT_CASES])
def test_update_real_applies_a_chosen_move_list_bit_for_bit(case):
    """BayesC with pi_1 = 0 removes exactly the installed effects (tests/test_gpu_update.py chooses its lists the same way), so the test
    chooses every panel's number of moves: none (the kernel returns before it touches a row), one, and both sides of its batches of 8 — 7, 8,
    9, 16, 17, 63, 64 — where the last batch reads s_dl[nev .. nev + 8), zero-filled, and its columns through min(e0 + k, nev - 1); 511 and 512
    at panel 512, where the staging clamps s_ix[min(e, 511)]; a ragged last panel with all its moves inside it; n = 2, 255, 257 around the
    256 lanes x 2 rows of a workgroup. The constant column sits in a panel whose other markers all move (p512) or in one without a move."""
    name, n, P, counts, ragged = case
    m = (len(counts) - 1) * P + ragged
    rng = np.random.default_rng(sum(map(ord, name)))
    base = 3 * P if name == "p64" else 0                    # the denormal and the -0.0 sit in columns that move
    X = special_dosages(rng, n, m, 5, base + 1, base + 2)
    g0 = install_counts(rng, X, P, counts, 0.5, must=(base + 1, base + 2))
    assert g0[5] == 0.0
    r0, u0 = rng.normal(size=n), rng.normal(size=n)
    res = run_sweeps(name, X, "BayesC", dict(varg=0.01, logpi=[0.0, -INF]), g0, r0, u0, P)
    assert res[0]["counts"] == counts, (name, res[0]["counts"])
    allc = np.concatenate([l[0] for l in res[0]["lists"]])
    assert set(allc.tolist()) == set(np.flatnonzero(g0).tolist()) and not res[0]["g"].any()


# ------------------------------------------------------------------------------------------------------------------------
# 2. the row cache of k_chain<1, double>
# ------------------------------------------------------------------------------------------------------------------------
def hot_positions(P, nhot):
    """Panel-local positions of nhot hot markers (position 0 is kept for a column that never moves, 1 and P - 2 for markers that enter from
    zero): the cached ones spread up to lane 15 of wave wc = P / 128 - 1, the first one without a slot at lane 20 of that wave, further ones in
    the waves behind it."""
    nslot = nslot_real(P)
    if nhot >= P:
        return np.arange(P)
    wc = max(0, P // 128 - 1)
    ncached = min(nhot, nslot)
    pos = np.unique(np.rint(np.linspace(2, 64 * wc + 15, ncached)).astype(np.int64))
    assert len(pos) == ncached
    later = [64 * wc + 20] + sorted(64 * w + o for w in range(wc + 1, P // 64) for o in ((7,) if P >= 512 else (7, 40)))
    pos = np.concatenate([pos, np.array(later[:nhot - ncached], dtype=np.int64)])
    assert len(pos) == nhot and pos.max() < P - 2 and (np.diff(pos) > 0).all()
    return pos


CACHE_CASES = [(512, k) for k in (36, 37, 38, 41)] + [(256, k) for k in (75, 76, 77, 80)] + [(128, 128)]


@pytest.mark.parametrize("P,nhot", CACHE_CASES)
def test_chain_row_cache_edges_and_markers_without_a_slot(P, nhot):
    """k_chain<1, double> caches the Gram rows of the first nslot = (158 * 1024 - (16 P + 320)) / (8 P) hot markers (g_old != 0), in marker order:
    37 at P = 512, 76 at P = 256; a hot marker behind them has slot -1, packed into its event record as (slot << 16) | marker, and its row is
    read from global memory, like the row of a marker that enters from zero. nhot = nslot - 1, nslot, nslot + 1 and nslot + 4 in each of two
    full panels (the second sees a residual that moved) and a ragged third; the first marker without a slot shares wave wc with cached ones,
    the others sit in later waves, and a strong signal makes markers enter from zero before and behind them (asserted on the list). P = 128
    holds all of its 128 hot rows. BayesCpi: installed effects are redrawn or removed, the others may enter. Two sweeps: the second starts
    from the device's own state and replays the captured graph of the first; all eight class counts are compared, those past the model's two
    classes with 0 (the regression test of the sums' zeroing: a replayed memset left non-zero denormals there and under every sum)."""
    n, ragged = 301, 37
    m = 2 * P + ragged
    nslot = nslot_real(P)
    assert nslot == {512: 37, 256: 76, 128: 155}[P]
    rng = np.random.default_rng(P + nhot)
    const_col = 2 * P + 4 if nhot >= P else 0
    X = special_dosages(rng, n, m, const_col, P + 1, P - 2)   # (the denormal in the second panel's entrant, the -0.0 in the first's)
    g0 = np.zeros(m)
    pos = hot_positions(P, nhot)
    for p in range(2):
        g0[p * P + pos] = rng.choice([-1.0, 1.0], size=nhot) * rng.uniform(0.02, 0.2, size=nhot)
    g0[2 * P + np.arange(0, 30, 3) + 5] = 0.05
    assert g0[const_col] == 0.0
    r0 = rng.normal(size=n)
    enter = [] if nhot >= P else [1, P - 2, P + 1, 2 * P - 2]
    for j in enter:
        assert g0[j] == 0.0
        r0 = r0 + 2.0 * X[:, j]
    res = run_sweeps("cache P=%d nhot=%d" % (P, nhot), X, "BayesCpi", dict(varg=0.01, logpi=[math.log(0.5), math.log(0.5)]), g0, r0,
                     rng.normal(size=n), P, sweeps=2)
    # the placement, from the effects the sweep started with
    for p in range(2):
        hot = np.flatnonzero(g0[p * P:(p + 1) * P])
        assert len(hot) == nhot
        cached, without = hot[:nslot], hot[nslot:]
        assert len(without) == max(0, nhot - nslot)
        moved = res[0]["lists"][p][0] - p * P
        assert set(hot.tolist()) <= set(moved.tolist())          # a hot marker always moves
        entrants = np.setdiff1d(moved, hot)
        if nhot < P:
            edge = without[0] if len(without) else cached[-1]
            last = without[-1] if len(without) else cached[-1]
            assert (entrants < edge).any() and (entrants > last).any(), (P, nhot, p, entrants.tolist())
        if len(without):
            assert (cached // 64 == without[0] // 64).any(), "the first marker without a slot shares its wave with cached ones"
            assert (without[1:] // 64 > without[0] // 64).all(), "the others sit in later waves"
    assert res[1]["counts"][0] > 0 and res[1]["counts"][1] > 0


# ------------------------------------------------------------------------------------------------------------------------
# 3. every instantiation
# ------------------------------------------------------------------------------------------------------------------------
R4 = dict(varg=1.0, logpi=np.log([0.95, 0.02, 0.02, 0.01]).tolist(), fold=[0.0, 1e-4, 1e-3, 1e-2])
R6 = dict(varg=1.0, logpi=np.log([0.5, 0.1, 0.1, 0.1, 0.1, 0.1]).tolist(), fold=[0.0, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1])
MODEL_CASES = [("BayesRR", "BayesRR", dict(varg=0.01)), ("BayesA", "BayesA", dict(varg=0.01, s2varg_df=0.05, dfvara=4.0)),
               ("BayesL", "BayesL", dict(varg=0.01)), ("BayesR-4", "BayesR", R4), ("BayesR-6", "BayesR", R6),
               ("BayesBpi", "BayesBpi", dict(varg=0.01, s2varg_df=0.05, dfvara=4.0, logpi=[math.log(0.9), math.log(0.1)]))]


@pytest.mark.parametrize("P", [64, 512])
@pytest.mark.parametrize("case", MODEL_CASES, ids=[c[0] for c in MODEL_CASES])
def test_every_instantiation_of_the_chain_bit_for_bit(case, P):
    """k_chain<1, double> under BayesRR, BayesA, BayesL and BayesBpi, k_chain<3, double> under BayesR with four classes, k_chain<7, double>
    under BayesR with six. In BayesRR, BayesA and BayesL every polymorphic marker moves: 512 moves in the full panel at P = 512 (the
    staging clamp of k_update_real again), and the rows of the hot markers past slot 37 and of every marker that starts at zero come from
    global memory. BayesL: one installed effect is chosen so that the draw lands inside (-1e-6, 1e-6) and the kernel's clamp sets 1e-6
    (marker 0 sees no move before it, so its right-hand side is dot_0 + xpx_0 g_0 and g_0 = (-sd z / (1 / v) - dot_0) / xpx_0 makes the draw
    a rounding error; sd z and 1 / v do not depend on g in this model and are read from a sweep on a scratch context)."""
    name, model, kw = case
    n = 301
    m = P + (100 if P == 512 else 64 + 5)
    rng = np.random.default_rng(sum(map(ord, name)) + P)
    X = special_dosages(rng, n, m, P + 3, 1, 2)             # the constant column in the last panel: the first one moves whole
    g0 = np.where(rng.random(m) < 0.3, rng.normal(size=m) * 0.1, 0.0)
    g0[P + 3] = 0.0
    g0[0] = 0.1
    beta = np.zeros(m)
    beta[rng.choice(m, 8, replace=False)] = rng.normal(size=8)
    r0, u0 = X @ beta + rng.normal(size=n), rng.normal(size=n)
    if model == "BayesL":
        with Context(n, m, panel=P, seed=SEED) as e:
            e.upload_real(X)
            e.build_gram()
            e.set_effects(g0, (g0 != 0).astype(np.uint8), np.ones(m))
            e.set_residual(r0, u0)
            e.sweep(model, 0, 1.0, **kw)
            _, invv, sdz = e.pre()
            e.set_residual(r0, u0)
            dot0 = e.dot(0, 1)[0]
            xpx0 = e.marker_stats()[0][0]
        g0[0] = (-sdz[0, 0] / invv[0, 0] - dot0) / xpx0
    res = run_sweeps("%s P=%d" % (name, P), X, model, kw, g0, r0, u0, P)[0]
    assert res["kpad"] == {"BayesR-4": 3, "BayesR-6": 7}.get(name, 1)
    if model in ("BayesRR", "BayesA", "BayesL"):
        assert res["counts"][0] == P and sum(res["counts"]) == m - 1, res["counts"]
    if model == "BayesL":
        assert res["g"][0] == 1e-6 and res["lists"][0][0][0] == 0
    if model == "BayesR":
        top = 3 if name == "BayesR-4" else 5
        print(name, P, "classes drawn:", np.bincount(res["cls"], minlength=top + 1).tolist())
        assert res["cls"].max() <= top and len(set(res["cls"].tolist())) >= 2, sorted(set(res["cls"].tolist()))
        assert np.isinf(res["thr"][top:]).all() and np.isfinite(res["thr"][top - 1][:m][X.min(0) != X.max(0)]).any()
    if model == "BayesBpi":
        assert 0 < sum(res["counts"]) < m - 1


# ------------------------------------------------------------------------------------------------------------------------
# 4. row splits
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,int8", [(4097, False), (65537, False), (65537, True)])
def test_chain_sums_the_row_splits_in_split_order(n, int8):
    """n = 4 097: ld = 4 352, two row splits of k_dot_real, which the chain adds as 0 + ps[0] + ps[1]. n = 65 537: ld = 65 792, 17 splits —
    the sixteen the chain holds in registers and one trip of its tail loop `for (sp = 16; sp < nsplit; sp++)`. The same at n = 65 537 on
    int8 codes 0/1/2 with precise = 1 on the per-panel kernels: k_dot's 17 partials into k_chain<1> (the integer Gram block, the same
    restatement). m = 64 + 5 at panel 64, BayesCpi with a signal and installed effects. The chain is bit for bit; so is the residual (the
    host's fma is vectorised: see the module docstring), and it is also held to the dot-product bound of the update."""
    P, m = 64, 69
    rng = np.random.default_rng(n + int(int8))
    if int8:
        p = rng.uniform(0.05, 0.5, m)
        X = np.asfortranarray(((rng.random((n, m)) < p).astype(np.int8) + (rng.random((n, m)) < p).astype(np.int8)).astype(np.int8))
        Xf = X.astype(np.float64)
    else:
        X = Xf = special_dosages(rng, n, m, 5, 1, 2)
    assert -(-(-(-n // 256) * 256) // 4096) == (2 if n == 4097 else 17)
    g0 = np.zeros(m)
    hot = np.array([1, 2, 9, 30, 40, 63, 64, 66])
    g0[hot] = rng.normal(size=hot.size) * 0.05
    beta = np.zeros(m)
    beta[[3, 20, 50, 67]] = [0.3, -0.2, 0.25, 0.2]
    r0 = Xf @ beta + rng.normal(size=n)
    res = run_sweeps("splits n=%d int8=%d" % (n, int8), X, "BayesCpi", dict(varg=0.01, logpi=[math.log(0.9), math.log(0.1)]), g0, r0,
                     rng.normal(size=n), P, int8=int8, bound_too=True)[0]
    moved = np.concatenate([l[0] for l in res["lists"]])
    assert set(hot.tolist()) <= set(moved.tolist()) and len(moved) > hot.size     # the signal's markers entered from zero
