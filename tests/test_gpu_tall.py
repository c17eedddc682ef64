"""The fixed-point mat-vec and its helpers on tall columns, at the range of their sums.

Every other kernel-alone test runs at n <= 5 100, where neither row split of plan_matvec binds: k_dotq's cap of 1023 stages per tile (int32
accumulators: 1023 x 128 rows x 128 x 128 < 2^31) and the 2-bit kernels' floor of ceil(rows / 131 072) tiles. With the default knobs they
bind for no launch of hb_ctx_dot either (NS = 2 at ld = 131 072), so every case runs under the defaults and again under HB_DOTQ_TILES = 1 /
HB_DOTQ2_TILES = 1, where test_tall_host.py shows from the plan header that a tile is as tall as the plan lets it be. Random data cannot
reach the accumulators' range (plane sums grow like sqrt(n)), so the columns and residuals are the extremes: all 3, all 127, all -127, all
-128 against digit planes that are all -128 or all 127.

Sizes: n = 131 072 (ld = 1024 stages: one more than the cap), 131 073, 174 001, 262 145 with m = 192, panel 64; n = 700 001 with m = 64 on
the 2-bit layout, past the 699 050 rows at which the scale-32 accumulator of k_dotq2 / k_dotq2m would wrap in one tile.

Equalities: every dot product of every kernel, shape and knob setting is the integer restatement of tall_restatement.py bit for bit; the
digit planes of slot 0 are the restatement's on rows [0, n) and zero on [n, ld); xpx, nvar0, download(); the sweep's yadj, u, r32, digits.
Bounds, each from the operation's own rounding count: the restatement within R / 2 ulp of the exact product (R: the Horner steps at or above
2^53, up to 4 here); vx within 2 ulp; X alpha within nnz eps sum |x alpha|; the residual sums within (ceil(n / 1024) + 22) eps sum |term|; the
fp64 mat-vec within n eps sum |x r|."""
import math
from fractions import Fraction

import numpy as np
import pytest

import hibayes_amd as H
from tall_restatement import HB_ND, SPECIAL2, SPECIAL8, restate, tall_genotypes, tall_residuals
from test_gpu_kernels import Q2M_SHAPES
from test_gpu_update import geno, install, residuals, run_sweep, same_bits

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
INF = float("inf")
SIZES = (131072, 131073, 174001, 262145)
TALLEST = 700001                                         # 2-bit kernels only, m = 64
KNOBS = {"default": {}, "one-tile": {"HB_DOTQ_TILES": "1", "HB_DOTQ2_TILES": "1"}}
RIDER_SIZES = (131073, 262145)
_INPUTS = {}                                             # the inputs and restatements by n: computed once, shared by every test below
WORST = {"R": 0, "ulps of R/2": 0.0}


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def inputs(n):
    """X (codes 0..3), X8 (the int8 context's: four more special columns), the residuals, and per residual the restatement of X (ref2)
    and of X8 (ref8: X's with the four columns restated again). Computed once per n and never modified."""
    if n not in _INPUTS:
        m = 64 if n == TALLEST else 192
        X, X8 = tall_genotypes(n, m, n)
        res = tall_residuals(n, n + 1)
        sp = sorted(SPECIAL8.values())
        ref2, ref8 = {}, {}
        for name, r in res.items():
            a = restate(X, r)
            ref2[name] = a
            if n != TALLEST:
                b = restate(np.asfortranarray(X8[:, sp]), r)
                d, acc, R, ulps = a["d"].copy(), a["acc"].copy(), a["R"].copy(), a["ulps"].copy()
                d[sp], acc[sp], R[sp], ulps[sp] = b["d"], b["acc"], b["R"], b["ulps"]
                ref8[name] = dict(a, d=d, acc=acc, R=R, ulps=ulps)
            for ref in (a, ref8.get(name)):
                if ref is not None and ref["R"].max() > 0:
                    WORST["R"] = max(WORST["R"], int(ref["R"].max()))
                    WORST["ulps of R/2"] = max(WORST["ulps of R/2"], float((2 * ref["ulps"][ref["R"] > 0] / ref["R"][ref["R"] > 0]).max()))
        for X_ in (X, X8):
            X_.setflags(write=False)
        _INPUTS[n] = (X, X8, res, ref2, ref8)
    return _INPUTS[n]


def set_env(monkeypatch, *settings):
    for name in ("HB_DOTQ_TILES", "HB_DOTQ2_TILES", "HB_Q2M_G", "HB_Q2M_CT", "HB_Q2M_SC", "HB_DOTQ2_KIND"):
        monkeypatch.delenv(name, raising=False)
    for s in settings:
        for k, v in s.items():
            monkeypatch.setenv(k, v)


def planes_wrong(c, n, ref, what):
    """After set_residual + dot() on a context that has not swept, hb_ctx_debug_get_mirrors serves slot 0: the residual as set, the digit
    planes launch_quant0 wrote for the dot products, and their exponent. Returns what differs from the restatement."""
    mir = c.mirrors()
    wrong = []
    if mir["slot"] != 0 or mir["vexp"] != ref["E"]:
        wrong.append(what + ("slot %d, exponent %s against %d" % (mir["slot"], mir["vexp"], ref["E"]),))
    for k in range(HB_ND):
        if not np.array_equal(mir["rq"][k, :n], ref["planes"][k]):
            wrong.append(what + ("digit plane %d on rows [0, n): %d rows differ" % (k, int((mir["rq"][k, :n] != ref["planes"][k]).sum())),))
    if mir["rq"][:, n:].any() or mir["r"][n:].any():
        wrong.append(what + ("rows [n, ld) are not zero",))
    return wrong


def dots_wrong(d, ref, what):
    bad = np.flatnonzero(u64(d) != u64(ref["d"]))
    return [what + ("columns", bad[:8].tolist(), d[bad[:4]].tolist(), ref["d"][bad[:4]].tolist())] if len(bad) else []


def the_extreme_sums_are_extreme(n, ref8):
    """A change of fixture must not hollow the test out: the plane sums of the +-127 columns against planes of -128 are the largest an
    int32 tile of 131 072 rows can hold (0.992 of 2^31), and -128 is 2^31 itself."""
    acc = ref8["every row at q_low"]["acc"]
    assert (ref8["every row at q_low"]["planes"][:HB_ND - 1] == -128).all()
    assert acc[SPECIAL8["all 127"], :6].tolist() == [-127 * 128 * n] * 6 and acc[SPECIAL8["all -127"], :6].tolist() == [127 * 128 * n] * 6
    assert acc[SPECIAL8["all -128"], :6].tolist() == [128 * 128 * n] * 6
    hi = ref8["one row at 1, the others at q_high"]
    assert (hi["planes"][:HB_ND - 1].max(1) == 127).all() and hi["acc"][SPECIAL8["all 127"], 0] == 127 * 127 * (n - 1)
    if n == 131072:
        assert abs(int(acc[SPECIAL8["all 127"], 0])) == abs(int(acc[SPECIAL8["all -127"], 0])) == 2130706432
        assert int(acc[SPECIAL8["all -128"], 0]) == 2 ** 31


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("knobs", list(KNOBS))
def test_tall_dot_products_are_the_integer_restatement(n, knobs, monkeypatch):
    """k_dotq on the int8 context and k_dotq2, k_dotq2r, k_dotq2m on a second one that dropped its int8 copy: bit for bit the restatement,
    and so the same bits on the columns they share; slot 0's digit planes; under the default knobs also the riders (marker_stats,
    download() after pack, drop and unpack, hb_ctx_matvec and matmul, residual_sums). The all -128 column under HB_DOTQ_TILES = 1 at
    n = 131 072 is the finding of DESIGN.md §7: with a cap of 1024 stages its six low plane sums are 2^31 in one tile and wrap."""
    set_env(monkeypatch, KNOBS[knobs])
    X, X8, res, ref2, ref8 = inputs(n)
    the_extreme_sums_are_extreme(n, ref8)
    shared = np.setdiff1d(np.arange(192), sorted(SPECIAL8.values()))
    with H.Context(n, 192, panel=64, precise=2) as c8, H.Context(n, 192, panel=64, precise=2) as c2:
        assert c8.ld == -(-n // 256) * 256
        c8.upload(X8)
        c2.upload(X)
        c2.set_layout(2, keep_int8=False)
        assert c8.layout() == (8, True) and c2.layout() == (2, False)
        wrong = []                                        # everything that differs, so that a failure names every kernel and plane it concerns
        for name, r in res.items():
            c8.set_residual(r, np.zeros(n))
            c2.set_residual(r, np.zeros(n))
            d8 = c8.dot()
            wrong += dots_wrong(d8, ref8[name], (name, "k_dotq"))
            wrong += planes_wrong(c8, n, ref8[name], (name, "int8"))
            for kind in (0, 1, 2):
                c2.set_matvec_kernel(kind)
                d2 = c2.dot()
                wrong += dots_wrong(d2, ref2[name], (name, "2-bit kind %d" % kind))
                if not np.array_equal(u64(d2[shared]), u64(d8[shared])):
                    wrong.append((name, "2-bit kind %d and k_dotq differ on the columns they share" % kind))
            wrong += planes_wrong(c2, n, ref2[name], (name, "2-bit"))
        assert not wrong, (n, knobs, len(wrong), wrong[:12])
        if knobs == "default":
            if n == 262145:
                assert np.array_equal(c2.download(), X), "download() after pack, drop and unpack"
            if n in RIDER_SIZES:
                marker_stats_rider(c8, X8, n)
                for c, Xc, what in ((c8, X8, "int8"), (c2, X, "2-bit")):
                    x_alpha_riders(c, Xc, n, what)
                residual_sums_rider(c8, n)
    print("tall n = %d %s: largest R %d, the restatement at most %.3f of R / 2 ulp from the exact product" % (n, knobs, WORST["R"], WORST["ulps of R/2"]))


@pytest.mark.parametrize("knobs", list(KNOBS))
def test_the_two_bit_kernels_past_the_scaled_accumulators_bound(knobs, monkeypatch):
    """n = 700 001, m = 64: a single tile would hold 700 416 rows, 175 001 of them in the scale-32 accumulator of k_dotq2 and k_dotq2m — the
    all-3 column against planes of -128 sums to 96 x 128 x 175 001 > 2^31 there. plan_matvec's floor of ceil(rows / 131 072) tiles keeps
    them apart under HB_DOTQ2_TILES = 1 too."""
    set_env(monkeypatch, KNOBS[knobs])
    n = TALLEST
    X, _, res, ref2, _ = inputs(n)
    acc = ref2["every row at q_low"]["acc"][SPECIAL2["all 3"]]
    assert acc[:6].tolist() == [-3 * 128 * n] * 6 and -(-n // 4) * 96 * 128 >= 2 ** 31
    with H.Context(n, 64, panel=64, precise=2) as c2:
        c2.upload(X)
        c2.set_layout(2, keep_int8=False)
        wrong = []
        for name, r in res.items():
            c2.set_residual(r, np.zeros(n))
            for kind in (0, 1, 2):
                c2.set_matvec_kernel(kind)
                wrong += dots_wrong(c2.dot(), ref2[name], (name, "2-bit kind %d" % kind))
            wrong += planes_wrong(c2, n, ref2[name], (name, "2-bit"))
        assert not wrong, (n, knobs, len(wrong), wrong[:12])
        if knobs == "default":
            assert np.array_equal(c2.download(), X), "download() after pack, drop and unpack"
    print("tall n = %d %s: largest R %d, at most %.3f of R / 2 ulp" % (n, knobs, WORST["R"], WORST["ulps of R/2"]))


@pytest.mark.parametrize("n", SIZES + (TALLEST,))
@pytest.mark.parametrize("knobs", list(KNOBS))
@pytest.mark.parametrize("shape", Q2M_SHAPES, ids=["-".join("%s%s" % (k[7:], v) for k, v in s.items()) for s in Q2M_SHAPES])
def test_every_shape_of_the_matrix_core_matvec_on_tall_columns(n, knobs, shape, monkeypatch):
    """Every template shape of k_dotq2m (the knobs are read at hb_ctx_create: a context per shape), the restatement bit for bit."""
    set_env(monkeypatch, KNOBS[knobs], shape)
    X, _, res, ref2, _ = inputs(n)
    with H.Context(n, X.shape[1], panel=64, precise=2) as c2:
        c2.upload(X)
        c2.set_layout(2, keep_int8=False)
        c2.set_matvec_kernel(2)
        wrong = []
        for name, r in res.items():
            c2.set_residual(r, np.zeros(n))
            wrong += dots_wrong(c2.dot(), ref2[name], (name,))
        assert not wrong, (n, knobs, shape, len(wrong), wrong[:6])


# ------------------------------------------------------------------------------------------------------------------------
# riders on the same contexts
# ------------------------------------------------------------------------------------------------------------------------
def marker_stats_rider(c8, X8, n):
    """k_stats: xpx = S2 and the numerator n S2 - S1^2 are int64 sums, exact; vx = (double)num / ((double)n (double)(n - 1)) rounds the
    numerator, the denominator and the quotient once each: within 2 ulp of the correctly rounded quotient. nvar0 counts num == 0."""
    xpx, vx, _, nvar0 = c8.marker_stats()
    worst, zero = 0.0, 0
    for j in range(X8.shape[1]):
        col = X8[:, j].astype(np.int64)
        s1, s2 = int(col.sum()), int((col * col).sum())
        assert xpx[j] == s2 and float(s2) == s2, (j, xpx[j], s2)
        num = n * s2 - s1 * s1
        zero += num == 0
        want = float(Fraction(num, n * (n - 1)))
        if num == 0:
            assert vx[j] == 0.0
        else:
            worst = max(worst, abs(vx[j] - want) / float(np.spacing(want)))
    print("tall n = %d marker_stats: vx at most %.2f ulp off (bound 2)" % (n, worst))
    assert worst <= 2.0 and nvar0 == zero and zero >= 5       # (all 3, all 0, all 127, all -127, all -128)


def x_alpha_riders(c, X, n, what):
    """hb_ctx_matvec (k_xalpha: an fma chain over the non-zero effects of a block of 256 columns, the blocks joined by atomic adds in no
    fixed order) and matmul (k_xmat: one fma chain), 12 non-zero effects per record: every one of the at most nnz roundings is half an
    eps of a partial sum that sum |x alpha| bounds, so |err| <= nnz eps sum |x alpha| per row with a factor two to spare. The reference
    is the sum in 80-bit long double (x alpha is exact there; its own error, nnz 2^-64 sum |x alpha|, is taken off the bound)."""
    assert np.finfo(np.longdouble).nmant >= 63
    rng = np.random.default_rng(n + len(what))
    m, nnz = X.shape[1], 12
    special = [j for j in list(SPECIAL2.values()) + list(SPECIAL8.values()) if j < m]

    def record():
        a = np.zeros(m)
        cols = np.concatenate([rng.choice(special, 4, replace=False), rng.choice(np.setdiff1d(np.arange(m), special), nnz - 4, replace=False)])
        a[cols] = rng.normal(0, 1, nnz) * rng.choice([1e-3, 1.0, 1e3], nnz)
        return a

    def reference(a):
        ref, ab = np.zeros(n, dtype=np.longdouble), np.zeros(n, dtype=np.longdouble)
        for j in np.flatnonzero(a):
            t = X[:, j].astype(np.longdouble) * np.longdouble(a[j])
            ref += t
            ab += np.abs(t)
        return ref, ab.astype(np.float64)

    a = record()
    out = np.zeros(n)
    H._lib.check(c.L.hb_ctx_matvec(c.h, a.ctypes.data, out.ctypes.data))
    A = np.stack([record() for _ in range(3)], axis=1)
    got = [out] + list(c.matmul(A).T)
    worst = 0.0
    for g, al in zip(got, [a] + list(A.T)):
        ref, ab = reference(al)
        lim = (nnz * EPS - nnz * 2.0 ** -64) * ab
        err = np.abs(g.astype(np.longdouble) - ref).astype(np.float64)
        assert ((err <= lim) | (ab == 0)).all() and not g[ab == 0].any(), (what, float((err / np.maximum(lim, 1e-300)).max()))
        worst = max(worst, float((err[ab > 0] / lim[ab > 0]).max()))
    print("tall n = %d %s X alpha: at most %.3f of nnz eps sum |x alpha|" % (n, what, worst))


def residual_sums_rider(c8, n):
    """k_reduce_ru with test_gpu_boundary.py's bound: ceil(n / 1024) serial adds per lane, six shuffle levels, sixteen wave sums. sum r
    against math.fsum (exact), sum r^2 against fsum of the rounded squares, whose error of eps / 2 sum r^2 is taken off the bound."""
    rng = np.random.default_rng(n)
    r = 1e3 + rng.normal(size=n)
    c8.set_residual(r, np.zeros(n))
    s1, s2 = c8.residual_sums()
    f = (-(-n // 1024) + 22) * EPS
    sq = r * r
    e1 = abs(s1 - math.fsum(r)) / (f * float(np.abs(r).sum()))
    e2 = abs(s2 - math.fsum(sq)) / ((f - EPS / 2) * float(sq.sum()))
    print("tall n = %d residual_sums: sum r %.3f, sum r^2 %.3f of the bound" % (n, e1, e2))
    assert e1 <= 1.0 and e2 <= 1.0, (e1, e2)


def test_fp64_matvec_on_a_tall_column():
    """precise = 1 (k_dot, fp64 fma chains and a reduction in some order) against the product with the residual as it is, not quantised:
    n roundings of at most half an eps of sum |x r| each, bound n eps sum |x r|. The reference is the 80-bit long double sum (x r is
    exact there: 8 + 53 bits), its own error n 2^-64 sum |x r| taken off the bound."""
    n = 131073
    X, X8, res, _, _ = inputs(n)
    r = res["normal, five rows x 1e6"]
    with H.Context(n, 192, panel=64, precise=1) as c:
        c.upload(X8)
        c.set_residual(r, np.zeros(n))
        d = c.dot()
    rl = r.astype(np.longdouble)
    worst = 0.0
    for j in range(192):
        t = X8[:, j].astype(np.longdouble) * rl
        ab = float(np.abs(t).sum())
        lim = (n * EPS - n * 2.0 ** -64) * ab
        err = float(abs(np.longdouble(d[j]) - t.sum()))
        assert err <= lim and (ab > 0 or d[j] == 0.0), (j, err, lim)
        worst = max(worst, err / lim if ab else 0.0)
    print("tall n = %d fp64 mat-vec: at most %.2e of n eps sum |x r|" % (n, worst))


def test_a_sweep_removes_installed_effects_on_a_tall_column():
    """One pipelined BayesC sweep with pi_1 = 0 at n = 131 073, panel 64, with test_gpu_update.py's own helpers: the update rows apply the
    move lists bit for bit — yadj, u, rows [n, ld) zero, r32, exponent and digit planes are equalities there — on the int8 and on the
    2-bit layout, which agree bit for bit; the dot products after the sweep are the quantised ones."""
    n, panel, geo, counts = 131073, 64, (1, 2, 1), [9, 0, 3]
    m = (len(counts) - 1) * panel + 5
    rng = np.random.default_rng(n)
    X = geno(rng, n, m, "0123")
    r0, u0, gmag = residuals(rng, n, True)
    g0 = install(rng, m, panel, 1, counts, gmag, must=(0, 1))
    memo, first = {}, None
    for layout in (8, 2):
        tag = "tall sweep layout=%d" % layout
        got = run_sweep(tag, X, r0, u0, g0, panel=panel, geo=geo, precise=2, model="BayesC", logpi=[0.0, -INF], layout=layout, nblocks=1, memo=memo)
        assert got["counts"] == counts, (tag, got["counts"])
        assert set(np.concatenate([rg["cols"] for rg in got["ranges"]]).tolist()) == set(np.flatnonzero(g0).tolist()), tag
        if first is None:
            first = got
        else:
            same_bits(tag, first, got, "2-bit against int8")
