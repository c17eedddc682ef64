"""tests/opening_restatement.py against its own properties, on the CPU: the numpy restatements tests/test_gpu_opening.py holds the device's
certificate, opening filter and row-cache lists against must themselves be what they claim — a bound that bounds, a float that lies below,
a list whose slots lie inside the cache. Also the inputs the GPU file shares (wide_codes, tie_columns), and the plan-level fact behind the
two places that size the row cache."""
import os
import subprocess

import numpy as np
import pytest

import opening_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_WIDE = 133143          # one below the largest n the Gram's range check admits for codes of +-127: 127^2 n = 2 147 463 447, 127^2 (n + 2) > 2^31 - 1


def wide_codes():
    """64 columns of +-127 at n = N_WIDE. Six are patterned: two of all +127 and one of all -127 (|ga gB| at its largest, 66051 * 32512),
    a column b of alternating signs (sum +127: ga = 0, so the whole of b . b' stays in c), its copy and its negative (c = +-127^2 n, the largest
    entry the Gram admits); the rest are random signs."""
    rng = np.random.default_rng(133143)
    X = (127 * (2 * rng.integers(0, 2, size=(N_WIDE, 64), dtype=np.int8) - 1)).astype(np.int8)
    b = np.where(np.arange(N_WIDE) % 2 == 0, 127, -127).astype(np.int8)
    X[:, 3], X[:, 40], X[:, 17] = 127, 127, -127
    X[:, 9], X[:, 33], X[:, 50] = b, b, -b
    return np.asfortranarray(X)


def tie_columns(n, m):
    """0/1/2 columns at n = 512 with prescribed sums: s 256 / n = s / 2 is an exact tie for every odd sum (40 of them here), and the sums 128,
    384 and 640 are exact ties of s / 256; one monomorphic column of 0 and one of 2."""
    rng = np.random.default_rng(512)
    sums = rng.integers(1, 2 * n, size=m)
    sums[:40] = 2 * rng.integers(0, n - 1, size=40) + 1
    sums[40:45] = [128, 384, 640, 0, 2 * n]
    X = np.zeros((n, m), dtype=np.int8)
    for j, s in enumerate(sums):
        col = np.zeros(n, dtype=np.int8)
        col[:s // 2] = 2
        if s % 2:
            col[s // 2] = 1
        X[:, j] = rng.permutation(col)
    assert np.array_equal(X.sum(axis=0, dtype=np.int64), sums)
    return np.asfortranarray(X), sums


def brute_cert(X, P, Lg, n):
    """the definition, pair by pair, in Python integers"""
    Xp = R.padded(X, P).astype(object)
    m_pad = Xp.shape[1]
    s = [int(v) for v in Xp.sum(axis=0)]
    ga, gB = R.cert_reference(X, P, Lg, n)[:2]
    cm = []
    for k in range(m_pad):
        hi = min(m_pad, (k // P + Lg + 1) * P)
        cm.append(max([abs(int(Xp[:, k] @ Xp[:, j]) - int(ga[k]) * int(gB[j])) for j in range(k // P * P, hi) if j != k], default=0))
    return s, cm


@pytest.mark.parametrize("signed", [False, True])
def test_cert_reference_is_the_definition(signed):
    rng = np.random.default_rng(5)
    n, P, Lg = 700, 8, 2
    X = rng.binomial(2, rng.uniform(0.01, 0.99, 29), size=(n, 29)).astype(np.int64) - (1 if signed else 0)
    X[:, 4] = X[:, 3]
    ga, gB, gcmax = R.cert_reference(X, P, Lg, n)
    s, cm = brute_cert(X, P, Lg, n)
    assert gcmax.tolist() == cm and max(cm) < R.INT32_MAX
    # rint, ties to even, from the definition of a nearest integer: |ga 256 - s| <= 128 and |gB n - 256 s| <= n / 2, in integers
    for j, sj in enumerate(s):
        assert abs(int(ga[j]) * 256 - sj) <= 128 and 2 * abs(int(gB[j]) * n - 256 * sj) <= n
    assert not gcmax[29:].any() and not gB[29:].any() and not ga[29:].any()          # padding
    # every stored pair is inside the bound, from either end of the pair's row
    G = R.cross(R.padded(X, P), R.padded(X, P))
    for k in range(32):
        for j in range(k // P * P, min(32, (k // P + Lg + 1) * P)):
            if j != k:
                assert abs(int(G[k, j]) - int(ga[k]) * int(gB[j])) <= gcmax[k]
    # the band matters: a narrower one leaves out pairs, and the bound can only grow with it
    narrow = R.cert_reference(X, P, 0, n)[2]
    assert (narrow <= gcmax).all() and (narrow < gcmax).any()


def test_cert_reference_at_the_edge_of_int32():
    X = wide_codes()
    assert 127 * 127 * N_WIDE < R.INT32_MAX < 127 * 127 * (N_WIDE + 2)
    ga, gB, gcmax = R.cert_reference(X, 64, 0, N_WIDE)
    assert int(gcmax.max()) == 2147463447 == 127 * 127 * N_WIDE        # b against its copy and its negative: ga[b] = 0
    assert gcmax[9] == gcmax[33] == gcmax[50] == 2147463447 and ga[9] == 0 and ga[50] == 0
    prod = np.abs(ga[:, None] * gB[None, :])
    assert int(prod.max()) == 2147450112 == 66051 * 32512 and ga[3] == 66051 and gB[17] == -32512
    # the clamp is never reached: the Gram's own range check keeps |G| below 2^31, and where |ga gB| is large G has its sign
    G = R.cross(X.astype(np.int64), X.astype(np.int64))
    c = np.abs(G - ga[:, None] * gB[None, :])
    np.fill_diagonal(c, 0)
    assert int(c.max()) == 2147463447 < R.INT32_MAX and np.array_equal(c.max(axis=1), gcmax)


def test_cert_reference_rounds_ties_to_even():
    n = 512
    X, sums = tie_columns(n, 64 * 3 + 17)
    ga, gB, _ = R.cert_reference(X, 64, 1, n)
    assert (sums % 2 == 1).sum() >= 32
    for j, s in enumerate(sums):
        s = int(s)
        if s % 2:                                   # s / 2 is a tie: the even neighbour
            assert gB[j] in (s // 2, s // 2 + 1) and gB[j] % 2 == 0
        else:
            assert gB[j] == s // 2
    assert ga[40:45].tolist() == [0, 2, 2, 0, 4] and gB[40:45].tolist() == [64, 192, 320, 0, 512]


def test_filter_reference_is_the_largest_float_not_above():
    rng = np.random.default_rng(11)
    f32 = rng.normal(0, 30, 50).astype(np.float32).astype(np.float64)             # exact floats stay
    thr0 = np.concatenate([rng.normal(0, 50, 4000), 10.0 ** rng.uniform(-30, 30, 2000), -10.0 ** rng.uniform(-30, 30, 2000), f32,
                           np.nextafter(f32, np.inf), np.nextafter(f32, -np.inf), [0.0, -0.0, np.inf, 1e300, -1e300, 3.5e38, -3.5e38]])
    m = thr0.size
    vx, g = np.ones(m), np.zeros(m)
    vx[5::17], g[3::13] = 0.0, 0.25
    gB = rng.integers(-2 ** 31, 2 ** 31, m)
    f, opn = R.filter_reference(thr0, vx, g, 0.64, gB)
    mono, inm = vx == 0, (vx != 0) & (g != 0)
    plain = ~mono & ~inm
    assert f.dtype == np.float32 and np.isnan(f[mono]).all() and np.isneginf(f[inm]).all()
    assert (f[mono].view(np.int32) == 0x7fc00000).all()
    fd, t = f[plain].astype(np.float64), thr0[plain]
    assert (fd <= t).all()
    with np.errstate(over="ignore"):
        above = np.nextafter(f[plain], np.float32(np.inf)).astype(np.float64)
    assert ((above > t) | np.isposinf(fd)).all()                                   # no float in between
    k = np.flatnonzero(plain)[np.isin(t, f32)]
    assert k.size >= 40 and np.array_equal(f[k].astype(np.float64), thr0[k])       # an exact float is kept
    assert (fd < t).sum() > 3000 and (t < 0).sum() > 1000
    # the records: the threshold the chain compares, the word, gB
    thc = np.ascontiguousarray(opn[:, 0:2]).view(np.float64).ravel()
    assert (thc[inm] == -1.0).all() and np.isnan(thc[mono]).all() and np.array_equal(thc[plain], np.where(np.isneginf(fd), -1.0, 0.64 * fd))
    assert np.array_equal(opn[:, 2], f.view(np.int32)) and np.array_equal(opn[:, 3], gB.astype(np.int32))
    assert R.float_below(np.array([1e300]))[0] == np.finfo(np.float32).max and np.isposinf(R.float_below(np.array([np.inf]))[0])
    assert np.isneginf(R.float_below(np.array([-1e300]))[0])


PANELS = [64, 128, 256, 512]


def panel_cases(P, nslot):
    """one panel per pattern, and after them a panel whose first half is monomorphic, its second half hot"""
    pats = R.hot_patterns(P, nslot)
    hot = np.concatenate(list(pats.values()) + [np.arange(P) >= P // 2])
    active = np.ones(hot.size, dtype=bool)
    active[-P:-P // 2] = False
    active[hot.size - 2 * P + 7] = False       # ("all": one monomorphic marker among the hot ones' places)
    return list(pats) + ["first-half-monomorphic"], active, hot & active


@pytest.mark.parametrize("P", PANELS)
def test_hotlist_reference_keeps_its_own_invariants(P):
    for nslot in (1, 2, P // 4, P):
        names, active, hot = panel_cases(P, nslot)
        slot_of, lists, head = R.hotlist_reference(active, hot, P, nslot)
        bad = R.check_lists(slot_of, lists, head, active, hot, P, nslot)
        if R.fits_the_list(P, nslot):
            assert bad == [], (P, nslot, bad[:3])
        else:
            # a cache of more rows than the list can name — more than the device's LDS holds (fits_the_list) —: the layout as documented gives
            # places beyond the list, and nothing else goes wrong
            assert bad and all(": 3. " in b for b in bad), (P, nslot, bad[:3])
        U = max(P // 64, 1)
        for p, name in enumerate(names):
            sl, h, k = slot_of[p * P:(p + 1) * P], head[p], int(hot[p * P:(p + 1) * P].sum())
            assert h[1] == min(k, R.LIST_MAX) and len(lists[p]) == h[1]
            assert (sl >= 0).sum() >= min(h[0], k) and h[0] <= (2 * nslot if P == 512 else nslot)
            if name == "none":                                       # (no whole row: panel 512 reports its shift all the same)
                assert h.tolist() == [0, 0, 0, 1 if P == 512 else 0] and (sl == -1).all()
            if name == "at-half" and P == 512:                       # the shifted layout: base 0, the piece at [U/2, U)
                assert h.tolist() == [1, 1, 0, 1] and sl[P // 2] == 0
            if name == "at-half-1" or (name == "at-half" and P != 512):
                assert h.tolist() == [1, 1, 1, 0] and sl.max() == 0
            if name in ("nslot", "nslot+1", "all") and P != 512:     # whole rows only: the first nslot hot markers, side by side
                first = np.flatnonzero(hot[p * P:(p + 1) * P])[:nslot]
                assert np.array_equal(np.flatnonzero(sl >= 0), first) and sl[first].tolist() == [i * U for i in range(first.size)]
            if name == "first-half-monomorphic":
                assert (sl[:P // 2] == -2).all() and (sl[P // 2:] >= -1).all() and h[3] == (1 if P == 512 else 0)


def test_check_lists_notices_what_the_chain_could_not_survive():
    P, nslot = 512, 8
    names, active, hot = panel_cases(P, nslot)
    slot_of, lists, head = R.hotlist_reference(active, hot, P, nslot)
    assert R.check_lists(slot_of, lists, head, active, hot, P, nslot) == []
    p = names.index("at-half")
    s = slot_of.copy()
    s[p * P + P // 2] = -4                                           # the unshifted base of a lone half row
    assert any(": 2. " in b for b in R.check_lists(s, lists, head, active, hot, P, nslot))
    p = names.index("all")
    s = slot_of.copy()
    s[p * P + 1] = s[p * P]                                          # two rows in one place
    assert any("overlap" in b for b in R.check_lists(s, lists, head, active, hot, P, nslot))
    s = slot_of.copy()
    s[p * P + 300] = nslot * 8 - 4                                   # a piece that ends beyond the cache
    assert any("outside" in b for b in R.check_lists(s, lists, head, active, hot, P, nslot))
    h = head.copy()
    h[p, 0] -= 1                                                     # a row with a place that the fill leaves out
    assert any(": 3. " in b for b in R.check_lists(slot_of, lists, h, active, hot, P, nslot))
    h = head.copy()
    h[names.index("at-half"), 3] = 0
    assert any(": 4. " in b for b in R.check_lists(slot_of, lists, h, active, hot, P, nslot))
    s = slot_of.copy()
    s[len(names) * P - P + 3] = -1                                   # a monomorphic marker the chain would not skip
    assert any(": 5. " in b for b in R.check_lists(s, lists, head, active, hot, P, nslot))


PLAN_WALK = r"""
#include "hb_plan.hpp"
#include <cstdio>
int main()
{
    long seen = 0, persist = 0, wide = 0;
    for (int model = 1; model <= 6; model++) for (int nf = 2; nf <= (model == 6 ? 8 : 2); nf++)
    for (int P = 64; P <= 512; P *= 2) for (int Lv = 0; Lv <= 4; Lv++) for (int D = 1; D <= 8; D++) for (int L = 0; L <= 40; L++)
    for (int bits = 0; bits < 32; bits++) {
        const hb_sweep_plan p = plan_sweep(hb_sweep_shape{model, nf, P, Lv, D, L, (bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) != 0, (bits & 16) != 0});
        seen++;
        if (!p.ok) continue;
        if (L > HB_LBMAX) wide++;
        if (p.chain == HB_CHAIN_PERSIST) {
            persist++;
            if (L > HB_LBMAX) { printf("per-panel chain at band %d: model %d P %d Lv %d D %d\n", L, model, P, Lv, D); return 1; }
        }
    }
    printf("%ld %ld %ld\n", seen, persist, wide);
    return 0;
}
"""


def test_the_per_panel_chain_never_runs_beyond_the_band_its_lists_are_sized_for(tmp_path):
    """enqueue_sweep_pipeline sizes the row cache twice: k_hotlist's lists for the band min(L, HB_LBMAX), the per-panel chain's LDS for L. The two
    are one number wherever that chain runs: plan_sweep gives a band beyond HB_LBMAX to the group chain only (which has no row cache). Every
    input of the plan, bands beyond any geometry included."""
    src = tmp_path / "walk.cpp"
    src.write_text(PLAN_WALK)
    exe = tmp_path / "walk"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "hibayes_amd", "csrc"), str(src), "-o", str(exe)])
    seen, persist, wide = (int(v) for v in subprocess.check_output([str(exe)]).split())
    assert persist > 1000 and wide > 0 and seen > persist
