"""The host restatements tests/test_gpu_update.py compares the update rows with, checked on their own (no GPU): emulate_update against an
all-Fraction evaluation of the same recurrence, digits_of against the carry cases of the quantiser tests, fix_exp at its edges."""
import math
from fractions import Fraction

import numpy as np

from test_gpu_update import HB_ND, LIST_CASES, digits_of, emulate_update, fix_exp, install, move_class, quantised_dots, ragged_panel


def fraction_update(X, r, u, groups):
    """a = 0; a = fl(x d + a) per move; r = fl(r - a); u = fl(u + a) where the list is non-empty — every fl() through float(Fraction)"""
    r, u = [float(v) for v in r], [float(v) for v in u]
    versions = []
    for cols, deltas in groups:
        a = [0.0] * len(r)
        for j, d in zip(cols, deltas):
            a = [float(Fraction(int(X[i, j])) * Fraction(float(d)) + Fraction(a[i])) for i in range(len(r))]
        r = [float(Fraction(r[i]) - Fraction(a[i])) for i in range(len(r))]
        if len(cols):
            u = [float(Fraction(u[i]) + Fraction(a[i])) for i in range(len(r))]
        versions.append(np.array(r))
    return np.array(r), np.array(u), versions


def test_emulate_update_is_the_fma_recurrence():
    """n = 8, 40 moves in four groups (one of them empty), codes 0..3 with an all-3 column among the moved, changes over twelve orders of
    magnitude so that most additions round: bit for bit the all-Fraction evaluation."""
    rng = np.random.default_rng(5)
    n, m = 8, 24
    X = rng.integers(0, 4, size=(n, m)).astype(np.int8)
    X[:, 3] = 3
    r, u = rng.normal(size=n), rng.normal(size=n)
    cols = rng.permutation(np.repeat(np.arange(m), 2))[:40]
    cols[0] = 3
    dl = rng.normal(size=40) * 10.0 ** rng.uniform(-6, 6, size=40)
    groups = [(cols[:17], dl[:17]), (cols[:0], dl[:0]), (cols[17:18], dl[17:18]), (cols[18:], dl[18:])]
    assert (X[:, cols] == 3).sum() > 40
    got, want = emulate_update(X, r, u, groups), fraction_update(X, r, u, groups)
    assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64))
    assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))
    assert len(got[2]) == 4 and all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(got[2], want[2]))
    assert np.array_equal(got[2][0], got[2][1]) and not np.array_equal(got[2][1], got[2][2])     # the empty group changes nothing
    # ... and it is not the unfused recurrence: with code 3 the product rounds on its own
    plain_r = r.copy()
    for cs, ds in groups:
        a = np.zeros(n)
        for j, d in zip(cs, ds):
            a = a + X[:, j].astype(np.float64) * d
        plain_r = plain_r - a
    assert not np.array_equal(plain_r, got[0])


def test_digits_of_at_the_carries():
    """the qs of test_gpu_kernels._digit_edge_residuals, both signs: 0x80 in every byte is digit -128 and a carry seven times over, 0x7f the
    largest digit without one; the digits recombine to q, the lower six lie in [-128, 127], the top one too while |q| < 2^54 + 2^47"""
    qs = [0x1f808080808080, 0x1f7f7f7f7f7f7f, 0x007f7f7f7f7f7f, 0x00808080808080, 0x1fffffffffffff, 0x00ffffffffff80]
    for q in qs + [-q for q in qs] + [0, 1, -1, 127, 128, -128, -129, 2 ** 54 - 2, -(2 ** 54 - 2), 2 ** 53, -2 ** 53]:
        d = digits_of(q)
        assert len(d) == HB_ND and sum(v << (8 * k) for k, v in enumerate(d)) == q, q
        assert all(-128 <= v <= 127 for v in d), (q, d)
    assert digits_of(0x00808080808080) == [-128, -127, -127, -127, -127, -127, 1]
    assert digits_of(0x007f7f7f7f7f7f) == [127] * 6 + [0]
    assert digits_of(0x1fffffffffffff) == [-1, 0, 0, 0, 0, 0, 32]
    assert digits_of(-129) == [127, -1, 0, 0, 0, 0, 0]
    assert digits_of(2 ** 55)[-1] == 128                    # what no longer fits shows in the top digit


def test_fix_exp_at_its_edges():
    assert fix_exp(0.0) == 0 and fix_exp(float("inf")) == 0 and fix_exp(float("nan")) == 0 and fix_exp(1e300) == 0
    for b in (1.0, np.nextafter(2.0, 0.0), 2.0, 1e-3, 2.5e3, 2.0 ** -1000, 2.0 ** 900 / 3):
        E = fix_exp(float(b))
        if abs(E) < 900:
            assert 2.0 ** 53 <= math.ldexp(float(b), E) < 2.0 ** 54, b
    assert fix_exp(2.0 ** -1000) == 900 and fix_exp(1e299) == -900 and fix_exp(2.0 ** 100) == -47


def test_quantised_dots_is_the_big_integer_product():
    rng = np.random.default_rng(2)
    X = rng.integers(-1, 4, size=(37, 11)).astype(np.int8)
    r = rng.normal(size=37) * 1e3
    E = fix_exp(float(np.abs(r).max()))
    want = [math.ldexp(float(sum(int(x) * int(np.rint(np.ldexp(v, E))) for x, v in zip(X[:, j], r))), -E) for j in range(11)]
    got, small = quantised_dots(X, r)
    assert np.array_equal(got, np.array(want)) and small.all()


def test_the_case_table_installs_what_it_lists():
    """install() puts counts[h] effects into launch group h, the last group's into the ragged last panel, and the classes are the batch and
    pass boundaries of update_rows"""
    assert [move_class(k) for k in (0, 1, 8, 9, 32, 33, 64, 65, 448, 449, 896, 897)] == \
        ["0", "1..8", "1..8", "9..32", "9..32", "33..64", "33..64", "65..448", "65..448", "449..896", "449..896", ">=897"]
    rng = np.random.default_rng(0)
    for name, n, panel, geo, codes, layouts, precise, counts, blocks, small_r in LIST_CASES:
        D = geo[2] if geo[0] else 1
        m = (len(counts) - 1) * D * panel + (panel if D > 1 else 0) + ragged_panel(panel)
        g = install(rng, m, panel, D, counts, 1e3, must=(0, 1) if codes == "0123" else ())
        nz = np.flatnonzero(g)
        assert [int(((nz >= h * D * panel) & (nz < (h + 1) * D * panel)).sum()) for h in range(len(counts))] == counts, name
        assert (nz[nz >= (len(counts) - 1) * D * panel] >= m - ragged_panel(panel)).all() and np.abs(g).max() == 1e3, name
        assert codes != "0123" or (g[0] != 0 and g[1] != 0), name
