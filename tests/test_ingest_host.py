"""tests/ingest_restatement.py against literal formulations, without a GPU: xalpha_blocks and xmat_pass against scalar loops of exact
rational fused multiply-adds, their sums against the exactly rounded product, exact_dot against fractions.Fraction, bed_image against a
decoder written out bit by bit, and the two host .bed decoders against the reference's imputation rule on the crafted markers."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ingest_restatement as I
from real_restatement import fma_fraction

from hibayes_amd import plink
from oracle import oracle as O

EPS = 2.0 ** -52
CODES = [-127, -1, 0, 1, 2, 3, 127]
BED_NIND = [5, 6, 7, 8, 255, 1003]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def case_9x40():
    """9 x 40 with every code of CODES in every row; effects of very different sizes, a -0.0 and a denormal among them"""
    rng = np.random.default_rng(940)
    X = rng.choice(CODES, size=(9, 40)).astype(np.int8)
    for i in range(9):
        X[i, rng.permutation(40)[:len(CODES)]] = CODES
    alpha = rng.normal(size=40) * 10.0 ** rng.integers(-8, 9, 40)
    alpha[rng.choice(40, 12, replace=False)] = 0.0
    alpha[5], alpha[6] = -0.0, 1e-310
    assert all((X == c).any() for c in CODES)
    return rng, X, alpha


def scalar_chain(xs, coefs, skip_zero):
    a = 0.0
    for x, al in zip(xs, coefs):
        if skip_zero and al == 0.0:
            continue
        a = fma_fraction(float(x), float(al), a)
    return a


@pytest.mark.parametrize("block", [16, 256])
def test_xalpha_blocks_against_a_scalar_loop(block):
    rng, X, alpha = case_9x40()
    if block == 256:                                   # the kernel's own block: 3 x 300, two blocks, the second ragged at m_pad = 320
        X = rng.choice(CODES, size=(3, 300)).astype(np.int8)
        alpha = np.zeros(300)
        alpha[rng.choice(300, 30, replace=False)] = rng.normal(size=30)
    n, m = X.shape
    m_pad = -(-m // 64) * 64
    got = I.xalpha_blocks(X, alpha, m_pad, block=block)
    nb = -(-m_pad // block)
    assert got.shape == (nb, n)
    for b in range(nb):
        js = range(b * block, min(m, (b + 1) * block))
        want = [scalar_chain([X[i, j] for j in js], [alpha[j] for j in js], True) for i in range(n)]
        assert np.array_equal(bits(got[b]), bits(want)), b
    # their sum against the exactly rounded product: a term goes through at most nnz roundings
    nnz = int((alpha != 0).sum())
    lim = nnz * EPS * (np.abs(X.astype(np.float64)) @ np.abs(alpha))
    assert np.all(np.abs(got.sum(0) - I.exact_dot(X, alpha)) <= lim)
    assert not I.xalpha_blocks(X, np.zeros(m), m_pad, block=block).any()


def test_xmat_pass_against_a_scalar_loop():
    rng, X, alpha = case_9x40()
    n, m = X.shape
    R = 11
    A = np.zeros((m, R))
    for r in range(R):
        j = rng.choice(m, 6, replace=False)
        A[j, r] = rng.normal(size=6) * 10.0 ** rng.integers(-6, 7, 6)
    A[3, 2] = -0.0                                      # no non-zero: column 3 enters a support only through another record
    A[:, 9] = 0.0                                       # an empty record inside the second pass
    for r0 in (0, 8):
        recs = list(range(r0, min(R, r0 + 8)))
        support, out = I.xmat_pass(X, A, r0)
        want_support = [j for j in range(m) if any(A[j, r] != 0.0 for r in recs)]
        assert support.tolist() == want_support and out.shape == (n, len(recs))
        for k, r in enumerate(recs):
            want = [scalar_chain([X[i, j] for j in want_support], [A[j, r] for j in want_support], False) for i in range(n)]
            assert np.array_equal(bits(out[:, k]), bits(want)), r
            lim = max(1, len(support)) * EPS * (np.abs(X.astype(np.float64)) @ np.abs(A[:, r]))
            assert np.all(np.abs(out[:, k] - I.exact_dot(X, A[:, r])) <= lim)
            # a record alone: its own support is smaller, the zeros the pass walks change no bit (acc + 0 x = acc, and acc is never -0.0)
            s1, o1 = I.xmat_pass(X, A[:, r:r + 1], 0)
            assert set(s1) <= set(support) and np.array_equal(bits(o1[:, 0]), bits(out[:, k]))
    assert not I.xmat_pass(X, A, 8)[1][:, 1].any()
    s0, o0 = I.xmat_pass(X, np.zeros((m, 8)), 0)
    assert s0.size == 0 and o0.shape == (n, 8) and not o0.any()


def test_exact_dot_is_the_rounded_rational_sum():
    rng, X, alpha = case_9x40()
    got = I.exact_dot(X, alpha)
    want = [float(sum(Fraction(int(x)) * Fraction(float(a)) for x, a in zip(X[i], alpha))) for i in range(X.shape[0])]
    assert np.array_equal(bits(got), bits(want))
    # a sum that numpy's doubles lose: 127 * 1e16 + 3 * 1.0 - 127 * 1e16
    assert I.exact_dot(np.array([[127, 3, -127]]), np.array([1e16, 1.0, 1e16]))[0] == 3.0
    assert I.exact_dot(np.array([[1, 2]]), np.array([5e-324, 1e-310]))[0] == 2e-310 + 5e-324
    z = I.exact_dot(X, np.zeros(40))
    assert not z.any() and not np.signbit(z).any()


def literal_decode(img, nind, nsnp):
    """the image read bit pair by bit pair: 00 -> 2, 01 -> NA, 10 -> 1, 11 -> 0"""
    bpc = (nind + 3) // 4
    G = np.zeros((nind, nsnp), dtype=np.int8)
    for j in range(nsnp):
        for i in range(nind):
            code = (img[3 + j * bpc + (i >> 2)] >> (2 * (i & 3))) & 3
            G[i, j] = (2, I.NA, 1, 0)[code]
    return G


@pytest.mark.parametrize("nind", BED_NIND)
def test_bed_image_and_the_two_host_decoders_on_the_crafted_markers(nind):
    """bed_image() round-trips through a literal decoder, with the unused bit pairs of each marker's last byte as asked for. Then
    hibayes_amd.plink.decode_bed and oracle.decode_bed on the crafted markers of bed_markers(), against the reference's rule restated as a
    literal loop (impute_major: counts in the order 0, 1, 2, a strict >, the major genotype starting at 0 — so the lowest code wins a tie and
    a marker that is missing everywhere becomes 0).

    Found: the two host decoders agree with each other and with that rule on every listed case — nind = 5, 6, 7, 8, 255 and 1003; no missing
    call; counts tied 0 = 1 > 2, 1 = 2 > 0, 0 = 2 > 1 and all three equal (imputed 0, 1, 0, 0); every call missing (imputed 0); majors 1 and 2;
    and the unused bit pairs all 00 or all 01, which change nothing. No disagreement was found."""
    G = I.bed_markers(nind, inside=1, outside=[nind - 1, nind - 2], seed=nind)
    bpc = (nind + 3) // 4
    want = I.impute_major(G)
    # the markers are what their list says
    assert not (G[:, [0, 11]] == I.NA).any() and (G[:, 5] == I.NA).all()
    assert set(np.flatnonzero(G[:, 6] == I.NA)) == {nind - 1, nind - 2}
    cnt = lambda j: [int((G[:, j] == g).sum()) for g in (0, 1, 2)]
    c1, c2, c3, c4 = cnt(1), cnt(2), cnt(3), cnt(4)
    assert c1[0] == c1[1] > c1[2] and c2[1] == c2[2] > c2[0] and c3[0] == c3[2] > c3[1] and c4[0] == c4[1] == c4[2] > 0
    assert all(int((G[:, j] == I.NA).sum()) == 1 for j in (1, 2, 3, 8, 10)) and int((G[:, 4] == I.NA).sum()) == 1 + (nind - 1) % 3
    for j, major in enumerate(I.BED_MAJOR):
        if major is not None:
            assert G[1, j] == I.NA and want[1, j] == major, j
    images = [I.bed_image(G, nind, tail) for tail in (0, 1)]
    assert len(images[0]) == 3 + bpc * I.BED_NSNP
    if nind % 4:
        assert images[0] != images[1]
        for tail, img in zip((0, 1), images):
            last = np.frombuffer(img, dtype=np.uint8)[3:].reshape(I.BED_NSNP, bpc)[:, -1]
            for k in range(nind % 4, 4):
                assert np.all((last >> (2 * k)) & 3 == tail)
    else:
        assert images[0] == images[1]
    for img in images:
        assert np.array_equal(literal_decode(img, nind, I.BED_NSNP), G)
        for impute, ref in ((False, G), (True, want)):
            a = plink.decode_bed(img, nind, I.BED_NSNP, impute=impute)
            b = O.decode_bed(img, nind, I.BED_NSNP, impute=impute)
            assert np.array_equal(a, ref), (nind, impute, "plink.decode_bed")
            assert np.array_equal(b, ref), (nind, impute, "oracle.decode_bed")
    # a partial image: the first eight markers decode alone
    assert np.array_equal(plink.decode_bed(images[0][:3 + bpc * 8], nind, 8), want[:, :8])


def test_bed_image_refuses_what_is_no_genotype():
    with pytest.raises(AssertionError):
        I.bed_image(np.full((5, 1), 3, dtype=np.int8), 5, 0)
