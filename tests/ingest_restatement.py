"""Host restatement of the data paths either side of the genotype matrix (hibayes_amd/csrc/hb_ingest.hpp, drivers in hb_ctx.hip), in the
arithmetic the kernels use, so that tests/test_gpu_ingest.py can ask for equal bits. No GPU in here; tests/test_ingest_host.py checks every
function against a literal formulation.

What is exact, and why. k_xalpha's thread walks its block of 256 columns in ascending order, a = 0; a = fma(x_j, alpha_j, a), past every
alpha_j == 0 (a -0.0 included): xalpha_blocks(). The blocks' sums meet in fp64 atomics on a zeroed vector, a zero sum is not sent: with two
blocks a row is fl(p0 + p1) whichever comes first, with three or more the order is free and only a bound holds. k_xmat has no atomics: per
record acc = 0; acc = fma(x_j, A[j, r], acc) over the columns hb_ctx_matmul hands over for the pass of eight records, ascending:
xmat_pass(). Both need fl(a b + c) in one rounding: real_restatement.fma. For the codes -1 .. 2 the product is exact anyway, for 3 and +-127
it is not (3 alpha needs a bit more than alpha has).

What the bounds are measured against: exact_dot(), the exactly rounded X a through Python integers and fractions.Fraction.

bed_image() writes a PLINK .bed image from genotype codes, with the unused bit pairs of each marker's last byte as the caller wants them;
bed_markers() is the list of crafted markers both test files decode."""
from fractions import Fraction

import numpy as np

from real_restatement import fma

NA = -128                        # hibayes_amd.plink.NA_CHAR, the oracle's code for a missing call
MAGIC = bytes([0x6C, 0x1B, 0x01])
XA_BLOCK = 256                   # columns per block of k_xalpha
XM_RB = 8                        # records per pass of hb_ctx_matmul


# ------------------------------------------------------------------------------------------------------------------------
# k_xalpha
# ------------------------------------------------------------------------------------------------------------------------
def xalpha_blocks(X, alpha, m_pad, block=XA_BLOCK):
    """k_xalpha's partial sums: out[b, i] = the chain a = 0; a = fma(X[i, j], alpha[j], a) over the columns j of block b (j in [b block,
    min(m_pad, (b + 1) block)), ascending, alpha[j] == 0 skipped; columns at and past m carry no effect). X: n x m integer codes, alpha: m
    doubles. Returns (ceil(m_pad / block), n) doubles."""
    X = np.asarray(X)
    alpha = np.asarray(alpha, dtype=np.float64)
    n, m = X.shape
    nb = (m_pad + block - 1) // block
    out = np.zeros((nb, n))
    for b in range(nb):
        a = np.zeros(n)
        for j in range(b * block, min(m_pad, m, (b + 1) * block)):
            if alpha[j] == 0.0:
                continue
            a = fma(X[:, j].astype(np.float64), float(alpha[j]), a)
        out[b] = a
    return out


# ------------------------------------------------------------------------------------------------------------------------
# hb_ctx_matmul's pass, k_xmat
# ------------------------------------------------------------------------------------------------------------------------
def xmat_pass(X, A, r0):
    """The pass of records r0 .. min(R, r0 + 8) - 1 of X @ A (A: m x R). Returns (support, out): support = the columns with a non-zero in
    any record of the pass, ascending (hb_ctx_matmul's rule; a -0.0 is no non-zero), out[:, k] = acc = 0; acc = fma(X[:, j], A[j, r0 + k],
    acc) over the support — the entries that are zero in that record are walked too."""
    X = np.asarray(X)
    A = np.asarray(A, dtype=np.float64)
    n = X.shape[0]
    recs = range(r0, min(A.shape[1], r0 + XM_RB))
    support = np.flatnonzero((A[:, list(recs)] != 0.0).any(axis=1))
    out = np.zeros((n, len(recs)))
    cols = [X[:, j].astype(np.float64) for j in support]
    for k, r in enumerate(recs):
        acc = np.zeros(n)
        for x, j in zip(cols, support):
            acc = fma(x, float(A[j, r]), acc)
        out[:, k] = acc
    return support, out


# ------------------------------------------------------------------------------------------------------------------------
# the exactly rounded product
# ------------------------------------------------------------------------------------------------------------------------
def exact_dot(X, a):
    """fl(X a), one rounding per row: X integer codes (n x m), a finite doubles (m). Every a_j is an integer over a power of two; over
    their common denominator the row sums are Python integers, and int / int rounds to nearest even."""
    X = np.asarray(X)
    a = np.asarray(a, dtype=np.float64)
    n = X.shape[0]
    nz = np.flatnonzero(a != 0.0)
    if nz.size == 0:
        return np.zeros(n)
    fr = [Fraction(float(a[j])) for j in nz]
    den = max(f.denominator for f in fr)
    num = np.array([f.numerator * (den // f.denominator) for f in fr], dtype=object)
    s = np.dot(X[:, nz].astype(np.int64).astype(object), num)
    return np.array([float(Fraction(int(v), den)) for v in s], dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------------
# .bed images
# ------------------------------------------------------------------------------------------------------------------------
_BED_CODE = {2: 0, NA: 1, 1: 2, 0: 3}    # genotype -> the file's bit pair (00 -> 2, 01 -> NA, 10 -> 1, 11 -> 0)


def bed_image(G, nind, tail_bits):
    """A SNP-major PLINK .bed image, magic bytes included, of G (nind x nsnp codes 0 / 1 / 2 / NA): individual i of marker j in bits
    2 (i & 3) of byte i >> 2 of the marker's ceil(nind / 4) bytes. tail_bits (0 .. 3) is the bit pair written to the unused positions of each
    marker's last byte: 0 reads as genotype 2 and 1 as a missing call to a decoder that looks past nind."""
    G = np.asarray(G)
    assert G.shape[0] == nind and 0 <= tail_bits <= 3
    nsnp = G.shape[1]
    bpc = (nind + 3) // 4
    codes = np.full((bpc * 4, nsnp), tail_bits, dtype=np.uint8)
    for g, code in _BED_CODE.items():
        codes[:nind][G == g] = code
    assert np.isin(G, list(_BED_CODE)).all()
    c4 = codes.reshape(bpc, 4, nsnp)
    body = (c4[:, 0] | (c4[:, 1] << 2) | (c4[:, 2] << 4) | (c4[:, 3] << 6)).astype(np.uint8)      # bpc x nsnp
    return MAGIC + np.ascontiguousarray(body.T).tobytes()


def _tied_pair(k):
    """(a, c): 2 a + c == k, a > c >= 0, c as large as it goes"""
    for c in range(k, -1, -1):
        if (k - c) % 2 == 0 and (k - c) // 2 > c:
            return (k - c) // 2, c
    raise ValueError(k)


BED_NSNP = 12
# what the crafted markers impute to (None: the marker has no missing call or is left to the decoders' agreement)
BED_MAJOR = [None, 0, 1, 0, 0, 0, None, 2, 1, None, 2, None]


def bed_markers(nind, inside, outside, seed):
    """nind x 12 genotype codes, the crafted markers of the .bed tests. inside: an individual that the test's row list selects, outside: at
    least one that it does not. A tie needs the other calls to split evenly: each tied marker has one missing call where nind allows it and
    the fewest otherwise, the first of them at `inside` so that the imputed value is downloaded.
      0   no missing call                          6   missing calls only at `outside`
      1   counts 0 = 1 > 2 (imputes 0)             7   2 the major genotype, missing at `inside` and `outside`
      2   counts 1 = 2 > 0 (imputes 1)             8   1 the major genotype, one missing call
      3   counts 0 = 2 > 1 (imputes 0)             9   random calls, a quarter missing
      4   all three equal (imputes 0)              10  every call 2 but the one missing
      5   every call missing (imputes 0)           11  no missing call"""
    rng = np.random.default_rng(seed)
    outside = np.atleast_1d(outside)
    G = np.zeros((nind, BED_NSNP), dtype=np.int8)

    def place(j, counts, nmiss):
        """marker j: counts[g] calls of genotype g and nmiss missing ones, `inside` missing, the rest shuffled"""
        assert sum(counts) + nmiss == nind and nmiss >= 1
        rest = np.array([0] * counts[0] + [1] * counts[1] + [2] * counts[2] + [NA] * (nmiss - 1), dtype=np.int8)
        rng.shuffle(rest)
        G[np.arange(nind) != inside, j] = rest
        G[inside, j] = NA

    G[:, 0] = rng.integers(0, 3, nind)
    a, c = _tied_pair(nind - 1)
    place(1, (a, a, c), 1)
    place(2, (c, a, a), 1)
    place(3, (a, c, a), 1)
    nm = 1 + (nind - 1) % 3
    place(4, ((nind - nm) // 3,) * 3, nm)
    G[:, 5] = NA
    G[:, 6] = rng.integers(0, 3, nind)
    G[:, 6][outside] = NA
    G[:, 7] = 2
    few = (nind - 2) // 4                    # (nind - 2 - few calls of 2 at the least: more than few at every nind >= 5)
    G[rng.choice(nind, few, replace=False), 7] = rng.integers(0, 2, few)
    G[inside, 7] = NA
    G[outside[0], 7] = NA
    k = nind - 1
    place(8, (k // 4, k - 2 * (k // 4), k // 4), 1)
    G[:, 9] = rng.integers(0, 3, nind)
    G[rng.random(nind) < 0.25, 9] = NA
    G[:, 10] = 2
    G[inside, 10] = NA
    G[:, 11] = rng.integers(0, 3, nind)
    return G


def impute_major(G):
    """The reference's rule, marker by marker, as a literal loop: counts of 0, 1, 2 over all individuals; the major genotype starts at 0 with
    a count of 0 and is replaced only by a strictly larger count, taken in the order 0, 1, 2; every missing call becomes it."""
    G = np.array(G, dtype=np.int8)
    for j in range(G.shape[1]):
        best, major = 0, 0
        for g in (0, 1, 2):
            cnt = sum(1 for v in G[:, j] if v == g)
            if cnt > best:
                best, major = cnt, g
        for i in range(G.shape[0]):
            if G[i, j] == NA:
                G[i, j] = major
    return G
