"""ldmat() (reference R/ldm.r:31-112) without a GPU: the numpy restatement the GPU tests compare against is pinned to a literal
loop of the reference's arithmetic, and the host part of hibayes_amd.ldmat() — argument rules, error texts, chromosome
relabelling — is checked; the device part must refuse loudly where there is no device."""
import os

import numpy as np
import pytest

import hibayes_amd as H
from hibayes_amd import ldmat
from hibayes_amd.ldm import chromosome_ids, ldmat_mode
from ldmat_restatement import big_stat, ldmat_restatement

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def literal(X, chisq=None, chr=None):
    """tXXmat_Geno / tXXmat_Chr as loops over scalars (src/tXXmat.cpp:124-184, :527-604), dense output."""
    X = np.asarray(X)
    n, m = X.shape
    ind = n
    s, mean, xx = np.zeros(m), np.zeros(m), np.zeros(m)
    for j in range(m):
        p1 = 0.0
        for k in range(n):
            p1 += float(X[k, j])
        s[j], mean[j] = p1, p1 / ind
    for j in range(m):
        p1 = 0.0
        for k in range(n):
            d = float(X[k, j]) - mean[j]
            p1 += d * d
        xx[j] = np.sqrt(p1)
    out = np.zeros((m, m))
    sparse = (chisq is not None) if chr is not None else (chisq is not None and chisq > 0)
    blocks = [np.arange(m)] if chr is None else [np.flatnonzero(np.asarray(chr) == c) for c in np.unique(chr)]
    for ix in blocks:
        for a in range(len(ix)):
            j = ix[a]
            p1, m1, sum1 = xx[j], mean[j], s[j]
            if not sparse:
                out[j, j] = p1 * p1 / ind
            for b in range(a if sparse else a + 1, len(ix)):
                i = ix[b]
                p2, m2, sum2 = xx[i], mean[i], s[i]
                p12 = 0.0
                for k in range(n):
                    p12 += float(X[k, i]) * float(X[k, j])
                p12 -= sum1 * m2 + sum2 * m1 - ind * m1 * m2
                if sparse:
                    with np.errstate(invalid="ignore", divide="ignore"):
                        r = np.float64(p12) / np.float64(p1 * p2)
                    if r * r * ind <= chisq:
                        continue
                out[i, j] = out[j, i] = p12 / ind
    return out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(3)
    X = rng.integers(0, 3, (8, 7)).astype(np.int8)
    X[:, 2] = 1                                   # monomorphic
    X[:, 4] = rng.integers(-1, 2, 8)              # -1 / 0 / 1
    X[0, 4], X[1, 4] = -1, 1
    return X


@pytest.mark.parametrize("chisq,chr", [(None, None), (0.7, None), (None, [1, 2, 1, 2, 2, 1, 1]), (0.0, [1, 2, 1, 2, 2, 1, 1]),
                                       (0.7, [1, 2, 1, 2, 2, 1, 1])])
def test_restatement_equals_a_literal_loop_bit_for_bit(small, chisq, chr):
    got, want = ldmat_restatement(small, chisq, chr), literal(small, chisq, chr)
    assert same_bits(got, want)
    assert np.array_equal(got, got.T)
    if chisq is not None:
        assert (got == 0).any() and (got != 0).any()


def test_restatement_is_the_population_covariance_on_the_demo():
    X = H.read_plink(os.path.join(G, "demo", "demo"))["geno"]
    ld = ldmat_restatement(X)
    assert ld.shape == (1000, 1000) and np.abs(ld - np.cov(X.astype(np.float64), rowvar=False, ddof=0)).max() < 1e-12
    s, mean, xx = big_stat(X)
    assert int((xx == 0).sum()) == int((X == X[0]).all(axis=0).sum())     # the monomorphic markers
    sp = ldmat_restatement(X, chisq=5.0)
    assert 0 < np.count_nonzero(sp) < sp.size


def test_argument_rules_and_error_texts():
    names = ["s%d" % i for i in range(5)]
    tab = lambda chrs, snp=names: [[s, c, 100 * i] for i, (s, c) in enumerate(zip(snp, chrs))]
    assert ldmat_mode(5) == (None, None)                                            # no map: genome-wide dense
    assert ldmat_mode(5, chisq=-1.0) == (None, None)                                # R/ldm.r:44-46
    assert ldmat_mode(5, chisq=0.0) == (None, None)                                 # :78-80
    assert ldmat_mode(5, chisq=5.0) == (None, 5.0)
    assert ldmat_mode(5, tab([1, 1, 1, 1, 1]), chisq=0.0) == (None, None)           # :51-54 one chromosome
    assert ldmat_mode(5, tab([1, 1, 1, 1, 1]), chisq=2.0, ldchr=False) == (None, 2.0)
    c, q = ldmat_mode(5, tab([1, 2, 1, 2, 2]), chisq=0.0)                           # chisq = 0 stays with several chromosomes
    assert list(c) == [1, 2, 1, 2, 2] and q == 0.0
    c, q = ldmat_mode(5, tab([1, 2, 1, 2, 2]), ldchr=True)
    assert c is None and q is None
    c, q = ldmat_mode(5, tab(["1", "X", "2", "Y", "X"]))
    assert list(c) == [1, 3, 2, 4, 3] and q is None
    assert list(chromosome_ids(["X", "Y", "X"])) == [1, 2, 1]                       # max.chr = 0 (:67)
    assert list(ldmat_mode(5, {"SNP": names, "Chr": ["2", "2", "7", "MT", "7"], "Pos": [1, 2, 3, 4, 5]})[0]) == [2, 2, 7, 8, 7]
    for bad, msg in [(tab([1, 2, 1, 2, 2], ["a", "b", "a", "c", "d"]), "Same SNPs names detected."),
                     (tab([1, None, 1, 2, 2]), "NAs are not allowed in chromosome."),
                     (tab([1, "NA", 1, 2, 2]), "NAs are not allowed in chromosome."),
                     (tab([1, 0, 1, 2, 2]), "0 is not allowed in chromosome.")]:
        with pytest.raises(ValueError) as ei:
            ldmat(np.zeros((4, 5), dtype=np.int8), bad)
        assert str(ei.value) == msg
    with pytest.raises(ValueError, match="Same SNPs names detected."):
        ldmat(np.zeros((4, 5), dtype=np.int8), tab([1, 2, 1, 2, 2]), gwas_geno=np.zeros((4, 2), dtype=np.int8),
              gwas_map=[["a", 1, 1], ["a", 1, 2]])
    with pytest.raises(NotImplementedError):
        ldmat(np.zeros((4, 5), dtype=np.int8), tab([1, 2, 1, 2, 2]), gwas_geno=np.zeros((4, 5), dtype=np.int8), gwas_map=tab([1, 2, 1, 2, 2]))
    with pytest.raises(ValueError):
        ldmat(np.zeros((4, 6), dtype=np.int8), tab([1, 2, 1, 2, 2]))


def test_sbrm_and_sbayesd_take_the_handle_type():
    assert hasattr(H, "LDMatrix") and hasattr(H.Context, "ldmat")
    from hibayes_amd import _lib
    assert {"hb_ldm_build", "hb_ldm_info", "hb_ldm_download_dense", "hb_ldm_download_csc", "hb_ldm_destroy", "hb_sbayes_run_ldm"} <= set(_lib.SYMBOLS)


def test_without_a_device_the_call_refuses_loudly():
    if H.lib().hb_device_count() > 0:
        return                                    # a device is present: tests/test_gpu_ldmat.py covers the call
    X = H.read_plink(os.path.join(G, "demo", "demo"))["geno"][:, :64]
    with pytest.raises(H.HibayesError, match="no HIP device available") as ei:
        ldmat(X)
    assert ei.value.status == 2
    with pytest.raises(H.HibayesError, match="no HIP device available"):
        ldmat(X.astype(np.float64), chisq=5.0, keep_on_device=True)
