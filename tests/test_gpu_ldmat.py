"""ldmat() on the MI355X (hb_ldm_build: k_ld_stats, k_ld_strip, k_ld_compact) against the numpy restatement of the reference's
arithmetic (tests/ldmat_restatement.py). Every comparison is exact — np.array_equal on the int64 views: the cross-products are
exact integers and every later step is one correctly rounded fp64 operation in the same order on both sides, so a differing bit
would be a fused or reordered operation in the kernel's epilogue."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import hibayes_amd as H
from ldmat_restatement import big_stat, ldmat_restatement
from test_oracle_sbayes import sdemo  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    ok = a.shape == b.shape and np.array_equal(bits(a), bits(b))
    if not ok and a.shape == b.shape:
        print("mismatching entries: %d of %d, max abs diff %g" % (int((bits(a) != bits(b)).sum()), a.size, np.nanmax(np.abs(a - b))))
    return ok


def same_csc(got, dense_ref):
    want = sp.csc_matrix(dense_ref)
    want.eliminate_zeros()
    want.sort_indices()
    assert isinstance(got, sp.csc_matrix) and got.shape == want.shape
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
    assert np.array_equal(bits(got.data), bits(want.data))
    for j in (0, got.shape[0] // 2, got.shape[0] - 1):                       # rows sorted inside a column
        assert np.all(np.diff(got.indices[got.indptr[j]:got.indptr[j + 1]]) > 0)
    return True


@pytest.fixture(scope="module")
def geno():
    X = H.read_plink(os.path.join(G, "demo", "demo"))["geno"]              # 600 x 1000 int8: ld = 768, four column tiles, the last 232 wide
    assert X.shape == (600, 1000) and X.dtype == np.int8
    return X


@pytest.fixture(scope="module")
def ref(geno):
    """the restatement's matrices on the demo genotypes, computed once"""
    chrs = ["X" if j in (5, 333, 334, 999) else str(j * 7 % 3 + 1) for j in range(1000)]
    ids = H.ldm.chromosome_ids(chrs)
    return {"dense": ldmat_restatement(geno), "sp5": ldmat_restatement(geno, 5.0), "chr": chrs, "ids": ids,
            "blk": ldmat_restatement(geno, None, ids), "blk0": ldmat_restatement(geno, 0.0, ids), "blk5": ldmat_restatement(geno, 5.0, ids)}


@pytest.fixture(scope="module")
def signed():
    """n = 257 (255 padding rows: ind must be 257), m = 513 (a last tile of one column), codes -1 / 0 / 1, markers in LD blocks
    (a column copies its predecessor with probability 0.9 per individual), two constant columns"""
    rng = np.random.default_rng(11)
    n, m = 257, 513
    X = np.zeros((n, m), dtype=np.int8)
    X[:, 0] = rng.integers(-1, 2, n)
    for j in range(1, m):
        fresh = rng.integers(-1, 2, n)
        X[:, j] = np.where(rng.random(n) < 0.9, X[:, j - 1], fresh)
    X[:, 100] = -1
    X[:, 512] = 1
    return np.asfortranarray(X)


def test_demo_dense_genome_wide_default_strip_and_three_strips(geno, ref):
    assert int((big_stat(geno)[2] == 0).sum()) == int((geno == geno[0]).all(axis=0).sum()) > 0    # monomorphic columns are in
    got = H.ldmat(geno)
    assert isinstance(got, np.ndarray) and got.flags.f_contiguous
    assert same(got, ref["dense"])
    with H.ldmat(geno, strip_bytes=1, keep_on_device=True) as ld:
        st = ld.info()
        assert st["n_strips"] >= 3 and st["kind"] == 0 and st["nnz"] == 10 ** 6 and ld.shape == (1000, 1000)
        assert same(ld.toarray(), ref["dense"])


@pytest.mark.parametrize("chisq", [None, 3.84])
def test_signed_codes_padding_rows_and_a_one_column_tile(signed, chisq):
    want = ldmat_restatement(signed, chisq)
    got = H.ldmat(signed, chisq=chisq)
    if chisq is None:
        assert same(got, want)
    else:
        assert same_csc(got, want) and 0 < got.nnz < want.size
    got3 = H.ldmat(signed, chisq=chisq, strip_bytes=1)                       # three strips, the last one column wide
    assert same(got3 if chisq is None else got3.toarray(), want)


def test_demo_sparse_genome_wide(geno, ref):
    got = H.ldmat(geno, chisq=5.0)
    assert same_csc(got, ref["sp5"])
    s, mean, xx = big_stat(geno)
    d = got.diagonal()
    keep = d != 0
    assert keep.sum() > 900 and np.array_equal(bits(d[keep]), bits(np.diag(ref["sp5"])[keep]))
    assert (d[keep] != ((xx * xx) / 600.0)[keep]).any()                      # the cross-product value, not xx^2 / ind
    assert same_csc(H.ldmat(geno, chisq=5.0, strip_bytes=1), ref["sp5"])


@pytest.mark.parametrize("chisq,key", [(None, "blk"), (0.0, "blk0"), (5.0, "blk5")])
def test_chromosome_blocks_with_interleaved_ids(geno, ref, chisq, key):
    mp = [["snp%d" % j, c, 1000 + j] for j, c in enumerate(ref["chr"])]
    got = H.ldmat(geno, mp, chisq=chisq, ldchr=False, strip_bytes=1)
    assert same_csc(got, ref[key])
    ids = ref["ids"]
    coo = got.tocoo()
    assert np.all(ids[coo.row] == ids[coo.col])                              # no entry across chromosomes
    assert len(set(ids)) == 4


def test_two_bit_resident_without_the_int8_copy(geno, ref, monkeypatch):
    with H.Context(600, 1000) as c:
        c.upload(geno)
        c.set_layout(2, keep_int8=False)
        assert c.layout() == (2, False)
        with c.ldmat() as ld:
            assert same(ld.toarray(), ref["dense"])
        monkeypatch.setenv("HB_LDM_WINDOW_COLS", "256")                      # the capacity path: operand columns unpacked a window at a time
        with c.ldmat(strip_bytes=1) as ld:
            assert same(ld.toarray(), ref["dense"])
        with c.ldmat(chr=ref["ids"], chisq=5.0, strip_bytes=1) as ld:
            assert same_csc(ld.tocsc(), ref["blk5"])


def test_from_a_bed_file_on_the_device(geno, ref):
    raw = open(os.path.join(G, "demo", "demo.bed"), "rb").read()
    with H.Context(600, 1000) as c:
        c.upload_bed(raw, 600)
        assert same(H.ldmat(c), ref["dense"])


@pytest.mark.parametrize("model,Pi,fold", [("BayesCpi", [0.95, 0.05], None), ("BayesR", [0.95, 0.02, 0.02, 0.01], [0, 1e-4, 1e-3, 1e-2])])
def test_sampler_from_the_handle(geno, sdemo, model, Pi, fold):
    kw = dict(fold=fold, niter=12, nburn=4, thin=2, seed=2468, verbose=False)
    for chisq in (None, 5.0):
        with H.ldmat(geno, chisq=chisq, keep_on_device=True) as ld:
            a = H.SBayesD(sdemo["ss"], ld, model, Pi, **kw)
            b = H.SBayesD(sdemo["ss"], ld.toarray(), model, Pi, **kw)
        for k in ("alpha", "pi", "Vg", "Ve"):
            assert np.array_equal(a["MCMCsamples"][k], b["MCMCsamples"][k]), k
        assert np.any(a["MCMCsamples"]["alpha"] != 0)


def test_refusals_carry_a_status_and_a_text():
    with H.Context(300, 64) as c:                                            # nothing uploaded
        with pytest.raises(H.HibayesError, match="no genotypes on the device") as ei:
            c.ldmat()
        assert ei.value.status == 1
    n = 133200                                                               # 127^2 * n >= 2^31
    X = np.zeros((n, 2), dtype=np.int8, order="F")
    X[0, 0], X[1, 1] = 127, 1
    with H.Context(n, 2) as c:
        c.upload(X)
        with pytest.raises(H.HibayesError, match="genotype codes too large for the exact int32 Gram matrix at this n") as ei:
            c.ldmat()
        assert ei.value.status == 4
