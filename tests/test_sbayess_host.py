"""The sparse summary-level sampler (SBayesS(), reference src/SBayesS.cpp) without a GPU: the Python restatement the GPU tests
compare against (tests/sbayess_restatement.py) is pinned bit for bit to the C oracle of SBayesD() where the two samplers coincide,
varediff on a hand-made matrix, and the refusals of SBayesS() / sbrm(sparse_ld=True) / hb_ldm_from_csc that need no device."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import hibayes_amd as H
from oracle import oracle as O
from sbayess_restatement import arma_sum, sbayess_restatement, varediff_of
from test_oracle_sbayes import MODELS, sdemo  # noqa: F401  (fixture)


def full_csc(ld):
    """every entry stored, exact zeros included: nnz(column) = m, varediff = 0"""
    m = ld.shape[0]
    return sp.csc_matrix((np.asfortranarray(ld).ravel(order="F").copy(), np.tile(np.arange(m, dtype=np.int32), m),
                          np.arange(0, m * m + 1, m, dtype=np.int64)), shape=(m, m))


@pytest.mark.parametrize("model,Pi,fold", MODELS)
def test_restatement_equals_the_c_oracle_on_a_fully_stored_matrix(sdemo, model, Pi, fold):
    """With every entry stored varei = 0 * vara_ + vare_ = vare_ exactly and a move updates every row, and on the demo nothing is
    redrawn: SBayesS() is then SBayesD() operation for operation, so the records must agree in every bit — no tolerance."""
    ss, ld = sdemo["ss"], sdemo["ld"]
    A = full_csc(ld)
    assert A.nnz == 10 ** 6 and not varediff_of(A).any()
    kw = dict(fold=fold, niter=24, nburn=8, thin=4, seed=97)
    r = sbayess_restatement(ss, A, model, Pi, **kw)
    assert r["redraws"] == 0 and r["zeroed"] == 0
    ref = O.sbayes(ss, ld, model, Pi, rng=O.RNG_PHILOX, store_alpha=True, **kw)
    assert r["n_records"] == ref["n_records"] == 4 and r["n"] == ref["n"] and r["count_y"] == ref["count_y"] and r["nzct"] == ref["nzct"]
    for k in ("s_alpha", "s_Vg", "s_Ve", "s_pi", "r_hat", "g_last", "pip"):
        assert np.array_equal(r[k], ref[k]), k
    assert np.any(r["s_alpha"] != 0)


def test_varediff_and_the_interleaved_sum_on_a_hand_made_matrix():
    A = np.array([[2.0, 0.5, 0.0, 0.0, 0.1],
                  [0.5, 1.0, 0.0, 0.0, 0.0],
                  [0.0, 0.0, 0.0, 0.0, 0.0],      # a monomorphic marker: an empty column
                  [0.0, 0.0, 0.0, 3.0, 0.25],
                  [0.1, 0.0, 0.0, 0.25, 1.5]])
    S = sp.csc_matrix(A)
    np.testing.assert_array_equal(np.diff(S.indptr), [3, 2, 0, 2, 3])
    np.testing.assert_array_equal(varediff_of(S), [(5 - 3) / 5, (5 - 2) / 5, 1.0, (5 - 2) / 5, (5 - 3) / 5])   # :140 (m - j) / m
    assert not varediff_of(full_csc(A)).any()                                  # stored zeros count as entries
    assert arma_sum([1e16, 1.0, -1e16, 1.0]) == (1e16 - 1e16) + (1.0 + 1.0)


def test_refusals_that_need_no_device():
    ss8, eye = np.zeros((5, 8)), sp.identity(5, format="csc")
    with pytest.raises(NotImplementedError, match="sparse ldm.*sparse_ld=True"):     # the default route still refuses scipy sparse
        H.sbrm(ss8, eye, "BayesCpi")
    with pytest.raises(ValueError, match="sparse_ld=True needs a scipy sparse ldm or an LDMatrix"):
        H.sbrm(ss8, np.eye(5), "BayesCpi", sparse_ld=True)
    with pytest.raises(NotImplementedError, match="CG"):
        H.sbrm(ss8, eye, "CG", sparse_ld=True)
    with pytest.raises(ValueError, match="bad setting for collecting frequency 'thin'."):
        H.sbrm(ss8, eye, "BayesCpi", niter=10, nburn=8, thin=5, sparse_ld=True)
    with pytest.raises(ValueError, match="SBayesS needs an LDMatrix or a scipy sparse ldm"):
        H.SBayesS(np.zeros((5, 4)), np.eye(5), "BayesCpi", [0.95, 0.05])
    with pytest.raises(ValueError, match="square scipy sparse matrix"):
        H.LDMatrix.from_scipy(sp.csc_matrix(np.ones((3, 4))))
    # hb_ldm_from_csc validates before it looks for a device: a status and a text
    L, h = H.lib(), C.c_void_p()
    def from_csc(indptr, indices, data, m=3):
        ip, ix, dv = np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int32), np.array(data, dtype=np.float64)
        rc = L.hb_ldm_from_csc(m, ip.ctypes.data, ix.ctypes.data, dv.ctypes.data, 0, C.byref(h))
        return rc, L.hb_last_error().decode()
    assert from_csc([0, 2, 3, 4], [1, 0, 0, 2], [1.0, 1.0, 1.0, 1.0]) == (1, "hb_ldm_from_csc: row indices must be sorted and unique inside a column")
    assert from_csc([0, 2, 3, 4], [0, 0, 0, 2], [1.0, 1.0, 1.0, 1.0])[1] == "hb_ldm_from_csc: row indices must be sorted and unique inside a column"
    assert from_csc([0, 2, 3, 4], [0, 3, 0, 2], [1.0, 1.0, 1.0, 1.0]) == (1, "hb_ldm_from_csc: row index out of range")
    assert from_csc([0, 2, 1, 4], [0, 1, 0, 2], [1.0, 1.0, 1.0, 1.0]) == (1, "hb_ldm_from_csc: indptr must not decrease")
    sym = "hb_ldm_from_csc: the matrix must equal its transpose, in pattern and in value bits"
    assert from_csc([0, 2, 3, 4], [0, 1, 1, 2], [1.0, 0.5, 1.0, 1.0]) == (1, sym)                       # (1, 0) without (0, 1)
    assert from_csc([0, 2, 4, 5], [0, 1, 0, 1, 2], [1.0, 0.5, np.nextafter(0.5, 1), 1.0, 1.0]) == (1, sym)   # one bit apart
    assert not h.value
    if L.hb_device_count() == 0:                                              # a valid matrix, no device: refused loudly
        with pytest.raises(H.HibayesError, match="no HIP device available"):
            H.SBayesS(np.zeros((5, 4)), eye, "BayesCpi", [0.95, 0.05], niter=4, nburn=2, thin=1, verbose=False)
