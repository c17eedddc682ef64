"""Every device and pinned allocation has an owner that frees it (hibayes_amd/csrc/hb_bufs.hpp): the library's count of what it holds
(engine.live_buffers) is back where it was after a context's whole life, after every handle, and after refusals that allocate first. Every
comparison is with the count at the start of the test — a session fixture may hold a context —, never with the device's free memory, which
other processes move."""
import ctypes as C

import numpy as np
import pytest

import hibayes_amd as H
from hibayes_amd import _lib
from hibayes_amd import eig as HE
from hibayes_amd.engine import Context, live_buffers
from hibayes_amd.grm import grm_build_device
from hibayes_amd.impute import ImputeSystem
from hibayes_amd.ldm import LDMatrix

from test_epsl_host import tridiagonal
from test_impute_host import ss_demo  # noqa: F401  (the demo's single-step system, as tests/test_gpu_impute.py uses it)

pytestmark = pytest.mark.gpu


def twice(call):
    """the same call again leaves the count exactly where the first left it: what it replaced was freed"""
    call()
    first = live_buffers()
    call()
    assert live_buffers() == first, (call, first, live_buffers())
    return first


def one_life(y, M):
    n, m = M.shape
    rng = np.random.default_rng(11)
    start = live_buffers()
    c = Context(n, m, panel=512)  # (panel 512: the one at which a band wider than the default geometry's exists)
    created = live_buffers()
    assert created[0] > start[0] + 40 and created[1] > start[1] + n * m
    twice(lambda: c.upload(M))
    assert live_buffers() == created

    # layouts: the 2-bit copy comes, the int8 columns go, come back and go again
    def layouts():
        c.set_layout(2, keep_int8=False)
        assert c.layout() == (2, False)
        c.set_layout(8)
        assert c.layout() == (8, True)
        c.set_layout(2, keep_int8=False)
    two_bit_only = twice(layouts)
    assert two_bit_only[0] == created[0] and two_bit_only[1] < created[1]  # (X2 for X: one buffer for one, a quarter of the bytes)
    c.set_layout(8)
    assert live_buffers()[0] == created[0] + 1

    def real_and_back():
        c.upload_real(M.astype(np.float64))
        assert c.layout()[0] == 64 and live_buffers()[0] == created[0] + 2
        c.upload(M)  # integer genotypes over real ones: the fp64 columns go
        assert c.layout()[0] == 8
    assert twice(real_and_back)[0] == created[0] + 1

    # the band: built, built again, and regrown for a wider geometry
    c.set_pipeline(1, 2, 7)  # (the geometry a context is created with; the fp64 layout had left it on the per-panel kernels)
    band = c.pipeline()[3]
    assert band == 20
    built = twice(c.build_gram)
    c.set_pipeline(1, 3, 7)
    assert c.pipeline()[3] > band, (band, c.pipeline())
    wider = twice(c.build_gram)
    assert wider[0] == built[0] and wider[1] > built[1]  # (the old band was freed: as many buffers, more bytes)
    c.set_pipeline(1, 2, 7)

    # a short run on the context: the snapshot buffer comes with the first sweep and stays
    before_run = live_buffers()
    run = lambda: H.Bayes(y, None, "BayesCpi", [0.95, 0.05], niter=10, nburn=4, thin=1, verbose=False, ctx=c, genotype_bits=8)  # noqa: E731
    after_run = twice(run)
    assert after_run[0] >= before_run[0] + 1

    # covariates, levels, the blocks' state, windows
    c.set_covariates(rng.normal(size=(n, 2)))
    two = live_buffers()
    three = twice(lambda: c.set_covariates(rng.normal(size=(n, 3))))
    assert three == (two[0], two[1] + 8 * n)
    nlev = [3, 5]
    zid = np.column_stack([rng.integers(0, k, n) for k in nlev])
    twice(lambda: c.set_levels(zid, nlev))
    twice(lambda: c.blocks_setup(np.ones(3), np.ones(sum(nlev)), np.ones(len(nlev))))
    twice(lambda: c.set_windows(1 + np.arange(m) // 50))

    # the profiling switches that allocate: cycle stamps of the chain (bit 1, kept), block stamps of the mat-vec launches (bit 3, freed when off)
    def profiling():
        c.set_profiling(2 | 8)
        on = live_buffers()
        c.set_profiling(0)
        assert live_buffers() == (on[0] - 1, on[1] - 16 * 4608 * (c.m // 512 + (c.m % 512 != 0) + 1))
    twice(profiling)

    # the polygenic and the epsilon block
    Kival, Ki = np.linspace(0.1, 2.0, n), np.asfortranarray(np.linalg.qr(rng.normal(size=(n, n)))[0])
    poly = twice(lambda: c.poly_setup(Kival, Ki))
    assert c.L.hb_ctx_poly_setup(c.h, None, None, 0, 0) == 0  # (drops the block)
    assert live_buffers()[0] < poly[0]
    c.poly_setup(Kival, Ki)
    assert live_buffers() == poly
    G = tridiagonal(50)
    twice(lambda: c.epsl_setup(rng.normal(size=n), G, 1 + np.arange(40) % 50))

    assert live_buffers()[0] > created[0]
    c.close()
    assert live_buffers() == start


def test_a_contexts_whole_life_twice(demo):
    y, M = demo["y"], np.asfortranarray(demo["M"])
    assert M.shape[0] == 300 and M.shape[1] <= 1200 and M.dtype == np.int8
    for _ in range(2):
        one_life(y, M)


def test_every_handle_gives_back_what_it_took(demo, ss_demo):  # noqa: F811
    M = np.asfortranarray(demo["M"][:, :256])
    n, m = M.shape
    rng = np.random.default_rng(12)
    start = live_buffers()
    with Context(n, m) as c:
        c.upload(M)
        held = live_buffers()
        # ldmat(): the genome-wide dense matrix and a sparsified one, each read from its device copy by a solver before it goes
        sumstat = np.column_stack([np.full(m, 0.3), rng.normal(0, 0.01, m), np.full(m, 0.05), np.full(m, 1000.0)])
        with c.ldmat() as dense:
            assert dense.kind == "dense" and live_buffers()[0] > held[0]
            assert dense.toarray().shape == (m, m)
            assert np.all(np.isfinite(H.conjgt_den(sumstat, dense, lambda_=np.full(m, 10.0), verbose=False)["g"]))
        assert live_buffers() == held
        with c.ldmat(chisq=3.0) as sparse:
            assert sparse.kind != "dense" and live_buffers()[0] > held[0]
            assert sparse.tocsc().shape == (m, m)
            assert np.all(np.isfinite(H.conjgt_spa(sumstat, sparse, lambda_=np.full(m, 10.0), verbose=False)["g"]))
        assert live_buffers() == held
        # make_grm() with its matrix left on the device, and with the eigenvectors left there
        with grm_build_device(c, 0.01) as Gd:
            assert live_buffers() == (held[0] + 1, held[1] + 8 * n * n)
            G = Gd.toarray()
        assert live_buffers() == held
        with H.make_grm(c, 0.01, eigen=True, verbose=False, eigen_solver="device", keep_on_device=True, tridiagonal="device") as K:
            assert live_buffers()[0] == held[0] + 1 and K.values.shape == (n,)
        assert live_buffers() == held
    assert live_buffers() == start
    # hb_ldm_from_csc
    with LDMatrix.from_scipy(tridiagonal(64)) as L:
        assert L.shape == (64, 64)
        assert np.all(np.isfinite(H.conjgt_spa(sumstat[:64], L, lambda_=np.full(64, 10.0), verbose=False)["g"]))
        assert live_buffers()[0] > start[0]
    assert live_buffers() == start
    # eigh() with every stage on the device: the uploaded matrix, the reduction's handle, Z and its workspace all go; K stays until it is released
    A = G[:96, :96]
    K = H.eigh(A, keep_on_device=True, tridiagonal="device")
    assert live_buffers() == (start[0] + 1, start[1] + 8 * 128 * 128)
    assert np.allclose(K.values, np.linalg.eigvalsh(A), rtol=0, atol=1e-10 * np.abs(A).max())
    K.close()
    assert live_buffers() == start
    # the imputation's system
    with ImputeSystem(ss_demo["Ann"], ss_demo["Ang"]) as S:
        assert live_buffers()[0] > start[0]
        mid = live_buffers()
        x, st = S.solve(ss_demo["M"][:, :64], 1e-12, 2000)
        assert np.all(np.isfinite(x)) and live_buffers() == mid  # (a solve's buffers are its own)
    assert live_buffers() == start
    # spd_inverse(): the status word, the block column and the work copy of one call
    B = rng.normal(size=(64, 80))
    Sm = B @ B.T + 64 * np.eye(64)
    assert np.allclose(H.spd_inverse(Sm) @ Sm, np.eye(64), rtol=0, atol=1e-10)
    assert live_buffers() == start


def test_refusals_that_allocate_first_leave_nothing_behind():
    """each request is far beyond any card: refused by the allocation itself, before a kernel is launched"""
    L = H.lib()
    start = live_buffers()
    with HE.upload(np.eye(2)) as D:  # the 8 TB work copy of tests/test_gpu_chol.py
        held = live_buffers()
        info = C.c_int32(-1)
        assert L.hb_spd_inverse(D.ptr, 1000000, 1000000, 0, 0.0, C.byref(info)) == 3 and "out of memory" in L.hb_last_error().decode()
        assert "hb_spd_inverse" in L.hb_last_error().decode() and " GB" in L.hb_last_error().decode()
        assert live_buffers() == held
    assert live_buffers() == start
    # hb_eig_upload allocates before it reads the host matrix: 8 TB for n = 10^6
    A, p, ld = np.eye(2, order="F"), C.c_void_p(), C.c_int64()
    assert L.hb_eig_upload(A.ctypes.data, 10 ** 6, 10 ** 6, 0, C.byref(p), C.byref(ld)) == 3
    text = L.hb_last_error().decode()
    assert "hb_eig_upload" in text and "out of memory" in text and "8000.0 GB" in text and not p.value
    assert live_buffers() == start
    # hb_ctx_create: 1.1 TB of int8 columns (2^31 - 256 rows, one panel of 512 columns)
    par = _lib.CtxParams(device=0, n=2 ** 31 - 256, m=1, panel=512, precise=2, m_offset=0, seed=1)
    h = C.c_void_p()
    assert L.hb_ctx_create(C.byref(par), C.byref(h)) == 3 and "out of memory" in L.hb_last_error().decode() and not h.value
    assert live_buffers() == start
    with Context(300, 64) as c:  # and an ordinary context still works
        X = (np.arange(300 * 64).reshape(300, 64) % 3).astype(np.int8)
        c.upload(X)
        xpx = c.marker_stats()[0]
        assert np.array_equal(xpx, (X.astype(np.float64) ** 2).sum(axis=0))
    assert live_buffers() == start
