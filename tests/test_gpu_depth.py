"""Parity where the bench runs: the DEFAULT pipeline geometries at pipeline depth.

The round-1 goldens (m <= 1000) give at most two mat-vec groups, so the fused update row, the residual version
ping-pong, the wrap of the LDS correction ring and the band blocks l >= 2 never ran under an oracle comparison.
Here: >= 10 mat-vec groups at D = 7 (64 panels of 512, and 64 panels of 64), draw-for-draw against the live oracle
under the same Philox counters, from a cold start and from a dense installed state; every band Gram block against
int64 numpy; pipeline vs serial kernels at the BASELINE size. Reference loop: src/Bayes.cpp:627-717, :743-815."""
import numpy as np
import pytest

import hibayes_amd as H
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def geno(rng, n, m):
    p = rng.uniform(0.05, 0.5, m)
    X = np.empty((n, m), dtype=np.int8, order="F")
    for j0 in range(0, m, 4096):
        pj = p[j0:j0 + 4096]
        X[:, j0:j0 + 4096] = (rng.random((n, pj.size)) < pj).astype(np.int8) + (rng.random((n, pj.size)) < pj).astype(np.int8)
    X[:, 7::997] = 1                      # monomorphic markers: skipped by the sweep (src/Bayes.cpp:589)
    return X


def pheno(rng, X, ncausal=40):
    n, m = X.shape
    idx = rng.choice(m, ncausal, replace=False)
    xb = X[:, idx].astype(np.float64) @ rng.normal(0, 1, ncausal)
    xb *= np.sqrt(0.5 / xb.var())
    return xb + rng.normal(0, np.sqrt(0.5), n)


CASES = [  # model, Pi, fold, expected default geometry (pipeline, look-ahead groups, panels per mat-vec)
    ("BayesCpi", [0.95, 0.05], None, (1, 3, 7)),   # (three groups of look-ahead with k_fwd beside the chain: panel 512; else (1, 2, 7))
    ("BayesB", [0.8, 0.2], None, (1, 3, 7)),
    ("BayesCpi", [0.95, 0.05], None, (1, 2, 8)),   # round 6: eight panels per launch (k_chain_group<1, 8, 8, 3, CERT> + k_fwd<8, 1, 8>)
    ("BayesB", [0.8, 0.2], None, (1, 2, 8)),
    ("BayesR", [0.95, 0.02, 0.02, 0.01], [0, 1e-4, 1e-3, 1e-2], (1, 2, 1)),   # k_chain_persist: the geometry a BayesR run holds while many markers move
    ("BayesR", [0.95, 0.02, 0.02, 0.01], [0, 1e-4, 1e-3, 1e-2], (1, 2, 2)),   # round 6: the certified group chain (k_chain_group<3, 2, 4, 10>), its geometry once few do
    ("BayesR", [0.95, 0.02, 0.02, 0.01], [0, 1e-4, 1e-3, 1e-2], (1, 3, 7)),   # ... and BayesR on the wide group chain with k_fwd (k_chain_group<3, 8, 7, 4>)
    ("BayesRR", [0.95, 0.05], None, (1, 2, 1)),
]


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(20250929)
    n, m = 2048, 32768
    X = geno(rng, n, m)
    return {"X": X, "y": pheno(rng, X), "rng_state": rng.bit_generator.state}


def _compare(r, ref, tol=1e-9):
    a, b = r["MCMCsamples"]["alpha"], ref["s_alpha"]
    assert np.array_equal(a != 0, b != 0), "inclusion pattern differs in %d entries" % int(((a != 0) != (b != 0)).sum())
    np.testing.assert_allclose(a, b, rtol=tol, atol=1e-13)
    np.testing.assert_allclose([r["Vg"], r["Ve"], r["h2"], r["mu"]], [ref["Vg"], ref["Ve"], ref["h2"], ref["mu"]], rtol=tol)
    np.testing.assert_allclose(r["pi"], ref["pi"], rtol=tol, atol=1e-14)
    np.testing.assert_allclose(r["pip"], ref["pip"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["g"], ref["g"], rtol=1e-8, atol=1e-9)     # final-iteration u = X g (src/Bayes.cpp:1023)
    np.testing.assert_allclose(r["e"], ref["e"], rtol=1e-8, atol=1e-9)


@pytest.mark.parametrize("model,Pi,fold,geo", CASES)
@pytest.mark.parametrize("panel,mcols", [(512, 32768), (64, 4096)])
@pytest.mark.parametrize("start", ["cold", "dense"])
@pytest.mark.parametrize("precise", [2, 1])   # 2: exact fixed-point mat-vec (library default); 1: fp64 FMA mat-vec
def test_default_geometry_draw_for_draw_at_pipeline_depth(big, model, Pi, fold, geo, panel, mcols, start, precise):
    if precise == 1 and panel == 64:
        pytest.skip("the fp64-FMA mat-vec is covered at panel 512 (and by the goldens at panel 64): not repeated here, to keep the suite's run time")
    X, y = big["X"][:, :mcols], big["y"]
    if model == "BayesRR":
        if panel == 512:
            panel = 0          # every marker moves: the library's own default panel for RR/A/L (128)
        X = X[:, :min(mcols, 8192)]
    m = X.shape[1]
    g0 = None
    if start == "dense":       # 30 % of the markers in the model before the first sweep: crowded panels from the start
        rng = np.random.default_rng(5 + m)
        g0 = np.where(rng.random(m) < 0.3, rng.normal(0, 0.03, m), 0.0)
    kw = dict(fold=fold, niter=8, nburn=0, thin=1, seed=97531)
    ref = O.bayes(y, X, model, Pi, rng=O.RNG_PHILOX, store_alpha=True, g_init=g0, **kw)
    with H.Context(X.shape[0], m, panel=panel, precise=precise, seed=97531) as c:
        c.upload(X)
        # the geometry hb_bayes_run() itself chooses for this model (hb_run.hip: setup)
        c.set_pipeline(*geo)
        if geo == (1, 3, 7) and c.panel != 512:
            geo = (1, 2, 7)
        if geo == (1, 2, 8) and c.panel != 512:
            geo = (1, 1, 8)    # (eight panels per launch with two groups of look-ahead need k_fwd: panel 512)
        assert c.pipeline()[:3] == geo
        if geo[2] == 7:
            assert (m + c.panel - 1) // c.panel >= 9 * 7 + 1      # >= 10 mat-vec groups
        r = H.Bayes(y, None, model, Pi, verbose=False, precise=precise, g_init=g0, ctx=c, **kw)
        ev = r["timing"]["mean_events"]
    _compare(r, ref)
    if start == "dense" and model != "BayesRR":
        assert ev > 0.03 * m                                       # it really was a dense chain
    # and through the one-call boundary, which picks the geometry by itself (no context): same chain
    if panel in (0, 512) and start == "cold":
        r2 = H.Bayes(y, X, model, Pi, verbose=False, precise=precise, panel=panel, **kw)
        _compare(r2, ref)


@pytest.mark.parametrize("model,Pi,fold,geo", CASES)
@pytest.mark.parametrize("panel,mcols", [(512, 32768), (64, 4096)])
def test_two_bit_resident_layout_is_the_same_chain(big, model, Pi, fold, geo, panel, mcols):
    """genotype_bits = 2 (2 bits per genotype resident, expanded in registers: hb_dotq2.hpp; the format is PLINK's,
    reference src/read_bed.cpp:116-167): the digit-plane dot products are the same exact integers as on int8 columns, so the
    chain is the int8 chain BIT FOR BIT — and the oracle's draw for draw. Through the one-call boundary (the run packs and drops
    its int8 copy after the Gram build) and through a context whose layout was switched by hand, from a cold and a dense start."""
    X, y = big["X"][:, :mcols], big["y"]
    if model == "BayesRR":
        panel = 0 if panel == 512 else panel
        X = X[:, :min(mcols, 8192)]
    m = X.shape[1]
    kw = dict(fold=fold, niter=6, nburn=0, thin=1, seed=1357)
    ref = O.bayes(y, X, model, Pi, rng=O.RNG_PHILOX, store_alpha=True, **kw)
    r8 = H.Bayes(y, X, model, Pi, verbose=False, panel=panel, genotype_bits=8, **kw)
    r2 = H.Bayes(y, X, model, Pi, verbose=False, panel=panel, genotype_bits=2, **kw)
    assert (r8["timing"]["resident_bits"], r2["timing"]["resident_bits"]) == (8, 2)
    _compare(r2, ref)
    for k in ("alpha", "pip", "g", "pi"):
        assert np.array_equal(r2[k], r8[k]), k
    np.testing.assert_allclose(r2["e"], r8["e"], rtol=0, atol=1e-10)   # (X * alpha sums its column blocks with atomics: last bits)
    assert np.array_equal(r2["MCMCsamples"]["alpha"], r8["MCMCsamples"]["alpha"])
    rng = np.random.default_rng(9 + m)
    g0 = np.where(rng.random(m) < 0.3, rng.normal(0, 0.03, m), 0.0)
    refd = O.bayes(y, X, model, Pi, rng=O.RNG_PHILOX, store_alpha=True, g_init=g0, **kw)
    with H.Context(X.shape[0], m, panel=panel, seed=1357) as c:
        c.upload(X)
        c.set_pipeline(*geo)
        c.build_gram()
        c.set_layout(2, keep_int8=False)
        rd = H.Bayes(y, None, model, Pi, verbose=False, g_init=g0, ctx=c, **kw)
        assert c.layout() == (2, False)
    _compare(rd, refd)


def test_auto_layout_picks_two_bits_where_exact_and_faster_and_is_the_same_chain(big):
    """hb_bayes_args.genotype_bits = 0 — what ibrm(), the Rcpp shim and Bayes() pass — is "auto" since round 6 (round-5 verdict: "make the
    fast layout the default where it is exact"): 2 bits per genotype resident for BayesB / BayesC at panel 512 when every code is in
    0..3, int8 columns for the other models and for other codes (the reference also accepts -1/0/1). Whatever it picks
    is the forced-int8 chain bit for bit, and the result says which layout ran."""
    X, y = big["X"][:, :16384], big["y"]
    kw = dict(niter=5, nburn=0, thin=1, seed=4242, verbose=False)
    ra = H.Bayes(y, X, "BayesCpi", [0.95, 0.05], **kw)
    r8 = H.Bayes(y, X, "BayesCpi", [0.95, 0.05], genotype_bits=8, **kw)
    assert (ra["timing"]["resident_bits"], r8["timing"]["resident_bits"]) == (2, 8)
    for k in ("alpha", "pip", "g", "pi"):
        assert np.array_equal(ra[k], r8[k]), k
    assert np.array_equal(ra["MCMCsamples"]["alpha"], r8["MCMCsamples"]["alpha"])
    # codes -1/0/1: not representable at 2 bits -> int8, silently (forcing 2 is refused with a text, as before)
    Xs = (X[:, :8192] - 1).astype(np.int8)
    rs = H.Bayes(y, Xs, "BayesCpi", [0.95, 0.05], **kw)
    assert rs["timing"]["resident_bits"] == 8
    with pytest.raises(H.HibayesError, match="codes 0..3"):
        H.Bayes(y, Xs, "BayesCpi", [0.95, 0.05], genotype_bits=2, **kw)
    # BayesR with up to four classes at panel 512: 2 bits too (k_dotq2m beside both of its chains); the models in which every marker moves
    # (dense update rows read int8 columns) and a small problem (panel < 512): int8
    kr = dict(kw, fold=[0, 1e-4, 1e-3, 1e-2])
    rr2 = H.Bayes(y, X[:, :8192], "BayesR", [0.95, 0.02, 0.02, 0.01], **kr)
    rr8 = H.Bayes(y, X[:, :8192], "BayesR", [0.95, 0.02, 0.02, 0.01], genotype_bits=8, **kr)
    assert (rr2["timing"]["resident_bits"], rr8["timing"]["resident_bits"]) == (2, 8)
    for k in ("alpha", "pip", "g", "pi"):
        assert np.array_equal(rr2[k], rr8[k]), k
    assert H.Bayes(y, X[:, :8192], "BayesRR", [0.95, 0.05], **kw)["timing"]["resident_bits"] == 8
    assert H.Bayes(y, X[:, :2048], "BayesCpi", [0.95, 0.05], **kw)["timing"]["resident_bits"] == 8


@pytest.mark.parametrize("model,Pi,fold,geo", [CASES[0], CASES[2]])
def test_matrix_core_matvec_is_the_same_chain_bit_for_bit(big, model, Pi, fold, geo):
    """hb_ctx_set_matvec_kernel(c, 2): the 2-bit mat-vec with the seven digit planes as a skinny int8 GEMM on the matrix cores
    (k_dotq2m, an A/B beside the default v_dot4 kernel). Integer sums in another order: the same integers, hence the same chain
    bit for bit, and the oracle's draw for draw."""
    X, y = big["X"], big["y"]
    kw = dict(fold=fold, niter=6, nburn=0, thin=1, seed=8642)
    ref = O.bayes(y, X, model, Pi, rng=O.RNG_PHILOX, store_alpha=True, **kw)
    out = []
    for kind in (0, 2):
        with H.Context(X.shape[0], X.shape[1], panel=512, seed=8642) as c:
            c.upload(X)
            c.set_pipeline(*geo)
            c.build_gram()
            c.set_layout(2, keep_int8=False)
            c.set_matvec_kernel(kind)
            out.append(H.Bayes(y, None, model, Pi, verbose=False, ctx=c, **kw))
    _compare(out[1], ref)
    for k in ("alpha", "pip", "g", "pi"):
        assert np.array_equal(out[0][k], out[1][k]), k
    assert np.array_equal(out[0]["MCMCsamples"]["alpha"], out[1]["MCMCsamples"]["alpha"])


@pytest.mark.parametrize("panel,geo", [(64, (1, 2, 7)), (512, (1, 2, 7)), (128, (1, 2, 1)), (256, (1, 1, 8)), (64, (0, 3, 1))])
def test_every_band_gram_block_exact(panel, geo):
    rng = np.random.default_rng(panel + geo[2])
    n, m = 311, panel * 21 + 9
    X = geno(rng, n, m)
    if panel == 128:
        X = (X - 1).astype(np.int8)           # signed codes (-1/0/1)
    X = np.asfortranarray(X)
    with H.Context(n, m, panel=panel) as c:
        c.upload(X)
        c.set_pipeline(*geo)
        c.build_gram()
        pipe, Lv, D, band = c.pipeline()
        assert band == max((Lv + 1) * D - 1, Lv) if pipe else band == Lv
        npan = (m + panel - 1) // panel
        Xp = np.zeros((n, npan * panel))          # float64 BLAS products of small integers are exact (|G| <= 4 n << 2^53)
        Xp[:, :m] = X
        checked = 0
        for p in range(npan):
            cols = Xp[:, p * panel:(p + 1) * panel]
            for l in range(0, band + 1):
                if p - l < 0:
                    continue
                rows = Xp[:, (p - l) * panel:(p - l + 1) * panel]
                G = c.gram_band(p, l)
                assert np.array_equal(G, (rows.T @ cols).astype(np.int64)), "band block p=%d l=%d" % (p, l)   # int32, bit-exact
                checked += 1
        assert checked >= npan * (band + 1) - (band + 1) * (band + 2) // 2


@pytest.mark.parametrize("wide", [(1, 3, 7), (1, 2, 7)])
def test_geometry_by_regime_is_the_same_chain(big, wide):
    """hb_ctx_set_adaptive: hb_run switches between the narrow band (while many markers move) and the wide one on ONE stored
    band and cached per-geometry graphs; the chain is the oracle's draw for draw, and the switch really happened."""
    X, y = big["X"], big["y"]
    m = X.shape[1]
    kw = dict(niter=14, nburn=4, thin=2, seed=777)
    ref = O.bayes(y, X, "BayesCpi", [0.95, 0.05], rng=O.RNG_PHILOX, store_alpha=True, **kw)
    with H.Context(X.shape[0], m, panel=512, seed=97531) as c:
        c.upload(X)
        c.set_pipeline(*wide)
        c.build_gram()
        c.set_adaptive(True)
        r = H.Bayes(y, None, "BayesCpi", [0.95, 0.05], verbose=False, ctx=c, **kw)
        geo_end = c.pipeline()
    _compare(r, ref)
    # a cold start puts ~26 markers per panel into the model (narrow band); by the end ~1 per panel moves (wide band)
    assert r["timing"]["mean_events"] > 2.6 * 64 / 4
    assert geo_end[:3] in (wide, (1, 2, 2))


@pytest.mark.parametrize("model,Pi,fold,blocks", [("BayesCpi", [0.95, 0.05], None, 4), ("BayesR", [0.95, 0.02, 0.02, 0.01], [0, 1e-4, 1e-3, 1e-2], 3),
                                                  ("BayesRR", [0.95, 0.05], None, 5)])
def test_a_sweep_in_blocks_is_the_same_chain(big, model, Pi, fold, blocks):
    """hb_bayes_args.sync_blocks cuts a sweep into runs of whole mat-vec groups (each run a self-contained pipeline: chain,
    mat-vec launches, updates, drain); unsharded nothing is exchanged between them, and the chain must be the oracle's draw
    for draw — which checks the range machinery (first / last run, version slots, absolute group indices) by itself."""
    X, y = big["X"], big["y"]
    if model == "BayesRR":
        X = X[:, :8192]
    kw = dict(niter=8, nburn=2, thin=2, seed=4242)
    if fold is not None:
        kw["fold"] = fold
    ref = O.bayes(y, X, model, Pi, rng=O.RNG_PHILOX, store_alpha=True, **kw)
    r = H.Bayes(y, X, model, Pi, verbose=False, sync_every_blocks=blocks, **kw)
    _compare(r, ref)


@pytest.mark.parametrize("model", ["BayesRR", "BayesA", "BayesL"])
def test_all_move_models_at_panel_256(big, model):
    """BayesRR / A / L at P = 256 (a panel size no other case uses for these models): every marker moves every sweep, most Gram
    rows of a round come from memory, not from the LDS row cache. Draw for draw against the oracle; BayesL to 1e-6: its
    per-marker variance 1 / inverse-Gaussian(|g|) amplifies the last-bit differences in the order of the band corrections
    (measured: 2e-7 relative on 4 % of the stored effects, none on the inclusion pattern)."""
    X, y = big["X"][:, :8192], big["y"]
    kw = dict(niter=6, nburn=2, thin=2, seed=31337)
    ref = O.bayes(y, X, model, [0.95, 0.05], rng=O.RNG_PHILOX, store_alpha=True, **kw)
    r = H.Bayes(y, X, model, [0.95, 0.05], verbose=False, panel=256, **kw)
    _compare(r, ref, tol=1e-6 if model == "BayesL" else 1e-9)


@pytest.mark.parametrize("model", ["BayesRR", "BayesA", "BayesL"])
@pytest.mark.parametrize("geo", [(1, 2, 2), (1, 2, 1), (1, 1, 1), (1, 1, 2)])
def test_dense_chain_of_the_all_move_models_at_panel_512(big, model, geo):
    """BayesRR / A / L at panel 512 run k_chain_dense + k_fold_dense (hb_chain_dense.hpp: static order, the 64 x 64 diagonal
    blocks in registers, the band folded by workgroups spread over the chip and handed back through fcorr[]) and, with the
    fixed-point mat-vec, the one-row-per-lane update with the panel's slab through LDS-DMA. Draw for draw against the oracle
    (src/Bayes.cpp:587-625, :719-741) under every geometry the kernel supports, on a marker count that leaves a ragged last
    panel, with monomorphic markers, from a cold start and from installed effects; BayesL to 1e-6 (see above)."""
    X, y = big["X"][:, :8192 + 100], big["y"]
    m = X.shape[1]
    tol = 1e-6 if model == "BayesL" else 1e-9
    kw = dict(niter=6, nburn=2, thin=2, seed=31337)
    ref = O.bayes(y, X, model, [0.95, 0.05], rng=O.RNG_PHILOX, store_alpha=True, **kw)
    rng = np.random.default_rng(77)
    g0 = rng.normal(0, 0.01, m)
    g0[7::997] = 0.0
    refw = O.bayes(y, X, model, [0.95, 0.05], rng=O.RNG_PHILOX, store_alpha=True, g_init=g0, **kw)
    with H.Context(X.shape[0], m, panel=512, seed=31337) as c:
        c.upload(X)
        c.set_pipeline(*geo)
        assert c.pipeline()[:3] == geo and c.panel == 512
        r = H.Bayes(y, None, model, [0.95, 0.05], verbose=False, ctx=c, **kw)
        _compare(r, ref, tol=tol)
        assert r["timing"]["mean_events"] == m - len(range(7, m, 997))     # every polymorphic marker moves every sweep
        rw = H.Bayes(y, None, model, [0.95, 0.05], verbose=False, ctx=c, g_init=g0, **kw)
        _compare(rw, refw, tol=tol)


@pytest.mark.parametrize("precise", [2, 1])
def test_dense_chain_through_the_one_call_boundary(big, precise):
    """hb_bayes_run's own choice for BayesRR on a problem of this size is panel 512 at (Lv, D) = (2, 2); precise = 1 keeps the
    fp64 mat-vec with its 256-thread update rows beside the dense chain; a sweep cut into blocks is the same chain."""
    X, y = big["X"][:, :8192], big["y"]
    kw = dict(niter=6, nburn=2, thin=2, seed=2468)
    ref = O.bayes(y, X, "BayesRR", [0.95, 0.05], rng=O.RNG_PHILOX, store_alpha=True, **kw)
    r = H.Bayes(y, X, "BayesRR", [0.95, 0.05], verbose=False, precise=precise, **kw)
    _compare(r, ref)
    rb = H.Bayes(y, X, "BayesRR", [0.95, 0.05], verbose=False, precise=precise, sync_every_blocks=3, **kw)
    _compare(rb, ref)


@pytest.mark.parametrize("n,m", [(100, 300), (333, 600)])
@pytest.mark.parametrize("bits", [8, 2])
def test_dense_chain_on_a_single_or_ragged_panel(n, m, bits):
    """Panel 512 forced on problems of less than one panel and of one panel and a ragged second one, few individuals (four
    update blocks), int8 and 2-bit resident genotypes (the 2-bit layout keeps the 256-row update rows beside k_chain_dense)."""
    rng = np.random.default_rng(3 + m)
    X = geno(rng, n, m)
    y = pheno(rng, X, ncausal=20)
    kw = dict(niter=5, nburn=1, thin=2, seed=99)
    for model in ("BayesRR", "BayesL"):
        ref = O.bayes(y, X, model, [0.95, 0.05], rng=O.RNG_PHILOX, store_alpha=True, **kw)
        r = H.Bayes(y, X, model, [0.95, 0.05], verbose=False, panel=512, genotype_bits=bits, **kw)
        _compare(r, ref, tol=1e-6 if model == "BayesL" else 1e-9)


def test_dense_update_rows_are_the_old_update_rows_bit_for_bit(big, monkeypatch):
    """update_rows_dense (one row per lane, the panel's genotype slab through LDS-DMA, changes from dd[]) sums the same products in
    the same marker order as update_rows (four rows per lane, move list): the whole run must agree BIT FOR BIT with the one that
    keeps the old update rows beside k_chain_dense (HB_DENSE_UPD=0)."""
    X, y = big["X"][:, :8192 + 100], big["y"]
    kw = dict(niter=6, nburn=2, thin=2, seed=777)
    r_new = H.Bayes(y, X, "BayesRR", [0.95, 0.05], verbose=False, **kw)
    monkeypatch.setenv("HB_DENSE_UPD", "0")
    r_old = H.Bayes(y, X, "BayesRR", [0.95, 0.05], verbose=False, **kw)
    for k in ("alpha", "g", "Vg", "Ve", "h2", "mu"):     # (g: the final u = X g, accumulated by the update rows themselves)
        assert np.array_equal(np.asarray(r_new[k]), np.asarray(r_old[k])), k
    assert np.array_equal(r_new["MCMCsamples"]["alpha"], r_old["MCMCsamples"]["alpha"])
    np.testing.assert_allclose(r_new["e"], r_old["e"], rtol=0, atol=1e-10)   # (X * alpha sums its column blocks with atomics: last bits)


LONG = [  # model, Pi, fold, geometry, resident bits, adaptive geometry, markers, sweeps, tolerance
    ("BayesCpi", [0.95, 0.05], None, (1, 3, 7), 2, True, 32768, 200, 1e-9),     # (measured on MI355X: 1.4e-15, 1.1e-14, 7e-15 of max |alpha|)
    ("BayesCpi", [0.95, 0.05], None, (1, 2, 8), 2, True, 32768, 200, 1e-9),     # round 6: eight panels per launch, with the adaptive switch to (2, 2) and back
    ("BayesR", [0.95, 0.02, 0.02, 0.01], [0, 1e-4, 1e-3, 1e-2], (1, 2, 1), 8, False, 32768, 200, 1e-9),
    # round 6: BayesR on the certified group chain (k_chain_group<3, 2, 4, 10>) for 200 sweeps (this small problem keeps ~40 moves a panel: its crowded
    # rounds and its certified ones; the sparse regime and the switch are test_bayesr_geometry_by_regime's)
    ("BayesR", [0.95, 0.02, 0.02, 0.01], [0, 1e-4, 1e-3, 1e-2], (1, 2, 2), 8, False, 32768, 200, 1e-9),
    ("BayesRR", [0.95, 0.05], None, (1, 2, 2), 8, False, 8192 + 100, 100, 1e-9),
]


@pytest.mark.parametrize("model,Pi,fold,geo,bits,adaptive,mcols,niter,tol", LONG)
def test_long_chain_draw_for_draw_at_pipeline_depth(big, model, Pi, fold, geo, bits, adaptive, mcols, niter, tol):
    """The reference runs 20 000 iterations by default (R/bayes.r:264-269, the loop at src/Bayes.cpp:477); rounds 1-4 compared at
    most 16 sweeps at pipeline depth. Here 200 (the dense model: 100) at n = 2 048 x m = 32 768, panel 512, against the live oracle
    draw for draw: BayesCpi on 2-bit genotypes with the geometry chosen by regime — the cold start's narrow band, the switch to
    (3, 7), then 150+ sweeps in the stationary regime the bench's `value` is measured in (k_chain_group + k_fwd, the wrap of the
    correction ring hundreds of times over); BayesR under its hot list / row cache / k_warm as the model empties (entry
    prediction, cache churn); BayesRR on k_chain_dense + k_fold_dense. Every stored record (nburn = niter / 2, thin 5), the PIP
    counters of every post-burn iteration, and the final state."""
    X, y = big["X"][:, :mcols], big["y"]
    m = X.shape[1]
    kw = dict(fold=fold, niter=niter, nburn=niter // 2, thin=5, seed=8086)
    ref = O.bayes(y, X, model, Pi, rng=O.RNG_PHILOX, store_alpha=True, **kw)
    with H.Context(X.shape[0], m, panel=512, seed=8086) as c:
        c.upload(X)
        c.set_pipeline(*geo)
        c.build_gram()
        if adaptive:
            c.set_adaptive(True)
        if bits == 2:
            c.set_layout(2, keep_int8=False)
        r = H.Bayes(y, None, model, Pi, verbose=False, ctx=c, **kw)
        geo_end = c.pipeline()[:3]
        assert c.layout()[0] == bits
    assert r["MCMCsamples"]["alpha"].shape[1] == niter // 2 // 5
    _compare(r, ref, tol=tol)
    np.testing.assert_allclose(r["last"]["g"], ref["last"]["g"], rtol=tol, atol=1e-13)
    for k in ("mu", "vare", "varg"):
        assert r["last"]["warm"][k] == pytest.approx(ref["last"]["warm"][k], rel=tol), k
    np.testing.assert_allclose(r["last"]["warm"]["pi"], ref["last"]["warm"]["pi"], rtol=tol)
    err = np.max(np.abs(r["MCMCsamples"]["alpha"] - ref["s_alpha"])) / np.max(np.abs(ref["s_alpha"]))
    print("%s: %d sweeps, %d records, max |alpha - oracle| / max |alpha| = %.2e, %.1f moves per sweep, geometry at the end %s"
          % (model, niter, niter // 2 // 5, err, r["timing"]["mean_events"], geo_end))
    if adaptive:
        assert geo_end == geo          # the run ended in the wide geometry: the stationary regime was reached and run in


def test_bayesr_geometry_by_regime(big):
    """Round 6: a BayesR run (up to four classes, panel 512) picks its geometry per sweep from the moves of the sweep before — (2, 1) and
    k_chain_persist while more than ~27 markers a panel move, (2, 2) and the certified group chain below ~22 (hb_run.hip; measured:
    profiles/r06_bayesr_regime2.txt). From a cold start (5 % of the markers expected in the model: 26 a panel) the run leaves the stored (2, 2)
    before its first sweep; from a sparse state with pi0 = 0.995 it stays there; either way it is the oracle's chain draw for draw."""
    X, y = big["X"][:, :32768], big["y"]
    m = X.shape[1]
    Pi, fold = [0.95, 0.02, 0.02, 0.01], [0, 1e-4, 1e-3, 1e-2]
    kw = dict(fold=fold, niter=10, nburn=0, thin=1, seed=6809)
    rng = np.random.default_rng(77)
    g0 = np.where(rng.random(m) < 0.004, rng.normal(0, 0.02, m), 0.0)
    warm = dict(mu=float(y.mean()), vare=float(0.6 * y.var()), varg=2e-4, pi=[0.995, 0.003, 0.0015, 0.0005])
    for start, expect in (("cold", (1, 2, 1)), ("sparse", (1, 2, 2))):
        k2 = dict(kw, g_init=g0, warm=warm) if start == "sparse" else kw
        ref = O.bayes(y, X, "BayesR", Pi, rng=O.RNG_PHILOX, store_alpha=True, **k2)
        with H.Context(X.shape[0], m, panel=512, seed=6809) as c:
            c.upload(X)
            c.set_pipeline(1, 2, 2)
            c.set_adaptive(True)
            r = H.Bayes(y, None, "BayesR", Pi, verbose=False, ctx=c, **k2)
            geo_end = c.pipeline()[:3]
        print("BayesR from a %s start: %.1f moves per sweep (%.1f per panel), geometry at the end %s" % (start, r["timing"]["mean_events"], r["timing"]["mean_events"] / 64, geo_end))
        assert geo_end == expect, (start, geo_end)
        _compare(r, ref)
        # the one-call boundary (a context of the run's own) takes the same decisions: the same chain
        r1 = H.Bayes(y, X, "BayesR", Pi, verbose=False, **k2)
        _compare(r1, ref)


@pytest.mark.parametrize("model,Pi,fold", [("BayesCpi", [0.95, 0.05], None), ("BayesR", [0.95, 0.02, 0.02, 0.01], [0, 1e-4, 1e-3, 1e-2]),
                                            ("BayesL", [0.95, 0.05], None)])
def test_continued_chain_is_the_oracles_continued_chain(big, model, Pi, fold):
    """hb_bayes_args.warm + g_init (ABI 6): a run continued from the state another run reported. Both sides run 30 sweeps, hand
    their OWN last state (effects, mu, vare, varg, pi, BayesL's lambda2 and per-marker variances) to a second run of 6 sweeps under a
    new seed: the second runs agree draw for draw, i.e. the state crosses the boundary completely on both sides."""
    mc = 8192 + 100
    X, y = big["X"][:, :mc], big["y"]
    tol = 1e-5 if model == "BayesL" else 1e-9   # (BayesL: 1 / inverse-Gaussian(|g|) amplifies last-bit differences, 3e-6 after 30 sweeps)
    k1 = dict(fold=fold, niter=30, nburn=29, thin=1, seed=4004)
    k2 = dict(fold=fold, niter=6, nburn=0, thin=1, seed=6502)
    ref1 = O.bayes(y, X, model, Pi, rng=O.RNG_PHILOX, store_alpha=True, **k1)
    ref2 = O.bayes(y, X, model, Pi, rng=O.RNG_PHILOX, store_alpha=True, g_init=ref1["last"]["g"], warm=ref1["last"]["warm"], **k2)
    r1 = H.Bayes(y, X, model, Pi, verbose=False, **k1)
    _compare(r1, ref1, tol=tol)
    r2 = H.Bayes(y, X, model, Pi, verbose=False, g_init=r1["last"]["g"], warm=r1["last"]["warm"], **k2)
    _compare(r2, ref2, tol=10 * tol)
    # and it IS a continuation: the first sweep of the second run moves about as many markers as the last of the first
    if model == "BayesCpi":
        nnz1 = int((r1["last"]["g"] != 0).sum())
        assert abs(int((r2["MCMCsamples"]["alpha"][:, 0] != 0).sum()) - nnz1) < max(20, nnz1)


@pytest.mark.parametrize("knob,values", [("HB_CERT", ("0", "1"))])
def test_certified_check_and_compact_band_are_the_plain_group_chain(big, monkeypatch, knob, values):
    """A round-5 variant of k_chain_group at (3, 7) must change NOTHING in the results:
    HB_CERT (on by default): the violation check of a round from the rank-one part of the moves, G[k][j] = ga[k] gB[j] + c[k][j], and the bound
    |c[k][j]| <= gcmax[k] — passed-over markers proven to stay cost no Gram rows, proven crossers join the candidates before anything is fetched,
    the undecided ones send the round through the full fold and the exact check. A cold start with the geometry switch, and a dense start (5 % of the markers in the model:
    rounds that do not reach the group's end, roll-backs); and the oracle's draw for draw."""
    X, y = big["X"], big["y"]
    m = X.shape[1]
    rng = np.random.default_rng(12)
    g0 = np.where(rng.random(m) < 0.05, rng.normal(0, 0.03, m), 0.0)
    out = []
    for on in values:
        monkeypatch.setenv(knob, on)
        res = []
        with H.Context(X.shape[0], m, panel=512, seed=99) as c:
            c.upload(X)
            c.set_pipeline(1, 3, 7)
            c.build_gram()
            c.set_adaptive(True)
            c.set_layout(2, keep_int8=False)
            res.append(H.Bayes(y, None, "BayesCpi", [0.95, 0.05], verbose=False, ctx=c, niter=60, nburn=20, thin=4, seed=99))
            c.set_adaptive(False)
            c.set_pipeline(1, 3, 7)
            res.append(H.Bayes(y, None, "BayesCpi", [0.95, 0.05], verbose=False, ctx=c, niter=6, nburn=0, thin=1, seed=98, g_init=g0))
        out.append(res)
    # the cold run (one round per group once the wide geometry is on): every number bit for bit
    a, b = out[0][0], out[1][0]
    for k in ("alpha", "pip", "g", "pi", "Vg", "Ve"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert np.array_equal(a["MCMCsamples"]["alpha"], b["MCMCsamples"]["alpha"])
    # the dense start (groups of several rounds: the certified path repeats a round with FEWER new candidates than a roll-back adds, so a
    # crowded group may be cut into rounds differently and its forward sums grouped differently): the same decisions and moves, effects to
    # the last bits' rounding (measured: 1e-16)
    a, b = out[0][1], out[1][1]
    assert a["timing"]["mean_events"] == b["timing"]["mean_events"]
    assert np.array_equal(a["MCMCsamples"]["alpha"] != 0, b["MCMCsamples"]["alpha"] != 0) and np.array_equal(a["pip"], b["pip"])
    np.testing.assert_allclose(a["MCMCsamples"]["alpha"], b["MCMCsamples"]["alpha"], rtol=1e-12, atol=1e-15)
    ref = O.bayes(y, X, "BayesCpi", [0.95, 0.05], rng=O.RNG_PHILOX, store_alpha=True, niter=6, nburn=0, thin=1, seed=98, g_init=g0)
    _compare(out[1][1], ref)
