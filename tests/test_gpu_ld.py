"""Parity on markers in linkage disequilibrium, on the -1/0/1 coding and on genotype code 3.

Every other GPU test draws independent columns coded 0/1/2 (the demo set apart: 300 x 1000). There the part of a Gram entry that
the certificate of k_chain_group does not model — c[k][j] in G[k][j] = ga[k] gB[j] + c[k][j], bounded by gcmax[k] (hb_chain_group.hpp,
hb_gram.hip: hb_build_gcert / k_gcmax) — is sampling noise, a stationary sweep moves unrelated markers, and column sums are
positive. Real genotypes are none of that: c is about n cov(k, j), a sweep is mostly signal hopping between LD neighbours (a
marker enters because its neighbour just changed: the forward correction ring, k_fwd, k_chain_persist's row cache and entry
prediction see exactly that), the reference also accepts -1/0/1 (ga, gB near zero or negative: the bound rests on gcmax alone),
and the 2-bit layout holds code 3 (both bits of a genotype set; at sub-position 3 of a byte the 0xc0 pattern of hb_dotq2.hpp).

Fixture: geno_ld() — blocks of 40 markers (40 divides neither 64 nor 512: blocks straddle panels and mat-vec groups), one allele
frequency per block, each column a copy of its left neighbour per individual with probability 0.92; every 200 markers an exact
duplicate, an exact complement and a copy one panel of 512 away; monomorphic markers. n = 1000, m = 32 768 = 64 panels of 512
(9 x 7 + 1: ten mat-vec groups at D = 7). The phenotype has 40 causal markers.

Measured on the CPU with the oracle alone (test_the_fixture_reaches_the_ld_regime, which asserts the floors):
  LD hops = markers that enter the model in the traced sweep (the 8th) while a marker with |r| >= 0.5 earlier in the same window
  of D x P consecutive markers changed its effect in that sweep
    data                     model      start                       hops  entrants  moves
    LD                       BayesCpi   cold                         762      1479   2994
    LD                       BayesB     cold                        4754      5253  11900
    LD                       BayesR     cold                         767      1503   3044   (window 2 x 512)
    LD                       BayesCpi   oracle's state, 100 sweeps    29       196    483   (52.8 moves per group of 3584)
    LD, -1/0/1               BayesCpi   cold                         844      1580   3207
    LD, -1/0/1               BayesCpi   oracle's state, 100 sweeps    51       253    622
    independent columns      all three  cold                           0   (1462 / 5228 / 1500 entrants)
  BayesL, sensitivity of the oracle itself (y against y moved by one ulp in every element, 12 sweeps, the first 8292 LD columns):
    max |d alpha| / max |alpha| = 2.5e-9 (-1/0/1 coding: 2.3e-9), the inclusion pattern unchanged; hence BAYESL_TOL below.
"""
import numpy as np
import pytest

import hibayes_amd as H
from oracle import oracle as O

gpu = pytest.mark.gpu

N, M, MD = 1000, 32768, 8192 + 100       # individuals; markers of the point-mass cases; of the dense and the code-3 cases
SEED = 97531
MODELS = {  # Pi, fold
    "BayesCpi": ([0.95, 0.05], None),
    "BayesB": ([0.8, 0.2], None),
    "BayesR": ([0.95, 0.02, 0.02, 0.01], [0, 1e-4, 1e-3, 1e-2]),
    "BayesRR": ([0.95, 0.05], None),
    "BayesA": ([0.95, 0.05], None),
    "BayesL": ([0.95, 0.05], None),
}
# BayesL draws a marker's variance as 1 / inverse-Gaussian(|g|): the chain amplifies last-bit differences (test_gpu_depth.py). The
# oracle against itself with y moved by one ulp, 12 sweeps on the first 8292 LD columns: max |d alpha| / max |alpha| = 2.5e-9
# (-1/0/1 coding: 2.3e-9). The GPU's sums differ from the oracle's in every panel, not in one input: 100 times that,
# and never below the 1e-6 the other BayesL tests use — 100 x 2.5e-9 = 2.5e-7 < 1e-6, so the tolerance is 1e-6.
BAYESL_SWEEPS = 12
BAYESL_SENS = 2.5e-9
BAYESL_TOL = max(1e-6, 100 * BAYESL_SENS)


def geno_ld(rng, n, m, block=40, keep=0.92, top=2):
    """Genotypes in LD blocks (see the module's text). top = 3 adds a third allele draw: codes 0..3."""
    X = np.empty((n, m), dtype=np.int8, order="F")
    for j0 in range(0, m, block):
        nb = min(block, m - j0)
        p = rng.uniform(0.1, 0.5)
        fresh = (rng.random((nb, n)) < p).astype(np.int8) + (rng.random((nb, n)) < p).astype(np.int8)
        if top == 3:
            fresh += (rng.random((nb, n)) < 0.3 * p).astype(np.int8)
        copy = rng.random((nb, n)) < keep
        X[:, j0] = fresh[0]
        for k in range(1, nb):
            X[:, j0 + k] = np.where(copy[k], X[:, j0 + k - 1], fresh[k])
    for j in range(block // 2, m, 5 * block):
        if j + 1 < m:
            X[:, j + 1] = X[:, j]              # exact duplicate
        if j + 3 < m:
            X[:, j + 3] = top - X[:, j]        # exact complement
        if j + 512 < m:
            X[:, j + 512] = X[:, j]            # a copy one panel of 512 away
    X[:, 7::997] = 1                           # monomorphic markers: skipped by the sweep (src/Bayes.cpp:589)
    return X


def geno_independent(rng, n, m):
    p = rng.uniform(0.05, 0.5, m)
    X = np.empty((n, m), dtype=np.int8, order="F")
    for j0 in range(0, m, 4096):
        pj = p[j0:j0 + 4096]
        X[:, j0:j0 + 4096] = (rng.random((n, pj.size)) < pj).astype(np.int8) + (rng.random((n, pj.size)) < pj).astype(np.int8)
    X[:, 7::997] = 1
    return X


def pheno(rng, X, ncausal=40):
    n, m = X.shape
    idx = rng.choice(m, ncausal, replace=False)
    xb = X[:, idx].astype(np.float64) @ rng.normal(0, 1, ncausal)
    xb *= np.sqrt(0.5 / xb.var())
    return xb + rng.normal(0, np.sqrt(0.5), n)


@pytest.fixture(scope="module")
def ld():
    """X: LD, codes 0/1/2. Xs: the same matrix coded -1/0/1. X3: LD with code 3 (8292 markers). Xi: independent columns, Xis: the same
    minus 1. One phenotype per matrix (the signed ones share their unsigned matrix's). refs: the oracle runs, computed once each."""
    rng = np.random.default_rng(20261021)
    X = geno_ld(rng, N, M)
    y = pheno(rng, X)
    X3 = geno_ld(rng, N, MD, top=3)
    y3 = pheno(rng, X3)
    Xi = geno_independent(rng, N, M)
    yi = pheno(rng, Xi)
    Xs, Xis = np.asfortranarray(X - 1, dtype=np.int8), np.asfortranarray(Xi - 1, dtype=np.int8)
    return {"X": {"ld": X, "sld": Xs, "ld3": X3, "ind": Xi, "sind": Xis}, "y": {"ld": y, "sld": y, "ld3": y3, "ind": yi, "sind": yi}, "refs": {}}


def oracle_run(D, name, mcols, model, start="cold", niter=8, pre=100, y=None, tag=None, thin=1):
    """The oracle's chain on the first mcols columns of D["X"][name]: niter sweeps, every record, the last sweep traced. start = "cont":
    continued from the oracle's own state after `pre` sweeps (another seed). Returns (oracle result, keywords of the same run on the GPU)."""
    key = (name, mcols, model, start, niter, pre, tag, thin)
    if key not in D["refs"]:
        Pi, fold = MODELS[model]
        kw = dict(fold=fold, niter=niter, nburn=0, thin=thin, seed=SEED)
        yy = D["y"][name] if y is None else y
        X = D["X"][name][:, :mcols]
        if start == "cont":
            kp = ("state", name, mcols, model, pre)
            if kp not in D["refs"]:
                first = O.bayes(yy, X, model, Pi, fold=fold, rng=O.RNG_PHILOX, niter=pre, nburn=pre - 1, thin=1, seed=SEED + 1)
                D["refs"][kp] = first["last"]
            kw.update(g_init=D["refs"][kp]["g"], warm=D["refs"][kp]["warm"])
        ref = O.bayes(yy, X, model, Pi, rng=O.RNG_PHILOX, store_alpha=True, trace_iter=niter - 1, **kw)
        D["refs"][key] = (ref, kw)
    return D["refs"][key]


def ld_hops(X, old, new, W, rmin=0.5):
    """(LD hops, entrants, moves) of one sweep old -> new: an LD hop is a marker that enters the model (old effect 0, new != 0) while a
    marker with |r| >= rmin earlier in the same window of W consecutive markers changed its effect in that sweep."""
    changed, enter = old != new, (old == 0) & (new != 0)
    hops = 0
    for w0 in range(0, X.shape[1], W):
        ch = np.flatnonzero(changed[w0:w0 + W]) + w0
        en = np.flatnonzero(enter[w0:w0 + W]) + w0
        if not en.size:
            continue
        Z = X[:, ch].astype(np.float64)
        Z -= Z.mean(0)
        Z /= np.maximum(np.sqrt((Z * Z).sum(0)), 1e-300)
        R = np.abs(Z[:, np.searchsorted(ch, en)].T @ Z)
        hops += int(((R >= rmin) & (ch[None, :] < en[:, None])).any(1).sum())
    return hops, int(enter.sum()), int(changed.sum())


def traced_sweep(ref, kw):
    """(effects before, effects after) the last sweep of an oracle_run()."""
    s = ref["s_alpha"]
    old = s[:, -2] if s.shape[1] > 1 else (kw.get("g_init") if kw.get("g_init") is not None else np.zeros(s.shape[0]))
    assert np.array_equal(ref["trace_g"], s[:, -1])       # the traced sweep is the last record
    return old, ref["trace_g"]


def _compare(r, ref, tol=1e-9):
    a, b = r["MCMCsamples"]["alpha"], ref["s_alpha"]
    assert np.array_equal(a != 0, b != 0), "inclusion pattern differs in %d entries" % int(((a != 0) != (b != 0)).sum())
    np.testing.assert_allclose(a, b, rtol=tol, atol=1e-13)
    np.testing.assert_allclose([r["Vg"], r["Ve"], r["h2"], r["mu"]], [ref["Vg"], ref["Ve"], ref["h2"], ref["mu"]], rtol=tol)
    np.testing.assert_allclose(r["pi"], ref["pi"], rtol=tol, atol=1e-14)
    np.testing.assert_allclose(r["pip"], ref["pip"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["g"], ref["g"], rtol=1e-8, atol=1e-9)     # final-iteration u = X g (src/Bayes.cpp:1023)
    np.testing.assert_allclose(r["e"], ref["e"], rtol=1e-8, atol=1e-9)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _report(what, err, r):
    print("LD parity: %s: max |alpha - oracle| / max |alpha| = %.2e, %.1f moves per sweep" % (what, err, r["timing"]["mean_events"]))


def gpu_run(D, name, mcols, model, kw, geo, panel=512, bits=8, precise=2, adaptive=False):
    """The same run through a context with the geometry, layout and arithmetic set by hand. Returns (result, geometry before, geometry
    after, panel)."""
    X, y = D["X"][name][:, :mcols], D["y"][name]
    Pi, _ = MODELS[model]
    with H.Context(X.shape[0], X.shape[1], panel=panel, precise=precise, seed=SEED) as c:
        c.upload(X)
        c.set_pipeline(*geo)
        c.build_gram()
        if adaptive:
            c.set_adaptive(True)
        if bits == 2:
            c.set_layout(2, keep_int8=False)
        geo0 = c.pipeline()[:3]
        r = H.Bayes(y, None, model, Pi, verbose=False, precise=precise, ctx=c, **kw)
        assert c.layout()[0] == bits
        return r, geo0, c.pipeline()[:3], c.panel


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the inputs reach the regime (CPU, oracle only)
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_fixture_reaches_the_ld_regime(ld):
    """A condition on the INPUTS of the GPU tests below, from the oracle alone: the traced sweep (the 8th) holds LD hops — at least 100 from
    a cold start and at least 6 in the state continued from the oracle's 100th sweep (a quarter of what the oracle showed when the fixture
    was designed: 548 and 24; this fixture: 762 and 29, see the module's table) — none at all on independent columns of the same shape, and the
    continued state moves fewer than 64 markers per group of 3584 on average: under the candidate count at which k_chain_group certifies
    a round, i.e. the sparse certified regime the bench's number comes from. Also the one-ulp sensitivity of BayesL that BAYESL_TOL is derived from."""
    cases = [("ld", "BayesCpi", "cold", 3584, 100), ("ld", "BayesB", "cold", 3584, 100), ("ld", "BayesR", "cold", 1024, 100),
             ("ld", "BayesCpi", "cont", 3584, 6), ("sld", "BayesCpi", "cold", 3584, 100), ("sld", "BayesCpi", "cont", 3584, 6),
             ("ind", "BayesCpi", "cold", 3584, None), ("ind", "BayesB", "cold", 3584, None), ("ind", "BayesR", "cold", 1024, None)]
    for name, model, start, W, floor in cases:
        ref, kw = oracle_run(ld, name, M, model, start)
        old, new = traced_sweep(ref, kw)
        hops, entrants, moves = ld_hops(ld["X"][name], old, new, W)
        print("%-4s %-8s %-4s: %5d LD hops, %5d entrants, %5d moves (%.1f per group of %d)" % (name, model, start, hops, entrants, moves, moves * W / M, W))
        if floor is None:
            assert hops == 0, (name, model)
        else:
            assert hops >= floor, (name, model, start, hops)
        if (name, start) == ("ld", "cont"):
            assert moves * 3584 / M < 64
    for name in ("ld", "sld"):
        y = ld["y"][name]
        a = oracle_run(ld, name, MD, "BayesL", niter=BAYESL_SWEEPS)[0]["s_alpha"]
        b = oracle_run(ld, name, MD, "BayesL", niter=BAYESL_SWEEPS, y=np.nextafter(y, np.inf), tag="ulp")[0]["s_alpha"]
        sens = np.max(np.abs(a - b)) / np.max(np.abs(a))
        print("BayesL on %s, %d sweeps: one-ulp sensitivity of the oracle %.2e" % (name, BAYESL_SWEEPS, sens))
        assert np.array_equal(a != 0, b != 0)
        assert 0 < sens <= BAYESL_TOL / 100       # the stated tolerance covers 100 times what the oracle does to itself
    assert BAYESL_TOL <= 1e-5


# ------------------------------------------------------------------------------------------------------------------------------
# 2. point-mass chains under LD
# ------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("model", ["BayesCpi", "BayesB"])
@pytest.mark.parametrize("geo,panel,mcols", [((1, 3, 7), 512, M), ((1, 2, 8), 512, M), ((1, 2, 7), 64, 4096)])
@pytest.mark.parametrize("bits", [2, 8])
def test_point_mass_chain_under_ld_draw_for_draw(ld, model, geo, panel, mcols, bits):
    """k_chain_group + k_fwd from a cold start on LD data: real crossers, undecided markers, repeated rounds and the fall-back to the full
    fold in every group, on 2-bit and int8 resident genotypes; the oracle's chain draw for draw at 1e-9."""
    ref, kw = oracle_run(ld, "ld", mcols, model)
    r, geo0, _, p = gpu_run(ld, "ld", mcols, model, kw, geo, panel=panel, bits=bits)
    assert (geo0, p) == (geo, panel)
    _report("%s %s panel %d, %d bits" % (model, geo, panel, bits), _compare(r, ref), r)


@gpu
def test_continued_sparse_chain_under_ld_draw_for_draw(ld):
    """The regime the bench's number is measured in, on LD data: both sides start from the oracle's state after 100 sweeps; geometry by
    regime on 2-bit genotypes. The run's moves per sweep are the oracle's (within 20 %): it was the sparse, certified regime."""
    ref, kw = oracle_run(ld, "ld", M, "BayesCpi", "cont")
    r, geo0, geo1, _ = gpu_run(ld, "ld", M, "BayesCpi", kw, (1, 3, 7), bits=2, adaptive=True)
    assert geo0 == (1, 3, 7)
    s = np.column_stack([kw["g_init"], ref["s_alpha"]])
    moves = (s[:, 1:] != s[:, :-1]).sum(0).mean()
    _report("BayesCpi continued, geometry at the end %s, oracle's moves per sweep %.1f" % (geo1, moves), _compare(r, ref), r)
    assert abs(r["timing"]["mean_events"] - moves) <= 0.2 * moves


@gpu
@pytest.mark.parametrize("geo,start", [((1, 2, 1), "cold"), ((1, 2, 2), "cold"), ((1, 3, 7), "cold"), ((1, 2, 2), "sparse")])
def test_bayesr_chains_under_ld_draw_for_draw(ld, geo, start):
    """BayesR on k_chain_persist (2, 1) — its Gram-row cache and entry prediction meet entrants that ARE predicted by their neighbours —, on
    the certified group chain (2, 2) and on the wide one (3, 7); (2, 2) also from a sparse installed state with pi0 = 0.995."""
    X, y = ld["X"]["ld"], ld["y"]["ld"]
    Pi, fold = MODELS["BayesR"]
    if start == "cold":
        ref, kw = oracle_run(ld, "ld", M, "BayesR")
    else:
        if "bayesr_sparse" not in ld["refs"]:
            rng = np.random.default_rng(77)
            g0 = np.where(rng.random(M) < 0.004, rng.normal(0, 0.02, M), 0.0)
            g0[7::997] = 0.0
            warm = dict(mu=float(y.mean()), vare=float(0.6 * y.var()), varg=2e-4, pi=[0.995, 0.003, 0.0015, 0.0005])
            kw = dict(fold=fold, niter=8, nburn=0, thin=1, seed=SEED, g_init=g0, warm=warm)
            ld["refs"]["bayesr_sparse"] = (O.bayes(y, X, "BayesR", Pi, rng=O.RNG_PHILOX, store_alpha=True, **kw), kw)
        ref, kw = ld["refs"]["bayesr_sparse"]
    r, geo0, geo1, _ = gpu_run(ld, "ld", M, "BayesR", kw, geo)
    assert geo0 == geo and geo1 == geo
    _report("BayesR %s %s" % (geo, start), _compare(r, ref), r)


@gpu
def test_certified_check_is_the_plain_group_chain_under_ld(ld, monkeypatch):
    """HB_CERT=0 against 1 where the certificate has work to do: under LD the part of G[k][j] the rank-one model leaves out is n cov(k, j),
    hundreds, not sampling noise. Cold (crowded groups of several rounds, which the two variants may cut differently: effects to the last
    bits) and continued (about 64 moves per group of 3584, the candidate count up to which a round is certified: certified rounds and
    full folds side by side), both on the wide geometry itself: the same decisions and move counts, and the oracle's chain."""
    for start in ("cold", "cont"):
        ref, kw = oracle_run(ld, "ld", M, "BayesCpi", start)
        out = []
        for on in ("0", "1"):
            monkeypatch.setenv("HB_CERT", on)
            r, geo0, geo1, _ = gpu_run(ld, "ld", M, "BayesCpi", kw, (1, 3, 7), bits=2)
            assert geo0 == (1, 3, 7) and geo1 == (1, 3, 7)      # (not adaptive: the wide group chain itself runs both states)
            out.append(r)
        a, b = out
        assert a["timing"]["mean_events"] == b["timing"]["mean_events"]
        assert np.array_equal(a["MCMCsamples"]["alpha"] != 0, b["MCMCsamples"]["alpha"] != 0) and np.array_equal(a["pip"], b["pip"])
        np.testing.assert_allclose(a["MCMCsamples"]["alpha"], b["MCMCsamples"]["alpha"], rtol=1e-12, atol=1e-15)
        for r in out:
            _compare(r, ref)


@gpu
@pytest.mark.parametrize("model", ["BayesCpi", "BayesB", "BayesR"])
def test_one_call_boundary_under_ld(ld, model):
    """hb_bayes_run with a context of its own (geometry, geometry by regime and layout are its choices): the same chain, on 2 bits."""
    ref, kw = oracle_run(ld, "ld", M, model)
    r = H.Bayes(ld["y"]["ld"], ld["X"]["ld"], model, MODELS[model][0], verbose=False, **kw)
    assert r["timing"]["resident_bits"] == 2
    _report("%s one call" % model, _compare(r, ref), r)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the -1/0/1 coding through the chains
# ------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["sld", "sind"])
@pytest.mark.parametrize("model,geo,mcols", [("BayesCpi", (1, 3, 7), M), ("BayesR", (1, 2, 2), M), ("BayesRR", (1, 2, 2), MD)])
@pytest.mark.parametrize("start", ["cold", "cont"])
@pytest.mark.parametrize("precise", [2, 1])
def test_signed_coding_through_the_chains(ld, name, model, geo, mcols, start, precise):
    """Codes -1/0/1 (the reference accepts them; k_dot<*, true> and the signed branches of the host's bounds): column sums near zero or
    negative, so ga, gB of the certificate vanish or change sign and the bound rests on gcmax. On LD data and on independent columns,
    with the exact fixed-point mat-vec and the fp64 one, cold and continued from the oracle's state (100 sweeps; BayesRR: 30)."""
    ref, kw = oracle_run(ld, name, mcols, model, start, pre=30 if model == "BayesRR" else 100)
    r, geo0, _, p = gpu_run(ld, name, mcols, model, kw, geo, precise=precise)
    assert p == 512 and geo0 == geo        # (3, 7) holds at panel 512; smaller panels fall to (2, 7): plan_band_limit
    _report("%s on %s, %s, precise %d" % (model, name, start, precise), _compare(r, ref), r)


@gpu
def test_signed_coding_keeps_int8_columns_in_the_auto_layout(ld):
    ref, kw = oracle_run(ld, "sld", M, "BayesCpi")
    r = H.Bayes(ld["y"]["sld"], ld["X"]["sld"], "BayesCpi", MODELS["BayesCpi"][0], verbose=False, **kw)
    assert r["timing"]["resident_bits"] == 8
    _compare(r, ref)


@gpu
@pytest.mark.parametrize("panel,geo,mcols", [(512, (1, 2, 2), MD), (64, (1, 2, 7), 4096)])
def test_band_gram_blocks_exact_on_signed_ld_data(ld, panel, geo, mcols):
    """Every diagonal and band Gram block against int64 numpy on the -1/0/1 LD data: large entries of both signs, and — from the exact
    duplicates, complements and the copies 512 markers away — off-diagonal entries of exactly +xpx and -xpx."""
    X = ld["X"]["sld"][:, :mcols]
    n, m = X.shape
    npan = (m + panel - 1) // panel
    Xp = np.zeros((n, npan * panel))              # float64 products of small integers are exact (|G| <= n << 2^53)
    Xp[:, :m] = X
    xpx = (Xp * Xp).sum(0)
    plus = minus = 0
    with H.Context(n, m, panel=panel) as c:
        c.upload(X)
        c.set_pipeline(*geo)
        c.build_gram()
        assert c.pipeline()[:3] == geo
        band = c.pipeline()[3]
        for p in range(npan):
            cols = Xp[:, p * panel:(p + 1) * panel]
            for l in range(0, min(band, p) + 1):
                rows = Xp[:, (p - l) * panel:(p - l + 1) * panel]
                want = (rows.T @ cols).astype(np.int64)
                assert np.array_equal(c.gram_band(p, l), want), "band block p=%d l=%d" % (p, l)
                if l == 0:
                    assert np.array_equal(c.gram(p), want), "diagonal block p=%d" % p
                    want = want - np.diag(np.diag(want))
                d = xpx[p * panel:(p + 1) * panel][None, :]
                plus += int(((want == d) & (d > 0)).sum())
                minus += int(((want == -d) & (d > 0)).sum())
    assert plus >= m // 200 and minus >= m // 200 - 1


# ------------------------------------------------------------------------------------------------------------------------------
# 4. dense chains under LD
# ------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("model", ["BayesRR", "BayesA", "BayesL"])
@pytest.mark.parametrize("geo", [(1, 2, 2), (1, 2, 1)])
def test_dense_chains_under_ld_draw_for_draw(ld, model, geo):
    """k_chain_dense + k_fold_dense where the band corrections are large: every marker moves and its LD neighbours' moves reach it through
    the band, 12 sweeps. BayesRR / BayesA at 1e-9; BayesL at BAYESL_TOL = max(1e-6, 100 x the oracle's own one-ulp sensitivity 2.5e-9) = 1e-6."""
    ref, kw = oracle_run(ld, "ld", MD, model, niter=BAYESL_SWEEPS)
    r, geo0, _, p = gpu_run(ld, "ld", MD, model, kw, geo)
    assert (geo0, p) == (geo, 512)
    assert r["timing"]["mean_events"] == MD - len(range(7, MD, 997))     # every polymorphic marker moves every sweep
    _report("%s %s" % (model, geo), _compare(r, ref, tol=BAYESL_TOL if model == "BayesL" else 1e-9), r)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. code 3 on LD data
# ------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_code_three_under_ld_auto_layout(ld):
    """Genotype code 3 (both bits set) in the 2-bit layout the run picks by itself: the forced-int8 chain bit for bit, the oracle's at 1e-9."""
    X, y = ld["X"]["ld3"], ld["y"]["ld3"]
    assert X.max() == 3 and 0.005 < (X == 3).mean() < 0.05
    ref, kw = oracle_run(ld, "ld3", MD, "BayesCpi")
    ra = H.Bayes(y, X, "BayesCpi", MODELS["BayesCpi"][0], verbose=False, panel=512, **kw)
    r8 = H.Bayes(y, X, "BayesCpi", MODELS["BayesCpi"][0], verbose=False, panel=512, genotype_bits=8, **kw)
    assert (ra["timing"]["resident_bits"], r8["timing"]["resident_bits"]) == (2, 8)
    for k in ("alpha", "pip", "g", "pi"):
        assert np.array_equal(ra[k], r8[k]), k
    assert np.array_equal(ra["MCMCsamples"]["alpha"], r8["MCMCsamples"]["alpha"])
    _report("BayesCpi code 3, auto layout", _compare(ra, ref), ra)
