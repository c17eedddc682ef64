"""The single-step model's epsilon block on the device (hibayes_amd/csrc/hb_epsl.hip): one step against the restatement's expression in long
double — every row from the device's own new values below it and old values above it —, bit-for-bit determinism under every forced schedule,
and whole chains through ssbrm() / Bayes() against the restatement (tests/epsl_restatement.py) within 1000 times its own order-to-order
spread."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import hibayes_amd as H
from hibayes_amd import _lib

import epsl_restatement as E
from test_epsl_host import DEMO, hub, read_ped, tridiagonal

pytestmark = pytest.mark.gpu
EPS = E.EPS
LD = np.longdouble
KW = dict(niter=60, nburn=20, thin=5, seed=20261020)
SEED, IT = 987654321, 11


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def gamma(k):
    return k * EPS / (1 - k * EPS)


@pytest.fixture(scope="module")
def demo_ss():
    pl = H.read_plink(DEMO)
    phe = H.read_table(DEMO + ".phe")
    M_id = [r[1] for r in pl["fam"]]
    ped = read_ped()
    pr = H.ssbrm_prepare("T1 ~ 1", phe, pl["geno"], M_id, ped)
    G = pr["Ai_nn"]
    return {"pr": pr, "phe": phe, "M_id": M_id, "geno": pl["geno"], "ped": ped, "G": (G.indptr, G.indices, G.data)}


# ---------------------------------------------------------------------------------------------------------------------------------
# one step
# ---------------------------------------------------------------------------------------------------------------------------------
def pattern(q, demo_ss):
    if q == 900:
        return sp.csc_matrix(demo_ss["pr"]["Ai_nn"])
    if q == 257:
        return tridiagonal(257)
    if q == "hub_first":
        return hub(5000, True)
    if q == "hub_last":
        return hub(5000, False)
    if q == 1:
        return sp.csc_matrix(np.array([[2.0]]))
    rng = np.random.default_rng(q)  # a random sparse symmetric pattern, diagonally dominant
    A = sp.random(q, q, density=min(1.0, 3.0 / q), random_state=rng, format="csr")
    A = A + A.T
    A = A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() + 1.0)
    G = sp.csc_matrix(A)
    G.sort_indices()
    return G


def step_case(G, seed=5):
    rng = np.random.default_rng(seed + G.shape[0])
    q = G.shape[0]
    reps = rng.integers(0, 3, q)                         # zz of 0, 1 and 2
    reps[rng.integers(0, q)] = 2
    index0 = rng.permutation(np.repeat(np.arange(q), reps))
    n = index0.size + 37
    return dict(index0=index0, yJ=rng.normal(size=n), yadj=rng.normal(size=n), u=rng.normal(size=n), vare=1.3, veps=0.7, zJ=0.4, chis=float(q) + 3.5,
                s2_df=0.5, n=n)


def run_steps(c, G, cs, modes=(0, 0), steps=2):
    c.epsl_setup(cs["yJ"], G, cs["index0"] + 1)
    c.epsl_force(*modes)
    c.set_residual(cs["yadj"], cs["u"])
    out = []
    for s in range(steps):
        c.epsl_step(cs["vare"], cs["veps"] if s == 0 else -1.0, SEED, IT + s, cs["zJ"] + 0.1 * s, cs["chis"], cs["s2_df"])
        x, veps, qv, J = c.epsl_state()
        r, u = c.get_residual()
        out.append(dict(x=x, veps=veps, q=qv, J=J, r=r, u=u, dbg=c.epsl_debug(), mir=c.mirrors()))
    return out


def check_step(G, cs, pre, post, it, zJ, veps_used, J_old):
    """post against the expression of DESIGN.md section 18, evaluated in long double from the device's own operands"""
    n, q, idx = cs["n"], G.shape[0], cs["index0"]
    ne = idx.size
    vare = cs["vare"]
    d = post["dbg"]
    yJ = cs["yJ"]
    # J: the dot within the dot-product bound, the draw from the device's own dot within a few roundings
    terms = yJ.astype(LD) * pre["r"].astype(LD)
    assert abs(d["rhs"] - float(terms.sum())) <= gamma(n) * float(np.abs(terms).sum())
    JtJ = float(E.seq_sum(yJ * yJ, np.float64))
    parts = (d["rhs"] / JtJ, J_old, np.sqrt(vare / JtJ) * zJ)
    assert abs(post["J"] - ((d["rhs"] + JtJ * J_old) / JtJ + parts[2])) <= 8 * EPS * sum(abs(p) for p in parts)
    # the residual: yadj += (J_old - J) y_J, then the tail += x_old - x; u the negative; both bit for bit, and yadj + u conserved
    dJ = (J_old - post["J"]) * yJ
    r1 = pre["r"] + dJ
    u1 = pre["u"] - dJ
    dx = d["x_old"] - post["x"]
    r2, u2 = r1.copy(), u1.copy()
    r2[n - ne:] = r1[n - ne:] + dx[idx]
    u2[n - ne:] = u1[n - ne:] - dx[idx]
    np.testing.assert_array_equal(post["r"], r2)
    np.testing.assert_array_equal(post["u"], u2)
    assert np.all(np.abs((post["r"] + post["u"]) - (pre["r"] + pre["u"])) <= 4 * EPS * (np.abs(post["r"]) + np.abs(post["u"]) + np.abs(dJ) + 1e-300))
    np.testing.assert_array_equal(post["mir"]["r32"][:n], post["r"].astype(np.float32))
    np.testing.assert_array_equal(post["mir"]["r"][:n], post["r"])
    np.testing.assert_array_equal(d["x_old"], pre["x"])
    # b from the residual after the J step
    rec = E.records_of(idx, q)
    zz = np.array([len(r) for r in rec], dtype=np.float64)
    tail = r1[n - ne:]
    bsum = np.array([float(tail[r].astype(LD).sum()) for r in rec])
    babs = np.array([float(np.abs(tail[r]).sum()) for r in rec])
    assert np.all(np.abs(d["b"] - (bsum + zz * d["x_old"])) <= gamma(4) * (babs + np.abs(zz * d["x_old"])) + 1e-300)
    # every row: new values below it, old values above it (and its own old value)
    z = E.epsl_normals(SEED, it, q)
    lam = vare / veps_used
    ip, ix = G.indptr, G.indices
    dat, xn, xo = G.data.astype(LD), post["x"].astype(LD), d["x_old"].astype(LD)
    worst = 0.0
    for i in range(q):
        ks = slice(ip[i], ip[i + 1])
        js = ix[ks]
        t = dat[ks] * np.where(js < i, xn[js], xo[js])
        s, sabs, k = t.sum(), float(np.abs(t).sum()), js.size
        gii = float(dat[ks][js == i][0])
        aii = LD(zz[i]) + LD(lam) * gii
        Ax = LD(zz[i]) * xo[i] + LD(lam) * s
        sd = np.sqrt(LD(vare) / aii)
        ref = ((LD(d["b"][i]) - Ax) / aii + xo[i]) + sd * LD(z[i])
        # the dot-product bound gamma_k sum |terms| on the row's sums, and 8 roundings of the scalar operations' operands: the quotient, the two
        # additions, and the draw — sqrt, the product, and the device's log / cos / sqrt inside z against the host's (each a few ulps at most)
        tol = (gamma(k + 3) * (lam * sabs + abs(zz[i] * d["x_old"][i]) + abs(d["b"][i]))) / float(aii) \
            + 8 * EPS * (abs(float((LD(d["b"][i]) - Ax) / aii)) + abs(d["x_old"][i]) + abs(float(sd * z[i])))
        err = abs(float(LD(post["x"][i]) - ref))
        worst = max(worst, err / tol)
        assert err <= tol, (i, err, tol)
    # q = x'Gx and veps
    tq = np.array([float((dat[ip[i]:ip[i + 1]] * xn[ix[ip[i]:ip[i + 1]]]).sum()) for i in range(q)])
    tqa = np.array([float(np.abs(dat[ip[i]:ip[i + 1]] * xn[ix[ip[i]:ip[i + 1]]]).sum()) for i in range(q)])
    kmax = int(np.diff(ip).max())
    assert abs(post["q"] - float((xn * tq.astype(LD)).sum())) <= gamma(kmax + (q + 255) // 256 + 12) * float((np.abs(post["x"]) * tqa).sum())
    assert post["veps"] == (post["q"] + cs["s2_df"]) / cs["chis"]
    return worst


@pytest.mark.parametrize("q", [1, 2, 63, 65, 257, 900, "hub_first", "hub_last"])
def test_one_step_against_the_long_double_restatement(q, demo_ss):
    G = pattern(q, demo_ss)
    cs = step_case(G)
    with H.Context(cs["n"], 4) as c:
        c.upload(np.zeros((cs["n"], 4), dtype=np.int8))
        a, b = run_steps(c, G, cs)
        cnt = a["dbg"]
    pre = dict(r=cs["yadj"], u=cs["u"], x=np.zeros(G.shape[0]))
    w1 = check_step(G, cs, pre, a, IT, cs["zJ"], cs["veps"], 0.0)
    w2 = check_step(G, cs, a, b, IT + 1, cs["zJ"] + 0.1, a["veps"], a["J"])   # goes on from x != 0, J != 0 and the device's veps
    print("q = %s: levels %d, launches %d, longest column %d; worst row error / tolerance %.3g, %.3g" % (q, cnt["levels"], cnt["launches"], cnt["max_col"], w1, w2))
    assert not np.array_equal(a["x"], b["x"]) and np.all(np.isfinite(b["x"]))
    # the whole block against the restatement in long double, loosely (the staged checks above are the sharp ones)
    ref = E.epsl_block(G.indptr, G.indices, G.data, cs["index0"], cs["yJ"], cs["yadj"], cs["u"], np.zeros(G.shape[0]), 0.0, cs["vare"], cs["veps"],
                       E.epsl_normals(SEED, IT, G.shape[0]), cs["zJ"], cs["chis"], cs["s2_df"], dtype=LD)
    scale = float(np.max(np.abs(ref["x"])))
    assert np.max(np.abs(a["x"] - ref["x"].astype(np.float64))) < 1e-10 * scale * max(1, cnt["levels"])
    assert abs(a["veps"] - float(ref["veps"])) < 1e-10 * float(ref["veps"]) * max(1, cnt["levels"])


@pytest.mark.parametrize("q", [65, 257, 900, "hub_first", "hub_last"])
def test_every_schedule_gives_one_result_bit_for_bit(q, demo_ss):
    G = pattern(q, demo_ss)
    cs = step_case(G)
    runs = []
    with H.Context(cs["n"], 4) as c:
        c.upload(np.zeros((cs["n"], 4), dtype=np.int8))
        for modes in ((0, 0), (0, 0), (1, 0), (2, 0), (0, 1), (0, 2), (1, 2), (2, 1), (1, 1), (2, 2)):
            runs.append(run_steps(c, G, cs, modes)[-1])
    for r in runs[1:]:
        for key in ("x", "r", "u"):
            np.testing.assert_array_equal(r[key], runs[0][key])
        assert (r["veps"], r["q"], r["J"]) == (runs[0]["veps"], runs[0]["q"], runs[0]["J"])


# ---------------------------------------------------------------------------------------------------------------------------------
# whole chains on the demo
# ---------------------------------------------------------------------------------------------------------------------------------
def compare_chain(got, a, b, extra=()):
    """got (the device) against restatement a, every quantity within 1000 times the restatement's own order-to-order spread |a - b|
    (relative to the quantity's largest magnitude), floored at one rounding times 1000 — as tests/test_gpu_bslmm.py builds it."""
    mc = got["MCMCsamples"]
    pairs = [("s_alpha", mc["alpha"]), ("alpha", got["alpha"]), ("Vg", got["Vg"]), ("Ve", got["Ve"]), ("mu", got["mu"]), ("pi", got["pi"]),
             ("Veps", got["Veps"]), ("J", got["J"]), ("epsilon", got["epsilon"]), ("s_Veps", mc["Veps"].ravel()), ("s_J", mc["J"].ravel()),
             ("s_epsilon", mc["epsilon"]), ("e", got["e"]), ("g", got["g"])] + list(extra)
    worst = {}
    for name, g in pairs:
        tol = 1000 * max(rel(a[name], b[name]), EPS)
        worst[name] = (rel(g, a[name]), tol)
    print("device vs restatement (rel. error, tolerance):", worst)
    bad = {k: v for k, v in worst.items() if not v[0] <= v[1]}
    assert not bad, bad


def restated(pr, G, model, Pi, fold=None, Cmat=None, R=None, X=None):
    X = pr["y_M"] if X is None else X
    return [E.ssbayes(pr["y"], X, model, Pi, yJ=pr["y_J"], G=G, index1=pr["index"], fold=fold, Cmat=Cmat, R=R,
                      rows=rows, jdot=jdot, **KW) for rows, jdot in (("asc", "chunk"), ("desc", "rev"))]


@pytest.mark.parametrize("model,Pi,fold", [("BayesCpi", [0.95, 0.05], None), ("BayesRR", [0.95, 0.05], None),
                                           ("BayesR", [0.95, 0.02, 0.02, 0.01], [0, 0.0001, 0.001, 0.01])])
def test_chain_on_the_demo_is_the_restatements(demo_ss, model, Pi, fold):
    pr = demo_ss["pr"]
    a, b = restated(pr, demo_ss["G"], model, Pi, fold)
    # through ssbrm() itself, which forwards the method and supplies its defaults of Pi and fold (R/ssbayes.r:216-223)
    samples = model == "BayesCpi"
    fit = H.ssbrm("T1 ~ 1", demo_ss["phe"], demo_ss["geno"], demo_ss["M_id"], demo_ss["ped"], method=model, verbose=False, gebv_samples=samples, **KW)
    got = dict(fit, epsilon=fit["epsilon"]["epsilon"], e=fit["e"]["e"][pr["y_indx"]], g=fit["u_last"])
    assert fit["epsilon"]["id"] == pr["Mn_id"] and fit["g"]["id"] == pr["M_id"] + pr["Mn_id"] and fit["e"]["id"] == pr["y_id"]
    assert fit["timing"]["resident_bits"] == 64 and fit["n_records"] == 8 and fit["model"] == "Single-step Bayesian model fit by [%s]" % model
    # g, R/ssbayes.r:325 and :337, from the posterior means and from the samples
    Mall, Jall = np.vstack([pr["M"], pr["Mn"]]), np.concatenate([pr["J"], pr["Jn"]])
    gebv = Mall @ a["alpha"] + Jall * a["J"]
    gebv[600:] += a["epsilon"]
    tol = 1000 * max(rel(a["alpha"], b["alpha"]), rel(a["epsilon"], b["epsilon"]), rel(a["J"], b["J"]), EPS)
    assert rel(fit["g"]["gebv"], gebv) <= tol
    if samples:
        assert fit["MCMCsamples"]["g"].shape == (1500, 8) and rel(fit["MCMCsamples"]["g"].mean(axis=1), gebv) <= tol
    compare_chain(got, a, b)
    assert got["MCMCsamples"]["epsilon"].shape == (900, 8) and got["MCMCsamples"]["Veps"].shape == (1, 8)


def test_chain_with_covariates_and_random_effects_keeps_the_draw_order(demo_ss):
    phe, ped = demo_ss["phe"], demo_ss["ped"]
    formula = "T1 ~ season + bwt + (1 | loc) + (1 | dam)"
    pr = H.ssbrm_prepare(formula, phe, demo_ss["geno"], demo_ss["M_id"], ped)
    G = (pr["Ai_nn"].indptr, pr["Ai_nn"].indices, pr["Ai_nn"].data)
    a, b = restated(pr, G, "BayesCpi", [0.95, 0.05], Cmat=pr["X"], R=pr["R"])
    fit = H.ssbrm(formula, phe, demo_ss["geno"], demo_ss["M_id"], ped, method="BayesCpi", verbose=False, **KW)
    got = dict(fit, epsilon=fit["epsilon"]["epsilon"], e=fit["e"]["e"][pr["y_indx"]], g=fit["u_last"])
    compare_chain(got, a, b, extra=[("beta", fit["beta"]), ("Vr", fit["Vr"])])


def test_layouts_give_one_chain_and_a_repeat_is_bit_identical(demo_ss):
    pr = demo_ss["pr"]
    X = np.clip(np.rint(pr["y_M"]), 0, 2).astype(np.int8)       # integer codes: every resident layout can hold them
    a, b = restated(pr, demo_ss["G"], "BayesCpi", [0.95, 0.05], X=X)
    kw = dict(epsl_y_J=pr["y_J"], epsl_Gi=demo_ss["G"], epsl_index=pr["index"], verbose=False, **KW)   # (the matrix as a CSC triple here)
    runs = {bits: H.Bayes(pr["y"], X, "BayesCpi", [0.95, 0.05], genotype_bits=bits, **kw) for bits in (8, 2, 64)}
    assert [runs[bits]["timing"]["resident_bits"] for bits in (8, 2, 64)] == [8, 2, 64]
    for bits in (8, 2, 64):
        compare_chain(runs[bits], a, b)
    again = H.Bayes(pr["y"], X, "BayesCpi", [0.95, 0.05], genotype_bits=8, **kw)
    for key in ("alpha", "epsilon", "g"):
        np.testing.assert_array_equal(again[key], runs[8][key])
    for key in ("alpha", "epsilon", "Veps", "J", "Vg", "Ve"):
        np.testing.assert_array_equal(again["MCMCsamples"][key], runs[8]["MCMCsamples"][key])
    for key in ("alpha", "epsilon"):   # int8 and 2 bits: the same chain bit for bit, as without the block
        np.testing.assert_array_equal(runs[2]["MCMCsamples"][key], runs[8]["MCMCsamples"][key])
    # store_epsilon = 0 keeps the running mean alone
    lean = H.Bayes(pr["y"], X, "BayesCpi", [0.95, 0.05], genotype_bits=8, store_epsilon=False, **kw)
    assert "epsilon" not in lean["MCMCsamples"]
    np.testing.assert_array_equal(lean["epsilon"], runs[8]["epsilon"])
    stored = runs[8]["MCMCsamples"]["epsilon"]
    assert np.all(np.abs(lean["epsilon"] - stored.mean(axis=1)) <= 16 * EPS * np.abs(stored).sum(axis=1) / stored.shape[1] + 1e-300)
    assert (lean["Veps"], lean["J"]) == (runs[8]["Veps"], runs[8]["J"])
    assert abs(runs[8]["Veps"] - runs[8]["MCMCsamples"]["Veps"].mean()) <= 8 * EPS * runs[8]["Veps"]


class _TwoRanks:
    """a communicator of two ranks as far as Bayes() looks at it before the library refuses"""
    world, rank = 2, 0

    def make_callback(self, count):
        return _lib.ALLREDUCE_FN(lambda buf, cnt, user: 1), None

    def max_int(self, v):
        return v


def test_refusals(demo_ss):
    pr = demo_ss["pr"]
    y, X = pr["y"], pr["y_M"]
    eps = dict(epsl_y_J=pr["y_J"], epsl_Gi=pr["Ai_nn"], epsl_index=pr["index"])
    kw = dict(verbose=False, **KW)

    def refused(status, text, model="BayesCpi", **more):
        with pytest.raises(H.HibayesError, match=text) as e:
            H.Bayes(y, X, model, [0.95, 0.05], **dict(kw, **more))
        assert e.value.status == status, str(e.value)

    refused(4, "the epsilon block is not sharded", comm=_TwoRanks(), m_global=2 * X.shape[1], **eps)
    Xi = np.clip(np.rint(X), 0, 2).astype(np.int8)
    with pytest.raises(H.HibayesError, match="the epsilon block is not available with shard_rows") as e:
        H.Bayes(y, Xi, "BayesCpi", [0.95, 0.05], shard_rows=True, **dict(kw, **eps))
    assert e.value.status == 4
    refused(4, "the epsilon block: a warm start", warm=dict(mu=0.0, vare=1.0, varg=1e-3, pi=[0.9, 0.1]), g_init=np.zeros(X.shape[1]), **eps)
    n = y.size
    refused(4, "the epsilon block is not available with BSLMM", model="BSLMM", Kival=np.ones(n), Ki=np.eye(n), **eps)
    refused(4, "the epsilon block is not available with BSLMM", model="BSLMM", **eps)
    refused(1, "variance-covariance matrix should be provided for epsilon term.", epsl_y_J=pr["y_J"], epsl_index=pr["index"])
    refused(1, "go together", epsl_Gi=pr["Ai_nn"], epsl_index=pr["index"])
    refused(1, "go together", epsl_Gi=pr["Ai_nn"], epsl_y_J=pr["y_J"])
    refused(1, "epsl_index: an index is outside 1 .. q", epsl_y_J=pr["y_J"], epsl_Gi=pr["Ai_nn"], epsl_index=np.full(pr["index"].size, 901))
    refused(1, "must be symmetric", epsl_y_J=pr["y_J"], epsl_Gi=sp.triu(pr["Ai_nn"]).tocsc(), epsl_index=pr["index"])
    with pytest.raises(H.HibayesError, match="call hb_ctx_epsl_setup first"):
        with H.Context(8, 4) as c:
            c.epsl_step(1.0, 1.0, 1, 0, 0.0, 1.0, 0.0)
    # the library's own texts for an incomplete descriptor (what a C caller or the shim meets; Bayes() answers earlier)
    G = sp.csc_matrix(pr["Ai_nn"])
    ip, ix, dt = G.indptr.astype(np.int64), G.indices.astype(np.int32), G.data
    gi = _lib.EpslGi(900, 3, ip.ctypes.data, ix.ctypes.data, dt.ctypes.data)
    idx, yj = np.array([1, 2, 3], dtype=np.uint32), np.ones(8)
    with H.Context(8, 4) as c:
        for desc, text in ((_lib.EpslDesc(None, idx.ctypes.data, yj.ctypes.data), "variance-covariance matrix should be provided for epsilon term."),
                           (_lib.EpslDesc(C.pointer(gi), None, yj.ctypes.data), "epsl_y_J, epsl_Gi and epsl_index go together"),
                           (_lib.EpslDesc(C.pointer(gi), idx.ctypes.data, None), "epsl_y_J, epsl_Gi and epsl_index go together")):
            assert c.L.hb_ctx_epsl_setup(c.h, C.byref(desc)) == 1
            assert text in c.L.hb_last_error().decode()


def test_a_run_without_the_block_drops_it_from_a_callers_context(demo_ss):
    pr = demo_ss["pr"]
    X = np.clip(np.rint(pr["y_M"]), 0, 2).astype(np.int8)
    kw = dict(niter=6, nburn=2, thin=2, seed=3, verbose=False)
    with H.Context(X.shape[0], X.shape[1]) as c:
        c.upload(X)
        with_block = H.Bayes(pr["y"], None, "BayesCpi", [0.95, 0.05], ctx=c, epsl_y_J=pr["y_J"], epsl_Gi=pr["Ai_nn"], epsl_index=pr["index"], **kw)
        c.epsl_step(1.0, 1.0, 1, 0, 0.0, 900.0, 0.0)                      # the run left its block on the context
        plain = H.Bayes(pr["y"], None, "BayesCpi", [0.95, 0.05], ctx=c, **kw)
        with pytest.raises(H.HibayesError, match="call hb_ctx_epsl_setup first"):
            c.epsl_step(1.0, 1.0, 1, 0, 0.0, 900.0, 0.0)
    with H.Context(X.shape[0], X.shape[1]) as c2:                          # the same run on a context that never held a block
        c2.upload(X)
        alone = H.Bayes(pr["y"], None, "BayesCpi", [0.95, 0.05], ctx=c2, **kw)
    assert "Veps" in with_block and "Veps" not in plain
    np.testing.assert_array_equal(plain["MCMCsamples"]["alpha"], alone["MCMCsamples"]["alpha"])
