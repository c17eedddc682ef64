"""BSLMM on the device (hibayes_amd/csrc/hb_grm.hip): hb_grm_build against exact rational values, one polygenic block against the numpy
restatement evaluated in long double with the dot-product bound, and whole chains against the restatement (tests/bslmm_restatement.py)
within 1000 times its own order-to-order spread. The whole file takes about 12 s on an MI355X."""
import numpy as np
import pytest

import hibayes_amd as H

import bslmm_restatement as B

pytestmark = pytest.mark.gpu
EPS = B.EPS
KW = dict(niter=60, nburn=20, thin=2, seed=20251019)
LAMBDA = 0.01


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


# ---------------------------------------------------------------------------------------------------------------------------------
# GRM
# ---------------------------------------------------------------------------------------------------------------------------------
def codes_matrix(n, m, lo, hi, seed):
    return np.random.default_rng(seed).integers(lo, hi + 1, size=(n, m)).astype(np.int8)


@pytest.mark.parametrize("lo,hi", [(0, 2), (0, 3), (-1, 1)])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("n", [2, 17, 64, 300])
def test_grm_within_the_stated_bound_of_the_exact_values(n, m, lo, hi):
    M = codes_matrix(n, m, lo, hi, 1000 * n + m)
    with H.Context(n, m) as c:
        c.upload(M)
        raw = c.grm(raw=True)
        if n <= 64:
            err, bound = B.grm_raw_error(M, raw)
        else:               # (n = 300: the exact rationals on rows around the tile edges, the expression's own value everywhere below)
            err, bound = _sampled_error(M, raw, [0, 1, 127, 128, 129, 255, 256, 299])
        assert np.all(err <= bound), float(np.max(err / np.maximum(bound, 1e-300)))
        assert np.array_equal(raw, B.grm_expression(M))        # one fixed expression: the host's evaluation of it, bit for bit
        assert np.array_equal(raw, raw.T)
        if not np.any(np.diag(raw) > 0):
            return
        G = c.grm(lambda_=0.25)
        Gx, gb = B.grm_scaled_bound(M, 0.25)
        assert np.all(np.abs(G.astype(np.longdouble) - Gx) <= gb), float(np.max(np.abs(G.astype(np.longdouble) - Gx) / gb))
        assert np.array_equal(G, G.T)
        assert np.array_equal(G, c.grm(lambda_=0.25))                       # two builds, bit for bit
        G0 = c.grm(lambda_=0.0)
        off = ~np.eye(n, dtype=bool)
        assert np.array_equal(G[off], G0[off])                              # lambda lands on the diagonal only
        assert np.array_equal(np.diag(G), np.diag(G0) + 0.25)


def _sampled_error(M, raw, rows):
    S, a, Cc = B.grm_integers(M)
    n = M.shape[0]
    err, bound = [], []
    for i in rows:
        for j in range(n):
            N = n * n * int(S[i, j]) - n * (int(a[i]) + int(a[j])) + Cc
            p, q = float(raw[i, j]).as_integer_ratio()
            err.append(abs(p * n * n - N * q) / (q * n * n))
            bound.append(4 * EPS * (abs(int(S[i, j])) + abs(int(a[i]) + int(a[j])) / n + Cc / (n * n)))
    return np.array(err), np.array(bound)


def test_grm_hands_over_to_int64_before_int32_overflows():
    n, m = 17, 140000                                           # S_ii = 127^2 m = 2.26e9 > 2^31
    M = (np.random.default_rng(5).integers(0, 2, size=(n, m)) * 254 - 127).astype(np.int8)
    with H.Context(n, m) as c:
        c.upload(M)
        raw = c.grm(raw=True)
    S, _, _ = B.grm_integers(M)
    assert S[0, 0] == 127 * 127 * m > 2 ** 31
    err, bound = B.grm_raw_error(M, raw)
    assert np.all(err <= bound), float(np.max(err / bound))


def test_grm_refuses_all_monomorphic_markers():
    M = np.ones((17, 70), dtype=np.int8) * np.arange(70, dtype=np.int8)[None, :] % 3
    with H.Context(17, 70) as c:
        c.upload(M.astype(np.int8))
        with pytest.raises(H.HibayesError, match="every marker is monomorphic") as e:
            c.grm()
        assert e.value.status == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# one polygenic block
# ---------------------------------------------------------------------------------------------------------------------------------
def block_case(n, seed=3):
    rng = np.random.default_rng(seed + n)
    K, _ = np.linalg.qr(rng.normal(size=(n, n)))
    Kval = rng.uniform(0.05, 3.0, n)
    return dict(K=np.asfortranarray(K), Kval=Kval, yadj=rng.normal(size=n), u=rng.normal(size=n), vare=0.7, vb=0.4, chis=float(n) + 3.5,
                s2_df=0.3, seed=987654321, it=11)


def gamma(k):
    return k * EPS / (1 - k * EPS)


def run_block(c, cs, device_K, steps=1, go_on=0):
    """`steps` single blocks, each from the same state (k = 0, the case's residual), then `go_on` more that continue the last one with
    the device's own vb"""
    buf = None
    if device_K:
        torch = pytest.importorskip("torch")
        n = c.n
        buf = torch.zeros((n, n + (n & 1)), dtype=torch.float64, device="cuda")
        buf[:, :n] = torch.from_numpy(np.ascontiguousarray(cs["K"].T)).cuda()   # row j of the tensor = column j of K
    out = []
    for s in range(steps + go_on):
        if s < steps:
            if device_K:
                c.poly_setup(cs["Kval"], buf, on_device=True)
            else:
                c.poly_setup(cs["Kval"], cs["K"])
            c.set_residual(cs["yadj"], cs["u"])
        c.poly_step(cs["vare"], cs["vb"] if s < steps else -1.0, cs["seed"], cs["it"] + max(0, s - steps + 1), cs["chis"], cs["s2_df"])
        k, vb, q, flag = c.poly_state()
        r, u = c.get_residual()
        out.append(dict(k=k, vb=vb, q=q, flag=flag, r=r, u=u, dbg=c.poly_debug(), mir=c.mirrors()))
    return out


@pytest.mark.parametrize("device_K", [False, True])
@pytest.mark.parametrize("n", [2, 63, 65, 257, 1025])
def test_one_block_against_the_long_double_restatement(n, device_K):
    cs = block_case(n)
    ld_ = np.longdouble
    K, Kval = cs["K"].astype(ld_), cs["Kval"].astype(ld_)
    with H.Context(n, 4) as c:
        c.upload(np.zeros((n, 4), dtype=np.int8))
        a, b, nxt = run_block(c, cs, device_K, steps=2, go_on=1)
    d = a["dbg"]
    z = B.poly_normals(cs["seed"], cs["it"], n)
    k_old = np.zeros(n)
    # t = K'(yadj + k_old): n products and the addition in front of them
    p = (cs["yadj"] + k_old).astype(ld_)
    assert np.all(np.abs(d["t"] - K.T @ p) <= gamma(n + 1) * (np.abs(K).T @ np.abs(p)).astype(np.float64) + 1e-300)
    # w from the device's own t: a handful of roundings and the device's log / cos in the normal
    ev = (cs["Kval"] * cs["vare"]) / (cs["Kval"] + cs["vare"] / cs["vb"])
    np.testing.assert_allclose(d["eval"], ev, rtol=4 * EPS)
    wa, wb = (ev / cs["vare"]) * d["t"], np.sqrt(ev) * z
    assert np.all(np.abs(d["w"] - (wa + wb)) <= 1e-13 * (np.abs(wa) + np.abs(wb)))
    # k_new = K w and Kg = K' k_new, each from the device's own operand: the dot-product bound gamma_n sum |terms|
    w, kn = d["w"].astype(ld_), a["k"].astype(ld_)
    assert np.all(np.abs(a["k"] - K @ w) <= gamma(n) * (np.abs(K) @ np.abs(w)).astype(np.float64))
    assert np.all(np.abs(d["Kg"] - K.T @ kn) <= gamma(n) * (np.abs(K).T @ np.abs(kn)).astype(np.float64))
    # q, vb: consistent with Kg; the residual moved by k_old - k_new and u by its negative: yadj + u is conserved to rounding
    terms = d["Kg"] ** 2 / cs["Kval"]
    assert abs(a["q"] - float(np.sum(terms.astype(ld_)))) <= gamma(n + 2) * float(np.sum(terms))
    assert a["vb"] == (a["q"] + cs["s2_df"]) / cs["chis"]
    assert not a["flag"]
    np.testing.assert_array_equal(a["r"], cs["yadj"] + (k_old - a["k"]))
    np.testing.assert_array_equal(a["u"], cs["u"] - (k_old - a["k"]))
    assert np.all(np.abs((a["r"] + a["u"]) - (cs["yadj"] + cs["u"])) <= 2 * EPS * (np.abs(a["r"]) + np.abs(a["u"])))
    # the residual's fp32 mirror, as k_axpy leaves it
    np.testing.assert_array_equal(a["mir"]["r32"][:n], a["r"].astype(np.float32))
    np.testing.assert_array_equal(a["mir"]["r"][:n], a["r"])
    # the whole block against the restatement in long double, loosely (the staged checks above are the sharp ones)
    ref = B.poly_block(K, Kval, cs["yadj"].astype(ld_), cs["u"].astype(ld_), k_old.astype(ld_), ld_(cs["vare"]), ld_(cs["vb"]), z.astype(ld_),
                       ld_(cs["chis"]), ld_(cs["s2_df"]))
    assert rel(a["k"], ref["k"]) < 1e-11 and abs(a["vb"] - float(ref["vb"])) < 1e-11 * float(ref["vb"])
    # two steps from equal state: bit for bit
    for key in ("k", "r", "u"):
        np.testing.assert_array_equal(a[key], b[key])
    assert (a["vb"], a["q"]) == (b["vb"], b["q"])
    # the next iteration goes on from k and from the vb on the device: t = K'(yadj + k_old) with k_old != 0, eval from that vb
    d2 = nxt["dbg"]
    p2 = (a["r"] + a["k"]).astype(ld_)
    assert np.all(np.abs(d2["t"] - K.T @ p2) <= gamma(n + 1) * (np.abs(K).T @ np.abs(p2)).astype(np.float64) + 1e-300)
    np.testing.assert_allclose(d2["eval"], (cs["Kval"] * cs["vare"]) / (cs["Kval"] + cs["vare"] / a["vb"]), rtol=4 * EPS)
    np.testing.assert_array_equal(nxt["r"], a["r"] + (a["k"] - nxt["k"]))
    np.testing.assert_array_equal(nxt["u"], a["u"] - (a["k"] - nxt["k"]))
    assert not np.array_equal(nxt["k"], a["k"])


def test_a_clearly_negative_eigenvalue_is_refused_with_the_references_text(demo):
    cs = block_case(65)
    cs["Kval"][7] = -0.5
    with H.Context(65, 4) as c:
        c.upload(np.zeros((65, 4), dtype=np.int8))
        out = run_block(c, cs, False)[0]
    assert out["flag"]
    Kval, K = H.make_grm(demo["M"], LAMBDA, eigen=True, verbose=False)
    Kval = Kval.copy()
    Kval[:3] = -1.0
    with pytest.raises(H.HibayesError, match="matrix is not positive definite, try to specify parameter 'lambda' with a small value, eg: 0.001 or bigger") as e:
        H.Bayes(demo["y"], demo["M"], "BSLMM", [0.95, 0.05], Kival=Kval, Ki=K, verbose=False, **KW)
    assert e.value.status == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# whole chains on the demo
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eig(demo):
    return H.make_grm(demo["M"], LAMBDA, eigen=True, verbose=False)


def full_formula(demo):
    """y, genotypes, fixed-effect matrix and random-effect columns of ibrm("T1 ~ season + bwt + (1 | loc) + (1 | dam)") on the demo"""
    from hibayes_amd import bayes as hb
    phe, ids = demo["phe"], demo["ids"]
    pos = {}
    for i, v in enumerate([str(v) for v in phe["id"]]):
        pos.setdefault(v, i)
    match = [pos.get(v, -1) for v in ids]
    cols = {nm: [phe[nm][j] if j >= 0 else None for j in match] for nm in ("T1", "season", "bwt", "loc", "dam")}
    na = np.zeros(len(ids), dtype=bool)
    for nm in cols:
        na |= np.array([hb._isna(v) for v in cols[nm]])
    rows = np.flatnonzero(~na)
    Xfix, _ = hb._model_matrix(cols, ["season", "bwt"], rows)
    R = np.array([[str(cols[p][i]) for i in rows] for p in ("loc", "dam")], dtype=object).T
    y = np.array([float(cols["T1"][i]) for i in rows])
    return y, np.asfortranarray(demo["plink"]["geno"][rows, :]), Xfix, R


def compare_chain(got, a, b):
    """got (the device) against restatement a, every quantity within 1000 times the restatement's own order-to-order spread |a - b|
    (relative to the quantity's largest magnitude), with the floor of one rounding of that magnitude times 1000."""
    pairs = [("s_alpha", got["MCMCsamples"]["alpha"]), ("k", got["k"]), ("Va", got["Va"]), ("Vb", got["Vb"]), ("Vg", got["Vg"]), ("Ve", got["Ve"]),
             ("mu", got["mu"]), ("pi", got["pi"]), ("ghat", got["ghat"]), ("s_Vb", got["MCMCsamples"]["Vb"].ravel()), ("alpha", got["alpha"]),
             ("e", got["e"])]
    worst = {}
    for name, g in pairs:
        tol = 1000 * max(rel(a[name], b[name]), EPS)
        worst[name] = (rel(g, a[name]), tol)
    print("device vs restatement (rel. error, tolerance):", worst)
    bad = {k: v for k, v in worst.items() if not v[0] <= v[1]}
    assert not bad, bad


def test_chain_on_the_demo_is_the_restatements(demo, eig):
    Kval, K = eig
    got = H.Bayes(demo["y"], demo["M"], "BSLMM", [0.95, 0.05], Kival=Kval, Ki=K, verbose=False, **KW)
    a = B.bslmm(demo["y"], demo["M"], [0.95, 0.05], Kival=Kval, Ki=K, order="blas", **KW)
    b = B.bslmm(demo["y"], demo["M"], [0.95, 0.05], Kival=Kval, Ki=K, order="rev", **KW)
    compare_chain(got, a, b)
    assert got["n_records"] == 20 and got["MCMCsamples"]["Va"].shape == (1, 20)


def test_chain_with_covariates_and_random_effects_keeps_the_draw_order(demo):
    y, M, Xfix, R = full_formula(demo)
    Kval, K = H.make_grm(M, LAMBDA, eigen=True, verbose=False)
    got = H.Bayes(y, M, "BSLMM", [0.95, 0.05], Kival=Kval, Ki=K, C_=Xfix, R=R, verbose=False, **KW)
    a = B.bslmm(y, M, [0.95, 0.05], Kival=Kval, Ki=K, Cmat=Xfix, R=R, order="blas", **KW)
    b = B.bslmm(y, M, [0.95, 0.05], Kival=Kval, Ki=K, Cmat=Xfix, R=R, order="rev", **KW)
    compare_chain(got, a, b)
    tol = 1000 * max(rel(a["beta"], b["beta"]), rel(a["Vr"], b["Vr"]), EPS)
    assert rel(got["beta"], a["beta"]) <= tol and rel(got["Vr"], a["Vr"]) <= tol


def test_layouts_and_repeats_give_one_chain_bit_for_bit(demo, eig):
    Kval, K = eig
    runs = [H.Bayes(demo["y"], demo["M"], "BSLMM", [0.95, 0.05], Kival=Kval, Ki=K, verbose=False, genotype_bits=bits, **KW) for bits in (8, 2, 8)]
    assert [r["timing"]["resident_bits"] for r in runs] == [8, 2, 8]
    for r in runs[1:]:
        for key in ("alpha", "k", "ghat", "g"):
            np.testing.assert_array_equal(r[key], runs[0][key])
        np.testing.assert_allclose(r["e"], runs[0]["e"], rtol=0, atol=1e-10)   # (X * alpha sums its column blocks with atomics: last bits)
        for key in ("alpha", "Va", "Vb", "Vg", "Ve"):
            np.testing.assert_array_equal(r["MCMCsamples"][key], runs[0]["MCMCsamples"][key])
    # without store_alpha the posterior alpha still includes ghat
    r = H.Bayes(demo["y"], demo["M"], "BSLMM", [0.95, 0.05], Kival=Kval, Ki=K, verbose=False, store_alpha=False, **KW)
    assert "alpha" not in r["MCMCsamples"]
    np.testing.assert_allclose(r["alpha"], runs[0]["alpha"], rtol=0, atol=1e-12 * np.max(np.abs(runs[0]["alpha"])))
    np.testing.assert_array_equal(r["ghat"], runs[0]["ghat"])
    assert np.max(np.abs(r["ghat"])) > 0


def test_ibrm_bslmm_is_bayes_on_make_grms_output(demo):
    pl, phe = demo["plink"], demo["phe"]
    fit = H.ibrm("T1 ~ 1", data=phe, M=pl["geno"], M_id=demo["ids"], method="BSLMM", lambda_=LAMBDA, verbose=False, niter=60, nburn=20, thin=2,
                 seed=KW["seed"])
    Kval, K = H.make_grm(demo["M"], LAMBDA, eigen=True, verbose=False)
    ref = H.Bayes(demo["y"], demo["M"], "BSLMM", [0.95, 0.05], Kival=Kval, Ki=K, verbose=False, **KW)
    for key in ("alpha", "k", "ghat"):
        np.testing.assert_array_equal(fit[key], ref[key])
    np.testing.assert_array_equal(fit["MCMCsamples"]["Vb"], ref["MCMCsamples"]["Vb"])
    assert len(fit["g"]["gebv"]) == 600 and np.all(np.isfinite(fit["g"]["gebv"]))
    for key in ("Va", "Vb", "Vg", "Ve", "mu", "h2"):
        assert np.isfinite(fit[key])
    assert np.all(np.isfinite(fit["alpha"])) and np.all(np.isfinite(fit["e"]["e"]))


def test_refusals(demo, eig):
    Kval, K = eig
    y, M = demo["y"], demo["M"]
    for kw in (dict(Kival=Kval), dict(Ki=K), dict()):
        with pytest.raises(H.HibayesError, match=r"BSLMM \(Ki/Kival\) is not part of the GPU path") as e:
            H.Bayes(y, M, "BSLMM", [0.95, 0.05], verbose=False, **kw, **KW)
        assert e.value.status == 4
    with pytest.raises(H.HibayesError, match=r"BSLMM \(Ki/Kival\) is not part of the GPU path"):
        H.Bayes(y, M, "BayesCpi", [0.95, 0.05], Kival=Kval, Ki=K, verbose=False, **KW)
    warm = dict(mu=0.0, vare=1.0, varg=1e-3, pi=[0.9, 0.1])
    with pytest.raises(H.HibayesError, match="warm start") as e:
        H.Bayes(y, M, "BSLMM", [0.95, 0.05], Kival=Kval, Ki=K, warm=warm, g_init=np.zeros(M.shape[1]), verbose=False, **KW)
    assert e.value.status == 4
    with pytest.raises(H.HibayesError, match="shard_rows") as e:
        H.Bayes(y, M, "BSLMM", [0.95, 0.05], Kival=Kval, Ki=K, shard_rows=True, verbose=False, **KW)
    assert e.value.status == 4
