"""The device eigensolver (hibayes_amd/csrc/hb_eig.hip, hibayes_amd/eig.py): the reduction alone, the pair, determinism, refusals, and BSLMM end to
end with neither G nor K on the host. Every error measure is asserted against the same measure of LAPACK's own pipeline (dsytrd -> dstemr ->
dormtr, tests/eig_restatement.py) on the same matrix, computed here: device <= MARGIN * LAPACK + n, in units of eps. Both are backward stable with
the same first-order bound c n eps ||G||, are fed the same kind of Z by the same dstemr and differ in blocking and summation order only, hence
MARGIN = 4; the floor n eps is there because the reference can be luckily small. HB_EIG_ACCURACY_OUT=<file> appends every measured pair to it
(profiles/eig_accuracy.txt was written that way)."""
import os

import numpy as np
import pytest

import hibayes_amd as H
from hibayes_amd import eig as HE

import bslmm_restatement as B
import eig_restatement as E

pytestmark = pytest.mark.gpu
EPS = E.EPS
MARGIN = 4
NB = 64          # EIG_NB of hb_eig.hip
LAMBDA = 0.01
KW = dict(niter=60, nburn=20, thin=2, seed=20251019)


def judge(case, n, measures):
    """measures: {name: (device, LAPACK)} in eps. Prints and records every pair, then asserts all of them."""
    lines = ["%-28s n=%-4d %-8s device %10.2f eps   LAPACK %10.2f eps   ratio %6.2f" % (case, n, k, a, b, a / b if b > 0 else float("inf") if a > 0 else 1.0)
             for k, (a, b) in measures.items()]
    print("\n".join(lines))
    out = os.environ.get("HB_EIG_ACCURACY_OUT")
    if out:
        with open(out, "a") as f:
            f.write("\n".join(lines) + "\n")
    bad = {k: v for k, v in measures.items() if not v[0] <= MARGIN * v[1] + n}
    assert not bad, bad


def tri(d, e):
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


def reduction_measures(G, Q, d, e):
    n, scale = G.shape[0], max(E.norm2(G), 1e-300)
    wr = np.linalg.eigvalsh(G)
    wt = E.tridiagonal_eigh(d, e)[0]
    return {"Q orth": E.orth_eps(Q), "Q'GQ - T": float(np.max(np.abs(Q.T @ G @ Q - tri(d, e)))) / scale / EPS,
            "eig(T)": float(np.max(np.abs(wt - wr))) / max(float(np.max(np.abs(wr))), 1e-300) / EPS}


def pair_measures(G, w, K):
    wr = np.linalg.eigvalsh(G)
    return {"res": E.res_eps(G, w, K), "orth": E.orth_eps(K), "values": float(np.max(np.abs(w - wr))) / max(float(np.max(np.abs(wr))), 1e-300) / EPS}


def lapack_all(G):
    n = G.shape[0]
    c, d, e, tau = E.lapack_tridiagonal(G)
    Q = E.lapack_back_transform(c, tau, np.eye(n))
    w, Z = E.tridiagonal_eigh(d, e)
    return reduction_measures(G, Q, d, e), pair_measures(G, w, E.lapack_back_transform(c, tau, Z))


def device_all(G):
    """the reduction alone (Z = identity) and the pair, from one reduction"""
    with HE.Reduction(HE.upload(G)) as red:
        with red.vectors() as Qh:
            Q = Qh.toarray()
        w, Z = HE.tridiagonal_eigh(red.d, red.e)
        with red.vectors(Z, w) as Kh:
            K = Kh.toarray()
        Ap, tau = red.reflectors()
        d, e = red.d.copy(), red.e.copy()
        red.A.close()
    return dict(Q=Q, d=d, e=e, w=w, K=K, Ap=Ap, tau=tau)


def check_matrix(case, G):
    n = G.shape[0]
    dev = device_all(G)
    ref_red, ref_pair = lapack_all(G)
    assert np.all(np.diff(dev["w"]) >= 0)
    # the packed matrix is dsytrd's: d on the diagonal, e below it, and Q rebuilt from the reflectors is the Q the device applied
    assert np.array_equal(np.diag(dev["Ap"]), dev["d"]) and np.array_equal(np.diag(dev["Ap"], -1), dev["e"])
    assert np.all((dev["tau"] >= 0) & (dev["tau"] <= 2))
    if n > 1:
        assert dev["tau"][-1] == 0.0
        Qr = E.back_transform(E.reflectors_from_packed(dev["Ap"], dev["tau"]), dev["tau"])
        assert np.max(np.abs(Qr - dev["Q"])) <= (MARGIN * ref_red["Q orth"] + n) * EPS
    m = {k: (v, ref_red[k]) for k, v in reduction_measures(G, dev["Q"], dev["d"], dev["e"]).items()}
    m.update({k: (v, ref_pair[k]) for k, v in pair_measures(G, dev["w"], dev["K"]).items()})
    judge(case, n, m)
    return dev


@pytest.mark.parametrize("n,m,lam", E.grm_cases(NB))
def test_grm_matrices_reduction_and_pair(n, m, lam):
    dev = check_matrix("grm m=%d lambda=%g" % (m, lam), E.grm_case(n, m, lam))
    if n == 1:
        assert dev["K"].tolist() == [[1.0]] and dev["w"][0] == E.grm_case(n, m, lam)[0, 0]
    if n == 2:
        assert dev["tau"][0] == 0.0                                   # no reflector: H = I


def crafted():
    rng = np.random.default_rng(11)
    G = E.grm_case(140, 300, .01)
    G[:, 77] = G[:, 3]
    G[77, :] = G[3, :]
    G[77, 77] = G[3, 3]
    return {"diagonal": np.diag(rng.uniform(0.5, 2.0, 131)), "multiple of I": 1.75 * np.eye(70), "two identical rows": np.asfortranarray(G)}


@pytest.mark.parametrize("name", ["diagonal", "multiple of I", "two identical rows"])
def test_crafted_inputs_through_eigh(name):
    G = crafted()[name]
    n = G.shape[0]
    w, K = H.eigh(G)
    assert K.shape == (n, n) and K.flags.f_contiguous and np.all(np.diff(w) >= 0)
    _, ref = lapack_all(G)
    judge(name, n, {k: (v, ref[k]) for k, v in pair_measures(G, w, K).items()})
    if name != "two identical rows":                                   # every reflector has tau = 0
        with HE.Reduction(HE.upload(G)) as red:
            Ap, tau = red.reflectors()
            assert np.all(tau == 0) and np.all(red.e == 0) and np.array_equal(red.d, np.diag(G))
            red.A.close()
    with H.eigh(G, keep_on_device=True) as Kh:
        assert Kh.shape == (n, n) and Kh.ld % 2 == 0 and Kh.ld >= n
        assert np.array_equal(Kh.values, w) and np.array_equal(Kh.toarray(), K)


def codes(n, m, seed=0):
    return np.random.default_rng(7000 * n + m + seed).integers(0, 3, size=(n, m)).astype(np.int8)


@pytest.mark.parametrize("n,m", [(2, 5), (3, 7), (17, 63), (NB + 1, 200), (129, 64), (300, 120)])
def test_make_grm_device_route_from_resident_genotypes(n, m):
    """G goes from hb_grm_build's device copy (leading dimension n: odd n takes the mat-vec's unaligned variant) straight into the reduction"""
    M = codes(n, m)
    with H.Context(n, m) as c:
        c.upload(M)
        G = c.grm(lambda_=LAMBDA)
        w, K = H.make_grm(c, LAMBDA, eigen=True, verbose=False, eigen_solver="device")
    _, ref = lapack_all(G)
    assert np.all(np.diff(w) >= 0)
    judge("make_grm m=%d" % m, n, {k: (v, ref[k]) for k, v in pair_measures(G, w, K).items()})
    # the default route is the host's, byte for byte
    wh, Kh = H.make_grm(M, LAMBDA, eigen=True, verbose=False)
    wn, Kn = np.linalg.eigh(G)
    assert np.array_equal(wh, wn) and np.array_equal(Kh, Kn)


@pytest.mark.parametrize("n,m", [(129, 64), (300, 1000)])
def test_two_runs_agree_bit_for_bit(n, m):
    G = E.grm_case(n, m, LAMBDA)
    a, b = device_all(G), device_all(G)
    for key in ("d", "e", "tau", "Ap", "Q", "K", "w"):
        assert np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize("tridiagonal", ["host", "device"])
@pytest.mark.parametrize("n", [130, 70])
def test_eigh_is_bit_for_bit_the_recorded_pair(n, tridiagonal):
    """The measures above bound the error and would not notice a reordered fp64 accumulation in the matrix-core kernels; this does. The pair was
    recorded from an earlier build of this library (tests/golden/eigh_device.txt names the commit and the shapes' reasons)."""
    rec = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eigh_device_n%d.npz" % n))
    w, K = H.eigh(E.grm_case(n, 200, LAMBDA), tridiagonal=tridiagonal)
    assert np.array_equal(w, rec["w_" + tridiagonal]) and np.array_equal(K, rec["K_" + tridiagonal])


def test_refusals():
    G = E.grm_case(40, 90, LAMBDA)
    bad = G.copy()
    bad[17, 5] = bad[5, 17] = np.nan
    with pytest.raises(H.HibayesError, match="the matrix holds a non-finite value") as ex:
        H.eigh(bad)
    assert ex.value.status == 1
    with pytest.raises(H.HibayesError, match="leading dimension smaller than n") as ex:
        HE.upload(G, lda=39)
    assert ex.value.status == 1
    A = HE.upload(G)
    red = HE.Reduction(A)
    K = red.vectors()
    K.close()
    with pytest.raises(H.HibayesError, match="has been closed") as ex:
        K.toarray()
    assert ex.value.status == 1
    red.close()
    with pytest.raises(H.HibayesError, match="has been closed") as ex:
        red.vectors()
    assert ex.value.status == 1
    A.close()
    with pytest.raises(H.HibayesError, match="has been closed"):
        HE.Reduction(A)
    with H.Context(40, 4) as c, H.eigh(E.grm_case(17, 63, LAMBDA), keep_on_device=True) as small:
        c.upload(np.zeros((40, 4), dtype=np.int8))
        with pytest.raises(ValueError, match="poly_setup"):
            c.poly_setup(small.values, small)
    w, K = H.eigh(G)                                                   # and the device is still fine
    assert E.res_eps(G, w, K) <= 64 * 40


# ---------------------------------------------------------------------------------------------------------------------------------
# BSLMM end to end on the demo: neither G nor K on the host
# ---------------------------------------------------------------------------------------------------------------------------------
def gamma(k):
    return k * EPS / (1 - k * EPS)


def test_polygenic_block_on_the_device_pair(demo):
    M = demo["M"]
    n = M.shape[0]
    rng = np.random.default_rng(5)
    yadj, u = rng.normal(size=n), rng.normal(size=n)
    vare, vb, chis, s2_df, seed, it = 0.7, 0.4, float(n) + 3.5, 0.3, 987654321, 11
    with H.make_grm(M, LAMBDA, eigen=True, verbose=False, eigen_solver="device", keep_on_device=True) as Kh, H.Context(n, 4) as c:
        Kval, K = Kh.values, Kh.toarray()
        c.upload(np.zeros((n, 4), dtype=np.int8))
        c.poly_setup(Kval, Kh)
        c.set_residual(yadj, u)
        c.poly_step(vare, vb, seed, it, chis, s2_df)
        k, vb1, q, flag = c.poly_state()
        dbg = c.poly_debug()
    assert not flag and np.all(Kval > 0)
    ld_ = np.longdouble
    Kl = K.astype(ld_)
    # the existing test's bounds (tests/test_gpu_bslmm.py), on the downloaded pair
    assert np.all(np.abs(dbg["t"] - Kl.T @ yadj.astype(ld_)) <= gamma(n + 1) * (np.abs(K).T @ np.abs(yadj)) + 1e-300)
    w = dbg["w"].astype(ld_)
    assert np.all(np.abs(k - Kl @ w) <= gamma(n) * (np.abs(K) @ np.abs(dbg["w"])))
    assert np.all(np.abs(dbg["Kg"] - Kl.T @ k.astype(ld_)) <= gamma(n) * (np.abs(K).T @ np.abs(k)))
    z = B.poly_normals(seed, it, n)
    ref = B.poly_block(Kl, Kval.astype(ld_), yadj.astype(ld_), u.astype(ld_), np.zeros(n, dtype=ld_), ld_(vare), ld_(vb), z.astype(ld_), ld_(chis), ld_(s2_df))
    rel = float(np.max(np.abs(k - ref["k"].astype(np.float64))) / np.max(np.abs(ref["k"].astype(np.float64))))
    assert rel < 1e-11 and abs(vb1 - float(ref["vb"])) < 1e-11 * float(ref["vb"])


def test_ibrm_device_route_is_the_restatements_chain_on_the_downloaded_pair(demo):
    import test_gpu_bslmm as TB
    pl, phe = demo["plink"], demo["phe"]
    fit = H.ibrm("T1 ~ 1", data=phe, M=pl["geno"], M_id=demo["ids"], method="BSLMM", lambda_=LAMBDA, verbose=False, eigen_solver="device", **KW)
    Kval, K = H.make_grm(demo["M"], LAMBDA, eigen=True, verbose=False, eigen_solver="device")      # (bit for bit the pair ibrm() held on the device)
    a = B.bslmm(demo["y"], demo["M"], [0.95, 0.05], Kival=Kval, Ki=K, order="blas", **KW)
    b = B.bslmm(demo["y"], demo["M"], [0.95, 0.05], Kival=Kval, Ki=K, order="rev", **KW)
    got = dict(fit)
    got["e"] = fit["e"]["e"]
    TB.compare_chain(got, a, b)
    assert fit["n_records"] == 20 and len(fit["g"]["gebv"]) == 600 and np.all(np.isfinite(fit["g"]["gebv"]))
