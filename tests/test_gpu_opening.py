"""What every chain kernel of a sweep trusts at its opening, read back and held against plain numpy (tests/opening_restatement.py, itself
tested in tests/test_opening_host.py), with equality throughout:

  a. the Gram band's blocks (k_gram, k_gram_tiled: every stored (p, l), not the diagonal alone) and the certificate's three arrays
     (hb_build_gcert: k_g16_ab, k_gcmax) against exact integers — Context.cert() is hb_ctx_debug_get_cert;
  b. the certificate as state: after a second upload, after a wider band, after the int8 copy was dropped, and where there is none;
  c. the opening filter, the 16-byte opening records and the row-cache lists k_hotlist writes — Context.opening() is
     hb_ctx_debug_get_opening — after one pipelined sweep whose effects set_effects() installed, at ordinary hyper-parameters.

A gcmax that is too small makes the certified check unsound, a filter word above the fp64 threshold drops a marker that should have been
decided exactly, a slot outside the cache makes the chain read another row: each shows in a whole chain only on a rare draw, and here on
every input."""
import math

import numpy as np
import pytest

import hibayes_amd as H
import opening_restatement as R
from test_gpu_ld import geno_ld
from test_opening_host import N_WIDE, tie_columns, wide_codes

pytestmark = pytest.mark.gpu

SEED = 20261021
PANELS = [64, 128, 256, 512]
N_A = 257


# ------------------------------------------------------------------------------------------------------------------------
# a. band blocks and certificate
# ------------------------------------------------------------------------------------------------------------------------
def geno_a(kind, n, m):
    """012: codes 0/1/2, allele frequencies from 0.01 to 0.99, with a monomorphic column, an all-2 column and columns of sums 128 and 384 (exact
    ties of s / 256; a sum of 640 needs more than 257 individuals: tie_columns() has it at n = 512). signed: the same minus 1 (ga, gB near zero
    or negative). ld: columns in LD blocks (gcmax large against the rank-one part)."""
    rng = np.random.default_rng(4000 + m)
    if kind == "ld":
        return geno_ld(rng, n, m)
    X = rng.binomial(2, np.linspace(0.01, 0.99, m), size=(n, m)).astype(np.int8)
    X[:, 5], X[:, 6] = 1, 2
    for j, s in ((m // 4 + 3, 128), (m // 2 + 1, 384)):
        col = np.zeros(n, dtype=np.int8)
        col[:s // 2] = 2
        X[:, j] = rng.permutation(col)
    assert X[:, m // 4 + 3].sum(dtype=np.int64) == 128 and X[:, m // 2 + 1].sum(dtype=np.int64) == 384
    return np.asfortranarray(X - 1 if kind == "signed" else X, dtype=np.int8)


def assert_band_and_cert(c, X, P, n):
    """every stored block of the band is X_{p-l}' X_p, and the certificate's arrays are the reference's over the band read back"""
    L = c.pipeline()[3]
    cert = c.cert()
    assert cert["ok"] and cert["Lg"] == L
    Xp = R.padded(X, P)
    npan = Xp.shape[1] // P
    for p in range(npan):
        for l in range(min(L, p) + 1):
            want = R.cross(Xp[:, (p - l) * P:(p - l + 1) * P], Xp[:, p * P:(p + 1) * P])
            assert np.array_equal(c.gram_band(p, l), want), (p, l)
    ga, gB, gcmax = R.cert_reference(X, P, L, n)
    assert np.array_equal(cert["ga"], ga), np.flatnonzero(cert["ga"] != ga)[:8]
    assert np.array_equal(cert["gB"], gB), np.flatnonzero(cert["gB"] != gB)[:8]
    assert np.array_equal(cert["gcmax"], gcmax), np.flatnonzero(cert["gcmax"] != gcmax)[:8]
    assert int(gcmax.max()) < R.INT32_MAX                       # the clamp is not reached
    m = X.shape[1]
    assert not cert["gcmax"][m:].any() and not cert["gB"][m:].any()
    return L, cert


@pytest.mark.parametrize("kind", ["012", "signed", "ld"])
@pytest.mark.parametrize("panel", PANELS)
def test_band_blocks_and_certificate_are_exact(panel, kind):
    n, m = N_A, 4 * panel + 17
    X = geno_a(kind, n, m)
    col = np.zeros(n, dtype=np.int8)
    col[:128] = 2                                               # (sum 256, or -1 in the signed coding: no rounding in ga to drown the pair in)
    X[:, 20] = np.random.default_rng(panel).permutation(col) - (1 if kind == "signed" else 0)
    with H.Context(n, m, panel=panel) as c:
        c.upload(X)
        c.set_pipeline(1, 1, 2)
        L = c.pipeline()[3]
        assert 1 <= L <= 3 and c.panel == panel
        far = L * panel + 30                                    # a copy of marker 20 in the last block of the band as read back
        X[:, far] = X[:, 20]
        c.upload(X[:, far:far + 1], col0=far)
        c.build_gram()
        assert assert_band_and_cert(c, X, panel, n)[0] == L
        cert = c.cert()
    # marker 20's copy lies in the band's last block, and its maximum there alone: every block of the band is needed for these arrays
    assert R.cert_reference(X, panel, L - 1, n)[2][20] < R.cert_reference(X, panel, L, n)[2][20] == cert["gcmax"][20]
    if kind == "signed":
        assert (cert["ga"] <= 0).any() and (cert["gB"] < 0).any()


def test_certificate_rounds_ties_to_even():
    n, panel = 512, 64
    X, sums = tie_columns(n, 64 * 3 + 17)
    assert (sums % 2 == 1).sum() >= 32 and sums[40:43].tolist() == [128, 384, 640]
    with H.Context(n, X.shape[1], panel=panel) as c:
        c.upload(X)
        c.set_pipeline(1, 1, 2)
        c.build_gram()
        _, cert = assert_band_and_cert(c, X, panel, n)
    assert cert["ga"][40:43].tolist() == [0, 2, 2]


def test_certificate_at_the_edge_of_int32():
    X = wide_codes()
    with H.Context(N_WIDE, 64, panel=64) as c:
        c.upload(X)
        c.set_pipeline(1, 1, 2)
        c.build_gram()
        _, cert = assert_band_and_cert(c, X, 64, N_WIDE)
    assert int(cert["gcmax"].max()) == 2147463447
    assert int(np.abs(cert["ga"].astype(np.int64)[:, None] * cert["gB"].astype(np.int64)[None, :]).max()) == 2147450112


# ------------------------------------------------------------------------------------------------------------------------
# b. the certificate as state
# ------------------------------------------------------------------------------------------------------------------------
def test_certificate_follows_a_second_upload():
    n, panel, m = N_A, 64, 3 * 64 + 17
    X = geno_a("012", n, m)
    X2 = X.copy()
    X2[:, 60:130] = geno_a("ld", n, 70)                         # columns of two panels, in LD now
    with H.Context(n, m, panel=panel) as c:
        c.upload(X)
        c.set_pipeline(1, 1, 2)
        c.build_gram()
        _, first = assert_band_and_cert(c, X, panel, n)
        c.upload(X2[:, 60:130], col0=60)
        assert not c.cert()["ok"]                               # (until the band is built again)
        c.build_gram()
        _, second = assert_band_and_cert(c, X2, panel, n)
    assert not np.array_equal(first["gcmax"], second["gcmax"]) and not np.array_equal(first["gB"], second["gB"])


def test_certificate_covers_a_widened_band():
    """A stale, narrower bound is the unsound direction: marker 10's copy lies three panels on, in a block only the wider band stores."""
    n, panel, m = N_A, 64, 5 * 64 + 17
    X = geno_a("012", n, m)
    col = np.zeros(n, dtype=np.int8)
    col[:128] = 2                                               # sum 256: ga = 1 without rounding, so c is the covariance part alone
    X[:, 10] = np.random.default_rng(10).permutation(col)
    X[:, 3 * 64 + 20] = X[:, 10]
    with H.Context(n, m, panel=panel) as c:
        c.upload(X)
        c.set_pipeline(1, 1, 1)
        c.build_gram()
        L1, narrow = assert_band_and_cert(c, X, panel, n)
        c.set_pipeline(1, 2, 2)
        assert not c.cert()["ok"]
        c.build_gram()
        L2, wide = assert_band_and_cert(c, X, panel, n)
    assert L1 < 3 <= L2
    ref1, ref2 = R.cert_reference(X, panel, L1, n)[2], R.cert_reference(X, panel, L2, n)[2]
    assert ref2[10] > ref1[10] and (ref2 >= ref1).all()         # on the reference: the maximum lies in a block of the wider band alone
    assert wide["gcmax"][10] == ref2[10] > narrow["gcmax"][10]


def test_certificate_from_the_two_bit_layout_alone():
    n, panel, m = N_A, 64, 6 * 64 + 17
    X = geno_a("ld", n, m)
    with H.Context(n, m, panel=panel, precise=2) as c:
        c.upload(X)
        c.set_pipeline(1, 1, 2)
        c.build_gram()
        _, a = assert_band_and_cert(c, X, panel, n)
        c.set_layout(2, keep_int8=False)
        assert c.layout() == (2, False)
        c.build_gram()                                          # the windowed unpack path
        _, b = assert_band_and_cert(c, X, panel, n)
    for k in ("ga", "gB", "gcmax"):
        assert np.array_equal(a[k], b[k])


def test_where_there_is_no_certificate(monkeypatch):
    n, panel, m = N_A, 64, 2 * 64 + 17
    X = geno_a("012", n, m)
    with H.Context(n, m, panel=panel) as c:
        c.upload(X)
        got = c.cert()                                          # before any build
        assert not got["ok"] and got["ga"] is None
    with H.Context(n, m, panel=panel) as c:                     # the fp64 layout
        c.upload_real(X.astype(np.float64))
        c.build_gram()
        assert not c.cert()["ok"]
    monkeypatch.setenv("HB_CERT", "0")
    with H.Context(n, m, panel=panel) as c:
        c.upload(X)
        c.set_pipeline(1, 1, 2)
        c.build_gram()
        assert not c.cert()["ok"]
        assert np.array_equal(c.gram_band(1, 1), R.cross(X[:, :64].astype(np.int64), X[:, 64:128].astype(np.int64)))


# ------------------------------------------------------------------------------------------------------------------------
# c. opening filter, records and lists
# ------------------------------------------------------------------------------------------------------------------------
N_C = 200
SWEEPS = {
    "BayesCpi": (dict(varg=0.01, logpi=[math.log(0.95), math.log(0.05)]), (1, 1, 2)),                       # the group chain
    "BayesR": (dict(varg=0.5, logpi=[math.log(v) for v in (0.95, 0.02, 0.02, 0.01)], fold=[0.0, 1e-4, 1e-3, 1e-2],
                    vara_fold=[0.0, 0.5e-4, 0.5e-3, 0.5e-2]), (1, 2, 1)),                                   # the per-panel chain: the lists' reader
}


def geno_c(P):
    """six panels less three markers; the first half of panel 4 monomorphic"""
    rng = np.random.default_rng(6000 + P)
    m = 6 * P - 3
    X = rng.binomial(2, rng.uniform(0.05, 0.5, m), size=(N_C, m)).astype(np.int8)
    X[:, 4 * P:4 * P + P // 2] = 1
    X[:, 9] = 2
    y = X[:, ::37].astype(np.float64) @ rng.normal(0, 0.3, X[:, ::37].shape[1]) + rng.normal(0, 1.0, N_C)
    return np.asfortranarray(X), y - y.mean()


def pattern_sets(P, nslot):
    pat = R.hot_patterns(P, nslot)
    big = pat["beyond-the-list"] if "beyond-the-list" in pat else pat["second-half-all"]
    return [[pat[k] for k in ("none", "at-0", "at-half-1", "at-half", "at-last", "second-half-few")],
            [pat["nslot"], pat["nslot+1"], pat["all"], big, pat["second-half-all"], pat["all"]]]


def sweep_and_check(c, X, y, model, g0, it, want_predicted=False):
    """install g0, run one sweep, and hold everything k_hotlist wrote against the restatement of the read-outs"""
    kw = SWEEPS[model][0]
    P, m = c.panel, X.shape[1]
    m_pad = -(-m // P) * P
    pad = lambda a: np.concatenate([a, np.zeros(m_pad - m)])          # noqa: E731
    xpx, vx, _, _ = c.marker_stats()
    c.set_residual(y - X.astype(np.float64) @ g0, np.zeros(X.shape[0]))
    c.set_effects(g0, np.ones(m, dtype=np.uint8), None)
    c.sweep(model, it, 1.0, **kw)
    op, thr0, cert = c.opening(), c.pre()[0][0], c.cert()
    g1, t1, _ = c.get_effects()
    assert cert["ok"] and op["opn"] is not None
    xpx, vx, g = pad(xpx), pad(vx), pad(g0)
    # the filter and the records, bit for bit
    f, opn = R.filter_reference(thr0, vx, g, op["candf"], cert["gB"])
    assert np.array_equal(op["thr0f"].view(np.int32), f.view(np.int32)), np.flatnonzero(op["thr0f"].view(np.int32) != f.view(np.int32))[:8]
    assert np.array_equal(op["opn"], opn), np.flatnonzero((op["opn"] != opn).any(axis=1))[:8]
    assert np.array_equal(op["opn"][:, 3], cert["gB"])
    plain = (vx != 0) & (g == 0)
    fd = op["thr0f"][plain].astype(np.float64)
    assert (fd <= thr0[plain]).all() and (fd < thr0[plain]).any()      # a superset test, and one that had to step down somewhere
    # the class of a marker that was and stays at zero
    still = (g0 == 0) & (g1 == 0)
    assert still.any() and not t1[still].any()
    # the lists
    nslot = op["nslot"]
    assert R.fits_the_list(P, nslot) and 1 <= nslot <= min(P, 250)
    active, hot = R.hot_flags(vx, g, thr0, xpx, op["kappa"], 1.0)
    if want_predicted:
        assert (hot & (g == 0)).any() and (active & ~hot).any()
    else:
        assert np.array_equal(hot, active & (g != 0))
    slot_of, lists, head = R.hotlist_reference(active, hot, P, nslot)
    dlists, dhead = R.lists_from_pack(op["hotpack"])
    assert np.array_equal(op["slot_of"], slot_of), np.flatnonzero(op["slot_of"] != slot_of)[:8]
    assert np.array_equal(dhead, head), (dhead.tolist(), head.tolist())
    for p in range(len(lists)):
        assert np.array_equal(dlists[p], lists[p]), p
    assert R.check_lists(op["slot_of"], dlists, dhead, active, hot, P, nslot) == []
    return op, thr0, plain


@pytest.mark.parametrize("model", list(SWEEPS))
@pytest.mark.parametrize("panel", PANELS)
def test_opening_filter_records_and_lists(panel, model, monkeypatch):
    """One panel per hot pattern (tests/opening_restatement.py: hot_patterns), the prediction switched off: HB_KAPPA is read when the context is
    created, and a hugely negative value leaves g != 0 as the only way onto a list."""
    monkeypatch.setenv("HB_KAPPA", "-1e30")
    X, y = geno_c(panel)
    m = X.shape[1]
    with H.Context(N_C, m, panel=panel, precise=2, seed=SEED) as c:
        c.upload(X)
        c.set_pipeline(*SWEEPS[model][1])
        c.build_gram()
        with pytest.raises(H.HibayesError, match="no pipelined sweep"):
            c.opening()
        assert c.pipeline()[0] == 1
        op, thr0, plain = sweep_and_check(c, X, y, model, np.zeros(m), 0)            # (and the nslot the patterns are cut to)
        assert op["kappa"] == -1e30
        negative = (thr0[plain] < 0).any()
        _, vx, _, _ = c.marker_stats()
        rng = np.random.default_rng(panel)
        for it, pats in enumerate(pattern_sets(panel, op["nslot"]), start=1):
            hot = np.concatenate(pats)[:m] & (vx != 0)
            g0 = np.where(hot, rng.choice([-1.0, 1.0], m) * rng.uniform(0.005, 0.05, m), 0.0)
            op, thr0, plain = sweep_and_check(c, X, y, model, g0, it)
            negative = negative or (thr0[plain] < 0).any()
            if panel == 512 and it == 1:                                             # the shifted layout was reached
                assert op["hotpack"][3, :4].tolist() == [1, 1, 0, 1] and op["slot_of"][3 * panel + panel // 2] == 0
        if model == "BayesCpi":
            assert negative                                                          # thresholds below zero went through the filter


def test_opening_lists_with_the_prediction_on():
    """the default kappa: markers at zero whose threshold lies below kappa xpx vare are listed beside those in the model"""
    panel = 128
    X, y = geno_c(panel)
    m = X.shape[1]
    rng = np.random.default_rng(3)
    g0 = np.where(rng.random(m) < 0.03, rng.normal(0, 0.05, m), 0.0)
    with H.Context(N_C, m, panel=panel, precise=2, seed=SEED) as c:
        c.upload(X)
        c.set_pipeline(*SWEEPS["BayesCpi"][1])
        c.build_gram()
        op, _, _ = sweep_and_check(c, X, y, "BayesCpi", g0, 0, want_predicted=True)
        assert op["kappa"] > 0
