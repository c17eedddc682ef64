"""The single-step model as far as a machine without a GPU can see it: the schedule of the Gibbs pass (hb_epslplan.hpp through hb_epsl_plan),
the restatement evaluated by that schedule against the row-by-row pass, make_ped / make_Ainv, ssbrm()'s preparation on the reference's demo,
the validation of the block's arguments, the exports and the compiler's resource report of the new kernels."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import hibayes_amd as H
from hibayes_amd import _lib
from hibayes_amd.ssbayes import epsl_check, epsl_plan
import epsl_restatement as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "tests", "golden", "demo", "demo")
NEW = ["hb_ctx_epsl_setup", "hb_ctx_epsl_step", "hb_ctx_epsl_state", "hb_ctx_epsl_debug_get", "hb_ctx_epsl_debug_set", "hb_epsl_check", "hb_epsl_plan",
       "hb_bayes_run_epsl", "hb_run_epsl", "hb_run_epsl_store"]


# ---- patterns ----
def diagonal(q=50):
    return sp.identity(q, format="csc") * 2.0


def tridiagonal(q=257):
    G = sp.csc_matrix(sp.diags([np.full(q - 1, -1.0), np.full(q, 2.5), np.full(q - 1, -1.0)], [-1, 0, 1]))
    G.sort_indices()
    return G


def hub(nb=5000, first=True):
    """one individual with nb neighbours (a sire and its offspring), placed first or last"""
    q = nb + 1
    h = 0 if first else nb
    others = np.array([i for i in range(q) if i != h])
    r = np.concatenate([np.arange(q), np.full(nb, h), others])
    c = np.concatenate([np.arange(q), others, np.full(nb, h)])
    diag = np.full(q, 2.0)
    diag[h] = 1.0 + 0.5 * nb
    G = sp.coo_matrix((np.concatenate([diag, np.full(2 * nb, -1.0)]), (r, c)), shape=(q, q)).tocsc()
    G.sort_indices()
    return G


def read_ped():
    rows = [l.split() for l in open(DEMO + ".ped")][1:]
    return np.array(rows, dtype=object)


@pytest.fixture(scope="module")
def demo_ped():
    ped = read_ped()
    ids, s, d = H.make_ped(ped[:, 0], ped[:, 1], ped[:, 2])
    Ai = H.make_Ainv(s, d)
    fam = [l.split()[1] for l in open(DEMO + ".fam")]
    pos = {v: i for i, v in enumerate(ids)}
    g = np.zeros(len(ids), dtype=bool)
    g[[pos[v] for v in fam]] = True
    Ann = Ai.tocsr()[~g][:, ~g].tocsc()
    Ann.sort_indices()
    return {"ped": ped, "ids": ids, "s": s, "d": d, "Ai": Ai, "fam": fam, "Ann": Ann}


def patterns(demo_ped):
    return {"diagonal": diagonal(), "tridiagonal": tridiagonal(), "hub_first": hub(first=True), "hub_last": hub(first=False), "demo": demo_ped["Ann"]}


def check_plan(G, pl):
    G = sp.csc_matrix(G)
    q = G.shape[0]
    level = pl["level"]
    for i in range(q):
        js = G.indices[G.indptr[i]:G.indptr[i + 1]]
        js = js[js < i]
        assert np.all(level[js] < level[i]), i
    seen = np.zeros(q, dtype=np.int64)
    last_level = -1
    for kind, s0, s1 in pl["launches"]:
        assert kind in (0, 1) and s1 > s0 and (kind == 0 or s1 == s0 + 1)
        for s in range(s0, s1):
            lv, lane0, nlane, wave0, nwave = pl["steps"][s]
            assert lv >= last_level
            last_level = lv
            rows = np.concatenate([pl["rows"][lane0:lane0 + nlane], pl["rows"][wave0:wave0 + nwave]])
            seen[rows] += 1
            assert np.all(level[rows] == lv)
            inset = np.zeros(q, dtype=bool)
            inset[rows] = True
            for i in rows:  # the rows of one barrier-free step share no stored entry
                js = G.indices[G.indptr[i]:G.indptr[i + 1]]
                assert not np.any(inset[js[js != i]]), (s, i)
    assert np.all(seen == 1)
    s_prev = 0
    for kind, s0, s1 in pl["launches"]:  # the launches cover the steps in order
        assert s0 == s_prev
        s_prev = s1
    assert s_prev == len(pl["steps"])


@pytest.mark.parametrize("name", ["diagonal", "tridiagonal", "hub_first", "hub_last", "demo"])
@pytest.mark.parametrize("modes", [(0, 0), (1, 1), (2, 2), (1, 2), (2, 1)])
def test_plan_orders_every_dependency(demo_ped, name, modes):
    G = patterns(demo_ped)[name]
    pl = epsl_plan(G, *modes)
    check_plan(G, pl)
    lev, _ = E.levels_of(G.indptr, G.indices)
    assert np.array_equal(lev, pl["level"])


def test_plan_shapes(demo_ped):
    P = patterns(demo_ped)
    pl = epsl_plan(P["diagonal"])
    assert pl["levels"] == 1 and len(pl["launches"]) == 1
    pl = epsl_plan(P["tridiagonal"])
    assert pl["levels"] == 257 and [tuple(l) for l in pl["launches"]] == [(0, 0, 257)]  # all in ONE single-workgroup launch
    pl = epsl_plan(P["hub_first"])
    assert pl["levels"] == 2 and pl["max_col"] == 5001
    assert pl["steps"][0][2] + pl["steps"][0][4] == 1 and pl["steps"][0][4] == 1      # the hub alone, on a wave
    assert [int(k) for k, _, _ in pl["launches"]] == [0, 1]                            # then its 5000 neighbours over the chip
    pl = epsl_plan(P["hub_last"])
    assert pl["levels"] == 2 and [int(k) for k, _, _ in pl["launches"]] == [1, 0]
    pl = epsl_plan(P["demo"])  # the figures of the issue: 17 levels of 2 to 150 rows, 4500 stored entries, at most 18 per column
    cnt = np.bincount(pl["level"])
    assert P["demo"].shape == (900, 900) and P["demo"].nnz == 4500
    assert pl["levels"] == 17 and cnt.min() == 2 and cnt.max() == 150 and pl["max_col"] == 18 and len(pl["launches"]) == 1
    # the forced modes
    assert all(k == 0 for k, _, _ in epsl_plan(P["hub_first"], 1, 0)["launches"]) and all(k == 1 for k, _, _ in epsl_plan(P["demo"], 2, 0)["launches"])
    assert sum(s[4] for s in epsl_plan(P["demo"], 0, 1)["steps"]) == 0 and sum(s[2] for s in epsl_plan(P["demo"], 0, 2)["steps"]) == 0


def _block_inputs(G, seed, zz_max=2):
    rng = np.random.default_rng(seed)
    q = G.shape[0]
    reps = rng.integers(0, zz_max + 1, q)
    reps[rng.integers(0, q)] = max(1, zz_max)
    index0 = rng.permutation(np.repeat(np.arange(q), reps))
    ne = index0.size
    n = ne + 37
    return dict(index0=index0, yJ=rng.normal(size=n), yadj=rng.normal(size=n), u=rng.normal(size=n), x=rng.normal(size=q) * 0.3, J=0.2, vare=1.3, veps=0.7,
                z=rng.normal(size=q), zJ=0.4, chis=float(q), s2_df=0.5)


@pytest.mark.parametrize("name", ["tridiagonal", "hub_first", "hub_last", "demo"])
def test_the_schedule_is_the_sequential_pass_bit_for_bit(demo_ped, name):
    G = sp.csc_matrix(patterns(demo_ped)[name])
    kw = _block_inputs(G, 11)
    a = E.epsl_block(G.indptr, G.indices, G.data, **kw)
    pl = epsl_plan(G)
    sched = [np.concatenate([pl["rows"][s[1]:s[1] + s[2]], pl["rows"][s[3]:s[3] + s[4]]]) for s in pl["steps"]]
    b = E.epsl_block(G.indptr, G.indices, G.data, schedule=sched, **kw)
    for k in ("x", "yadj", "u", "q", "veps", "J"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert not np.array_equal(a["x"], kw["x"])


# ---- make_Ainv, make_ped ----
def test_make_Ainv_inverts_the_tabular_A_and_both_one_parent_rules():
    s = [0, 0, 0, 0, 1, 3, 5, 5, 0]
    d = [0, 0, 0, 0, 2, 4, 6, 6, 0]
    A = E.tabular_A(s, d)
    Ai = H.make_Ainv(s, d).toarray()
    assert np.max(np.abs(Ai @ A - np.eye(len(s)))) < 1e-12
    assert np.array_equal(Ai, E.ainv_dense(s, d))
    # one known parent: the reference's integer divisions add 1 to the diagonal and nothing else; Henderson's rule 4/3, -2/3, 1/3
    s1, d1 = [0, 1, 0], [0, 0, 1]
    ref = H.make_Ainv(s1, d1).toarray()
    assert np.array_equal(ref, np.eye(3))
    hen = H.make_Ainv(s1, d1, one_parent="henderson").toarray()
    assert np.allclose(hen, [[1 + 2 / 3, -2 / 3, -2 / 3], [-2 / 3, 4 / 3, 0], [-2 / 3, 0, 4 / 3]], rtol=0, atol=1e-15)
    assert np.max(np.abs(hen @ E.tabular_A(s1, d1) - np.eye(3))) < 1e-12
    for mode in ("reference", "henderson"):
        assert np.allclose(H.make_Ainv(s1, d1, one_parent=mode).toarray(), E.ainv_dense(s1, d1, mode), rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match="one_parent"):
        H.make_Ainv(s1, d1, one_parent="x")


def test_make_Ainv_on_the_demo_pedigree_is_the_references_loop(demo_ped):
    for mode in ("reference", "henderson"):
        Ai = H.make_Ainv(demo_ped["s"], demo_ped["d"], one_parent=mode)
        assert np.allclose(Ai.toarray(), E.ainv_dense(demo_ped["s"], demo_ped["d"], mode), rtol=0, atol=1e-12)
        assert Ai.has_sorted_indices and (Ai != Ai.T).nnz == 0


def _parents_first(ids, s, d):
    for i, (a, b) in enumerate(zip(s, d)):
        assert a <= i and b <= i, (ids[i], a, b)


def test_make_ped_orders_adds_founders_and_reads_the_na_tokens(demo_ped):
    ids, s, d = H.make_ped(["c", "b", "a", "k"], ["a", "0", "0", "c"], ["b", "0", "0", "b"])  # a shuffled file
    assert ids == ["b", "a", "c", "k"] and s == [0, 0, 2, 3] and d == [0, 0, 1, 1]
    ids, s, d = H.make_ped(["x", "y"], ["p", "p"], ["m", "x"])  # parents missing from column 1 become founders where first met
    assert ids == ["p", "m", "x", "y"] and s == [0, 0, 1, 1] and d == [0, 0, 2, 3]
    ids, s, d = H.make_ped(["a", "NA", "b", "c"], ["NA", "a", ".", "a"], ["<NA>", "a", "n/a", "b"])  # NA ids leave, NA parents are unknown
    assert ids == ["a", "b", "c"] and s == [0, 0, 1] and d == [0, 0, 2]
    with pytest.raises(ValueError, match="repeated records are not allowed in the first column of pedigree file."):
        H.make_ped(["a", "a"], ["0", "0"], ["0", "0"])
    with pytest.raises(ValueError, match="no individuals detected;"):
        H.make_ped(["NA"], ["0"], ["0"])
    # the demo, shuffled: every individual once, parents first
    ped = demo_ped["ped"]
    perm = np.random.default_rng(5).permutation(len(ped))
    ids, s, d = H.make_ped(ped[perm, 0], ped[perm, 1], ped[perm, 2])
    assert sorted(ids) == sorted(ped[:, 0]) and len(ids) == 1500
    _parents_first(ids, s, d)
    par = {r[0]: (r[1], r[2]) for r in ped}
    for i in range(0, 1500, 7):
        assert (ids[s[i] - 1] if s[i] else "0", ids[d[i] - 1] if d[i] else "0") == par[ids[i]]


# ---- the preparation on the demo ----
@pytest.fixture(scope="module")
def demo_prep(demo_ped):
    pl = H.read_plink(DEMO)
    phe = H.read_table(DEMO + ".phe")
    M_id = [r[1] for r in pl["fam"]]
    pr = H.ssbrm_prepare("T1 ~ 1", phe, pl["geno"], M_id, demo_ped["ped"])
    return {"pr": pr, "phe": phe, "M_id": M_id, "geno": pl["geno"]}


def test_preparation_on_the_demo(demo_ped, demo_prep):
    pr, phe, M_id = demo_prep["pr"], demo_prep["phe"], demo_prep["M_id"]
    # the counts, from the files themselves
    ped_ids = set(demo_ped["ped"][:, 0])
    assert len(M_id) == 600 and len(pr["Mn_id"]) == len(ped_ids - set(M_id)) == 900
    rec = [v for v, t in zip(phe["id"], phe["T1"]) if t is not None]
    g_rec = [v for v in rec if v in set(M_id)]
    assert pr["n_genotyped_records"] == len(g_rec) and pr["n_other_records"] == len(rec) - len(g_rec) > 0
    assert pr["y_id_comb"][:len(g_rec)] == [v for v in M_id if v in set(rec)]            # genotyped records first, in M's order
    assert all(v not in set(M_id) for v in pr["y_id_comb"][len(g_rec):])
    assert [pr["Mn_id"][i - 1] for i in pr["index"]] == pr["y_id_comb"][len(g_rec):]
    t1 = {v: float(t) for v, t in zip(phe["id"], phe["T1"]) if t is not None}
    assert np.array_equal(pr["y"], [t1[v] for v in pr["y_id_comb"]])
    assert pr["y_M"].shape == (len(rec), 1000) and np.array_equal(pr["y_J"][:len(g_rec)], np.full(len(g_rec), -1.0))
    # A^-1_nn Mn + A^-1_ng M vanishes to 1e-10 of its terms (and the same for J)
    res = pr["Ai_nn"] @ pr["Mn"] + pr["Ai_ng"] @ pr["M"]
    terms = abs(pr["Ai_nn"]) @ np.abs(pr["Mn"]) + abs(pr["Ai_ng"]) @ np.abs(pr["M"])
    assert np.all(np.abs(res) <= 1e-10 * terms)                         # entry by entry
    resJ = pr["Ai_nn"] @ pr["Jn"] + pr["Ai_ng"] @ pr["J"]
    termsJ = abs(pr["Ai_nn"]) @ np.abs(pr["Jn"]) + abs(pr["Ai_ng"]) @ np.abs(pr["J"])
    assert np.all(np.abs(resJ) <= 1e-10 * termsJ) and np.max(termsJ) > 1
    # MAF: a marker below 0.01 is zeroed
    p = demo_prep["geno"].astype(np.float64).mean(axis=0) / 2
    low = np.minimum(p, 1 - p) < 0.01
    assert np.all(pr["M"][:, low] == 0) and np.array_equal(pr["M"][:, ~low], demo_prep["geno"][:, ~low].astype(np.float64))
    # the dense restatement
    pos = {v: i for i, v in enumerate(demo_ped["ids"])}
    g_indx = np.array([pos[v] for v in M_id])
    n_indx, Ann, Ang, Mn, Jn = E.impute_dense(E.ainv_dense(demo_ped["s"], demo_ped["d"]), g_indx, pr["M"][:, :40])
    assert [demo_ped["ids"][i] for i in n_indx] == pr["Mn_id"]
    assert np.allclose(pr["Mn"][:, :40], Mn, rtol=0, atol=1e-10) and np.allclose(pr["Jn"], Jn, rtol=0, atol=1e-10)
    assert np.array_equal(pr["Ai_nn"].toarray(), Ann)


def test_preparation_raises_the_references_texts(demo_ped, demo_prep):
    phe, M_id, geno, ped = demo_prep["phe"], demo_prep["M_id"], demo_prep["geno"], demo_ped["ped"]
    small = geno[:, :8]
    cases = [
        (dict(data=None), "no data assigned."),
        (dict(data={"id": phe["id"]}), "the first column in 'data' should be the individual id."),
        (dict(M=None), "no genotype data."),
        (dict(M_id=None), "please assign the individuals id to 'M.id'."),
        (dict(M_id=M_id[:-1]), "number of individuals mismatched in 'M' and 'M.id'."),
        (dict(pedigree=None), "pedigree should be provided for single-step bayesian model."),
        (dict(pedigree=ped[:, :2]), r"3 columns \('id', 'sir', 'dam'\) are required in pedigree."),
        (dict(M_id=["Z%d" % i for i in range(600)]), "no shared individuals between 'M.id' and 'pedigree'."),
        (dict(pedigree=np.array([[v, v, v] for v in M_id], dtype=object)), "all individuals have been genotyped, no necessaries to fit single-step bayes model."),
        (dict(data={"id": ["Q%d" % i for i in range(len(phe["id"]))], "T1": phe["T1"]}), "no shared individuals between 'data' and 'pedigree'."),
        (dict(data={"id": phe["id"], "T1": [None] * len(phe["id"])}), "no effective data left."),
    ]
    for over, text in cases:
        kw = dict(formula="T1 ~ 1", data=phe, M=small, M_id=M_id, pedigree=ped)
        kw.update(over)
        with pytest.raises(ValueError, match=text):
            H.ssbrm_prepare(**kw)
    with pytest.raises(ValueError, match="'arg' should be one of"):
        H.ssbrm("T1 ~ 1", phe, small, M_id, ped, method="BSLMM")
    with pytest.raises(ValueError, match="bad setting for collecting frequency 'thin'."):
        H.ssbrm("T1 ~ 1", phe, small, M_id, ped, niter=10, nburn=8, thin=5)


# ---- validation ----
def test_each_invalid_descriptor_gets_its_error():
    G = tridiagonal(6)
    ip, ix, dt = G.indptr.copy(), G.indices.copy(), G.data.copy()
    epsl_check(G, [1, 6, 6], 10)

    def bad(triple, index, n, text):
        with pytest.raises(H.HibayesError, match=text) as e:
            epsl_check(triple, index, n)
        assert e.value.status == 1

    bad((ip, ix, dt), [0], 10, "epsl_index: an index is outside 1 .. q")
    bad((ip, ix, dt), [7], 10, "epsl_index: an index is outside 1 .. q")
    bad((ip, ix, dt), [1] * 11, 10, "epsl_index: between 1 and n records")
    bad((ip, ix, dt), [], 10, "epsl_index: between 1 and n records")
    i2 = ix.copy()
    i2[0], i2[1] = ix[1], ix[0]
    bad((ip, i2, dt), [1], 10, "sorted and unique")
    i2 = ix.copy()
    i2[-1] = 6
    bad((ip, i2, dt), [1], 10, "a row index is outside 0 .. q - 1")
    U = sp.triu(G).tocsc()
    bad((U.indptr, U.indices, U.data), [1], 10, "must be symmetric")
    d2 = dt.copy()
    d2[1] = -0.5  # (1, 0) without changing (0, 1)
    bad((ip, ix, d2), [1], 10, "must be symmetric")
    d2 = dt.copy()
    d2[0] = 0.0
    bad((ip, ix, d2), [1], 10, "the diagonal must be positive")
    Z = sp.csc_matrix(np.array([[1.0, 0.0], [0.0, 0.0]]))
    bad((Z.indptr, Z.indices, Z.data), [1], 10, "the diagonal must be positive")
    d2 = dt.copy()
    d2[2] = np.nan
    bad((ip, ix, d2), [1], 10, "not finite")
    d2[2] = np.inf
    bad((ip, ix, d2), [1], 10, "not finite")
    with pytest.raises(H.HibayesError, match="variance-covariance matrix should be in square."):
        epsl_check(sp.csc_matrix(np.ones((2, 3))), [1], 10)
    with pytest.raises(H.HibayesError, match="variance-covariance matrix should be provided for epsilon term."):
        H.Bayes(np.zeros(4), np.zeros((4, 2), dtype=np.int8), "BayesCpi", [0.95, 0.05], epsl_y_J=np.ones(4), epsl_index=[1])
    with pytest.raises(H.HibayesError, match="go together"):
        H.Bayes(np.zeros(4), np.zeros((4, 2), dtype=np.int8), "BayesCpi", [0.95, 0.05], epsl_Gi=G)


# ---- the library ----
def test_the_librarys_own_texts_for_an_incomplete_triple():
    """hb_bayes_run() itself (what a C caller or the shim reaches; Bayes() answers earlier): validation comes before any device call"""
    import ctypes as C
    L = H.lib()
    G = tridiagonal(6)
    ip, ix, dt = G.indptr.astype(np.int64), G.indices.astype(np.int32), G.data
    y, X, Pi = np.arange(8.0), np.zeros((8, 2), dtype=np.int8, order="F"), np.array([0.95, 0.05])
    idx, yj = np.array([1, 6], dtype=np.uint32), np.ones(8)
    gi = _lib.EpslGi(6, 2, ip.ctypes.data, ix.ctypes.data, dt.ctypes.data)

    def run(model=b"BayesCpi", **f):
        a = _lib.BayesArgs()
        a.n, a.m, a.y, a.X_i8, a.ld_i8, a.model, a.Pi, a.n_pi = 8, 2, y.ctypes.data, X.ctypes.data, 8, model, Pi.ctypes.data, 2
        a.niter, a.nburn, a.thin = 4, 2, 1
        for k, v in f.items():
            setattr(a, k, v)
        rc = L.hb_bayes_run(C.byref(a), C.byref(_lib.BayesOut()))
        return rc, L.hb_last_error().decode()

    full = dict(epsl_y_J=yj.ctypes.data, epsl_Gi=C.addressof(gi), epsl_index=idx.ctypes.data)
    for drop, text in (("epsl_Gi", "variance-covariance matrix should be provided for epsilon term."),
                       ("epsl_y_J", "epsl_y_J, epsl_Gi and epsl_index go together"), ("epsl_index", "epsl_y_J, epsl_Gi and epsl_index go together")):
        rc, msg = run(**{k: v for k, v in full.items() if k != drop})
        assert rc == 1 and text in msg, (drop, rc, msg)
    bad = np.array([1, 7], dtype=np.uint32)
    rc, msg = run(**dict(full, epsl_index=bad.ctypes.data))
    assert rc == 1 and "epsl_index: an index is outside 1 .. q" in msg
    rc, msg = run(model=b"BSLMM", **full)
    assert rc == 4 and "the epsilon block is not available with BSLMM" in msg
    rc, msg = run(shard_rows=1, n_global=8, precise=2, **full)
    assert rc == 4 and "the epsilon block is not available with shard_rows" in msg


def test_new_symbols_are_declared_exported_and_the_abi_is_still_6():
    lib = H.lib()
    hdr = open(os.path.join(ROOT, "include", "hibayes_gpu.h")).read()
    for s in NEW:
        assert s in _lib.SYMBOLS and hasattr(lib, s) and re.search(r"\b%s\s*\(" % s, hdr), s
    assert "typedef struct hb_epsl_gi" in hdr and "typedef struct hb_epsl_out" in hdr and "src/Bayes.cpp:554-584" in hdr
    assert lib.hb_abi_version() == 6
    assert "ssbrm" in H.__all__ and "make_ped" in H.__all__ and "make_Ainv" in H.__all__


def test_epsl_kernels_are_built_without_scratch():
    path = os.path.join(ROOT, "hibayes_amd", "csrc", "hb_epsl.res.txt")
    assert os.path.exists(path), "no resource report: the library was not built by the Makefile here"
    rows, cur = {}, None
    for line in open(path):
        mm = re.search(r"Function Name: (\S+)", line)
        if mm:
            cur = mm.group(1)
            rows[cur] = {}
            continue
        mm = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if mm and cur:
            rows[cur][mm.group(1).strip()] = int(mm.group(2))
    for name in ("k_epsl_narrow", "k_epsl_wide", "k_epsl_chunkdot", "k_epsl_jfin", "k_epsl_japply", "k_epsl_b", "k_epsl_scatter", "k_epsl_gx", "k_epsl_vfin",
                 "k_epsl_add"):
        found = [k for k in rows if name in k]
        assert found, "kernel missing from the report: " + name
        for k in found:
            assert "ScratchSize" in rows[k] and "VGPRs Spill" in rows[k], (k, rows[k])      # (the report's format is still the one read here)
            assert rows[k]["ScratchSize"] == 0 and rows[k]["VGPRs Spill"] == 0, (k, rows[k])
