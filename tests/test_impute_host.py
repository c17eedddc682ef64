"""ssbrm()'s device imputation as far as a machine without a GPU can see it: the numpy restatement of the batched conjugate-gradient solve
(tests/impute_restatement.py) against dense and sparse-factor algebra, its freeze, the planning header (hb_imputeplan.hpp, compiled here with
g++), the library's validation texts, the exports, the compiler's resource report of the new kernels and the Python surface."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import hibayes_amd as H
from hibayes_amd import _lib
from hibayes_amd.impute import ImputeSystem
import epsl_restatement as E
import impute_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "tests", "golden", "demo", "demo")
NEW = ["hb_impute_create", "hb_impute_solve", "hb_impute_destroy"]


@pytest.fixture(scope="module")
def ss_demo():
    """the demo's system: A_nn (900 x 900), A_ng (900 x 600), the first 130 MAF-filtered marker columns and J, and the dense solution"""
    ped = np.array([l.split() for l in open(DEMO + ".ped")][1:], dtype=object)
    pl = H.read_plink(DEMO)
    phe = H.read_table(DEMO + ".phe")
    M_id = [r[1] for r in pl["fam"]]
    pr = H.ssbrm_prepare("T1 ~ 1", phe, pl["geno"], M_id, ped)
    ids, s, d = H.make_ped(ped[:, 0], ped[:, 1], ped[:, 2])
    pos = {v: i for i, v in enumerate(ids)}
    g_indx = np.array([pos[v] for v in M_id])
    M = np.column_stack([pr["M"][:, :130], pr["J"]])
    _n, Ann, _Ang, Mn, Jn = E.impute_dense(E.ainv_dense(s, d), g_indx, M[:, :130])
    assert np.array_equal(pr["Ai_nn"].toarray(), Ann)
    return {"Ann": pr["Ai_nn"], "Ang": pr["Ai_ng"], "M": M, "dense": np.column_stack([Mn, Jn]), "lmin": float(np.linalg.eigvalsh(Ann)[0]), "pr": pr,
            "phe": phe, "geno": pl["geno"], "M_id": M_id, "ped": ped}


def test_restatement_against_dense_algebra_on_the_demo(ss_demo):
    tol = 1e-12
    out = R.pcg_batched(ss_demo["Ann"], ss_demo["Ang"], ss_demo["M"], tol, 2000)
    b = -(ss_demo["Ang"] @ ss_demo["M"])
    bn = np.linalg.norm(b, axis=0)
    assert ss_demo["lmin"] > 0
    err = np.linalg.norm(out["x"] - ss_demo["dense"], axis=0)
    res = np.linalg.norm(b - ss_demo["Ann"] @ out["x"], axis=0)
    print("demo: %d iterations, lambda_min %.4g, largest error / bound %.3g, largest residual / (tol ||b||) %.3g"
          % (out["iterations"], ss_demo["lmin"], np.max(err[bn > 0] / (2 * tol * bn[bn > 0] / ss_demo["lmin"])), np.max(res[bn > 0] / (tol * bn[bn > 0]))))
    assert np.all(err <= 2 * tol * bn / ss_demo["lmin"])
    assert np.all(res <= 1.5 * tol * bn)
    zero = np.flatnonzero(~ss_demo["M"].any(axis=0))
    assert zero.size >= 1                                   # the MAF filter's columns among the first 130
    assert np.all(out["x"][:, zero] == 0.0) and np.all(out["col_iterations"][zero] == 0)
    assert 1 <= out["iterations"] <= 2000 and out["col_iterations"][-1] >= 1


@pytest.fixture(scope="module")
def deep():
    """20 generations x family 40 of about 20 000 individuals, the first tenth of the youngest generation genotyped; 8 columns of 0/1/2"""
    size = 20000 // 21
    s, d = R.pedigree(20, 40, size, 1)
    N = s.size
    geno = np.arange(N - size, N - size + size // 10)
    Ann, Ang, _ = R.split(H.make_Ainv(s, d, one_parent="henderson"), geno)
    M = np.random.default_rng(2).integers(0, 3, size=(geno.size, 8)).astype(np.float64)
    return {"Ann": Ann, "Ang": Ang, "M": M}


def test_restatement_on_a_deep_generated_pedigree(deep):
    """tol = 1e-10: on this shape the true residual drifts from the recurrence's by about 9e-13 of ||b||, so 1e-12 is not asked of it"""
    from scipy.sparse.linalg import eigsh, splu
    tol = 1e-10
    Ann, Ang, M = deep["Ann"], deep["Ang"], deep["M"]
    assert 19000 < Ann.shape[0] < 20000
    out = R.pcg_batched(Ann, Ang, M, tol, 5000)
    lu = splu(Ann, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
    b = -(Ang @ M)
    star = lu.solve(b)
    lmin = float(eigsh(Ann, k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0])
    bn = np.linalg.norm(b, axis=0)
    res = np.linalg.norm(b - Ann @ out["x"], axis=0)
    err = np.linalg.norm(out["x"] - star, axis=0)
    print("deep pedigree q = %d, %d stored entries: %d iterations at tol %g; lambda_min %.4g; largest residual / (tol ||b||) %.3g; largest error / bound %.3g"
          % (Ann.shape[0], Ann.nnz, out["iterations"], tol, lmin, np.max(res / (tol * bn)), np.max(err / (2 * tol * bn / lmin))))
    assert lmin > 0
    assert np.all(res <= 1.5 * tol * bn)
    assert np.all(err <= 2 * tol * bn / lmin)
    assert np.allclose(out["residual"], res / bn, rtol=1e-6, atol=0)


def test_restatement_freezes_a_column_where_it_stops(ss_demo):
    """a column alone, inside a block of others, and at a permuted position: identical bits"""
    M = ss_demo["M"][:, :24].copy()
    M[:, 5] = 0.0
    M[:, 7] = 0.0
    M[3, 7] = 1.0  # a single non-zero genotype: it stops at another iteration than its neighbours
    tol = 1e-12
    block = R.pcg_batched(ss_demo["Ann"], ss_demo["Ang"], M, tol, 2000)
    assert len(set(block["col_iterations"].tolist())) >= 3
    perm = np.random.default_rng(4).permutation(M.shape[1])
    shuffled = R.pcg_batched(ss_demo["Ann"], ss_demo["Ang"], M[:, perm], tol, 2000)
    assert np.array_equal(shuffled["x"], block["x"][:, perm]) and np.array_equal(shuffled["col_iterations"], block["col_iterations"][perm])
    for c in (0, 5, 7, 23):
        alone = R.pcg_batched(ss_demo["Ann"], ss_demo["Ang"], M[:, c], tol, 2000)
        assert np.array_equal(alone["x"][:, 0], block["x"][:, c]), c
        assert alone["col_iterations"][0] == block["col_iterations"][c]


def test_restatement_errors(ss_demo):
    with pytest.raises(R.NotConverged, match="3 of 4 columns did not converge") as e:
        M = ss_demo["M"][:, :4].copy()
        M[:, 1] = 0.0
        R.pcg_batched(ss_demo["Ann"], ss_demo["Ang"], M, 1e-12, 5)
    assert e.value.live == 3
    with pytest.raises(R.NotPositiveDefinite):
        R.pcg_batched(sp.csc_matrix(np.array([[1.0, 2.0], [2.0, 1.0]])), sp.csr_matrix(np.eye(2)), np.array([[1.0], [-1.0]]), 1e-12, 10)


# ---- the planning header ----
_PLAN_PROGRAM = r"""
#include "hb_imputeplan.hpp"
#include <cstdio>
int main()
{
    const long long MiB = 1ll << 20, GiB = 1ll << 30;
    struct { int q; long long nnz; int ng; long long nnzg; int cols; long long free_b; } cases[] = {
        {900, 4500, 600, 1200, 131, 64 * GiB},        {900, 4500, 600, 1200, 1, 64 * GiB},           {19897, 132803, 95, 5000, 8, 64 * GiB},
        {20000, 133000, 2000, 9000, 512, 64 * GiB},   {20000, 133000, 2000, 9000, 512, 100 * MiB},   {100000, 668031, 476, 3000, 512, 64 * GiB},
        {1000000, 6900000, 4761, 30000, 512, 64 * GiB}, {1000000, 6900000, 4761, 30000, 512, 2 * GiB}, {5, 5, 2, 2, 3, 64 * GiB},
        {5, 5, 2, 2, 3, 1000},                        {0, 0, 2, 2, 3, 64 * GiB},
    };
    for (auto &c : cases) {
        const hb_impute_plan p = hb_impute_plan_of(c.q, c.nnz, c.ng, c.nnzg, c.cols, c.free_b);
        printf("%d %d %d %d %d %d | %s\n", p.ok, p.width, p.groups, p.parts, p.rows_per_part, p.cached, p.why.c_str());
    }
    for (int q : {1, 15, 16, 17, 900, 8192, 8193, 19897, 100000, 1000000, 2000000000}) {
        int parts, rows;
        hb_impute_partition(q, &parts, &rows);
        printf("part %d %d %d\n", q, parts, rows);
    }
}
"""


def test_plan_header_chooses_the_width_and_refuses_what_does_not_fit(tmp_path):
    """hb_imputeplan.hpp is plain C++: W is the widest block, no wider than the columns, whose 11 blocks of q x W doubles (p and one iteration's
    streamed traffic) fit the 256 MiB Infinity Cache, else 64; narrower until the solve's five blocks fit the free memory; refused where 64
    does not fit. The partition: at most 512 parts of a multiple of 16 rows, from q alone."""
    src, exe = tmp_path / "plan.cpp", tmp_path / "plan"
    src.write_text(_PLAN_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "hibayes_amd", "csrc"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    plans = [l.split(" | ") for l in lines if not l.startswith("part")]
    got = [tuple(int(v) for v in p[0].split()) for p in plans]
    # 900 x 192 x 88 bytes = 15 MB: the three groups the 131 columns need; one column: one group
    assert got[0] == (1, 192, 3, 57, 16, 1) and got[1] == (1, 64, 1, 57, 16, 1)
    assert got[2] == (1, 64, 1, 415, 48, 1)                       # 19 897 rows in 415 runs of 48
    assert got[3] == (1, 128, 2, 417, 48, 1)                      # 20 000 x W x 88 <= 2^28: W <= 152
    assert got[4] == (1, 64, 1, 417, 48, 1)                       # ... 5 x 20.5 MB do not fit 100 MiB, 5 x 10.2 MB do
    assert got[5] == (1, 64, 1, 481, 208, 0)                      # 10^5 x 64 x 88 = 563 MB: not cached, the narrowest block
    assert got[6] == (1, 64, 1, 509, 1968, 0)
    assert got[7][0] == 0 and "needs" in plans[7][1] and "MiB" in plans[7][1]   # 5 x 512 MB against 2 GiB
    assert got[8] == (1, 64, 1, 1, 16, 1)
    assert got[9][0] == 0 and got[10][0] == 0 and "empty" in plans[10][1]
    parts = {int(l.split()[1]): (int(l.split()[2]), int(l.split()[3])) for l in lines if l.startswith("part")}
    assert parts[1] == (1, 16) and parts[15] == (1, 16) and parts[16] == (1, 16) and parts[17] == (2, 16) and parts[900] == (57, 16)
    assert parts[8192] == (512, 16) and parts[8193] == (257, 32) and parts[19897] == (415, 48) and parts[2000000000][0] <= 512
    for q, (p, r) in parts.items():
        assert r % 16 == 0 and p * r >= q > (p - 1) * r and p <= 512


# ---- validation, without a device ----
def _tri(q=6):
    G = sp.csc_matrix(sp.diags([np.full(q - 1, -1.0), np.full(q, 2.5), np.full(q - 1, -1.0)], [-1, 0, 1]))
    G.sort_indices()
    return G


def _create(nn, ng):
    ImputeSystem(nn, ng).close()


def test_each_invalid_matrix_gets_its_text_before_any_device_call():
    G = _tri()
    ip, ix, dt = G.indptr.copy(), G.indices.copy(), G.data.copy()
    ng = sp.csr_matrix(np.arange(12.0).reshape(6, 2))

    def bad(nn, g, text):
        with pytest.raises(H.HibayesError, match=text) as e:
            _create(nn, g)
        assert e.value.status == 1, e.value

    d2 = dt.copy()
    d2[1] = -0.5  # (1, 0) without (0, 1)
    bad((ip, ix, d2, (6, 6)), ng, "must equal its transpose in value bits")
    U = sp.triu(G).tocsc()
    bad(U, ng, "must equal its transpose in pattern")
    i2 = ix.copy()
    i2[0], i2[1] = ix[1], ix[0]
    bad((ip, i2, dt, (6, 6)), ng, "A_nn: the indices of a row or column must be sorted and unique")
    i2 = ix.copy()
    i2[1] = i2[0]
    bad((ip, i2, dt, (6, 6)), ng, "sorted and unique")
    i2 = ix.copy()
    i2[-1] = 6
    bad((ip, i2, dt, (6, 6)), ng, "A_nn: an index is outside its range")
    d2 = dt.copy()
    d2[0] = 0.0
    bad((ip, ix, d2, (6, 6)), ng, "A_nn: the diagonal must be positive")
    Z = sp.csc_matrix(np.array([[1.0, 0.0], [0.0, 0.0]]))
    bad(Z, sp.csr_matrix(np.ones((2, 2))), "A_nn: the diagonal must be positive")
    d2 = dt.copy()
    d2[2] = np.nan
    bad((ip, ix, d2, (6, 6)), ng, "A_nn: a stored value is not finite")
    bad(G, sp.csr_matrix(np.ones((5, 2))), "A_ng must have as many rows as A_nn \\(5 against 6\\)")
    g = ng.copy()
    gi = g.indices.copy()
    gi[1] = 2
    bad(G, (g.indptr, gi, g.data, (6, 2)), "A_ng: an index is outside its range")
    bad(sp.csc_matrix(np.ones((2, 3))), ng, "A_nn must be square")
    # a valid system: only the device is missing
    if H.lib().hb_device_count() > 0:
        _create(G, ng)
        return
    with pytest.raises(H.HibayesError, match="no HIP device available") as e:
        _create(G, ng)
    assert e.value.status == 2


def test_solve_refuses_tol_and_max_iter_first():
    L = H.lib()
    buf = np.zeros(4)
    for tol, mi, text in ((0.0, 10, "tol must lie inside \\(0, 1\\)"), (1.0, 10, "tol must lie inside"), (-1e-3, 10, "tol must lie inside"),
                          (float("nan"), 10, "tol must lie inside"), (1e-12, 0, "max_iter must be at least 1"), (1e-12, 10, "null handle")):
        rc = L.hb_impute_solve(None, buf.ctypes.data, 2, 1, tol, mi, buf.ctypes.data, 2, None)
        assert rc == 1 and re.search(text, L.hb_last_error().decode()), (tol, mi, L.hb_last_error())
    L.hb_impute_destroy(None)


# ---- the library ----
def test_new_symbols_are_declared_exported_and_the_abi_is_still_6():
    lib = H.lib()
    hdr = open(os.path.join(ROOT, "include", "hibayes_gpu.h")).read()
    for s in NEW:
        assert s in _lib.SYMBOLS and hasattr(lib, s) and re.search(r"\b%s\s*\(" % s, hdr), s
    assert hdr.count("R/ssbayes.r:295-307") >= 3 and "typedef struct hb_impute_stats" in hdr
    assert lib.hb_abi_version() == 6
    assert "impute_device" in H.__all__ and callable(H.impute_device)


def test_stats_struct_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hibayes_gpu.h"\nint main(){printf("%zu %zu %zu %zu\\n",sizeof(hb_impute_stats),'
                   'offsetof(hb_impute_stats,max_residual),offsetof(hb_impute_stats,product_bytes),offsetof(hb_impute_stats,looks));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S = _lib.ImputeStats
    assert got == [C.sizeof(S), S.max_residual.offset, S.product_bytes.offset, S.looks.offset]


def test_impute_kernels_are_built_without_scratch():
    path = os.path.join(ROOT, "hibayes_amd", "csrc", "hb_impute.res.txt")
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
    for name in ("k_imp_transpose", "k_imp_init", "k_imp_start", "k_imp_product", "k_imp_step1", "k_imp_step2", "k_imp_resid", "k_imp_fin"):
        found = [k for k in rows if name in k]
        assert found, "kernel missing from the report: " + name
        for k in found:
            assert "ScratchSize" in rows[k] and "VGPRs Spill" in rows[k], (k, rows[k])
            assert rows[k]["ScratchSize"] == 0 and rows[k]["VGPRs Spill"] == 0, (k, rows[k])
            assert rows[k]["VGPRs"] <= 128, (k, rows[k])  # 1024 threads per workgroup: four waves on a SIMD


# ---- the Python surface ----
def test_python_surface(ss_demo):
    kw = dict(formula="T1 ~ 1", data=ss_demo["phe"], M=ss_demo["geno"][:, :8], M_id=ss_demo["M_id"], pedigree=ss_demo["ped"])
    with pytest.raises(ValueError, match="impute must be \"host\" or \"device\""):
        H.ssbrm_prepare(impute="bogus", **kw)
    with pytest.raises(ValueError, match="impute must be"):
        H.ssbrm(niter=30, nburn=10, impute="bogus", **kw)
    assert "impute_stats" not in ss_demo["pr"]  # the host route's dict is what it was
    with pytest.raises(H.HibayesError, match="M must have n_g"):
        ImputeSystem.solve(type("S", (), {"n_g": 3, "q": 2})(), np.zeros((2, 2)))
    if H.lib().hb_device_count() > 0:
        return
    with pytest.raises(H.HibayesError, match="no HIP device available") as e:
        H.ssbrm_prepare(impute="device", **kw)
    assert e.value.status == 2
    with pytest.raises(H.HibayesError, match="no HIP device available"):
        H.impute_device(ss_demo["Ann"], ss_demo["Ang"], ss_demo["M"][:, :3])
