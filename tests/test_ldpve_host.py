"""What of the LD matrix's window PVE (hibayes_amd/csrc/hb_ldquad.hip, hb_ldqplan.hpp, hibayes_amd/pve.py: ld_window_pve, sbayes_vary) can be
checked without a device: the restatement against literal loops, the select rule, the plan header alone, the ABI, the resource report and the
argument checks of the Python surface."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import hibayes_amd as H
from hibayes_amd import _lib
from hibayes_amd import pve as HP

import ldpve_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hb_ldm_window_var", "hb_ldm_diagonal")


def literal(V, stored, A, w, nw):
    """the definitions as triple loops in longdouble, with the select rule"""
    m, Rn = A.shape
    var, tot = np.zeros((nw, Rn), dtype=np.longdouble), np.zeros(Rn, dtype=np.longdouble)
    for r in range(Rn):
        for j in range(m):
            if A[j, r] == 0.0:
                continue
            for i in range(m):
                if not stored[i, j] or A[i, r] == 0.0:
                    continue
                term = np.longdouble(A[j, r]) * (np.longdouble(V[i, j]) * np.longdouble(A[i, r]))
                tot[r] += term
                if w[i] == w[j]:
                    var[w[j] - 1, r] += term
    return var, tot


def symmetric(m, seed, density=1.0):
    rng = np.random.default_rng(seed)
    U_ = np.triu(rng.standard_normal((m, m)) * (rng.random((m, m)) < density))
    return U_ + np.triu(U_, 1).T


@pytest.mark.parametrize("m,Rn,density", [(1, 1, 1.0), (2, 3, 1.0), (7, 2, 0.5), (12, 9, 0.3), (12, 4, 1.0)])
def test_restatement_against_literal_loops(m, Rn, density):
    rng = np.random.default_rng(10 * m + Rn)
    V = symmetric(m, m + Rn, density)
    A = rng.standard_normal((m, Rn)) * (rng.random((m, Rn)) < 0.7)
    for w, nw in ((np.ones(m, dtype=int), 1), (np.arange(m) % 3 + 1, 4), (np.arange(1, m + 1), m)):
        # as a dense array every entry is stored; as CSC only the non-zero ones are — the absent ones would add 0.0, so the results agree
        for Vin, stored in ((V, np.ones((m, m), dtype=bool)), (sp.csc_matrix(V), V != 0.0)):
            var, tot = R.ld_window_var_ref(Vin, A, w, nw)
            lv, lt = literal(V, stored, A, w, nw)
            scale = np.abs(A).T @ np.abs(V) @ np.abs(A)
            assert var.shape == (nw, Rn) and tot.shape == (Rn,)
            assert np.all(np.abs(var - lv) <= 1e-17 * np.diag(scale)[None, :]) and np.all(np.abs(tot - lt) <= 1e-17 * np.diag(scale))
            bv, bt = R.ld_var_bound(Vin, A, w, nw)
            assert np.all(bv >= 0) and np.all(bt >= 0) and np.all(bv[np.abs(lv) > 0] > 0)
            assert np.all(bt <= R.gamma(2 * m + 2) * np.diag(scale) * (1 + 1e-12))


def test_an_indefinite_matrix_gives_a_negative_window_form():
    V = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 3.0]])   # eigenvalues 3, -1, 3
    A = np.array([[1.0], [-1.0], [0.5]])
    var, tot = R.ld_window_var_ref(V, A, np.array([1, 1, 2]), 2)
    assert var[0, 0] == -2.0 and var[1, 0] == 0.75 and tot[0] == -1.25
    lv, lt = literal(V, np.ones((3, 3), dtype=bool), A, np.array([1, 1, 2]), 2)
    assert np.array_equal(lv, var) and np.array_equal(lt, tot)


def test_a_nan_entry_counts_only_between_two_nonzero_effects():
    V = symmetric(6, 3)
    V[2, 2] = np.nan                  # a monomorphic marker's diagonal
    V[1, 4] = V[4, 1] = np.nan
    w = np.array([1, 1, 1, 2, 2, 2])
    A = np.ones((6, 3))
    A[2, 0] = A[4, 0] = 0.0           # record 0: neither NaN meets two effects
    A[2, 1] = 0.0                     # record 1: the off-diagonal one does, across the windows: only the total sees it
    for Vin in (V, sp.csc_matrix(V)):
        var, tot = R.ld_window_var_ref(Vin, A, w, 2)
        assert np.isfinite(var[:, 0]).all() and np.isfinite(tot[0])
        assert np.isfinite(var[:, 1]).all() and np.isnan(tot[1])
        assert np.isnan(var[0, 2]) and np.isfinite(var[1, 2]) and np.isnan(tot[2])
        lv, lt = literal(V, np.ones((6, 6), dtype=bool), A, w, 2)
        assert np.array_equal(np.isnan(lv), np.isnan(var)) and np.array_equal(np.isnan(lt), np.isnan(tot))
        assert np.allclose(lv[:, :2].astype(float), var[:, :2].astype(float), rtol=1e-15, atol=0)
        bv, bt = R.ld_var_bound(Vin, A, w, 2)
        assert np.isfinite(bv[:, :2]).all() and np.isfinite(bt[0]) and not np.isfinite(bt[1]) and not np.isfinite(bv[0, 2])


_PLAN_PROGRAM = r"""
#include "hb_ldqplan.hpp"
#include <cstdio>
int main()
{
    const int m = 7, nr = 2, nw = 4;
    const double A[2 * 7] = {0, 1, 0, 2, 3, 0, 0,  0, 0, 0, 0, 0, 0, 5};
    const uint32_t w[7] = {3, 2, 1, 2, 1, 1, 3};
    const hb_ldqplan p = hb_ldqplan_of(A, m, m, nr, w, nw);
    if (!p.error.empty()) return 1;
    for (int j : p.idx) printf("%d ", j);
    printf("|");
    for (const hb_ldqseg &s : p.segs) printf(" %d,%d,%d", s.window, s.first, s.count);
    printf(" |");
    for (int j = 0; j < m; j++) printf(" %u", p.win[j]);
    printf(" | %g %g %g %g\n", p.aw[8 * 1], p.aw[8 * 6], p.aw[8 * 6 + 1], p.aw[8 * 6 + 2]);
    double B[7] = {0, 1, 0, 1.0 / 0.0, 0, 0, 0};
    printf("%s\n", hb_ldq_check(B, m, m, 1, w, nw).c_str());
    const uint32_t w5[7] = {3, 2, 1, 5, 1, 1, 3};
    printf("%s\n", hb_ldq_check(A, m, m, 2, w5, nw).c_str());
    printf("%s\n", hb_ldq_check(A, m, m, 0, w, nw).c_str());
    printf("%s\n", hb_ldqplan_of(A, m, m, 9, w, nw).error.c_str());
    printf("%s\n", hb_ldqplan_of(A, m, m, 2, w5, nw).error.c_str());
}
"""


def test_plan_header_alone(tmp_path):
    """hb_ldqplan.hpp is plain C++: the list by window and marker, a segment per window with an entry, the effects row by row, the rows' ids"""
    src, exe = tmp_path / "plan.cpp", tmp_path / "plan"
    src.write_text(_PLAN_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "hibayes_amd", "csrc"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    # windows: 1 <- marker 4 (3.0), 2 <- markers 1 (1.0), 3 (2.0), 3 <- marker 6 (record 1: 5.0); window 4 has no marker, windows of rows without an effect read 0
    assert lines[0] == "4 1 3 6 | 0,0,1 1,1,2 2,3,1 | 0 2 0 2 1 0 3 | 1 0 5 0"
    assert lines[1] == "the effects must be finite (marker 4, record 1)"
    assert lines[2] == "windindx must hold window ids in 1 .. nw (marker 4 has 5)"
    assert lines[3] == "no record (R must be >= 1)"
    assert lines[4] == "a batch holds 1 .. 8 records"
    assert lines[5] == "windindx must hold window ids in 1 .. nw"     # (a batch alone: the id it could not index with, no more)


def test_new_symbols_are_declared_exported_and_the_abi_is_still_6():
    lib = H.lib()
    hdr = open(os.path.join(ROOT, "include", "hibayes_gpu.h")).read()
    for s in NEW:
        assert s in _lib.SYMBOLS and hasattr(lib, s) and re.search(r"\b%s\s*\(" % s, hdr), s
    assert lib.hb_abi_version() == 6 and "#define HB_ABI_VERSION 6" in hdr
    assert "R/sbayes.r:231-234" in hdr
    assert "ld_window_pve" in H.__all__ and callable(H.ld_window_pve) and callable(H.LDMatrix.window_var) and callable(H.LDMatrix.diagonal)


def test_ldquad_kernels_are_built_without_scratch():
    path = os.path.join(ROOT, "hibayes_amd", "csrc", "hb_ldquad.res.txt")
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
    for name in ("k_ldq_cols_denseE", "k_ldq_cols_cscE", "k_ldq_windowsE", "k_ldq_totalE", "k_ldq_diag_denseE", "k_ldq_diag_cscE"):
        found = [k for k in rows if name in k]
        assert len(found) == 1, "kernel missing from the report: " + name
        k = found[0]
        assert "ScratchSize" in rows[k] and "VGPRs Spill" in rows[k], (k, rows[k])
        assert rows[k]["ScratchSize"] == 0 and rows[k]["VGPRs Spill"] == 0, (k, rows[k])
    assert len(rows) == 6, sorted(rows)


def test_entries_refuse_a_null_handle_before_any_device_work():
    L = H.lib()
    buf = np.zeros(8)
    assert L.hb_ldm_window_var(None, buf.ctypes.data, 1, 1, 1, buf.ctypes.data, 1, buf.ctypes.data, 1, buf.ctypes.data) == 1
    assert L.hb_last_error().decode() == "hb_ldm_window_var: null handle"
    assert L.hb_ldm_diagonal(None, buf.ctypes.data) == 1
    assert L.hb_last_error().decode() == "hb_ldm_diagonal: null argument"


# ---- the Python surface ----
def test_ld_window_pve_argument_checks_need_no_device():
    V = np.eye(4)
    for ldm in (V, sp.identity(4, format="csc")):
        for kw, text in ((dict(alpha=np.ones(3)), r"alpha must be \(m,\) or \(m, R\)"), (dict(alpha=np.ones((4, 0))), "no record"),
                         (dict(alpha=[1, np.nan, 0, 0]), "alpha must be finite"), (dict(alpha=np.ones(4), windindx=[1, 2, 3]), "one integer window id per marker"),
                         (dict(alpha=np.ones(4), windindx=[1.0, 2.0, 1.0, 1.0]), "one integer window id per marker"),
                         (dict(alpha=np.ones(4), windindx=[1, 0, 1, 2]), r"window ids in 1 \.\. nw"), (dict(alpha=np.ones(4), vary=0.0), "vary must be a positive number"),
                         (dict(alpha=np.ones(4), threshold=-0.1), "threshold must be")):
            with pytest.raises(ValueError, match=text):
                H.ld_window_pve(ldm, **kw)
    for bad in (np.zeros((3, 4)), np.zeros(5), sp.csc_matrix(np.zeros((3, 4)))):
        with pytest.raises(ValueError, match="a scipy sparse matrix or a square array"):
            H.ld_window_pve(bad, np.ones(4))


def test_sbrm_pve_is_an_explicit_keyword():
    import inspect
    for f in (H.sbrm, H.ssbrm):
        p = inspect.signature(f).parameters["pve"]
        assert p.default is False
    assert "pve" not in inspect.signature(H.sbrm_cg).parameters


def test_vary_is_the_samplers_own():
    """hibayes_amd.pve.sbayes_vary against the literal loops of src/SBayesD.cpp:33-34, :93-115 on the demo's summary statistics. The m terms are
    non-negative and both sums are within gamma_m of the exact one, whatever their order: 2 gamma_m between them."""
    d = os.path.join(ROOT, "tests", "golden", "demo", "demo")
    Gm = H.read_plink(d)["geno"].astype(np.float64)
    diag = Gm.var(axis=0)
    rows = [l.split() for l in open(d + ".ma")][1:]
    f = lambda x: float(x) if x != "NA" else np.nan
    ss = np.array([[f(r[3]), f(r[4]), f(r[5]), f(r[7])] for r in rows])
    m = ss.shape[0]
    vary, n, count_y = R.sbayes_vary_loop(ss, diag)
    assert 0 < count_y < m and np.isnan(ss[:, 1:]).any() and n > 2 and vary > 0
    got = HP.sbayes_vary(ss, diag)
    assert abs(got - vary) <= 2 * R.gamma(m) * vary
    # one marker's NA moves the count and the value
    ss2 = ss.copy()
    k = int(np.flatnonzero(~np.isnan(ss[:, 1:]).any(axis=1))[0])
    ss2[k, 2] = np.nan
    v2, _, c2 = R.sbayes_vary_loop(ss2, diag)
    assert c2 == count_y - 1 and abs(HP.sbayes_vary(ss2, diag) - v2) <= 2 * R.gamma(m) * v2 and v2 != vary
    with pytest.raises(ValueError, match="four columns"):
        HP.sbayes_vary(ss[:, :3], diag)
    with pytest.raises(ValueError, match="one entry per marker"):
        HP.sbayes_vary(ss, diag[:-1])
    allna = ss.copy()
    allna[:, 2] = np.nan
    with pytest.raises(ValueError, match="Lack of SE"):
        HP.sbayes_vary(allna, diag)
