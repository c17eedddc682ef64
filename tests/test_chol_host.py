"""What of the device Cholesky inverse (hibayes_amd/csrc/hb_chol.hip, hb_cholplan.hpp, hibayes_amd/chol.py) can be checked without a device: the plan,
the refusals, the resource report, solver_lu() and the Python surface."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hibayes_amd as H
from hibayes_amd import _lib
from hibayes_amd import chol as HC

import chol_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = 64
NEW = ("hb_chol_factor", "hb_chol_invert_factor", "hb_spd_inverse", "hb_chol_plan")
SIZES = (1, NB - 1, NB, NB + 1, 2 * NB + 1, 5 * NB + 7)


def check_plan(n, nb, ldw, by, steps):
    """steps: [(k0, width, row_tiles, tri_tiles)]"""
    assert nb == NB
    assert ldw % 2 == 0 and n <= ldw <= n + 1
    T = (n + NB - 1) // NB
    assert len(steps) == T
    assert [s[0] for s in steps] == [NB * t for t in range(T)]
    assert [s[1] for s in steps] == [min(NB, n - NB * t) for t in range(T)] and sum(s[1] for s in steps) == n
    assert [s[2] for s in steps] == [T - 1 - t for t in range(T)]
    # the diagonal tiles and the panels' row tiles are the tiles of the lower triangle, each once
    assert sum(1 + s[2] for s in steps) == T * (T + 1) // 2
    # each update covers the lower triangle of what is left: (T - 1 - t)(T - t) / 2 tiles; together the tetrahedral number
    assert [s[3] for s in steps] == [(T - 1 - t) * (T - t) // 2 for t in range(T)]
    assert sum(s[3] for s in steps) == (T - 1) * T * (T + 1) // 6
    info, panel, work = 16, 8 * ldw * 256, 8 * ldw * n  # (256: HB_CHOL_SB, the width of a block column of the factor's inverse)
    assert by == [info, info + panel, info + panel + work]


_PLAN_PROGRAM = r"""
#include "hb_cholplan.hpp"
#include <cstdio>
int main()
{
    for (int n : {%s}) {
        const hb_cholplan p = hb_cholplan_of(n);
        printf("%%d %%d %%lld %%zu %%zu %%zu %%d", p.n, p.nb, (long long)p.ldw, p.factor_bytes, p.invert_bytes, p.inverse_bytes, p.blocks);
        for (const hb_cholstep &s : p.steps) printf(" %%d,%%d,%%d,%%lld", s.k0, s.width, s.row_tiles, s.tri_tiles);
        printf("\n");
    }
    const hb_cholplan z = hb_cholplan_of(0);
    printf("%%d %%zu %%zu\n", z.n, z.inverse_bytes, z.steps.size());
}
"""


def test_plan_header_alone(tmp_path):
    """hb_cholplan.hpp is plain C++"""
    src, exe = tmp_path / "plan.cpp", tmp_path / "plan"
    src.write_text(_PLAN_PROGRAM % ", ".join(str(n) for n in SIZES + (20000,)))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "hibayes_amd", "csrc"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    for n, line in zip(SIZES + (20000,), lines):
        f = line.split()
        assert int(f[0]) == n and int(f[6]) == (n + NB - 1) // NB
        check_plan(n, int(f[1]), int(f[2]), [int(v) for v in f[3:6]], [tuple(int(v) for v in s.split(",")) for s in f[7:]])
    assert lines[-1].split() == ["0", "0", "0"]
    # the documented size: two n x n matrices are 6.4 GB at n = 20 000, of which the call allocates one, and a block column
    f = lines[len(SIZES)].split()
    assert int(f[5]) == 16 + 8 * 20000 * 256 + 8 * 20000 * 20000


@pytest.mark.parametrize("n", SIZES)
def test_plan_through_the_library(n):
    p = HC.chol_plan(n)
    check_plan(n, p["nb"], p["ldw"], [p["factor_bytes"], p["invert_bytes"], p["inverse_bytes"]], p["steps"])


def test_plan_refusals():
    L = H.lib()
    a = np.zeros(4, dtype=np.int64)
    args = [a.ctypes.data] * 8
    assert L.hb_chol_plan(0, 4, *args) == 1 and L.hb_last_error().decode() == "hb_chol_plan: n < 1"
    assert L.hb_chol_plan(5 * NB, 4, *args) == 1 and "shorter than the number of panels" in L.hb_last_error().decode()
    assert L.hb_chol_plan(5, 4, None, *args[1:]) == 1 and L.hb_last_error().decode() == "hb_chol_plan: null argument"


def test_invalid_arguments_are_refused_before_any_device_is_asked_for():
    L = H.lib()
    buf, info = np.zeros(16), C.c_int32(7)
    p = buf.ctypes.data  # (never dereferenced: every call below is refused first)
    for name, call in (("hb_chol_factor", lambda A, lda, n, lam, inf: L.hb_chol_factor(A, lda, n, 0, lam, inf)),
                       ("hb_spd_inverse", lambda A, lda, n, lam, inf: L.hb_spd_inverse(A, lda, n, 0, lam, inf))):
        for args, text in (((None, 4, 4, 0.0, C.byref(info)), "null argument"), ((p, 4, 4, 0.0, None), "null argument"),
                           ((p, 4, 0, 0.0, C.byref(info)), "n < 1"), ((p, 4, -3, 0.0, C.byref(info)), "n < 1"),
                           ((p, 3, 4, 0.0, C.byref(info)), "leading dimension smaller than n"),
                           ((p, 4, 4, float("nan"), C.byref(info)), "lambda must be finite"), ((p, 4, 4, float("inf"), C.byref(info)), "lambda must be finite")):
            assert call(*args) == 1, (name, args)
            assert L.hb_last_error().decode() == name + ": " + text
    for args, text in (((None, 4, 4, 0), "null argument"), ((p, 4, 0, 0), "n < 1"), ((p, 3, 4, 0), "leading dimension smaller than n")):
        assert L.hb_chol_invert_factor(*args) == 1
        assert L.hb_last_error().decode() == "hb_chol_invert_factor: " + text
    assert info.value == 7 and not buf.any()


def test_without_a_device_the_entries_say_so():
    L = H.lib()
    if L.hb_device_count() > 0:  # (valid arguments: only the device could have been missing)
        assert np.array_equal(H.spd_inverse(np.diag([1.0, 4.0, 0.25])), np.diag([1.0, 0.25, 4.0]))
        return
    buf, info = np.eye(4, order="F"), C.c_int32()
    for rc in (L.hb_spd_inverse(buf.ctypes.data, 4, 4, 0, 0.0, C.byref(info)), L.hb_chol_factor(buf.ctypes.data, 4, 4, 0, 0.0, C.byref(info)),
               L.hb_chol_invert_factor(buf.ctypes.data, 4, 4, 0)):
        assert rc == 2 and "no HIP device available" in L.hb_last_error().decode()
    with pytest.raises(H.HibayesError, match="no HIP device available") as e:
        H.spd_inverse(np.eye(3))
    assert e.value.status == 2


def test_new_symbols_are_declared_exported_and_the_abi_is_still_6():
    lib = H.lib()
    hdr = open(os.path.join(ROOT, "include", "hibayes_gpu.h")).read()
    for s in NEW:
        assert s in _lib.SYMBOLS and hasattr(lib, s) and re.search(r"\b%s\s*\(" % s, hdr), s
    assert "The inverse is not part of the library" not in hdr and "src/solver.cpp:159-202" in hdr
    assert lib.hb_abi_version() == 6
    for name in ("spd_inverse", "grm_inverse", "solver_lu", "chol_factor"):
        assert name in H.__all__ and callable(getattr(H, name)), name


def test_make_grm_names_grm_inverse():
    with pytest.raises(NotImplementedError, match=r"grm_inverse\(\)"):
        H.make_grm(np.zeros((5, 3), dtype=np.int8), inverse=True)


def test_chol_kernels_are_built_without_scratch():
    path = os.path.join(ROOT, "hibayes_amd", "csrc", "hb_chol.res.txt")
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
    for name in ("k_chol_shift", "k_chol_copy", "k_chol_diag", "k_chol_panel", "k_chol_trail", "k_chol_dinv", "k_chol_trmm", "k_chol_tscale", "k_chol_lauum"):
        found = [k for k in rows if name in k]
        assert found, "kernel missing from the report: " + name
        for k in found:
            assert "ScratchSize" in rows[k] and "VGPRs Spill" in rows[k], (k, rows[k])
            assert rows[k]["ScratchSize"] == 0 and rows[k]["VGPRs Spill"] == 0, (k, rows[k])
    assert all("k_chol_" in k for k in rows), sorted(rows)  # every kernel of the unit is named above
    assert len(rows) == 9, sorted(rows)


# ---- solver_lu(): src/solver.cpp:204-249 on the host ----
def test_solver_lu_inverts_a_nonsymmetric_matrix():
    rng = np.random.default_rng(5)
    A = rng.standard_normal((37, 37)) + 8.0 * np.eye(37)
    X = H.solver_lu(A)
    assert X.flags.f_contiguous and np.allclose(X, np.linalg.inv(A), rtol=1e-11, atol=1e-13)
    Xl = H.solver_lu(A, 0.5)
    assert np.allclose(Xl, np.linalg.inv(A + 0.5 * np.eye(37)), rtol=1e-11, atol=1e-13)
    assert np.allclose(A @ X, np.eye(37), atol=1e-12)   # (and A was not written to)


def test_solver_lu_raises_the_references_texts(demo):
    with pytest.raises(ValueError, match="^matrix is not invertible, try to specify parameter 'lambda' with a small value, eg: 0.001 or bigger$"):
        H.solver_lu(np.ones((4, 4)))
    G = R.grm_host(demo["plink"]["geno"])
    assert G.shape == (600, 600)
    with pytest.raises(ValueError, match=r"^system is computationally singular: reciprocal condition number = \d\.\d{6}e-\d\d,\n"
                                         r"try to specify parameter 'lambda' with a small value, eg: 0.001 or bigger$"):
        H.solver_lu(G, 0.0)
    with pytest.raises(ValueError, match="square"):
        H.solver_lu(np.ones((3, 4)))
    X = H.solver_lu(G, 0.01)
    assert np.allclose(X @ (G + 0.01 * np.eye(600)), np.eye(600), atol=1e-9)


def test_the_restatement_measures_lapack_as_the_issue_records_it():
    """LAPACK's own resR is 0.5-2.5 eps on the well-conditioned matrices and well under 1 eps on the graded ones: the floor n of the rule is what
    the device is held to there"""
    for n in (63, 129, 391):
        B = R.well_conditioned(n, n)
        X, info = R.lapack_inverse(B)
        assert info == 0 and np.array_equal(X, X.T) and 0.1 < R.res_right(B, X) < 5.0 and R.res_left(B, X) < 5.0
        L, info = R.lapack_factor(B)
        assert info == 0 and R.fac(B, L) < 3.0 and R.tri(L, R.lapack_invert_factor(L)) < 3.0
        Bg = R.graded(n, n)
        Xg, info = R.lapack_inverse(Bg)
        assert info == 0 and R.res_right(Bg, Xg) < 1.0
    E = np.eye(130)
    E[64, 64] = -1.0
    assert R.lapack_factor(E)[1] == 65 and R.lapack_inverse(E) == (None, 65)
