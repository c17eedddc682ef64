"""The device tridiagonal eigensolver's host side (hibayes_amd/csrc/hb_stedc.hip, hb_stedcplan.hpp, hibayes_amd/eig.py): the numpy restatement of
its algorithm against LAPACK's divide and conquer, the merge plan from the library itself, the additive C ABI, and the refusals that need no
device. Runs without a GPU.

The accuracy rule is tests/test_gpu_eig.py's: every measure of the restatement's pair is asserted against the same measure of LAPACK's dstedc on the
same (d, e): restatement <= 4 * LAPACK + n, in eps — the algorithm and its first-order bound are the same, only the leaf solver, the secular
iteration and the summation order differ; the floor n eps is there because the reference can be luckily small."""
import ctypes as C
import functools
import inspect
import os

import numpy as np
import pytest

import hibayes_amd as H
from hibayes_amd import _lib
from hibayes_amd import eig as HE

import stedc_restatement as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEDC_SYMBOLS = ["hb_eig_tridiagonal", "hb_eig_vectors_dev", "hb_stedc_plan", "hb_stedc_stats"]
NO_DEVICE = H.lib().hb_device_count() < 1
MARGIN = 4


@functools.lru_cache(maxsize=None)
def matrices():
    return S.matrices()


@pytest.mark.parametrize("name", S.MATRIX_NAMES)
def test_restatement_against_lapacks_divide_and_conquer(name):
    d, e = matrices()[name]
    n = len(d)
    stats = {}
    w, Z = S.stedc(d, e, stats)
    assert np.all(np.diff(w) >= 0) and Z.shape == (n, n) and stats.get("maxit", 0) < S.MAXIT
    mine, ref = S.measures(d, e, w, Z), S.measures(d, e, *S.lapack_dc(d, e))
    for k in mine:
        print("%-18s n=%-4d %-7s restatement %8.2f eps   LAPACK %8.2f eps   %s" % (name, n, k, mine[k], ref[k], stats))
    # LAPACK's own divide and conquer is a usable yardstick on every one of these matrices (dstemr is not: its orthogonality reaches 1 938 eps)
    assert all(np.isfinite(v) and v <= 64 for v in ref.values()), ref
    bad = {k: (mine[k], ref[k]) for k in mine if not mine[k] <= MARGIN * ref[k] + n}
    assert not bad, bad
    if name.startswith("toeplitz"):
        exact = S.toeplitz_values(n)
        assert np.max(np.abs(w - exact)) <= (MARGIN * np.max(np.abs(S.lapack_dc(d, e)[0] - exact)) + n * S.EPS * 4.0)


def test_restatement_exact_cases():
    d = np.random.default_rng(11).uniform(0.5, 2.0, 131)
    w, Z = S.stedc(d, np.zeros(130))
    assert np.array_equal(w, np.sort(d)) and np.array_equal(Z, np.eye(131)[:, np.argsort(d, kind="stable")])
    w, Z = S.stedc(np.zeros(40), np.zeros(39))
    assert np.all(w == 0) and np.array_equal(Z, np.eye(40))
    w, Z = S.stedc(np.full(70, 1.75), np.full(69, 1e-20))
    assert np.all(w == 1.75) and np.array_equal(Z, np.eye(70))


def test_restatement_forces_the_cases_it_is_meant_to():
    """no deflation on the Toeplitz matrix's first merge, rotations on Wilkinson's, nearly everything deflated in the cluster"""
    st = {}
    S.stedc(*S.toeplitz(33), st)
    assert st["deflated"] == 0 and st["rotations"] == 0
    st = {}
    S.stedc(*S.wilkinson(201), st)
    assert st["rotations"] > 0
    st = {}
    S.stedc(*matrices()["glued 10 x 1e-14"], st)
    assert st["rotations"] > 0 and st["deflated"] > 100
    st = {}
    S.stedc(*matrices()["clustered"], st)
    assert "deflated" not in st                           # the splits leave no part longer than a leaf: no merge at all
    st = {}
    S.stedc(*matrices()["clustered 1e-12"], st)
    assert st["deflated"] >= 100                          # here the merges run, and nearly every column deflates


SPLITS = {1: [], 2: [0], 31: [3, 4], 32: [15], 33: [0, 31], 65: [32], 97: [10, 50, 51], 513: [100, 101, 300]}


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 65, 97, 513])
@pytest.mark.parametrize("split", [False, True])
def test_plan_from_the_library(n, split):
    splits = SPLITS[n] if split and n > 1 else []
    p = HE.stedc_plan(n, splits)
    leaf = p["leaf_rows"]
    assert leaf == S.LEAF == 32
    rows = np.zeros(n, dtype=int)
    for lo, hi in p["leaves"]:
        assert 0 <= lo < hi <= n and hi - lo <= leaf
        rows[lo:hi] += 1
    assert np.all(rows == 1)                              # every row in exactly one leaf
    bounds = [0] + [s + 1 for s in splits] + [n]
    parts = list(zip(bounds[:-1], bounds[1:]))
    done = {(lo, hi): 0 for lo, hi in p["leaves"]}         # node -> level
    used = set()
    for lo, mid, hi, level in p["merges"]:
        assert lo < mid < hi and hi - lo > leaf
        assert (lo, mid) in done and (mid, hi) in done      # the children are adjacent, complete nodes, and come before their parent
        assert level == 1 + max(done[(lo, mid)], done[(mid, hi)])
        assert (lo, mid) not in used and (mid, hi) not in used
        used.update([(lo, mid), (mid, hi)])
        assert any(a <= lo and hi <= b for a, b in parts)  # never across a split
        done[(lo, hi)] = level
    for a, b in parts:                                     # every part ends as one node
        assert (a, b) in done and (a, b) not in used
    for level in range(1, p["levels"] + 1):
        cover = np.zeros(n, dtype=int)
        for lo, mid, hi, lv in p["merges"]:
            if lv == level:
                cover[lo:hi] += 1
        assert cover.max() == 1                            # the merges of a level are disjoint
    assert p["levels"] == max([lv for *_, lv in p["merges"]], default=0)
    # and it is the restatement's plan
    leaves, merges, levels = S.plan(n, splits)
    assert leaves == p["leaves"] and merges == p["merges"] and levels == p["levels"]


def test_plan_refusals():
    with pytest.raises(H.HibayesError, match="n < 1") as ex:
        HE.stedc_plan(0)
    assert ex.value.status == 1
    with pytest.raises(H.HibayesError, match="split points must be ascending") as ex:
        HE.stedc_plan(10, [5, 5])
    assert ex.value.status == 1
    with pytest.raises(H.HibayesError, match="split points must be ascending"):
        HE.stedc_plan(10, [9])


def test_new_symbols_are_declared_exported_and_the_abi_is_still_6():
    lib = H.lib()
    hdr = open(os.path.join(ROOT, "include", "hibayes_gpu.h")).read()
    for s in STEDC_SYMBOLS:
        assert s in _lib.SYMBOLS and hasattr(lib, s) and (s + "(") in hdr, s
    assert lib.hb_abi_version() == 6


def test_the_defaults_are_unchanged_and_the_keyword_is_checked():
    for f in (H.eigh, H.make_grm, H.ibrm, HE.eigh_device):
        assert inspect.signature(f).parameters["tridiagonal"].default == "host"
    M = np.zeros((4, 6), dtype=np.int8)
    with pytest.raises(ValueError, match="tridiagonal"):
        H.eigh(np.eye(3), tridiagonal="gpu")
    with pytest.raises(ValueError, match="tridiagonal"):
        H.make_grm(M, eigen=True, eigen_solver="device", tridiagonal="lapack", verbose=False)
    with pytest.raises(ValueError, match="tridiagonal"):
        H.make_grm(M, eigen=True, tridiagonal="device", verbose=False)                      # without eigen_solver="device"
    with pytest.raises(ValueError, match="tridiagonal"):
        H.ibrm("T1 ~ 1", data={"id": ["a"], "T1": [1.0]}, M=M[:1], M_id=["a"], method="BSLMM", eigen_solver="device", tridiagonal="dc")
    with pytest.raises(ValueError, match="tridiagonal"):
        H.ibrm("T1 ~ 1", data={"id": ["a"], "T1": [1.0]}, M=M[:1], M_id=["a"], method="BSLMM", tridiagonal="device")
    with pytest.raises(ValueError, match="n - 1"):
        HE.tridiagonal_eigh_device(np.ones(4), np.ones(4))


def test_arguments_are_refused_before_any_device_is_asked_for():
    lib = H.lib()
    d, e, w = np.ones(3), np.ones(2), np.zeros(3)
    Z, ldz = C.c_void_p(), C.c_int64()
    assert lib.hb_eig_tridiagonal(None, e.ctypes.data, 3, 0, w.ctypes.data, C.byref(Z), C.byref(ldz)) == 1
    assert "hb_eig_tridiagonal: null argument" in lib.hb_last_error().decode()
    assert lib.hb_eig_tridiagonal(d.ctypes.data, None, 3, 0, w.ctypes.data, C.byref(Z), C.byref(ldz)) == 1
    assert "null argument" in lib.hb_last_error().decode()
    assert lib.hb_eig_tridiagonal(d.ctypes.data, e.ctypes.data, 0, 0, w.ctypes.data, C.byref(Z), C.byref(ldz)) == 1
    assert "n < 1" in lib.hb_last_error().decode() and not Z.value
    for bad in (np.nan, np.inf):
        dd = d.copy()
        dd[1] = bad
        assert lib.hb_eig_tridiagonal(dd.ctypes.data, e.ctypes.data, 3, 0, w.ctypes.data, C.byref(Z), C.byref(ldz)) == 1
        assert "non-finite" in lib.hb_last_error().decode()
    ee = e.copy()
    ee[1] = np.nan
    assert lib.hb_eig_tridiagonal(d.ctypes.data, ee.ctypes.data, 3, 0, w.ctypes.data, C.byref(Z), C.byref(ldz)) == 1
    assert "non-finite" in lib.hb_last_error().decode()
    K, ldk = C.c_void_p(), C.c_int64()
    assert lib.hb_eig_vectors_dev(None, None, 64, C.byref(K), C.byref(ldk)) == 1 and "null handle" in lib.hb_last_error().decode()
    assert lib.hb_stedc_stats(None, 6) == 1


@pytest.mark.skipif(not NO_DEVICE, reason="a HIP device is visible: the no-device refusals cannot be seen here")
def test_without_a_device_the_compute_entries_say_so():
    d, e = S.random_pair(17)
    with pytest.raises(H.HibayesError, match="no HIP device available") as ex:
        HE.tridiagonal_eigh_device(d, e)
    assert ex.value.status == 2
    with pytest.raises(H.HibayesError, match="no HIP device available") as ex:
        HE.tridiagonal_eigh_device(np.ones(1), None)          # e may be absent for n = 1
    assert ex.value.status == 2
    with pytest.raises(H.HibayesError, match="no HIP device available") as ex:
        H.eigh(S.tri(d, e), tridiagonal="device")
    assert ex.value.status == 2
    with pytest.raises(H.HibayesError, match="no HIP device available") as ex:
        H.make_grm(np.ones((5, 7), dtype=np.int8), 0.01, eigen=True, eigen_solver="device", tridiagonal="device", verbose=False)
    assert ex.value.status == 2
