"""What of the window PVE (hibayes_amd/csrc/hb_pve.hip, hb_pveplan.hpp, hibayes_amd/pve.py) can be checked without a device: the plan against a
brute-force restatement, its refusals, the ABI, the resource report and the argument checks of the Python surface."""
import os
import re
import subprocess

import numpy as np
import pytest

import hibayes_amd as H
from hibayes_amd import _lib
from hibayes_amd import pve as HP

import pve_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hb_ctx_window_var", "hb_pve_plan")


def batch(seed, m, nr, nw, density, n=300, wmap="random"):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, nr)) * (rng.random((m, nr)) < density)
    if wmap == "random":
        w = rng.integers(1, nw + 1, m)
    elif wmap == "blocks":
        w = np.arange(m) * nw // m + 1
    else:
        w = np.arange(m) % nw + 1
    s1 = rng.integers(0, 2 * n, m).astype(np.float64)
    return A, w.astype(np.uint32), s1


def check_against_restatement(A, w, nw, s1, n, num_cus):
    p = HP.pve_plan(A, w, nw, s1, n, num_cus=num_cus)
    r = R.plan(A, w, nw, s1, n, num_cus)
    # the list: sorted by window id, within a window by marker index; the effects beside it, records past nr zero
    assert p["idx"] == r["idx"]
    assert np.array_equal(p["val"], r["val"])
    assert [(int(w[j]), j) for j in p["idx"]] == sorted((int(w[j]), j) for j in p["idx"])
    # the segments: one per window with an entry, in window order; a window without one does not appear
    assert p["segs"] == r["segs"]
    has = {int(w[j]) - 1 for j in range(len(w)) if np.any(A[j] != 0.0)}
    assert [s[0] for s in p["segs"]] == sorted(has)
    assert sum(s[2] for s in p["segs"]) == len(p["idx"]) and all(s[2] >= 1 for s in p["segs"])
    # the shifts
    for si, seg in enumerate(p["segs"]):
        bound = R.shift_bound(A, w, s1, n, seg, p["idx"])
        err = np.abs(p["shift"][si, :A.shape[1]].astype(np.longdouble) - r["shift"][si, :A.shape[1]])
        assert np.all(err <= bound), (si, err, bound)
        assert not p["shift"][si, A.shape[1]:].any()
    tb = R.shift_bound(A, w, s1, n, (0, 0, len(p["idx"])), p["idx"])
    assert np.all(np.abs(p["total_shift"][:A.shape[1]].astype(np.longdouble) - r["total_shift"][:A.shape[1]]) <= tb)
    # the grid: chunks of whole segments that cover every segment once, in order; row blocks from n alone
    assert p["row_blocks"] == r["row_blocks"] == (n + 1023) // 1024
    nseg = len(p["segs"])
    if nseg:
        assert p["chunks"][0][0] == 0 and all(c[1] >= 1 for c in p["chunks"])
        assert all(a[0] + a[1] == b[0] for a, b in zip(p["chunks"], p["chunks"][1:]))
        assert p["chunks"][-1][0] + p["chunks"][-1][1] == nseg
        want = -(-R.FILL * num_cus // p["row_blocks"])
        assert len(p["chunks"]) == min(nseg, want)
        if nseg >= num_cus:
            assert p["row_blocks"] * len(p["chunks"]) >= num_cus
    else:
        assert p["chunks"] == []
    return p


@pytest.mark.parametrize("m,nr,nw,density,wmap", [(1, 1, 1, 1.0, "random"), (9, 8, 3, 0.5, "interleaved"), (130, 8, 40, 0.1, "random"), (130, 3, 130, 1.0, "blocks"),
                                                  (700, 8, 50, 0.02, "blocks"), (700, 5, 700, 0.3, "interleaved"), (64, 2, 9, 0.0, "random")])
@pytest.mark.parametrize("n,num_cus", [(2, 256), (1025, 256), (50000, 256), (5000, 8)])
def test_plan_against_the_restatement(m, nr, nw, density, wmap, n, num_cus):
    A, w, s1 = batch(m * 31 + nr, m, nr, nw, density, n=n, wmap=wmap)
    check_against_restatement(A, w, nw, s1, n, num_cus)


def test_plan_skips_empty_windows_exactly_and_ignores_what_other_records_hold():
    A, w, s1 = batch(4, 60, 8, 12, 0.4, wmap="blocks")
    A[(w == 3) | (w == 7)] = 0.0
    A[w == 5, 1:] = 0.0       # window 5 has effects in record 0 only: still one segment, with the zeros of the other records in val
    p = check_against_restatement(A, w, 15, s1, 300, 256)   # (nw larger than the ids used)
    assert [s[0] for s in p["segs"]] == [k for k in range(12) if k not in (2, 6)]
    # a window's list entries and shift are the same whatever the other windows' effects are
    B = A.copy()
    B[w != 5] *= 3.0
    q = HP.pve_plan(B, w, 15, s1, 300)
    sa, sb = [s for s in p["segs"] if s[0] == 4][0], [s for s in q["segs"] if s[0] == 4][0]
    assert sa[2] == sb[2] and p["idx"][sa[1]:sa[1] + sa[2]] == q["idx"][sb[1]:sb[1] + sb[2]]
    assert np.array_equal(p["shift"][p["segs"].index(sa)], q["shift"][q["segs"].index(sb)])


def test_plan_chunks_are_balanced_by_entries():
    """one heavy window among many light ones: the heavy one gets a chunk to itself wherever the cut can give it one"""
    m = 2000
    w = np.concatenate([np.full(1000, 1), np.arange(1000) // 2 + 2]).astype(np.uint32)
    A = np.ones((m, 1))
    p = HP.pve_plan(A, w, int(w.max()), np.ones(m), 5000, num_cus=10)
    assert len(p["chunks"]) == 8 and p["chunks"][0] == (0, 1)
    per = [sum(p["segs"][s][2] for s in range(c[0], c[0] + c[1])) for c in p["chunks"]]
    assert per[0] == 1000 and max(per[1:]) - min(per[1:]) <= 4 and sum(per) == m


def test_plan_refusals():
    A, w, s1 = batch(2, 20, 2, 4, 0.5)

    def refused(**kw):
        a = dict(A=A, windindx=w, nw=4, s1=s1, n=300)
        a.update(kw)
        with pytest.raises(H.HibayesError) as e:
            HP.pve_plan(**a)
        assert e.value.status == 1 and str(e.value).startswith("hb_pve_plan: ")
        return str(e.value)

    assert "n >= 2" in refused(n=1)
    w0 = w.copy()
    w0[7] = 0
    assert "window ids in 1 .. nw (marker 8 has 0)" in refused(windindx=w0)
    w5 = w.copy()
    w5[3] = 5
    assert "window ids in 1 .. nw (marker 4 has 5)" in refused(windindx=w5)
    An = A.copy()
    An[11, 1] = np.nan
    assert "must be finite (marker 12, record 2)" in refused(A=An)
    An[11, 1] = np.inf
    assert "must be finite" in refused(A=An)
    assert "1 .. 8 records" in refused(A=np.ones((20, 9)))
    assert "ld must be" in refused(ld=299)
    assert H.lib().hb_pve_plan(*([None] * 1 + [20, 20, 2] + [None] * 1 + [4, None, 300, 512, 256] + [None] * 7)) == 1
    assert H.lib().hb_last_error().decode() == "hb_pve_plan: null argument"


_PLAN_PROGRAM = r"""
#include "hb_pveplan.hpp"
#include <cstdio>
int main()
{
    const int m = 7, nr = 2, nw = 3, n = 10;
    const double A[2 * 7] = {0, 1, 0, 2, 3, 0, 0,  0, 0, 0, 0, 0, 0, 5};
    const uint32_t w[7] = {3, 2, 1, 2, 1, 1, 3};
    const double s1[7] = {1, 2, 3, 4, 5, 6, 7};
    const hb_pveplan p = hb_pveplan_of(A, m, m, nr, w, nw, s1, n, 256, 4);
    if (!p.error.empty()) return 1;
    for (int j : p.idx) printf("%d ", j);
    printf("|");
    for (const hb_pveseg &s : p.segs) printf(" %d,%d,%d", s.window, s.first, s.count);
    printf(" | %g %g %g | %d %zu\n", p.shift[0], p.shift[8], p.shift[17], p.row_blocks, p.chunks.size());
    const hb_pveplan z = hb_pveplan_of(A, m, m, nr, w, nw, s1, 1, 256, 4);
    printf("%s\n", z.error.c_str());
}
"""


def test_plan_header_alone(tmp_path):
    """hb_pveplan.hpp is plain C++"""
    src, exe = tmp_path / "plan.cpp", tmp_path / "plan"
    src.write_text(_PLAN_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "hibayes_amd", "csrc"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    # windows: 1 <- markers 4 (3.0), 2 <- markers 1 (1.0), 3 (2.0), 3 <- marker 6 (record 1: 5.0)
    assert lines[0] == "4 1 3 6 | 0,0,1 1,1,2 2,3,1 | 1.5 1 3.5 | 1 3"
    assert lines[1] == "a variance needs n >= 2 individuals"


def test_new_symbols_are_declared_exported_and_the_abi_is_still_6():
    lib = H.lib()
    hdr = open(os.path.join(ROOT, "include", "hibayes_gpu.h")).read()
    for s in NEW:
        assert s in _lib.SYMBOLS and hasattr(lib, s) and re.search(r"\b%s\s*\(" % s, hdr), s
    assert lib.hb_abi_version() == 6 and "#define HB_ABI_VERSION 6" in hdr
    assert "R/bayes.r:303-308" in hdr
    assert "window_pve" in H.__all__ and callable(H.window_pve) and callable(H.Context.window_var)


def test_pve_kernels_are_built_without_scratch():
    path = os.path.join(ROOT, "hibayes_amd", "csrc", "hb_pve.res.txt")
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
    for name in ("k_window_varE", "k_window_var_realE", "k_window_var_finE"):
        found = [k for k in rows if name in k]
        assert len(found) == 1, "kernel missing from the report: " + name
        k = found[0]
        assert "ScratchSize" in rows[k] and "VGPRs Spill" in rows[k], (k, rows[k])
        assert rows[k]["ScratchSize"] == 0 and rows[k]["VGPRs Spill"] == 0, (k, rows[k])
    assert len(rows) == 3, sorted(rows)


def test_entry_refuses_bad_arguments_before_any_device_work():
    L = H.lib()
    buf = np.zeros(8)
    assert L.hb_ctx_window_var(None, buf.ctypes.data, 1, 1, buf.ctypes.data, 1, buf.ctypes.data, 1, buf.ctypes.data) == 1
    assert L.hb_last_error().decode() == "hb_ctx_window_var: null context"


# ---- the Python surface ----
def test_window_pve_argument_checks():
    M = np.zeros((5, 4), dtype=np.int8)
    for kw, text in ((dict(alpha=np.ones(3)), r"alpha must be \(m,\) or \(m, R\)"), (dict(alpha=np.ones((4, 2, 2))), "alpha must be"),
                     (dict(alpha=np.ones((4, 0))), "no record"), (dict(alpha=[1, np.nan, 0, 0]), "alpha must be finite"),
                     (dict(alpha=np.ones(4), windindx=[1, 2, 3]), "one integer window id per marker"),
                     (dict(alpha=np.ones(4), windindx=[1.0, 2.0, 1.0, 1.0]), "one integer window id per marker"),
                     (dict(alpha=np.ones(4), windindx=[1, 0, 1, 2]), r"window ids in 1 \.\. nw"),
                     (dict(alpha=np.ones(4), vary=0.0), "vary must be a positive number"), (dict(alpha=np.ones(4), vary=np.nan), "vary must be"),
                     (dict(alpha=np.ones(4), threshold=-0.1), "threshold must be")):
        with pytest.raises(ValueError, match=text):
            H.window_pve(M, **kw)
    with pytest.raises(ValueError, match="n x m matrix or a Context"):
        H.window_pve(np.zeros(5), np.ones(5))
    with pytest.raises(ValueError, match="n >= 2"):
        H.window_pve(np.zeros((1, 4), dtype=np.int8), np.ones(4))


def test_pve_summary_is_the_stated_host_arithmetic():
    var = np.array([[1.0, 0.0, 2.0], [3.0, 0.0, 0.5], [0.0, 0.0, 0.5], [0.0, 0.0, 1.0]])
    total = np.array([4.0, 0.0, 3.0])
    s = HP.pve_summary(var, total)
    assert np.array_equal(s["pve"], np.array([[0.25, 0.0, 2 / 3.0], [0.75, 0.0, 0.5 / 3.0], [0.0, 0.0, 0.5 / 3.0], [0.0, 0.0, 1 / 3.0]]))
    assert np.array_equal(s["mean"], s["pve"].mean(axis=1)) and s["threshold"] == 0.25
    assert np.array_equal(s["wppa"], np.array([1 / 3.0, 1 / 3.0, 0.0, 1 / 3.0]))   # strictly more than 1 / nw: 0.25 itself does not count
    t = HP.pve_summary(var, total, vary=8.0, threshold=0.5)
    assert np.array_equal(t["pve"], var / 8.0) and np.array_equal(t["wppa"], np.array([1 / 3.0, 1 / 3.0, 0.0, 0.0]))
    one = HP.pve_summary(var[:, :1], total[:1])
    assert "wppa" not in one and np.array_equal(one["mean"], one["pve"][:, 0])


def test_ibrm_pve_is_refused_in_a_sharded_run():
    class TwoRanks:
        world, rank = 2, 0

    with pytest.raises(ValueError, match=r"pve=True is not available in a sharded run"):
        H.ibrm("T1 ~ 1", data={"id": ["a"], "T1": [1.0]}, M=np.zeros((1, 2), dtype=np.int8), M_id=["a"], comm=TwoRanks(), pve=True)
